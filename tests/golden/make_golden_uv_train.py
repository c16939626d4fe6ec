#!/usr/bin/env python3
"""Capture the UV-Mapping training golden vectors FROM THE REFERENCE ITSELF (run in the build container only).

    python tests/golden/make_golden_uv_train.py     # writes tests/golden/uv_train_{square,sphere}.npz

The reference's own sub-modules (GeometryMlpDecoder, GaugeTransform, TextureMlpDecoder, InverseNetwork, cube_ray_generation, ray_march,
simple_tone_map), composed as NeuTex.forward does (model.py:27-59; the module itself is CUDA-hardwired), on CPU in fp64 and in fp32, with the
jitter and the template points pinned; the reference's own Model.compute_loss (model.py:300-349) with weights 1/1/1/0 and 1/1/1/1.  The inverse mapping runs the
reference's InverseNetwork on the flattened uv (``InverseGauge.map``'s ``uv.view(input_shape, -1, D)`` raises in torch).  Stored: outputs,
losses, each parameter's gradient norm, 128 seeded entries and its products with seeded probe matrices (uv_train_eager.probes); per-tensor arrays are concatenated in the order of `names`.  Parameters come from tests/uv_train_eager.model_params (sums stored)."""
import contextlib
import importlib
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF  # noqa: E402
import uv_train_eager as E  # noqa: E402


def _reference(prim):
    for k in [k for k in sys.modules if k in ("model", "util") or k.startswith("model.")]:
        del sys.modules[k]
    sys.path.insert(0, os.path.join(REF, "UV-Mapping"))
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            mods = {n: importlib.import_module("model." + n) for n in ("decoder", "gauge_fields", "renderer", "model")}
    finally:
        sys.path.pop(0)
    return mods


def run(mods, params, prim, b, bg, dtype, weights):
    dec, gf, rn, mm = mods["decoder"], mods["gauge_fields"], mods["renderer"], mods["model"]
    with contextlib.redirect_stdout(io.StringIO()):
        geo = dec.GeometryMlpDecoder(pos_freqs=10, hidden_size=256, num_layers=10)
        gauge = gf.GaugeTransform(prim)
        tex = dec.TextureMlpDecoder(3, 10, 6, uv_dim=2 if prim == "square" else 3, layers=[5, 3], width=256, clamp=False, primitive_type=prim,
                                    target_texture="None")
        inv = gf.InverseNetwork(2 if prim == "square" else 3)
    parts = {"net_geometry_decoder.": geo, "gauge_transform.": gauge, "net_texture.": tex, "inverse_gauge.inverse_network.": inv}
    for pre, m in parts.items():
        m.load_state_dict({k[len(pre):]: torch.from_numpy(v.copy()) for k, v in params.items() if k.startswith(pre)})
        m.to(dtype)
    named = {pre + k: p for pre, m in parts.items() for k, p in m.named_parameters()}
    assert set(named) == set(params)
    t = lambda k: torch.from_numpy(b[k]).to(dtype)          # noqa: E731
    cam, rd, U, tp = t("campos"), t("raydir"), t("U"), t("template")
    bgt = None if bg is None else torch.from_numpy(np.array([bg], np.float32)).to(dtype)
    real_rand = torch.rand
    torch.rand = lambda *a, **k: U.clone()
    try:
        ray_pos, ray_dist, ray_valid, _ = rn.cube_ray_generation(cam, rd, U.shape[-1], jitter=0.05)
    finally:
        torch.rand = real_rand
    density = geo(ray_pos)["density"][..., None]
    pts3 = inv(tp.unsqueeze(0)).unsqueeze(1)
    o = {"points": pts3.view(pts3.shape[0], -1, pts3.shape[-1]).permute(0, 2, 1)}
    uv = gauge(ray_pos)
    feats = tex(uv, rd[:, :, None, :])
    bsdf = torch.cat([density, feats[..., :3]], -1)
    m = rn.ray_march(rd, ray_pos, ray_dist, ray_valid, bsdf, None, None, rn.radiance_render, rn.alpha_blend)
    ray_color, blend_weight, bgw = m[0], m[4], m[6]
    if bgt is not None:
        ray_color = ray_color + bgt[:, None, :] * bgw[:, :, None]
    o["color"] = rn.simple_tone_map(ray_color)
    o["transmittance"] = bgw
    o["points_original"] = ray_pos
    o["points_inverse"] = inv(uv.reshape(-1, uv.shape[-1])).view(uv.shape[:-1] + (3,))
    o["points_inverse_weights"] = blend_weight
    # the reference's own loss: Model.compute_loss on a stand-in `self` (model.py:300-349)
    me = types.SimpleNamespace(output=o, input={"gt_image": t("gt_image"), "transmittance": t("gt_trans")},
                               opt=types.SimpleNamespace(loss_color_weight=weights[0], loss_bg_weight=weights[1], loss_origin_weight=weights[2],
                                                         loss_inverse_mapping_weight=weights[3]))
    mm.Model.compute_loss(me)
    me.loss_total.backward()
    return o, me.loss_total, named


def capture(name, seed, prim, bg):
    mods = _reference(prim)
    params = E.model_params(seed, prim)
    b = E.batch(seed, prim)
    out = {}
    rng = np.random.default_rng(seed)
    names = sorted(params)
    idx = {k: np.sort(rng.choice(params[k].size, size=min(128, params[k].size), replace=False)) for k in names}
    for dt, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        for tag, w in (("l0", (1.0, 1.0, 1.0, 0.0)), ("l1", (1.0, 1.0, 1.0, 1.0))):
            o, loss, named = run(mods, params, prim, b, bg, dtype, w)
            out[f"{dt}.{tag}.loss"] = np.float64(loss.item())
            if tag == "l0":
                out[f"{dt}.color"] = o["color"].detach().numpy().copy()
                out[f"{dt}.transmittance"] = o["transmittance"].detach().numpy().copy()
            gs = {k: p.grad.double().numpy() for k, p in named.items()}
            out[f"{dt}.{tag}.gnorm"] = np.array([np.linalg.norm(gs[k]) for k in names])
            out[f"{dt}.{tag}.gval"] = np.concatenate([gs[k].reshape(-1)[idx[k]] for k in names]).astype(np.float64 if dt == "f64" else np.float32)
            out[f"{dt}.{tag}.probe"] = np.stack([E.probe_products(k, gs[k]) for k in names])
    sums = np.array([np.asarray(params[k], np.float64).sum() for k in names])
    np.savez_compressed(os.path.join(HERE, name + ".npz"), primitive_type=prim, seed=seed, S=b["U"].shape[-1], campos=b["campos"], raydir=b["raydir"],
                        U=b["U"], template=b["template"], gt_image=b["gt_image"], gt_trans=b["gt_trans"],
                        bg=np.zeros((0,), np.float32) if bg is None else np.array([bg], np.float32),
                        names=np.array(names), idx=np.concatenate([idx[k] for k in names]).astype(np.int32),
                        idx_len=np.array([len(idx[k]) for k in names]), sums=sums, **out)
    print(f"{name}: loss fp64 {out['f64.l0.loss']:.9f} / {out['f64.l1.loss']:.9f}, fp32 {out['f32.l0.loss']:.6f} / {out['f32.l1.loss']:.6f}")


if __name__ == "__main__":
    capture("uv_train_square", 71, "square", None)
    capture("uv_train_sphere", 72, "sphere", (0.2, 0.5, 0.8))
