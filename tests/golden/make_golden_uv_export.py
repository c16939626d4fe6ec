#!/usr/bin/env python3
"""Capture the UV-Mapping texture-export golden vectors FROM THE REFERENCE ITSELF (run in the build container only).

    python tests/golden/make_golden_uv_export.py     # writes tests/golden/uv_export.npz

The reference's own TextureMlpDecoder (decoder.py:11-179) with the synth.uvmapping_params weights of uv_edit.npz (seed 61): its
export_textures / _export_sphere for the cases of tests/uv_export_eager.CASES, once as it computes them (fp32) and once from a .double() copy of
the same module on the same fp32 points (an edit texture is looked up in float32 in both); the points it evaluated (recorded at its forward); util.merge_cube_to_single_texture of the R = 32
cube; and the residue of sampling its own exports back at their cell centres (util.sample_cubemap / sample_square), the yardstick of the
export -> set_target_texture(mode 4) round trip."""
import contextlib
import copy
import importlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF  # noqa: E402
import ngf_amd  # noqa: E402,F401
from ngf_amd import synth  # noqa: E402
import uv_export_eager as E  # noqa: E402


def _reference():
    for k in [k for k in sys.modules if k in ("model", "util") or k.startswith("model.")]:
        del sys.modules[k]
    sys.path.insert(0, os.path.join(REF, "UV-Mapping"))
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            return importlib.import_module("model.decoder"), importlib.import_module("util")
    finally:
        sys.path.pop(0)


def decoder(dec, prim):
    with contextlib.redirect_stdout(io.StringIO()):
        tex = dec.TextureMlpDecoder(3, 10, 6, uv_dim=2 if prim == "square" else 3, layers=[5, 3], width=256, clamp=False, primitive_type=prim,
                                    target_texture="None")
    params = synth.uvmapping_params(E.SEED, prim)
    tex.load_state_dict({k[len("net_texture."):]: torch.from_numpy(v.copy()) for k, v in params.items() if k.startswith("net_texture.")})
    return tex.eval()


def run64(tex64, util, kind, pts, viewdir):
    """The exporters' bodies (decoder.py:123-170) on given fp32 points, through the .double() module."""
    p = pts.double()

    def one(x):
        if viewdir is None:
            return torch.sigmoid(tex64.color1(tex64.block1(torch.cat([x, util.positional_encoding(x, tex64.num_freqs)], dim=-1))))
        return tex64.forward(x, torch.tensor(viewdir).float().double().expand(x.shape[:-1] + (3,)))

    with torch.no_grad():
        if kind == "cube":
            return torch.stack([one(p[i]) for i in range(6)], dim=0)
        return one(p).flip(0) if kind == "equi" else one(p)


def main():
    dec, util = _reference()
    edit = np.load(os.path.join(HERE, "uv_edit.npz"))
    out, seen = {}, {}
    for key, prim, kind, R, viewdir, with_edit in E.CASES:
        tex = decoder(dec, prim)
        if with_edit:
            tex.cubemap_, tex.cubemap_mode_ = torch.from_numpy(E.edit_texture(edit, prim).copy()), 1
        rec = []
        real_forward = tex.forward
        tex.forward = lambda uv, view: (rec.append(uv.clone()), real_forward(uv, view))[1]
        out[key + ".f32"] = E.export(tex, kind, R, viewdir).numpy().copy()
        tex.forward = real_forward
        if viewdir is not None:
            seen[(prim, kind, R)] = torch.stack(rec, 0) if kind == "cube" else rec[0]
        pts = seen[(prim, kind, R)]          # (a diffuse case follows the view case of its point set)
        tex64 = copy.deepcopy(tex).double()
        # (the edit texture is looked up in float32 also here: util.sample_cubemap collects its samples in a float32 buffer and cannot run in
        # another dtype; the points are float32 values, so the look-up is the fp32 run's, bit for bit, and the MLPs around it run in float64)
        lookups = {n: getattr(dec, n) for n in ("sample_cubemap", "sample_square")}
        for n, f in lookups.items():
            setattr(dec, n, lambda t, uv, f=f: f(t.float(), uv.float()))
        try:
            out[key + ".f64"] = run64(tex64, util, kind, pts, viewdir).numpy().copy()
        finally:
            for n, f in lookups.items():
                setattr(dec, n, f)
        assert out[key + ".f64"].dtype == np.float64 and out[key + ".f32"].dtype == np.float32
        print(f"{key}: {out[key + '.f32'].shape} range {out[key + '.f32'].min():.3g} .. {out[key + '.f32'].max():.3g}, "
              f"zeros {float((out[key + '.f32'] == 0).mean()):.3f}, max|f32 - f64| {np.abs(out[key + '.f32'] - out[key + '.f64']).max():.3g}")
    for (prim, kind, R), pts in seen.items():
        out[E.points_key(prim, kind, R)] = pts.numpy().copy()
    cube = torch.from_numpy(out["sphere.cube32.view.f32"])
    for rotate in (1, 0):
        out[f"merge.rotate{rotate}"] = util.merge_cube_to_single_texture(cube, rotate=bool(rotate)).numpy().copy()
    # the reference's own round-trip residue: its export (clamped to [0,1]) as the edit texture, sampled at the export's own points
    c = cube.clamp(0, 1)
    out["rt.sphere.residue"] = np.float64((util.sample_cubemap(c, seen[("sphere", "cube", 32)]) - c).abs().max().item())
    a = torch.from_numpy(out["square.sq32.view.f32"]).clamp(0, 1)
    out["rt.square.residue"] = np.float64((util.sample_square(a.transpose(0, 1).contiguous(), seen[("square", "sq", 32)]) - a).abs().max().item())
    print("round-trip residues:", out["rt.sphere.residue"], out["rt.square.residue"])
    path = os.path.join(HERE, "uv_export.npz")
    np.savez_compressed(path, seed=E.SEED, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
