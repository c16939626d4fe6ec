#!/usr/bin/env python3
"""Capture the UV-Mapping point-query golden vectors FROM THE REFERENCE ITSELF (run in the build container only).

    python tests/golden/make_golden_uv_query.py     # writes tests/golden/uv_query.npz

The reference's own GeometryMlpDecoder (decoder.py:201-237), GaugeTransform (gauge_fields.py:49-74) and TextureMlpDecoder (decoder.py:11-78)
with the synth.uvmapping_params weights of uv_edit.npz (seed 61), both primitives, on the 161 points and per-point view directions of
tests/uv_query_eager.py: density, uv and colour (at the reference's own uv) once as it computes them (fp32) and once from .double() copies of the
same modules on the same fp32 points (the colour then at the fp64 uv)."""
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
import uv_query_eager as Q  # noqa: E402


def _reference():
    for k in [k for k in sys.modules if k in ("model", "util") or k.startswith("model.")]:
        del sys.modules[k]
    sys.path.insert(0, os.path.join(REF, "UV-Mapping"))
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            return importlib.import_module("model.decoder"), importlib.import_module("model.gauge_fields")
    finally:
        sys.path.pop(0)


def modules(dec, gf, prim):
    params = synth.uvmapping_params(Q.SEED, prim)

    def load(mod, prefix):
        mod.load_state_dict({k[len(prefix):]: torch.from_numpy(v.copy()) for k, v in params.items() if k.startswith(prefix)})
        return mod.eval()

    with contextlib.redirect_stdout(io.StringIO()):
        geo = dec.GeometryMlpDecoder(10, 256, 10)
        gauge = gf.GaugeTransform(prim)
        tex = dec.TextureMlpDecoder(3, 10, 6, uv_dim=2 if prim == "square" else 3, layers=[5, 3], width=256, clamp=False, primitive_type=prim,
                                    target_texture="None")
    return load(geo, "net_geometry_decoder."), load(gauge, "gauge_transform."), load(tex, "net_texture.")


def run(mods, pts, view):
    geo, gauge, tex = mods
    with torch.no_grad():
        p = pts[None, None]                                   # (N, Rays, Samples, 3)
        sigma = geo(p)["density"][0, 0]
        uv = gauge(p)
        rgb = tex(uv, view[None, None])[0, 0]
    return sigma.numpy().copy(), uv[0, 0].numpy().copy(), rgb.numpy().copy()


def main():
    dec, gf = _reference()
    xyz, view = Q.points(), Q.views()
    out = {"xyz": xyz, "view": view}
    for prim in Q.PRIMS:
        mods = modules(dec, gf, prim)
        f32 = run(mods, torch.from_numpy(xyz), torch.from_numpy(view))
        f64 = run(tuple(copy.deepcopy(m).double() for m in mods), torch.from_numpy(xyz).double(), torch.from_numpy(view).double())
        for name, a, b in zip(("sigma", "uv", "rgb"), f32, f64):
            assert a.dtype == np.float32 and b.dtype == np.float64 and a.shape == b.shape
            out[f"{prim}.{name}.f32"], out[f"{prim}.{name}.f64"] = a, b
            print(f"{prim}.{name}: {a.shape} range {a.min():.3g} .. {a.max():.3g}, max|f32 - f64| {np.abs(a - b).max():.3g}")
    path = os.path.join(HERE, "uv_query.npz")
    np.savez_compressed(path, seed=Q.SEED, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
