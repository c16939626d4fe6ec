#!/usr/bin/env python3
"""Capture the inverse-gauge golden vectors FROM THE REFERENCE ITSELF (run in the build container only).

    python tests/golden/make_golden_uv_inverse.py     # writes tests/golden/uv_inverse.npz

The reference's own InverseNetwork (gauge_fields.py:78-120) with the synth.inverse_gauge_params weights of two seeds, both primitives, on the
161 points of tests/uv_inverse_eager.py: xyz once as the reference computes it (fp32) and once from a .double() copy of the same module on the
same fp32 points.  Checked here, on the CPU, and stored: every hidden layer's share of active ReLU units lies in [0.2, 0.8] and max|xyz| in
[0.1, 10] -- the fixture is neither dead nor saturating.  (synth.inverse_gauge_params' gains were chosen so that both hold.)"""
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
import uv_inverse_eager as V  # noqa: E402


def _reference():
    for k in [k for k in sys.modules if k in ("model", "util") or k.startswith("model.")]:
        del sys.modules[k]
    sys.path.insert(0, os.path.join(REF, "UV-Mapping"))
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            return importlib.import_module("model.gauge_fields")
    finally:
        sys.path.pop(0)


def module(gf, seed, prim):
    params = synth.inverse_gauge_params(seed, prim)
    with contextlib.redirect_stdout(io.StringIO()):
        net = gf.InverseNetwork(V.DIMS[prim])
    net.load_state_dict({k[len(V.PREFIX):]: torch.from_numpy(v.copy()) for k, v in params.items()})
    return net.eval()


def main():
    gf = _reference()
    out = {"seeds": np.asarray(V.SEEDS)}
    for prim in V.PRIMS:
        uv = V.points(prim)
        out[f"{prim}.uv"] = uv
        for seed in V.SEEDS:
            net = module(gf, seed, prim)
            with torch.no_grad():
                f32 = net(torch.from_numpy(uv)).numpy().copy()
                f64 = copy.deepcopy(net).double()(torch.from_numpy(uv).double()).numpy().copy()
                shares = []
                V.forward(V.weights(seed, prim, torch.float64), torch.from_numpy(uv).double(), shares)
            assert f32.dtype == np.float32 and f64.dtype == np.float64 and f32.shape == f64.shape == (V.N_POINTS, 3)
            top = float(np.abs(f64).max())
            print(f"{prim} seed {seed}: active shares {[round(s, 3) for s in shares]}, max|xyz| {top:.3g}, max|f32 - f64| {np.abs(f32 - f64).max():.3g}")
            assert len(shares) == 4 and all(0.2 <= s <= 0.8 for s in shares), shares
            assert 0.1 <= top <= 10, top
            key = f"{prim}.s{seed}"
            out[key + ".xyz.f32"], out[key + ".xyz.f64"] = f32, f64
            out[key + ".active"], out[key + ".max_abs"] = np.asarray(shares), np.asarray(top)
    path = os.path.join(HERE, "uv_inverse.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
