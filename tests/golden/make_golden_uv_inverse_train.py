#!/usr/bin/env python3
"""Capture the inverse-gauge TRAINING golden vectors from the reference itself (run in the build container only).

    python tests/golden/make_golden_uv_inverse_train.py     # writes tests/golden/uv_inverse_train.npz

The reference's own InverseNetwork (gauge_fields.py:78-120) with the synth.inverse_gauge_params weights, one seed per primitive, on the 161
points of tests/uv_inverse_eager.py under the loss sum_p w_p |xyz_p - t_p|^2 of tests/uv_inverse_train_eager.py (hash targets and weights; the
weight of a point within MARGIN of a ReLU kink in the fp64 restatement is zero, the kept-point rule).  torch.autograd gives the gradients, once
as the reference computes them (fp32) and once from a .double() copy on the same points: d_uv, every bias, linear1 and last_linear whole, rows
ROWS of linear2 and of each 512 x 512 gradient."""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_uv_inverse import _reference, module  # noqa: E402
import uv_inverse_eager as V  # noqa: E402
import uv_inverse_train_eager as T  # noqa: E402

SEED = {"sphere": 71, "square": 72}
WHOLE = ("linear1.weight", "last_linear.weight")


def grads(net, uv, t, w):
    uv = uv.clone().requires_grad_(True)
    names = [n for n, _ in net.named_parameters()]
    g = torch.autograd.grad(T.loss(net(uv), t, w), [uv] + [p for _, p in net.named_parameters()])
    return g[0], dict(zip(names, g[1:]))


def main():
    gf = _reference()
    out = {"rows": np.asarray(T.ROWS), "margin": np.asarray(T.MARGIN)}
    for prim in V.PRIMS:
        seed = SEED[prim]
        uv = torch.from_numpy(V.points(prim))
        t, w = (torch.from_numpy(a) for a in T.targets(seed, V.N_POINTS))
        keep = T.kept(V.weights(seed, prim, torch.float64), uv.double())
        w = w * keep
        key = f"{prim}.s{seed}"
        out[key + ".keep"], out[key + ".t"], out[key + ".w"] = keep.numpy(), t.numpy(), w.numpy()
        net = module(gf, seed, prim)
        for tag, m, cast in (("f32", net, lambda a: a), ("f64", copy.deepcopy(net).double(), lambda a: a.double())):
            d_uv, g = grads(m, cast(uv), cast(t), cast(w))
            assert sorted(g) == sorted(T.NAMES)
            out[f"{key}.d_uv.{tag}"] = d_uv.numpy().copy()
            for name, v in g.items():
                v = v.numpy()
                out[f"{key}.{name}.{tag}"] = (v if name.endswith(".bias") or name in WHOLE else v[list(T.ROWS)]).copy()
        print(f"{prim} seed {seed}: dropped {int((~keep).sum())} of {V.N_POINTS}; |d_uv| {float(np.abs(out[key + '.d_uv.f64']).max()):.3g}")
        assert int((~keep).sum()) <= T.CAP * V.N_POINTS
    path = os.path.join(HERE, "uv_inverse_train.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    main()
