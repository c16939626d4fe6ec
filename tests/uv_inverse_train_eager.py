"""Torch restatement of the inverse network's training step on given weights (tests/uv_inverse_eager.py carries the network): the loss
``sum_p w_p |xyz_p - t_p|^2``, its gradients in any dtype on any device, and the kept-point rule the gradient tests share.

ReLU makes the gradient discontinuous where a pre-activation crosses zero, and a kernel and fp64 need not agree on the sign of one that lies
within rounding of it.  So a point is DROPPED -- its weight w_p is set to zero for every side of a comparison -- when any of its 1600 hidden
pre-activations in the fp64 restatement lies within ``MARGIN`` of zero; a test asserts that it drops at most ``CAP`` of its points."""
import numpy as np
import torch
import torch.nn.functional as F

from ngf_amd import synth
import uv_inverse_eager as V

MARGIN = 4e-6          # 13 x the largest |hip - fp64| measured for the forward's outputs (3e-7)
CAP = 0.10             # share of a test's points that may be dropped
ROWS = (0, 170, 341, 511)      # the rows of linear2's and the 512 x 512 gradients the fixture keeps
NAMES = tuple(f"{n}.{k}" for n in V.LAYERS for k in ("weight", "bias"))


def hash_points(seed, prim, n):
    """[n, D] float32: synth.hash_uniform(seed, 960, (n, D)) * 2 - 1, normalised for the sphere."""
    D = V.DIMS[prim]
    x = (synth.hash_uniform(seed, 960, (n, D)) * np.float32(2) - np.float32(1)).astype(np.float32)
    if prim == "sphere":
        x = (x.astype(np.float64) / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    return x


def targets(seed, n):
    """(t [n, 3] in [-1, 1), w [n] in [0.5, 1.5)): hash targets and weights of the loss."""
    t = (synth.hash_uniform(seed, 961, (n, 3)) * np.float32(2) - np.float32(1)).astype(np.float32)
    w = (synth.hash_uniform(seed, 962, (n,)) + np.float32(0.5)).astype(np.float32)
    return t, w


def pre_activations(wb, x):
    """The four hidden layers' pre-activations [n, 64], [n, 512] x 3."""
    out = []
    for w, b in wb[:-1]:
        z = F.linear(x, w, b)
        out.append(z)
        x = F.relu(z)
    return out


def kept(wb64, x64, margin=MARGIN):
    """bool [n]: no hidden pre-activation of the point lies within ``margin`` of zero (fp64 weights and points)."""
    with torch.no_grad():
        near = [(z.abs() <= margin).any(dim=1) for z in pre_activations(wb64, x64)]
    return ~torch.stack(near).any(dim=0)


def loss(xyz, t, w):
    return (w * ((xyz - t) ** 2).sum(-1)).sum()


def d_xyz(xyz, t, w):
    """d loss / d xyz in closed form: 2 w (xyz - t)."""
    return 2 * w.unsqueeze(-1) * (xyz - t)


def gradients(wb, x, t, w):
    """-> (xyz, d_uv [n, D], [the ten gradients in NAMES order]) of ``loss`` by torch autograd in the dtype / on the device of the arguments."""
    leaves = [p.detach().clone().requires_grad_(True) for pair in wb for p in pair]
    x = x.detach().clone().requires_grad_(True)
    xyz = V.forward(list(zip(leaves[0::2], leaves[1::2])), x)
    g = torch.autograd.grad(loss(xyz, t, w), [x] + leaves)
    return xyz.detach(), g[0], list(g[1:])


def rel_err(g, g64):
    """|g - g64| / |g64| over a whole tensor (Frobenius), in fp64."""
    g, g64 = g.double(), g64.double()
    return float((g - g64).norm() / g64.norm())


WHOLE = ("linear1.weight", "last_linear.weight")


def fixture_rows(name, g):
    """What the fixture keeps of gradient ``name``: biases, linear1 and last_linear whole, rows ROWS of the others."""
    return g if name.endswith(".bias") or name in WHOLE else g[list(ROWS)]


def chunk(n):
    """Rows per split-K chunk of a weight gradient (csrc/ngf_uv_inverse_train.hpp: uvit_chunk): 1024 up to 65 536 points, then n / 64 rounded up
    to 16."""
    return max(1024, (-(-n // 64) + 15) // 16 * 16)
