"""Row-pair layout of the march's planes (levels 2 and 3): padded texel (x, y) of a baked density plane or a gauge plane holds its own
channels, then those of (x, y + 1), so a bilinear cell is one contiguous run.  The arithmetic is untouched, so a handle in the row-pair form must give
the very bits of a handle in the one-row form (libngf_hip_exp.so keeps that one behind ngf_debug_set("pairpack", 0)); gauge planes that are three
squares of one size take the shared per-axis cell set-up, any other sizes the general one -- both are checked against the oracle.  The size
arithmetic of the handle is checked without a GPU against the layout written out in numpy."""
import functools

import numpy as np
import pytest
import torch

import ngf_amd  # noqa: F401
from ngf_amd import _lib, geometry, synth
from helpers import field_for_case, oracle_for_case

PLANE_HW = ((5, 7), (7, 5), (6, 6))          # (H, W) of plane_xy / plane_yz / plane_xz: small and not square, so an idx / stride / W-H mix-up shows
GAUGE_HW = {"equal": ((6, 6),) * 3, "unequal": ((5, 7), (7, 5), (6, 6))}
S, N_RAYS = 16, 96
RTOL, ATOL, ATOL_DEPTH = 1e-4, 1e-5, 5e-5    # tests/test_gpu_parity.py


# ---- CPU: the layout and the handle's size arithmetic ----------------------------------------------------------------------------------------------
def pack_rowpair(plane):
    """[nc, H, W] -> the row-pair image [(H + 2), (W + 2), 2, nc] as the pack kernels write it."""
    nc, H, W = plane.shape
    pad = np.zeros((H + 3, W + 2, nc), np.float32)          # one more zero row below: what the last padded row pairs with
    pad[1:H + 1, 1:W + 1] = plane.transpose(1, 2, 0)
    return np.stack([pad[:H + 2], pad[1:H + 3]], axis=2)


@pytest.mark.parametrize("nc", [1, 2])
def test_every_clamped_cell_reads_inside_the_allocation(nc):
    H, W = 5, 7
    floats = int(_lib.lib().ngf_debug_packed_plane_floats(H, W, nc, 1))
    assert floats == 2 * int(_lib.lib().ngf_debug_packed_plane_floats(H, W, nc, 0)) == (H + 2) * (W + 2) * 2 * nc
    plane = np.arange(1, nc * H * W + 1, dtype=np.float32).reshape(nc, H, W)
    img = pack_rowpair(plane)
    assert img.size == floats                             # the numpy layout has the rows the handle allocates
    flat = img.reshape(-1)
    pad = np.zeros((nc, H + 2, W + 2), np.float32)
    pad[:, 1:H + 1, 1:W + 1] = plane
    run = 4 * nc                                          # floats of a cell: 16 bytes (density), 32 bytes (gauge)
    for y0 in range(-1, H):                               # every (x0, y0) bil_setup's clamp can produce
        for x0 in range(-1, W):
            idx = (y0 + 1) * (W + 2) + (x0 + 1)           # Bil::idx: padded texel index
            lo = idx * 2 * nc
            assert 0 <= lo and lo + run <= floats, (x0, y0)
            assert (lo * 4) % (8 * nc) == 0                # 8-byte (density) / 16-byte (gauge) aligned
            cell = flat[lo:lo + run].reshape(2, 2, nc)    # [x tap][row][channel]
            for dx in (0, 1):
                for dy in (0, 1):
                    assert np.array_equal(cell[dx, dy], pad[:, y0 + 1 + dy, x0 + 1 + dx]), (x0, y0, dx, dy)


# ---- GPU: the two layouts give the same bits -------------------------------------------------------------------------------------------------------
def _case():
    # box of +-1: normalize_coord is then exact ((p + 1) * 1 - 1), so the lattice rays below sample lattice points exactly
    return {"model": np.array("triplane"), "aabb": np.array([[-1.0] * 3, [1.0] * 3], np.float32), "grid": np.array([9, 9, 9]),
            "near_far": np.array([1.0, 4.0], np.float32), "step_ratio": np.float32(0.5), "distance_scale": np.float32(25), "thr": np.float32(1e-4)}


@functools.lru_cache(maxsize=None)
def _params(gauge):
    p = synth.triplane_params(11, PLANE_HW, (6, 6), preset="R1", gauge_std=0.5)          # a gauge large enough to push density coordinates out of range
    for k, (name, hw) in enumerate(zip(("xy", "yz", "xz"), GAUGE_HW[gauge])):
        p[f"gauge_{name}"] = (synth.hash_normal(11, 60 + k, (1, 2, hw[0], hw[1])) * np.float32(0.5)).astype(np.float32)
    return p


@functools.lru_cache(maxsize=None)
def _rays():
    rays = []
    for y in (-1.0, -0.5, 0.0, 0.5, 1.0):                 # along +z through lattice points of plane_xy (W = 7: x = -1, 0, 1; H = 5: every y) -- x = 1 / y = 1 are the
        for x in (-1.0, -0.5, 0.0, 0.5, 1.0):             # cells x0 = W - 1 / y0 = H - 1; the step is 0.125, so z = -1, -0.5, 0 are hit exactly as well
            rays.append([x, y, -2.5, 0.0, 0.0, 1.0])
    for k in range(7):                                    # rays that miss the box
        rays.append([3.0 + k, 3.0, -2.5, 0.0, 0.0, 1.0])
    n = N_RAYS - len(rays)
    o = synth.hash_normal(5, 1, (n, 3)).astype(np.float32)
    o *= np.float32(2.5) / np.linalg.norm(o, axis=1, keepdims=True)
    tgt = (synth.hash_uniform(5, 2, (n, 3)) * np.float32(1.8) - np.float32(0.9)).astype(np.float32)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays += np.concatenate([o, d], axis=1).tolist()
    return np.asarray(rays, np.float32)


def _mask(on):
    if not on:
        return None
    dhw = (6, 5, 7)
    _, bits = synth.alpha_mask_bits(9, dhw, keep=0.8)
    return bits, dhw, np.array([[-1.0] * 3, [1.0] * 3], np.float32)


@functools.lru_cache(maxsize=None)
def _oracle(gauge, masked):
    g = _case()
    step = geometry.step_size(g["aabb"], g["grid"], float(g["step_ratio"]))
    return oracle_for_case(g, _params(gauge), step, _mask(masked)).render(_rays(), S, white_bg=True)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _render(params, masked, flags, pairpack):
    rays = torch.from_numpy(_rays()).cuda()
    with _lib.library("exp"), _lib.knobs(pairpack=pairpack):
        f = field_for_case(_case(), params, _mask(masked), **flags)
        with torch.no_grad():
            out = f(rays, N_samples=S, white_bg=True, iteration=30001)
        rgb, depth = out["rgb_map"].clone(), out["depth_map"].clone()
        torch.cuda.synchronize()
        f.release()
    return rgb, depth


def test_the_rays_reach_the_border_cells():
    """What the cases below rely on, recomputed on the CPU: density coordinates (position + gauge offsets) in the cells x0 = -1, x0 = W - 1, y0 = -1,
    y0 = H - 1 and beyond, and samples exactly on lattice points."""
    import torch.nn.functional as F
    rays = _rays()
    z = 1.0 + 0.125 * np.arange(S, dtype=np.float32)
    p = rays[:, None, :3] + rays[:, None, 3:] * z[None, :, None]
    inside = np.all(np.abs(p) <= 1.0, axis=2)
    assert inside.any(axis=1).sum() >= 60 and (~inside.any(axis=1)).sum() >= 7          # most rays cross the box, some miss it
    x = p[inside]
    assert (np.abs(x * 2 - np.round(x * 2)).max(axis=1) == 0).sum() >= 20                 # samples on lattice points of the 5-texel axes
    par = _params("unequal")
    uv = {"xy": (0, 1), "yz": (1, 2), "xz": (0, 2)}
    off = {}
    for name, (a, b) in uv.items():
        grid = torch.from_numpy(np.stack([x[:, a], x[:, b]], axis=1)).view(1, -1, 1, 2)
        off[name] = F.grid_sample(torch.from_numpy(par[f"gauge_{name}"]), grid, mode="bilinear", padding_mode="zeros", align_corners=True).view(2, -1).numpy()
    t = {"xy": (x[:, 0] + off["xy"][0] + off["xz"][0], x[:, 1] + off["xy"][1] + off["yz"][0])}          # compute_gauge's sums for plane_xy (Field.py:53-75)
    H, W = PLANE_HW[0]
    x0 = np.floor((t["xy"][0] + 1) / 2 * (W - 1)).astype(int)
    y0 = np.floor((t["xy"][1] + 1) / 2 * (H - 1)).astype(int)
    for want in (-1, W - 1):
        assert (x0 == want).any(), want
    for want in (-1, H - 1):
        assert (y0 == want).any(), want
    assert (x0 < -1).any() and (x0 > W - 1).any() and (y0 < -1).any() and (y0 > H - 1).any()          # and out of range altogether


LEVELS = {"level2": dict(bake=True), "level3": dict(bake=True, bake_color=True), "level3_bf16": dict(bake=True, bake_color=True, split_bf16=True)}


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("level", list(LEVELS))
def test_rowpair_layout_gives_the_bits_of_the_one_row_layout(level, masked):
    for gauge in ("equal", "unequal"):                     # shared per-axis cell set-up / every plane's cell on its own
        old = _render(_params(gauge), masked, LEVELS[level], 0)
        new = _render(_params(gauge), masked, LEVELS[level], 1)
        assert torch.equal(_bits(new[0]), _bits(old[0])) and torch.equal(_bits(new[1]), _bits(old[1])), gauge
        assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1]), gauge
        o_rgb, o_depth = _oracle(gauge, masked)
        for tag, (rgb, depth) in (("one-row", old), ("row-pair", new)):
            rgb, depth = rgb.cpu().numpy(), depth.cpu().numpy()
            err = np.abs(rgb - o_rgb)
            print(f"{level} mask={masked} gauge={gauge} {tag}: max|rgb - oracle| = {err.max():.3e}, max|depth - oracle| = {np.abs(depth - o_depth).max():.3e}")
            assert not (err > ATOL + RTOL * np.abs(o_rgb)).any(), (gauge, tag, float(err.max()))
            assert not (np.abs(depth - o_depth) > ATOL_DEPTH + RTOL * np.abs(o_depth)).any(), (gauge, tag)


@pytest.mark.gpu
@pytest.mark.parametrize("level", list(LEVELS))
def test_non_finite_gauge_output_gives_the_old_layouts_bits(level):
    """A diverged gauge: one texel is inf, so the rays through its cells get non-finite density coordinates (bil_setup's comment: the cell is clamped,
    every weight is zeroed).  sigma (ngf_field_march) and the pixels must be the one-row layout's bits."""
    for gauge in ("equal", "unequal"):
        par = {k: v.copy() for k, v in _params(gauge).items()}
        par["gauge_xy"][0, 0, 2, 3] = np.inf
        par["gauge_yz"][0, 1, 1, 1] = -np.inf
        old = _render(par, False, LEVELS[level], 0)
        new = _render(par, False, LEVELS[level], 1)
        assert torch.equal(_bits(new[0]), _bits(old[0])) and torch.equal(_bits(new[1]), _bits(old[1])), gauge
        sig = []
        rays = torch.from_numpy(_rays()).cuda()
        for pp in (0, 1):
            with _lib.library("exp"), _lib.knobs(pairpack=pp):
                f = field_for_case(_case(), par, None, **LEVELS[level])
                s, w = f.march(rays, S, mode=1)
                torch.cuda.synchronize()
                f.release()
            sig.append((s, w))
        assert torch.equal(_bits(sig[0][0]), _bits(sig[1][0])) and torch.equal(_bits(sig[0][1]), _bits(sig[1][1])), gauge
