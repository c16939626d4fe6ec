"""The sixteen-wave level-3 render kernel: four waves per SIMD instead of three, the pass in 128 registers because the
colour gather runs in quarter-plane stages.  Per channel the quarter-plane pass does the half-plane pass's four FMAs in its order (tap 0, 1, 2, 3
onto the running sum, planes in order), so the two kernels must give the same bits: every case renders one handle of libngf_hip_exp.so under
ngf_debug_set("waves", 12) and ("waves", 16) and compares rgb_map and depth_map bit for bit -- with and without an alpha mask (the MaskSkip
instantiations), with three equal square gauge planes and with unequal ones (GaugeAny), with and without jitter, on a launch whose tile plan has
all four tile widths and on one below one tile per wave.  One case is checked against the oracle at the tolerances of tests/test_pairpack.py.
ngf_debug_get("last_waves") says which kernel a launch took, so a silent fall-back to twelve waves fails the test.  The product library picks the
kernel by launch size (level3_waves16 in csrc/ngf_field.hip: sixteen waves from 312 rays per CU on): the last test renders on both sides of that
threshold without a knob."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ngf_amd  # noqa: F401
from ngf_amd import _lib, geometry, synth
from helpers import field_for_case, oracle_for_case

PLANE_HW = ((32, 32),) * 3
GAUGE_HW = {"equal": ((32, 32),) * 3, "unequal": ((24, 32), (32, 24), (32, 32))}
S = 64
LEVEL3 = dict(bake=True, bake_color=True)
RTOL, ATOL, ATOL_DEPTH = 1e-4, 1e-5, 5e-5    # tests/test_pairpack.py
# (rays, knob grid): 5000 rays on 8 workgroups are more than eight rays per resident wave of either kernel (8 x 16 and 8 x 12 waves) -> tiles of
# 8, 4, 2 and 1 rays; 300 rays on the whole device are fewer than its waves -> one-ray tiles, most waves idle
LAUNCHES = {"four_widths": (5000, 8), "below_one_tile_per_wave": (300, -1)}


def _plan(n, resident):
    rays, shift = (C.c_int64 * 4)(), (C.c_int32 * 4)()
    nseg = _lib.lib().ngf_debug_tile_plan(n, 8, resident, -1, rays, shift)
    return [(int(rays[k]), int(shift[k])) for k in range(nseg)]


def test_the_launch_shapes_are_what_the_cases_say():
    """Host arithmetic, no GPU: the tile plans of the two launch shapes for sixteen and for twelve resident waves per workgroup."""
    n, grid = LAUNCHES["four_widths"]
    for waves in (12, 16):
        plan = _plan(n, grid * waves)
        assert [s for _, s in plan] == [3, 2, 1, 0], (waves, plan)
        assert sum(r for r, _ in plan) == n
        assert [r for r, _ in plan[1:]] == [grid * waves * 4, grid * waves * 2, grid * waves], (waves, plan)      # one narrow tile per resident wave and width
    n, _ = LAUNCHES["below_one_tile_per_wave"]
    for waves in (12, 16):
        assert _plan(n, 256 * waves) == [(n, 0)], waves


def _case():
    # step = 2 / 32 * 1.0: 64 steps cover 4 units, every chord of the +-1 box
    return {"model": np.array("triplane"), "aabb": np.array([[-1.0] * 3, [1.0] * 3], np.float32), "grid": np.array([33, 33, 33]),
            "near_far": np.array([1.0, 6.0], np.float32), "step_ratio": np.float32(1.0), "distance_scale": np.float32(25), "thr": np.float32(1e-4)}


@functools.lru_cache(maxsize=None)
def _params(gauge):
    p = synth.triplane_params(17, PLANE_HW, (32, 32), preset="R1", gauge_std=0.05)
    for k, (name, hw) in enumerate(zip(("xy", "yz", "xz"), GAUGE_HW[gauge])):
        p[f"gauge_{name}"] = (synth.hash_normal(17, 60 + k, (1, 2, hw[0], hw[1])) * np.float32(0.05)).astype(np.float32)
    return p


@functools.lru_cache(maxsize=None)
def _rays(n):
    miss = n // 16                                       # rays that miss the box: tiles with nothing to march
    m = n - miss
    o = synth.hash_normal(7, 1, (m, 3)).astype(np.float32)
    o *= np.float32(2.5) / np.linalg.norm(o, axis=1, keepdims=True)
    tgt = (synth.hash_uniform(7, 2, (m, 3)) * np.float32(1.8) - np.float32(0.9)).astype(np.float32)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    hit = np.concatenate([o, d], axis=1)
    out = np.tile(np.array([[3.0, 3.0, -2.5, 0.0, 0.0, 1.0]], np.float32), (miss, 1))
    out[:, 0] += np.arange(miss, dtype=np.float32)
    rays = np.concatenate([hit[:m // 2], out, hit[m // 2:]], axis=0)
    return np.ascontiguousarray(rays, np.float32)


@functools.lru_cache(maxsize=None)
def _jitter(n):
    return synth.hash_uniform(7, 3, (n,)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _mask(on):
    """Occupancy inside a ball of radius 0.6 only: the march meets open space (blocks of 8 and of 4 empty cells) in front of and behind it."""
    if not on:
        return None
    dhw = (40, 36, 44)
    vol, _ = synth.alpha_mask_bits(9, dhw, keep=0.8)
    zz, yy, xx = np.meshgrid(*[np.linspace(-1.0, 1.0, k) for k in dhw], indexing="ij")
    vol = np.logical_and(vol, zz * zz + yy * yy + xx * xx < 0.36)
    return np.packbits(vol.reshape(-1)), dhw, np.array([[-1.0] * 3, [1.0] * 3], np.float32)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _render_both(gauge, masked, launch, jitter):
    """{12: (rgb, depth), 16: (rgb, depth)} of ONE handle of the experiment library."""
    n, grid = LAUNCHES[launch]
    rays = torch.from_numpy(_rays(n)).cuda()
    kw = dict(is_train=True, jitter=torch.from_numpy(_jitter(n)).cuda(), coin=0.7) if jitter else {}
    out = {}
    with _lib.library("exp") as L:
        f = field_for_case(_case(), _params(gauge), _mask(masked), **LEVEL3)
        for waves in (12, 16):
            with _lib.knobs(waves=waves, grid=grid), torch.no_grad():
                o = f(rays, N_samples=S, white_bg=True, iteration=30001, **kw)
                assert L.ngf_debug_get(b"last_waves") == waves          # the kernel that was asked for ran
            out[waves] = (o["rgb_map"].clone(), o["depth_map"].clone())
        torch.cuda.synchronize()
        f.release()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("jitter", [False, True], ids=["nojitter", "jitter"])
@pytest.mark.parametrize("gauge", ["equal", "unequal"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("launch", list(LAUNCHES))
def test_sixteen_waves_give_the_bits_of_twelve(launch, masked, gauge, jitter):
    out = _render_both(gauge, masked, launch, jitter)
    rgb12, depth12 = out[12]
    rgb16, depth16 = out[16]
    assert torch.isfinite(rgb12).all() and torch.isfinite(depth12).all()
    lit = int((rgb12 < 1.0).any(dim=1).sum())
    print(f"{launch} mask={masked} gauge={gauge} jitter={jitter}: {lit} of {rgb12.shape[0]} rays are not background")
    assert lit >= rgb12.shape[0] // 4                       # the colour path ran: a frame of background pixels would compare equal whatever the pass does
    assert torch.equal(_bits(rgb16), _bits(rgb12)) and torch.equal(_bits(depth16), _bits(depth12))


@pytest.mark.gpu
def test_sixteen_waves_against_the_oracle():
    launch = "below_one_tile_per_wave"
    n, _ = LAUNCHES[launch]
    g = _case()
    step = geometry.step_size(g["aabb"], g["grid"], float(g["step_ratio"]))
    o_rgb, o_depth = oracle_for_case(g, _params("equal"), step, None).render(_rays(n), S, white_bg=True)
    rgb, depth = (t.cpu().numpy() for t in _render_both("equal", False, launch, False)[16])
    err, derr = np.abs(rgb - o_rgb), np.abs(depth - o_depth)
    print(f"sixteen waves: max|rgb - oracle| = {err.max():.3e}, max|depth - oracle| = {derr.max():.3e}")
    assert not (err > ATOL + RTOL * np.abs(o_rgb)).any(), float(err.max())
    assert not (derr > ATOL_DEPTH + RTOL * np.abs(o_depth)).any(), float(derr.max())


@pytest.mark.gpu
def test_the_product_library_picks_the_kernel_by_launch_size():
    """No knob: twelve waves below 312 rays per CU, sixteen from there on -- and the same pixels as the other kernel on both sides."""
    L = _lib.lib()
    edge = 312 * torch.cuda.get_device_properties(0).multi_processor_count
    f = field_for_case(_case(), _params("equal"), None, **LEVEL3)
    for n, want in ((edge - 1, 12), (edge, 16)):
        rays = torch.from_numpy(np.resize(_rays(5000), (n, 6))).cuda()
        with torch.no_grad():
            own = f(rays, N_samples=16, white_bg=True, iteration=30001)
            assert L.ngf_debug_get(b"last_waves") == want, n
            with _lib.knobs(waves=28 - want):
                other = f(rays, N_samples=16, white_bg=True, iteration=30001)
                assert L.ngf_debug_get(b"last_waves") == 28 - want, n
        assert torch.equal(_bits(own["rgb_map"]), _bits(other["rgb_map"])) and torch.equal(_bits(own["depth_map"]), _bits(other["depth_map"])), n
    torch.cuda.synchronize()
    f.release()
