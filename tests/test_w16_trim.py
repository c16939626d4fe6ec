"""The sixteen-wave level-3 kernel's owner collect without v_cmpx (TriPlanePolicy::COLLECT3): a ray's three colour sums live
in its seg-0, 1, 2 lanes, an entry's EXEC mask is made on the scalar unit and the entry is one v_add_f32.  Per channel the adds and their order are
those of the twelve-wave kernel's collect, so the two kernels must give the same bits.  Geometry, rays, masks and launch shapes are those of
tests/test_waves16.py (32 x 32 planes, S = 64; 5 000 rays on 8 workgroups = tiles of 8, 4, 2 and 1 rays; 300 rays on the whole device = one-ray
tiles in which one ray owns all sixteen entries of a pass, and partial last passes); every case renders ONE handle of libngf_hip_exp.so under
ngf_debug_set("waves", 12) and ("waves", 16), compares rgb_map and depth_map as int32 and asserts ngf_debug_get("last_waves").

The cases beyond tests/test_waves16.py:
  - out-of-range cells: gauge planes drawn with gauge_std = 0.5 shift the plane coordinates far enough that 33.6 % (equal gauge planes) / 36.3 %
    (unequal) of the 5 000-ray launch's in-box samples, 34.1 % / 37.4 % of the 300-ray launch's, have at least one density / colour cell outside its
    plane (computed on the CPU with the oracle's gauge formula and asserted to lie in 10 % .. 90 %; 0.5 is the first value tried, 0.05 gives 0.6 %);
  - non-finite gauge: a 3 x 3 patch of +inf and one NaN texel in one gauge plane -- the same bits, NaN where the twelve-wave kernel has NaN;
  - widths the tile plan never makes: tile_w = 64 (the unsplit kernel: one lane per ray, the v_cmpx collect, at sixteen waves) and tile_w = 16 (split
    tiles for which the three-lane collect has no lane pattern: the launch keeps the twelve-wave kernel, level3_waves16 in csrc/ngf_field.hip -- what
    that case checks is the `last_waves == 12` assertion; its bit comparison is twelve waves against twelve waves and cannot fail).  So no knob-forced
    width runs the three-lane collect: it exists for the plan's widths only, which the other cases cover;
  - the out-of-range case against the oracle at the tolerances of tests/test_pairpack.py;
  - the product library above its sixteen-wave threshold, no knob, against the experiment library's twelve-wave render."""
import functools

import numpy as np
import pytest
import torch

import ngf_amd  # noqa: F401
from ngf_amd import _lib, geometry, synth
from helpers import field_for_case, oracle_for_case
from oracle.eager import EagerField
import test_waves16 as w16

S = w16.S
GAUGE_STD_OUT = 0.5


@functools.lru_cache(maxsize=None)
def _params(gauge, std=GAUGE_STD_OUT, nonfinite=False):
    p = dict(synth.triplane_params(17, w16.PLANE_HW, (32, 32), preset="R1", gauge_std=0.05))
    for k, (name, hw) in enumerate(zip(("xy", "yz", "xz"), w16.GAUGE_HW[gauge])):
        p[f"gauge_{name}"] = (synth.hash_normal(17, 60 + k, (1, 2, hw[0], hw[1])) * np.float32(std)).astype(np.float32)
    if nonfinite:
        g = p["gauge_xy"].copy()
        g[0, 0, 10:13, 14:17] = np.inf
        g[0, 1, 20, 7] = np.nan
        p["gauge_xy"] = g
    return p


@functools.lru_cache(maxsize=None)
def _out_of_range_share(gauge, n):
    """Share of the launch's in-box samples (no jitter) with at least one density / colour cell out of range: cell index floor(pixel coordinate)
    outside [-1, size - 1] on either axis, i.e. none of its four taps inside the plane -- with the gauge formula of oracle/eager.py."""
    g, p = w16._case(), _params(gauge)
    E = EagerField(p, g["aabb"], geometry.step_size(g["aabb"], g["grid"], float(g["step_ratio"])), near_far=g["near_far"])
    r = torch.from_numpy(w16._rays(n))
    o, d = r[:, :3], r[:, 3:6]
    vec = torch.where(d == 0, torch.full_like(d, 1e-6), d)
    tmin = torch.minimum((E.aabb[1] - o) / vec, (E.aabb[0] - o) / vec).amax(-1).clamp(min=E.near, max=E.far)
    z = tmin[:, None] + E.step * torch.arange(S)[None].float()
    pts = o[:, None, :] + d[:, None, :] * z[..., None]
    valid = ~((E.aabb[0] > pts) | (pts > E.aabb[1])).any(-1)
    c = E._coords(((pts - E.aabb[0]) * E.inv - 1)[valid], True)
    out = torch.zeros(int(valid.sum()), dtype=torch.bool)
    for name, uv in zip(("plane_xy", "plane_yz", "plane_xz"), c):
        H, W = p[name].shape[2:]
        for k, size in ((0, W), (1, H)):
            cell = torch.floor((uv[:, k] + 1) / 2 * (size - 1))
            out |= ~((cell >= -1) & (cell <= size - 1))
    return float(out.float().mean())


def test_the_out_of_range_case_has_out_of_range_cells():
    """CPU: the condition of the out-of-range cases, for both launches and both gauge shapes."""
    for gauge in ("equal", "unequal"):
        for n, _ in w16.LAUNCHES.values():
            share = _out_of_range_share(gauge, n)
            print(f"gauge_std {GAUGE_STD_OUT} gauge={gauge} {n} rays: {share:.3f} of the in-box samples have an out-of-range plane cell")
            assert 0.10 <= share <= 0.90, (gauge, n, share)


def _render_both(params, masked, launch, jitter, want16=16, **knobs):
    """{12: (rgb, depth), 16: (rgb, depth)} of ONE handle of the experiment library; want16: the kernel a launch under waves = 16 must take."""
    n, grid = w16.LAUNCHES[launch]
    rays = torch.from_numpy(w16._rays(n)).cuda()
    kw = dict(is_train=True, jitter=torch.from_numpy(w16._jitter(n)).cuda(), coin=0.7) if jitter else {}
    out = {}
    with _lib.library("exp") as L:
        f = field_for_case(w16._case(), params, w16._mask(masked), **w16.LEVEL3)
        for waves in (12, 16):
            with _lib.knobs(waves=waves, grid=grid, **knobs), torch.no_grad():
                o = f(rays, N_samples=S, white_bg=True, iteration=30001, **kw)
                assert L.ngf_debug_get(b"last_waves") == (want16 if waves == 16 else 12)
            out[waves] = (o["rgb_map"].clone(), o["depth_map"].clone())
        torch.cuda.synchronize()
        f.release()
    return out


def _assert_same_bits(out, finite=True):
    (rgb12, depth12), (rgb16, depth16) = out[12], out[16]
    if finite:
        assert torch.isfinite(rgb12).all() and torch.isfinite(depth12).all()
    lit = int((rgb12 < 1.0).any(dim=1).sum())
    assert lit >= rgb12.shape[0] // 4, lit                   # the colour path ran: background pixels compare equal whatever the collect does
    for a, b in ((rgb16, rgb12), (depth16, depth12)):
        if finite:
            assert torch.equal(w16._bits(a), w16._bits(b))
        else:                                                # NaN where the twelve-wave kernel has NaN, the same bits everywhere else
            nan = torch.isnan(b)
            assert torch.equal(torch.isnan(a), nan)
            assert torch.equal(w16._bits(a)[~nan], w16._bits(b)[~nan])
    return lit


@pytest.mark.gpu
@pytest.mark.parametrize("jitter", [False, True], ids=["nojitter", "jitter"])
@pytest.mark.parametrize("gauge", ["equal", "unequal"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
def test_out_of_range_cells_give_the_bits_of_twelve_waves(masked, gauge, jitter):
    n, _ = w16.LAUNCHES["four_widths"]
    share = _out_of_range_share(gauge, n)
    assert 0.10 <= share <= 0.90, share
    lit = _assert_same_bits(_render_both(_params(gauge), masked, "four_widths", jitter))
    print(f"out of range: mask={masked} gauge={gauge} jitter={jitter}: share {share:.3f}, {lit} of {n} rays are not background")


@pytest.mark.gpu
@pytest.mark.parametrize("launch", list(w16.LAUNCHES))
def test_non_finite_gauge_gives_the_bits_of_twelve_waves(launch):
    out = _render_both(_params("equal", 0.05, True), False, launch, False)
    _assert_same_bits(out, finite=False)
    print(f"non-finite gauge, {launch}: {int(torch.isnan(out[12][0]).any(dim=1).sum())} rays with a NaN colour, {int(torch.isnan(out[12][1]).sum())} with a NaN depth")


@pytest.mark.gpu
@pytest.mark.parametrize("launch,knobs,want16", [("four_widths", {}, 16), ("below_one_tile_per_wave", {}, 16), ("four_widths", {"tile_w": 64}, 16),
                                                 ("four_widths", {"tile_w": 16}, 12)],
                         ids=["four_widths", "one_ray_tiles", "tile_w64_unsplit", "tile_w16_keeps_twelve_waves"])
def test_the_collect_gives_the_bits_of_twelve_waves(launch, knobs, want16):
    _assert_same_bits(_render_both(w16._params("equal"), False, launch, False, want16=want16, **knobs))


@pytest.mark.gpu
def test_out_of_range_cells_against_the_oracle():
    launch = "below_one_tile_per_wave"
    n, _ = w16.LAUNCHES[launch]
    g = w16._case()
    step = geometry.step_size(g["aabb"], g["grid"], float(g["step_ratio"]))
    o_rgb, o_depth = oracle_for_case(g, _params("equal"), step, None).render(w16._rays(n), S, white_bg=True)
    rgb, depth = (t.cpu().numpy() for t in _render_both(_params("equal"), False, launch, False)[16])
    err, derr = np.abs(rgb - o_rgb), np.abs(depth - o_depth)
    print(f"out of range, sixteen waves: max|rgb - oracle| = {err.max():.3e}, max|depth - oracle| = {derr.max():.3e}")
    assert not (err > w16.ATOL + w16.RTOL * np.abs(o_rgb)).any(), float(err.max())
    assert not (derr > w16.ATOL_DEPTH + w16.RTOL * np.abs(o_depth)).any(), float(derr.max())


@pytest.mark.gpu
def test_the_product_library_above_its_threshold_gives_the_bits_of_twelve_waves():
    """No knob: a launch of 312 rays per CU takes the sixteen-wave kernel of the product library; the experiment library's twelve-wave render of the
    same field is the reference."""
    n = 312 * torch.cuda.get_device_properties(0).multi_processor_count
    rays = torch.from_numpy(np.resize(w16._rays(5000), (n, 6))).cuda()
    f = field_for_case(w16._case(), _params("equal"), None, **w16.LEVEL3)
    with torch.no_grad():
        own = f(rays, N_samples=16, white_bg=True, iteration=30001)
    assert _lib.lib().ngf_debug_get(b"last_waves") == 16
    torch.cuda.synchronize()
    f.release()
    with _lib.library("exp") as L:
        f = field_for_case(w16._case(), _params("equal"), None, **w16.LEVEL3)
        with _lib.knobs(waves=12), torch.no_grad():
            ref = f(rays, N_samples=16, white_bg=True, iteration=30001)
            assert L.ngf_debug_get(b"last_waves") == 12
        torch.cuda.synchronize()
        f.release()
    assert int((ref["rgb_map"] < 1.0).any(dim=1).sum()) >= n // 4
    assert torch.equal(w16._bits(own["rgb_map"]), w16._bits(ref["rgb_map"])) and torch.equal(w16._bits(own["depth_map"]), w16._bits(ref["depth_map"]))
