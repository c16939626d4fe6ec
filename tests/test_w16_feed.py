"""The sixteen-wave level-3 pass reads its colour planes' descriptors (pointer, row stride) ONCE, at the top of the pass, instead of once per
quarter-plane stage (csrc/ngf_shade16.hpp baked16q_issue).  The addresses it loads from are the same, so the pass must
keep the bits of the twelve-wave kernel, which reads every descriptor where it uses it.  Every case renders ONE handle of libngf_hip_exp.so under
ngf_debug_set("waves", 12) and ("waves", 16), asserts ngf_debug_get("last_waves") and compares rgb_map and depth_map with torch.equal on their
int32 views (NaN where the reference has NaN in the non-finite case).  Geometry, rays, masks and launches are those of tests/test_waves16.py
(S = 64; 5 000 rays on 8 workgroups = tiles of 8, 4, 2 and 1 rays; 300 rays on the whole device = fewer tiles than waves, one-ray tiles).

What these cases add to tests/test_waves16.py and tests/test_w16_trim.py:
  - colour planes of THREE sizes (32 x 32, 30 x 28, 32 x 24: row strides 34, 30, 26), so a pass that took one plane's pointer or stride for another
    reads other texels -- the existing cases have three equal planes and cannot see that;
  - a 12 x 12 patch of +inf (four channels) and a 3 x 3 patch of NaN (one channel) in ONE plane's appearance channels: non-finite colour texels.  What
    the MLP makes of them may be finite again (a sigmoid saturates, the integer ReLU takes a negative NaN to 0), so the case asserts that the frame
    is not the finite planes' frame, not that it has NaNs;
  - a launch of one-ray tiles chosen by their number of active samples, so that last passes of 1, 15 and 16 entries are there (a ray's passes run
    back to back once its march has ended, its first pass straight after a march iteration);
  - one handle rendered, its parameters replaced (other values, other plane sizes, hence other pointers and strides), rendered again;
  - the MaskSkip<> and GaugeAny<> instantiations, jitter, and the product library above its 312-rays-per-CU switch, all on the unequal planes."""
import functools

import numpy as np
import pytest
import torch

import ngf_amd  # noqa: F401
from ngf_amd import _lib, synth
from helpers import field_for_case
import test_waves16 as w16

S = w16.S
CROPS = {"xy": (32, 32), "yz": (30, 28), "xz": (32, 24)}      # (H, W) kept of the 32 x 32 planes


@functools.lru_cache(maxsize=None)
def _params(gauge="equal", seed=17, nonfinite=False, swap=False):
    p = dict(synth.triplane_params(seed, w16.PLANE_HW, (32, 32), preset="R1", gauge_std=0.05))
    for k, (name, hw) in enumerate(zip(("xy", "yz", "xz"), w16.GAUGE_HW[gauge])):
        p[f"gauge_{name}"] = (synth.hash_normal(seed, 60 + k, (1, 2, hw[0], hw[1])) * np.float32(0.05)).astype(np.float32)
    names = ("xz", "xy", "yz") if swap else ("xy", "yz", "xz")      # swap: every plane gets another plane's size
    for name, src in zip(("xy", "yz", "xz"), names):
        h, w = CROPS[src]
        p[f"plane_{name}"] = np.ascontiguousarray(p[f"plane_{name}"][:, :, :h, :w])
    if nonfinite:
        q = p["plane_yz"].copy()
        q[0, 20:24, 8:20, 8:20] = np.inf            # appearance channels (16 ..): density stays finite
        q[0, 40, 22:25, 3:6] = np.nan
        p["plane_yz"] = q
    return p


def test_the_three_colour_planes_have_three_strides():
    """CPU: the condition of every case below."""
    for swap in (False, True):
        p = _params(swap=swap)
        shapes = [p[f"plane_{n}"].shape[2:] for n in ("xy", "yz", "xz")]
        assert len({s[1] for s in shapes}) == 3 and len(set(shapes)) == 3, shapes
    assert not np.isfinite(_params(nonfinite=True)["plane_yz"][0, 16:]).all() and np.isfinite(_params(nonfinite=True)["plane_yz"][0, :16]).all()


def _render(f, L, rays, waves, grid, jitter=None):
    kw = dict(is_train=True, jitter=jitter, coin=0.7) if jitter is not None else {}
    with _lib.knobs(waves=waves, grid=grid), torch.no_grad():
        o = f(rays, N_samples=S, white_bg=True, iteration=30001, **kw)
        assert L.ngf_debug_get(b"last_waves") == waves          # the kernel that was asked for ran
    return o["rgb_map"].clone(), o["depth_map"].clone()


def _assert_same_bits(got, ref, finite=True):
    (rgb16, depth16), (rgb12, depth12) = got, ref
    if finite:
        assert torch.isfinite(rgb12).all() and torch.isfinite(depth12).all()
    lit = int((rgb12 < 1.0).any(dim=1).sum())
    assert lit >= rgb12.shape[0] // 4, lit                       # the colour path ran
    for a, b in ((rgb16, rgb12), (depth16, depth12)):
        nan = torch.isnan(b)
        assert finite is False or not nan.any()
        assert torch.equal(torch.isnan(a), nan)
        assert torch.equal(w16._bits(a)[~nan], w16._bits(b)[~nan])
    return lit


def _both(params, masked, launch, jitter):
    n, grid = w16.LAUNCHES[launch]
    rays = torch.from_numpy(w16._rays(n)).cuda()
    jit = torch.from_numpy(w16._jitter(n)).cuda() if jitter else None
    with _lib.library("exp") as L:
        f = field_for_case(w16._case(), params, w16._mask(masked), **w16.LEVEL3)
        out = {waves: _render(f, L, rays, waves, grid, jit) for waves in (12, 16)}
        torch.cuda.synchronize()
        f.release()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("jitter", [False, True], ids=["nojitter", "jitter"])
@pytest.mark.parametrize("gauge", ["equal", "unequal"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("launch", list(w16.LAUNCHES))
def test_planes_of_three_sizes_give_the_bits_of_twelve_waves(launch, masked, gauge, jitter):
    out = _both(_params(gauge), masked, launch, jitter)
    lit = _assert_same_bits(out[16], out[12])
    print(f"{launch} mask={masked} gauge={gauge} jitter={jitter}: {lit} rays are not background")


@pytest.mark.gpu
@pytest.mark.parametrize("launch", list(w16.LAUNCHES))
def test_non_finite_colour_texels_give_the_bits_of_twelve_waves(launch):
    out = _both(_params(nonfinite=True), False, launch, True)
    _assert_same_bits(out[16], out[12], finite=False)
    clean = _both(_params(), False, launch, True)[12][0]
    changed = int((w16._bits(out[12][0]) != w16._bits(clean)).any(dim=1).sum())
    bad = int((~torch.isfinite(out[12][0])).any(dim=1).sum())
    print(f"non-finite colour texels, {launch}: {changed} rays differ from the finite planes' frame, {bad} of them have a non-finite colour")
    assert changed > 0                                           # the patches were hit


@pytest.mark.gpu
def test_last_passes_of_one_fifteen_and_sixteen_entries():
    """One-ray tiles (fewer rays than the device has waves) picked by their number of active samples A (weight > the field's threshold, from the
    march hook): A mod 16 = 1, 15 and 0, A > 0 -- the last pass of such a ray has 1, 15 and 16 entries; the rays with A > 16 among them run several
    passes back to back."""
    with _lib.library("exp") as L:
        f = field_for_case(w16._case(), _params("unequal"), None, **w16.LEVEL3)
        cand = torch.from_numpy(w16._rays(20000)).cuda()
        _, weight = f.march(cand, S)
        active = (weight > float(w16._case()["thr"])).sum(dim=1)
        pick = []
        for r in (1, 15, 0):
            idx = torch.nonzero((active % 16 == r) & (active > 0)).flatten()[:60]
            assert idx.numel() >= 1, (r, int(idx.numel()))      # the candidates have such rays
            pick.append(idx)
        rays = cand[torch.cat(pick)].contiguous()
        assert int((active[torch.cat(pick)] > 16).sum()) >= 8     # rays with more than one pass
        assert rays.shape[0] < 256                               # below one tile per wave: every tile is one ray
        out = {waves: _render(f, L, rays, waves, -1) for waves in (12, 16)}
        torch.cuda.synchronize()
        f.release()
    _assert_same_bits(out[16], out[12])
    print(f"{rays.shape[0]} one-ray tiles, active samples per ray {int(active[torch.cat(pick)].min())} .. {int(active[torch.cat(pick)].max())}")


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
def test_replaced_parameters_are_read_through_new_descriptors(masked):
    """One field object: render, replace every parameter (other seed; every plane takes another plane's size), render again -- both times the bits of
    the twelve-wave kernel, and the second frame is not the first."""
    n, grid = w16.LAUNCHES["four_widths"]
    rays = torch.from_numpy(w16._rays(n)).cuda()
    frames = []
    with _lib.library("exp") as L:
        f = field_for_case(w16._case(), _params("unequal"), w16._mask(masked), **w16.LEVEL3)
        for params in (_params("unequal"), _params("unequal", seed=23, swap=True)):
            f.load_params(params)
            out = {waves: _render(f, L, rays, waves, grid) for waves in (16, 12)}
            _assert_same_bits(out[16], out[12])
            frames.append(out[16][0])
        torch.cuda.synchronize()
        f.release()
    assert not torch.equal(frames[0], frames[1])


@pytest.mark.gpu
def test_the_product_library_above_its_threshold_on_planes_of_three_sizes():
    """No knob: 312 rays per CU take the product library's sixteen-wave kernel; the experiment library's twelve-wave render is the reference."""
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
    _assert_same_bits((own["rgb_map"], own["depth_map"]), (ref["rgb_map"], ref["depth_map"]))
