"""GPU checks of the NeuTex occupancy grid (csrc/ngf_uv_occupancy.hip, the OCC instantiations of uv_render_kernel in csrc/ngf_uv.hpp, and the
Python surface in uvmapping.py) against the numpy restatements of tests/uv_occupancy_ref.py, which tests/test_uv_occupancy_cpu.py checks first.

The masked frame is, by definition, the reference's frame with sigma set to 0 in empty cells.  So the render is held to three things: every
sample's density and colour are either the unmasked launch's bits or exactly 0; which of the two equals the restated look-up at the sample's
float32 position (for every sample whose float64 position keeps 1e-5 from the cell boundaries: all but <= 0.07 % of them on these batches); and
the pixel is the float64 compositing of the kernel's own masked samples inside the rounding bound B(S) of tests/uv_render_ref.py."""
import ctypes as C
import functools
import pickle

import numpy as np
import pytest
import torch

import uv_occupancy_ref as O
import uv_render_ref as R
from ngf_amd import _lib, synth, uvmapping

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRIMS = ("sphere", "square")
F = np.float32
BG1 = np.array([0.2, 0.5, 0.8], F)
BG2 = np.array([[0.2, 0.5, 0.8], [0.9, 0.1, 0.3]], F)
ALL = ("color", "transmittance", "sigma", "point_color")


def _seed(prim):
    return R.MODEL_SEEDS[PRIMS.index(prim)]


@functools.lru_cache(maxsize=8)
def _net(prim, split=False):
    net = uvmapping.NeuTex(primitive_type=prim, sample_num=64, device=DEV, split_bf16=split)
    net.load_params(synth.uvmapping_params(_seed(prim), prim))
    return net


def _bg(bg, N):
    return None if bg is None else np.broadcast_to(np.asarray(bg, F).reshape(-1, 3)[:N], (N, 3)).copy()


def _render(net, cam, rd, U, bg=None, debug=True, stats=True):
    net.sample_num = U.shape[-1]
    b = _bg(bg, rd.shape[0])
    out = net(torch.from_numpy(cam), torch.from_numpy(rd), None if b is None else torch.from_numpy(b), jitter_u=torch.from_numpy(U), debug=debug,
              collect_stats=stats)
    r = {k: v.cpu().numpy() for k, v in out.items()}
    if stats:
        r["stats"] = tuple(int(x) for x in net.last_stats[:2].cpu())
    return r


def _same_bits(a, b, keys=ALL):
    return all(a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in keys)


class _masked:
    """``with _masked(net, mask):`` -- the cached model with a mask, without one again afterwards."""

    def __init__(self, net, mask):
        self.net, self.mask = net, mask

    def __enter__(self):
        self.net.set_occupancy(self.mask)
        return self.net

    def __exit__(self, *exc):
        self.net.set_occupancy(None)
        return False


# ---- 1. the look-up ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", O.LOOKUP_SHAPES)
def test_lookup_equals_the_restatement(shape):
    net = _net("sphere")
    pts = np.concatenate([(synth.hash_uniform(31, 920, (4096, 3)) * F(2.4) - F(1.2)).astype(F), O.special_points(shape)])
    assert np.isnan(pts).any() and (pts == 1).any() and (pts == -1).any()
    for vol in (O.random_mask(shape), O.checkerboard(shape)):
        with _masked(net, vol):
            got = net.occupied(pts).cpu().numpy()
            assert np.array_equal(net.occupancy.volume().cpu().numpy(), vol)
        want = O.lookup(O.pack(vol), shape, pts)
        assert got.dtype == bool and np.array_equal(got, want), np.flatnonzero(got != want)[:10]
        assert want.any() or not vol.any()
    assert net.occupancy is None
    with pytest.raises(RuntimeError):
        net.occupied(pts)


# ---- 2. the reduction ----------------------------------------------------------------------------------------------------------------------------
GUARD = 64


def _reduce(sigma, shape, thr, dilate):
    """ngf_uv_occupancy_from_lattice -> (image bytes, the 64 guard bytes behind them)"""
    L = _lib.lib()
    nbytes = (int(np.prod(shape)) + 7) // 8
    s = torch.from_numpy(np.ascontiguousarray(sigma, F)).to(DEV)
    bits = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    need = L.ngf_uv_occupancy_workspace_bytes(*shape)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(L.ngf_uv_occupancy_from_lattice(s.data_ptr(), *shape, float(thr), dilate, bits.data_ptr(), ws.data_ptr(), need,
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    b = bits.cpu().numpy()
    return b[:nbytes], b[nbytes:]


def _lattices(shape):
    """[(name, lattice, thresholds)]: random values, single hot corners (a grid corner, an edge, the interior), NaN and infinities."""
    full = tuple(n + 1 for n in shape)
    rnd = synth.hash_normal(53, 930, full).astype(F)
    out = [("random", rnd, (float(rnd.min()) - 1.0, float(np.median(rnd)), float(rnd.max()) + 1.0))]
    for name, at in (("corner", tuple(n for n in shape)), ("edge", (shape[0] // 2, 0, shape[2])), ("interior", tuple(n // 2 for n in shape))):
        s = np.zeros(full, F)
        s[at] = 1.0
        out.append(("hot " + name, s, (0.5,)))
    odd = rnd.copy()
    flat = odd.reshape(-1)
    flat[::7] = np.nan
    flat[1::11] = np.inf
    flat[2::5] = -np.inf
    finite = flat[np.isfinite(flat)]
    out.append(("nan and inf", odd, (float(finite.min()) - 1.0, float(np.median(finite)), float(finite.max()) + 1.0) if finite.size else (0.0,)))
    return out


@pytest.mark.parametrize("shape", O.REDUCE_SHAPES)
def test_reduction_equals_the_restatement_byte_for_byte(shape):
    for name, sigma, thresholds in _lattices(shape):
        for thr in thresholds:
            for dilate in (0, 1, 2):
                got, guard = _reduce(sigma, shape, thr, dilate)
                want = O.from_lattice(sigma, thr, dilate)
                assert np.array_equal(got, want), (name, thr, dilate, np.flatnonzero(got != want)[:10])
                assert (guard == 0xA5).all(), (name, thr, dilate)
        again, _ = _reduce(sigma, shape, thresholds[0], 1)
        assert np.array_equal(again, _reduce(sigma, shape, thresholds[0], 1)[0])          # two runs, the same bytes
    name, sigma, thresholds = _lattices(shape)[0]
    assert not np.unpackbits(_reduce(sigma, shape, thresholds[2], 2)[0]).any()            # above all values: empty
    assert np.unpackbits(_reduce(sigma, shape, thresholds[0], 0)[0]).sum() == int(np.prod(shape))          # below all: full, tail bits 0


# ---- 3. the render: decisions and values ---------------------------------------------------------------------------------------------------------
def _composite_check(out, U, bg, tag):
    N, Rn, S = U.shape
    sigma, col = out["sigma"].reshape(N * Rn, S), out["point_color"].reshape(N * Rn, S, 3)
    b = _bg(bg, N)
    lin64, _, T64 = R.composite64(sigma, col, sigma != 0, U.reshape(N * Rn, S), None if b is None else np.repeat(b, Rn, 0))
    c = out["color"].reshape(N * Rn, 3).astype(np.float64)
    open_ = c < 1.0
    assert open_.mean() > 0.5
    e_lin = float(np.abs(c ** 2.2 - 1e-5 - lin64)[open_].max())
    e_T = float(np.abs(out["transmittance"].reshape(-1).astype(np.float64) - T64).max())
    B = R.bound(S, max(float(col.max()), 0.0))
    print(f"uv_occupancy {tag}: compositing alone colour {e_lin:.2e} T {e_T:.2e}, B(S) {B:.2e}")
    assert e_lin <= B and e_T <= B, (tag, e_lin, e_T, B)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("prim", PRIMS)
@pytest.mark.parametrize("S", O.RENDER_S)
def test_masked_render_decides_by_the_restatement_and_keeps_the_bits(S, prim, split):
    net = _net(prim, split)
    for bname, cam, rd, U in O.render_batches(prim, S):
        bg = BG2[:rd.shape[0]]
        plain = _render(net, cam, rd, U, bg)
        for mname, vol in O.render_masks():
            tag = f"{bname} S={S} {prim} split={int(split)} {mname}"
            with _masked(net, vol):
                out = _render(net, cam, rd, U, bg)
            keep, pinned, valid, _, _ = O.decisions(cam, rd, U, vol)
            assert np.array_equal(plain["sigma"] != 0, valid)
            # every sample: the unmasked bits or exactly 0
            kept = out["sigma"] != 0
            same_s = out["sigma"].view(np.uint32) == plain["sigma"].view(np.uint32)
            same_c = (out["point_color"].view(np.uint32) == plain["point_color"].view(np.uint32)).all(-1)
            assert (same_s & same_c)[kept].all(), tag
            assert not out["point_color"][~kept].any() and (kept <= valid).all()
            # the decision is the restated look-up at the float32 position wherever the float64 position keeps the margin
            assert np.array_equal(kept[pinned], keep[pinned]), (tag, int((kept != keep)[pinned].sum()))
            near = valid & ~pinned
            assert near.sum() <= O.NEAR_LIMIT * valid.sum()
            print(f"uv_occupancy {tag}: {valid.sum()} in-cube, {kept.sum()} kept, {near.sum()} near a boundary ({int((kept != keep)[near].sum())} of them decided the other way)")
            assert 0 < kept.sum() < valid.sum()
            assert out["stats"] == R.expected_stats(kept, S), (tag, out["stats"], R.expected_stats(kept, S))
            assert out["stats"][0] < plain["stats"][0]
            _composite_check(out, U, bg, tag)
        assert _same_bits(_render(net, cam, rd, U, bg), plain)          # without the mask again: the original bits


# ---- 4. limits -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
def test_an_all_ones_mask_changes_nothing(split):
    S, prim = 65, "sphere"
    net = _net(prim, split)
    _, cam, rd, U = O.render_batches(prim, S)[0]
    plain = _render(net, cam, rd, U, BG1)
    for shape in ((1, 1, 1), (5, 7, 16)):
        with _masked(net, np.ones(shape, bool)):
            out = _render(net, cam, rd, U, BG1)
        assert _same_bits(out, plain) and out["stats"] == plain["stats"], shape
    assert plain["stats"][0] > 0


@pytest.mark.parametrize("bg", [None, "one", "per camera"])
def test_an_all_zeros_mask_leaves_the_background(bg):
    S, prim = 64, "square"
    net = _net(prim)
    _, cam, rd, U = O.render_batches(prim, S)[1]          # two cameras
    b = {None: None, "one": BG1, "per camera": BG2}[bg]
    with _masked(net, np.zeros((4, 3, 2), bool)):
        out = _render(net, cam, rd, U, b)
    assert out["stats"] == (0, 0) and not out["sigma"].any() and not out["point_color"].any()
    assert (out["transmittance"] == 1.0).all()
    rows = np.zeros((rd.shape[0], 3), F) if b is None else _bg(b, rd.shape[0])
    want = np.clip(np.power(rows * F(1.0) + F(1e-5), F(1.0 / 2.2)), F(0.0), F(1.0))[:, None, :]
    assert want.dtype == F
    assert (np.abs(out["color"] - want) <= 2 * np.spacing(want)).all()          # the tone-mapped background (2 ulp for powf)
    if bg == "per camera":
        assert not np.array_equal(out["color"][0], out["color"][1])


def test_a_mask_with_one_occupied_cell():
    S, prim, shape = 129, "sphere", (4, 4, 4)
    net = _net(prim)
    _, cam, rd, U = O.render_batches(prim, S)[0]
    plain = _render(net, cam, rd, U)
    keep_all, _, valid, p32, _ = O.decisions(cam, rd, U, np.ones(shape, bool))
    c = np.stack([O.cell(p32[..., k], shape[k]) for k in range(3)], -1)[valid]
    cells, counts = np.unique(c, axis=0, return_counts=True)
    at = tuple(int(x) for x in cells[np.argmax(counts)])          # the cell most samples fall in
    vol = O.single_cell(shape, at)
    with _masked(net, vol):
        out = _render(net, cam, rd, U)
    keep, pinned, _, _, _ = O.decisions(cam, rd, U, vol)
    kept = out["sigma"] != 0
    assert np.array_equal(kept[pinned], keep[pinned]) and kept.sum() > 0
    assert np.array_equal(out["sigma"][kept].view(np.uint32), plain["sigma"][kept].view(np.uint32))
    assert out["stats"] == R.expected_stats(kept, S)
    net.set_occupancy(vol)
    net.set_occupancy(None)
    assert _same_bits(_render(net, cam, rd, U), plain)          # set_occupancy(None) restores the original bits


# ---- 5. the Python surface -----------------------------------------------------------------------------------------------------------------------
def _fresh(prim="sphere", S=64):
    net = uvmapping.NeuTex(primitive_type=prim, sample_num=S, device=DEV)
    net.load_params(synth.uvmapping_params(_seed(prim), prim))
    return net


def test_build_occupancy_equals_the_restatement_on_the_lattice_and_is_installed():
    S, prim, shape = 64, "sphere", (8, 9, 10)
    net = uvmapping.NeuTex(primitive_type=prim, sample_num=S, device=DEV)
    net.load_params(O.smooth_density_params(_seed(prim), prim))          # a density with empty regions: the seeded one leaves no cell empty
    _, cam, rd, U = O.render_batches(prim, S)[0]
    plain = _render(net, cam, rd, U)
    vol, lo, step = net.density_lattice(tuple(n + 1 for n in shape), clip=False)
    assert np.array_equal(lo, np.full(3, -1, F)) and np.array_equal(step, (F(2.0) / np.asarray(shape, F)).astype(F))
    sigma = vol.cpu().numpy()
    thr = float(np.median(sigma))
    occ = net.build_occupancy(shape, threshold=thr, dilate=1)
    assert occ is net.occupancy and occ.shape == shape and occ.dilate == 1 and occ.threshold == float(F(thr))
    want = O.from_lattice(sigma, F(thr), 1)
    assert np.array_equal(occ.bits.cpu().numpy(), want)
    assert np.array_equal(occ.volume().cpu().numpy(), O.unpack(want, shape)) and occ.fraction() == pytest.approx(O.unpack(want, shape).mean())
    assert 0 < occ.fraction() < 1
    out = _render(net, cam, rd, U)
    assert out["stats"][0] < plain["stats"][0] and out["stats"][1] <= plain["stats"][1]
    keep, pinned, _, _, _ = O.decisions(cam, rd, U, O.unpack(want, shape))
    assert np.array_equal((out["sigma"] != 0)[pinned], keep[pinned])
    # the default threshold: the density whose opacity over one nominal segment is alpha_thres
    d = net.build_occupancy(4, alpha_thres=1e-3, dilate=0)
    assert d.threshold == float(F(-np.log1p(-1e-3) / (2.0 / S))) and d.shape == (4, 4, 4)
    for bad in ({"dilate": 3}, {"dilate": -1}, {"resolution": 0}, {"resolution": (4, 4)}, {"threshold": float("nan")}):
        with pytest.raises(ValueError):
            net.build_occupancy(**{"resolution": 4, **bad})
    net.release()


def test_the_mask_survives_a_checkpoint_a_handle_rebuild_and_pickling():
    S, prim = 65, "square"
    net = _fresh(prim, S)
    _, cam, rd, U = O.render_batches(prim, S)[0]
    vol = O.random_mask((5, 7, 16))
    net.set_occupancy(vol)
    out = _render(net, cam, rd, U, BG1)
    twin = _fresh(prim, S)
    twin.load_occupancy(net.occupancy_state())
    assert _same_bits(_render(twin, cam, rd, U, BG1), out)
    clone = pickle.loads(pickle.dumps(net))
    assert clone._handle is None and np.array_equal(clone.occupancy.volume().cpu().numpy(), vol)
    assert _same_bits(_render(clone, cam, rd, U, BG1), out)
    # a parameter change rebuilds the handle; the mask is pushed again (and is NOT rebuilt: it is the user's)
    key0 = net._key
    with torch.no_grad():
        net.net_texture.color1.bias.add_(0.125)
    moved = _render(net, cam, rd, U, BG1)
    assert net._key != key0
    assert np.array_equal(moved["sigma"] != 0, out["sigma"] != 0) and moved["stats"] == out["stats"]
    assert not np.array_equal(moved["point_color"], out["point_color"])
    for m in (net, twin, clone):
        m.release()


def test_one_ray_per_wave_with_a_mask_raises():
    S, prim = 64, "sphere"
    net = _net(prim)
    _, cam, rd, U = O.render_batches(prim, S)[0]
    try:
        with _masked(net, O.random_mask((5, 7, 16))):
            with pytest.raises(RuntimeError, match="uv_tiles"):
                with _lib.knobs(uv_tiles=1):
                    _render(net, cam, rd, U)
            out = _render(net, cam, rd, U)          # the handle is whole after the refusal
            assert (out["sigma"] != 0).any()
    finally:
        _lib.check(_lib.lib().ngf_debug_set(b"uv_tiles", -1))
    assert _lib.lib().ngf_debug_get(b"uv_tiles") == -1


def test_the_differentiable_path_ignores_the_mask():
    S, prim = 64, "square"
    net = _fresh(prim, S)
    _, cam, rd, U = O.render_batches(prim, S)[1]
    tp = torch.from_numpy(R.template(prim)).to(DEV)
    args = (torch.from_numpy(cam), torch.from_numpy(rd), torch.from_numpy(BG2), torch.from_numpy(U))
    net.differentiable = True

    def run():
        o = net(args[0], args[1], args[2], jitter_u=args[3], template_points=tp)
        return {k: o[k].detach().cpu().numpy() for k in ("color", "transmittance", "points", "points_original", "points_inverse_weights", "uv")}

    a = run()
    net.set_occupancy(np.zeros((4, 4, 4), bool))
    b = run()
    assert all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)
    with torch.no_grad():          # the eval path of the same module does consult it
        assert (_render(net, cam, rd, U, BG2)["transmittance"] == 1.0).all()
    net.release()
    net.release_grad_engine()
