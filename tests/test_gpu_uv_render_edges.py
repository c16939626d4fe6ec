"""GPU checks of the NeuTex render kernel (csrc/ngf_uv.hpp uv_render_kernel) where tests/test_gpu_uv.py never takes it: past one 64-sample
chunk (the carried prefix sum, transmittance and colour, the partial last chunk), at chosen in-cube totals of a ray pair (none, one tile, one
padded two-tile pass, the loop, both rays full), and at ray geometries the DTU camera never gives (misses, a camera inside the cube,
axis-parallel rays, the cube's diagonal, rays that graze an edge).  tests/uv_render_ref.py builds the batches and
tests/test_uv_render_edges_cpu.py checks them, the oracle above 64 samples and the bound B(S) on the CPU first.

Three yardsticks.  The fp64 eager forward (tests/uv_train_eager.py) under the project's rule e_hip < max(2e-5, 4 e_torch32), on batches whose
samples keep 1e-5 from the faces.  The C oracle, fp32 like the kernel and in the reference's operation order: the in-cube mask and the work
counters exactly, the per-sample and per-pixel tolerances of tests/test_gpu_uv.py.  And compositing alone: the kernel's pixel with the tone map
undone against float64 compositing of the kernel's OWN per-sample densities and colours, inside the rounding bound B(S) -- the networks'
ill-conditioning cancels, a dropped, doubled or stale sample or a restarted transmittance does not.  All rays and all samples are compared."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import uv_render_ref as R
import uv_train_eager as E
from ngf_amd import _lib, synth, uvmapping
from test_gpu_uv import PCOL_TOL, SIGMA_RTOL, T_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRIMS = ("sphere", "square")
PIX_TOL, POSE_TOL = 2e-5, 1e-4          # the project's rule against fp64; north_star's pixel bound for made-up poses against the oracle
BG1 = np.array([0.2, 0.5, 0.8], np.float32)
BG3 = np.array([[0.2, 0.5, 0.8], [0.9, 0.1, 0.3], [0.05, 0.7, 0.45]], np.float32)
GEOMETRY_MODEL = {"miss": 0, "inside": 1, "axis": 0, "diagonal": 1, "graze": 0}          # kind -> index into PRIMS and R.MODEL_SEEDS


def _seed(prim):
    return R.MODEL_SEEDS[PRIMS.index(prim)]


@functools.lru_cache(maxsize=8)
def _net(prim, split=False):
    net = uvmapping.NeuTex(primitive_type=prim, sample_num=64, device=DEV, split_bf16=split)
    net.load_params(synth.uvmapping_params(_seed(prim), prim))
    return net


def _bg(bg, N):
    return None if bg is None else np.broadcast_to(np.asarray(bg, np.float32).reshape(-1, 3)[:N], (N, 3)).copy()


def _render(net, cam, rd, U, bg=None, debug=False, stats=False):
    """One launch of the batch entry -> numpy: color [N,R,3], transmittance [N,R], with debug sigma [N,R,S] and point_color [N,R,S,3],
    with stats (st_samples, st_pass)."""
    net.sample_num = U.shape[-1]
    b = _bg(bg, rd.shape[0])
    out = net(torch.from_numpy(cam), torch.from_numpy(rd), None if b is None else torch.from_numpy(b), jitter_u=torch.from_numpy(U),
              debug=debug, collect_stats=stats)
    r = {k: v.cpu().numpy() for k, v in out.items()}
    if stats:
        r["stats"] = tuple(int(x) for x in net.last_stats[:2].cpu())
    return r


def _same_bits(a, b, keys=("color", "transmittance")):
    return all(a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in keys)


def _eager(prim, cam, rd, U, bg, dtype):
    net = E.make_net(E.model_params(_seed(prim), prim), prim, U.shape[-1], DEV, dtype)
    t = lambda a: torch.from_numpy(np.asarray(a)).to(DEV, dtype)          # noqa: E731
    b = _bg(bg, rd.shape[0])
    with torch.no_grad():
        o = E.forward(net, t(cam), t(rd), None if b is None else t(b), t(U), t(R.template(prim)), extras=True)
    return o["color"].double().cpu().numpy(), o["transmittance"].double().cpu().numpy(), o["valid"].cpu().numpy()


def _compositing_residual(out, U, bg):
    """max |pixel with the tone map undone - composite64 of the kernel's own samples| and max |T - T64|, and B(S) for them."""
    N, Rn, S = U.shape
    sigma, col = out["sigma"].reshape(N * Rn, S), out["point_color"].reshape(N * Rn, S, 3)
    b = _bg(bg, N)
    lin64, _, T64 = R.composite64(sigma, col, sigma != 0, U.reshape(N * Rn, S), None if b is None else np.repeat(b, Rn, 0))
    c = out["color"].reshape(N * Rn, 3).astype(np.float64)
    open_ = c < 1.0                                   # below the clamp the tone map can be undone
    assert open_.mean() > 0.5
    lin = c ** 2.2 - 1e-5
    e_lin = float(np.abs(lin - lin64)[open_].max())
    e_T = float(np.abs(out["transmittance"].reshape(-1).astype(np.float64) - T64).max())
    return e_lin, e_T, R.bound(S, col.max())


# ---- (a) sample counts across the chunk edge, against fp64 ------------------------------------------------------------------------------
def _chunk_case(S, prim, split):
    cam, rd, U = R.pool_rays(prim, S, R.SEED)
    assert rd.shape[1] % 2 == 1
    net = _net(prim, split)
    out = _render(net, cam, rd, U, BG1, debug=True, stats=True)
    c64, t64, v64 = _eager(prim, cam, rd, U, BG1, torch.float64)
    c32, t32, _ = _eager(prim, cam, rd, U, BG1, torch.float32)
    assert (v64.sum(-1) == 0).sum() == 3 and v64.any()
    assert np.array_equal(out["sigma"] != 0, v64), "in-cube mask differs from fp64"
    assert out["stats"] == R.expected_stats(v64, S)
    bad = []          # every figure is printed and every check made before the test fails: one run names all that a defect breaks
    for name, got, r32, r64 in (("colour", out["color"], c32, c64), ("transmittance", out["transmittance"], t32, t64)):
        e_hip, e_t32 = float(np.abs(got - r64).max()), float(np.abs(r32 - r64).max())
        print(f"uv_render_edges S={S} {prim} split={int(split)} {name}: e_hip {e_hip:.2e} e_torch32 {e_t32:.2e} of fp64")
        if not e_hip < max(PIX_TOL, 4 * e_t32):
            bad.append((name + " against fp64", e_hip, e_t32))
    e_lin, e_T, B = _compositing_residual(out, U, BG1)
    print(f"uv_render_edges S={S} {prim} split={int(split)} compositing alone: colour {e_lin:.2e} T {e_T:.2e}, B(S) {B:.2e}")
    if not (e_lin <= B and e_T <= B):
        bad.append(("compositing alone", e_lin, e_T, B))
    assert not bad, bad
    assert _same_bits(_render(net, cam, rd, U, BG1), out)          # a second launch


@pytest.mark.parametrize("prim", PRIMS)
@pytest.mark.parametrize("S", R.CHUNK_S)
def test_sample_counts_across_the_chunk_edge_against_fp64(S, prim):
    _chunk_case(S, prim, False)


@pytest.mark.parametrize("prim", PRIMS)
@pytest.mark.parametrize("S", [65, 128])
def test_sample_counts_across_the_chunk_edge_against_fp64_split_bf16(S, prim):
    _chunk_case(S, prim, True)


def test_the_host_pointer_entry_gives_the_batch_entry_bits_at_129_samples():
    S, prim = 129, "sphere"
    cam, rd, U = R.pool_rays(prim, S, R.SEED)
    net = _net(prim)
    out = _render(net, cam, rd, U, BG1, debug=True, stats=True)
    n = rd.shape[1]
    d, u = torch.from_numpy(rd[0]).to(DEV), torch.from_numpy(U[0]).to(DEV)
    col, tr = torch.empty((n, 3), device=DEV), torch.empty((n,), device=DEV)
    sg, pc = torch.zeros((n, S), device=DEV), torch.zeros((n, S, 3), device=DEV)
    st = torch.zeros(16, dtype=torch.int64, device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib().ngf_uv_render(net.handle(), (C.c_float * 3)(*cam[0].tolist()), d.data_ptr(), (C.c_float * 3)(*BG1.tolist()), u.data_ptr(),
                                            n, S, col.data_ptr(), tr.data_ptr(), sg.data_ptr(), pc.data_ptr(), st.data_ptr(),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    host = {"color": col.cpu().numpy()[None], "transmittance": tr.cpu().numpy()[None], "sigma": sg.cpu().numpy()[None], "point_color": pc.cpu().numpy()[None]}
    assert _same_bits(host, out, ("color", "transmittance", "sigma", "point_color"))
    assert tuple(int(x) for x in st[:2].cpu()) == out["stats"]


# ---- (b), (c) pair totals and geometry kinds, against the C oracle -------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def _oracle_case(kind, S, prim, with_bg):
    cam, rd, U = R.paired_rays(S, R.pair_targets(S)) if kind == "paired" else R.geometry_rays(kind, S)
    bg = BG3[:rd.shape[0]] if with_bg else None
    return cam, rd, U, bg, R.oracle_render(_seed(prim), prim, cam, rd, U, bg)


def _against_oracle(kind, S, prim, with_bg, split):
    """Exact mask, exact counters, the tolerances of tests/test_gpu_uv.py per sample and north_star's per pixel -> (out, oracle dict)."""
    cam, rd, U, bg, o = _oracle_case(kind, S, prim, with_bg)
    net = _net(prim, split)
    out = _render(net, cam, rd, U, bg, debug=True, stats=True)
    valid = o["valid"]
    assert np.array_equal(out["sigma"] != 0, valid), "in-cube mask differs from the oracle's"
    assert out["stats"] == R.expected_stats(valid, S), (out["stats"], R.expected_stats(valid, S))
    if valid.any():
        np.testing.assert_allclose(out["sigma"][valid], o["sigma"][valid], rtol=SIGMA_RTOL, atol=1e-6)
        e_p = float(np.abs(out["point_color"][valid] - o["col"][valid]).max())
        assert e_p < PCOL_TOL, e_p
    assert not out["point_color"][~valid].any()
    e_c, e_t = float(np.abs(out["color"] - o["color"]).max()), float(np.abs(out["transmittance"] - o["trans"]).max())
    print(f"uv_render_edges {kind} S={S} {prim} bg={int(with_bg)} split={int(split)}: max|color-oracle| {e_c:.2e} max|T-oracle| {e_t:.2e}")
    assert e_c < POSE_TOL and e_t < T_TOL, (e_c, e_t)
    assert _same_bits(_render(net, cam, rd, U, bg), out)          # a second launch
    return out, o


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("prim", PRIMS)
@pytest.mark.parametrize("S", R.PAIR_S)
def test_pair_totals_and_passes_against_the_oracle(S, prim, split):
    _, o = _against_oracle("paired", S, prim, True, split)
    totals = R.pair_chunk_totals(o["valid"], S)
    assert set(R.PAIR_TARGETS) <= set(totals.reshape(-1).tolist()), totals


@pytest.mark.parametrize("with_bg", [False, True])
@pytest.mark.parametrize("S", R.GEOMETRY_S)
@pytest.mark.parametrize("kind", R.GEOMETRY_KINDS)
def test_geometry_kinds_against_the_oracle(kind, S, with_bg):
    prim = PRIMS[GEOMETRY_MODEL[kind]]
    out, o = _against_oracle(kind, S, prim, with_bg, False)
    cam, rd, _, bg, _ = _oracle_case(kind, S, prim, with_bg)
    n = o["valid"].sum(-1)
    assert rd.shape[0] * rd.shape[1] >= 4
    if kind == "miss":
        # no in-cube sample: T = (1 + 1e-10f)^S = 1 in float32 and the pixel is the tone-mapped background, the same expression in numpy
        # (2 ulp for powf)
        none = n == 0
        assert none.sum() >= 4 and (n > 0).sum() >= 4 and (~R.slab_hits(cam, rd)[none]).sum() >= 4
        f = np.float32
        back = np.zeros(3, f) if bg is None else bg[0] * f(1.0)
        want = np.clip(np.power(back * f(1.0) + f(1e-5), f(1.0 / 2.2)), f(0.0), f(1.0))
        assert want.dtype == f and (out["transmittance"][none] == 1.0).all()
        assert (np.abs(out["color"][none] - want) <= 2 * np.spacing(want)).all(), (out["color"][none], want)
    if kind == "diagonal":
        totals = R.pair_chunk_totals(o["valid"], S)
        assert o["valid"].all() and (totals[:, :S // R.CHUNK] == 128).all()
        pairs = rd.shape[1] // 2
        assert out["stats"][1] == pairs * (8 * (S // R.CHUNK) + -(-2 * (S % R.CHUNK) // R.TILE))          # 8 passes per pair and full chunk
    if kind == "graze":
        assert (n == 0).any() and ((n >= 1) & (n <= 4)).any()
    if kind == "inside":
        assert (np.abs(cam) < 1).all() and (n > 0).all()
    if kind == "axis":
        assert ((rd == 0).sum(-1) >= 1).all() and (n[0] == S).any() and (n[0] == 0).any() and (n[1] > 0).all()


# ---- (d) bit identities at the new shapes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", ["paired", "graze"])
@pytest.mark.parametrize("S", [1, 65, 128])
def test_one_ray_per_wave_gives_the_bits_of_two(S, batch):
    cam, rd, U = R.paired_rays(S, R.pair_targets(S, 19)) if batch == "paired" else R.geometry_rays("graze", S)
    net = _net("sphere")
    for n in (1, 2, 37):
        two = _render(net, cam, rd[:, :n].copy(), U[:, :n].copy(), debug=True)
        with _lib.knobs(uv_tiles=1):
            one = _render(net, cam, rd[:, :n].copy(), U[:, :n].copy(), debug=True)
        assert _same_bits(one, two, ("color", "transmittance", "sigma", "point_color")), n
    assert (two["sigma"] != 0).any() or (batch, S) == ("graze", 1)          # (one sample per ray never lands in a chord of a few 1e-2)


def test_a_subset_rendered_alone_keeps_its_bits_at_128_samples():
    S = 128
    cam, rd, U = R.paired_rays(S, R.pair_targets(S))
    net = _net("sphere")
    whole = _render(net, cam, rd, U, BG1, debug=True)
    for idx in (np.arange(1, 24), np.arange(5, rd.shape[1], 3)):          # an odd offset: every ray changes its partner and its slot in the pair
        part = _render(net, cam, rd[:, idx].copy(), U[:, idx].copy(), BG1, debug=True)
        assert _same_bits(part, {k: v[:, idx] for k, v in whole.items()}, ("color", "transmittance", "sigma", "point_color"))


def test_three_cameras_in_one_launch_give_the_bits_of_three_at_65_samples():
    S, n = 65, 11
    parts = [R.pool_rays("sphere", S, R.SEED), R.pool_rays("square", S, R.SEED), R.geometry_rays("inside", S)]
    cam = np.concatenate([p[0] for p in parts])
    rd = np.stack([p[1][0, :n] for p in parts])
    U = np.stack([p[2][0, :n] for p in parts])
    assert n % 2 == 1 and (np.abs(cam[2]) < 1).all() and (np.abs(cam[:2]) > 1).any(-1).all()
    net = _net("sphere")
    out = _render(net, cam, rd, U, BG3, debug=True, stats=True)
    samples = 0
    for c in range(3):
        one = _render(net, cam[c:c + 1], rd[c:c + 1], U[c:c + 1], BG3[c:c + 1], debug=True, stats=True)
        assert _same_bits(one, {k: v[c:c + 1] for k, v in out.items() if k != "stats"}, ("color", "transmittance", "sigma", "point_color")), c
        assert (one["sigma"] != 0).any()
        samples += one["stats"][0]
    assert out["stats"][0] == samples
    assert _same_bits(_render(net, cam, rd, U, BG3), out)


# ---- (e) colour against transmittance through a constant texture -------------------------------------------------------------------------------
@pytest.mark.parametrize("prim", PRIMS)
@pytest.mark.parametrize("S", [64, 65, 200])
def test_a_constant_texture_ties_the_colour_to_the_transmittance(S, prim):
    """Mode 4 of the edit stage makes every sample's colour the texture's: with a constant c0 the pixel before the tone map is c0 sum(w), and
    sum(w) = 1 - T up to S 1e-10 -- the two quantities the march carries from chunk to chunk, with no network between them."""
    c0 = 0.5
    cam, rd, U = R.pool_rays(prim, S, R.SEED)
    net = uvmapping.NeuTex(primitive_type=prim, sample_num=S, device=DEV)
    net.load_params(synth.uvmapping_params(_seed(prim), prim))
    net.set_target_texture(np.full((6, 4, 4, 3) if prim == "sphere" else (4, 4, 3), c0, np.float32), 4)
    out = _render(net, cam, rd, U, None, debug=True)
    net.release()
    valid = out["sigma"] != 0
    assert np.array_equal(valid, R.valid64(cam, rd, U)) and np.abs(out["point_color"][valid] - c0).max() < 1e-6
    c = out["color"].astype(np.float64)
    assert (c < 1).all()
    lin, T = c ** 2.2 - 1e-5, out["transmittance"].astype(np.float64)
    e = float(np.abs(lin / c0 - (1.0 - T)[..., None]).max())
    print(f"uv_render_edges S={S} {prim} constant texture: max|lin / c0 - (1 - T)| {e:.2e}, B(S) {R.bound(S, 1.0):.2e}")
    assert e <= R.bound(S, 1.0) and (T < 0.5).any() and (T == 1).sum() == 3


# ---- (f) argument edges ---------------------------------------------------------------------------------------------------------------------------
def test_no_rays_no_samples_and_split_on_one_tile():
    cam, rd, U = R.pool_rays("sphere", 64, R.SEED)
    net = _net("sphere")
    for N in (1, 3):
        out = _render(net, np.repeat(cam, N, 0), np.zeros((N, 0, 3), np.float32), np.zeros((N, 0, 64), np.float32), BG3[:N], debug=True, stats=True)
        assert out["color"].shape == (N, 0, 3) and out["transmittance"].shape == (N, 0) and out["sigma"].shape == (N, 0, 64)
        assert out["stats"] == (0, 0)          # nothing ran
    with pytest.raises(RuntimeError):
        _render(net, cam, rd, np.zeros((1, rd.shape[1], 0), np.float32))          # S = 0
    net.sample_num = 64
    d, u = torch.from_numpy(rd[0]).to(DEV), torch.from_numpy(U[0]).to(DEV)
    col, tr = torch.empty((rd.shape[1], 3), device=DEV), torch.empty((rd.shape[1],), device=DEV)
    L, st = _lib.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (net.handle(), (C.c_float * 3)(*cam[0].tolist()), d.data_ptr(), None, u.data_ptr())
    assert L.ngf_uv_render(*args, rd.shape[1], 0, col.data_ptr(), tr.data_ptr(), None, None, None, st) != 0
    assert b"n_samples=0" in L.ngf_last_error()
    assert L.ngf_uv_render(*args, 0, 64, col.data_ptr(), tr.data_ptr(), None, None, None, st) == 0          # R = 0: no launch, no error
    split = _net("sphere", True)
    with pytest.raises(RuntimeError):
        with _lib.knobs(uv_tiles=1):
            _render(split, cam, rd, U)
    assert _same_bits(_render(net, cam, rd, U), _render(net, cam, rd, U))          # the handle is whole after the refusals
