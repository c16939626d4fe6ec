"""GPU checks of TriPlane training at the batch edges that tests/test_gpu_train.py and tests/test_gpu_autograd.py never pin down, on the toy
planes of the triplane_r1_gauge fixture (24 x 20 x 18 grid): an exact active count of 0, 1, 15, 16, 17, 31, 32 and 33 (the 16-sample pass of the
colour kernels, the 32-row k-chunk of xty_block), a batch without one valid sample, activation rows in chunks of 64 with 63, 64, 65 and 129 active
samples, speculative rows that the batch fills exactly, ray and sample counts at the edges of the ray kernels (one, two and three rays per
train_prefix_kernel thread), one ray repeated until a colour bin holds 255, 256, 257 and 513 pairs, gauge shifts that leave the planes, the gauge
off, an alpha mask, a saturated colour head, softplus arguments on both sides of ATen's threshold of 20, a small batch after a large one on the
same trainer and engine, and one Adam step on planes of 63, 64, 65 and 130 texels per row.

Both HIP paths run on every case: the autograd path (``field(rays, is_train=True)`` under autograd, MSE, ``backward()``) and ``Trainer.backward``
+ ``Trainer.gradient`` of the fused path, against tests/triplane_train_eager.py in fp64 (the truth) and fp32 (the yardstick) on the same device,
under ``E.check``: three seeds (model and batch); the loss within 1e-5 relative of fp64; rgb_map within max(2e-6, 4 e_torch32); per tensor (and
per channel group of the planes), over the three gradients stacked, e_hip <= max(4 e_torch32, 1e-5) in the 2-norm and, entry-wise relative to the
largest fp64 entry, <= max(k e_torch32, 1e-5) with k = 4; where the fp64 gradient of a tensor is exactly zero on all three seeds the HIP gradient
is exactly zero.  Batches come from E.edge_batch, whose margins make fp32 and fp64 agree on every discrete decision; every case asserts the
builder's exact active count against both engines."""
import ctypes as C

import numpy as np
import pytest
import torch

import triplane_train_eager as E
from ngf_amd import _engine, _lib, optim, train
from ngf_amd.cases import field_for_case
from oracle import train as otrain

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = train.PARAM_NAMES
EDGE = E.edge_cases()
HIP = ("auto", "fused")
L1 = 8e-5
assert tuple(NAMES) == tuple(E.PARAM_NAMES)


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.asarray(a)).to(DEV, dtype)


def _field(b, params=None, geometry=None):
    f = field_for_case(geometry or b["geometry"], params or b["params"], E.toy()[3] if b["masked"] else None, device=DEV)
    f.gauge_start = 0 if b["gauge_on"] else 10          # every batch runs at iteration 0
    f.differentiable = True
    return f


def _release(f):
    _engine.release_engine(f, "_grad_engine")


def _auto(f, b, white):
    """the autograd path -> (rgb_map, loss, gradients, active count of the engine)"""
    f.zero_grad()
    out = f(_t(b["rays"]), is_train=True, white_bg=white, N_samples=b["S"], iteration=0, jitter=_t(b["jitter"]), coin=0.7)
    loss = torch.mean((out["rgb_map"] - _t(b["rgb_train"])) ** 2)
    loss.backward()
    grads = {k: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()) for k, p in f.named_parameters()}
    assert set(grads) == set(NAMES)
    if not b["gauge_on"]:
        assert all(dict(f.named_parameters())[k].grad is None for k in E.GAUGES)          # compute_gauge was not in the graph
    return out["rgb_map"].detach().clone(), float(loss.detach().double()), grads, f._grad_engine.last_active


def _fused(f, b, white, trainer=None, **tk):
    """Trainer.backward + Trainer.gradient -> (None, loss, gradients, active count of the trainer)"""
    tr = trainer or train.Trainer(f, batch_size=len(b["rays"]), max_samples=b["S"], **tk)
    loss = tr.backward(_t(b["rays"]), _t(b["rgb_train"]), b["S"], white_bg=white, iteration=0, jitter=_t(b["jitter"]), coin=0.7, keep_loss=True)
    grads = {k: tr.gradient(k).clone() for k in NAMES}
    out = (None, float(loss), grads, tr.last_active)
    if trainer is None:
        if tr.chunk_samples < 0:
            assert tr.overflows()[0] == 0, tr.overflows()          # the rows hold the batch: nothing is flagged
        tr.release()
    return out


def _eager(b, white, dtype):
    e = E.Eager(b["params"], b["geometry"], dtype, DEV, E.toy()[3] if b["masked"] else None, gauge_start=0 if b["gauge_on"] else 10)
    rgb, loss, grads, aux = e.gradients(_t(b["rays"], dtype), _t(b["rgb_train"], dtype), b["S"], _t(b["jitter"], dtype), white, 0)
    return rgb, loss, grads, int(aux["active"].sum())


def _three(case):
    """the three seeds on both HIP paths, fp32 torch and fp64 torch -> [{run: (rgb_map, loss, gradients, active count)}]"""
    kw, white, tk = EDGE[case]
    res = []
    for seed in E.EDGE_SEEDS:
        b = E.edge_batch(seed, **kw)
        f = _field(b)
        r = {"batch": b, "auto": _auto(f, b, white)}
        r["fused"] = _fused(f, b, white, **tk)
        _release(f)
        r["t32"], r["t64"] = _eager(b, white, torch.float32), _eager(b, white, torch.float64)
        want = int(b["active"].sum())
        for k in ("auto", "fused", "t32", "t64"):
            assert r[k][3] == want, (case, seed, k, r[k][3], want)
        res.append(r)
    return res, white


# a case whose entry-wise k is raised above 4 (16 at most) names its reason here
ENTRY_K = {}


def _run(case):
    res, white = _three(case)
    E.check(res, case, HIP, entry_k=ENTRY_K.get(case, E.ENTRY_K))
    return res, white


def _all_zero(g, names=NAMES):
    return all(bool((g[k] == 0).all()) for k in names)


@pytest.mark.parametrize("bg", ["white", "black"])
def test_no_active_sample(bg):
    res, white = _run(f"active0-{bg}")
    for r in res:
        assert r["auto"][3] == 0 and int(r["batch"]["valid"].sum()) > len(r["batch"]["rays"])
        for p in HIP:
            g = r[p][2]
            assert _all_zero(g, E.COLOUR), p          # no row reaches the colour kernels
            assert all(bool((g[k][:, E.DD:] == 0).all()) for k in E.PLANES), p
            dens = [bool((g[k] != 0).any()) for k in E.PLANES + ("density_decoder.weight", "density_decoder.bias")]
            # black: nothing reaches the pixels.  white: 1 - sum of the weights does, through the density alone
            assert (all(dens) if white else not any(dens)), (p, bg, dens)
        if not white:
            assert bool((r["auto"][0] == 0).all())


@pytest.mark.parametrize("bg", ["white", "black"])
def test_no_valid_sample_at_all(bg):
    res, white = _run(f"novalid-{bg}")
    for r in res:
        assert bool((r["auto"][0] == (1.0 if white else 0.0)).all())          # the background
        assert all(_all_zero(r[p][2]) for p in HIP)
    # a following optimizer_step: finite parameters, the planes moved by the L1 term only
    b = res[0]["batch"]
    f = _field(b)
    tr = train.Trainer(f, batch_size=len(b["rays"]), max_samples=b["S"], L1_reg_weight=L1)
    before = [p.detach().clone() for p in tr.params]
    lrs = list(tr.lr)
    _fused(f, b, white, trainer=tr)
    tr.optimizer_step()
    for k, name in enumerate(NAMES):
        now = tr.params[k].detach()
        assert bool(torch.isfinite(now).all()), name
        if k >= 3:
            assert torch.equal(now, before[k]), name          # a zero gradient: m = v = 0 and a step of 0 / (0 + eps)
            continue
        gk = L1 * torch.sign(before[k]) / before[k].numel()
        _check_adam(name, now, tr.exp_avg[k], tr.exp_avg_sq[k], before[k], gk, lrs[k])
    tr.release()


@pytest.mark.parametrize("active", E.EDGE_ACTIVE)
def test_an_exact_active_count_at_the_edges_of_the_colour_passes_and_the_k_chunk(active):
    _run(f"active{active}")


@pytest.mark.parametrize("active", E.CHUNK_ACTIVE)
def test_activation_rows_in_chunks_of_64(active):
    res, _ = _run(f"chunk{active}")
    assert EDGE[f"chunk{active}"][2] == {"chunk_samples": E.CHUNK}


@pytest.mark.parametrize("case", ["spec-full", "spec-less"])
def test_speculative_rows_that_hold_the_batch_exactly(case):
    _run(case)          # _fused asserts that no overflow is reported


@pytest.mark.parametrize("R,S", E.EDGE_RAYS, ids=[f"{R}x{S}" for R, S in E.EDGE_RAYS])
def test_ray_and_sample_counts_at_the_edges_of_the_ray_kernels(R, S):
    res, _ = _run(f"rays{R}x{S}")
    assert res[0]["auto"][0].shape == (R, 3)


@pytest.mark.parametrize("n", E.EDGE_DUP)
def test_one_ray_repeated_until_a_colour_bin_is_full_and_over(n):
    _run(f"dup{n}")


@pytest.mark.parametrize("case", ["far_gauge", "gauge-off", "mask-on-black", "mask-off-white", "bright", "softplus"])
def test_the_switches_and_the_variants(case):
    res, _ = _run(case)
    if case == "gauge-off":
        assert all(_all_zero(r[p][2], E.GAUGES) for r in res for p in HIP)
    if case == "bright":          # saturated on white; E's docstring: the clamp itself cannot cut a pixel
        assert all(float(r["auto"][0].min()) > 0.9 for r in res)


@pytest.mark.parametrize("path", HIP)
def test_a_small_batch_after_the_largest_one_reads_none_of_its_rows(path):
    """one ray of seven samples (six active rows: the colour kernels' 16-sample pass and the product's 32-row chunk reach past them) after
    2049 x 24: bit for bit the result of a fresh trainer.  (One ray: every gradient entry is then one wave's sum, so the float atomics have no
    order to differ in.)"""
    seed = E.EDGE_SEEDS[0]
    big = E.edge_batch(seed, E.EDGE_S, R=2049)
    small = E.edge_batch(seed, 7, R=1)
    assert int(small["active"].sum()) > 1

    def run(f, b, tr):
        return _auto(f, b, True) if path == "auto" else _fused(f, b, True, trainer=tr)

    def trainer(f, b):
        return train.Trainer(f, batch_size=len(b["rays"]), max_samples=b["S"]) if path == "fused" else None

    f = _field(small)
    tr = trainer(f, small)
    fresh = run(f, small, tr)
    _release(f)
    if tr:
        tr.release()
    f = _field(small)
    tr = trainer(f, big)
    run(f, big, tr)
    after = [run(f, small, tr)]
    run(f, big, tr)
    after.append(run(f, small, tr))
    if path == "auto":
        assert (f._grad_engine.max_rays, f._grad_engine.max_samples) == (2049, E.EDGE_S)
    _release(f)
    if tr:
        tr.release()
    for got in after:
        assert got[3] == fresh[3] == int(small["active"].sum())
        assert got[1] == fresh[1]
        if path == "auto":
            assert torch.equal(got[0], fresh[0])
        assert all(torch.equal(got[2][k], fresh[2][k]) for k in NAMES), [k for k in NAMES if not torch.equal(got[2][k], fresh[2][k])]


# ---- one Adam step, element by element ---------------------------------------------------------------------------------------------------------
# (plane_xy, plane_yz, plane_xz) [H, W] and the gauge planes' [H, W]: rows of 63, 64, 65 and 130 texels, a plane two texels high
ADAM_SIZES = ((((63, 64), (65, 130), (2, 64)), (19, 23)), (((2, 64), (63, 64), (65, 130)), (64, 65)))
ADAM_IDS = ["gauge19x23", "gauge64x65"]


def _adam_case(sizes):
    hw, ghw = sizes
    b = dict(E.edge_batch(E.EDGE_SEEDS[0], E.EDGE_S, R=128))
    b["params"] = E.model_params(500 + ghw[0], "base", hw, ghw)
    return b


def _check_adam(name, now, m, v, before, gk, lr):
    """the tolerances of tests/test_gpu_infoinv_train_edges.py"""
    want, wm, wv = otrain.adam_update(before, gk, torch.zeros_like(gk), torch.zeros_like(gk), 1, lr)
    err = float((now - want).abs().max())
    assert err < 2e-6 * max(1.0, float(before.abs().max())) + 1e-3 * lr, (name, err)
    assert torch.allclose(m, wm, rtol=1e-5, atol=1e-12) and torch.allclose(v, wv, rtol=1e-5, atol=1e-20), name
    assert not torch.equal(now, before), name


def _next_forward_is_that_of_a_fresh_field(f, b):
    """a differentiable forward through the engine whose packed planes the Adam pass wrote, against a field built from the state: the pixels and
    the loss bit for bit; the gradients are sums of float atomics in any order, and equal to 1e-5 of each tensor's largest entry"""
    fresh_f = _field(b, params={k: v.detach().cpu().numpy() for k, v in f.state_dict().items() if k in NAMES})
    got, want = _auto(f, b, True), _auto(fresh_f, b, True)
    assert torch.equal(got[0], want[0]) and got[1] == want[1] and got[3] == want[3]
    for k in NAMES:
        d = float((got[2][k] - want[2][k]).abs().max())
        assert d <= 1e-5 * float(want[2][k].abs().max()), (k, d)
    _release(fresh_f)


@pytest.mark.parametrize("sizes", ADAM_SIZES, ids=ADAM_IDS)
def test_one_fused_adam_step_on_odd_plane_widths_element_by_element(sizes):
    b = _adam_case(sizes)
    f = _field(b)
    assert [tuple(p.shape[2:]) for p in (f.plane_xy, f.plane_yz, f.plane_xz, f.gauge_xy)] == list(sizes[0]) + [sizes[1]]
    tr = train.Trainer(f, batch_size=len(b["rays"]), max_samples=b["S"], L1_reg_weight=L1)
    before = [p.detach().clone() for p in tr.params]
    lrs = list(tr.lr)
    _, _, grads, active = _fused(f, b, True, trainer=tr)
    assert active > 0
    tr.optimizer_step()
    for k, name in enumerate(NAMES):
        gk = grads[name]
        assert bool((gk != 0).any()), name
        if k < 3:
            gk = gk + L1 * torch.sign(before[k]) / before[k].numel()
        _check_adam(name, tr.params[k].detach(), tr.exp_avg[k], tr.exp_avg_sq[k], before[k], gk, lrs[k])
    # the trainer's packed copies are the Adam kernel's: its next backward is that of a trainer built on the updated field
    again = _fused(f, b, True, trainer=tr)
    tr.release()
    want = _fused(f, b, True)
    assert abs(again[1] - want[1]) <= 1e-9 * abs(want[1]) and again[3] == want[3]
    for k in NAMES:
        assert float((again[2][k] - want[2][k]).abs().max()) <= 1e-5 * float(want[2][k].abs().max()), k
    _next_forward_is_that_of_a_fresh_field(f, b)
    _release(f)


@pytest.mark.parametrize("sizes", ADAM_SIZES, ids=ADAM_IDS)
def test_one_library_adam_step_through_the_optimizer_on_odd_plane_widths(sizes):
    b = _adam_case(sizes)
    f = _field(b)
    opt = optim.Adam(f.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99))
    out = f(_t(b["rays"]), is_train=True, white_bg=True, N_samples=b["S"], iteration=0, jitter=_t(b["jitter"]), coin=0.7)
    total = torch.mean((out["rgb_map"] - _t(b["rgb_train"])) ** 2) + L1 * f.density_L1()
    opt.zero_grad()
    total.backward()
    params = dict(f.named_parameters())
    before = {k: p.detach().clone() for k, p in params.items()}
    grads = {k: p.grad.detach().clone() for k, p in params.items()}
    opt.step()
    for k, name in enumerate(NAMES):
        st = opt.state[params[name]]
        assert float(st["step"]) == 1
        _check_adam(name, params[name].detach(), st["exp_avg"], st["exp_avg_sq"], before[name], grads[name], 0.02 if k < 3 else 1e-4 if k < 6 else 1e-3)
    _next_forward_is_that_of_a_fresh_field(f, b)
    _release(f)


@pytest.mark.parametrize("sizes", ADAM_SIZES, ids=ADAM_IDS)
def test_the_single_parameter_adam_entry_point_on_odd_plane_widths(sizes):
    b = _adam_case(sizes)
    f = _field(b)
    tr = train.Trainer(f, batch_size=len(b["rays"]), max_samples=b["S"], L1_reg_weight=L1)
    _, _, grads, _ = _fused(f, b, True, trainer=tr)
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for k, name in enumerate(NAMES):
        before = tr.params[k].detach().clone()
        gk = grads[name] + (L1 * torch.sign(before) / before.numel() if k < 3 else 0.0)
        _lib.check(L.ngf_train_adam(tr._h, k, 1, float(tr.lr[k]), 0.9, 0.99, 1e-8, L1, st))
        _check_adam(name, tr.params[k].detach(), tr.exp_avg[k], tr.exp_avg_sq[k], before, gk, tr.lr[k])
    again = _fused(f, b, True, trainer=tr)
    tr.release()
    want = _fused(f, b, True)
    for k in NAMES:
        assert float((again[2][k] - want[2][k]).abs().max()) <= 1e-5 * float(want[2][k].abs().max()), k
    _release(f)
