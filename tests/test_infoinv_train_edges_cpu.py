"""CPU checks behind the InfoInv trainers' edge tests (tests/test_gpu_ii_product.py, tests/test_gpu_infoinv_train_edges.py): the product case
list covers every listed shape and row count, the derived bounds can see a defect in every case (a dropped last row of the sum, a missing last
output row or column), the torch restatement reproduces what the reference module produced (tests/golden/infoinv_train_*.npz) and agrees with
the eager port, and the batch builder hits its counts with the margins it promises, so that fp32 and fp64 agree on the valid and the active
set of every batch the GPU file uses."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ngf_amd  # noqa: E402,F401
import ii_product_ref as R  # noqa: E402
import infoinv_train_eager as E  # noqa: E402
from test_gpu_infoinv_train import CASES as FIXTURES, GRAD_TOL, _EagerInfoInv, load, rel  # noqa: E402

CASES = R.cases()
EDGE = E.edge_cases()


def test_the_product_cases_cover_every_shape_and_every_row_count_on_a_narrow_and_the_widest_product():
    for form in R.FORMS:
        mine = [c for c in CASES if c["form"] == form]
        assert {(c["M"], c["N"]) for c in mine} == set(R.SHAPES)
        assert {c["rows"] for c in mine if c["dev"] is None} == set(R.ROWS)
        assert {(c["rows"], c["dev"]) for c in mine if c["dev"] is not None} == {(R.DEV[0], d) for d in R.DEV[1]}
        for r in R.ROWS:
            shapes = [(c["M"], c["N"]) for c in mine if c["rows"] == r and c["dev"] is None]
            assert any(s[0] in (1, 3) for s in shapes) and R.WIDE in shapes, (form, r)
        assert all(c["ld"] == c["rows"] + 3 for c in mine)
    assert len({c["id"] for c in CASES}) == len(CASES)
    # the row counts sit on both sides of every edge of the two kernels
    for edge in (R.MM_K, R.XTY_STAGE, R.MM_SUB, R.XTY_CHUNK, R.MM_CHUNK):
        assert {edge - 1, edge, edge + 1} <= set(R.ROWS), edge
    assert R.DEV[0] == R.MM_CHUNK + 1 and 33 % R.MM_K and max(R.DEV[1]) > R.DEV[0] and 2 * R.MM_CHUNK + 1 in R.ROWS


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_the_bound_sees_a_dropped_row_and_a_missing_output_row_or_column(c):
    d = R.inputs(c)
    m = R.eff_rows(c)
    assert np.isnan(d["x"][:, m:]).all() and np.isnan(d["y"][:, m:]).all() and np.isfinite(d["x"][:, :m]).all()
    for acc in ((False, True) if c["form"] == "mfma" else (False,)):
        full = R.reference(c, d, accumulate=acc)
        for name, (want, bound) in full.items():
            assert np.isfinite(want).all() and np.isfinite(bound).all() and (bound >= 0).all(), name          # no NaN padding reaches the reference
        if m == 0:
            # nothing is summed: the GPU test asserts exact zeros, or the previous contents bit for bit
            assert all(np.array_equal(want, d["prev_" + k].astype(np.float64) if acc else np.zeros_like(want)) for k, (want, _) in full.items())
            continue
        short = R.reference(c, d, drop_row=True, accumulate=acc)
        for name, (want, bound) in full.items():
            assert (np.abs(short[name][0] - want) > bound).any(), (name, acc, "dropping the last row of the sum stays inside the bound")
            if not acc:          # an output that was never written: against zero (under accumulate the sentinel-free check is the value itself)
                assert (np.abs(want[-1]) > bound[-1]).any(), (name, "a missing last output row stays inside the bound")
                if want.ndim == 2:
                    assert (np.abs(want[:, -1]) > bound[:, -1]).any(), (name, "a missing last output column stays inside the bound")
            else:
                prev = d["prev_" + name].astype(np.float64)
                assert (np.abs(prev[-1] - want[-1]) > bound[-1]).any(), (name, "an output row that kept its contents stays inside the bound")
    assert R.gamma(R.MM_SUB + 4) < 6.2e-5          # the bound is tight: a relative 6e-5 of sum |x| |y| at the longest fp32 sub-sum


@pytest.mark.parametrize("case", FIXTURES)
def test_the_restatement_reproduces_the_reference_modules_pixels_and_gradients(case):
    """the tolerances tests/test_gpu_infoinv_train.py applies to the same arrays"""
    g, params, mask = load(case)
    t = torch.from_numpy
    white = bool(int(g["white_bg"])) or float(g["coin"]) < 0.5
    e = E.Eager(params, g, torch.float32, "cpu", mask)
    rgb, loss, grads, aux = e.gradients(t(g["rays"]), t(g["rgb_train"]), int(g["S"]), t(g["jitter0"]), white, bool(int(g["infoinv"])))
    np.testing.assert_allclose(rgb.numpy(), g["rgb_map0"], rtol=1e-4, atol=2e-6)
    assert abs(loss - float(g["rgb_loss0"])) < 2e-6
    for name in E.PARAM_NAMES:
        assert rel(grads[name].numpy(), g[f"grad_rgb0.{name}"]) < GRAD_TOL, name
    assert int(aux["active"].sum()) > 100 and int(aux["valid"].sum()) > int(aux["active"].sum())


@pytest.mark.parametrize("infoinv,white,masked", [(True, False, True), (False, True, True), (True, True, False)])
def test_the_restatement_agrees_with_the_eager_port_and_its_fp64_run_differs_by_rounding(infoinv, white, masked):
    g, _, mask = E.toy()
    mask = mask if masked else None
    b = E.edge_batch(E.EDGE_SEEDS[0], E.EDGE_S, infoinv=infoinv, masked=masked, R=128)
    t = torch.from_numpy
    from ngf_amd import geometry
    port = _EagerInfoInv(b["params"], g, geometry.step_size(g["aabb"], g["grid"], 0.5), infoinv)
    if masked:
        vol = np.unpackbits(mask[0])[:int(np.prod(mask[1]))].reshape(mask[1]).astype(np.float32)
        maabb = torch.as_tensor(mask[2], dtype=torch.float32)
        port.mask = (torch.as_tensor(vol)[None, None], maabb, 1.0 / (maabb[1] - maabb[0]) * 2)
    rgb_p, aux_p = port.forward_train(t(b["rays"]), E.EDGE_S, t(b["jitter"]), white, 0)
    torch.mean((rgb_p - t(b["rgb_train"])) ** 2).backward()
    res = {}
    for dt in (torch.float32, torch.float64):
        e = E.Eager(b["params"], g, dt, "cpu", mask)
        res[dt] = e.gradients(t(b["rays"]).to(dt), t(b["rgb_train"]).to(dt), E.EDGE_S, t(b["jitter"]).to(dt), white, infoinv)
    rgb32, _, g32, aux32 = res[torch.float32]
    rgb64, _, g64, aux64 = res[torch.float64]
    # the same operators in the same order: the port and the fp32 restatement agree to the last bits
    assert torch.equal(aux32["active"], aux_p["active"]) and float((rgb32 - rgb_p.detach()).abs().max()) <= 1e-6
    for name in E.PARAM_NAMES:
        assert rel(g32[name].numpy(), port.p[name].grad.numpy()) <= 1e-5, name
    # fp64: the same sets (the batch keeps its margins), pixels within a few fp32 roundings, gradients within the fixtures' tolerance, not equal
    assert torch.equal(aux32["valid"], aux64["valid"]) and torch.equal(aux32["active"], aux64["active"])
    assert int(aux64["valid"].sum()) == int(b["valid"].sum()) and int(aux64["active"].sum()) == int(b["active"].sum())
    assert 0 < float((rgb32.double() - rgb64).abs().max()) < 2e-6
    # A gradient entry is a sum over the n samples that reach the tensor, of terms that each went through sums of up to 231 products: fp32
    # leaves it within gamma_k sum |terms| with k below 1024 (231 + 64 + 64 + the samples of a ray + a few hundred samples per texel or
    # weight), and a sum of n terms of either sign is about sqrt(n) times smaller than the sum of their magnitudes
    tol = R.gamma(1024) * float(np.sqrt(int(aux64["valid"].sum())))
    assert tol < 3e-3
    for name in E.PARAM_NAMES:
        r = rel(g32[name].double().numpy(), g64[name].numpy())
        assert 0 < r < tol, (name, r, tol)


def _sets(b, dtype):
    g, _, mask = E.toy()
    return E.facts(b["params"], dict(g, **b.get("geometry", {})), mask if b["masked"] else None, b["rays"], b["jitter"], b["S"], b["infoinv"], dtype)


def _check_batch(b, label):
    f64, f32 = _sets(b, torch.float64), _sets(b, torch.float32)
    assert np.array_equal(f64["valid_set"], f32["valid_set"]) and np.array_equal(f64["active_set"], f32["active_set"]), label
    assert np.array_equal(f64["valid"], b["valid"]) and np.array_equal(f64["active"], b["active"]), label
    face, weight, cell = b["margin"]
    assert face >= E.FACE_MARGIN and weight >= E.WEIGHT_MARGIN and cell >= E.CELL_MARGIN, (label, b["margin"])
    assert b["rays"].dtype == np.float32 and b["jitter"].shape == (len(b["rays"]),) and b["rgb_train"].shape == (len(b["rays"]), 3)


@pytest.mark.parametrize("seed", E.EDGE_SEEDS)
@pytest.mark.parametrize("case", list(EDGE))
def test_every_edge_batch_has_its_counts_and_fp32_and_fp64_agree_on_both_sets(case, seed):
    kw, _ = EDGE[case]
    b = E.edge_batch(seed, **kw)
    _check_batch(b, (case, seed))
    n, S = len(b["rays"]), kw["S"]
    if "active" in kw:
        assert int(b["active"].sum()) == kw["active"] and (b["valid"][-3:] == 0).all()
        if kw["active"] == 0:
            assert n == kw["R"] + 3 and int(b["valid"].sum()) > n          # a density the pixels see, below the threshold everywhere
    elif kw.get("no_valid"):
        assert n == kw["R"] and int(b["valid"].sum()) == 0 and int(b["active"].sum()) == 0
    else:
        assert n == kw["R"] and (n == 1 or 0 < int(b["active"].sum()) < int(b["valid"].sum()) < n * S)
    if case.startswith("mask"):
        bare = E.facts(b["params"], E.toy()[0], None, b["rays"], b["jitter"], S, b["infoinv"])
        assert int(bare["valid"].sum()) > int(b["valid"].sum()) and np.isfinite(b["margin"][2])          # the mask removes samples


def test_the_ray_cases_reach_the_edges_they_are_there_for():
    pairs = {R_ * S for R_, S in E.EDGE_RAYS}
    assert any(R.XTY_CHUNK < p < R.XTY_CHUNK + R.XTY_STAGE for p in pairs) and any(R.MM_CHUNK < p < R.MM_CHUNK + R.MM_K for p in pairs)
    rays = {R_ for R_, _ in E.EDGE_RAYS}
    assert 1 in rays and any(1024 < r <= 2048 for r in rays) and any(2048 < r <= 3072 for r in rays) and all(r % 256 for r in rays)
    assert min(S for _, S in E.EDGE_RAYS) == 7 and max(S for _, S in E.EDGE_RAYS) == 45
    # the pool holds rays with a zero direction component, rays that miss the box, and rays that start inside it
    rays_, _, f, order = E._pool(E.EDGE_SEEDS[0], E.EDGE_S, True, False, "base")
    use = rays_[order]
    assert (use[:, 3:] == 0).any(1).sum() > 50 and (f["valid"][order] == 0).sum() > 100
    assert (np.abs(use[:, :3]) < 1.5).all(1).sum() > 50


def test_an_unfiltered_pool_has_samples_inside_every_margin():
    rays, _, f, order = E._pool(E.EDGE_SEEDS[0], E.EDGE_S, True, True, "base")
    assert len(order) < len(rays) and len(order) > 4000          # the filter is needed, and it leaves plenty of rays
    assert f["weight"].min() < E.WEIGHT_MARGIN and f["cell"].min() < E.CELL_MARGIN


@pytest.mark.parametrize("seed", E.EDGE_SEEDS)
def test_the_softplus_case_straddles_the_threshold_with_alpha_away_from_zero_and_one(seed):
    params, g, b, s = E.softplus_case(seed)
    assert 0.1 <= s["above"] <= 0.9 and s["gap"] > 1e-4 and s["valid"] > 500 and s["active"] > 100, s
    assert 0.005 < s["alpha"][0] and s["alpha"][1] < 0.9, s
    b = dict(b, geometry={"distance_scale": g["distance_scale"]})
    _check_batch(b, ("softplus", seed))
    # fp32 takes the same branch of softplus on every sample
    u32, u64 = _sets(b, torch.float32)["u"], _sets(b, torch.float64)["u"]
    assert np.array_equal(u32 > 20, u64 > 20)
    # without the scaling no argument comes near the threshold from below: the branch would never run otherwise ... or always
    base = E.facts(E.model_params(seed), E.toy()[0], None, b["rays"], b["jitter"], b["S"], True)["u"]
    assert ((base > 20).mean() < 0.1) or ((base > 20).mean() > 0.9)


def test_the_subset_sum_names_every_ray_once():
    counts = np.array([3, 5, 5, 2, 7, 1, 4, 0, 6], np.int64)
    for target in range(1, int(counts.sum()) + 1):
        pick = E._subset(counts, np.arange(len(counts)), target)
        assert len(set(pick)) == len(pick) and int(counts[pick].sum()) == target
