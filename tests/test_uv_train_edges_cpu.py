"""CPU checks behind the UV-Mapping trainer's edge tests (tests/test_gpu_uv_train_gemm.py, tests/test_gpu_uv_train_edges.py): the GEMM case list
covers every listed width and row count, the derived bound can see a defect in every case (a dropped index of the summed dimension, a missing
output row), the batch builder hits its in-cube counts with the margin it promises, and the softplus cases straddle the threshold."""
import numpy as np
import pytest

import ngf_amd  # noqa: F401
import uv_gemm_ref as R
import uv_train_eager as E

CASES = R.cases()


def test_the_gemm_cases_cover_every_listed_value_and_every_row_count_on_a_narrow_and_a_wide_side():
    by = lambda form: [c for c in CASES if c["form"] == form]          # noqa: E731
    fwd, dx, dw = by("fwd"), by("dx"), by("dw")
    assert {(c["in"], c["ld_x"]) for c in fwd} == set(R.FWD_K) and {(c["out"], c["ld_z"]) for c in fwd} == set(R.FWD_N)
    assert {c["act"] for c in fwd} == {0, 1, 2} and {c["rows"] for c in fwd if c["dev"] is None} == set(R.ROWS)
    assert {(c["rows"], c["dev"]) for c in fwd if c["dev"] is not None} == {(R.FWD_DEV[0], d) for d in R.FWD_DEV[1]}
    assert {(c["out"], c["ld_z"]) for c in dx} == set(R.DX_K) and {(c["n_dx"], c["ld_dx"]) for c in dx} == set(R.DX_N)
    assert {(c["act"], c["add"]) for c in dx} == {(a, b) for a in (0, 1, 2) for b in (False, True)}
    assert {c["rows"] for c in dx if c["dev"] is None} == set(R.ROWS)
    assert {(c["out"], c["ld_z"]) for c in dw} == set(R.DW_OUT) and {(c["in"], c["ld_x"]) for c in dw} == set(R.DW_IN)
    assert {c["rows"] for c in dw if c["dev"] is None} == set(R.DW_ROWS)
    assert {(c["rows"], c["dev"]) for c in dw if c["dev"] is not None} == {(R.DW_DEV[0], d) for d in R.DW_DEV[1]}
    sides = {"fwd": lambda c: (c["out"],), "dx": lambda c: (c["out"], c["n_dx"]), "dw": lambda c: (c["out"], c["in"])}
    for form, rows in (("fwd", R.ROWS), ("dx", R.ROWS), ("dw", R.DW_ROWS)):
        for r in rows:
            w = [sides[form](c) for c in by(form) if c["rows"] == r and c["dev"] is None]
            assert any(min(s) <= 3 for s in w) and any(max(s) == 256 for s in w), (form, r)
    assert len({c["id"] for c in CASES}) == len(CASES)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_the_bound_sees_a_dropped_summand_and_a_missing_output_row(c):
    d = R.inputs(c)
    full = R.reference(c, d)
    m = R.eff_rows(c)
    for name, (want, bound) in full.items():
        assert np.isfinite(want).all() and np.isfinite(bound).all() and (bound >= 0).all(), name      # no NaN padding reaches the reference
    if m == 0:
        # nothing is summed and no row exists: the GPU test asserts untouched sentinels (fwd, dx) and exact zeros (dw) instead
        assert all(want.size == 0 or not want.any() for want, _ in full.values())
        return
    short = R.reference(c, d, drop_k=True)
    for name, (want, bound) in full.items():
        assert (np.abs(short[name][0] - want) > bound).any(), (name, "dropping the last summand stays inside the bound")
        assert (np.abs(want[-1]) > bound[-1]).any(), (name, "a missing last output row stays inside the bound")
    assert R.gamma(c["in"] + 4) < 1e-4 and R.gamma(R.CHUNK + 8) < 1e-4          # the bound is tight: a relative 1e-4 at the widest layer


def test_the_inputs_put_half_of_aux_at_or_below_zero_with_exact_zeros():
    for c in CASES:
        if c["form"] == "dx" and c["act"] != R.NONE and R.eff_rows(c) >= 15:
            x = R.inputs(c)["x"][:R.eff_rows(c), :c["n_dx"]]
            assert 0.35 < float((x <= 0).mean()) < 0.65 and (x == 0).any(), c["id"]


@pytest.mark.parametrize("seed", E.EDGE_SEEDS)
def test_the_batch_builder_hits_its_counts_and_keeps_its_margin(seed):
    for V in E.EDGE_V:
        b = E.edge_batch(seed, "square", E.EDGE_V_S, V=V)
        n = b["raydir"].shape[1]
        assert int(b["counts"].sum()) == V and b["margin"] >= E.FACE_MARGIN, V
        assert (b["counts"][0, -3:] == 0).all() and (n * E.EDGE_V_S) % 16 != 0, V
        hit = b["counts"][0][b["counts"][0] > 0]
        assert len(hit) <= -(-V // E.EDGE_V_S) + 2, (V, len(hit))          # the fewest rays: at most two beyond ceil(V / S)
        cnt, mg = E.in_cube_counts(b["campos"][0], b["raydir"][0], b["U"][0])          # from the returned arrays alone
        assert (cnt == b["counts"][0]).all() and float(mg.min()) == b["margin"]
    for Rn in E.EDGE_RAYS:
        b = E.edge_batch(seed, "sphere", E.EDGE_RAYS_S, R=Rn)
        assert b["raydir"].shape == (1, Rn, 3) and b["U"].shape == (1, Rn, E.EDGE_RAYS_S) and b["margin"] >= E.FACE_MARGIN
    n, Rn = E.EDGE_CAMS
    b = E.edge_batch(seed, "square", E.EDGE_RAYS_S, R=Rn, n_cams=n)
    assert b["raydir"].shape == (n, Rn, 3) and b["margin"] >= E.FACE_MARGIN and (b["counts"].sum(1) > 0).all()
    assert np.allclose(b["campos"][2], b["campos"][0] * 1.1, rtol=1e-6) and not np.array_equal(b["raydir"][0], b["raydir"][1])
    for c in range(n):
        cnt, _ = E.in_cube_counts(b["campos"][c], b["raydir"][c], b["U"][c])
        assert (cnt == b["counts"][c]).all()


def test_an_unfiltered_pool_has_samples_closer_to_a_face_than_the_margin():
    _, _, _, _, mg, order = E._pool(E.EDGE_SEEDS[0], E.EDGE_V_S, 0)
    assert float(mg.min()) < E.FACE_MARGIN and len(order) > 4000          # the filter is needed, and it leaves plenty of rays


@pytest.mark.parametrize("seed", E.EDGE_SEEDS)
@pytest.mark.parametrize("which", ["density", "color1"])
def test_the_softplus_cases_straddle_the_threshold(which, seed):
    _, _, s = E.softplus_case(seed, which)
    assert 0.1 <= s["above"] <= 0.9 and s["gap"] > 1e-4 and s["in_cube"] > 100, s
    if which == "color1":
        assert s["unclamped"] >= 0.5, s
