"""The InfoInv trainer's weight-gradient products alone (ngf_debug_ii_product: ii_mm_kernel + ii_mm_reduce_kernel of the fused step and
ii_xty_kernel + ii_xty_reduce_kernel of the autograd path, through the trainer's own launch code) against numpy float64 on the same fp32 inputs:
the trainer's six shapes at row counts around the 32-row k-step, the 64-row stage, the 1024-row fp32-to-fp64 hand-over and the 4096- and
8192-row chunks, and a device row count of 0, 1, inside a k-step, at, and above the launch (tests/ii_product_ref.py: cases, references and the
derived bounds; tests/test_infoinv_train_edges_cpu.py shows on the CPU that the bound sees a dropped row or column in every case).

Every output word holds a sentinel before the call, with sentinel tails behind each buffer, and the chunk scratch holds NaN: a reduce that reads a
partial nobody wrote shows as NaN, and so does a load past the row count (surplus rows and the padding up to ld are NaN).  Every case of the
MFMA form runs a second time with accumulate = 1 on top of known contents."""
import numpy as np
import pytest
import torch

import ii_product_ref as R
from ngf_amd import _lib, infoinv_train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = R.cases()
FORM = {"mfma": infoinv_train.PRODUCT_MFMA, "fp64": infoinv_train.PRODUCT_FP64}
TAIL = 64          # sentinel words behind gw, gb and gw64


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _buffers(c, d, accumulate):
    """gw, gb (int32 words) and gw64 (int64 words): sentinels, or the known contents with a sentinel tail"""
    M, N = c["M"], c["N"]
    out = {"gw": torch.full((M * N + TAIL,), R.SENTINEL, dtype=torch.int32, device=DEV),
           "gb": torch.full((M + TAIL,), R.SENTINEL, dtype=torch.int32, device=DEV),
           "gw64": torch.full((M * N + TAIL,), R.SENTINEL64, dtype=torch.int64, device=DEV)}
    if accumulate:
        out["gw"][:M * N] = _dev(d["prev_gw"].reshape(-1).view(np.int32))
        out["gb"][:M] = _dev(d["prev_gb"].view(np.int32))
        out["gw64"][:M * N] = _dev(d["prev_gw64"].reshape(-1).view(np.int64))
    return out


def _run(c, d, accumulate=False, skip=()):
    """-> {name: the whole output buffer's words} after one call; `skip`: outputs passed as NULL"""
    x, y = _dev(d["x"]), _dev(d["y"])
    pe, pbe = R.scratch_elems(c)
    part = torch.full((pe,), float("nan"), dtype=torch.float64, device=DEV)
    kw = dict(m=c["M"], n=c["N"], rows=c["rows"], ld=c["ld"], x=x, y=y, part=part, accumulate=int(accumulate))
    if pbe:
        kw["partb"] = torch.full((pbe,), float("nan"), dtype=torch.float64, device=DEV)
    if c["dev"] is not None:
        kw["rows_dev"] = torch.tensor([c["dev"]], dtype=torch.int32, device=DEV)
    out = _buffers(c, d, accumulate)
    kw.update({k: v for k, v in out.items() if k not in skip})
    _lib.check(infoinv_train.debug_product(FORM[c["form"]], **kw))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(c, d, words, accumulate, skip=()):
    """values within the bound, sentinels outside the computed region and none inside -> the largest error / bound"""
    ref = R.reference(c, d, accumulate=accumulate)
    m, worst = R.eff_rows(c), 0.0
    for name, (want, bound) in ref.items():
        sent, ftype = (R.SENTINEL64, np.float64) if name == "gw64" else (R.SENTINEL, np.float32)
        n = want.size
        body, rest = words[name][:n].reshape(want.shape), words[name][n:]
        assert (rest == sent).all(), (name, "a word behind the output was written", int((rest != sent).sum()))
        if name in skip:
            assert (body == sent).all(), (name, "an output passed as NULL was written")
            continue
        assert not (body == sent).any(), (name, "a word of the output was not written")
        if m == 0:          # no rows: exactly +0, or the contents bit for bit
            prev = d["prev_" + name].reshape(want.shape).view(body.dtype) if accumulate else np.zeros_like(body)
            assert np.array_equal(body, prev), name
        got = body.view(ftype).astype(np.float64)
        err = np.abs(got - want)
        bad = np.argwhere(~(err <= bound))
        assert not len(bad), (name, len(bad), [(tuple(i), float(got[tuple(i)]), float(want[tuple(i)]), float(bound[tuple(i)])) for i in bad[:4]])
        if (bound > 0).any():
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    return worst


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_product_is_within_the_derived_bound_of_fp64_and_writes_nothing_else(c):
    d = R.inputs(c)
    worst = _check(c, d, _run(c, d), False)
    line = f"ii_product {c['id']}: largest error / bound = {worst:.3f}"
    if c["form"] == "mfma":
        worst = _check(c, d, _run(c, d, accumulate=True), True)
        line += f", accumulate {worst:.3f}"
    print(line)


@pytest.mark.parametrize("form", R.FORMS)
def test_null_outputs_are_skipped(form):
    c = next(k for k in CASES if k["form"] == form and (k["M"], k["N"], k["rows"]) == (64, 231, 4097))
    d = R.inputs(c)
    for skip in (("gw",), ("gb", "gw64"), ("gw64",)):
        _check(c, d, _run(c, d, skip=skip), False, skip=skip)


def test_the_entry_refuses_scratch_that_is_too_small_and_bad_shapes():
    err = lambda: _lib.lib().ngf_last_error()          # noqa: E731
    for form in R.FORMS:
        c = next(k for k in CASES if k["form"] == form and (k["M"], k["N"], k["rows"]) == (64, 231, 8193))
        d = R.inputs(c)
        x, y = _dev(d["x"]), _dev(d["y"])
        pe, pbe = R.scratch_elems(c)
        part = torch.full((pe,), float("nan"), dtype=torch.float64, device=DEV)
        partb = torch.full((max(pbe, 1),), float("nan"), dtype=torch.float64, device=DEV)
        out = _buffers(c, d, False)
        kw = dict(m=c["M"], n=c["N"], rows=c["rows"], ld=c["ld"], x=x, y=y, part=part, partb=partb, **out)
        call = lambda **over: infoinv_train.debug_product(FORM[form], **dict(kw, **over))          # noqa: E731
        assert call(part=part[:pe - 1]) == 1 and b"too small" in err()
        if form == "mfma":
            assert call(partb=partb[:pbe - 1]) == 1 and b"too small" in err()
            assert infoinv_train.debug_product(FORM[form], **{k: v for k, v in kw.items() if k != "partb"}) == 1
        else:
            assert call(accumulate=1) == 1
        assert call(m=65) == 1 and call(m=0) == 1 and call(n=232) == 1 and call(n=0) == 1
        assert call(rows=0) == 1 and call(rows=-5) == 1 and call(rows=1 << 31) == 1 and call(ld=c["rows"] - 1) == 1
        assert call(x=None) == 1 and call(y=None) == 1 and call(part=None) == 1
        assert infoinv_train.debug_product(7, **kw) == 1 and b"unknown form" in err()
        torch.cuda.synchronize()
        for k, v in out.items():
            assert (v.cpu().numpy() == (R.SENTINEL64 if k == "gw64" else R.SENTINEL)).all(), (form, k)
        assert call() == 0          # and the same arguments, unchanged, run
        torch.cuda.synchronize()
