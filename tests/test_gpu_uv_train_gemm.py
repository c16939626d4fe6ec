"""The UV-Mapping trainer's layer GEMM alone (ngf_debug_uvt_gemm: uvt_gemm_kernel and uvt_reduce_kernel through the trainer's own launch code)
against numpy float64 on the same fp32 inputs, at the network's widths and the smallest row counts that reach each branch: ragged 16- and
64-row tiles, a device row count below, at and above the launch, and 1024-row split-K chunk edges (tests/uv_gemm_ref.py: cases, references and
the derived bound; tests/test_uv_train_edges_cpu.py shows on the CPU that the bound sees a dropped index or row in every case).

Every output word holds a sentinel before the call, and the split-K scratch holds NaN: rows from min(rows, device rows) on and columns from N
to the leading dimension must keep their bits, and a reduce that reads a chunk nobody wrote shows as NaN.  Padding columns and surplus rows
of the inputs are NaN too."""
import numpy as np
import pytest
import torch

import uv_gemm_ref as R
from ngf_amd import _lib, uv_train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = R.cases()
FORM = {"fwd": uv_train.GEMM_FORWARD, "dx": uv_train.GEMM_DX, "dw": uv_train.GEMM_DW}
TAIL = 64          # sentinel words behind gw and gb


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sentinel(n):
    return torch.full((n,), R.SENTINEL, dtype=torch.int32, device=DEV)


def _run(c):
    """-> {name: int32 bits of the whole output buffer} after one call."""
    d = {k: _dev(v) for k, v in R.inputs(c).items()}
    rows = c["rows"]
    kw = {"in_": c["in"], "out": c["out"], "rows": rows, "w": d["w"]}
    if c["dev"] is not None:
        d["rows_dev"] = torch.tensor([c["dev"]], dtype=torch.int32, device=DEV)
        kw["rows_dev"] = d["rows_dev"]
    out = {}
    if c["form"] == "fwd":
        out["z"] = _sentinel(rows * c["ld_z"])
        kw.update(x=d["x"], ld_x=c["ld_x"], b=d["b"], z=out["z"], ld_z=c["ld_z"], act=c["act"])
    elif c["form"] == "dx":
        out["dx"] = _sentinel(rows * c["ld_dx"])
        kw.update(z=d["dz"], ld_z=c["ld_z"], dx=out["dx"], ld_dx=c["ld_dx"], n_dx=c["n_dx"], act=c["act"])
        if c["act"] != R.NONE:
            kw.update(x=d["x"], ld_x=c["ld_x"])
        if c["add"]:
            kw.update(add=d["add"], ld_add=c["ld_dx"])
    else:
        nz = R.n_chunks(rows)
        out["gw"], out["gb"] = _sentinel(c["out"] * c["in"] + TAIL), _sentinel(c["out"] + TAIL)
        d["part"] = torch.full((nz * c["out"] * c["in"],), float("nan"), device=DEV)
        d["partb"] = torch.full((nz * c["out"],), float("nan"), device=DEV)
        kw.update(x=d["x"], ld_x=c["ld_x"], z=d["dz"], ld_z=c["ld_z"], part=d["part"], partb=d["partb"], gw=out["gw"], gb=out["gb"])
    _lib.check(uv_train.debug_gemm(FORM[c["form"]], **kw))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_layer_gemm_is_within_the_derived_bound_of_fp64_and_writes_nothing_else(c):
    bits = _run(c)
    ref = R.reference(c, R.inputs(c))
    m = R.eff_rows(c)
    worst = 0.0
    for name, (want, bound) in ref.items():
        if c["form"] == "dw":
            n = want.size
            body, rest = bits[name][:n].reshape(want.shape), bits[name][n:]
        else:
            ld, cols = (c["ld_z"], c["out"]) if c["form"] == "fwd" else (c["ld_dx"], c["n_dx"])
            whole = bits[name].reshape(c["rows"], ld)
            body, rest = whole[:m, :cols], np.concatenate([whole[:m, cols:].reshape(-1), whole[m:].reshape(-1)])
        assert (rest == R.SENTINEL).all(), (name, "a word outside the computed region was written", int((rest != R.SENTINEL).sum()))
        assert not (body == R.SENTINEL).any(), (name, "a word of the computed region was not written")
        got = body.view(np.float32).astype(np.float64)
        if c["form"] == "dw" and m == 0:
            assert (body == 0).all(), name          # no rows: exactly +0
        err = np.abs(got - want)
        bad = np.argwhere(~(err <= bound))
        assert not len(bad), (name, len(bad), [(tuple(i), float(got[tuple(i)]), float(want[tuple(i)]), float(bound[tuple(i)])) for i in bad[:4]])
        if want.size and (bound > 0).any():
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    print(f"uvt_gemm {c['id']}: largest error / bound = {worst:.3f}")


def test_the_entry_refuses_scratch_that_is_too_small_and_bad_shapes():
    c = dict(CASES[-1], dev=None)
    d = {k: _dev(v) for k, v in R.inputs(c).items()}
    gw, gb = _sentinel(c["out"] * c["in"]), _sentinel(c["out"])
    nz = R.n_chunks(c["rows"])
    part, partb = torch.empty((nz - 1) * c["out"] * c["in"], device=DEV), torch.empty(nz * c["out"], device=DEV)
    kw = dict(in_=c["in"], out=c["out"], rows=c["rows"], w=d["w"], x=d["x"], ld_x=c["ld_x"], z=d["dz"], ld_z=c["ld_z"], gw=gw, gb=gb)
    assert uv_train.debug_gemm(uv_train.GEMM_DW, part=part, partb=partb, **kw) == 1
    assert b"chunks" in _lib.lib().ngf_last_error()
    assert uv_train.debug_gemm(uv_train.GEMM_DW, part=part, partb=partb, **dict(kw, ld_z=c["out"] - 1)) == 1
    assert uv_train.debug_gemm(7, **kw) == 1
    torch.cuda.synchronize()
    assert (gw.cpu().numpy() == R.SENTINEL).all() and (gb.cpu().numpy() == R.SENTINEL).all()
