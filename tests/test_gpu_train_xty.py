"""The TriPlane trainer's weight-gradient products alone (ngf_debug_train_xty: one launch of xty_all_kernel through the step's own set-up code)
against float64 on the same float32 inputs, at the row counts a batch never pins down: 1, around one and two 32-row k-chunks, around the grid's
cap of G = 2 x CU count workgroups (32 G - 1, 32 G, 32 G + 1: the first chunk of a second lap; 32 G + 33; 64 G + 1: of a third), a device row
count of 0, 1, 17, the launch's own and one above it, and rows that cancel in pairs.  Cases, references and the derived bounds:
tests/train_xty_ref.py.  Every surplus row, every row from min(rows, *rows_dev) on and the pad column of D3 and V are NaN, so a read past the count
or into the pad shows; the outputs start from known contents (the products are added), with sentinels behind every buffer, in columns 0..143
of gW1 and in the rows behind gW3's three."""
import numpy as np
import pytest
import torch

import train_xty_ref as X
from ngf_amd import train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAIL = 64          # sentinel words behind every buffer


def _sentinel(n):
    return torch.full((n,), X.SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def _with_tail(a):
    """the array on the device, TAIL sentinel words behind it -> (view of the array, the whole buffer)"""
    a = np.ascontiguousarray(a, np.float32)
    buf = _sentinel(a.size + TAIL)
    buf[:a.size] = torch.from_numpy(a.reshape(-1)).to(DEV)
    return buf[:a.size].view(*a.shape), buf


def _tail_intact(buf, n):
    return bool((buf[n:].view(torch.int32) == X.SENTINEL).all())


@pytest.mark.parametrize("name", X.names())
def test_the_four_products_against_float64(name):
    G = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    c = next(k for k in X.cases(G) if k["id"] == name)
    d = X.inputs(c)
    m = X.eff_rows(c)
    ops = {k: _with_tail(d[k]) for k in X.OPERANDS}
    # outputs: M and gW2 as they are; gW1 the whole [64][159] tensor, sentinels in columns 0..143; gW3 three rows of a [16][64] sentinel block
    gw1 = _sentinel(64 * 159 + TAIL)
    gw1_v = gw1[:64 * 159].view(64, 159)
    gw1_v[:, 144:] = torch.from_numpy(d["prev_gW1"]).to(DEV)
    gw3 = _sentinel(16 * 64 + TAIL)
    gw3[:3 * 64] = torch.from_numpy(d["prev_gW3"].reshape(-1)).to(DEV)
    M_v, M = _with_tail(d["prev_M"])
    gw2_v, gw2 = _with_tail(d["prev_gW2"])
    rows_dev = None if c["dev"] is None else torch.tensor([c["dev"]], dtype=torch.int32, device=DEV)
    rc = train.debug_xty(rows=c["rows"], rows_dev=rows_dev, d1=ops["D1"][1], d2=ops["D2"][1], d3=ops["D3"][1], f=ops["F"][1], h1=ops["H1"][1],
                         h2=ops["H2"][1], v=ops["V"][1], m=M, gw2=gw2, gw1=gw1, gw3=gw3)
    assert rc == 0
    torch.cuda.synchronize()
    got = {"M": M_v, "gW2": gw2_v, "gW1": gw1_v[:, 144:], "gW3": gw3[:3 * 64].view(3, 64)}
    # nothing but the outputs was written
    for k, (view, buf) in ops.items():
        assert _tail_intact(buf, view.numel()) and torch.equal(view.cpu().view(torch.int32), torch.from_numpy(d[k]).view(torch.int32)), k
    assert _tail_intact(M, 64 * 144) and _tail_intact(gw2, 64 * 64) and _tail_intact(gw1, 64 * 159)
    assert bool((gw1_v[:, :144].contiguous().view(torch.int32) == X.SENTINEL).all()), "gW1 columns 0..143 were written"
    assert bool((gw3[3 * 64:].view(torch.int32) == X.SENTINEL).all()), "memory behind gW3's three rows was written"
    ref = X.reference(c, d)
    for k, (want, bound) in ref.items():
        g = got[k].cpu().double().numpy()
        assert np.isfinite(g).all(), (k, "a NaN row or pad column was read")
        if m == 0:
            assert np.array_equal(got[k].cpu().numpy().view(np.int32), d["prev_" + k].view(np.int32)), (k, "no row: the contents must stay")
            continue
        err = np.abs(g - want)
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"tp_xty {name} {k}: rows {m} depth {X.depth(c)} largest error / bound {worst:.3f}, largest error {float(err.max()):.3e}")
        assert (err <= bound).all(), (k, worst)
