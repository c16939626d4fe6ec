"""CPU checks of the NeuTex occupancy grid (include/ngf.h: ngf_uv_occupancy_*; neural-gauge-fields_amd/uvmapping.py): properties of the numpy
restatements in tests/uv_occupancy_ref.py that tests/test_gpu_uv_occupancy.py holds the kernels to, the argument checks of the four entry points
(all made before any GPU work), the host-side validation of the Python surface, and the condition the render test's batches must meet -- nearly
every in-cube sample keeps 1e-5 from the cell boundaries, and float32 and float64 agree on the cell of every sample that does."""
import ctypes as C

import numpy as np
import pytest

import uv_occupancy_ref as O
from ngf_amd import _lib, uvmapping

E_ARG = 1
F = np.float32


# ---- the restatements ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", O.REDUCE_SHAPES)
def test_dilation_grows_the_mask(shape):
    sigma = np.random.default_rng(5).standard_normal(tuple(n + 1 for n in shape)).astype(F)
    thr = float(np.quantile(sigma, 0.97))
    m = [O.dilate_cells(O.hot_cells(sigma, thr), d) for d in (0, 1, 2)]
    assert m[0].any() or shape == (1, 1, 1)
    assert (m[0] <= m[1]).all() and (m[1] <= m[2]).all()
    if min(shape) >= 7:
        assert m[0].sum() < m[1].sum() < m[2].sum()


@pytest.mark.parametrize("corner", [(0, 0, 0), (9, 8, 7), (4, 0, 7), (9, 3, 0), (3, 4, 5)])          # grid corners, edges, the interior
def test_a_single_hot_corner_lights_exactly_the_cells_that_share_it(corner):
    shape = (9, 8, 7)
    sigma = np.zeros(tuple(n + 1 for n in shape), F)
    sigma[corner] = 1.0
    hot = O.hot_cells(sigma, 0.5)
    want = np.zeros(shape, bool)
    sl = tuple(slice(max(c - 1, 0), min(c, n - 1) + 1) for c, n in zip(corner, shape))
    want[sl] = True
    assert np.array_equal(hot, want) and hot.sum() == np.prod([s.stop - s.start for s in sl])
    for d in (1, 2):
        grown = np.zeros(shape, bool)
        grown[tuple(slice(max(s.start - d, 0), min(s.stop + d, n)) for s, n in zip(sl, shape))] = True
        assert np.array_equal(O.dilate_cells(hot, d), grown)


def test_a_nan_corner_makes_its_cells_hot_and_infinities_compare():
    shape = (4, 4, 4)
    sigma = np.zeros((5, 5, 5), F)
    sigma[2, 2, 2] = np.nan
    hot = O.hot_cells(sigma, 1e30)
    assert hot.sum() == 8 and hot[1:3, 1:3, 1:3].all()
    sigma[:] = -np.inf
    assert not O.hot_cells(sigma, -1e30).any()
    sigma[0, 0, 0] = np.inf
    assert O.hot_cells(sigma, 1e30).sum() == 1 and O.hot_cells(sigma, 1e30)[0, 0, 0]
    assert O.unpack(O.from_lattice(sigma, 1e30, 0), shape).sum() == 1


@pytest.mark.parametrize("shape", O.LOOKUP_SHAPES)
def test_bit_order_is_packbits_and_tail_bits_are_zero(shape):
    vol = O.random_mask(shape)
    bits = O.pack(vol)
    n = int(np.prod(shape))
    assert bits.dtype == np.uint8 and bits.shape == ((n + 7) // 8,)
    assert np.array_equal(bits, np.packbits(vol.reshape(-1)))
    if n % 8:
        assert int(bits[-1]) & ((1 << (8 - n % 8)) - 1) == 0
    assert np.array_equal(O.unpack(bits, shape), vol)
    flat = vol.reshape(-1)
    for i in range(0, n, max(1, n // 50)):          # most significant bit first
        assert bool((bits[i >> 3] >> (7 - (i & 7))) & 1) == bool(flat[i])
    ones = O.pack(np.ones(shape, bool))
    assert np.unpackbits(ones).sum() == n


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 16, 33, 128, 1024])
def test_lookup_of_an_axis_at_its_special_values(n):
    assert O.cell(F(-1.0 + 2.0 ** -24), n) == 0 and O.cell(F(0.0), n) == n // 2
    # for p = 1 - 2^-24 the float32 sum rounds to 2.0 and the product is n: the clamp keeps the cell inside
    p = F(1.0 - 2.0 ** -24)
    assert p < 1 and (p + F(1.0)).astype(F) == F(2.0) and O.cell(p, n) == n - 1
    # a cell edge -1 + 2 i / n (where float32 holds it exactly) belongs to cell i, a point 2^-20 below it to cell i - 1; the edge's lower float32
    # neighbour may land in either (near 0 the sum p + 1 rounds it back onto the edge), never elsewhere
    i = np.arange(1, n)
    edges = (F(-1.0) + F(2.0) * i.astype(F) / F(n)).astype(F)
    exact = edges.astype(np.float64) == -1.0 + 2.0 * i / n
    assert np.array_equal(O.cell(edges, n)[exact], i[exact])
    assert np.array_equal(O.cell((edges - F(2.0 ** -20)).astype(F), n)[exact], i[exact] - 1)
    below = O.cell(np.nextafter(edges, F(-2.0)), n)[exact]
    assert ((below == i[exact]) | (below == i[exact] - 1)).all()
    vals = O.special_values(n)
    pts = np.zeros((vals.shape[0], 3), F)
    pts[:, 1] = vals
    inside = O.in_cube(pts)
    assert not inside[[0, 4, 5]].any() and inside[[1, 2, 3]].all()          # -1, 1 and NaN are out; their neighbours inside and 0 are in
    full, none = O.pack(np.ones((3, n, 2), bool)), O.pack(np.zeros((3, n, 2), bool))
    assert np.array_equal(O.lookup(full, (3, n, 2), pts), inside) and not O.lookup(none, (3, n, 2), pts).any()
    vol = np.zeros((3, n, 2), bool)
    vol[:, n - 1, :] = True          # only the last cell of the axis
    got = O.lookup(O.pack(vol), (3, n, 2), pts)
    assert got[3] and (n == 1 or not got[1])


def test_lookup_agrees_with_float64_cells_away_from_the_boundaries():
    shape = (7, 8, 9)
    pts = (np.random.default_rng(3).random((20000, 3)) * 2.4 - 1.2).astype(F)
    vol = O.random_mask(shape)
    got = O.lookup(O.pack(vol), shape, pts)
    p64 = pts.astype(np.float64)
    ok = (np.abs(p64) < 1).all(-1)
    c = O.cells64(p64, shape)
    want = np.zeros(len(pts), bool)
    want[ok] = vol[c[ok, 0], c[ok, 1], c[ok, 2]]
    far = ~O.near_boundary(p64, shape, 1e-6)
    assert np.array_equal(got[far], want[far]) and not got[~ok].any() and far.mean() > 0.99


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------------------------------------------
NEW = ("ngf_uv_occupancy_workspace_bytes", "ngf_uv_occupancy_from_lattice", "ngf_uv_set_occupancy", "ngf_uv_occupancy_lookup")


def test_occupancy_symbols_are_exported_by_both_libraries():
    for path in (_lib.SO_PATH, _lib.SO_PATH_EXP):
        L = C.CDLL(path)
        for name in NEW:
            assert hasattr(L, name), (path, name)
    assert set(NEW) <= set(_lib.SYMBOLS)
    assert _lib.lib().ngf_abi_version() == 5


def _fake():
    buf = (C.c_char * 8192)()           # zeroed: stands in for a handle without a mask; as a data pointer it is never dereferenced
    return buf, C.c_void_p(C.addressof(buf))


def test_from_lattice_refuses_bad_arguments_without_a_gpu():
    L = _lib.lib()
    f, wb = L.ngf_uv_occupancy_from_lattice, L.ngf_uv_occupancy_workspace_bytes
    keep, p = _fake()
    big = 1 << 40
    assert f(None, 4, 4, 4, 0.0, 1, p, p, big, None) == E_ARG and b"ngf_uv_occupancy_from_lattice" in L.ngf_last_error()
    assert f(p, 4, 4, 4, 0.0, 1, None, p, big, None) == E_ARG and b"bits" in L.ngf_last_error()
    assert f(p, 4, 4, 4, 0.0, 1, p, None, big, None) == E_ARG and b"workspace" in L.ngf_last_error()
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (1025, 4, 4), (4, 1025, 4), (4, 4, 1025)):
        assert f(p, *dims, 0.0, 1, p, p, big, None) == E_ARG, dims
        assert b"1024" in L.ngf_last_error()
        assert wb(*dims) == -E_ARG and b"ngf_uv_occupancy_workspace_bytes" in L.ngf_last_error()
    for d in (-1, 3):
        assert f(p, 4, 4, 4, 0.0, d, p, p, big, None) == E_ARG and b"dilate" in L.ngf_last_error()
    assert f(p, 4, 4, 4, float("nan"), 1, p, p, big, None) == E_ARG and b"NaN" in L.ngf_last_error()
    need = wb(4, 5, 6)
    assert need >= 4 * 5 * 6 and wb(1024, 1024, 1024) >= 1 << 30 and wb(1, 1, 1) >= 1
    assert f(p, 4, 5, 6, 0.0, 1, p, p, need - 1, None) == E_ARG and b"workspace" in L.ngf_last_error()
    assert f(p, 4, 5, 6, 0.0, 1, p, p, -5, None) == E_ARG


def test_set_occupancy_and_lookup_refuse_bad_arguments_without_a_gpu():
    L = _lib.lib()
    s, q = L.ngf_uv_set_occupancy, L.ngf_uv_occupancy_lookup
    keep, p = _fake()
    assert s(None, p, 4, 4, 4, None) == E_ARG and b"ngf_uv_set_occupancy" in L.ngf_last_error()
    assert s(None, None, 0, 0, 0, None) == E_ARG
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (4, -2, 4), (1025, 4, 4), (4, 1025, 4), (4, 4, 1025)):
        assert s(p, p, *dims, None) == E_ARG, dims
        assert b"1024" in L.ngf_last_error()
    assert q(None, p, 1, p, None) == E_ARG and b"ngf_uv_occupancy_lookup" in L.ngf_last_error()
    assert q(p, None, 1, p, None) == E_ARG and b"points" in L.ngf_last_error()
    assert q(p, p, 1, None, None) == E_ARG and b"output" in L.ngf_last_error()
    assert q(p, p, -1, p, None) == E_ARG and b"n=-1" in L.ngf_last_error()
    assert q(p, p, 1, p, None) == E_ARG and b"no occupancy mask" in L.ngf_last_error()          # the zeroed block: a handle without a mask
    assert q(p, p, 0, p, None) == E_ARG                                                         # ... also for an empty list


# ---- the Python surface on the host --------------------------------------------------------------------------------------------------------------
def _cpu_net():
    return uvmapping.NeuTex(primitive_type="square", sample_num=64, device="cpu")


def test_set_occupancy_validates_on_the_host():
    net = _cpu_net()
    assert net.occupancy is None and net.occupancy_state() == {}
    for bad in (np.zeros((4, 4), bool), np.zeros((4, 4, 4), np.float32), np.zeros((0, 4, 4), bool), np.zeros((1025, 1, 1), bool), "mask"):
        with pytest.raises((ValueError, TypeError)):
            net.set_occupancy(bad)
    for bits, shape in ((np.zeros(8, np.uint8), (4, 4, 5)), (np.zeros(10, np.int32), (4, 4, 5)), (np.zeros((2, 5), np.uint8), (4, 4, 5)),
                        (np.zeros(10, np.uint8), (4, 4)), (np.zeros(10, np.uint8), (4, 4, 0)), (np.full(10, 255, np.uint8), (3, 5, 5))):          # the last: 75 cells in 10 bytes with their 5 tail bits set
        with pytest.raises(ValueError):
            net.set_occupancy((bits, shape))
    assert net.occupancy is None
    for res in (0, 1025, (4, 4), (4, 0, 4)):
        with pytest.raises(ValueError):
            uvmapping._occupancy_shape(res)
    assert uvmapping._occupancy_shape(7) == (7, 7, 7) and uvmapping._occupancy_shape((1, 1024, 3)) == (1, 1024, 3)
    with pytest.raises(RuntimeError):
        net.build_occupancy(8)          # a CPU model builds nothing: there is no CPU path
    with pytest.raises(RuntimeError):
        net.occupied(np.zeros((1, 3), np.float32))


def test_occupancy_state_round_trips_on_the_host():
    import pickle
    net = _cpu_net()
    vol = O.random_mask((5, 7, 3))
    occ = net.set_occupancy(vol)
    assert occ is net.occupancy and occ.shape == (5, 7, 3) and occ.threshold is None and occ.dilate is None
    assert np.array_equal(occ.bits.numpy(), O.pack(vol)) and np.array_equal(occ.volume().numpy(), vol)
    assert occ.fraction() == pytest.approx(vol.mean())
    state = net.occupancy_state()
    assert sorted(state) == ["occupancy.mask", "occupancy.shape"]
    assert state["occupancy.shape"].tolist() == [5, 7, 3] and np.array_equal(state["occupancy.mask"], np.packbits(vol.reshape(-1)))
    assert not any(k.startswith("occupancy") for k in net.state_dict())          # not a buffer
    twin = _cpu_net()
    twin.load_occupancy(state)
    assert np.array_equal(twin.occupancy.volume().numpy(), vol)
    twin.load_occupancy({})
    assert twin.occupancy is None
    for bad in ({"occupancy.shape": state["occupancy.shape"]}, {"occupancy.shape": np.array([5, 7]), "occupancy.mask": state["occupancy.mask"]},
                {"occupancy.shape": np.array([5, 7, 4]), "occupancy.mask": state["occupancy.mask"]}):
        with pytest.raises(ValueError):
            twin.load_occupancy(bad)
    net.set_occupancy(vol.astype(np.uint8) * 3)          # uint8: non-zero = occupied
    assert np.array_equal(net.occupancy.volume().numpy(), vol)
    clone = pickle.loads(pickle.dumps(net))
    assert np.array_equal(clone.occupancy.volume().numpy(), vol) and clone.occupancy.shape == (5, 7, 3)
    net.set_occupancy(None)
    assert net.occupancy is None


# ---- the render test's batches, for the reference alone ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prim", ["sphere", "square"])
@pytest.mark.parametrize("S", O.RENDER_S)
def test_render_batches_keep_off_the_cell_boundaries(S, prim):
    for bname, cam, rd, U in O.render_batches(prim, S):
        for mname, vol in O.render_masks():
            keep, pinned, valid, p32, p64 = O.decisions(cam, rd, U, vol)
            near = valid & ~pinned
            share = near.sum() / valid.sum()
            print(f"uv_occupancy {bname} S={S} {prim} {mname} {vol.shape}: {valid.sum()} in-cube samples, {near.sum()} within 1e-5 of a cell boundary ({100 * share:.3f} %), "
                  f"{keep.sum()} kept")
            assert valid.sum() > 100 and share <= O.NEAR_LIMIT
            # float32 and float64 agree on the cell wherever the float64 position keeps the margin
            c32 = np.stack([O.cell(p32[..., k], vol.shape[k]) for k in range(3)], -1)
            assert np.array_equal(c32[pinned], O.cells64(p64, vol.shape)[pinned])
            assert 0 < keep.sum() < valid.sum()          # the mask both keeps and skips
