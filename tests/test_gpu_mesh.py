"""GPU tests of the mesh export (csrc/ngf_mesh.hip, ngf_amd.mesh, Base.export_mesh).  Unless a test says otherwise the
device arrays are compared with the numpy restatement tests/mesh_ref.py: vertices bit for bit, faces equal.

Sizes.  One thread per lattice point in blocks of 256 points (kMeshBlock); the block sums are scanned in chunks of 1024 pairs (kMeshScanChunk),
level upon level.  BLOCK_SHAPES are one below, at and just above 256 points (257 is prime: 257 x 1 x 1 has no cells, 258 = 2 x 3 x 43 is the
nearest volume above with cells); CHUNK_SHAPES give 1023 full blocks, 1024 blocks with the last one short by a point, 1024 full blocks (64^3)
and 1025 blocks -- the first shape whose block sums need the second scan level.  A third level needs more than 2^28 lattice points (a 1 GiB
volume), so the levels above are driven through the unit's scan alone (ngf_debug_mesh_scan) at one below, at and one above 1024 and 1024^2
pairs.  A volume whose x stride is smaller than its z stride (layout "z") is classified by 16 x 16 tiles (kMeshTile) in a kernel of its own:
every shape also runs in that layout, none of those above 16 a multiple of the tile on all axes but 64^3 and 64 x 62 x 66's x."""
import ctypes as C

import numpy as np
import pytest
import torch

import ngf_amd  # noqa: F401
from ngf_amd import _lib, mesh, synth
from helpers import field_for_case
import mesh_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x7FC0DEAD

SMALL_SHAPES = [(2, 2, 2), (3, 2, 2), (1, 5, 5), (5, 7, 9)]
BLOCK_SHAPES = [(3, 5, 17), (4, 8, 8), (257, 1, 1), (2, 3, 43)]
CHUNK_SHAPES = [(64, 62, 66), (27, 133, 73), (64, 64, 64), (65, 37, 109)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def on_device(vol, layout):
    """The numpy volume [gx,gy,gz] as a device tensor of the same shape: x-major (contiguous), z-major (the memory of [gz,gy,gx]) or a
    non-contiguous view with a storage offset."""
    t = torch.from_numpy(np.ascontiguousarray(vol))
    if layout == "x":
        return t.to(DEV)
    if layout == "z":
        return t.permute(2, 1, 0).contiguous().to(DEV).permute(2, 1, 0)
    gx, gy, gz = vol.shape
    big = torch.full((gx + 2, 2 * gy + 1, gz + 3), float("nan"), device=DEV)
    view = big[1:-1, 1::2, 2:-1]
    view.copy_(t.to(DEV))
    assert view.shape == t.shape and not view.is_contiguous()
    return view


def check(vol, level, layout="x", **kw):
    """marching_cubes on the device equals the restatement; returns the host arrays."""
    want = R.marching_cubes_ref(vol, level, **kw)
    got = mesh.marching_cubes(on_device(vol, layout), level, **kw)
    v, f = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert v.dtype == np.float32 and f.dtype == np.int32 and v.shape == want[0].shape and f.shape == want[1].shape, (v.shape, want[0].shape, f.shape, want[1].shape)
    assert np.array_equal(bits(v), bits(want[0])), f"{int((bits(v) != bits(want[0])).sum())} vertex words differ"
    assert np.array_equal(f, want[1])
    return v, f


def smooth(shape, seed):
    """A sum of random plane waves: smooth, both signs, no symmetry."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), -1)
    out = np.zeros(shape)
    for _ in range(6):
        k = rng.uniform(-0.9, 0.9, 3)
        out += rng.uniform(0.3, 1.0) * np.sin(g @ k + rng.uniform(0, 6.28))
    return out.astype(np.float32)


def binary(shape, seed, border=False):
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 2, shape).astype(np.float32)
    if border:
        v[0] = v[-1] = 0
        v[:, 0] = v[:, -1] = 0
        v[:, :, 0] = v[:, :, -1] = 0
    return v


@pytest.mark.parametrize("layout", ["x", "z", "view"])
def test_all_256_corner_configurations(layout):
    rng = np.random.default_rng(256)
    level = 0.37
    total = 0
    for case in range(256):
        ins = np.array([case >> c & 1 for c in range(8)], bool).reshape(2, 2, 2).transpose(2, 1, 0)       # corner c = x + 2y + 4z -> [x,y,z]
        mag = rng.uniform(0.1, 1.0, (2, 2, 2))
        vol = np.where(ins, level + mag, level - mag).astype(np.float32)
        v, f = check(vol, level, layout, spacing=(0.5, 1.25, 2.0), origin=(-1.0, 0.25, 3.0))
        assert f.shape[0] == R.TRI_COUNT[case] and v.shape[0] == sum((case >> a & 1) != (case >> b & 1) for a, b in R.T.EDGE_CORNERS)
        total += f.shape[0]
    assert total == 820


@pytest.mark.parametrize("shape", SMALL_SHAPES + BLOCK_SHAPES + CHUNK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_volumes_at_the_edge_sizes(shape):
    n = shape[0] * shape[1] * shape[2]
    v, f = check(smooth(shape, n), 0.1, "x", spacing=(0.3, 0.2, 0.7), origin=(-2.0, 1.0, 0.5))
    assert v.shape[0] == 0 if min(shape) == 1 else (v.shape[0] > 0 or n < 100)
    check(binary(shape, n + 1), 0.5, "x")
    check(smooth(shape, n + 2), -0.2, "z", flip=True)
    if n < 1000:
        check(binary(shape, n + 3), 0.5, "view")


@pytest.mark.parametrize("n", [1, 255, 1023, 1024, 1025, 1024 * 1024 - 1, 1024 * 1024, 1024 * 1024 + 1])
def test_device_wide_scan_at_every_level(n):
    rng = np.random.default_rng(n)
    a = np.stack([rng.integers(0, 4, n), rng.integers(0, 6, n)], 1).astype(np.uint32)
    pairs = torch.from_numpy(a.view(np.int32)).to(DEV)
    scratch = torch.zeros((n // 512 + 8, 2), dtype=torch.int32, device=DEV)
    totals = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    _lib.check(_lib.lib().ngf_debug_mesh_scan(pairs.data_ptr(), n, scratch.data_ptr(), scratch.shape[0], totals.data_ptr(),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    want = np.cumsum(a.astype(np.int64), 0) - a
    assert np.array_equal(pairs.cpu().numpy().view(np.uint32).astype(np.int64), want)
    assert totals.tolist() == a.astype(np.int64).sum(0).tolist()


def test_closed_and_oriented_on_the_device_arrays():
    for seed in range(6):
        shape = [(9, 8, 7), (12, 5, 6), (4, 17, 9)][seed % 3]
        v, f = check(binary(shape, 40 + seed, border=True), 0.5, ["x", "z"][seed % 2])
        assert f.shape[0] > 0 and R.closed_and_oriented(f) and len(np.unique(f)) == v.shape[0]
    r, shape, sp = 6.3, (20, 18, 22), (1.0, 1.0, 1.0)
    v, f = check(R.ball(shape, r), 0.0)
    assert R.closed_and_oriented(f) and R.euler_characteristic(f) == 2
    assert 0.95 * 4 / 3 * np.pi * r ** 3 < R.signed_volume(v, f) < 4 / 3 * np.pi * r ** 3
    d = np.linalg.norm(v.astype(np.float64) - np.array([9.5, 8.5, 10.5]), axis=1)
    assert np.abs(d - r).max() <= 1.0            # r - |p| is 1-Lipschitz: a sign change on an edge of length 1 puts the vertex within 1 of the sphere
    vf, ff = check(R.ball(shape, r), 0.0, flip=True)
    assert R.signed_volume(vf, ff) < 0 and np.array_equal(bits(vf), bits(v))


def test_normals_against_fp64():
    """DESIGN.md section 4.7's criterion: e_hip <= max(4 * e_numpy32, 1e-6) against the fp64 restatement, over the vertices whose interpolated
    gradient is not below 1e-3 of the largest."""
    for shape, seed, layout in (((5, 7, 9), 1, "x"), ((33, 18, 21), 2, "z"), ((2, 2, 2), 3, "view"), ((3, 40, 2), 4, "x")):
        vol = smooth(shape, seed)
        kw = dict(spacing=(0.3, 0.2, 0.7), origin=(-2.0, 1.0, 0.5), normals=True)
        v64, f64, n64 = R.marching_cubes_ref(vol, 0.1, dtype=np.float64, **kw)
        v32, f32, n32 = R.marching_cubes_ref(vol, 0.1, **kw)
        v, f, n = (t.cpu().numpy() for t in mesh.marching_cubes(on_device(vol, layout), 0.1, **kw))
        assert np.array_equal(bits(v), bits(v32)) and np.array_equal(f, f32) and n.shape == n64.shape and n.dtype == np.float32
        g = R._gradient(vol.astype(np.float64), [np.float32(s) for s in kw["spacing"]], np.float64).reshape(3, -1)
        size = interpolated_gradient_size(vol, 0.1, kw["spacing"])
        assert size.shape[0] == n64.shape[0]
        big = size >= 1e-3 * np.sqrt((g * g).sum(0)).max()
        assert big.sum() > 0.9 * big.size
        e_hip = float(np.abs(n[big] - n64[big]).max())
        e_np = float(np.abs(n32[big] - n64[big]).max())
        print(f"normals {shape} {layout}: e_hip {e_hip:.3e}, e_numpy32 {e_np:.3e}, {int(big.sum())} of {big.size} vertices")
        assert e_hip <= max(4 * e_np, 1e-6)
        assert np.abs(np.linalg.norm(n[big], axis=1) - 1).max() < 1e-6


def interpolated_gradient_size(vol, level, spacing):
    """|g0 + t (g1 - g0)| per vertex in fp64, in the vertex order of the restatement."""
    vol64 = vol.astype(np.float64)
    g = R._gradient(vol64, [np.float32(s) for s in spacing], np.float64).reshape(3, -1)
    flat = vol64.reshape(-1)
    inside = (vol >= np.float32(level)).reshape(vol.shape)
    step = (vol.shape[1] * vol.shape[2], vol.shape[2], 1)
    recs = []
    for a in range(3):
        m = np.zeros(vol.shape, bool)
        sl = [slice(None)] * 3
        sl[a] = slice(0, -1)
        hi = [slice(None)] * 3
        hi[a] = slice(1, None)
        m[tuple(sl)] = inside[tuple(sl)] != inside[tuple(hi)]
        p = np.nonzero(m.reshape(-1))[0]
        t = (np.float64(np.float32(level)) - flat[p]) / (flat[p + step[a]] - flat[p])
        gi = g[:, p] + t * (g[:, p + step[a]] - g[:, p])
        recs.append((p, np.full(p.shape, a), np.sqrt((gi * gi).sum(0))))
    p = np.concatenate([r[0] for r in recs])
    a = np.concatenate([r[1] for r in recs])
    s = np.concatenate([r[2] for r in recs])
    return s[np.lexsort((a, p))]                               # point order, a point's edges in x, y, z order


def test_level_on_corner_values_and_non_finite_volumes():
    rng = np.random.default_rng(11)
    ints = rng.integers(0, 3, (6, 7, 5)).astype(np.float32)
    for level in (0.0, 1.0, 2.0, 3.0):
        check(ints, level)                                     # t = 0 where the owner sits on the level; level 0 / 3: everything inside / outside
    vol = smooth((7, 6, 8), 5)
    pick = rng.integers(0, 6, vol.shape)
    vol[pick == 0] = np.nan
    vol[pick == 1] = np.inf
    vol[pick == 2] = -np.inf
    for layout in ("x", "z"):
        v, f = check(vol, 0.1, layout)
        assert np.isfinite(v).all() and f.shape[0] > 0
    for value, level in ((0.25, 0.25), (0.25, 0.5), (np.nan, 0.0), (np.inf, 1.0), (-np.inf, 1.0)):
        v, f = check(np.full((4, 5, 3), value, np.float32), level)
        assert v.shape[0] == 0 and f.shape[0] == 0


def raw_count(vol, level, stream=None):
    L = _lib.lib()
    nbytes = L.ngf_mesh_workspace_bytes(*vol.shape)
    work = torch.zeros((nbytes,), dtype=torch.uint8, device=DEV)
    counts = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    dims, strides = (C.c_int32 * 3)(*vol.shape), (C.c_int64 * 3)(*vol.stride())
    _lib.check(L.ngf_mesh_count(vol.data_ptr(), dims, strides, C.c_float(level), work.data_ptr(), nbytes, counts.data_ptr(),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return work, counts.tolist()


def raw_emit(vol, level, work, nv, nt, rows_v, rows_f, flags=0):
    """ngf_mesh_emit into buffers of rows_v / rows_f rows pre-filled with sentinels; (rc, vertices, normals, faces) as uint32 / int32 host arrays."""
    L = _lib.lib()
    verts = torch.full((rows_v, 3), SENTINEL, dtype=torch.int32, device=DEV)
    nrm = torch.full((rows_v, 3), SENTINEL, dtype=torch.int32, device=DEV)
    faces = torch.full((rows_f, 3), -7, dtype=torch.int32, device=DEV)
    dims, strides = (C.c_int32 * 3)(*vol.shape), (C.c_int64 * 3)(*vol.stride())
    rc = L.ngf_mesh_emit(vol.data_ptr(), dims, strides, C.c_float(level), (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), flags, work.data_ptr(),
                         work.numel(), nv, nt, verts.data_ptr(), nrm.data_ptr(), faces.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, verts.cpu().numpy().view(np.uint32), nrm.cpu().numpy().view(np.uint32), faces.cpu().numpy()


def test_sentinels_keep_their_bits_and_wrong_counts_are_refused():
    for shape, seed in (((5, 7, 9), 1), ((27, 19, 13), 2), ((1, 5, 5), 3)):
        host = smooth(shape, seed)
        vol = on_device(host, "x")
        want_v, want_f = R.marching_cubes_ref(host, 0.1)
        work, (nv, nt) = raw_count(vol, 0.1)
        assert (nv, nt) == (want_v.shape[0], want_f.shape[0])                      # count's totals are what emit writes
        pad = 5
        rc, v, n, f = raw_emit(vol, 0.1, work, nv, nt, nv + pad, nt + pad, flags=_lib.MESH_NORMALS)
        assert rc == 0
        assert np.array_equal(v[:nv], bits(want_v)) and np.array_equal(f[:nt], want_f)
        assert (v[nv:] == SENTINEL).all() and (n[nv:] == SENTINEL).all() and (f[nt:] == -7).all()
        assert (n[:nv] != SENTINEL).all() and (f[:nt] >= 0).all() and (f[:nt] < max(nv, 1)).all()
        if nv == 0:
            continue
        for bad_nv, bad_nt in ((nv + 1, nt), (nv - 1, nt), (nv, nt + 1), (nv, nt - 1), (0, 0)):
            rc, v, n, f = raw_emit(vol, 0.1, work, bad_nv, bad_nt, nv + pad, nt + pad, flags=_lib.MESH_NORMALS)
            assert rc == 1 and b"ngf_mesh_emit" in _lib.lib().ngf_last_error()
            assert (v == SENTINEL).all() and (n == SENTINEL).all() and (f == -7).all()      # nothing written
        rc, v, n, f = raw_emit(vol, 0.2, work, nv, nt, nv + pad, nt + pad)                      # the workspace holds another level's count
        assert rc == 1 and (v == SENTINEL).all() and (f == -7).all()
        rc, v, n, f = raw_emit(vol, 0.1, work, nv, nt, nv, nt)                                  # no normals asked for: that buffer stays
        assert rc == 0 and (n == SENTINEL).all() and np.array_equal(v, bits(want_v))


def test_two_calls_and_a_side_stream_are_bit_identical():
    host = smooth((33, 29, 31), 9)
    vol = on_device(host, "z")
    kw = dict(spacing=(0.3, 0.2, 0.7), origin=(-2.0, 1.0, 0.5), normals=True)
    first = [t.cpu().numpy() for t in mesh.marching_cubes(vol, 0.1, **kw)]
    second = [t.cpu().numpy() for t in mesh.marching_cubes(vol, 0.1, **kw)]
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = [t.cpu().numpy() for t in mesh.marching_cubes(vol, 0.1, **kw)]
    side.synchronize()
    assert first[0].shape[0] > 1000
    for other in (second, third):
        for a, b in zip(first, other):
            assert a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
BALL_A, BALL_C, PLANE_RES = 14.0, 20.0, 64


def ball_field():
    """A TriPlane field whose density pre-activation is a - c |p|^2 in normalised coordinates: the density is a sum of three plane functions,
    so -c (u^2 + v^2) / 2 (+ a / 3) on one density channel per plane, weight 1 on those three channels, zero gauge planes."""
    g = {"model": np.array("triplane"), "aabb": np.array([[-1.5] * 3, [1.5] * 3], np.float32), "grid": np.array([32] * 3),
         "near_far": np.array([2.0, 6.0], np.float32), "step_ratio": np.float32(0.5), "distance_scale": np.float32(25), "thr": np.float32(1e-4)}
    p = synth.triplane_params(5, ((PLANE_RES, PLANE_RES),) * 3, (8, 8), preset="R0")
    u = np.linspace(-1.0, 1.0, PLANE_RES)
    quad = (BALL_A / 3 - BALL_C * (u[None, :] ** 2 + u[:, None] ** 2) / 2).astype(np.float32)
    w = np.zeros((1, 48), np.float32)
    for k, name in enumerate(("xy", "yz", "xz")):
        p[f"plane_{name}"][0, 0] = quad
        p[f"gauge_{name}"][:] = 0
        w[0, 16 * k] = 1
    p["density_decoder.weight"] = w
    p["density_decoder.bias"] = np.zeros((1,), np.float32)
    return field_for_case(g, p, None, device=DEV)


def check_field(f, level, grid, tmp_path, **kw):
    alpha, _ = f.getDenseAlpha(grid, **kw)
    lo, hi = f.aabb.cpu().numpy().astype(np.float32)
    spacing = (hi - lo) / (np.asarray(grid, np.float32) - np.float32(1))
    want_v, want_f = R.marching_cubes_ref(alpha.cpu().numpy(), level, spacing=spacing, origin=lo)
    path = str(tmp_path / "mesh.ply")
    v, fc = (t.cpu().numpy() for t in f.export_mesh(path, level=level, gridSize=grid, **kw))
    assert want_f.shape[0] > 0 and np.array_equal(bits(v), bits(want_v)) and np.array_equal(fc, want_f)
    pv, pf = R.read_ply(path)
    assert np.array_equal(bits(pv), bits(v)) and np.array_equal(pf, fc)
    return v, fc, spacing


def test_export_mesh_of_a_ball_field_end_to_end(tmp_path):
    f = ball_field()
    level, grid = 0.005, (24, 20, 28)
    v, fc, spacing = check_field(f, level, grid, tmp_path)
    assert R.closed_and_oriented(fc) and R.euler_characteristic(fc) == 2 and R.signed_volume(v, fc) > 0
    # the radius at which alpha = 1 - exp(-softplus(a - c r^2 - 10) * stepSize) crosses the level, in fp64; world = 1.5 x normalised
    sigma = -np.log1p(-level) / float(f.stepSize)
    pre = np.log(np.expm1(sigma)) + 10.0
    radius = 1.5 * np.sqrt((BALL_A - pre) / BALL_C)
    err = np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - radius).max()
    print(f"ball field: radius {radius:.6f}, worst vertex {err:.3e}, cell diagonal {np.linalg.norm(spacing):.3e}")
    assert 0.5 < radius < 1.2 and err <= np.linalg.norm(spacing.astype(np.float64))
    out = f.export_mesh(level=level, gridSize=grid, normals=True)
    assert len(out) == 3 and np.array_equal(bits(out[0].cpu().numpy()), bits(v))
    unit = v / np.linalg.norm(v, axis=1, keepdims=True)
    assert (out[2].cpu().numpy() * unit).sum(1).min() > 0.9                                       # outward
    # the dense alpha updateAlphaMask leaves, marched in its own [gz,gy,gx] layout
    f.updateAlphaMask(grid)
    dense = f.last_dense_alpha
    assert tuple(dense.shape) == grid[::-1] and dense.is_contiguous()
    want_v, want_f = R.marching_cubes_ref(dense.cpu().numpy().transpose(2, 1, 0), level)
    got_v, got_f = mesh.marching_cubes(dense.permute(2, 1, 0), level)
    assert want_f.shape[0] > 0 and np.array_equal(bits(got_v.cpu().numpy()), bits(want_v)) and np.array_equal(got_f.cpu().numpy(), want_f)


@pytest.mark.parametrize("infoinv", [True, False])
def test_export_mesh_of_an_infoinv_field(tmp_path, infoinv):
    g = {"model": np.array("infoinv"), "aabb": np.array([[-1.5, -1.0, -1.25], [1.5, 1.0, 1.25]], np.float32), "grid": np.array([32] * 3),
         "near_far": np.array([2.0, 6.0], np.float32), "step_ratio": np.float32(0.5), "distance_scale": np.float32(25), "thr": np.float32(1e-4)}
    f = field_for_case(g, synth.infoinv_params(7, ((32, 32),) * 3, preset="R1"), None, device=DEV)
    grid = (12, 10, 14)
    alpha, _ = f.getDenseAlpha(grid, infoinv=infoinv)
    lo, hi = float(alpha.min()), float(alpha.max())
    assert lo < hi
    check_field(f, 0.5 * (lo + hi), grid, tmp_path, infoinv=infoinv)


def test_convert_sdf_samples_to_ply_on_the_device(tmp_path):
    host = R.ball((12, 10, 14), 3.7)
    bbox = np.array([[-1.0, -0.5, 0.0], [2.0, 1.5, 3.5]], np.float32)
    path = str(tmp_path / "sdf.ply")
    pts, faces = mesh.convert_sdf_samples_to_ply(on_device(host, "x"), path, bbox, level=0.0, offset=np.array([0.5, 0.0, -0.5]), scale=2.0)
    voxel = list((bbox[1] - bbox[0]) / np.array(host.shape))
    v, f = R.marching_cubes_ref(host, 0.0, spacing=voxel, flip=True)
    assert np.array_equal(faces, f) and np.array_equal(pts, mesh.mesh_points(v, bbox, np.array([0.5, 0.0, -0.5]), 2.0))
    pv, pf = R.read_ply(path)
    assert np.array_equal(pf, f) and np.array_equal(pv, pts.astype(np.float32))
    assert R.signed_volume(pv, pf) < 0                                                            # the reference reverses the faces
