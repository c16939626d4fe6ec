"""CPU checks of the UV-Mapping (NeuTex) point queries and the UV-textured mesh export: the two C-ABI symbols are exported by both libraries and
refuse bad arguments without a GPU; the torch restatement (tests/uv_query_eager.py) reproduces the reference's own outputs
(tests/golden/uv_query.npz); the lattice formula, mesh.atlas_coords, mesh.unwrap_seam and mesh.write_obj do what they say; the new translation
unit's kernels use no scratch; and a CPU model refuses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ngf_amd  # noqa: F401
from ngf_amd import _lib, mesh, uvmapping
import uv_query_eager as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-gauge-fields_amd", "csrc")
G = np.load(os.path.join(ROOT, "tests", "golden", "uv_query.npz"))
E_ARG = 1


def test_query_symbols_are_exported_by_both_libraries():
    hdr = open(os.path.join(ROOT, "include", "ngf.h")).read()
    for name in ("ngf_uv_query", "ngf_uv_density_lattice"):
        assert re.search(r"\b%s\s*\(" % name, hdr)
        assert name in _lib.SYMBOLS
        assert hasattr(_lib.lib(), name)
        with _lib.library("exp") as X:
            assert hasattr(X, name)
    assert re.search(r"NGF_UV_QUERY_NO_CLIP\s*=\s*2\b", hdr) and _lib.UV_QUERY_NO_CLIP == 2 and _lib.UV_TEX_DIFFUSE == 1
    assert re.search(r"#define NGF_ABI_VERSION 5\b", hdr) and _lib.lib().ngf_abi_version() == 5


def test_query_refuses_bad_arguments_without_a_gpu():
    L = _lib.lib()
    buf = (C.c_float * 6)()
    p = C.cast(buf, C.c_void_p)
    fake = C.c_void_p(C.addressof(buf))           # never dereferenced: every call below fails on an argument check first
    q = L.ngf_uv_query
    assert q(None, p, 1, p, 0, 0, p, p, p, None) == E_ARG                       # null handle
    assert b"ngf_uv_query" in L.ngf_last_error()
    assert q(fake, None, 1, p, 0, 0, p, p, p, None) == E_ARG                    # null points
    assert q(fake, p, 1, p, 0, 0, None, None, None, None) == E_ARG              # no output requested
    assert b"no output" in L.ngf_last_error()
    assert q(fake, p, 1, None, 0, 0, None, None, p, None) == E_ARG              # rgb without a view
    assert q(fake, p, 1, None, 0, 0, p, p, p, None) == E_ARG
    assert q(fake, p, 1, p, 2, 0, None, None, p, None) == E_ARG                 # stride neither 0 nor 3
    assert b"view_stride" in L.ngf_last_error()
    assert q(fake, p, 1, p, 0, 4, p, None, None, None) == E_ARG                 # unknown flag bit
    assert q(fake, p, -1, p, 0, 0, p, None, None, None) == E_ARG                # n < 0
    for flags in (0, _lib.UV_TEX_DIFFUSE, _lib.UV_QUERY_NO_CLIP, _lib.UV_TEX_DIFFUSE | _lib.UV_QUERY_NO_CLIP):
        assert q(fake, p, 0, None, 0, flags, p, p, p if flags & 1 else None, None) == 0          # n == 0: nothing to do, no launch


def test_density_lattice_refuses_bad_arguments_without_a_gpu():
    L = _lib.lib()
    buf = (C.c_float * 6)()
    p = C.cast(buf, C.c_void_p)
    fake = C.c_void_p(C.addressof(buf))
    lo, step = (C.c_float * 3)(-1, -1, -1), (C.c_float * 3)(0.5, 0.5, 0.5)
    d = L.ngf_uv_density_lattice
    assert d(None, lo, step, 5, 5, 5, 0, p, None) == E_ARG
    assert b"ngf_uv_density_lattice" in L.ngf_last_error()
    assert d(fake, None, step, 5, 5, 5, 0, p, None) == E_ARG
    assert d(fake, lo, None, 5, 5, 5, 0, p, None) == E_ARG
    assert d(fake, lo, step, 5, 5, 5, 0, None, None) == E_ARG
    for dims in ((1, 5, 5), (5, 1, 5), (5, 5, 1), (0, 5, 5), (5, -3, 5)):
        assert d(fake, lo, step, *dims, 0, p, None) == E_ARG, dims              # an axis below 2
    assert d(fake, lo, step, 5, 5, 5, 1, p, None) == E_ARG                      # the diffuse bit means nothing here
    assert d(fake, lo, step, 5, 5, 5, 4, p, None) == E_ARG
    for bad in (float("nan"), float("inf"), -float("inf")):
        for k in range(3):
            lo_b, step_b = (C.c_float * 3)(-1, -1, -1), (C.c_float * 3)(0.5, 0.5, 0.5)
            lo_b[k] = bad
            assert d(fake, lo_b, step, 5, 5, 5, 0, p, None) == E_ARG
            step_b[k] = bad
            assert d(fake, lo, step_b, 5, 5, 5, 0, p, None) == E_ARG
            assert b"finite" in L.ngf_last_error()


def test_fixture_holds_the_points_of_the_helper():
    assert np.array_equal(G["xyz"].view(np.uint32), Q.points().view(np.uint32)) and np.array_equal(G["view"].view(np.uint32), Q.views().view(np.uint32))
    xyz = G["xyz"]
    assert xyz.shape == (Q.N_POINTS, 3) and np.abs(xyz).max() <= 1.2 and (np.abs(xyz) >= 1).any(axis=1).sum() > 40
    assert (np.abs(xyz[:8]) >= 1).any(axis=1).sum() == 7 and np.abs(xyz[6]).max() < 1          # placed: seven on / outside the faces, one an ulp inside
    assert np.allclose(np.linalg.norm(G["view"].astype(np.float64), axis=1), 1, atol=1e-6)


@pytest.mark.parametrize("prim", Q.PRIMS)
def test_fp64_restatement_matches_the_reference_fp64_fixture(prim):
    net = Q.make_net(prim, "cpu", torch.float64)
    got = Q.restate(net, torch.from_numpy(G["xyz"]).double(), torch.from_numpy(G["view"]).double())
    for name in ("sigma", "uv", "rgb"):
        want = G[f"{prim}.{name}.f64"]
        assert got[name].dtype == torch.float64 and tuple(got[name].shape) == want.shape
        assert float(np.abs(got[name].numpy() - want).max()) <= 1e-12, name


@pytest.mark.parametrize("prim", Q.PRIMS)
def test_fp32_restatement_matches_the_reference_fp32_fixture(prim):
    """The same modules in float32 on the same points.  The restatement and the reference run the same torch operators on the same values, so
    the distance is expected to be 0; what is allowed is the project's criterion for an fp32 evaluation: 4x the
    reference's own fp32 distance to fp64, from the fixture, with the floor of 2e-6."""
    net = Q.make_net(prim, "cpu")
    got = Q.restate(net, torch.from_numpy(G["xyz"]), torch.from_numpy(G["view"]))
    for name in ("sigma", "uv", "rgb"):
        f32, f64 = G[f"{prim}.{name}.f32"], G[f"{prim}.{name}.f64"]
        bound = max(4 * float(np.abs(f32 - f64).max()), 2e-6)
        err = float(np.abs(got[name].numpy().astype(np.float64) - f64).max())
        print(f"{prim}.{name}: max|restatement fp32 - fp64| = {err:.3e} (bound {bound:.3e}), max|restatement - reference fp32| = "
              f"{float(np.abs(got[name].numpy() - f32).max()):.3e}")
        assert got[name].dtype == torch.float32 and err <= bound, name


@pytest.mark.parametrize("lo,hi,res", [((-1, -1, -1), (1, 1, 1), (5, 4, 3)), ((-0.5, -0.25, 0), (0.5, 0.75, 1), (6, 7, 9)), ((-1, -1, -1), (1, 1, 1), (33, 33, 33))])
def test_numpy_lattice_formula_equals_a_plain_float32_loop(lo, hi, res):
    step = Q.lattice_step(lo, hi, res)
    pts = Q.lattice_points(lo, step, res)
    assert pts.dtype == np.float32 and pts.shape == tuple(res) + (3,) and step.dtype == np.float32
    lo32 = np.asarray(lo, np.float32)
    rng = np.random.RandomState(3)
    picks = [(0, 0, 0), tuple(r - 1 for r in res)] + [tuple(int(rng.randint(r)) for r in res) for _ in range(200)]
    for ijk in picks:
        for k in range(3):
            prod = np.float32(np.float32(ijk[k]) * step[k])          # rounded product, then rounded sum: no fused multiply-add
            assert pts[ijk][k] == np.float32(lo32[k] + prod)
            assert np.float64(prod) == np.float32(np.float64(ijk[k]) * np.float64(step[k]))         # (the float32 product IS the rounded exact one)
    if tuple(lo) == (-1, -1, -1):
        assert (pts[0, ..., 0] == -1).all() and (pts[:, 0, :, 1] == -1).all() and (pts[..., 0, 2] == -1).all()


def test_lattice_reaches_hi_at_every_size():
    """(hi - lo) / (n - 1) rounded to float32 can leave the last point an ulp short of hi (n = 42 is the first such size for the unit cube), where
    the clip would not zero it: density_lattice's step is an ulp longer there.  The helper restates the rule; both agree bit for bit."""
    n_long = 0
    for n in range(2, 1025):
        res, lo, step = uvmapping.lattice_axes(n)
        assert res == (n, n, n) and lo.dtype == np.float32 and step.dtype == np.float32
        assert np.array_equal(step.view(np.uint32), Q.lattice_step((-1, -1, -1), (1, 1, 1), res).view(np.uint32))
        top = np.float32(lo[0] + np.float32(np.float32(n - 1) * step[0]))
        plain = np.float32(2) / np.float32(n - 1)
        assert 1 <= top <= 1 + 2e-6 and step[0] in (plain, np.nextafter(plain, np.float32(4)))
        n_long += int(step[0] != plain)
    assert n_long == 137 and uvmapping.lattice_axes(41)[2][0] == np.float32(0.05) and uvmapping.lattice_axes(42)[2][0] > np.float32(2) / np.float32(41)
    res, lo, step = uvmapping.lattice_axes((6, 7, 9), (-0.5, -0.25, 0), (0.5, 0.75, 1))
    assert res == (6, 7, 9) and np.array_equal(step, Q.lattice_step((-0.5, -0.25, 0), (0.5, 0.75, 1), res))
    for bad in (1, (5, 5), (5, 1, 5)):
        with pytest.raises(ValueError):
            uvmapping.lattice_axes(bad)


@pytest.mark.parametrize("R", [8, 16, 32])
def test_atlas_coords_map_the_exporters_points_to_their_texel_centres(R):
    """Every point export_sphere_points(R) / export_square_points(R) evaluates lands on the centre of the texel that holds its colour in the image
    the exporter returns: within 1e-3 texel for the sphere (s modulo 1; pole row 0, where the longitude is undefined, excluded), exactly for the
    square in float64."""
    # sphere: the exporter's image is its point grid flipped in the row index; OBJ t runs bottom to top
    pts = uvmapping.export_sphere_points(R)                      # [R,2R,3], row r, column c -> image row R - 1 - r, column c
    r, c = np.meshgrid(np.arange(R), np.arange(2 * R), indexing="ij")
    want_s, want_t = (c + 0.5) / (2 * R), 1 - ((R - 1 - r) + 0.5) / R
    for got in (mesh.atlas_coords(pts.double().numpy(), "sphere", R), mesh.atlas_coords(pts.double(), "sphere", R).numpy(),
                mesh.atlas_coords(pts, "sphere", R).double().numpy(), Q.atlas_coords_f64(pts.numpy(), "sphere", R)):
        ds = np.abs((got[..., 0] - want_s + 0.5) % 1.0 - 0.5) * (2 * R)          # in texels, modulo one turn
        dt = np.abs(got[..., 1] - want_t) * R
        assert ds[1:].max() <= 1e-3 and dt.max() <= 1e-3, (ds[1:].max(), dt.max())
    # square: texel [i,j] is evaluated at uv = (centre i, centre j); image row i, column j
    sq = uvmapping.export_square_points(R).double()
    i, j = np.meshgrid(np.arange(R), np.arange(R), indexing="ij")
    for got in (mesh.atlas_coords(sq.numpy(), "square"), Q.atlas_coords_f64(sq.numpy(), "square")):
        assert np.array_equal(got[..., 0], (j + 0.5) / R) and np.array_equal(got[..., 1], 1 - (i + 0.5) / R)
    got32 = mesh.atlas_coords(sq.float(), "square")
    assert got32.dtype == torch.float32 and np.abs(got32.numpy() - Q.atlas_coords_f64(sq.numpy(), "square")).max() * R <= 1e-3
    with pytest.raises(ValueError):
        mesh.atlas_coords(pts, "sphere")                         # the sphere image depends on R
    with pytest.raises(ValueError):
        mesh.atlas_coords(pts, "cube", R)


def test_unwrap_seam_on_hand_made_triangles():
    # s on a 1/64 lattice, so that (s + 1) mod 1 == s exactly
    s = np.array([2, 10, 20, 60, 62, 33, 1, 40, 30, 63, 34], dtype=np.float64) / 64
    st = np.stack([s, np.linspace(0.1, 0.9, len(s))], axis=-1)
    faces = np.array([[0, 1, 2],        # needs nothing
                      [3, 4, 0],        # crosses the seam: vertex 0 wraps
                      [4, 6, 0],        # vertices 6 and 0 wrap (0 shares its duplicate)
                      [1, 2, 5],        # needs nothing (span 23/64)
                      [9, 8, 0],        # 63, 30, 2: vertices 8 and 0 wrap
                      [0, 5, 7],        # does not fit in half a turn (2, 33, 40 -> 0 wraps to 66: span 33/64 > 0.5)
                      [6, 0, 1],        # needs nothing
                      [0, 10, 1]], dtype=np.int32)        # 2, 34, 10: a span of exactly 0.5 -- nothing lies MORE than 0.5 below the largest
    st_ext, fvt = mesh.unwrap_seam(faces, st)
    assert fvt.dtype == np.int32 and fvt.shape == faces.shape and st_ext.shape[1] == 2 and st_ext.dtype == st.dtype
    assert np.array_equal(st_ext[:len(st)], st)
    assert np.array_equal(st_ext[fvt][..., 0] % 1.0, st[faces][..., 0]) and np.array_equal(st_ext[fvt][..., 1], st[faces][..., 1])
    assert len(st_ext) == len(st) + 3                                             # one duplicate each for vertices 0, 6 and 8
    for t in (0, 3, 6, 7):
        assert np.array_equal(fvt[t], faces[t])                                   # untouched triangles share the original indices
    assert fvt[1, 2] == fvt[2, 2] == fvt[4, 2] >= len(st) and fvt[2, 1] >= len(st) and fvt[2, 1] != fvt[2, 2]
    assert fvt[4, 0] == 9 and fvt[4, 1] >= len(st)
    s_tri = st[faces][..., 0]
    span_after = np.ptp(st_ext[fvt][..., 0], axis=1)
    for t in range(len(faces)):
        srt = np.sort(s_tri[t])
        gaps = np.append(np.diff(srt), srt[0] + 1 - srt[2])
        fits = 1 - gaps.max() <= 0.5                                              # the three lie on an arc of at most half a turn
        assert fits == (t != 5)
        if fits:
            assert span_after[t] <= 0.5, t
    # tensors in, numpy out; an empty mesh
    a, b = mesh.unwrap_seam(torch.from_numpy(faces), torch.from_numpy(st))
    assert np.array_equal(a, st_ext) and np.array_equal(b, fvt)
    a, b = mesh.unwrap_seam(np.zeros((0, 3), np.int32), np.zeros((0, 2), np.float32))
    assert a.shape == (0, 2) and b.shape == (0, 3)


def test_write_obj_round_trip(tmp_path):
    rng = np.random.RandomState(5)
    verts = rng.randn(7, 3).astype(np.float32)
    verts[0] = [np.nextafter(np.float32(1), np.float32(2)), np.float32(1e-30), np.float32(-123456.789)]
    st = rng.rand(9, 2).astype(np.float32)
    st[8, 0] += 1
    faces = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 0, 3]], dtype=np.int32)
    fvt = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 7], [8, 0, 3]], dtype=np.int32)
    tex = rng.randint(0, 256, (6, 10, 3)).astype(np.uint8)
    nrm = rng.randn(7, 3).astype(np.float32)
    path = str(tmp_path / "m.obj")
    mesh.write_obj(path, torch.from_numpy(verts), torch.from_numpy(faces), st, fvt, texture=tex, normals=nrm)
    got = Q.read_obj(path)
    assert np.array_equal(got["v"].view(np.uint32), verts.view(np.uint32)) and np.array_equal(got["vt"].view(np.uint32), st.view(np.uint32))
    assert np.array_equal(got["vn"].view(np.uint32), nrm.view(np.uint32))
    assert np.array_equal(got["f"], faces) and np.array_equal(got["f_vt"], fvt) and np.array_equal(got["f_vn"], faces)
    assert got["mtllib"] == "m.mtl" and got["usemtl"] == "atlas"
    mtl = Q.read_mtl(Q.sibling(path, ".mtl"))
    assert mtl["newmtl"] == "atlas" and mtl["map_Kd"] == "m.png"
    from PIL import Image
    back = np.asarray(Image.open(Q.sibling(path, ".png")))
    assert back.dtype == np.uint8 and np.array_equal(back, tex)
    # defaults: the vertices' own indices, no normals, no image
    plain = str(tmp_path / "plain.obj")
    mesh.write_obj(plain, verts, faces, st[:7])
    got = Q.read_obj(plain)
    assert np.array_equal(got["f_vt"], faces) and got["f_vn"] is None and got["vn"].shape == (0, 3)
    assert "map_Kd" not in Q.read_mtl(Q.sibling(plain, ".mtl")) and not os.path.exists(Q.sibling(plain, ".png"))
    # an empty mesh is a valid file
    empty = str(tmp_path / "empty.obj")
    mesh.write_obj(empty, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 2), np.float32), texture=tex)
    got = Q.read_obj(empty)
    assert got["v"].shape == (0, 3) and got["f"].shape == (0, 3) and got["vt"].shape == (0, 2) and got["mtllib"] == "empty.mtl"
    with pytest.raises(ValueError):
        mesh.write_obj(plain, verts, faces, st[:5])                               # a corner points past st
    with pytest.raises(ValueError):
        mesh.write_obj(plain, verts, faces, st, texture=tex.astype(np.float32))


def test_query_kernels_use_no_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall", "-Wno-unused-function", "-save-temps", "-c"]
    p = subprocess.run([hipcc] + flags + [os.path.join(CSRC, "ngf_uv_query.hip"), "-o", "out.o"], cwd=tmp_path, capture_output=True, timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    text = open(tmp_path / "ngf_uv_query-hip-amdgcn-amd-amdhsa-gfx950.s").read()
    kernels = {m.group(1): int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
               for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)}
    # uv_query_kernel<GEO, GAUGE, TEX (0 none, 1 view, 2 diffuse), LATTICE>: GEO, GAUGE, GEO+GAUGE, GAUGE+TEX and GEO+GAUGE+TEX (TEX in both
    # colour modes) on a point list = 7, and GEO on the lattice
    want = {(1, 0, 0, 0), (0, 1, 0, 0), (1, 1, 0, 0), (0, 1, 1, 0), (0, 1, 2, 0), (1, 1, 1, 0), (1, 1, 2, 0), (1, 0, 0, 1)}
    got = set()
    for k in kernels:
        m = re.search(r"uv_query_kernelILb([01])ELb([01])ELi([0-2])ELb([01])EEE", k)
        assert m, k
        got.add(tuple(int(x) for x in m.groups()))
    assert got == want and len(kernels) == 8, sorted(kernels)
    assert all(v == 0 for v in kernels.values()), {k: v for k, v in kernels.items() if v}
    assert "v_mfma_f32_16x16x4" in text
    assert not re.search(r"\b(global|flat|buffer)_atomic", text)


@pytest.mark.parametrize("prim", Q.PRIMS)
def test_cpu_model_refuses(prim, tmp_path):
    net = uvmapping.NeuTex(primitive_type=prim, device="cpu")
    for call in (lambda: net.query(torch.zeros(4, 3), [0, 0, 1]), lambda: net.query(torch.zeros(4, 3), want=("sigma",)),
                 lambda: net.density_lattice(5), lambda: net.export_mesh(level=0.5, resolution=5),
                 lambda: net.export_mesh(str(tmp_path / "m.obj"), level=0.5, resolution=5)):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    assert not os.listdir(tmp_path)
