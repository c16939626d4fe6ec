"""CPU checks of the mesh export (marching cubes over a dense volume): the case table is regenerated and compared with
the committed header; its 256 cases use every crossing edge, hold at most 5 triangles and draw no diagonal inside a cube face; through the
numpy restatement (tests/mesh_ref.py) random {0,1} volumes are closed and consistently oriented and a ball has Euler characteristic 2 and
outward orientation; the C-ABI symbols are exported by both libraries and refuse bad arguments without a GPU; the PLY writer round-trips;
convert_sdf_samples_to_ply's point arithmetic is the reference's; a CPU field or tensor raises; the unit's kernels use no scratch.

The one refusal of ngf.h that needs a device -- nv / nt that are in range but differ from what count left in the workspace, which lives in device
memory -- is in tests/test_gpu_mesh.py; here nv / nt are refused where they cannot be the counts of ANY volume of those dims."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ngf_amd  # noqa: F401
from ngf_amd import _lib, mesh, mesh_table, triplane
import mesh_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-gauge-fields_amd", "csrc")
NAMES = ["ngf_mesh_workspace_bytes", "ngf_mesh_count", "ngf_mesh_emit", "ngf_debug_mesh_scan"]


def test_regenerated_table_equals_the_committed_header():
    assert mesh_table.header_text() == open(os.path.join(CSRC, "ngf_mesh_table.hpp")).read()
    loops, tris = mesh_table.build()
    assert loops == mesh_table.LOOPS and tris == mesh_table.TRIS


def test_every_case_uses_its_crossing_edges_in_at_most_five_triangles_without_in_face_diagonals():
    n_loops = n_tris = 0
    for case in range(256):
        crossing = {e for e, (c0, c1) in enumerate(mesh_table.EDGE_CORNERS) if (case >> c0 & 1) != (case >> c1 & 1)}
        loops, tris = mesh_table.LOOPS[case], mesh_table.TRIS[case]
        assert sorted(e for loop in loops for e in loop) == sorted(crossing)          # every crossing edge in exactly one loop
        assert {e for tri in tris for e in tri} == crossing
        assert len(tris) == sum(len(loop) - 2 for loop in loops) <= 5 == mesh_table.MAX_TRIS
        sides = {frozenset((loop[i], loop[(i + 1) % len(loop)])) for loop in loops for i in range(len(loop))}
        for tri in tris:
            for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
                assert frozenset((a, b)) in sides or not mesh_table.in_face(a, b), (case, tri)
        n_loops += len(loops)
        n_tris += len(tris)
    assert (n_loops, n_tris) == (358, 820)


def test_random_binary_volumes_are_closed_and_consistently_oriented():
    rng = np.random.default_rng(7)
    for _ in range(60):
        v = np.zeros((9, 8, 7), np.float32)
        v[1:-1, 1:-1, 1:-1] = rng.integers(0, 2, (7, 6, 5))
        verts, faces = R.marching_cubes_ref(v, 0.5)
        assert faces.shape[0] > 0 and R.closed_and_oriented(faces)
        assert len(np.unique(faces)) == verts.shape[0]
        _, flipped = R.marching_cubes_ref(v, 0.5, flip=True)
        assert np.array_equal(flipped, faces[:, ::-1])


def test_ball_has_euler_characteristic_two_and_outward_orientation():
    r = 6.3
    verts, faces, normals = R.marching_cubes_ref(R.ball((20, 18, 22), r), 0.0, normals=True)
    assert R.closed_and_oriented(faces) and R.euler_characteristic(faces) == 2
    vol = R.signed_volume(verts, faces)
    assert 0.95 * 4 / 3 * np.pi * r ** 3 < vol < 4 / 3 * np.pi * r ** 3               # inscribed in the ball, normals outward
    d = verts - np.array([9.5, 8.5, 10.5], np.float32)
    assert np.abs(np.linalg.norm(d, axis=1) - r).max() <= 1.0                         # 1-Lipschitz: a vertex within one edge length
    assert (normals * d).sum(1).min() > 0


def test_symbols_are_declared_bound_and_exported_by_both_libraries():
    hdr = open(os.path.join(ROOT, "include", "ngf.h")).read()
    for s in NAMES:
        assert re.search(r"\b%s\s*\(" % s, hdr) and s in _lib.SYMBOLS and hasattr(_lib.lib(), s), s
    assert "NGF_MESH_FLIP = 1" in hdr and "NGF_MESH_NORMALS = 2" in hdr and (_lib.MESH_FLIP, _lib.MESH_NORMALS) == (1, 2)
    with _lib.library("exp") as X:
        assert all(hasattr(X, s) for s in NAMES) and X.ngf_abi_version() == 5
    assert _lib.lib().ngf_abi_version() == 5


def test_workspace_stays_within_eight_bytes_per_lattice_point():
    L = _lib.lib()
    for shape in ((2, 2, 2), (4, 4, 4), (5, 7, 9), (64, 64, 64), (65, 37, 109), (256, 256, 256), (512, 512, 512), (1, 5, 5)):
        n = shape[0] * shape[1] * shape[2]
        assert 0 < L.ngf_mesh_workspace_bytes(*shape) <= max(8 * n, 512), shape
    assert L.ngf_mesh_workspace_bytes(894, 894, 894) > 0                                # 3 n = 2 143 550 952 < 2^31
    assert L.ngf_mesh_workspace_bytes(895, 895, 895) == -1                              # 3 n >= 2^31
    assert L.ngf_mesh_workspace_bytes(65536, 65536, 65536) == -1
    assert L.ngf_mesh_workspace_bytes(0, 4, 4) == -1 and L.ngf_mesh_workspace_bytes(4, 4, -1) == -1


def _args(dims=(4, 4, 4), strides=(16, 4, 1)):
    return (C.c_int32 * 3)(*dims), (C.c_int64 * 3)(*strides)


def test_count_and_emit_refuse_bad_arguments_without_a_gpu():
    L = _lib.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)              # never dereferenced: every call below fails on an argument check first
    dims, strides = _args()
    big = 1 << 20
    ok_count = [p, dims, strides, C.c_float(0.5), p, big, p, None]
    org, sp = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    ok_emit = [p, dims, strides, C.c_float(0.5), org, sp, 0, p, big, 1, 1, p, None, p, None]

    def refused(fn, ok, k, value, code=1, word=None):
        a = list(ok)
        a[k] = value
        assert fn(*a) == code, (fn.__name__, k)
        msg = L.ngf_last_error()
        assert fn.__name__.encode() in msg and (word is None or word in msg), msg

    for fn, ok, nulls in ((L.ngf_mesh_count, ok_count, (0, 1, 2, 4, 6)), (L.ngf_mesh_emit, ok_emit, (0, 1, 2, 4, 5, 7, 11, 13))):
        for k in nulls:
            refused(fn, ok, k, None, word=b"null")
        refused(fn, ok, 1, _args(dims=(4, 0, 4))[0], word=b"dims[1]")
        refused(fn, ok, 1, _args(dims=(-1, 4, 4))[0], word=b"dims[0]")
        refused(fn, ok, 2, _args(strides=(16, 4, 0))[1], word=b"strides[2]")
        for bad in (float("nan"), float("inf"), -float("inf")):
            refused(fn, ok, 3, C.c_float(bad), word=b"level")
        refused(fn, ok, 1, _args(dims=(895, 895, 895))[0], code=3, word=b"2^31")
    refused(L.ngf_mesh_count, ok_count, 5, L.ngf_mesh_workspace_bytes(4, 4, 4) - 1, word=b"workspace")
    refused(L.ngf_mesh_emit, ok_emit, 8, L.ngf_mesh_workspace_bytes(4, 4, 4) - 1, word=b"workspace")
    refused(L.ngf_mesh_emit, ok_emit, 6, 4, word=b"flags")
    refused(L.ngf_mesh_emit, ok_emit, 6, -1, word=b"flags")
    a = list(ok_emit)
    a[6] = _lib.MESH_NORMALS                 # normals asked for, no buffer
    assert L.ngf_mesh_emit(*a) == 1 and b"null" in L.ngf_last_error()
    for k, value in ((9, -1), (10, -1), (9, 3 * 64 + 1), (10, 5 * 64 + 1)):
        refused(L.ngf_mesh_emit, ok_emit, k, value, word=b"counts")
    a = list(ok_emit)
    a[1], a[9], a[10] = _args(dims=(1, 4, 4))[0], 1, 0          # no cells: any non-zero count is wrong ...
    assert L.ngf_mesh_emit(*a) == 1
    a[9] = 0                                                    # ... and the empty mesh is not an error (nothing is launched)
    assert L.ngf_mesh_emit(*a) == 0
    assert L.ngf_debug_mesh_scan(None, 4, p, 8, p, None) == 1 and L.ngf_debug_mesh_scan(p, 0, p, 8, p, None) == 1
    assert L.ngf_debug_mesh_scan(p, 1 << 21, p, 8, p, None) == 1 and b"scratch" in L.ngf_last_error()


def test_ply_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    verts = rng.standard_normal((37, 3)).astype(np.float32)
    faces = rng.integers(0, 37, (51, 3)).astype(np.int32)
    path = str(tmp_path / "m.ply")
    mesh.write_ply(path, verts, faces)
    v, f = R.read_ply(path)
    assert v.dtype == np.float32 and f.dtype == np.int32
    assert np.array_equal(v.view(np.uint32), verts.view(np.uint32)) and np.array_equal(f, faces)
    head = open(path, "rb").read(200).split(b"end_header\n")[0].decode().split("\n")
    assert head[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 37"] and "element face 51" in head
    mesh.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    v, f = R.read_ply(path)
    assert v.shape == (0, 3) and f.shape == (0, 3)


def test_convert_sdf_samples_point_arithmetic_is_the_reference_s():
    verts = np.array([[0.5, 1.25, 2.0], [3.0, 0.0, 0.125], [0.1, 0.2, 0.3]], np.float32)
    bbox = np.array([[-1.5, -1.0, 0.25], [1.5, 2.0, 3.0]], np.float32)
    # TriPlane/utils.py:206-217 by hand
    want = np.zeros_like(verts)
    for k in range(3):
        want[:, k] = bbox[0, k] + verts[:, k]
    assert np.array_equal(mesh.mesh_points(verts, bbox), want)
    offset = np.array([0.5, -0.25, 1.0])
    assert np.array_equal(mesh.mesh_points(verts, bbox, offset=offset, scale=2.0), want / 2.0 - offset)
    assert np.array_equal(mesh.mesh_points(verts, bbox, scale=3.0), want / 3.0)
    assert np.array_equal(mesh.mesh_points(verts, bbox, offset=offset), want - offset)
    assert mesh.mesh_points(verts, bbox).dtype == np.float32


def test_cpu_field_and_cpu_tensor_raise(tmp_path):
    f = triplane.TriPlane(torch.tensor([[-1.5] * 3, [1.5] * 3]), [16] * 3, "cpu", near_far=[2.0, 6.0], step_ratio=0.5)
    with pytest.raises(RuntimeError, match="GPU only"):
        f.export_mesh(gridSize=(8, 8, 8))
    with pytest.raises(RuntimeError, match="GPU only"):
        mesh.marching_cubes(torch.zeros(4, 4, 4), 0.5)
    with pytest.raises(RuntimeError, match="GPU only"):
        mesh.convert_sdf_samples_to_ply(torch.zeros(4, 4, 4), str(tmp_path / "x.ply"), np.array([[0.0] * 3, [1.0] * 3]))
    with pytest.raises(ValueError):
        mesh.marching_cubes(torch.zeros(4, 4), 0.5)


def test_mesh_kernels_use_no_scratch_and_never_wait_for_another_workgroup(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall", "-Wno-unused-function", "-save-temps", "-c"]
    p = subprocess.run([hipcc] + flags + [os.path.join(CSRC, "ngf_mesh.hip"), "-o", "out.o"], cwd=tmp_path, capture_output=True, timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    text = open(tmp_path / "ngf_mesh-hip-amdgcn-amd-amdhsa-gfx950.s").read()
    kernels = {m.group(1): int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
               for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)}
    for name in ("mesh_classify_tiles_kernel", "mesh_scan_chunks_kernel", "mesh_scan_add_kernel", "mesh_apply_kernel", "mesh_header_kernel"):
        assert len([k for k in kernels if name in k]) == 1, sorted(kernels)
    assert len([k for k in kernels if "mesh_count_kernel" in k]) == 2, sorted(kernels)                # classifying, or summing the tiles' words
    assert len([k for k in kernels if "mesh_emit_kernel" in k]) == 2, sorted(kernels)                 # with and without normals
    assert len(kernels) == 9 and all(v == 0 for v in kernels.values()), kernels
    assert not re.search(r"\b(global|flat|buffer)_atomic", text)                                      # nothing to spin on: no atomics at all
    src = open(os.path.join(CSRC, "ngf_mesh.hpp")).read() + open(os.path.join(CSRC, "ngf_mesh.hip")).read()
    assert "hipLaunchCooperativeKernel" not in src and "atomic" not in src and "while (" not in src.replace("while (sizes[l] >", "")
