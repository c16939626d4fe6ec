"""CPU checks of the inverse gauge on the GPU (include/ngf.h: ngf_uv_inverse_*): the three C-ABI symbols are exported by
both libraries and refuse bad arguments without a GPU; the torch restatement (tests/uv_inverse_eager.py) reproduces the reference's own outputs
(tests/golden/uv_inverse.npz); mesh.icosphere and mesh.square_template are the closed, oriented meshes they say they are; the new translation
unit's kernel uses no scratch; and a CPU model refuses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ngf_amd  # noqa: F401
from ngf_amd import _lib, mesh, uvmapping
import uv_inverse_eager as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-gauge-fields_amd", "csrc")
G = np.load(os.path.join(ROOT, "tests", "golden", "uv_inverse.npz"))
E_ARG = 1
NAMES = ("ngf_uv_inverse_create", "ngf_uv_inverse_destroy", "ngf_uv_inverse_map")


def test_inverse_symbols_are_exported_by_both_libraries():
    hdr = open(os.path.join(ROOT, "include", "ngf.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr)
        assert name in _lib.SYMBOLS
        assert hasattr(_lib.lib(), name)
        with _lib.library("exp") as X:
            assert hasattr(X, name)
    assert re.search(r"#define NGF_ABI_VERSION 5\b", hdr) and _lib.lib().ngf_abi_version() == 5
    assert re.search(r"#define NGF_UV_INVERSE_LAYERS 5\b", hdr) and _lib.UV_INVERSE_LAYERS == 5 and _lib.UV_LAYERS == 29
    # int32 input_dim, int32 pad, 5 + 5 pointers
    assert C.sizeof(_lib.UvInverseDesc) == 8 + 10 * C.sizeof(C.c_void_p)


def test_python_launch_constants_are_the_kernels():
    hpp = open(os.path.join(CSRC, "ngf_uv_inverse.hpp")).read()
    assert int(re.search(r"kUvInvTilePoints = (\d+);", hpp).group(1)) == uvmapping.INVERSE_TILE_POINTS
    assert int(re.search(r"kUvInvWaves = (\d+);", hpp).group(1)) == uvmapping.INVERSE_WAVES_PER_BLOCK


def test_map_refuses_bad_arguments_without_a_gpu():
    L = _lib.lib()
    buf = (C.c_float * 6)()
    p = C.cast(buf, C.c_void_p)
    fake = C.c_void_p(C.addressof(buf))           # never dereferenced: every call below ends on an argument check or on n == 0
    m = L.ngf_uv_inverse_map
    assert m(None, p, 1, p, None) == E_ARG
    assert b"ngf_uv_inverse_map" in L.ngf_last_error()
    assert m(fake, None, 1, p, None) == E_ARG
    assert b"ngf_uv_inverse_map" in L.ngf_last_error()
    assert m(fake, p, 1, None, None) == E_ARG
    assert m(fake, p, -1, p, None) == E_ARG
    assert b"ngf_uv_inverse_map" in L.ngf_last_error() and b"n=-1" in L.ngf_last_error()
    assert m(fake, p, 0, p, None) == 0                                           # n == 0: nothing to do, no launch
    assert L.ngf_uv_inverse_destroy(None) == 0


def test_create_refuses_bad_arguments_without_a_gpu():
    L = _lib.lib()
    buf = (C.c_float * 6)()
    out = C.c_void_p()
    d = _lib.UvInverseDesc()

    def fill(dim, skip=None):
        d.input_dim = dim
        for i in range(_lib.UV_INVERSE_LAYERS):
            d.w[i] = d.b[i] = C.addressof(buf)      # never dereferenced: every call below fails on an argument check first
        if skip is not None:
            (d.w if skip[0] == "w" else d.b)[skip[1]] = None

    c = L.ngf_uv_inverse_create
    fill(3)
    assert c(None, C.byref(out), None) == E_ARG
    assert b"ngf_uv_inverse_create" in L.ngf_last_error()
    assert c(C.byref(d), None, None) == E_ARG
    for dim in (0, 1, 4, -2, 63):
        fill(dim)
        out.value = 1
        assert c(C.byref(d), C.byref(out), None) == E_ARG, dim
        assert b"ngf_uv_inverse_create" in L.ngf_last_error() and b"input_dim" in L.ngf_last_error()
        assert out.value is None                                                 # a failed create leaves no handle behind
    for dim in (2, 3):
        for skip in [(k, i) for k in "wb" for i in range(_lib.UV_INVERSE_LAYERS)]:
            fill(dim, skip)
            assert c(C.byref(d), C.byref(out), None) == E_ARG, skip
            assert b"layer %d missing" % skip[1] in L.ngf_last_error()


def test_fixture_holds_the_points_of_the_helper_and_is_alive():
    assert tuple(G["seeds"]) == V.SEEDS
    for prim in V.PRIMS:
        uv = G[f"{prim}.uv"]
        assert uv.dtype == np.float32 and uv.shape == (V.N_POINTS, V.DIMS[prim])
        assert np.array_equal(uv.view(np.uint32), V.points(prim).view(np.uint32))
        for seed in V.SEEDS:
            act, top = G[f"{prim}.s{seed}.active"], float(G[f"{prim}.s{seed}.max_abs"])
            assert act.shape == (4,) and (act >= 0.2).all() and (act <= 0.8).all() and 0.1 <= top <= 10
            assert top == float(np.abs(G[f"{prim}.s{seed}.xyz.f64"]).max())
    sq = G["square.uv"]
    assert np.array_equal(sq[:9], V.PLACED_SQUARE) and (np.abs(sq[:4]) == 1).all() and (sq[4] == 0).all() and (np.abs(sq[5:9]).max(axis=1) > 1).all()
    assert np.abs(sq[9:]).max() <= 1
    sp = G["sphere.uv"]
    nrm = np.linalg.norm(sp.astype(np.float64), axis=1)
    assert np.array_equal(sp[:6], V.AXES) and np.allclose(nrm[6:9], 0.5, atol=1e-6) and np.allclose(nrm[9:12], 2, atol=1e-6)
    assert np.allclose(nrm[12:], 1, atol=1e-6)


@pytest.mark.parametrize("prim", V.PRIMS)
@pytest.mark.parametrize("seed", V.SEEDS)
def test_restatement_matches_the_reference_fixture(prim, seed):
    uv = torch.from_numpy(G[f"{prim}.uv"])
    with torch.no_grad():
        got32 = V.forward(V.weights(seed, prim), uv).numpy()
        got64 = V.forward(V.weights(seed, prim, torch.float64), uv.double()).numpy()
    assert got32.dtype == np.float32 and got64.dtype == np.float64
    e32 = float(np.abs(got32 - G[f"{prim}.s{seed}.xyz.f32"]).max())
    e64 = float(np.abs(got64 - G[f"{prim}.s{seed}.xyz.f64"]).max())
    print(f"{prim} seed {seed}: max|restatement - reference| fp32 {e32:.3e}, fp64 {e64:.3e}")
    assert e32 <= 1e-6 and e64 <= 1e-12


def test_drop_in_module_is_the_restatement():
    """uvmapping.InverseNetwork (what InverseGauge.map runs) on the synth weights under the reference's state-dict names."""
    for prim in V.PRIMS:
        net = V.make_net(prim, "cpu", V.SEEDS[1])
        uv = torch.from_numpy(G[f"{prim}.uv"])
        with torch.no_grad():
            assert torch.equal(net.inverse_gauge.map(uv), V.forward(V.weights(V.SEEDS[1], prim), uv))


@pytest.mark.parametrize("d", [0, 1, 2, 3])
def test_icosphere_is_a_closed_outward_unit_sphere(d):
    v, f = mesh.icosphere(d)
    assert v.dtype == np.float32 and f.dtype == np.int64
    assert v.shape == (10 * 4 ** d + 2, 3) and f.shape == (20 * 4 ** d, 3)
    assert f.min() == 0 and f.max() == len(v) - 1 and len(np.unique(f)) == len(v)
    nrm = np.linalg.norm(v.astype(np.float64), axis=1)
    ulp = float(np.spacing(np.float32(1)))
    assert np.abs(nrm - 1).max() <= 2 * ulp
    # every directed edge once, its reverse once: closed, consistently oriented, every edge shared by exactly two faces
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=0)
    directed = {(int(a), int(b)) for a, b in e}
    assert len(directed) == len(e) and all((b, a) in directed for a, b in directed) and all(a != b for a, b in directed)
    n_edges = len(e) // 2
    assert len(v) - n_edges + len(f) == 2
    p = v.astype(np.float64)[f]
    volume = float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6)
    assert 0 < volume <= 4 * np.pi / 3
    if d == 3:
        assert volume > 0.98 * 4 * np.pi / 3
    # a level keeps the vertices of the one before it
    if d:
        assert np.array_equal(v[:10 * 4 ** (d - 1) + 2], mesh.icosphere(d - 1)[0])


def test_icosphere_refuses_a_negative_division():
    with pytest.raises(ValueError):
        mesh.icosphere(-1)


@pytest.mark.parametrize("side", [2, 3, 50])
def test_square_template_is_the_references_grid(side):
    v, f = mesh.square_template(side)
    want = np.stack(np.meshgrid(*([np.linspace(-1, 1, side)] * 2), indexing="ij"), axis=-1).reshape((-1, 2))      # gauge_fields.py:141
    assert v.dtype == np.float32 and np.array_equal(v, torch.FloatTensor(want).numpy()) and np.array_equal(v, want.astype(np.float32))
    assert f.dtype == np.int64 and f.shape == (2 * (side - 1) ** 2, 3) and f.min() == 0 and f.max() == side * side - 1
    p = v.astype(np.float64)[f]
    a, b = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    area = (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]) / 2
    assert (area > 0).all() and abs(area.sum() - 4) <= 1e-6
    with pytest.raises(ValueError):
        mesh.square_template(1)


def test_inverse_kernel_uses_no_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall", "-Wno-unused-function", "-save-temps", "-c"]
    p = subprocess.run([hipcc] + flags + [os.path.join(CSRC, "ngf_uv_inverse.hip"), "-o", "out.o"], cwd=tmp_path, capture_output=True, timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    text = open(tmp_path / "ngf_uv_inverse-hip-amdgcn-amd-amdhsa-gfx950.s").read()
    for what in (r"; ScratchSize", r"\.sgpr_spill_count", r"\.vgpr_spill_count"):
        assert re.findall(r"%s: (\d+)" % what, text) == ["0"], what
    assert re.findall(r"; Occupancy: (\d+)", text) == ["1"]          # one wave per SIMD: 380 of the 512 registers a lane can have
    kernels = {m.group(1): int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
               for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)}
    assert len(kernels) == 1 and "uv_inverse_kernel" in next(iter(kernels)) and all(v == 0 for v in kernels.values()), kernels
    assert "v_mfma_f32_16x16x4" in text and not re.search(r"v_mfma\S*bf16", text)
    assert not re.search(r"\b(global|flat|buffer|ds)_atomic", text)


@pytest.mark.parametrize("prim", V.PRIMS)
def test_cpu_model_refuses(prim, tmp_path):
    net = uvmapping.NeuTex(primitive_type=prim, device="cpu")
    D = V.DIMS[prim]
    for call in (lambda: net.inverse_map(torch.zeros(4, D)), lambda: net.cycle_error(torch.zeros(4, 3)), lambda: net.coordinate_deformation(),
                 lambda: net.coordinate_deformation(str(tmp_path / "m.obj"), icosphere_division=1, side=3)):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    assert not os.listdir(tmp_path)
