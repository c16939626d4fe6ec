"""CPU checks of the UV-Mapping (NeuTex) texture export: the new C-ABI symbol is exported by both libraries and refuses bad arguments without
a GPU, the Python point builders and merge_cube_to_single_texture reproduce the reference's own (tests/golden/uv_export.npz) bit for bit, the
fp64 torch restatement (tests/uv_export_eager.py) reproduces the reference's fp64 outputs, the new translation unit's kernels use no
scratch, and a CPU model refuses to export."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ngf_amd  # noqa: F401
from ngf_amd import _lib, uvmapping
import uv_export_eager as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-gauge-fields_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
G = np.load(os.path.join(GOLDEN, "uv_export.npz"))
G_EDIT = np.load(os.path.join(GOLDEN, "uv_edit.npz"))


def test_texture_eval_symbol_is_exported_by_both_libraries():
    hdr = open(os.path.join(ROOT, "include", "ngf.h")).read()
    assert re.search(r"\bngf_uv_texture_eval\s*\(", hdr) and "NGF_UV_TEX_DIFFUSE" in hdr
    assert "ngf_uv_texture_eval" in _lib.SYMBOLS
    assert hasattr(_lib.lib(), "ngf_uv_texture_eval")
    with _lib.library("exp") as X:
        assert hasattr(X, "ngf_uv_texture_eval")
    assert _lib.lib().ngf_abi_version() == 5


def test_texture_eval_refuses_bad_arguments_without_a_gpu():
    L = _lib.lib()
    buf = (C.c_float * 6)()
    p = C.cast(buf, C.c_void_p)
    fake = C.c_void_p(C.addressof(buf))           # never dereferenced: every call below fails on an argument check first
    assert L.ngf_uv_texture_eval(None, p, p, 0, 1, 0, p, None) == 1
    assert b"ngf_uv_texture_eval" in L.ngf_last_error()
    assert L.ngf_uv_texture_eval(fake, None, p, 0, 1, 0, p, None) == 1
    assert L.ngf_uv_texture_eval(fake, p, p, 0, 1, 0, None, None) == 1
    assert L.ngf_uv_texture_eval(fake, p, None, 0, 1, 0, p, None) == 1                    # view mode without a direction
    assert L.ngf_uv_texture_eval(fake, p, p, 2, 1, 0, p, None) == 1                       # stride neither 0 nor 3
    assert b"view_stride" in L.ngf_last_error()
    assert L.ngf_uv_texture_eval(fake, p, p, 0, -1, 0, p, None) == 1
    assert L.ngf_uv_texture_eval(fake, p, p, 0, 1, 2, p, None) == 1                       # unknown flag bit
    assert L.ngf_uv_texture_eval(fake, p, None, 0, 0, _lib.UV_TEX_DIFFUSE, p, None) == 0  # nothing to do: no launch


@pytest.mark.parametrize("prim,kind,R", E.POINT_SETS)
def test_point_builders_equal_the_reference_points_bit_for_bit(prim, kind, R):
    got = E.build_points(kind, R)
    want = G[E.points_key(prim, kind, R)]
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("rotate", [1, 0])
def test_merge_cube_equals_the_reference(rotate):
    cube = torch.from_numpy(G["sphere.cube32.view.f32"])
    got = uvmapping.merge_cube_to_single_texture(cube, rotate=bool(rotate))
    assert np.array_equal(got.numpy(), G[f"merge.rotate{rotate}"])
    assert tuple(uvmapping.merge_cube_to_single_texture(cube, flip=False).shape) == (96, 128, 3)
    assert not torch.equal(uvmapping.merge_cube_to_single_texture(cube, flip=False), got)


@pytest.mark.parametrize("case", E.CASES, ids=[c[0] for c in E.CASES])
def test_fp64_restatement_matches_the_reference_fp64_fixture(case):
    key, prim, kind, R, viewdir, with_edit = case
    net = E.make_net(prim, "cpu", torch.float64)
    pts = E.build_points(kind, R).double()
    view = None if viewdir is None else torch.tensor(viewdir).float().double()
    tex = torch.from_numpy(E.edit_texture(G_EDIT, prim)) if with_edit else None
    with torch.no_grad():
        got = E.texture_forward(net.net_texture, pts, view, tex, 1)
    if kind == "equi":
        got = got.flip(0)
    want = G[key + ".f64"]
    assert got.dtype == torch.float64 and tuple(got.shape) == want.shape
    assert float(np.abs(got.numpy() - want).max()) <= 1e-12


def test_export_kernels_use_no_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall", "-Wno-unused-function", "-save-temps", "-c"]
    p = subprocess.run([hipcc] + flags + [os.path.join(CSRC, "ngf_uv_export.hip"), "-o", "out.o"], cwd=tmp_path, capture_output=True, timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    text = open(tmp_path / "ngf_uv_export-hip-amdgcn-amd-amdhsa-gfx950.s").read()
    kernels = {m.group(1): int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
               for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)}
    assert len([k for k in kernels if "uv_texture_eval_kernel" in k]) == 2, sorted(kernels)         # view and diffuse
    assert all(v == 0 for v in kernels.values()), {k: v for k, v in kernels.items() if v}
    assert "v_mfma_f32_16x16x4" in text
    assert not re.search(r"\b(global|flat|buffer)_atomic", text)


@pytest.mark.parametrize("prim", ["sphere", "square"])
def test_cpu_model_refuses_to_export(prim):
    net = uvmapping.NeuTex(primitive_type=prim, device="cpu")
    for call in (lambda: net.net_texture.export_textures(8), lambda: net.net_texture.export_textures(8, None),
                 lambda: net.net_texture._export_sphere(8, [0, 0, 1]), lambda: net.texture_colors(torch.zeros(4, 3), [0, 0, 1])):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()


def test_decoder_back_reference_adds_no_state_and_survives_a_copy():
    import copy
    net = uvmapping.NeuTex(primitive_type="sphere", device="cpu")
    keys = set(net.state_dict())
    assert not any("_owner" in k or "_points" in k for k in keys)
    assert len(list(net.net_texture.parameters())) == 24 and not list(net.net_texture.buffers())
    fresh = uvmapping.NeuTex(primitive_type="sphere", device="cpu")
    fresh.load_state_dict(net.state_dict(), strict=True)
    assert net.net_texture._owner() is net
    twin = copy.deepcopy(net)
    assert twin.net_texture._owner() is twin
