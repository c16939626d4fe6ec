"""CPU checks of the InfoInv training path: the new C-ABI symbols are exported by both libraries, the descriptor layout matches, the opt-in
switch stays out of the checkpoint, density_L1 of an InfoInv field is the reference's expression, and the new translation unit's kernels use
no scratch (checked on -save-temps assembly, as tests/test_isa_lint.py does for the other units)."""
import os
import re
import subprocess

import pytest
import torch

import ngf_amd  # noqa: F401
from ngf_amd import _lib, infoinv, infoinv_train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-gauge-fields_amd", "csrc")
NEW = ["ngf_infoinv_trainer_create", "ngf_infoinv_trainer_destroy", "ngf_infoinv_trainer_bytes", "ngf_sizeof_infoinv_train_desc",
       "ngf_infoinv_train_forward", "ngf_infoinv_train_backward_grad", "ngf_infoinv_train_get_grads", "ngf_infoinv_train_params_changed"]


def test_infoinv_trainer_symbols_are_exported_by_both_libraries():
    hdr = open(os.path.join(ROOT, "include", "ngf.h")).read()
    for s in NEW:
        assert re.search(r"\b" + s + r"\s*\(", hdr) and s in _lib.SYMBOLS, s
    L = _lib.lib()
    assert all(hasattr(L, s) for s in NEW)
    infoinv_train._bind(L)                   # checks sizeof(ngf_infoinv_train_desc) against the ctypes mirror
    with _lib.library("exp") as X:
        assert all(hasattr(X, s) for s in NEW)
        infoinv_train._bind(X)


def test_infoinv_trainer_refuses_bad_arguments_without_a_gpu():
    import ctypes as C
    L = _lib.lib()
    infoinv_train._bind(L)
    out = C.c_void_p()
    assert L.ngf_infoinv_trainer_create(None, C.byref(out), None) == 1
    assert L.ngf_infoinv_train_backward_grad(None, 1, None, None) == 1
    assert L.ngf_infoinv_train_forward(None, None, None, 0, 0, 0, 0, None, None, None, None) == 1


def test_differentiable_switch_defaults_off_and_stays_out_of_save(tmp_path):
    aabb = torch.tensor([[-1.5] * 3, [1.5] * 3])
    f = infoinv.TriPlane(aabb, [16, 16, 16], "cpu", step_ratio=0.5)
    assert f.differentiable is False
    f.differentiable = True
    p = str(tmp_path / "ck.th")
    f.save(p)
    ck = torch.load(p, weights_only=False)
    assert "differentiable" not in ck["kwargs"] and not any("differentiable" in k for k in ck["state_dict"])


def test_density_l1_of_an_infoinv_field_matches_torch_on_cpu():
    aabb = torch.tensor([[-1.5] * 3, [1.5] * 3])
    f = infoinv.TriPlane(aabb, [16, 16, 16], "cpu", step_ratio=0.5)
    f.plane_yz = torch.nn.Parameter(torch.randn(1, 96, 7, 9))            # any plane size
    l1 = f.density_L1()
    l1.backward()
    planes = [p.detach().clone().requires_grad_(True) for p in (f.plane_xy, f.plane_yz, f.plane_xz)]
    want = sum(torch.mean(torch.abs(p)) for p in planes)
    want.backward()
    assert torch.allclose(l1.detach(), want.detach(), rtol=1e-6, atol=0)
    for p, q in zip((f.plane_xy, f.plane_yz, f.plane_xz), planes):
        assert torch.equal(p.grad, q.grad)


def test_infoinv_training_kernels_use_no_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall", "-Wno-unused-function", "-save-temps", "-c"]
    p = subprocess.run([hipcc] + flags + [os.path.join(CSRC, "ngf_infoinv_train.hip"), "-o", "out.o"], cwd=tmp_path, capture_output=True,
                       timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    text = open(tmp_path / "ngf_infoinv_train-hip-amdgcn-amd-amdhsa-gfx950.s").read()
    kernels = {m.group(1): int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
               for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)}
    assert len([k for k in kernels if "ii_" in k]) >= 15, sorted(kernels)
    assert all(v == 0 for v in kernels.values()), {k: v for k, v in kernels.items() if v}
