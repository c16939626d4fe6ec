"""CPU checks of the fused InfoInv trainer (ngf_amd.infoinv_train.Trainer / fit; include/ngf.h: ngf_infoinv_train_step_backward, _set_moments,
_adam_all, _get_grad, _adam_ext): the symbols are exported by both libraries at ABI 5, bad arguments are refused without a GPU, the new kernels use
no scratch and the product kernel runs on the fp32 matrix pipe without fp64 FMAs (checked on -save-temps assembly), a CPU field is refused, and
``fit`` follows the schedule of InfoInv/main.py:243-336 (checked against a stub Trainer and a stub field)."""
import ctypes as C
import os
import re
import subprocess
import types

import pytest
import torch

import ngf_amd  # noqa: F401
from ngf_amd import _lib, geometry, infoinv, infoinv_train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-gauge-fields_amd", "csrc")
NEW = ["ngf_infoinv_train_step_backward", "ngf_infoinv_train_set_moments", "ngf_infoinv_train_adam_all", "ngf_infoinv_train_get_grad",
       "ngf_infoinv_train_adam_ext"]
NEW_KERNELS = ["ii_loss_kernel", "ii_mm_kernel", "ii_mm_reduce_kernel", "ii_plane_grad_add_kernel", "ii_adam_plane_kernel",
               "adam_dense_all_kernelILi13E"]          # the shared dense kernel (csrc/ngf_adam.hpp) at the thirteen decoder tensors


def test_fused_trainer_symbols_are_exported_by_both_libraries_at_abi_5():
    hdr = open(os.path.join(ROOT, "include", "ngf.h")).read()
    for s in NEW:
        assert re.search(r"\b" + s + r"\s*\(", hdr) and s in _lib.SYMBOLS, s
    L = _lib.lib()
    assert all(hasattr(L, s) for s in NEW)
    assert L.ngf_abi_version() == 5
    infoinv_train._bind(L)
    with _lib.library("exp") as X:
        assert all(hasattr(X, s) for s in NEW)
        assert X.ngf_abi_version() == 5
        infoinv_train._bind(X)


def test_fused_trainer_calls_refuse_bad_arguments_without_a_gpu():
    L = _lib.lib()
    infoinv_train._bind(L)
    sixteen = (C.c_void_p * 16)()
    counts, lrs = (C.c_int32 * 16)(), (C.c_float * 16)()
    assert L.ngf_infoinv_train_step_backward(None, None, None, None, 1, 1, 1, 1, None, None) == 1
    assert L.ngf_infoinv_train_set_moments(None, sixteen, sixteen) == 1
    assert L.ngf_infoinv_train_adam_all(None, counts, lrs, 0.9, 0.99, 1e-8, 8e-5, None) == 1
    assert L.ngf_infoinv_train_get_grad(None, 0, None, None) == 1
    assert L.ngf_infoinv_train_adam_ext(None, sixteen, sixteen, sixteen, counts, lrs, 0.9, 0.99, 1e-8, None) == 1
    assert b"null" in L.ngf_last_error()


def test_fused_kernels_use_no_scratch_and_the_product_runs_on_the_fp32_matrix_pipe(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall", "-Wno-unused-function", "-save-temps", "-c"]
    p = subprocess.run([hipcc] + flags + [os.path.join(CSRC, "ngf_infoinv_train.hip"), "-o", "out.o"], cwd=tmp_path, capture_output=True,
                       timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    text = open(tmp_path / "ngf_infoinv_train-hip-amdgcn-amd-amdhsa-gfx950.s").read()
    scratch = {m.group(1): int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
               for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)}
    for name in NEW_KERNELS:
        mine = {k: v for k, v in scratch.items() if name in k}
        assert mine, (name, sorted(scratch))
        assert all(v == 0 for v in mine.values()), mine
    # the body of the product kernel: from its label to its s_endpgm
    sym = next(k for k in scratch if "ii_mm_kernel" in k)
    body = text[text.index("\n" + sym + ":"):]
    body = body[:body.index("s_endpgm")]
    assert body.count("v_mfma_f32_16x16x4_f32") >= 32, body.count("v_mfma_f32_16x16x4_f32")       # 2 x 4 steps of up to four 16 x 16 sub-tiles
    assert "v_fma_f64" not in body and "v_mfma_f64" not in body and "v_mul_f64" not in body
    assert "scratch_" not in body and "buffer_store" not in body


def test_trainer_refuses_a_cpu_field():
    aabb = torch.tensor([[-1.5] * 3, [1.5] * 3])
    f = infoinv.TriPlane(aabb, [16, 16, 16], "cpu", step_ratio=0.5)
    with pytest.raises(RuntimeError, match="GPU only"):
        infoinv_train.Trainer(f)


class _StubField:
    device = "cpu"

    def __init__(self):
        self.gridSize = [32, 32, 32]
        self.log = []

    def filtering_rays(self, rays, rgbs, bbox_only=False, **kw):
        self.log.append(("filter", bool(bbox_only), int(rays.shape[0])))
        keep = rays.shape[0] if bbox_only else rays.shape[0] - 10
        return rays[:keep], rgbs[:keep]

    def updateAlphaMask(self, size, infoinv=True):
        self.log.append(("mask", tuple(size), bool(infoinv)))


def test_fit_follows_the_schedule_of_the_infoinv_loop(monkeypatch):
    made = []

    class StubTrainer:
        def __init__(self, field, **kw):
            self.kw, self.calls, self.released = kw, [], False
            made.append(self)

        def step(self, rays, rgb, N_samples=-1, white_bg=True, infoinv=True):
            self.calls.append((int(rays.shape[0]), int(N_samples), bool(white_bg), bool(infoinv)))
            return torch.tensor(0.01, dtype=torch.float64)

        def release(self):
            self.released = True

    monkeypatch.setattr(infoinv_train, "Trainer", StubTrainer)
    f = _StubField()
    args = types.SimpleNamespace(batch_size=8, n_iters=12, lr_init=0.02, lr_basis=1e-3, lr_decay_iters=-1, lr_decay_target_ratio=0.1,
                                 update_AlphaMask_list=[3, 7], nSamples=1000000, step_ratio=0.5)
    seen = []
    psnr = infoinv_train.fit(f, torch.zeros(64, 6), torch.zeros(64, 3), args, white_bg=False, infoinv=False,
                             on_iteration=lambda it, loss: seen.append(it))
    want_S = geometry.cal_n_samples([32, 32, 32], 0.5)
    assert len(psnr) == 12 and all(abs(p - 20.0) < 1e-9 for p in psnr) and seen == list(range(12))
    # one Trainer at the start, one after each mask update; every older one released, the last one too
    assert len(made) == 3 and all(t.released for t in made)
    assert [len(t.calls) for t in made] == [4, 4, 4]                      # iterations 0-3, 4-7, 8-11
    assert all(c == (8, want_S, False, False) for t in made for c in t.calls)
    assert all(t.kw["max_samples"] == want_S and t.kw["batch_size"] == 8 and t.kw["n_iters"] == 12 for t in made)
    # the L1 weight: 8e-5 until the first mask update, 4e-5 from then on; the optimiser state is carried
    assert [t.kw["L1_reg_weight"] for t in made] == [8e-5, 4e-5, 4e-5]
    assert made[0].kw["state_from"] is None and made[1].kw["state_from"] is made[0] and made[2].kw["state_from"] is made[1]
    # bbox filter first; both updates build a 256^3 mask with the loop's infoinv flag; only the first one filters the rays again
    assert f.log == [("filter", True, 64), ("mask", (256, 256, 256), False), ("filter", False, 64), ("mask", (256, 256, 256), False)]
