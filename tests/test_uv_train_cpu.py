"""CPU checks of UV-Mapping (NeuTex) training: the new C-ABI symbols are exported by both libraries and the descriptor layout matches its
ctypes mirror, bad arguments are refused without a GPU, the opt-in switch stays out of the checkpoint, the inverse gauge has the reference's
names and shapes, the fp64 torch restatement reproduces the reference's own fp64 numbers (tests/golden/uv_train_*.npz), and the new
translation unit's kernels use no scratch."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ngf_amd  # noqa: F401
from ngf_amd import _lib, uv_train, uvmapping
import uv_train_eager as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-gauge-fields_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ["ngf_uv_trainer_create", "ngf_uv_trainer_destroy", "ngf_uv_trainer_bytes", "ngf_sizeof_uv_train_desc", "ngf_uv_train_forward",
       "ngf_uv_train_backward", "ngf_uv_train_get_grads", "ngf_uv_train_params_changed"]

# gauge_fields.py:78-207: InverseGauge(...).inverse_network = InverseNetwork(D) with mid 64, hidden 512, two hidden layers
INVERSE = {"linear1.weight": (64, None), "linear1.bias": (64,), "linear2.weight": (512, 64), "linear2.bias": (512,),
           "linear_list.0.weight": (512, 512), "linear_list.0.bias": (512,), "linear_list.1.weight": (512, 512), "linear_list.1.bias": (512,),
           "last_linear.weight": (3, 512), "last_linear.bias": (3,)}


def test_uv_trainer_symbols_are_exported_by_both_libraries():
    hdr = open(os.path.join(ROOT, "include", "ngf.h")).read()
    for s in NEW:
        assert re.search(r"\b" + s + r"\s*\(", hdr) and s in _lib.SYMBOLS, s
    L = _lib.lib()
    assert all(hasattr(L, s) for s in NEW)
    uv_train._bind(L)                    # checks sizeof(ngf_uv_train_desc) against the ctypes mirror
    with _lib.library("exp") as X:
        assert all(hasattr(X, s) for s in NEW)
        uv_train._bind(X)


def test_uv_trainer_refuses_bad_arguments_without_a_gpu():
    import ctypes as C
    L = _lib.lib()
    uv_train._bind(L)
    out = C.c_void_p()
    assert L.ngf_uv_trainer_create(None, C.byref(out), None) == 1
    d = uv_train.UvTrainDesc()
    d.max_rays, d.max_samples = 0, 64
    assert L.ngf_uv_trainer_create(C.byref(d), C.byref(out), None) == 1
    d.max_rays, d.max_samples = 1 << 20, 1 << 10                 # rows past the 32-bit indexing
    assert L.ngf_uv_trainer_create(C.byref(d), C.byref(out), None) == 1
    assert L.ngf_uv_train_forward(None, None, None, None, None, 1, 1, 1, None, None, None, None, None, None, None) == 1
    assert L.ngf_uv_train_backward(None, 1, None, None, None, None, None) == 1
    assert L.ngf_uv_train_get_grads(None, None, None) == 1
    assert L.ngf_uv_train_params_changed(None) == 1
    assert L.ngf_uv_trainer_bytes(None) == 0


def test_differentiable_defaults_off_and_stays_out_of_state_dict(tmp_path):
    net = uvmapping.NeuTex(primitive_type="square", device="cpu")
    assert net.differentiable is False
    net.differentiable = True
    sd = net.state_dict()
    assert not any("differentiable" in k for k in sd)
    p = str(tmp_path / "net.pth")
    torch.save(sd, p)
    fresh = uvmapping.NeuTex(primitive_type="square", device="cpu")
    fresh.load_state_dict(torch.load(p), strict=True)
    assert fresh.differentiable is False


@pytest.mark.parametrize("prim,D", [("square", 2), ("sphere", 3)])
def test_inverse_gauge_names_and_shapes_match_the_reference(prim, D):
    net = uvmapping.NeuTex(primitive_type=prim, device="cpu")
    got = {k[len("inverse_gauge.inverse_network."):]: tuple(v.shape) for k, v in net.state_dict().items() if k.startswith("inverse_gauge.")}
    want = {k: tuple(D if s is None else s for s in v) for k, v in INVERSE.items()}
    assert got == want
    assert net.inverse_gauge.num_points_per_primitive == 2500
    assert uvmapping.NeuTex(primitive_type=prim, device="cpu", points_per_primitive=100).inverse_gauge.num_points_per_primitive == 100
    # the eval handle's key covers the 29 render layers only
    n_render = sum(2 for _ in net.layers())
    assert n_render == 58 and len(list(net.parameters())) == 58 + 10


@pytest.mark.parametrize("name", ["uv_train_square", "uv_train_sphere"])
def test_fp64_restatement_matches_the_reference_fp64_fixture(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    prim = str(g["primitive_type"])
    params = E.model_params(int(g["seed"]), prim)
    names = [str(n) for n in g["names"]]
    assert names == sorted(params)
    for k, want in zip(names, g["sums"]):
        assert abs(float(np.asarray(params[k], np.float64).sum()) - float(want)) <= 1e-6 * max(1.0, abs(float(want))), k
    net = E.make_net(params, prim, int(g["S"]), "cpu", torch.float64)
    t = lambda k: torch.from_numpy(g[k]).double()           # noqa: E731
    bg = t("bg") if g["bg"].size else None
    idx = E.fixture_idx(g)
    for tag, w in (("l0", (1.0, 1.0, 1.0, 0.0)), ("l1", (1.0, 1.0, 1.0, 1.0))):
        net.zero_grad()
        out = E.forward(net, t("campos"), t("raydir"), bg, t("U"), t("template"))
        loss = E.compute_loss(out, t("gt_image"), t("gt_trans"), w)
        loss.backward()
        assert abs(float(loss.detach()) - float(g[f"f64.{tag}.loss"])) <= 1e-9 * abs(float(g[f"f64.{tag}.loss"]))
        if tag == "l0":
            for k in ("color", "transmittance"):
                np.testing.assert_allclose(out[k].detach().numpy(), g[f"f64.{k}"], rtol=1e-9, atol=1e-12)
        ref = E.fixture_grads(g, "f64", tag)
        for k, p in net.named_parameters():
            gr = p.grad.numpy()
            n, vals, probe = ref[k]
            assert abs(float(np.linalg.norm(gr)) - n) <= 1e-9 * max(n, 1e-30), k
            np.testing.assert_allclose(gr.reshape(-1)[idx[k]], vals, rtol=1e-8, atol=1e-12 * max(n, 1e-30))
            np.testing.assert_allclose(E.probe_products(k, gr), probe, rtol=1e-8, atol=1e-10 * max(n, 1e-30))


def test_uv_training_kernels_use_no_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall", "-Wno-unused-function", "-save-temps", "-c"]
    p = subprocess.run([hipcc] + flags + [os.path.join(CSRC, "ngf_uv_train.hip"), "-o", "out.o"], cwd=tmp_path, capture_output=True, timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    text = open(tmp_path / "ngf_uv_train-hip-amdgcn-amd-amdhsa-gfx950.s").read()
    kernels = {m.group(1): int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
               for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)}
    assert len([k for k in kernels if "uvt_" in k]) >= 12, sorted(kernels)
    assert all(v == 0 for v in kernels.values()), {k: v for k, v in kernels.items() if v}
    assert "v_mfma_f32_16x16x4" in text
