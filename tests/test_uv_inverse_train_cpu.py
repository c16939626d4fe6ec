"""CPU checks of the inverse gauge's training unit (include/ngf.h: ngf_uv_inverse_trainer_*, ngf_uv_inverse_train_*):
the symbols are exported by both libraries and refuse bad arguments without a GPU; no kernel of the unit uses scratch or spills; a CPU model with
``differentiable`` set falls back to the torch code; engines are not state; the fixture (tests/golden/uv_inverse_train.npz, the reference module's
own gradients) keeps its points within the cap and the torch restatement reproduces it."""
import copy
import ctypes as C
import os
import pickle
import re
import subprocess

import numpy as np
import pytest
import torch

import ngf_amd  # noqa: F401
from ngf_amd import _lib, uv_inverse_train, uvmapping
import uv_inverse_eager as V
import uv_inverse_train_eager as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-gauge-fields_amd", "csrc")
G = np.load(os.path.join(ROOT, "tests", "golden", "uv_inverse_train.npz"))
E_ARG = 1
SEED = {"sphere": 71, "square": 72}
NAMES = ("ngf_uv_inverse_trainer_create", "ngf_uv_inverse_trainer_destroy", "ngf_uv_inverse_trainer_bytes", "ngf_uv_inverse_train_params_changed",
         "ngf_uv_inverse_train_forward", "ngf_uv_inverse_train_backward", "ngf_uv_inverse_train_get_grads", "ngf_debug_uv_inverse_train_dx")


def test_symbols_are_exported_by_both_libraries_and_declared():
    hdr = open(os.path.join(ROOT, "include", "ngf.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS
        assert hasattr(_lib.lib(), name)
        with _lib.library("exp") as X:
            assert hasattr(X, name)
    assert re.search(r"#define NGF_ABI_VERSION 5\b", hdr) and _lib.lib().ngf_abi_version() == 5
    assert re.search(r"#define NGF_UV_INVERSE_TRAIN_PARAMS \(2 \* NGF_UV_INVERSE_LAYERS\)", hdr) and uv_inverse_train.NPARAMS == 10
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^REST\s*=.*\bngf_uv_inverse_train\b", mk, re.M)


def test_bad_arguments_are_refused_without_a_gpu():
    L = _lib.lib()
    uv_inverse_train._bind(L)
    buf = (C.c_float * 8)()
    p = C.cast(buf, C.c_void_p)
    fake = C.c_void_p(C.addressof(buf))           # never dereferenced: every call below ends on a null or a sign check
    tk = C.c_int64(0)
    f, b, g = L.ngf_uv_inverse_train_forward, L.ngf_uv_inverse_train_backward, L.ngf_uv_inverse_train_get_grads
    for args in ((None, p, 1, p, C.byref(tk), None), (fake, None, 1, p, C.byref(tk), None), (fake, p, 1, None, C.byref(tk), None),
                 (fake, p, 1, p, None, None), (fake, p, -1, p, C.byref(tk), None)):
        assert f(*args) == E_ARG
        assert b"ngf_uv_inverse_train_forward" in L.ngf_last_error()
    assert b"n=-1" in L.ngf_last_error()
    assert b(None, 1, p, p, None) == E_ARG and b"ngf_uv_inverse_train_backward" in L.ngf_last_error()
    assert b(fake, 1, None, p, None) == E_ARG and b"d_xyz" in L.ngf_last_error()
    dx = L.ngf_debug_uv_inverse_train_dx
    assert dx(None, 1, p, p, None) == E_ARG and b"ngf_debug_uv_inverse_train_dx" in L.ngf_last_error()
    assert dx(fake, 1, None, p, None) == E_ARG and b"d_xyz" in L.ngf_last_error()
    assert g(None, p, None) == E_ARG and g(fake, None, None) == E_ARG
    assert L.ngf_uv_inverse_train_params_changed(None) == E_ARG
    assert L.ngf_uv_inverse_trainer_destroy(None) == 0 and L.ngf_uv_inverse_trainer_bytes(None) == 0
    out = C.c_void_p()
    d = _lib.UvInverseDesc()

    def fill(dim, skip=None):
        d.input_dim = dim
        for i in range(_lib.UV_INVERSE_LAYERS):
            d.w[i] = d.b[i] = C.addressof(buf)
        if skip is not None:
            (d.w if skip[0] == "w" else d.b)[skip[1]] = None

    c = L.ngf_uv_inverse_trainer_create
    fill(3)
    assert c(None, 16, C.byref(out), None) == E_ARG and c(C.byref(d), 16, None, None) == E_ARG
    for dim in (0, 1, 4, -2):
        fill(dim)
        out.value = 1
        assert c(C.byref(d), 16, C.byref(out), None) == E_ARG and b"input_dim" in L.ngf_last_error()
        assert out.value is None
    for skip in [(k, i) for k in "wb" for i in range(_lib.UV_INVERSE_LAYERS)]:
        fill(2, skip)
        assert c(C.byref(d), 16, C.byref(out), None) == E_ARG and b"layer %d missing" % skip[1] in L.ngf_last_error()
    fill(3)
    for n in (0, -1, 1 << 27):
        assert c(C.byref(d), n, C.byref(out), None) == E_ARG and b"max_points" in L.ngf_last_error()


def test_no_kernel_of_the_unit_uses_scratch_or_spills(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall", "-Wno-unused-function", "-save-temps", "-c"]
    p = subprocess.run([hipcc] + flags + [os.path.join(CSRC, "ngf_uv_inverse_train.hip"), "-o", "out.o"], cwd=tmp_path, capture_output=True, timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    text = open(tmp_path / "ngf_uv_inverse_train-hip-amdgcn-amd-amdhsa-gfx950.s").read()
    kernels = {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)}
    want = ("uvit_pack_kernel", "uvit_forward_kernel", "uvit_dx_kernel", "uvit_dw_kernel", "uvit_reduce_kernel")
    assert len(kernels) == 8 and all(any(w in k for k in kernels) for w in want), sorted(kernels)          # the dW kernel in four load forms
    assert all(int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0 for body in kernels.values())
    for what in (r"; ScratchSize", r"\.sgpr_spill_count", r"\.vgpr_spill_count"):
        assert set(re.findall(r"%s: (\d+)" % what, text)) == {"0"}, what
    # the two tile kernels: one wave per SIMD, as the forward they restate; LDS is dynamic (128 KB, set at the launch)
    occ = dict(zip(re.findall(r"^(_ZN3ngf\w+):", text, re.M), re.findall(r"; Occupancy: (\d+)", text)))
    assert [v for k, v in occ.items() if "uvit_forward_kernel" in k or "uvit_dx_kernel" in k] == ["1", "1"], occ
    assert "v_mfma_f32_16x16x4" in text and not re.search(r"v_mfma\S*bf16", text)
    assert not re.search(r"\b(global|flat|buffer|ds)_atomic", text)


@pytest.mark.parametrize("prim", V.PRIMS)
def test_a_cpu_model_with_the_flag_set_runs_the_torch_code(prim):
    net = V.make_net(prim, "cpu", V.SEEDS[1])
    g = net.inverse_gauge
    uv = torch.from_numpy(V.points(prim))
    assert g.differentiable is False and uvmapping.InverseGauge.differentiable is False
    ref_map = g.map(uv)
    _, ref_fwd = g(uv)
    g.differentiable = True
    assert not g._on_kernels()
    u = uv.clone().requires_grad_(True)
    got = g.map(u)
    assert torch.equal(got, ref_map) and got.requires_grad and g.inverse_grad_engines() == (None, None)
    got.sum().backward()
    assert u.grad is not None and g.inverse_network.linear2.weight.grad is not None
    pts, out = g(uv)
    assert pts is uv and torch.equal(out, ref_fwd) and tuple(out.shape) == (1, 1, V.N_POINTS, 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        uv_inverse_train.InverseGrad(g, 16)


def test_engines_are_not_state():
    net = V.make_net("square", "cpu")
    g = net.inverse_gauge
    keys = set(net.state_dict())
    marker = object()
    g._template_engine, g._map_engine = marker, marker          # (what a GPU run leaves there; a CPU run has none)
    try:
        assert set(net.state_dict()) == keys and not any("engine" in k for k in keys)
        for clone in (copy.deepcopy(g), pickle.loads(pickle.dumps(g))):
            assert clone.inverse_grad_engines() == (None, None)
            assert all(torch.equal(a, b) for a, b in zip(clone.state_dict().values(), g.state_dict().values()))
    finally:
        g._template_engine = g._map_engine = None
    g.release_inverse_grad_engines()
    net.release()
    assert g.inverse_grad_engines() == (None, None)


def test_chunk_rule_is_a_function_of_n_alone():
    hpp = open(os.path.join(CSRC, "ngf_uv_inverse_train.hpp")).read()
    assert re.search(r"kUvitMinChunk = 1024, kUvitMaxChunks = 64;", hpp)
    assert T.chunk(1) == T.chunk(1024) == T.chunk(65536) == 1024 and T.chunk(65537) == 1040 and T.chunk(1 << 18) == 4096
    for n in (1, 1023, 1025, 36864, 65536, 65537, 100000, 1 << 18, (1 << 27) - 1):
        c = T.chunk(n)
        assert c % 16 == 0 and c >= 1024 and -(-n // c) <= 64


@pytest.mark.parametrize("prim", V.PRIMS)
def test_the_fixture_keeps_its_points_within_the_cap(prim):
    seed = SEED[prim]
    key = f"{prim}.s{seed}"
    keep = G[key + ".keep"]
    assert keep.dtype == np.bool_ and keep.shape == (V.N_POINTS,) and float(G["margin"]) == T.MARGIN and tuple(G["rows"]) == T.ROWS
    mine = T.kept(V.weights(seed, prim, torch.float64), torch.from_numpy(V.points(prim)).double()).numpy()
    assert np.array_equal(mine, keep)
    dropped = int((~keep).sum())
    print(f"{prim} seed {seed}: {dropped} of {V.N_POINTS} points dropped")
    assert 0 < dropped <= T.CAP * V.N_POINTS
    t, w = T.targets(seed, V.N_POINTS)
    assert np.array_equal(G[key + ".t"], t) and np.array_equal(G[key + ".w"], w * keep) and (G[key + ".w"][~keep] == 0).all()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "uv_inverse_train.npz")) < 256 * 1024


@pytest.mark.parametrize("prim", V.PRIMS)
def test_the_restatements_gradients_equal_the_fixtures(prim):
    seed = SEED[prim]
    key = f"{prim}.s{seed}"
    uv = torch.from_numpy(V.points(prim))
    t, w = torch.from_numpy(G[key + ".t"]), torch.from_numpy(G[key + ".w"])
    for tag, dtype, tol in (("f32", torch.float32, 2e-6), ("f64", torch.float64, 1e-12)):
        _, d_uv, g = T.gradients(V.weights(seed, prim, dtype), uv.to(dtype), t.to(dtype), w.to(dtype))
        worst = T.rel_err(d_uv, torch.from_numpy(G[f"{key}.d_uv.{tag}"]))
        for name, v in zip(T.NAMES, g):
            ref = torch.from_numpy(G[f"{key}.{name}.{tag}"])
            assert v.dtype == dtype and ref.dtype == dtype
            worst = max(worst, T.rel_err(T.fixture_rows(name, v), ref))
        print(f"{prim} {tag}: worst |restatement - reference| / |reference| over the tensors {worst:.3e}")
        assert worst <= tol, (tag, worst)
