"""CPU checks of NeuTex training through the occupancy grid (``net.occupancy_in_training``): the three new C-ABI symbols are
exported by both libraries and refuse bad arguments without a GPU, the switch defaults off and is saved nowhere, the torch restatement with a
supplied valid mask (tests/uv_train_occ_eager.py) is tests/uv_train_eager.py's forward bit for bit when the mask is the in-cube mask, and the
batches and masks of tests/test_gpu_uv_train_occupancy.py are what that file takes them for: few samples near a cell boundary, kept counts on
both sides of the 1024-row chunk, rays that lose every sample, a case that keeps nothing."""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest
import torch

import ngf_amd  # noqa: F401
from ngf_amd import _lib, uv_train, uvmapping
import uv_occupancy_ref as O
import uv_train_eager as E
import uv_train_occ_eager as EO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ngf_uv_trainer_set_occupancy", "ngf_uv_train_counts", "ngf_uv_train_kept"]
# kept samples per seed (E.EDGE_SEEDS) by the float32 torch restatement on the CPU: the record the cases were chosen by
KEPT = {"checkerboard 8": (1048, 1033, 1022), "ball 16": (670, 604, 639), "ball 128": (316, 269, 334), "random 5x7x16": (7, 12, 11),
        "ball 16 at V=17": (0, 0, 0)}


def test_the_symbols_are_exported_by_both_libraries():
    hdr = open(os.path.join(ROOT, "include", "ngf.h")).read()
    for s in NEW:
        assert re.search(r"\b" + s + r"\s*\(", hdr) and s in _lib.SYMBOLS, s
    L = _lib.lib()
    assert all(hasattr(L, s) for s in NEW)
    uv_train._bind(L)
    assert L.ngf_abi_version() == 5
    with _lib.library("exp") as X:
        assert all(hasattr(X, s) for s in NEW)
        uv_train._bind(X)


def test_they_refuse_bad_arguments_without_a_gpu():
    L = _lib.lib()
    uv_train._bind(L)
    out = (C.c_int64 * 2)(-7, -7)
    assert L.ngf_uv_trainer_set_occupancy(None, None, 0, 0, 0, None) == 1
    assert b"null handle" in L.ngf_last_error()
    assert L.ngf_uv_trainer_set_occupancy(None, None, 4, 4, 4, None) == 1
    assert L.ngf_uv_train_counts(None, out, None) == 1
    assert L.ngf_uv_train_kept(None, None, None) == 1
    assert tuple(out) == (-7, -7)


def test_the_switch_defaults_off_and_is_saved_nowhere(tmp_path):
    net = uvmapping.NeuTex(primitive_type="square", device="cpu")
    assert net.occupancy_in_training is False and uvmapping.NeuTex.occupancy_in_training is False
    net.occupancy_in_training = True
    assert not any("occupancy" in k for k in net.state_dict())
    assert "occupancy_in_training" not in net.__getstate__()
    clone = pickle.loads(pickle.dumps(net))
    assert clone.occupancy_in_training is False and "occupancy_in_training" not in clone.__dict__
    p = str(tmp_path / "net.pth")
    torch.save(net.state_dict(), p)
    fresh = uvmapping.NeuTex(primitive_type="square", device="cpu")
    fresh.load_state_dict(torch.load(p), strict=True)
    assert fresh.occupancy_in_training is False
    assert net.occupancy_in_training is True


@pytest.mark.parametrize("prim", ["square", "sphere"])
def test_the_restatement_with_the_in_cube_mask_is_the_eager_forward_bit_for_bit(prim):
    seed, Sn = 311, 16
    b = E.batch(seed, prim, R=12, S=Sn, P=8)
    net = E.make_net(E.model_params(seed, prim), prim, Sn, "cpu")
    t = lambda k: torch.from_numpy(b[k])          # noqa: E731
    bg = torch.from_numpy(EO.BG1)
    with torch.no_grad():
        want = E.forward(net, t("campos"), t("raydir"), bg, t("U"), t("template"), extras=True)
        valid = want["valid"]
        got = EO.forward(net, t("campos"), t("raydir"), bg, t("U"), t("template"), valid)
        assert 0 < int(valid.sum()) < valid.numel()
        for k in got:
            assert got[k].dtype == torch.float32 and torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), k
        # with a mask: a masked sample's weight is exactly 0, and the picture changes
        keep = torch.from_numpy(EO.keep_of(O.checkerboard((4, 4, 4)), want["points_original"].numpy()))
        assert 0 < int(keep.sum()) < int(valid.sum()) and bool((keep <= valid).all())
        out = EO.forward(net, t("campos"), t("raydir"), bg, t("U"), t("template"), keep)
        assert bool((out["points_inverse_weights"][~keep] == 0).all()) and bool((out["points_inverse_weights"][keep] > 0).any())
        assert torch.equal(out["uv"], want["uv"]) and not torch.equal(out["color"], want["color"])


@pytest.mark.parametrize("case", EO.CASES + (EO.EMPTY_CASE,), ids=lambda c: c[0])
def test_the_gpu_cases_keep_their_samples_off_the_cell_boundaries(case):
    name, V, make = case
    vol = make()
    kept = []
    for seed in E.EDGE_SEEDS:
        b = E.edge_batch(seed, "square", EO.S, V=V)
        keep, pinned, valid, p32, _ = O.decisions(b["campos"], b["raydir"], b["U"], vol)
        assert int(valid.sum()) == V and np.array_equal(keep, EO.keep_of(vol, p32))
        near = int((valid & ~pinned).sum())
        print(f"uv_train_occupancy {name} seed {seed}: {V} in-cube, {int(keep.sum())} kept, {near} within {O.BOUNDARY_MARGIN} of a cell boundary")
        assert near <= EO.NEAR_SHARE * V, (name, seed, near)
        kept.append(int(keep.sum()))
        if name == "ball 16":          # rays that have in-cube samples and keep none of them
            lost = int(((valid.sum(-1) > 0) & (keep.sum(-1) == 0)).sum())
            assert 23 <= lost <= 29, lost
        if name == "checkerboard 8":          # masked and kept samples alternate within rays
            flips = (keep[..., 1:] != keep[..., :-1]) & valid[..., 1:] & valid[..., :-1]
            assert int((flips.sum(-1) >= 2).sum()) > 10
        # the batch does not depend on the primitive (only the template points do)
        assert np.array_equal(E.edge_batch(seed, "sphere", EO.S, V=V)["raydir"], b["raydir"])
    assert tuple(kept) == KEPT[name], (name, kept)
    if name == "checkerboard 8":
        assert min(kept) < 1024 < max(kept)
    if name == "ball 128":
        assert int(np.prod(vol.shape)) > 1 << 20
