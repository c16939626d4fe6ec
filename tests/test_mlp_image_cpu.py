"""The MLP image builders (csrc/ngf_mlp_image.hpp) on the CPU: tests/host/mlp_image_main.cpp, compiled with the host compiler under the address and
undefined-behaviour sanitizers, builds the seven configurations from synthetic weights; every image and pack must equal
tests/golden/mlp_images.npz word for word (the golden was written by the builders as they stood before they were rewritten piece by piece:
tests/golden/make_golden_mlp_images.py), and the slots no weight belongs to must be zero."""
import numpy as np
import pytest

import mlp_image_host as H


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("mlp_image"))
    exe, flags = H.compile_program(work)
    print("mlp_image_main built with", " ".join(flags))
    return H.run_program(exe, work)


def _section_of(sections, word):
    for name, off, count in sections:
        if off <= word < off + count:
            return f"{name}[{word - off}]"
    return "outside every section"


def test_images_equal_golden(built):
    words, sections, _ = built
    golden = np.load(H.GOLDEN)
    assert sorted(words) == sorted(golden.files), f"outputs {sorted(words)} != golden {sorted(golden.files)}"
    assert sorted(words) == sorted([c + ".img" for c in H.CONFIGS] + ["tri_nofold.pack", "ii_bf16.pack"])
    for key in sorted(words):
        got, want = words[key], golden[key]
        assert want.dtype == np.uint32 and got.shape == want.shape, f"{key}: {got.size} words, golden {want.size}"
        bad = np.flatnonzero(got != want)
        if bad.size:
            i = int(bad[0])
            where = _section_of(sections[key[:-4]], i) if key.endswith(".img") else "pack"
            pytest.fail(f"{key}: {bad.size} of {got.size} words differ, first at word {i} = {where}: got {int(got[i]):#010x}, golden {int(want[i]):#010x}")


def test_sections_tile_the_images(built):
    words, sections, _ = built
    for c in H.CONFIGS:
        at = 0
        for name, off, count in sections[c]:
            assert off == at and count > 0, f"{c}: section {name} at {off}, expected {at}"
            at += count
        assert at == words[c + ".img"].size, c


def test_pad_slots_are_zero(built):
    words, sections, _ = built
    sec = {c: {name: off for name, off, _ in sections[c]} for c in H.CONFIGS}

    def zero(c, what, a):
        assert not np.asarray(a).any(), f"{c}: {what} is not zero"

    for c in H.CONFIGS:
        img = words[c + ".img"]
        h16 = img.view(np.uint16)
        S = sec[c]
        zero(c, "B3 + 3", img[S["B3"] + 3])
        # view entry 15 (lane quarter 3's fourth view input): the zero pad column of [W1' | view | pad]
        if c in ("tri_fp32", "tri_nofold", "ii_fp32"):              # fp32 k-steps [4 mt][KT][64 lanes]; the last k-step, lanes 48..63
            KT = (S["W2"] - S["W1"]) // 256
            zero(c, "view entry 15", img[S["W1"]:S["W2"]].reshape(4, KT, 64)[:, KT - 1, 48:])
        elif c in ("tri_bake", "tri_bake_bf16"):                    # only the four view k-steps remain
            zero(c, "view entry 15", img[S["W1"]:S["W1"] + 1024].reshape(4, 4, 64)[:, 3, 48:])
        elif c == "tri_bf16":                                       # [4 mt][5 kb][3 parts][64 lanes][8]: input j = 39 of lane quarter 3
            zero(c, "view entry 15", h16[2 * S["W1"]:2 * S["W2"]].reshape(4, 5, 3, 64, 8)[:, 4, :, 48:, 7])
        else:                                                       # ii_bf16 [4 mt][8 kb][2 parts][64 lanes][8]: j = 57 of quarter 3, and j >= 58 everywhere
            w1 = h16[2 * S["W1"]:2 * S["W2"]].reshape(4, 8, 2, 64, 8)
            lo = words["ii_bf16.pack"].view(np.uint16).reshape(8, 4, 64, 8)
            zero(c, "view entry 15", w1[:, 7, :, 48:, 1])
            zero(c, "view entry 15 (lo pack)", lo[7, :, 48:, 1])
            zero(c, "inputs j >= 58", w1[:, 7, :, :, 2:])
            zero(c, "inputs j >= 58 (lo pack)", lo[7, :, :, 2:])
        if c.startswith("ii"):
            zero(c, "density B3 + 1..3", img[S["dens.B3"] + 1:S["dens.B3"] + 4])
        if c == "ii_bf16":                                          # density layer 1 [5 kb][3 parts][64 lanes][8]: inputs 72..79 = k-block 4, upper lane half
            zero(c, "density inputs k >= 72", h16[2 * S["dens.D1"]:2 * S["dens.D2"]].reshape(5, 3, 64, 8)[4, :, 32:, :])
    # the basis pack [36 k-steps][3 groups][64 lanes][4 tiles]: nine unit tiles, so elements 1..3 of group 2 are unused
    zero("tri_nofold", "unused tiles of the basis pack", words["tri_nofold.pack"].reshape(36, 3, 64, 4)[:, 2, :, 1:])
