"""The streamed weight images of the UV-Mapping kernels (csrc/ngf_uv_pack.hpp) on the CPU: tests/host/uv_pack_main.cpp, compiled with the host
compiler under the address and undefined-behaviour sanitizers, runs the plan of the packed inverse network and the slot function over every
segment, forward and transposed, for D = 2 and D = 3, and the slot arithmetic of ngf_uv.hip's UvPacker at four of its shapes.  Every word must
equal an independent numpy restatement, written as the loops of the host packer the shared header replaced (for t, g, l, e: unit
(4 g + e) 16 + (l & 15), input imap(t, l >> 4) ...), applied to W for the forward set and to W.T for the transposed set."""
import os
import subprocess

import numpy as np
import pytest

import mlp_image_host as H
from ngf_amd import synth

SOURCE = os.path.join(H.ROOT, "tests", "host", "uv_pack_main.cpp")
LAYERS = ("linear1", "linear2", "linear_list.0", "linear_list.1", "last_linear")
M, HID = 64, 512
UVP = (("w63", (256, 63)), ("w64", (128, 64)), ("w3", (3, 256)), ("w295", (256, 295)), ("b256", (256,)), ("b3", (3,)))


def shapes(D):
    return [(M, D), (HID, M), (HID, HID), (HID, HID), (3, HID)]


def seeded(D):
    p = synth.inverse_gauge_params(71, "square" if D == 2 else "sphere")
    pre = "inverse_gauge.inverse_network."
    return [(np.asarray(p[pre + n + ".weight"], np.float32), np.asarray(p[pre + n + ".bias"], np.float32)) for n in LAYERS]


def distinct(D):
    """Ten tensors whose values are nonzero and pairwise different over the whole network: a word of an image names the weight it came from."""
    flat = H._distinct(10 + D, sum(o * i + o for o, i in shapes(D)))
    out, at = [], 0
    for o, i in shapes(D):
        out.append((flat[at:at + o * i].reshape(o, i).copy(), flat[at + o * i:at + o * i + o].copy()))
        at += o * i + o
    return out


def uvp_tensors():
    flat = H._distinct(20, sum(int(np.prod(s)) for _, s in UVP))
    out, at = {}, 0
    for name, shape in UVP:
        n = int(np.prod(shape))
        out[name] = flat[at:at + n].reshape(shape).copy()
        at += n
    return out


def run(exe, work, tag, nets, uvp):
    wpath, outdir = os.path.join(work, tag + ".f32"), os.path.join(work, tag)
    os.makedirs(outdir)
    with open(wpath, "wb") as f:
        for D in (2, 3):
            for w, b in nets[D]:
                f.write(w.astype("<f4").tobytes() + b.astype("<f4").tobytes())
        for name, _ in UVP:
            f.write(uvp[name].astype("<f4").tobytes())
    r = subprocess.run([exe, wpath, outdir], capture_output=True, text=True)
    assert r.returncode == 0, f"{exe} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}"
    segs, at = {2: [], 3: []}, {2: {}, 3: {}}
    for line in r.stdout.splitlines():
        w = line.split()
        D = int(w[1][1:])
        if w[0] == "seg":
            segs[D].append(dict(zip(("kind", "dst", "count", "out_f", "in_f", "so", "si", "NT", "hid"), map(int, w[3:]))))
            assert int(w[2]) == len(segs[D]) - 1
        else:
            at[D][w[2]] = int(w[3])
    words = {fn[:-5]: np.fromfile(os.path.join(outdir, fn), dtype="<u4") for fn in sorted(os.listdir(outdir))}
    return words, segs, at


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("uv_pack"))
    exe, flags = H.compile_program(work, source=SOURCE)
    print("uv_pack_main built with", " ".join(flags))
    uvp = uvp_tensors()
    nets = {"seeded": {D: seeded(D) for D in (2, 3)}, "distinct": {D: distinct(D) for D in (2, 3)}}
    return {tag: (nets[tag], uvp) + run(exe, work, tag, nets[tag], uvp) for tag in nets}


# ---- the restatement: the loops of the host packer that ngf_uv_pack.hpp replaced ---------------------------------------------------------------
def nat(t, kq):
    return 4 * t + kq


def hid(t, kq):
    return (t >> 2) * 16 + 4 * kq + (t & 3)


def mixed(t, kq):
    return np.where(t < 64, hid(t, kq), 256 + 4 * (t - 64) + kq)


def _pick(W, o, i):
    out_f, in_f = W.shape
    ok = (o < out_f) & (i >= 0) & (i < in_f)
    return np.where(ok, W[np.clip(o, 0, out_f - 1), np.clip(i, 0, in_f - 1)], np.float32(0)).astype(np.float32)


def dense(W, KT, NT, imap):
    """[KT][NT / 4][64 lanes][4]"""
    t, g, l, e = np.meshgrid(np.arange(KT), np.arange(NT // 4), np.arange(64), np.arange(4), indexing="ij")
    return _pick(W, (4 * g + e) * 16 + (l & 15), imap(t, l >> 4)).reshape(-1)


def out_layer(W, KT, imap):
    """[KT / 4][64 lanes][4]: word ((t >> 2) 64 + l) 4 + (t & 3)"""
    t, l = np.meshgrid(np.arange(KT), np.arange(64), indexing="ij")
    buf = np.zeros(KT * 64, np.float32)
    buf[((t >> 2) * 64 + l) * 4 + (t & 3)] = _pick(W, l & 15, imap(t, l >> 4))
    return buf


def bias(b, NT):
    """[4 lane quarters][NT][4]: accumulator order"""
    kq, mt, r = np.meshgrid(np.arange(4), np.arange(NT), np.arange(4), indexing="ij")
    return b[mt * 16 + 4 * kq + r].reshape(-1).astype(np.float32)


def bias4(b):
    return np.concatenate([b, np.zeros(4 - b.size, np.float32)]).astype(np.float32)


def forward_images(net):
    """The host packer's sequence of the inference handle: (name, image) in buffer order."""
    (w1, b1), (w2, b2), (wa, ba), (wb, bb), (wo, bo) = net
    return [("w1", dense(w1, 4, M // 16, nat)), ("b1", bias(b1, M // 16)), ("w2", dense(w2, M // 4, HID // 16, hid)), ("b2", bias(b2, HID // 16)),
            ("wh", dense(wa, HID // 4, HID // 16, hid)), ("wh.1", dense(wb, HID // 4, HID // 16, hid)), ("bh", bias(ba, HID // 16)), ("bh.1", bias(bb, HID // 16)),
            ("wo", out_layer(wo, HID // 4, hid)), ("bo", bias4(bo))]


def transposed_images(net, D):
    """The dX chain's layers, last first: layer^T packed as a layer of its own (d_xyz enters in natural order, as uv does in linear1)."""
    (w1, _), (w2, _), (wa, _), (wb, _), (wo, _) = net
    T = np.ascontiguousarray
    return [("to", dense(T(wo.T), 4, HID // 16, nat)), ("th", dense(T(wb.T), HID // 4, HID // 16, hid)), ("th.1", dense(T(wa.T), HID // 4, HID // 16, hid)),
            ("t2", dense(T(w2.T), HID // 4, M // 16, hid)), ("t1", out_layer(T(w1.T), M // 4, hid))]


def expected(net, D):
    imgs = forward_images(net) + transposed_images(net, D) + [("zb", np.zeros(HID, np.float32))]
    offs, at = {}, 0
    for name, img in imgs:
        offs[name] = at
        at += img.size
    return np.concatenate([img for _, img in imgs]), offs, imgs


def _words(a):
    return np.ascontiguousarray(a, dtype="<f4").view("<u4")


# ---- the tests ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["seeded", "distinct"])
@pytest.mark.parametrize("D", [2, 3])
def test_every_word_equals_the_restatement(built, tag, D):
    nets, _, words, _, _ = built[tag]
    want, offs, _ = expected(nets[D], D)
    got = words[f"inv_d{D}"]
    assert got.size == want.size, (got.size, want.size)
    bad = np.flatnonzero(got != _words(want))
    if bad.size:
        i = int(bad[0])
        where = max((o, n) for n, o in offs.items() if o <= i)
        pytest.fail(f"D = {D}: {bad.size} of {got.size} words differ, first at word {i} = {where[1]}[{i - where[0]}]: got {int(got[i]):#010x}, want {int(_words(want)[i]):#010x}")


@pytest.mark.parametrize("D", [2, 3])
def test_segments_tile_the_buffer_and_offsets_are_the_old_sequence(built, D):
    _, _, words, segs, at = built["seeded"]
    segs, at = segs[D], at[D]
    assert at["nseg"] == len(segs) == 15 and at["nfwd"] == 10
    pos = 0
    for k, s in enumerate(segs):
        assert s["dst"] == pos and s["count"] > 0 and s["dst"] % 4 == 0 and s["count"] % 4 == 0, (k, s, pos)
        pos += s["count"]
        if k == at["nfwd"] - 1:
            assert pos == at["fwd_floats"]
    assert pos == at["zb"] and at["zb"] + HID == at["floats"] == words[f"inv_d{D}"].size
    # the forward offsets, from the sizes of the old host packer's calls in their order: dense KT NT 64, bias NT 16, out KT 64, bias4 4
    sizes = [("w1", 4 * (M // 16) * 64), ("b1", M), ("w2", (M // 4) * (HID // 16) * 64), ("b2", HID), ("wh", 2 * (HID // 4) * (HID // 16) * 64), ("bh", 2 * HID),
             ("wo", (HID // 4) * 64), ("bo", 4)]
    pos = 0
    for name, n in sizes:
        assert at[name] == pos, (name, at[name], pos)
        pos += n
    assert pos == at["fwd_floats"]
    _, offs, _ = expected(seeded(D), D)
    for name in ("to", "th", "t2", "t1", "zb"):
        assert at[name] == offs[name] and at[name] % 4 == 0, (name, at[name], offs[name])
    # the hidden layers are read at a stride: the second image follows the first directly
    assert segs[5]["dst"] - segs[4]["dst"] == HID * HID and segs[7]["dst"] - segs[6]["dst"] == HID and segs[12]["dst"] - segs[11]["dst"] == HID * HID


@pytest.mark.parametrize("D", [2, 3])
def test_every_weight_appears_once_and_every_other_slot_is_zero(built, D):
    nets, _, words, segs, at = built["distinct"]
    net, got, segs, at = nets[D], words[f"inv_d{D}"], segs[D], at[D]
    assert all((w != 0).all() and (b != 0).all() for w, b in net)
    src = [net[0][0], net[0][1], net[1][0], net[1][1], net[2][0], net[3][0], net[2][1], net[3][1], net[4][0], net[4][1],      # forward order
           net[4][0], net[3][0], net[2][0], net[1][0], net[0][0]]                                                               # transposed
    for k, (s, a) in enumerate(zip(segs, src)):
        img = got[s["dst"]:s["dst"] + s["count"]]
        nz = np.sort(img[img != 0])
        want = np.sort(_words(a).reshape(-1))
        assert nz.size == want.size and (nz == want).all(), f"D = {D} segment {k}: {nz.size} nonzero words for {want.size} weights, or other values"
    assert not got[at["zb"]:].any(), "the zero-bias block"


def test_uvpacker_slot_arithmetic(built):
    _, uvp, words, _, _ = built["distinct"]
    want = {"uvp_dense_256x63": dense(uvp["w63"], 16, 16, nat), "uvp_dense_128x64": dense(uvp["w64"], 16, 8, hid), "uvp_out_3x256": out_layer(uvp["w3"], 64, hid),
            "uvp_dense_256x295": dense(uvp["w295"], 76, 16, mixed), "uvp_bias_256": bias(uvp["b256"], 16), "uvp_bias4_3": bias4(uvp["b3"])}
    assert sorted(k for k in words if k.startswith("uvp_")) == sorted(want)
    for k, w in want.items():
        got = words[k]
        assert got.size == w.size, (k, got.size, w.size)
        bad = np.flatnonzero(got != _words(w))
        assert not bad.size, f"{k}: {bad.size} of {got.size} words differ, first at {int(bad[0])}"
        src = {"uvp_dense_256x63": "w63", "uvp_dense_128x64": "w64", "uvp_out_3x256": "w3", "uvp_dense_256x295": "w295", "uvp_bias_256": "b256", "uvp_bias4_3": "b3"}[k]
        nz = got[got != 0]
        assert (np.sort(nz) == np.sort(_words(uvp[src]).reshape(-1))).all(), f"{k}: not every weight exactly once"
