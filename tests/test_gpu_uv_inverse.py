"""GPU: NeuTex's inverse gauge in its HIP kernel (csrc/ngf_uv_inverse.hpp through ngf_uv_inverse_map, NeuTex.inverse_map / cycle_error /
coordinate_deformation) against the reference module's own outputs (tests/golden/uv_inverse.npz).

Accuracy criterion (DESIGN.md sections 4.7, 4.11, 4.12): the GPU's max-abs distance to the fp64 output is at most max(4x the distance of the
reference's fp32 evaluation to it, 2e-6); absolute, over every value, nothing masked.  Both distances come from the fixture."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ngf_amd  # noqa: E402,F401
from ngf_amd import _lib, mesh, uvmapping  # noqa: E402
import uv_inverse_eager as V  # noqa: E402
import uv_query_eager as Q  # noqa: E402

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(ROOT, "tests", "golden", "uv_inverse.npz"))
PRIMS = V.PRIMS
_NETS, _FULL = {}, {}


def model(prim, seed=V.SEEDS[0]):
    """One GPU model per (primitive, seed) for the whole module (no test changes it)."""
    if (prim, seed) not in _NETS:
        _NETS[prim, seed] = V.make_net(prim, "cuda", seed)
    return _NETS[prim, seed]


def uv_points(prim):
    return torch.from_numpy(G[f"{prim}.uv"]).cuda()


def full(prim, seed=V.SEEDS[0]):
    """inverse_map of the fixture's 161 points: computed once, never changed."""
    if (prim, seed) not in _FULL:
        _FULL[prim, seed] = model(prim, seed).inverse_map(uv_points(prim))
    return _FULL[prim, seed]


@pytest.mark.parametrize("seed", V.SEEDS)
@pytest.mark.parametrize("prim", PRIMS)
def test_inverse_map_matches_the_reference(prim, seed):
    got = full(prim, seed)
    assert tuple(got.shape) == (V.N_POINTS, 3) and got.device.type == "cuda" and got.dtype == torch.float32 and not got.requires_grad
    f32, f64 = G[f"{prim}.s{seed}.xyz.f32"], G[f"{prim}.s{seed}.xyz.f64"]
    ref = float(np.abs(f32.astype(np.float64) - f64).max())
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - f64).max())
    bound = max(4 * ref, 2e-6)
    print(f"{prim} seed {seed}: max|hip - fp64| = {err:.3e}, max|reference fp32 - fp64| = {ref:.3e}, bound {bound:.3e}")
    assert torch.isfinite(got).all()
    assert err <= bound, (prim, seed, err, ref, bound)


def grid_points():
    """One point more than a full grid of passes: every wave of every block runs a pass and the first wave a second one."""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return uvmapping.INVERSE_TILE_POINTS * uvmapping.INVERSE_WAVES_PER_BLOCK * cus + 1


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
@pytest.mark.parametrize("prim", PRIMS)
def test_a_points_value_does_not_depend_on_the_batch(prim, reverse):
    net, ref, uv = model(prim), full(prim), uv_points(prim)
    for n in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129):
        rows = torch.arange(n, device="cuda")
        if reverse:
            rows = rows.flip(0)
        assert torch.equal(net.inverse_map(uv[rows]), ref[rows]), n
    n = grid_points()
    assert n > V.N_POINTS
    rows = torch.arange(n, device="cuda") % V.N_POINTS
    if reverse:
        rows = rows.flip(0)
    assert torch.equal(net.inverse_map(uv[rows]), ref[rows]), n


@pytest.mark.parametrize("prim", PRIMS)
def test_nothing_is_written_past_the_end(prim):
    net, ref, uv = model(prim), full(prim), uv_points(prim)
    h = net.inverse_handle()
    sentinel = -12345.5
    for n in (1, 17, 33):
        out = torch.full((3 * n + 64,), sentinel, device="cuda")
        pts = uv[:n].contiguous()
        _lib.check(_lib.lib().ngf_uv_inverse_map(h, pts.data_ptr(), n, out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        assert torch.equal(out[:3 * n].view(n, 3), ref[:n]), n
        assert (out[3 * n:] == sentinel).all(), n


@pytest.mark.parametrize("prim", PRIMS)
def test_two_launches_give_equal_bits(prim):
    net, uv = model(prim), uv_points(prim)
    assert torch.equal(net.inverse_map(uv), full(prim)) and torch.equal(net.inverse_map(uv), net.inverse_map(uv.clone()))
    assert torch.equal(V.make_net(prim, "cuda").inverse_map(uv), full(prim))          # a second model with the same weights


@pytest.mark.parametrize("prim", PRIMS)
def test_leading_shapes_and_strides(prim):
    net, ref, uv = model(prim), full(prim), uv_points(prim)
    D = V.DIMS[prim]
    got = net.inverse_map(uv[:21].view(3, 7, D))
    assert tuple(got.shape) == (3, 7, 3) and torch.equal(got.view(21, 3), ref[:21])
    wide = torch.zeros((V.N_POINTS, D + 2), device="cuda")
    wide[:, 1:1 + D] = uv
    sliced = wide[::2, 1:1 + D]                                                          # every second point, a column window: no contiguous view
    assert not sliced.is_contiguous()
    assert torch.equal(net.inverse_map(sliced), ref[::2])
    one = net.inverse_map(uv[5])
    assert tuple(one.shape) == (3,) and torch.equal(one, ref[5])
    assert torch.equal(net.inverse_map(uv.cpu().numpy()), ref)                           # anything torch.as_tensor takes, from any device
    assert tuple(net.inverse_map(uv[:0]).shape) == (0, 3)
    with pytest.raises(ValueError):
        net.inverse_map(torch.zeros(4, D + 1, device="cuda"))


@pytest.mark.parametrize("prim", PRIMS)
def test_the_handle_follows_the_parameters(prim):
    uv, ref = uv_points(prim), full(prim)
    net = V.make_net(prim, "cuda")
    assert torch.equal(net.inverse_map(uv), ref)
    h0 = net._inv_handle.value
    assert torch.equal(net.inverse_map(uv), ref) and net._inv_handle.value == h0          # cached while nothing changes
    last = net.inverse_gauge.inverse_network.last_linear
    with torch.no_grad():
        last.weight.mul_(0.5)
    halved = net.inverse_map(uv)
    assert net._inv_handle.value is not None and not torch.equal(halved, ref)
    # a power of two on the last layer's weights: every product and partial sum scales exactly, so what stands in front of the bias halves; the
    # sums with the (unchanged) bias round once each on either side
    bias = last.bias.detach()
    assert float(((halved - bias) - 0.5 * (ref - bias)).abs().max()) <= 4 * float(np.spacing(np.float32(1)))
    fresh = uvmapping.NeuTex(primitive_type=prim, sample_num=64, device="cuda")
    fresh.load_state_dict(net.state_dict())
    assert torch.equal(fresh.inverse_map(uv), halved)
    net.release()
    assert net._inv_handle is None and net._handle is None
    assert torch.equal(net.inverse_map(uv), halved)             # rebuilt on demand


@pytest.mark.parametrize("prim", PRIMS)
def test_cycle_error_is_the_composition(prim):
    net = model(prim)
    xyz = torch.from_numpy(Q.points()).cuda()
    got = net.cycle_error(xyz)
    uv = net.query(xyz, want=("uv",))["uv"]
    assert tuple(uv.shape) == (Q.N_POINTS, V.DIMS[prim])
    want = ((net.inverse_map(uv) - xyz) ** 2).sum(-1)
    assert tuple(got.shape) == (Q.N_POINTS,) and torch.equal(got, want) and torch.isfinite(got).all() and float(got.max()) > 0
    shaped = net.cycle_error(xyz[:160].view(4, 40, 3))
    assert tuple(shaped.shape) == (4, 40) and torch.equal(shaped.reshape(160), want[:160])


@pytest.mark.parametrize("prim,kw", [("sphere", {"icosphere_division": 2}), ("square", {"side": 9})])
def test_coordinate_deformation(prim, kw, tmp_path):
    net = model(prim)
    R, view = 16, (0.0, 0.6, 0.8)
    tv, tf = mesh.icosphere(2) if prim == "sphere" else mesh.square_template(9)
    template = torch.from_numpy(tv).cuda()
    verts, faces, colors, st = net.coordinate_deformation(viewdir=view, texture_resolution=R, **kw)
    assert all(t.device.type == "cuda" for t in (verts, faces, colors, st))
    assert torch.equal(verts, net.inverse_map(template)) and tuple(verts.shape) == (len(tv), 3)
    assert torch.equal(faces.cpu(), torch.from_numpy(tf)) and faces.dtype == torch.int64
    assert torch.equal(colors, net.texture_colors(template, view)) and tuple(colors.shape) == (len(tv), 3)
    assert torch.equal(st, mesh.atlas_coords(template, prim, R if prim == "sphere" else None)) and tuple(st.shape) == (len(tv), 2)
    path = str(tmp_path / "deformed.obj")
    again = net.coordinate_deformation(path, viewdir=view, texture_resolution=R, **kw)
    assert all(torch.equal(a, b) for a, b in zip(again, (verts, faces, colors, st)))
    got = Q.read_obj(path)
    assert got["v"].shape == (len(tv), 3) and np.array_equal(got["v"].view(np.uint32), verts.cpu().numpy().view(np.uint32))
    assert got["f"].shape == tf.shape and np.array_equal(got["f"], tf) and got["f"].min() >= 0 and got["f"].max() < len(tv)
    assert got["f_vt"].min() >= 0 and got["f_vt"].max() < len(got["vt"]) and len(got["vt"]) >= len(tv)
    assert np.array_equal(got["vt"][:len(tv)].view(np.uint32), st.cpu().numpy().view(np.uint32))
    assert os.path.exists(Q.sibling(path, ".mtl")) and Q.read_mtl(Q.sibling(path, ".mtl"))["map_Kd"] == "deformed.png"
    from PIL import Image
    img = np.asarray(Image.open(Q.sibling(path, ".png")))
    assert img.shape == ((R, 2 * R, 3) if prim == "sphere" else (R, R, 3)) and img.dtype == np.uint8
