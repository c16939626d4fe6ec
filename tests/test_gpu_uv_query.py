"""GPU: the UV-Mapping (NeuTex) point queries (csrc/ngf_uv_query.hpp through ngf_uv_query / ngf_uv_density_lattice, NeuTex.query /
density_lattice) and the UV-textured mesh export (NeuTex.export_mesh) against the reference modules' own outputs (tests/golden/uv_query.npz).

Criterion 1 (DESIGN.md sections 4.7, 4.11): separately for sigma, uv and rgb, the GPU's max-abs distance to the fp64 output is at most
max(4x the distance of the fp32 torch evaluation to it, 2e-6); absolute, over every value, nothing masked."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ngf_amd  # noqa: E402,F401
from ngf_amd import evalout, mesh, synth, uvmapping  # noqa: E402
import mesh_ref  # noqa: E402
import uv_export_eager as E  # noqa: E402
import uv_query_eager as Q  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden")
G = np.load(os.path.join(GOLDEN, "uv_query.npz"))
G_EDIT = np.load(os.path.join(GOLDEN, "uv_edit.npz"))
PRIMS = Q.PRIMS
_NETS, _FULL = {}, {}


def model(prim):
    """One GPU model per primitive for the whole module (no test changes it without putting it back)."""
    if prim not in _NETS:
        _NETS[prim] = Q.make_net(prim, "cuda")
    return _NETS[prim]


def xyz_view():
    return torch.from_numpy(G["xyz"]).cuda(), torch.from_numpy(G["view"]).cuda()


def full(prim):
    """query of the fixture's 161 points, everything wanted, unclipped: computed once, never changed."""
    if prim not in _FULL:
        xyz, view = xyz_view()
        _FULL[prim] = model(prim).query(xyz, view, clip=False)
    return _FULL[prim]


def criterion1(name, got, f32, f64):
    ref = float(np.abs(np.asarray(f32, np.float64) - f64).max())
    err = float(np.abs(np.asarray(got, np.float64) - f64).max())
    bound = max(4 * ref, 2e-6)
    print(f"{name}: max|hip - fp64| = {err:.3e}, max|fp32 torch - fp64| = {ref:.3e}, bound {bound:.3e}, ratio err/ref {err / ref:.2f}")
    assert np.isfinite(got).all()
    assert err <= bound, (name, err, ref, bound)


@pytest.mark.parametrize("prim", PRIMS)
def test_query_matches_the_reference(prim):
    got = full(prim)
    D = 3 if prim == "sphere" else 2
    assert sorted(got) == ["rgb", "sigma", "uv"]
    assert tuple(got["sigma"].shape) == (161,) and tuple(got["uv"].shape) == (161, D) and tuple(got["rgb"].shape) == (161, 3)
    for name in ("sigma", "uv", "rgb"):
        t = got[name]
        assert t.device.type == "cuda" and t.dtype == torch.float32 and not t.requires_grad
        criterion1(f"{prim}.{name}", t.cpu().numpy(), G[f"{prim}.{name}.f32"], G[f"{prim}.{name}.f64"])      # rgb: the fp64 colour at the fp64 uv


@pytest.mark.parametrize("prim", PRIMS)
def test_a_points_values_depend_on_nothing_else(prim):
    net, ref = model(prim), full(prim)
    xyz, view = xyz_view()

    def same(got, rows, names=("sigma", "uv", "rgb")):
        assert sorted(got) == sorted(names)
        for k in names:
            assert torch.equal(got[k], ref[k][rows]), (k, rows)

    for m in (1, 17, 31, 32, 33, 47, 160):
        same(net.query(xyz[:m], view[:m], clip=False), slice(0, m))
    one = net.query(xyz[5], view[5], clip=False)
    assert tuple(one["sigma"].shape) == () and tuple(one["rgb"].shape) == (3,)
    same(one, 5)
    shaped = net.query(xyz[:160].view(4, 40, 3), view[:160].view(4, 40, 3), clip=False)
    assert tuple(shaped["sigma"].shape) == (4, 40) and tuple(shaped["uv"].shape)[:2] == (4, 40) and tuple(shaped["rgb"].shape) == (4, 40, 3)
    same({k: v.reshape((160,) + tuple(v.shape[2:])) for k, v in shaped.items()}, slice(0, 160))
    shared = net.query(xyz[:40], view[7], clip=False)
    expanded = net.query(xyz[:40], view[7].expand(40, 3), clip=False)
    assert all(torch.equal(shared[k], expanded[k]) for k in shared) and torch.equal(shared["rgb"][7], ref["rgb"][7])
    for want in (("sigma",), ("uv",), ("sigma", "uv"), ("uv", "rgb"), ("rgb",), ("sigma", "rgb")):
        same(net.query(xyz, view, want=want, clip=False), slice(None), want)
    same(net.query(xyz, view, clip=False), slice(None))                                  # two calls
    other = Q.make_net(prim, "cuda")                                                     # a second model with the same weights
    same(other.query(xyz, view, clip=False), slice(None))
    empty = net.query(xyz[:0], view[:0])
    D = 3 if prim == "sphere" else 2
    assert tuple(empty["sigma"].shape) == (0,) and tuple(empty["uv"].shape) == (0, D) and tuple(empty["rgb"].shape) == (0, 3)
    with pytest.raises(ValueError):
        net.query(xyz)                                   # rgb wanted, no view, not diffuse
    with pytest.raises(ValueError):
        net.query(xyz, want=("alpha",))
    with pytest.raises(ValueError):
        net.query(xyz[:, :2], want=("sigma",))


@pytest.mark.parametrize("prim", PRIMS)
def test_colour_is_the_export_paths_bit_for_bit(prim):
    net, ref = model(prim), full(prim)
    xyz, view = xyz_view()
    assert torch.equal(ref["rgb"], net.texture_colors(ref["uv"], view))
    dif = net.query(xyz, diffuse=True, clip=False)
    assert torch.equal(dif["uv"], ref["uv"]) and torch.equal(dif["sigma"], ref["sigma"])
    assert torch.equal(dif["rgb"], net.texture_colors(ref["uv"], diffuse=True)) and not torch.equal(dif["rgb"], ref["rgb"])
    assert torch.equal(net.query(xyz, want=("rgb",), diffuse=True)["rgb"], dif["rgb"])
    try:
        net.set_target_texture(E.edit_texture(G_EDIT, prim), 1)
        edited = net.query(xyz, view, clip=False)
        assert torch.equal(edited["uv"], ref["uv"]) and torch.equal(edited["sigma"], ref["sigma"])
        assert torch.equal(edited["rgb"], net.texture_colors(ref["uv"], view)) and not torch.equal(edited["rgb"], ref["rgb"])
        assert torch.equal(net.query(xyz, diffuse=True, want=("rgb",))["rgb"], dif["rgb"])          # the diffuse branch has no edit stage
    finally:
        net.set_target_texture(None)
    assert torch.equal(net.query(xyz, view, clip=False)["rgb"], ref["rgb"])


@pytest.mark.parametrize("prim", PRIMS)
def test_clip_zeroes_sigma_on_and_outside_the_faces_and_nothing_else(prim):
    net = model(prim)
    one = np.float32(1)
    inside, outside = np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2))
    rows = []
    for a in (one, -one):
        rows += [[a, 0.3, -0.2], [0.1, a, 0.4], [-0.7, 0.2, a], [a, -a, 0.5], [0.2, a, a], [a, a, -a]]          # faces, edges, corners
    on = np.array(rows, dtype=np.float32)
    pts = np.concatenate([on, on * inside, on * outside, np.array([[np.nan, 0, 0], [0, np.inf, 0], [0.5, -0.25, 0.125]], np.float32)]).astype(np.float32)
    # (x * inside: a coordinate of +-1 moves one ulp into the cube, the others shrink by a relative 6e-8 and stay inside)
    n_on = len(on)
    xyz = torch.from_numpy(pts).cuda()
    view = torch.tensor([0.3, -0.5, 0.8]).cuda()
    clipped = net.query(xyz, view)                       # clip=True is the default
    raw = net.query(xyz, view, clip=False)
    is_in = (np.abs(pts) < 1).all(axis=1)
    assert is_in[n_on:2 * n_on].all() and not is_in[:n_on].any() and not is_in[2 * n_on:3 * n_on + 2].any() and is_in[-1]
    sig, sig_raw = clipped["sigma"].cpu().numpy(), raw["sigma"].cpu().numpy()
    assert (sig[~is_in] == 0).all() and not np.signbit(sig[~is_in]).any()
    assert np.array_equal(sig[is_in].view(np.uint32), sig_raw[is_in].view(np.uint32)) and (sig[is_in] > 0).all()
    finite = np.isfinite(pts).all(axis=1)
    assert (sig_raw[finite] > 0).all()                   # the network's value everywhere
    for k in ("uv", "rgb"):
        a, b = clipped[k].cpu().numpy(), raw[k].cpu().numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.isfinite(a[finite]).all()
    assert torch.equal(net.query(xyz, want=("sigma",))["sigma"], clipped["sigma"])


LATTICES = [((5, 4, 3), (-1, -1, -1), (1, 1, 1)), (33, (-1, -1, -1), (1, 1, 1)), ((6, 7, 9), (-0.5, -0.25, 0), (0.5, 0.75, 1))]


@pytest.mark.parametrize("prim", PRIMS)
@pytest.mark.parametrize("res,lo,hi", LATTICES, ids=["5x4x3", "33", "subbox"])
def test_density_lattice_is_the_query_on_the_restated_points(prim, res, lo, hi):
    """33^3 = 35 937 points lie above the 32 768 one trip of a 256-CU grid covers: the grid-stride loop runs twice."""
    net = model(prim)
    shape = (res,) * 3 if isinstance(res, int) else res
    for clip in (True, False):
        vol, lo32, step = net.density_lattice(res, lo, hi, clip=clip)
        assert tuple(vol.shape) == shape and vol.dtype == torch.float32 and vol.device.type == "cuda" and vol.is_contiguous()
        assert lo32.dtype == np.float32 and np.array_equal(lo32, np.asarray(lo, np.float32)) and np.array_equal(step, Q.lattice_step(lo, hi, shape))
        pts = Q.lattice_points(lo32, step, shape)
        listed = net.query(torch.from_numpy(pts).cuda(), want=("sigma",), clip=clip)["sigma"]
        assert tuple(listed.shape) == shape and torch.equal(vol, listed)
        v = vol.cpu().numpy()
        if clip and tuple(lo) == (-1, -1, -1):
            for slab in (v[0], v[-1], v[:, 0], v[:, -1], v[:, :, 0], v[:, :, -1]):
                assert (slab == 0).all()
            assert (v[1:-1, 1:-1, 1:-1] > 0).all()
        else:
            assert (v[:-1, :-1, :-1] > 0).all()          # (the sub-box's upper faces y = 0.75 and z = 1: z = 1 is on the cube's face)
            if clip:
                assert (v[:, :, -1] == 0).all() and (v[:, :, :-1] > 0).all()
    assert torch.equal(net.density_lattice(res, lo, hi)[0], net.density_lattice(res, lo, hi)[0])


@pytest.mark.parametrize("prim", PRIMS)
def test_lattice_entries_meet_criterion_1(prim):
    net = model(prim)
    vol, lo32, step = net.density_lattice(33, clip=False)
    pts = Q.lattice_points(lo32, step, (33, 33, 33)).reshape(-1, 3)
    pick = (synth.hash_uniform(Q.SEED, 950, (64,)).astype(np.float64) * pts.shape[0]).astype(np.int64)
    pick[-1] = pts.shape[0] - 1                                                             # the last index among them
    p = torch.from_numpy(pts[pick])
    with torch.no_grad():
        f32 = Q.density(Q.make_net(prim, "cpu"), p).numpy()
        f64 = Q.density(Q.make_net(prim, "cpu", torch.float64), p.double()).numpy()
    criterion1(f"{prim} lattice 33^3, 64 entries", vol.reshape(-1)[torch.from_numpy(pick).cuda()].cpu().numpy(), f32, f64)


@pytest.mark.parametrize("prim", PRIMS)
def test_new_weights_are_seen(prim):
    xyz, view = xyz_view()
    net = Q.make_net(prim, "cuda")
    before = net.query(xyz, view, clip=False)
    assert all(torch.equal(before[k], full(prim)[k]) for k in before)
    net.load_params(synth.uvmapping_params(62, prim))
    after = net.query(xyz, view, clip=False)
    cpu32, cpu64 = Q.make_net(prim, "cpu", seed=62), Q.make_net(prim, "cpu", torch.float64, seed=62)
    f32 = Q.restate(cpu32, xyz.cpu(), view.cpu())
    f64 = Q.restate(cpu64, xyz.cpu().double(), view.cpu().double())
    for k in ("sigma", "uv", "rgb"):
        assert not torch.equal(after[k], before[k])
        criterion1(f"{prim}.{k} seed 62", after[k].cpu().numpy(), f32[k].numpy(), f64[k].numpy())


@pytest.mark.parametrize("prim", PRIMS)
def test_split_bf16_model_is_served_by_the_fp32_path(prim):
    xyz, view = xyz_view()
    net = uvmapping.NeuTex(primitive_type=prim, sample_num=64, split_bf16=True)
    net.load_params(synth.uvmapping_params(Q.SEED, prim))
    got = net.query(xyz, view, clip=False)
    assert all(torch.equal(got[k], full(prim)[k]) for k in ("sigma", "uv", "rgb"))
    assert torch.equal(net.density_lattice((5, 4, 3))[0], model(prim).density_lattice((5, 4, 3))[0])


def fits_half_turn(s_tri):
    """Per triangle: do its three s (modulo 1) lie on an arc of at most half a turn?"""
    srt = np.sort(np.mod(s_tri, 1.0), axis=1)
    gaps = np.concatenate([np.diff(srt, axis=1), srt[:, :1] + 1 - srt[:, 2:]], axis=1)
    return 1 - gaps.max(axis=1) <= 0.5


@pytest.mark.parametrize("prim", PRIMS)
@pytest.mark.parametrize("res", [17, (9, 17, 12)], ids=["17", "9x17x12"])
def test_export_mesh(prim, res, tmp_path):
    """Seed 61's density lies in 0.25 .. 0.9 and level 0.5 cuts most cells; the clipped boundary (0) is below the level, so the surface closes."""
    net = model(prim)
    TR = 16
    verts, faces, st = net.export_mesh(level=0.5, resolution=res, texture_resolution=TR)
    vol, lo, step = net.density_lattice(res)
    v2, f2 = mesh.marching_cubes(vol, 0.5, spacing=step.tolist(), origin=lo.tolist())
    assert verts.device.type == "cuda" and faces.dtype == torch.int32 and st.dtype == torch.float32 and tuple(st.shape) == (verts.shape[0], 2)
    assert verts.shape[0] > 100 and torch.equal(verts, v2) and torch.equal(faces, f2)
    assert mesh_ref.closed_and_oriented(faces.cpu().numpy())
    uv = net.query(verts, want=("uv",))["uv"]
    assert torch.equal(st, mesh.atlas_coords(uv, prim, TR if prim == "sphere" else None))
    st64 = Q.atlas_coords_f64(uv.cpu().numpy(), prim, TR)
    d = np.abs(st.cpu().numpy() - st64)
    d[:, 0] = np.minimum(d[:, 0], 1 - d[:, 0])                                  # (s modulo 1: a point next to the seam)
    assert d.max() <= 1e-5          # float32 acos / atan2 / remainder of values below 2 pi: a few ulp of 6e-8 each, against 1e-5
    # the files
    path = str(tmp_path / "model.obj")
    view = [0.3, -0.5, 0.8]
    got = net.export_mesh(path, level=0.5, resolution=res, viewdir=view, texture_resolution=TR)
    assert all(torch.equal(a, b) for a, b in zip(got, (verts, faces, st)))
    obj = Q.read_obj(path)
    assert np.array_equal(obj["v"].view(np.uint32), verts.cpu().numpy().view(np.uint32)) and np.array_equal(obj["f"], faces.cpu().numpy())
    st_ext, fvt = (mesh.unwrap_seam(faces, st) if prim == "sphere" else (st.cpu().numpy(), faces.cpu().numpy()))
    assert np.array_equal(obj["vt"].view(np.uint32), np.asarray(st_ext, np.float32).view(np.uint32)) and np.array_equal(obj["f_vt"], fvt)
    assert np.array_equal(obj["vt"][obj["f_vt"]][..., 1], st.cpu().numpy()[obj["f"]][..., 1])          # t is never touched; s: the spans below
    assert obj["mtllib"] == "model.mtl" and Q.read_mtl(Q.sibling(path, ".mtl"))["map_Kd"] == "model.png"
    from PIL import Image
    png = np.asarray(Image.open(Q.sibling(path, ".png")))
    tex = net.net_texture._export_sphere(TR, view) if prim == "sphere" else net.net_texture._export_square(TR, view)
    want = evalout.to_uint8((tex ** (1 / 2.2)).clamp(0, 1).contiguous()).cpu().numpy()
    assert png.shape == ((TR, 2 * TR, 3) if prim == "sphere" else (TR, TR, 3)) and np.array_equal(png, want)
    if prim == "sphere":
        s_tri = obj["vt"][obj["f_vt"]][..., 0].astype(np.float64)
        fits = fits_half_turn(s_tri)
        span = np.ptp(s_tri, axis=1)
        print(f"{prim} {res}: {len(fits)} triangles, {int((~fits).sum())} wider than half a turn, {int((obj['f_vt'] != obj['f']).any(axis=1).sum())} on the seam")
        assert (span[fits] <= 0.5).all()
    # diffuse atlas (viewdir None), normals and flip
    path2 = str(tmp_path / "diffuse.obj")
    v3, f3, _ = net.export_mesh(path2, level=0.5, resolution=res, texture_resolution=TR, normals=True, flip=True)
    v4, f4, n4 = mesh.marching_cubes(vol, 0.5, spacing=step.tolist(), origin=lo.tolist(), normals=True, flip=True)
    assert torch.equal(v3, v4) and torch.equal(f3, f4) and not torch.equal(f3, faces)
    obj2 = Q.read_obj(path2)
    assert np.array_equal(obj2["vn"].view(np.uint32), n4.cpu().numpy().view(np.uint32)) and np.array_equal(obj2["f_vn"], obj2["f"])
    assert np.array_equal(obj2["f"], f4.cpu().numpy())
    tex = net.net_texture._export_sphere(TR, None) if prim == "sphere" else net.net_texture._export_square(TR, None)
    assert np.array_equal(np.asarray(Image.open(Q.sibling(path2, ".png"))), evalout.to_uint8((tex ** (1 / 2.2)).clamp(0, 1).contiguous()).cpu().numpy())
    # a level above the volume's maximum: empty arrays and a valid empty OBJ
    path3 = str(tmp_path / "empty.obj")
    ve, fe, se = net.export_mesh(path3, level=float(vol.max()) + 1.0, resolution=res, texture_resolution=TR)
    assert tuple(ve.shape) == (0, 3) and tuple(fe.shape) == (0, 3) and tuple(se.shape) == (0, 2)
    obj3 = Q.read_obj(path3)
    assert obj3["v"].shape == (0, 3) and obj3["f"].shape == (0, 3) and obj3["mtllib"] == "empty.mtl" and os.path.exists(Q.sibling(path3, ".png"))
    with pytest.raises(TypeError):
        net.export_mesh(resolution=res)                  # level has no default
