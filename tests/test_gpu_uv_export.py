"""GPU: the UV-Mapping texture export (csrc/ngf_uv_export.hpp through ngf_uv_texture_eval, uvmapping.NeuTex.texture_colors and the
net_texture exporters) against the reference decoder's own outputs (tests/golden/uv_export.npz).

Criterion: the GPU's max-abs distance to the reference's fp64 output is at most 4x the distance of the reference's own
fp32 output to it, both taken from the fixture; absolute, over every value, nothing masked."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ngf_amd  # noqa: E402,F401
from ngf_amd import synth, uvmapping  # noqa: E402
import uv_export_eager as E  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden")
G = np.load(os.path.join(GOLDEN, "uv_export.npz"))
G_EDIT = np.load(os.path.join(GOLDEN, "uv_edit.npz"))


def model(prim):
    return E.make_net(prim, "cuda")


def check_against_fp64(name, got, f32, f64):
    ref = float(np.abs(f32.astype(np.float64) - f64).max())
    err = float(np.abs(got.astype(np.float64) - f64).max())
    print(f"{name}: max|hip - fp64| = {err:.3e}, max|reference fp32 - fp64| = {ref:.3e}, bound {4 * ref:.3e}")
    assert np.isfinite(got).all()
    assert err <= 4 * ref, (name, err, ref)


@pytest.mark.parametrize("case", E.CASES, ids=[c[0] for c in E.CASES])
def test_export_matches_the_reference(case):
    key, prim, kind, R, viewdir, with_edit = case
    net = model(prim)
    if with_edit:
        net.set_target_texture(E.edit_texture(G_EDIT, prim), 1)
    got = E.export(net.net_texture, kind, R, viewdir)
    want = G[key + ".f64"]
    assert got.device.type == "cuda" and got.dtype == torch.float32 and not got.requires_grad and tuple(got.shape) == want.shape
    check_against_fp64(key, got.cpu().numpy(), G[key + ".f32"], want)


def test_reference_driver_call_sites():
    """UV-Mapping/test.py:58-88 on the drop-in: export, gamma, merge, clamp."""
    viewdir = [0, 0, 1]
    net = model("sphere")
    texture = net.net_texture.export_textures(32, viewdir) ** (1 / 2.2)
    texture = uvmapping.merge_cube_to_single_texture(texture)
    texture = texture.clamp(0, 1).data.cpu().numpy()
    want = uvmapping.merge_cube_to_single_texture(torch.from_numpy(G["sphere.cube32.view.f64"]) ** (1 / 2.2)).clamp(0, 1).numpy()
    assert texture.shape == (96, 128, 3) and (texture * 255).astype(np.uint8).shape == (96, 128, 3)
    assert np.abs(texture - want)[want > 0.05].max() < 1e-4        # (the gamma curve is steep at 0: compared away from it)
    sph = (net.net_texture._export_sphere(16, viewdir) ** (1 / 2.2)).clamp(0, 1).data.cpu().numpy()
    assert sph.shape == (16, 32, 3)
    square = model("square")
    sq = (square.net_texture.export_textures(32, viewdir) ** (1 / 2.2)).clamp(0, 1).data.cpu().numpy()
    assert sq.shape == (32, 32, 3)
    net_texture = model("square").net_texture          # the decoder of a model that is gone: a clear refusal, not a stale handle
    with pytest.raises(RuntimeError, match="NeuTex"):
        net_texture.export_textures(8)
    assert tuple(net.net_texture.export_textures(8).shape) == (6, 8, 8, 3)          # the defaults' view direction


@pytest.mark.parametrize("prim", ["sphere", "square"])
def test_texture_colors_per_point_view_and_ragged_sizes(prim):
    """Per-point view directions (the edit fixture's: uv_edit.npz `plain` is the reference decoder's output for them), n = 1, n not a
    multiple of the 32-point pass, and a 2-column uv for the square model."""
    net = model(prim)
    n = 160
    uv = torch.from_numpy(G_EDIT[f"{prim}.uv"])
    view = synth.hash_normal(int(G_EDIT["seed"]), 920 + (3 if prim == "sphere" else 2), (n, 3))
    view = torch.from_numpy((view / np.linalg.norm(view, axis=1, keepdims=True)).astype(np.float32))
    net64 = E.make_net(prim, "cpu", torch.float64)
    with torch.no_grad():
        f64 = E.texture_forward(net64.net_texture, uv.double(), view.double()).numpy()
        f64_diffuse = E.texture_forward(net64.net_texture, uv.double()).numpy()
    f32 = G_EDIT[f"{prim}.plain"]
    full = net.texture_colors(uv, view)
    check_against_fp64(f"{prim} per-point view n=160", full.cpu().numpy(), f32, f64)
    for m in (1, 17, 33, 47, 159):
        part = net.texture_colors(uv[:m], view[:m])
        assert tuple(part.shape) == (m, 3) and torch.equal(part, full[:m]), m        # a point's colour does not depend on the launch around it
    one = net.texture_colors(uv[5], view[5])
    assert tuple(one.shape) == (3,) and torch.equal(one, full[5])
    shaped = net.texture_colors(uv[:156].view(4, 39, 3), view[:156].view(4, 39, 3))
    assert torch.equal(shaped.view(-1, 3), full[:156])
    shared = net.texture_colors(uv[:40], view[7])
    assert torch.equal(shared[7], full[7]) and torch.equal(shared, net.texture_colors(uv[:40], view[7].expand(40, 3)))
    dif = net.texture_colors(uv[:47], diffuse=True)
    with torch.no_grad():
        d32 = E.texture_forward(E.make_net(prim, "cpu").net_texture, uv[:47]).numpy()
    check_against_fp64(f"{prim} diffuse n=47", dif.cpu().numpy(), d32, f64_diffuse[:47])
    if prim == "square":
        assert torch.equal(net.texture_colors(uv[:33, :2], view[:33]), full[:33])
    with pytest.raises(ValueError):
        net.texture_colors(uv[:4])                       # view mode without a direction
    assert tuple(net.texture_colors(uv[:0], view[:0]).shape) == (0, 3)


@pytest.mark.parametrize("prim,kind", [("sphere", "cube"), ("sphere", "equi"), ("square", "sq")])
def test_two_exports_are_bit_identical(prim, kind):
    net = model(prim)
    for viewdir in ([0.3, -0.5, 0.8], None):
        a = E.export(net.net_texture, kind, 24, viewdir)
        b = E.export(net.net_texture, kind, 24, viewdir)
        other = model(prim)
        c = E.export(other.net_texture, kind, 24, viewdir)
        assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("prim", ["sphere", "square"])
def test_clearing_the_edit_texture_restores_the_plain_export(prim):
    net = model(prim)
    plain = net.net_texture.export_textures(32)
    diffuse = net.net_texture.export_textures(32, None)
    net.set_target_texture(E.edit_texture(G_EDIT, prim), 1)
    edited = net.net_texture.export_textures(32)
    assert not torch.equal(edited, plain)
    assert torch.equal(net.net_texture.export_textures(32, None), diffuse)          # the diffuse branch has no edit stage
    net.set_target_texture(None)
    assert torch.equal(net.net_texture.export_textures(32), plain)


def test_round_trip_sphere():
    """export -> clamp -> set_target_texture(mode 4) -> texture_edit at the export's own directions gives the export back, within 4x the
    residue of the reference doing the same with its own export (fixture)."""
    net = model("sphere")
    cube = net.net_texture.export_textures(32).clamp(0, 1)
    net.set_target_texture(cube, mode=4)
    pts = uvmapping.export_cube_points(32).reshape(-1, 3)
    back = net.texture_edit(pts, torch.zeros_like(pts)).view(6, 32, 32, 3)
    err, ref = float((back - cube).abs().max()), float(G["rt.sphere.residue"])
    print(f"sphere round trip: {err:.3e} (reference {ref:.3e})")
    assert err <= 4 * ref


def test_round_trip_square():
    """The same for the square atlas, which the exporter indexes [i <-> u, j <-> v]: the transpose of what sample_square reads."""
    net = model("square")
    atlas = net.net_texture.export_textures(32).clamp(0, 1)
    net.set_target_texture(atlas.transpose(0, 1).contiguous(), mode=4)
    g = uvmapping.export_square_points(32).reshape(-1, 2)
    pts = torch.cat([g, torch.zeros(g.shape[0], 1)], dim=-1)
    back = net.texture_edit(pts, torch.zeros_like(pts)).view(32, 32, 3)
    err, ref = float((back - atlas).abs().max()), float(G["rt.square.residue"])
    print(f"square round trip: {err:.3e} (reference {ref:.3e})")
    assert err <= 4 * ref


def test_a_parameter_update_changes_the_next_export():
    net = model("sphere")
    before = net.net_texture.export_textures(16)
    with torch.no_grad():
        net.net_texture.color1.bias[0] += 0.25
    after = net.net_texture.export_textures(16)
    assert not torch.equal(before, after)
    assert float((after[..., 1:] - before[..., 1:]).abs().max()) == 0.0          # the other channels' arithmetic is untouched
    assert float((after[..., 0] - before[..., 0]).max()) > 0.05


def test_an_export_leaves_the_render_unchanged():
    """The inputs of test_gpu_uv_edit.test_render_with_edit_texture, rendered before and after export calls, with and without an edit texture."""
    net = model("sphere")
    campos, dirs = synth.dtu_rays(600, 800)
    pick = (synth.hash_uniform(3, 1, (96,)) * np.float32(dirs.shape[0])).astype(np.int64)
    rd = torch.from_numpy(dirs[pick])[None].cuda()
    cp = torch.from_numpy(campos)[None].cuda()
    U = torch.from_numpy(synth.hash_uniform(3, 2, (1, 96, 64))).cuda()
    for tex in (None, np.full((6, 4, 4, 3), 0.8, np.float32)):
        net.set_target_texture(tex, 4)
        first = net(cp, rd, None, jitter_u=U)
        net.net_texture.export_textures(32)
        net.net_texture.export_textures(17, None)
        net.net_texture._export_sphere(8, [0.3, -0.5, 0.8])
        again = net(cp, rd, None, jitter_u=U)
        assert torch.equal(first["color"], again["color"]) and torch.equal(first["transmittance"], again["transmittance"])


def test_split_bf16_handle_is_served_by_the_fp32_path():
    plain = model("sphere")
    a = plain.net_texture.export_textures(16)
    net = uvmapping.NeuTex(primitive_type="sphere", sample_num=64, split_bf16=True)
    net.load_params(synth.uvmapping_params(E.SEED, "sphere"))
    assert torch.equal(net.net_texture.export_textures(16), a)
