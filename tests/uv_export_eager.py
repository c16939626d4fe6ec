"""Torch restatement of the UV-Mapping texture decoder on explicit points, for any dtype or device, over the drop-in's own modules
(UV-Mapping/model/decoder.py:56-179, util.py:172-238, 277-282, 427-438), and the list of export cases that tests/golden/uv_export.npz holds.
The reference itself cannot be imported where the GPU tests run; this carries its chain there."""
import numpy as np
import torch
import torch.nn.functional as F

from ngf_amd import synth, uvmapping

SEED = 61          # the weights of tests/golden/uv_edit.npz

# (fixture key, primitive, point set, resolution, view direction or None = diffuse, edit texture set with mode 1)
CASES = [
    ("sphere.cube32.view", "sphere", "cube", 32, [0, 0, 1], False),
    ("sphere.cube32.diffuse", "sphere", "cube", 32, None, False),
    ("sphere.equi16.view", "sphere", "equi", 16, [0, 0, 1], False),
    ("sphere.cube17.view", "sphere", "cube", 17, [0.3, -0.5, 0.8], False),
    ("sphere.cube32.edit1", "sphere", "cube", 32, [0, 0, 1], True),
    ("square.sq32.view", "square", "sq", 32, [0, 0, 1], False),
    ("square.sq32.diffuse", "square", "sq", 32, None, False),
    ("square.sq17.view", "square", "sq", 17, [0.3, -0.5, 0.8], False),
    ("square.sq32.edit1", "square", "sq", 32, [0, 0, 1], True),
]
POINT_SETS = sorted({(prim, kind, R) for _, prim, kind, R, _, _ in CASES})


def points_key(prim, kind, R):
    return f"pts.{prim}.{kind}{R}"


def build_points(kind, R):
    """The drop-in's own point builders (for ``equi``: before the exporter's final flip)."""
    return {"cube": uvmapping.export_cube_points, "equi": uvmapping.export_sphere_points, "sq": uvmapping.export_square_points}[kind](R)


def export(tex, kind, R, viewdir):
    """The exporter a case names, on any object with the reference's method names (the reference decoder or the drop-in's)."""
    if kind == "equi":
        return tex._export_sphere(R, viewdir)
    return tex.export_textures(R, viewdir)


def positional_encoding(x, freqs):
    fb = (2 ** torch.arange(freqs)).to(x)
    pts = (x[..., None] * fb).reshape(x.shape[:-1] + (freqs * x.shape[-1],))
    return torch.cat([torch.sin(pts), torch.cos(pts)], dim=-1)


def _grid_sample(tex, uv):
    out = F.grid_sample(tex.permute(2, 0, 1)[None], uv.reshape(1, -1, 1, 2), padding_mode="border", align_corners=False)
    return out.permute(0, 2, 3, 1).reshape(uv.shape[:-1] + (tex.shape[-1],))


def sample_cubemap(cube, xyz):
    """util.py:172-238: the six face masks in order, a later face overwrites an earlier one on ties."""
    x, y, z = xyz.unbind(-1)
    ax, ay, az = x.abs(), y.abs(), z.abs()
    mx, my, mz = (ax >= ay) & (ax >= az), (ay >= ax) & (ay >= az), (az >= ax) & (az >= ay)
    faces = [((x > 0) & mx, -z, y, ax), (~(x > 0) & mx, z, y, ax), ((y > 0) & my, x, -z, ay), (~(y > 0) & my, x, z, ay),
             ((z > 0) & mz, x, y, az), (~(z > 0) & mz, -x, y, az)]
    result = torch.zeros(xyz.shape[:-1] + (cube.shape[-1],), dtype=xyz.dtype, device=xyz.device)
    for tex, (m, u, v, a) in zip(cube.unbind(0), faces):
        result[m] = _grid_sample(tex, torch.stack([u[m] / a[m], v[m] / a[m]], dim=-1))
    return result


def sample_square(square, uv):
    return _grid_sample(square, uv)


def texture_forward(tex, uv, view=None, cubemap=None, mode=0):
    """TextureMlpDecoder.forward (view given) or the exporters' viewdir=None branch (view None), in the dtype of ``tex``'s parameters."""
    D = tex.block1[0].in_features // 21
    p = uv[..., :D]
    h = tex.block1(torch.cat([p, positional_encoding(p, 10)], dim=-1))
    if view is None:
        return torch.sigmoid(tex.color1(h))
    vd = view.expand(h.shape[:-1] + (3,))
    orig = F.softplus(tex.color1(h)) + tex.block2(torch.cat([h, vd, positional_encoding(vd, 6)], dim=-1))
    if cubemap is None:
        return orig.clamp(min=0)
    # the texture look-up in float32 whatever the dtype of the MLPs (the reference's sample_cubemap runs in no other; the fixture's fp64 outputs
    # were captured that way), on points that are float32 values
    cm, pf = cubemap.float(), p.float()
    cc = (sample_cubemap(cm, pf) if D == 3 else sample_square(cm, pf))[..., :3].to(orig.dtype)
    if mode == 0:
        return cc * (orig * 8).clamp(0, 1).mean(dim=-1, keepdim=True)
    if mode == 4:
        return cc.clamp(0, 1)
    o = orig.clamp(0, 1)
    if mode == 1:
        return torch.where((cc[..., :1] < 0.99).expand_as(o), o * cc, o)
    if mode == 2:
        return torch.where((cc[..., :1] < 0.99).expand_as(o), o * (1 / cc), o)
    m = (cc.sum(-1, keepdim=True) > 0.01).expand_as(o)
    return torch.where(m, 2 * o.mean(-1, keepdim=True) * cc, o) + cc


def make_net(prim, device, dtype=torch.float32):
    net = uvmapping.NeuTex(primitive_type=prim, sample_num=64, device=device)
    net.load_params(synth.uvmapping_params(SEED, prim))
    return net.to(dtype) if dtype != torch.float32 else net


def edit_texture(G_edit, prim):
    return np.ascontiguousarray(G_edit[f"{prim}.tex"][..., :3])
