"""Torch restatement of the UV-Mapping (NeuTex) training forward over the drop-in's own modules, for any dtype or device
(UV-Mapping/model/model.py:27-59, renderer.py:79-247, decoder.py, gauge_fields.py, util.py:427-438), and the reference's
compute_loss (model.py:300-349).  The reference itself cannot be imported where the GPU tests run; this carries its chain there.

``torch.rand`` of cube_ray_generation is replaced by ``U`` and the template's random points by ``template_points``.  The inverse
mapping runs the inverse network on the flattened uv (the reference's ``uv.view(input_shape, -1, D)`` raises in torch)."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from ngf_amd import synth, uvmapping


def positional_encoding(x, freqs):
    fb = (2 ** torch.arange(freqs).float()).to(x.device)
    pts = (x[..., None] * fb).reshape(x.shape[:-1] + (freqs * x.shape[-1],))
    return torch.cat([torch.sin(pts), torch.cos(pts)], dim=-1)


def cube_ray_generation(campos, raydir, S, U, jitter=0.05):
    with torch.no_grad():
        t1 = (-1.0 - campos[:, None, :]) / raydir
        t2 = (1.0 - campos[:, None, :]) / raydir
        tmin = torch.max(torch.min(t1[..., 0], t2[..., 0]), torch.max(torch.min(t1[..., 1], t2[..., 1]), torch.min(t1[..., 2], t2[..., 2])))
        tmax = torch.min(torch.max(t1[..., 0], t2[..., 0]), torch.min(torch.max(t1[..., 1], t2[..., 1]), torch.max(t1[..., 2], t2[..., 2])))
        inter = tmin < tmax
        t = torch.where(inter, tmin, torch.zeros_like(tmin)).clamp(min=0.0)
        dt = 2.0 / S
        seg = dt + dt * jitter * (U - 0.5)
        end = torch.cumsum(seg, dim=2)
        end = torch.cat([torch.zeros_like(end[:, :, :1]), end], dim=2)
        end = t[:, :, None] + end
        mid = (end[:, :, :-1] + end[:, :, 1:]) / 2
        pos = campos[:, None, None, :] + raydir[:, :, None, :] * mid[:, :, :, None]
        valid = torch.prod(torch.gt(pos, -1.0) * torch.lt(pos, 1.0), dim=-1).byte()
    return pos, seg, valid


def inverse_network(inv, x):
    x = F.relu(inv.linear1(x))
    x = F.relu(inv.linear2(x))
    for lin in inv.linear_list:
        x = F.relu(lin(x))
    return inv.last_linear(x)


def forward(net, campos, raydir, bg, U, template_points):
    """The training dict of model.py:27-59 (points_inverse computed eagerly)."""
    S = U.shape[-1]
    pos, seg, valid = cube_ray_generation(campos, raydir, S, U)
    density = F.softplus(net.net_geometry_decoder.block(torch.cat([pos, positional_encoding(pos, 10)], dim=-1))[..., 0])
    inv = net.inverse_gauge.inverse_network
    pts3 = inverse_network(inv, template_points.unsqueeze(0)).unsqueeze(1)
    points = pts3.view(pts3.shape[0], -1, pts3.shape[-1]).permute(0, 2, 1)
    e = net.gauge_transform.encoder
    x = F.relu(e.linear1(torch.cat([pos, positional_encoding(pos, 10)], dim=-1)))
    x = F.relu(e.linear2(x))
    for lin in e.linear_list:
        x = F.relu(lin(x))
    q = e.last_linear(x)
    uv = torch.tanh(q) if q.shape[-1] == 2 else F.normalize(q, dim=-1)
    t = net.net_texture
    h = t.block1(torch.cat([uv, positional_encoding(uv, 10)], dim=-1))
    c1 = F.softplus(t.color1(h))
    vd = raydir[:, :, None, :].expand(h.shape[:-1] + (3,))
    c2 = t.block2(torch.cat([h, vd, positional_encoding(vd, 6)], dim=-1))
    radiance = (c1 + c2).clamp(min=0)
    sigma = density * valid.to(density.dtype)
    opacity = 1 - torch.exp(-sigma * seg)
    acc = torch.cumprod(1.0 - opacity + 1e-10, dim=-1)
    bgT = acc[:, :, -1]
    acc = torch.cat([torch.ones_like(acc[:, :, :1]), acc[:, :, :-1]], dim=-1)
    w = opacity * acc
    color = torch.sum(radiance * w[..., None], dim=-2)
    if bg is not None:
        color = color + bg[:, None, :] * bgT[:, :, None]
    color = torch.pow(color + 1e-5, 1 / 2.2).clamp_(0, 1)
    pinv = inverse_network(inv, uv.reshape(-1, uv.shape[-1])).view(uv.shape[:-1] + (3,))
    return {"color": color, "transmittance": bgT, "points": points, "points_original": pos, "points_inverse": pinv,
            "points_inverse_weights": w, "uv": uv}


def compute_loss(out, gt_image, gt_trans, weights=(1.0, 1.0, 1.0, 0.0)):
    """model.py:300-349 with (color, bg, origin, inverse-mapping) weights."""
    total = 0
    if weights[0] > 0:
        total = total + weights[0] * F.mse_loss(out["color"], gt_image)
    if weights[1] > 0:
        total = total + weights[1] * F.mse_loss(out["transmittance"], gt_trans)
    if weights[2] > 0:
        total = total + weights[2] * (((out["points"] ** 2).sum(-2) - 1).clamp(min=0).sum())
    if weights[3] > 0:
        dist = ((out["points_original"] - out["points_inverse"]) ** 2).sum(-1)
        total = total + weights[3] * (dist * out["points_inverse_weights"]).sum(-1).mean()
    return total


def inverse_params(seed, primitive_type):
    """Seeded inverse-network parameters (inverse_gauge.inverse_network.*), scaled like a fan-in initialisation."""
    D = 2 if primitive_type == "square" else 3
    shapes = [("linear1", 64, D), ("linear2", 512, 64), ("linear_list.0", 512, 512), ("linear_list.1", 512, 512), ("last_linear", 3, 512)]
    p = {}
    for i, (n, o, k) in enumerate(shapes):
        p[f"inverse_gauge.inverse_network.{n}.weight"] = (synth.hash_normal(seed, 950 + 2 * i, (o, k)) * np.float32(np.sqrt(2.0 / k))).astype(np.float32)
        p[f"inverse_gauge.inverse_network.{n}.bias"] = (synth.hash_normal(seed, 951 + 2 * i, (o,)) * np.float32(0.05)).astype(np.float32)
    return p


def model_params(seed, primitive_type):
    p = dict(synth.uvmapping_params(seed, primitive_type))
    p.update(inverse_params(seed, primitive_type))
    return p


def batch(seed, primitive_type, R=48, S=64, P=64, n_cams=1):
    """DTU-like rays with misses, jitter uniforms, template points, targets (numpy, float32)."""
    campos, dirs = synth.dtu_rays(600, 800)
    cams, rds = [], []
    for c in range(n_cams):
        pick = (synth.hash_uniform(seed + c, 600, (R,)) * np.float32(dirs.shape[0])).astype(np.int64)
        rd = dirs[pick].copy()
        rd[-4:] = np.array([[0.3, 0.9, 0.3], [-0.6, 0.1, 0.79], [0, 0, 1], [0.577, 0.577, 0.578]], np.float32)
        rd = rd / np.linalg.norm(rd, axis=1, keepdims=True)
        cp = np.asarray(campos, np.float32) * np.float32(1.0 + 0.05 * c)
        cams.append(cp)
        rds.append(rd)
    U = synth.hash_uniform(seed, 601, (n_cams, R, S))
    if primitive_type == "square":
        tp = synth.hash_uniform(seed, 602, (P, 2)) * np.float32(2) - np.float32(1)
    else:
        q = synth.hash_normal(seed, 602, (P, 3)) * np.float32(2) - np.float32(1)
        tp = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    gt = synth.hash_uniform(seed, 603, (n_cams, R, 3))
    gtt = synth.hash_uniform(seed, 604, (n_cams, R))
    return {"campos": np.stack(cams).astype(np.float32), "raydir": np.stack(rds).astype(np.float32), "U": U, "template": tp.astype(np.float32),
            "gt_image": gt, "gt_trans": gtt}


def make_net(params, primitive_type, S, device, dtype=torch.float32):
    net = uvmapping.NeuTex(primitive_type=primitive_type, sample_num=S, device=device, points_per_primitive=64)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()}, strict=True)
    return net.to(dtype=dtype)


def probes(name, shape):
    """Seeded probe matrices of a gradient tensor: L [4, out], R [in, 4] (a bias is an [out, 1] matrix)."""
    out, inn = (shape[0], shape[1] if len(shape) > 1 else 1)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    return rng.standard_normal((4, out)), rng.standard_normal((inn, 4))


def probe_products(name, grad):
    """L . G . R (4 x 4, float64) of a gradient tensor (numpy or torch)."""
    g = np.asarray(grad.detach().cpu().double().numpy() if hasattr(grad, "detach") else grad, np.float64)
    g = g.reshape(g.shape[0], -1)
    L, R = probes(name, g.shape)
    return L @ g @ R


def fixture_grads(g, dt, tag):
    """{name: (norm, entries, probe products)} of a tests/golden/uv_train_*.npz fixture."""
    names = [str(n) for n in g["names"]]
    ends = np.cumsum(g["idx_len"])
    starts = ends - g["idx_len"]
    return {k: (float(g[f"{dt}.{tag}.gnorm"][i]), g[f"{dt}.{tag}.gval"][starts[i]:ends[i]].astype(np.float64), g[f"{dt}.{tag}.probe"][i])
            for i, k in enumerate(names)}


def fixture_idx(g):
    names = [str(n) for n in g["names"]]
    ends = np.cumsum(g["idx_len"])
    return {k: g["idx"][e - n:e] for k, e, n in zip(names, ends, g["idx_len"])}
