"""Torch restatement of the UV-Mapping (NeuTex) training forward over the drop-in's own modules, for any dtype or device
(UV-Mapping/model/model.py:27-59, renderer.py:79-247, decoder.py, gauge_fields.py, util.py:427-438), and the reference's
compute_loss (model.py:300-349).  The reference itself cannot be imported where the GPU tests run; this carries its chain there.

``torch.rand`` of cube_ray_generation is replaced by ``U`` and the template's random points by ``template_points``.  The inverse
mapping runs the inverse network on the flattened uv (the reference's ``uv.view(input_shape, -1, D)`` raises in torch)."""
import functools
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


def forward(net, campos, raydir, bg, U, template_points, extras=False):
    """The training dict of model.py:27-59 (points_inverse computed eagerly).  extras: also "valid", "raw_density" and "color1_pre" (the
    softplus arguments of every sample) and "color_unclamped" (the tone-mapped colour before clamp_(0, 1))."""
    S = U.shape[-1]
    pos, seg, valid = cube_ray_generation(campos, raydir, S, U)
    raw = net.net_geometry_decoder.block(torch.cat([pos, positional_encoding(pos, 10)], dim=-1))[..., 0]
    density = F.softplus(raw)
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
    c1_pre = t.color1(h)
    c1 = F.softplus(c1_pre)
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
    unclamped = torch.pow(color + 1e-5, 1 / 2.2)
    color = unclamped.clone().clamp_(0, 1)
    pinv = inverse_network(inv, uv.reshape(-1, uv.shape[-1])).view(uv.shape[:-1] + (3,))
    out = {"color": color, "transmittance": bgT, "points": points, "points_original": pos, "points_inverse": pinv,
           "points_inverse_weights": w, "uv": uv}
    if extras:
        out.update(valid=valid.bool(), raw_density=raw.detach(), color1_pre=c1_pre.detach(), color_unclamped=unclamped.detach())
    return out


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


# ---- batches at the edges (tests/test_gpu_uv_train_edges.py, tests/test_uv_train_edges_cpu.py) -------------------------------------------------
EDGE_SEEDS = (311, 312, 313)                         # every case runs on three seeds (model and batch)
EDGE_V, EDGE_V_S = (0, 1, 17, 1023, 1024, 1025, 2049), 23
EDGE_RAYS, EDGE_RAYS_S = (1, 257, 1025, 2051), 5
EDGE_CAMS = (3, 343)                                 # cameras x rays per camera, at EDGE_RAYS_S samples
POOL_STRIDE = 97          # every 97th ray of the 600 x 800 DTU frame: 4949 rays
FACE_MARGIN = 1e-5        # a pool ray is used only if each of its samples stays this far from every cube face


def in_cube_counts(campos, raydir, U):
    """fp64 in-cube count per ray and the smallest distance of any of its samples to a cube face (campos [3], raydir [R,3], U [R,S])."""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))          # noqa: E731
    pos, _, valid = cube_ray_generation(t(campos)[None], t(raydir)[None], U.shape[-1], t(U)[None])
    margin = (pos.abs() - 1.0).abs().amin(dim=(-1, -2))[0].numpy()
    return valid[0].sum(-1).numpy().astype(np.int64), margin


@functools.lru_cache(maxsize=32)
def _pool(seed, S, c):
    """camera c of a seed: its position, the pool's directions and jitter rows, their fp64 counts and margins, the usable rays in seeded order"""
    campos, dirs = synth.dtu_rays(600, 800)
    pool = dirs[::POOL_STRIDE]
    pool = (pool / np.linalg.norm(pool, axis=1, keepdims=True)).astype(np.float32)
    n = pool.shape[0]
    cp = (np.asarray(campos, np.float32) * np.float32(1.0 + 0.05 * c)).astype(np.float32)
    Up = synth.hash_uniform(seed + c, 601, (n, S))
    cnt, mg = in_cube_counts(cp, pool, Up)
    order = np.argsort(synth.hash_uniform(seed + c, 600, (n,)), kind="stable")
    return cp, pool, Up, cnt, mg, order[mg[order] >= FACE_MARGIN]


def edge_batch(seed, primitive_type, S, V=None, R=None, n_cams=1, misses=3, P=64):
    """A batch like ``batch`` whose rays come from the pool by their fp64 in-cube counts at S samples, every sample at least FACE_MARGIN
    away from the faces (so fp32 and fp64 agree on which samples are in the cube).  V: one camera, the fewest rays whose counts add up to
    exactly V in-cube samples, then `misses` rays that miss, then one more if the ray count is a multiple of 16 (rays x S stays ragged
    for odd S).  R: R rays per camera in a seeded order, whatever their counts; camera c stands at campos (1 + 0.05 c).
    Adds "counts" [n_cams, R] and "margin" (the smallest face distance of the batch) to the dict of ``batch``."""
    cams, rds, Us, cnts, margin = [], [], [], [], np.inf
    for c in range(n_cams):
        cp, pool, Up, cnt, mg, order = _pool(seed, S, c)
        if V is not None:
            assert n_cams == 1
            pick, left = [], int(V)
            for j in order[np.argsort(-cnt[order], kind="stable")]:
                if 0 < cnt[j] <= left:
                    pick.append(j)
                    left -= int(cnt[j])
            assert left == 0, "the pool cannot reach this count"
            miss = [j for j in order if cnt[j] == 0]
            pick += miss[:misses + (1 if (len(pick) + misses) % 16 == 0 else 0)]
            pick = np.asarray(pick, np.int64)
        else:
            pick = order[:R]
            assert len(pick) == R
        cams.append(cp)
        rds.append(pool[pick])
        Us.append(Up[pick])
        cnts.append(cnt[pick])
        margin = min(margin, float(mg[pick].min()))
    Rn = rds[0].shape[0]
    if primitive_type == "square":
        tp = synth.hash_uniform(seed, 602, (P, 2)) * np.float32(2) - np.float32(1)
    else:
        q = synth.hash_normal(seed, 602, (P, 3)) * np.float32(2) - np.float32(1)
        tp = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    return {"campos": np.stack(cams).astype(np.float32), "raydir": np.stack(rds).astype(np.float32), "U": np.stack(Us).astype(np.float32),
            "template": tp.astype(np.float32), "gt_image": synth.hash_uniform(seed, 603, (n_cams, Rn, 3)),
            "gt_trans": synth.hash_uniform(seed, 604, (n_cams, Rn)), "counts": np.stack(cnts), "margin": margin}


DENSITY_BIAS, COLOR1_BIAS = "net_geometry_decoder.block.22.bias", "net_texture.color1.bias"


def softplus_case(seed, which, R=24, S=24):
    """A square model and batch whose softplus arguments straddle torch's threshold of 20 (the seeded ones stay below 2.2, so that branch of
    uvt_softplus / uvt_dsoftplus never runs otherwise).  which = "density": the density bias is shifted so that 20 falls into the widest gap between the raw densities
    of the in-cube samples around their median.  which = "color1": the colour1 bias likewise, and the density bias DOWN to a median raw density of -4.5, so
    that the pixels stay below the tone map's clamp and d color1 is not zero.  The shifts come from the fp64 restatement on the CPU.
    -> (params, batch, stats) with stats = the fp64 shares the tests assert: "above" (share of the in-cube arguments above 20), "gap" (the
    smallest |argument - 20|: fp32 and fp64 must take the same branch) and "unclamped" (share of the colour values below the clamp)."""
    params = model_params(seed, "square")
    b = batch(seed, "square", R=R, S=S)
    t = lambda k: torch.from_numpy(b[k]).double()          # noqa: E731

    def look(p):
        net = make_net(p, "square", S, "cpu", torch.float64)
        with torch.no_grad():
            o = forward(net, t("campos"), t("raydir"), None, t("U"), t("template"), extras=True)
        v = o["valid"]
        return o["raw_density"][v], o["color1_pre"][v], o["color_unclamped"]

    def shifted(p, name, by):
        q = dict(p)
        q[name] = (np.asarray(p[name], np.float64) + by).astype(np.float32)
        return q

    def split_point(a):
        """the middle of the widest gap between neighbouring values from the 40th to the 60th percentile: no argument lands near 20"""
        a = np.sort(a.reshape(-1).numpy())
        a = a[int(0.4 * a.size):int(0.6 * a.size) + 1]
        i = int(np.argmax(np.diff(a)))
        return 0.5 * float(a[i] + a[i + 1])

    raw, c1, _ = look(params)
    if which == "density":
        params = shifted(params, DENSITY_BIAS, 20.0 - split_point(raw))
    else:
        params = shifted(shifted(params, COLOR1_BIAS, 20.0 - split_point(c1)), DENSITY_BIAS, -4.5 - float(raw.median()))
    raw, c1, unclamped = look(params)
    arg = raw if which == "density" else c1
    stats = {"above": float((arg > 20).double().mean()), "gap": float((arg - 20).abs().min()), "unclamped": float((unclamped < 1).double().mean()),
             "in_cube": int(raw.numel())}
    return params, b, stats
