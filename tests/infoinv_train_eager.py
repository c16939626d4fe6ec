"""Torch restatement of the InfoInv training-mode forward for any dtype and device, written from this project's own port (oracle/eager.py,
oracle/train.py): sample_ray with pinned jitter, the box test and the alpha mask, the PE modulation on and off, the density MLP,
softplus(o - 10) and raw2alpha, the active set, the basis, the view encoding and the colour MLP, compositing, the white background and the
clamp.  The GPU tests run it in float64 (the truth) and float32 (the yardstick) next to the HIP trainers; the port itself is float32 on the
host only.

``edge_batch`` builds batches whose valid and active sets are the same in float32 and float64 (every sample FACE_MARGIN away from the box
faces, every weight WEIGHT_MARGIN away from the threshold, relative to it) and can hit an exact active count; ``softplus_case`` puts the
arguments of softplus on both sides of ATen's threshold of 20."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from ngf_amd import geometry, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARAM_NAMES = ('plane_xy', 'plane_yz', 'plane_xz',
               'density_decoder.mlp.0.weight', 'density_decoder.mlp.0.bias', 'density_decoder.mlp.2.weight', 'density_decoder.mlp.2.bias',
               'density_decoder.mlp.4.weight', 'density_decoder.mlp.4.bias',
               'rgb_decoder.basis.weight', 'rgb_decoder.mlp.0.weight', 'rgb_decoder.mlp.0.bias', 'rgb_decoder.mlp.2.weight',
               'rgb_decoder.mlp.2.bias', 'rgb_decoder.mlp.4.weight', 'rgb_decoder.mlp.4.bias')
DENSITY = PARAM_NAMES[:9]          # what the density reaches: the planes (their first 24 channels) and the density MLP
COLOUR = PARAM_NAMES[9:]           # what only an active sample reaches
DD = 24                            # density channels per plane


def posenc(x, freqs):
    bands = 2.0 ** torch.arange(freqs, dtype=x.dtype, device=x.device)
    y = (x[..., None] * bands).reshape(*x.shape[:-1], -1)
    return torch.cat([torch.sin(y), torch.cos(y)], -1)


def sample2d(plane, uv):
    """[1,C,H,W] sampled at uv [M,2] -> [M,C] (bilinear, zeros padding, align_corners=True)."""
    return F.grid_sample(plane, uv.reshape(1, -1, 1, 2), align_corners=True).reshape(plane.shape[1], -1).T


class Eager:
    """The field of a geometry dict ``g`` (aabb, grid, near_far, distance_scale, thr, step_ratio: a fixture's keys) with differentiable
    parameters of ``dtype``.  mask: (np.packbits image, (D, H, W), aabb [2,3]) or None."""

    def __init__(self, params, g, dtype=torch.float32, device="cpu", mask=None):
        t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(device=device, dtype=dtype)          # noqa: E731
        self.dtype, self.device = dtype, device
        self.p = {k: t(params[k]).requires_grad_(True) for k in PARAM_NAMES}
        self.aabb = t(g["aabb"]).reshape(2, 3)
        self.inv = 2.0 / (self.aabb[1] - self.aabb[0])
        self.step = t(geometry.step_size(g["aabb"], g["grid"], float(g["step_ratio"])))
        self.near, self.far = float(g["near_far"][0]), float(g["near_far"][1])
        self.dscale, self.thr = float(g["distance_scale"]), float(np.float32(g["thr"]))
        self.mask = None
        if mask is not None:
            bits, dhw, maabb = mask
            vol = np.unpackbits(np.asarray(bits))[:int(np.prod(dhw))].reshape(tuple(int(v) for v in dhw)).astype(np.float32)
            maabb = t(maabb).reshape(2, 3)
            self.mask = (t(vol)[None, None], maabb, 1.0 / (maabb[1] - maabb[0]) * 2)

    def _feats(self, c, lo, hi, pe):
        out = []
        for name, uv in zip(PARAM_NAMES[:3], c):
            f = sample2d(self.p[name][:, lo:hi], uv)
            out.append(f * pe if pe is not None else f)
        return torch.cat(out, -1)

    def _mlp(self, h, prefix):
        for i in (0, 2, 4):
            h = F.linear(h, self.p[f"{prefix}.mlp.{i}.weight"], self.p[f"{prefix}.mlp.{i}.bias"])
            if i < 4:
                h = torch.relu(h)
        return h

    def forward(self, rays, S, jitter, white_bg, infoinv):
        """-> rgb_map [n,3] and a dict of the per-sample facts: "valid", "active" and "weight" [n,S], "u" (the softplus arguments o - 10 of the
        valid samples), "face" (per ray, the smallest distance of a sample to a box face) and "cell" (per ray, the smallest distance of a
        box-valid sample's mask coordinate to a cell boundary, in cells; inf without a mask)."""
        dt, dev = self.dtype, self.device
        n = rays.shape[0]
        o, d = rays[:, :3], rays[:, 3:6]
        vec = torch.where(d == 0, torch.full_like(d, 1e-6), d)
        tmin = torch.minimum((self.aabb[1] - o) / vec, (self.aabb[0] - o) / vec).amax(-1).clamp(min=self.near, max=self.far)
        rng = torch.arange(S, dtype=dt, device=dev)[None].repeat(n, 1) + jitter.reshape(-1, 1)
        z = tmin[:, None] + self.step * rng
        pts = o[:, None, :] + d[:, None, :] * z[..., None]
        valid = ~((self.aabb[0] > pts) | (pts > self.aabb[1])).any(-1)
        face = torch.minimum((pts - self.aabb[0]).abs(), (pts - self.aabb[1]).abs()).amin(dim=(-1, -2))
        dists = torch.cat((z[:, 1:] - z[:, :-1], torch.zeros_like(z[:, :1])), -1)
        cell = torch.full((n,), float("inf"), dtype=dt, device=dev)
        if self.mask is not None:
            vol, maabb, minv = self.mask
            q = (pts[valid] - maabb[0]) * minv - 1
            a = F.grid_sample(vol, q.reshape(1, -1, 1, 1, 3), align_corners=True).reshape(-1)
            ix = (q + 1) / 2 * torch.tensor([vol.shape[-1] - 1, vol.shape[-2] - 1, vol.shape[-3] - 1], dtype=dt, device=dev)
            near_cell = torch.full((n, S), float("inf"), dtype=dt, device=dev)
            near_cell[valid] = (ix - torch.round(ix)).abs().amin(-1)
            cell = near_cell.amin(-1)
            bad = ~valid
            bad[valid] |= ~(a > 0)
            valid = ~bad
        sigma = torch.zeros((n, S), dtype=dt, device=dev)
        coords = [torch.zeros((n, S, 2), dtype=dt, device=dev) for _ in range(3)]
        u = torch.zeros((0,), dtype=dt, device=dev)
        if valid.any():
            x = ((pts - self.aabb[0]) * self.inv - 1)[valid]
            c = (x[:, :2], x[:, 1:], x[:, ::2])
            pe = posenc(torch.cat([c[0], c[1][:, 1:]], -1), 4) if infoinv else None
            u = self._mlp(self._feats(c, 0, DD, pe), "density_decoder").reshape(-1) - 10
            sigma = sigma.masked_scatter(valid, F.softplus(u))
            coords = [ck.masked_scatter(valid[..., None].expand(n, S, 2), cv) for ck, cv in zip(coords, c)]
        alpha = 1.0 - torch.exp(-sigma * (dists * self.dscale))
        T = torch.cumprod(torch.cat([torch.ones((n, 1), dtype=dt, device=dev), 1.0 - alpha + 1e-10], -1), -1)
        w = alpha * T[:, :-1]
        act = w > self.thr
        rgb = torch.zeros((n, S, 3), dtype=dt, device=dev)
        if act.any():
            c = [ck[act] for ck in coords]
            dirs = d[:, None, :].expand(n, S, 3)[act]
            pe = posenc(torch.cat([c[0], c[1][:, 1:]], -1), 12) if infoinv else None
            f = self._feats(c, DD, self.p["plane_xy"].shape[1], pe)
            h = torch.cat([F.linear(f, self.p["rgb_decoder.basis.weight"]), dirs, posenc(dirs, 2)], -1)
            rgb = rgb.masked_scatter(act[..., None].expand(n, S, 3), torch.sigmoid(self._mlp(h, "rgb_decoder")))
        acc = w.sum(-1)
        rgb_map = (w[..., None] * rgb).sum(-2)
        if white_bg:
            rgb_map = rgb_map + (1.0 - acc[..., None])
        return rgb_map.clamp(0, 1), {"valid": valid, "active": act, "weight": w.detach(), "u": u.detach(), "face": face, "cell": cell}

    def gradients(self, rays, rgb_train, S, jitter, white_bg, infoinv):
        """mean((rgb_map - rgb_train)^2) and its gradients (a tensor the loss does not reach: zeros, as the HIP trainers return them)
        -> (rgb_map, loss, {name: gradient}, facts)"""
        for v in self.p.values():
            v.grad = None
        rgb_map, aux = self.forward(rays, S, jitter, white_bg, infoinv)
        loss = torch.mean((rgb_map - rgb_train) ** 2)
        if loss.requires_grad:
            loss.backward()
        grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad.detach().clone()) for k, v in self.p.items()}
        return rgb_map.detach(), float(loss.detach()), grads, aux


# ---- the toy scene of tests/golden/infoinv_train_*.npz and batches at the edges ---------------------------------------------------------------
EDGE_SEEDS = (411, 412, 413)          # every case runs on three seeds (model and batch)
FACE_MARGIN = 1e-5                    # a pool ray is used only if each of its samples stays this far from every box face, ...
WEIGHT_MARGIN = 0.02                  # ... each weight this far from rayMarch_weight_thres, relative to it (1 - exp(-x) at a weight of 1e-4 is
                                      # 3e-4 relative in fp32: the margin is sixty times that), ...
CELL_MARGIN = 1e-4                    # ... and, under a mask, each mask coordinate this far (in cells) from a cell boundary: the eight corner
                                      # weights are then positive in fp32 and fp64 alike, and the sign of the trilinear sum is the corners'
POOL_STRIDE = 157                     # every 157th ray of the 800 x 800 frame (4077 rays), plus 512 of synth.edge_rays
DARK_U = -16.0                        # "dark": the largest softplus argument after the density bias is lowered (model_params)


@functools.lru_cache(maxsize=None)
def toy():
    """The geometry of the toy fixtures (12 x 10 x 9 grid) and the alpha mask of the first -> (g, plane_hw, mask)"""
    g = dict(np.load(os.path.join(GOLDEN, "infoinv_train_on_white.npz"), allow_pickle=False))
    g = {k: g[k] for k in ("model", "aabb", "grid", "near_far", "distance_scale", "thr", "mask_bits", "mask_dhw", "mask_aabb")}
    g["step_ratio"] = np.float32(0.5)
    plane_hw = ((10, 12), (9, 10), (9, 12))
    return g, plane_hw, (g["mask_bits"], tuple(int(v) for v in g["mask_dhw"]), g["mask_aabb"])


def model_params(seed, variant="base", plane_hw=None):
    """variant "dark": the density bias lowered until the largest softplus argument of the seed's pool (PE modulation on or off, S = 24) is
    DARK_U: sigma <= 1.2e-7 and alpha <= 5e-7 there, so no weight comes near the threshold of 1e-4 -- no active sample, yet a density whose
    gradient is not zero"""
    p = dict(synth.infoinv_params(seed, plane_hw or toy()[1], preset="R1"))
    if variant == "dark":
        top = max(float(_pool(seed, 24, inf, False, "base")[2]["u"].max()) for inf in (True, False))
        p["density_decoder.mlp.4.bias"] = (p["density_decoder.mlp.4.bias"].astype(np.float64) + (DARK_U - top)).astype(np.float32)
    return p


def pool_rays(seed):
    """camera rays of the lookat frame, and synth.edge_rays: rays that start inside the box, axis-aligned rays with zero direction
    components, rays that point away from it"""
    frame = synth.lookat_rays(800, 800)[seed % POOL_STRIDE::POOL_STRIDE]
    return np.ascontiguousarray(np.concatenate([frame, synth.edge_rays(seed, 512)], 0), np.float32)


def facts(params, g, mask, rays, jitter, S, infoinv, dtype=torch.float64):
    """per ray: valid count, active count, the margins of the three kinds, and the softplus arguments (one eager forward on the host)"""
    e = Eager(params, g, dtype, "cpu", mask)
    with torch.no_grad():
        _, aux = e.forward(torch.from_numpy(rays).to(dtype), S, torch.from_numpy(jitter).to(dtype), True, infoinv)
    wm = (aux["weight"].double() / e.thr - 1.0).abs().amin(-1)
    return {"valid": aux["valid"].sum(-1).numpy().astype(np.int64), "active": aux["active"].sum(-1).numpy().astype(np.int64),
            "valid_set": aux["valid"].numpy(), "active_set": aux["active"].numpy(),
            "face": aux["face"].double().numpy(), "weight": wm.numpy(), "cell": aux["cell"].double().numpy(), "u": aux["u"].double().numpy()}


@functools.lru_cache(maxsize=64)
def _pool(seed, S, infoinv, masked, variant):
    g, _, mask = toy()
    rays = pool_rays(seed)
    jitter = synth.hash_uniform(seed, 701, (rays.shape[0],))
    f = facts(model_params(seed, variant), g, mask if masked else None, rays, jitter, S, infoinv)
    ok = (f["face"] >= FACE_MARGIN) & (f["weight"] >= WEIGHT_MARGIN) & (f["cell"] >= CELL_MARGIN)
    order = np.argsort(synth.hash_uniform(seed, 702, (rays.shape[0],)), kind="stable")
    return rays, jitter, f, order[ok[order]]


def _subset(counts, order, target):
    """rays of `order` whose counts add up to exactly `target` (a subset sum over small integers: reach[t] = the ray that first made t, from a
    sum that was reachable before that ray's turn -- so the chain back from `target` names every ray once)"""
    reach = np.full(target + 1, -2, np.int64)
    reach[0] = -1
    for j in order:
        c = int(counts[j])
        if c <= 0 or c > target:
            continue
        new = (reach[:target + 1 - c] != -2) & (reach[c:] == -2)          # both sides read before the write below
        reach[c:][new] = j
        if reach[target] != -2:
            break
    assert reach[target] != -2, "the pool cannot reach this count"
    pick, t = [], target
    while t > 0:
        j = int(reach[t])
        pick.append(j)
        t -= int(counts[j])
    assert len(set(pick)) == len(pick)
    return pick[::-1]


def edge_batch(seed, S, infoinv=True, masked=False, variant="base", active=None, R=None, no_valid=False, extra=3):
    """A batch of pool rays in a seeded order.  active: rays whose fp64 active counts add up to exactly that many (0: none of them has an
    active sample), then `extra` rays without a valid sample.  R: the first R usable rays whatever their counts.  no_valid: R rays
    without one valid sample.  -> rays [n,6], jitter [n], rgb_train [n,3] (float32), "valid" and "active" (the fp64 counts per ray),
    "margin" (the smallest face, weight and cell margin of the batch) and the "params" of the seed and variant."""
    rays, jitter, f, order = _pool(seed, S, bool(infoinv), bool(masked), variant)
    miss = [j for j in order if f["valid"][j] == 0]
    if no_valid:
        pick = miss[:R]
    elif active is not None:
        if active == 0:
            pick = [j for j in order if f["active"][j] == 0 and f["valid"][j] > 0][:R or 37]
        else:
            pick = _subset(f["active"], order, int(active))
        pick = list(pick) + miss[:extra]
    else:
        pick = list(order[:R])
    pick = np.asarray(pick, np.int64)
    n = len(pick)
    assert n > 0 and (active is not None or n == R), "the pool holds too few such rays"
    return {"rays": rays[pick], "jitter": jitter[pick], "rgb_train": synth.hash_uniform(seed, 703, (n, 3)),
            "valid": f["valid"][pick], "active": f["active"][pick],
            "margin": (float(f["face"][pick].min()), float(f["weight"][pick].min()), float(f["cell"][pick].min())),
            "params": model_params(seed, variant), "S": S, "infoinv": bool(infoinv), "masked": bool(masked)}


EDGE_S = 24
EDGE_ACTIVE = (1, 31, 32, 33, 1025)          # around the 32-row k-step and the 1024-row fp32-to-fp64 hand-over of the colour products
# (rays, samples): one ray; a ragged 256-thread ray block; two and three rays per ii_prefix_kernel thread (1024 threads); a short second
# chunk of ii_xty_kernel (171 x 24 = 4104 pairs) and of ii_mm_kernel (342 x 24 = 8208 pairs)
EDGE_RAYS = ((1, 7), (37, 45), (257, EDGE_S), (1025, EDGE_S), (2051, EDGE_S), (171, EDGE_S), (342, EDGE_S))


def edge_cases():
    """{id: (edge_batch keywords, white background)}: every batch of tests/test_gpu_infoinv_train_edges.py that is held to the fp64
    criterion (tests/test_infoinv_train_edges_cpu.py builds each of them on the CPU and checks its counts and margins)"""
    c = {}
    for white in (True, False):
        bg = "white" if white else "black"
        c[f"active0-{bg}"] = (dict(S=EDGE_S, variant="dark", active=0, R=37), white)
        c[f"novalid-{bg}"] = (dict(S=EDGE_S, no_valid=True, R=37), white)
    for i, a in enumerate(EDGE_ACTIVE):
        c[f"active{a}"] = (dict(S=EDGE_S, active=a, infoinv=i % 2 == 0), True)
    for i, (R, S) in enumerate(EDGE_RAYS):
        c[f"rays{R}x{S}"] = (dict(S=S, R=R, infoinv=i % 2 == 0), i % 3 != 2)
    c["mask-off-white"] = (dict(S=EDGE_S, R=128, masked=True, infoinv=False), True)
    c["mask-on-black"] = (dict(S=EDGE_S, R=128, masked=True, infoinv=True), False)
    c["chunks"] = (dict(S=EDGE_S, R=128), True)
    return c


SOFTPLUS_DSCALE = 0.15         # distance_scale of the softplus case: sigma is about 20 there, and 20 x 0.1635 x 0.15 keeps alpha near 0.4
SOFTPLUS_SPREAD = 5.0           # standard deviation of the arguments after the density head is scaled


def softplus_case(seed, S=24, R=64, infoinv=True):
    """The density head scaled and shifted so that the arguments o - 10 of softplus lie on both sides of ATen's threshold of 20 (20 falls into
    the widest gap between neighbouring arguments from the 40th to the 60th percentile), and distance_scale lowered to SOFTPLUS_DSCALE so
    that alpha stays away from 0 and 1.  -> (params, geometry, batch, stats); stats: "above" (the share of the valid samples' arguments above
    20), "gap" (the smallest |u - 20|: fp32 and fp64 must take the same branch), "alpha" (the range of alpha over the valid samples)."""
    g0, _, _ = toy()
    g = dict(g0, distance_scale=np.float32(SOFTPLUS_DSCALE))
    rays, jitter, f0, order = _pool(seed, S, bool(infoinv), False, "base")
    pick = np.asarray([j for j in order if f0["valid"][j] >= S // 4][:R], np.int64)
    params = model_params(seed)
    u = facts(params, g, None, rays[pick], jitter[pick], S, infoinv)["u"]
    o = np.sort(u + 10.0)
    mid = o[int(0.4 * o.size):int(0.6 * o.size) + 1]
    i = int(np.argmax(np.diff(mid)))
    split = 0.5 * float(mid[i] + mid[i + 1])
    a = SOFTPLUS_SPREAD / float(o.std())
    w3, b3 = "density_decoder.mlp.4.weight", "density_decoder.mlp.4.bias"
    params[w3] = (params[w3].astype(np.float64) * a).astype(np.float32)
    params[b3] = (params[b3].astype(np.float64) * a + (30.0 - a * split)).astype(np.float32)
    f = facts(params, g, None, rays[pick], jitter[pick], S, infoinv)
    pick = pick[f["weight"] >= WEIGHT_MARGIN]          # the weights moved with the head: the margin is taken again (rays are independent)
    f = facts(params, g, None, rays[pick], jitter[pick], S, infoinv)
    step =float(geometry.step_size(g["aabb"], g["grid"], 0.5))
    alpha = 1.0 - np.exp(-np.logaddexp(0.0, f["u"]) * step * SOFTPLUS_DSCALE)
    n = len(pick)
    b = {"rays": rays[pick], "jitter": jitter[pick], "rgb_train": synth.hash_uniform(seed, 703, (n, 3)), "valid": f["valid"], "active": f["active"],
         "margin": (float(f["face"].min()), float(f["weight"].min()), float(f["cell"].min())), "params": params, "S": S,
         "infoinv": bool(infoinv), "masked": False}
    stats = {"above": float((f["u"] > 20).mean()), "gap": float(np.abs(f["u"] - 20).min()), "alpha": (float(alpha.min()), float(alpha.max())),
             "valid": int(f["valid"].sum()), "active": int(f["active"].sum())}
    return params, g, b, stats
