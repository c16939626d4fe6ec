"""Torch restatement of the TriPlane training-mode forward for any dtype and device, written from this project's own port (oracle/eager.py,
oracle/train.py::EagerTrainer.forward_train): sample_ray with pinned jitter, the box test and the alpha mask, compute_gauge in the port's add
order, zeros-padded grid_sample, softplus(x - 10) and raw2alpha with its 1e-10, the active set, the colour MLP through ``basis``, compositing,
the white background and the clamp.  The GPU tests run it in float64 (the truth) and float32 (the yardstick) next to the HIP trainers; the port
itself is float32 on the host only.

``edge_batch`` builds batches on which float32 and float64 take every discrete decision alike (the margins below) and can hit an exact active
count; ``check`` is the criterion both tests/test_gpu_triplane_train_edges.py and tests/test_triplane_train_edges_cpu.py apply.

The clamp of rgb_map: a pixel is sum w rgb (+ 1 - sum w on white) with 0 <= rgb <= 1 (a sigmoid) and sum w <= 1 + S 1e-10 (raw2alpha), so
it lies in [0, 1] up to rounding whatever the parameters are: the clamp never cuts a pixel by more than a few ulps and no batch can have a
clamped pixel 1e-5 away from the bound.  The "bright" variant therefore saturates the sigmoid (pixels close to 1 on white) without a clamped
pixel; tests/test_triplane_train_edges_cpu.py asserts the range over every pool."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from ngf_amd import geometry, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PLANES = ("plane_xy", "plane_yz", "plane_xz")
GAUGES = ("gauge_xy", "gauge_yz", "gauge_xz")
PARAM_NAMES = PLANES + GAUGES + ("density_decoder.weight", "density_decoder.bias", "rgb_decoder.basis.weight", "rgb_decoder.mlp.0.weight",
                                 "rgb_decoder.mlp.0.bias", "rgb_decoder.mlp.2.weight", "rgb_decoder.mlp.2.bias", "rgb_decoder.mlp.4.weight",
                                 "rgb_decoder.mlp.4.bias")
COLOUR = PARAM_NAMES[8:]           # what only an active sample reaches (the planes' colour channels and the gauge planes see it as well)
DD = 16                            # density channels per plane


def posenc(x, freqs):
    bands = 2.0 ** torch.arange(freqs, dtype=x.dtype, device=x.device)
    y = (x[..., None] * bands).reshape(*x.shape[:-1], -1)
    return torch.cat([torch.sin(y), torch.cos(y)], -1)


def sample2d(plane, uv):
    """[1,C,H,W] sampled at uv [M,2] -> [M,C] (bilinear, zeros padding, align_corners=True)."""
    return F.grid_sample(plane, uv.reshape(1, -1, 1, 2), align_corners=True).reshape(plane.shape[1], -1).T


def texel_coords(plane, uv):
    """uv [M,2] in texels of [1,C,H,W] (align_corners=True: -1 is texel 0, +1 is texel W - 1 / H - 1)"""
    size = torch.tensor([plane.shape[3] - 1, plane.shape[2] - 1], dtype=uv.dtype, device=uv.device)
    return (uv + 1) / 2 * size


class Eager:
    """The field of a geometry dict ``g`` (aabb, grid, near_far, distance_scale, thr, step_ratio: a fixture's keys) with differentiable
    parameters of ``dtype``.  mask: (np.packbits image, (D, H, W), aabb [2,3]) or None.  The gauge is on from iteration ``gauge_start``."""

    def __init__(self, params, g, dtype=torch.float32, device="cpu", mask=None, gauge_start=0):
        t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(device=device, dtype=dtype)          # noqa: E731
        self.dtype, self.device = dtype, device
        self.p = {k: t(params[k]).requires_grad_(True) for k in PARAM_NAMES}
        self.aabb = t(g["aabb"]).reshape(2, 3)
        self.inv = 2.0 / (self.aabb[1] - self.aabb[0])
        self.step = t(g["stepSize"] if "stepSize" in g else geometry.step_size(g["aabb"], g["grid"], float(g["step_ratio"])))
        self.near, self.far = float(g["near_far"][0]), float(g["near_far"][1])
        self.dscale, self.thr = float(g["distance_scale"]), float(np.float32(g["thr"]))
        self.gauge_start = gauge_start
        self.mask = None
        if mask is not None:
            bits, dhw, maabb = mask
            vol = np.unpackbits(np.asarray(bits))[:int(np.prod(dhw))].reshape(tuple(int(v) for v in dhw)).astype(np.float32)
            maabb = t(maabb).reshape(2, 3)
            self.mask = (t(vol)[None, None], maabb, 1.0 / (maabb[1] - maabb[0]) * 2)

    def _coords(self, x, gauge_on):
        """compute_gauge: each plane's own shift first, then the two it shares an axis with"""
        xy, yz, xz = x[:, :2], x[:, 1:], x[:, ::2]
        if not gauge_on:
            return xy, yz, xz
        dxy, dyz, dxz = sample2d(self.p["gauge_xy"], xy), sample2d(self.p["gauge_yz"], yz), sample2d(self.p["gauge_xz"], xz)
        txy, tyz, txz = xy + dxy, yz + dyz, xz + dxz
        txy = torch.stack([txy[:, 0] + dxz[:, 0], txy[:, 1] + dyz[:, 0]], -1)
        tyz = torch.stack([tyz[:, 0] + dxy[:, 1], tyz[:, 1] + dxz[:, 1]], -1)
        txz = torch.stack([txz[:, 0] + dxy[:, 0], txz[:, 1] + dyz[:, 1]], -1)
        return txy, tyz, txz

    def _feats(self, c, lo, hi):
        return torch.cat([sample2d(self.p[name][:, lo:hi], uv) for name, uv in zip(PLANES, c)], -1)

    def forward(self, rays, S, jitter, white_bg, iteration=0):
        """-> rgb_map [n,3] and a dict of the per-sample facts: "valid", "active" and "weight" [n,S]; "coords": the three shifted coordinate sets
        of the valid samples; "u": their softplus arguments; "h1", "h2": the hidden pre-activations of the active samples; "pre": the pixels
        before the clamp; "rgb_act": the colour of the active samples (in the graph); and per ray the margins "face", "cell", "texel", "kink"
        and "pixel" (white and black), inf where a ray has nothing of the kind."""
        dt, dev = self.dtype, self.device
        n = rays.shape[0]
        inf = float("inf")
        o, d = rays[:, :3], rays[:, 3:6]
        vec = torch.where(d == 0, torch.full_like(d, 1e-6), d)
        tmin = torch.minimum((self.aabb[1] - o) / vec, (self.aabb[0] - o) / vec).amax(-1).clamp(min=self.near, max=self.far)
        rng = torch.arange(S, dtype=dt, device=dev)[None].repeat(n, 1) + jitter.reshape(-1, 1)
        z = tmin[:, None] + self.step * rng
        pts = o[:, None, :] + d[:, None, :] * z[..., None]
        valid = ~((self.aabb[0] > pts) | (pts > self.aabb[1])).any(-1)
        face = torch.minimum((pts - self.aabb[0]).abs(), (pts - self.aabb[1]).abs()).amin(dim=(-1, -2))
        dists = torch.cat((z[:, 1:] - z[:, :-1], torch.zeros_like(z[:, :1])), -1)
        cell = torch.full((n,), inf, dtype=dt, device=dev)
        if self.mask is not None:
            vol, maabb, minv = self.mask
            q = (pts[valid] - maabb[0]) * minv - 1
            a = F.grid_sample(vol, q.reshape(1, -1, 1, 1, 3), align_corners=True).reshape(-1)
            ix = (q + 1) / 2 * torch.tensor([vol.shape[-1] - 1, vol.shape[-2] - 1, vol.shape[-3] - 1], dtype=dt, device=dev)
            near_cell = torch.full((n, S), inf, dtype=dt, device=dev)
            near_cell[valid] = (ix - torch.round(ix)).abs().amin(-1)
            cell = near_cell.amin(-1)
            bad = ~valid
            bad[valid] |= ~(a > 0)
            valid = ~bad
        sigma = torch.zeros((n, S), dtype=dt, device=dev)
        coords = [torch.zeros((n, S, 2), dtype=dt, device=dev) for _ in range(3)]
        u = torch.zeros((0,), dtype=dt, device=dev)
        c_valid = [torch.zeros((0, 2), dtype=dt, device=dev)] * 3
        texel = torch.full((n,), inf, dtype=dt, device=dev)
        gauge_on = iteration >= self.gauge_start
        if valid.any():
            x = (pts - self.aabb[0]) * self.inv - 1
            c = self._coords(x[valid], gauge_on)
            u = F.linear(self._feats(c, 0, DD), self.p["density_decoder.weight"], self.p["density_decoder.bias"]).reshape(-1) - 10
            sigma = sigma.masked_scatter(valid, F.softplus(u))
            coords = [ck.masked_scatter(valid[..., None].expand(n, S, 2), cv) for ck, cv in zip(coords, c)]
            c_valid = [cv.detach() for cv in c]
            near = torch.full((n, S), inf, dtype=dt, device=dev)
            tx = torch.cat([texel_coords(self.p[name], cv) for name, cv in zip(PLANES, c_valid)], -1)
            near[valid] = (tx - torch.round(tx)).abs().amin(-1)
            texel = near.amin(-1)
        alpha = 1.0 - torch.exp(-sigma * (dists * self.dscale))
        T = torch.cumprod(torch.cat([torch.ones((n, 1), dtype=dt, device=dev), 1.0 - alpha + 1e-10], -1), -1)
        w = alpha * T[:, :-1]
        act = w > self.thr
        rgb = torch.zeros((n, S, 3), dtype=dt, device=dev)
        h1 = h2 = torch.zeros((0, 64), dtype=dt, device=dev)
        rgb_act = None
        kink = torch.full((n,), inf, dtype=dt, device=dev)
        if act.any():
            c = [ck[act] for ck in coords]
            dirs = d[:, None, :].expand(n, S, 3)[act]
            f = self._feats(c, DD, self.p["plane_xy"].shape[1])
            h = torch.cat([F.linear(f, self.p["rgb_decoder.basis.weight"]), dirs, posenc(dirs, 2)], -1)
            h1 = F.linear(h, self.p["rgb_decoder.mlp.0.weight"], self.p["rgb_decoder.mlp.0.bias"])
            h2 = F.linear(torch.relu(h1), self.p["rgb_decoder.mlp.2.weight"], self.p["rgb_decoder.mlp.2.bias"])
            rgb_act = torch.sigmoid(F.linear(torch.relu(h2), self.p["rgb_decoder.mlp.4.weight"], self.p["rgb_decoder.mlp.4.bias"]))
            rgb = rgb.masked_scatter(act[..., None].expand(n, S, 3), rgb_act)
            near = torch.full((n, S), inf, dtype=dt, device=dev)
            near[act] = torch.minimum(h1.detach().abs().amin(-1), h2.detach().abs().amin(-1))
            kink = near.amin(-1)
        acc = w.sum(-1)
        black = (w[..., None] * rgb).sum(-2)
        pre = black + (1.0 - acc[..., None]) if white_bg else black
        with torch.no_grad():
            white = black + (1.0 - acc[..., None])
            pixel = torch.stack([white.abs(), (white - 1).abs(), black.abs(), (black - 1).abs()]).amin(dim=(0, -1))
            pixel = torch.where(act.any(-1), pixel, torch.full_like(pixel, inf))     # without an active sample: background minus the weights
        aux = {"valid": valid, "active": act, "weight": w.detach(), "u": u.detach(), "coords": c_valid, "h1": h1.detach(), "h2": h2.detach(),
               "pre": pre.detach(), "rgb_act": rgb_act, "face": face, "cell": cell, "texel": texel, "kink": kink, "pixel": pixel,
               "range": (float(torch.minimum(black.detach().amin(), white.detach().amin())),
                         float(torch.maximum(black.detach().amax(), white.detach().amax())))}
        return pre.clamp(0, 1), aux

    def gradients(self, rays, rgb_train, S, jitter, white_bg, iteration=0, keep_graph=False):
        """mean((rgb_map - rgb_train)^2) and its gradients (a tensor the loss does not reach: zeros, as the HIP trainers return them)
        -> (rgb_map, loss, {name: gradient}, facts).  keep_graph: "loss" of the facts is the loss in its graph (``row_share``)."""
        for v in self.p.values():
            v.grad = None
        rgb_map, aux = self.forward(rays, S, jitter, white_bg, iteration)
        loss = torch.mean((rgb_map - rgb_train) ** 2)
        if loss.requires_grad:
            loss.backward(retain_graph=keep_graph)
        grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad.detach().clone()) for k, v in self.p.items()}
        if keep_graph:
            aux["loss"] = loss
        else:
            aux["rgb_act"] = None
        return rgb_map.detach(), float(loss.detach()), grads, aux

    def row_share(self, aux, row, names):
        """what active sample ``row`` adds to the gradients of ``names`` through its colour alone (after gradients(keep_graph=True))"""
        G = torch.autograd.grad(aux["loss"], aux["rgb_act"], retain_graph=True)[0]
        out = torch.autograd.grad(aux["rgb_act"][row], [self.p[k] for k in names], grad_outputs=G[row], retain_graph=True, allow_unused=True)
        return {k: (torch.zeros_like(self.p[k]) if v is None else v) for k, v in zip(names, out)}


# ---- the toy scene of tests/golden/triplane_r1_gauge.npz and batches at the edges -------------------------------------------------------------
EDGE_SEEDS = (511, 512, 513)          # every case runs on three seeds (model and batch)
FACE_MARGIN = 1e-5                    # a pool ray is used only if each of its samples stays this far from every box face, ...
WEIGHT_MARGIN = 0.02                  # ... each weight this far from rayMarch_weight_thres, relative to it, ...
TEXEL_MARGIN = 1e-4                   # ... each shifted coordinate this far (in texels) from a texel line of the plane it is sampled from: the
                                      # gradient with respect to the coordinate, which the gauge planes receive, jumps there, ...
CELL_MARGIN = 1e-4                    # ... under a mask, each mask coordinate this far (in cells) from a cell boundary, ...
KINK_MARGIN = 1e-5                    # ... each hidden pre-activation of an active sample this far from zero (the ReLU's kink: the comment of
                                      # test_full_size_batch_matches_autograd_oracle, tests/test_gpu_train.py), ...
PIXEL_MARGIN = 1e-5                   # ... each pixel before the clamp this far from 0 and 1, on white and on black, ...
SOFTPLUS_MARGIN = 1e-4                # ... and each softplus argument this far from ATen's threshold of 20
MARGINS = {"face": FACE_MARGIN, "weight": WEIGHT_MARGIN, "texel": TEXEL_MARGIN, "cell": CELL_MARGIN, "kink": KINK_MARGIN,
           "pixel": PIXEL_MARGIN, "soft": SOFTPLUS_MARGIN}
POOL_STRIDE = 157                     # every 157th ray of the 800 x 800 frame (4077 rays), plus 512 of synth.edge_rays
DARK_U = -16.0                        # "dark": the largest softplus argument after the density bias is lowered
FOG_SCALE, FOG_BIAS = 0.25, 7.0       # "fog": softplus arguments of about -3 +- 0.7: alpha of about 0.09 per step, so a ray keeps its
                                      # transmittance and nearly every sample inside the box is active
FAR_GAUGE = 6.0                       # "far_gauge": the gauge planes (std 0.05) times this: shifts of about 0.4 per axis
BRIGHT_B3 = 4.0                       # "bright": added to the last colour bias: sigmoid arguments of about 4, pixels of about 0.98 on white
SOFTPLUS_DSCALE = 0.3                 # distance_scale of "softplus": sigma is about 20 there, and 20 x 0.0775 x 0.3 keeps alpha near 0.4
SOFTPLUS_SPREAD = 5.0                 # standard deviation of its arguments after the density head is scaled
DUP_LAST_W = 0.05                     # the repeated ray's last active sample weighs this much or more (``_heavy_last``)
VARIANTS = ("base", "fog", "far_gauge", "bright", "softplus", "dark")
GAUGE_STD = 0.05


@functools.lru_cache(maxsize=None)
def toy():
    """The geometry of the triplane_r1_gauge fixture (24 x 20 x 18 grid) and the alpha mask of triplane_r1_mask (10 x 12 x 14 cells, the same
    grid) -> (g, plane_hw, gauge_hw, mask)"""
    g = dict(np.load(os.path.join(GOLDEN, "triplane_r1_gauge.npz"), allow_pickle=False))
    m = dict(np.load(os.path.join(GOLDEN, "triplane_r1_mask.npz"), allow_pickle=False))
    plane_hw = tuple(tuple(int(v) for v in hw) for hw in g["plane_hw"])
    gauge_hw = tuple(int(v) for v in g["gauge_hw"])
    g = {k: g[k] for k in ("model", "aabb", "grid", "near_far", "distance_scale", "thr", "step_ratio")}
    return g, plane_hw, gauge_hw, (m["mask_bits"], tuple(int(v) for v in m["mask_dhw"]), m["mask_aabb"])


def geometry_of(variant, g=None):
    g = g or toy()[0]
    return dict(g, distance_scale=np.float32(SOFTPLUS_DSCALE)) if variant == "softplus" else g


@functools.lru_cache(maxsize=None)
def _variant_numbers(seed, variant):
    """the two numbers a variant takes from the seed's base pool (S = 24, gauge on): "dark": the largest softplus argument; "softplus": the
    scale of the density head and its new bias"""
    u = _pool(seed, 24, False, "base", True)[2]["u"]
    if variant == "dark":
        return float(u.max()), 0.0
    o = np.sort(u + 10.0)
    mid = o[int(0.4 * o.size):int(0.6 * o.size) + 1]
    i = int(np.argmax(np.diff(mid)))
    split = 0.5 * float(mid[i] + mid[i + 1])
    a = SOFTPLUS_SPREAD / float(o.std())
    return a, 30.0 - a * split


def model_params(seed, variant="base", plane_hw=None, gauge_hw=None):
    """synth.triplane_params of the seed on the toy's planes (or the given sizes), and one change per variant (the constants above)"""
    assert variant in VARIANTS
    _, hw, ghw, _ = toy()
    p = dict(synth.triplane_params(seed, plane_hw or hw, gauge_hw or ghw, preset="R1", gauge_std=GAUGE_STD))
    wd, bd, b3 = "density_decoder.weight", "density_decoder.bias", "rgb_decoder.mlp.4.bias"
    f64 = lambda a: np.asarray(a, np.float64)          # noqa: E731
    if variant == "dark":
        p[bd] = (f64(p[bd]) + (DARK_U - _variant_numbers(seed, "dark")[0])).astype(np.float32)
    elif variant == "fog":
        p[wd] = (f64(p[wd]) * FOG_SCALE).astype(np.float32)
        p[bd] = np.full((1,), FOG_BIAS, np.float32)
    elif variant == "far_gauge":
        for k in GAUGES:
            p[k] = (f64(p[k]) * FAR_GAUGE).astype(np.float32)
    elif variant == "bright":
        p[b3] = (f64(p[b3]) + BRIGHT_B3).astype(np.float32)
    elif variant == "softplus":
        a, b = _variant_numbers(seed, "softplus")
        p[wd] = (f64(p[wd]) * a).astype(np.float32)
        p[bd] = (f64(p[bd]) * a + b).astype(np.float32)
    return p


def pool_rays(seed):
    """camera rays of the lookat frame, and synth.edge_rays: rays that start inside the box, axis-aligned rays with zero direction
    components, rays that point away from it"""
    frame = synth.lookat_rays(800, 800)[seed % POOL_STRIDE::POOL_STRIDE]
    return np.ascontiguousarray(np.concatenate([frame, synth.edge_rays(seed, 512)], 0), np.float32)


def colour_bins(coords, active_in_valid, plane_hw):
    """[A, 3]: per active sample and plane, the 8 x 8-cell bin of the padded plane its shifted coordinate falls into (row * 1024 + column), -1
    where all four taps are outside.  Also the per-pair tap facts of the valid samples: (one or more taps outside, all four outside)."""
    bins, some, none = [], [], []
    for cv, (H, W) in zip(coords, plane_hw):
        ix, iy = (cv[:, 0] + 1) / 2 * (W - 1), (cv[:, 1] + 1) / 2 * (H - 1)
        fx, fy = np.floor(ix), np.floor(iy)
        inside = (fx >= -1) & (fx <= W - 1) & (fy >= -1) & (fy <= H - 1)          # the cell touches the plane: one tap or more is a texel
        whole = (fx >= 0) & (fx <= W - 2) & (fy >= 0) & (fy <= H - 2)
        cx, cy = np.clip(fx, -1, W - 1).astype(np.int64) + 1, np.clip(fy, -1, H - 1).astype(np.int64) + 1
        b = np.where(inside, (cy >> 3) * 1024 + (cx >> 3), -1)
        bins.append(b[active_in_valid])
        some.append(~whole)
        none.append(~inside)
    return np.stack(bins, -1), np.stack(some, -1), np.stack(none, -1)


def facts(params, g, mask, rays, jitter, S, gauge_on=True, dtype=torch.float64):
    """per ray: the valid and active counts and every margin; per valid sample: the softplus arguments and the tap facts; per active sample:
    its colour bins (one eager forward on the host)"""
    e = Eager(params, g, dtype, "cpu", mask, gauge_start=0 if gauge_on else 1)
    with torch.no_grad():
        _, aux = e.forward(torch.from_numpy(rays).to(dtype), S, torch.from_numpy(jitter).to(dtype), True, 0)
    n = rays.shape[0]
    valid, act = aux["valid"].numpy(), aux["active"].numpy()
    wm = (aux["weight"].double() / e.thr - 1.0).abs().amin(-1)
    u = aux["u"].double().numpy()
    soft = np.full((n, S), np.inf)
    soft[valid] = np.abs(u - 20.0)
    hw = [tuple(e.p[k].shape[2:]) for k in PLANES]
    bins, some, none = colour_bins([c.double().numpy() for c in aux["coords"]], act[valid], hw)
    ray_of_active = np.nonzero(act)[0]
    w = aux["weight"].double().numpy()
    last = np.where(act.any(-1), S - 1 - np.argmax(act[:, ::-1], -1), 0)
    last_w = np.where(act.any(-1), w[np.arange(n), last], 0.0)
    return {"valid": valid.sum(-1).astype(np.int64), "active": act.sum(-1).astype(np.int64), "valid_set": valid, "active_set": act,
            "face": aux["face"].double().numpy(), "weight": wm.numpy(), "cell": aux["cell"].double().numpy(),
            "texel": aux["texel"].double().numpy(), "kink": aux["kink"].double().numpy(), "pixel": aux["pixel"].double().numpy(),
            "soft": soft.min(-1), "u": u, "last_w": last_w, "bins": bins, "ray_of_active": ray_of_active, "taps_some": some, "taps_none": none,
            "ray_of_valid": np.nonzero(valid)[0], "pre": aux["pre"].double().numpy(), "range": aux["range"]}


def margins_ok(f):
    ok = np.ones(f["face"].shape, bool)
    for k, m in MARGINS.items():
        ok &= f[k] >= m
    return ok


@functools.lru_cache(maxsize=64)
def _pool(seed, S, masked, variant, gauge_on):
    g, _, _, mask = toy()
    rays = pool_rays(seed)
    jitter = synth.hash_uniform(seed, 701, (rays.shape[0],))
    f = facts(model_params(seed, variant), geometry_of(variant, g), mask if masked else None, rays, jitter, S, gauge_on)
    order = np.argsort(synth.hash_uniform(seed, 702, (rays.shape[0],)), kind="stable")
    return rays, jitter, f, order[margins_ok(f)[order]]


def rejected_share(seed, S, masked, variant, gauge_on):
    rays, _, _, order = _pool(seed, S, bool(masked), variant, bool(gauge_on))
    return 1.0 - len(order) / len(rays)


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


def _lonely_bin(f, j):
    """(plane, bin) that holds exactly one of ray j's active samples, or None"""
    mine = f["bins"][f["ray_of_active"] == j]
    for p in range(3):
        ids, cnt = np.unique(mine[:, p][mine[:, p] >= 0], return_counts=True)
        if (cnt == 1).any():
            return p, int(ids[cnt == 1][0])
    return None


def _heavy_last(f, pick):
    """the ray whose last active sample weighs most goes last: the batch's last active row then carries a weight no yardstick hides (a batch's
    last row is otherwise as likely as not a sample just above the threshold, whose loss no criterion could see)"""
    if pick:
        pick.append(pick.pop(int(np.argmax(f["last_w"][pick]))))
    return pick


def edge_batch(seed, S, masked=False, variant="base", gauge_on=True, active=None, R=None, no_valid=False, extra=3, dup=None):
    """A batch of pool rays in a seeded order.  active: rays whose fp64 active counts add up to exactly that many (0: none of them has an
    active sample), then `extra` rays without a valid sample.  R: the first R usable rays whatever their counts.  no_valid: R rays
    without one valid sample.  Of both kinds the ray whose last active sample weighs most comes last (``_heavy_last``).  dup: the first usable ray of which some colour bin holds exactly one active sample, that many times, with one
    target ("bin": the plane and the bin).  -> rays [n,6], jitter [n], rgb_train [n,3] (float32), "valid" and "active" (the fp64 counts per ray), "margin"
    (the smallest margin of each kind over the batch) and the "params" and "geometry" of the seed and variant."""
    rays, jitter, f, order = _pool(seed, S, bool(masked), variant, bool(gauge_on))
    miss = [j for j in order if f["valid"][j] == 0]
    lonely = None
    if no_valid:
        pick = miss[:R]
    elif dup is not None:
        j = next(j for j in order if f["active"][j] > 1 and f["last_w"][j] >= DUP_LAST_W and _lonely_bin(f, j) is not None)
        lonely = _lonely_bin(f, j)
        pick = [j] * int(dup)
    elif active is not None:
        if active == 0:
            pick = [j for j in order if f["active"][j] == 0 and f["valid"][j] > 0][:R or 37]
        else:
            pick = _subset(f["active"], order, int(active))
        pick = _heavy_last(f, list(pick)) + miss[:extra]
    else:
        pick = _heavy_last(f, list(order[:R]))
    pick = np.asarray(pick, np.int64)
    n = len(pick)
    assert n > 0 and (active is not None or dup is not None or n == R), "the pool holds too few such rays"
    tgt = synth.hash_uniform(seed, 703, (n, 3))
    if dup is not None:
        # the copies share their target as well: with a target of its own per copy the gradient is (sum over copies of out - target) times one
        # ray's Jacobian, a sum that cancels to about 1 / sqrt(dup) of its terms -- a test of that conditioning, not of the colliding taps
        tgt = np.ascontiguousarray(np.broadcast_to(tgt[:1], (n, 3)))
    return {"rays": rays[pick], "jitter": jitter[pick], "rgb_train": tgt, "valid": f["valid"][pick], "active": f["active"][pick],
            "margin": {k: float(f[k][pick].min()) for k in MARGINS}, "params": model_params(seed, variant),
            "geometry": geometry_of(variant), "S": S, "masked": bool(masked), "gauge_on": bool(gauge_on), "variant": variant, "bin": lonely,
            "seed": seed}


EDGE_S = 24
EDGE_ACTIVE = (1, 15, 16, 17, 31, 32, 33)          # around the 16-sample pass of the colour kernels and the 32-row k-chunk of xty_block
CHUNK, CHUNK_ACTIVE = 64, (63, 64, 65, 129)        # chunk_samples = 64: a full chunk less one, one chunk, the first row of a second, of a third
SPEC_ROWS = 48                                     # chunk_samples = -48: speculative rows that the batch fills, and fills less one
# (rays, samples): one ray; 129 = two 64-step waves of train_density_kernel and one step; ragged four-ray blocks of train_scan_kernel; S not a
# multiple of 16; 1023 / 1025 / 2049 rays: one, two and three rays per train_prefix_kernel thread
EDGE_RAYS = ((1, 7), (3, 129), (5, 17), (37, 45), (257, 65), (1023, EDGE_S), (1025, EDGE_S), (2049, EDGE_S))
EDGE_DUP = (255, 256, 257, 513)                    # a bin one short of kBinChunk = 256, full, one over (two units), and of three units


def edge_cases():
    """{id: (edge_batch keywords, white background, trainer keywords)}: every batch of tests/test_gpu_triplane_train_edges.py that is held to
    the fp64 criterion (tests/test_triplane_train_edges_cpu.py builds each of them on the CPU and checks its counts and margins)"""
    c = {}
    for white in (True, False):
        bg = "white" if white else "black"
        c[f"active0-{bg}"] = (dict(S=EDGE_S, variant="dark", active=0, R=37), white, {})
        c[f"novalid-{bg}"] = (dict(S=EDGE_S, no_valid=True, R=37), white, {})
    for i, a in enumerate(EDGE_ACTIVE):
        c[f"active{a}"] = (dict(S=EDGE_S, active=a), i % 2 == 0, {})
    for a in CHUNK_ACTIVE:
        c[f"chunk{a}"] = (dict(S=EDGE_S, active=a, variant="fog"), True, dict(chunk_samples=CHUNK))
    c["spec-full"] = (dict(S=EDGE_S, active=SPEC_ROWS), True, dict(chunk_samples=-SPEC_ROWS))
    c["spec-less"] = (dict(S=EDGE_S, active=SPEC_ROWS - 1), False, dict(chunk_samples=-SPEC_ROWS))
    for i, (R, S) in enumerate(EDGE_RAYS):
        c[f"rays{R}x{S}"] = (dict(S=S, R=R), i % 3 != 2, {})
    for n in EDGE_DUP:
        c[f"dup{n}"] = (dict(S=EDGE_S, dup=n), True, {})
    c["far_gauge"] = (dict(S=EDGE_S, R=96, variant="far_gauge"), True, {})
    c["gauge-off"] = (dict(S=EDGE_S, R=96, gauge_on=False), True, {})
    c["mask-on-black"] = (dict(S=EDGE_S, R=128, masked=True), False, {})
    c["mask-off-white"] = (dict(S=EDGE_S, R=128, masked=True, gauge_on=False), True, {})
    c["bright"] = (dict(S=EDGE_S, R=96, variant="bright"), True, {})
    c["softplus"] = (dict(S=EDGE_S, R=96, variant="softplus"), True, {})
    return c


# ---- the criterion ----------------------------------------------------------------------------------------------------------------------------
PIX_TOL = 2e-6
NORM_K, FLOOR = 4.0, 1e-5
ENTRY_K = 4.0          # the entry-wise bound: max |hip - f64| / max |f64| <= max(ENTRY_K x the same of fp32 torch, FLOOR); a case may raise it to 16


def group(k):
    return "planes-density" if k.endswith("[:16]") else "planes-colour" if k.endswith("[16:]") else "planes" if k.startswith("plane_") else "gauges" if k.startswith("gauge_") else k.split(".")[0]


# what the criterion holds: every tensor, and the planes' density and colour channels on their own as well (the density channels carry the
# rounding of raw2alpha, about 1e-5; measured against that, a colour channel's 1e-6 would hide a missing tap)
PARTS = tuple((k, k, slice(None)) for k in PARAM_NAMES) + tuple((f"{k}[:16]", k, slice(0, DD)) for k in PLANES) \
    + tuple((f"{k}[16:]", k, slice(DD, None)) for k in PLANES)


def _errors(res, name, k, ch):
    """(2-norm error, entry-wise error) of run `name` on channels ch of tensor k over the seeds stacked, both relative to fp64; None where fp64 is
    all zero"""
    cut = (lambda a: a[:, ch]) if ch != slice(None) else (lambda a: a)
    num = sum(float(torch.linalg.norm(cut(r[name][2][k]).double() - cut(r["t64"][2][k]))) ** 2 for r in res)
    den = sum(float(torch.linalg.norm(cut(r["t64"][2][k]))) ** 2 for r in res)
    if den == 0:
        return None, None
    top = max(float(cut(r["t64"][2][k]).abs().max()) for r in res)
    return (num / den) ** 0.5, max(float((cut(r[name][2][k]).double() - cut(r["t64"][2][k])).abs().max()) for r in res) / top


def check(res, label, paths, entry_k=ENTRY_K, pixels=True, tag="tp_edges"):
    """The criterion over the seeds stacked, on every path of `paths`.  res: [{run: (rgb_map or None, loss, {name: gradient}, ...)}] with the
    runs "t32" (fp32 torch), "t64" (fp64 torch) and the paths.  Loss within 1e-5 relative of fp64; rgb_map within max(2e-6, 4 e_torch32); per
    tensor e_hip <= max(4 e_torch32, 1e-5) in the 2-norm and, entry-wise, relative to the largest fp64 entry, <= max(entry_k e_torch32, 1e-5);
    where fp64 is exactly zero on every seed the path's gradient is exactly zero.  Prints the ratios; raises AssertionError."""
    assert entry_k <= 16
    bad = {}
    for r in res:
        l64 = r["t64"][1]
        for p in paths:
            assert abs(r[p][1] - l64) <= 1e-5 * max(1.0, abs(l64)), (label, p, "loss", r[p][1], l64)
            if pixels and r[p][0] is not None:
                e_t = float((r["t32"][0].double() - r["t64"][0]).abs().max())
                e_h = float((r[p][0].double() - r["t64"][0]).abs().max())
                print(f"{tag} {label} {p} rgb_map: hip {e_h:.2e} fp32 torch {e_t:.2e} of fp64")
                assert e_h <= max(PIX_TOL, 4 * e_t), (label, p, "rgb_map", e_h, e_t)
    for p in paths:
        worst = {}
        for k, tensor, ch in PARTS:
            gh = [r[p][2][tensor][:, ch] if ch != slice(None) else r[p][2][tensor] for r in res]
            assert all(bool(torch.isfinite(g).all()) for g in gh), (label, p, k)
            (n_h, m_h), (n_t, m_t) = _errors(res, p, tensor, ch), _errors(res, "t32", tensor, ch)
            if n_h is None:          # the fp64 gradient is exactly zero on every seed
                assert all(bool((g == 0).all()) for g in gh), (label, p, k, "fp64 is exactly zero, this gradient is not")
                continue
            if not n_h <= max(NORM_K * n_t, FLOOR):
                bad[(p, k, "norm")] = (n_h, n_t)
            if not m_h <= max(entry_k * m_t, FLOOR):
                bad[(p, k, "entry")] = (m_h, m_t)
            w = worst.setdefault(group(k), [-1.0, -1.0, None, None])
            if n_h / max(n_t, 1e-30) >= w[0]:
                w[0], w[2] = n_h / max(n_t, 1e-30), (n_h, n_t, k)
            if m_h / max(m_t, 1e-30) >= w[1]:
                w[1], w[3] = m_h / max(m_t, 1e-30), (m_h, m_t, k)
        for grp, (rn, rm, a, b) in sorted(worst.items()):
            print(f"{tag} {label} {p} {grp}: norm e_hip {a[0]:.3e} e_torch32 {a[1]:.3e} ratio {rn:.2f} ({a[2]}); "
                  f"entry e_hip {b[0]:.3e} e_torch32 {b[1]:.3e} ratio {rm:.2f} ({b[2]})")
    assert not bad, (label, bad)
