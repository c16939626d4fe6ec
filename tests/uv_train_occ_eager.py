"""tests/uv_train_eager.py's ``forward`` with the valid mask SUPPLIED by the caller: the torch restatement of NeuTex training through an
occupancy mask (``net.occupancy_in_training``).  ``keep`` [N,R,S] says which samples count; ``sigma = density * keep``
is the one line that differs, so with ``keep`` = the in-cube mask of the batch this returns ``E.forward``'s tensors bit for bit
(tests/test_uv_train_occupancy_cpu.py).  Every network still runs on every sample here -- a masked sample's weight is exactly 0, so the
geometry and texture networks get exactly no gradient from it, which is what the kernels do by not evaluating it.

Also the cases of tests/test_gpu_uv_train_occupancy.py (batch x mask), so that the CPU test can check them where the GPU test cannot."""
import numpy as np
import torch
import torch.nn.functional as F

import uv_occupancy_ref as O
import uv_train_eager as E

S = E.EDGE_V_S          # 23
BG1 = np.array([[0.2, 0.5, 0.8]], np.float32)
# (name, in-cube count V of the batch, the mask's volume): the cases of the gradient test, then the one that masks everything
CASES = (("checkerboard 8", 2049, lambda: O.checkerboard((8, 8, 8))),
         ("ball 16", 2049, lambda: O.ball_mask((16, 16, 16), radius=0.7)),
         ("ball 128", 2049, lambda: O.ball_mask((128, 128, 128))),
         ("random 5x7x16", 17, lambda: O.random_mask((5, 7, 16))))
EMPTY_CASE = ("ball 16 at V=17", 17, lambda: O.ball_mask((16, 16, 16), radius=0.7))
NEAR_SHARE = 0.01       # at most this share of a batch's in-cube samples lies within O.BOUNDARY_MARGIN of a cell boundary


def forward(net, campos, raydir, bg, U, template_points, keep):
    """E.forward(...) with ``valid`` replaced by ``keep`` (bool / uint8 [N,R,S], on the tensors' device)."""
    Sn = U.shape[-1]
    pos, seg, _ = E.cube_ray_generation(campos, raydir, Sn, U)
    raw = net.net_geometry_decoder.block(torch.cat([pos, E.positional_encoding(pos, 10)], dim=-1))[..., 0]
    density = F.softplus(raw)
    inv = net.inverse_gauge.inverse_network
    pts3 = E.inverse_network(inv, template_points.unsqueeze(0)).unsqueeze(1)
    points = pts3.view(pts3.shape[0], -1, pts3.shape[-1]).permute(0, 2, 1)
    e = net.gauge_transform.encoder
    x = F.relu(e.linear1(torch.cat([pos, E.positional_encoding(pos, 10)], dim=-1)))
    x = F.relu(e.linear2(x))
    for lin in e.linear_list:
        x = F.relu(lin(x))
    q = e.last_linear(x)
    uv = torch.tanh(q) if q.shape[-1] == 2 else F.normalize(q, dim=-1)
    t = net.net_texture
    h = t.block1(torch.cat([uv, E.positional_encoding(uv, 10)], dim=-1))
    c1 = F.softplus(t.color1(h))
    vd = raydir[:, :, None, :].expand(h.shape[:-1] + (3,))
    c2 = t.block2(torch.cat([h, vd, E.positional_encoding(vd, 6)], dim=-1))
    radiance = (c1 + c2).clamp(min=0)
    sigma = density * keep.to(density.dtype)
    opacity = 1 - torch.exp(-sigma * seg)
    acc = torch.cumprod(1.0 - opacity + 1e-10, dim=-1)
    bgT = acc[:, :, -1]
    acc = torch.cat([torch.ones_like(acc[:, :, :1]), acc[:, :, :-1]], dim=-1)
    w = opacity * acc
    color = torch.sum(radiance * w[..., None], dim=-2)
    if bg is not None:
        color = color + bg[:, None, :] * bgT[:, :, None]
    color = torch.pow(color + 1e-5, 1 / 2.2).clamp(0, 1)
    pinv = E.inverse_network(inv, uv.reshape(-1, uv.shape[-1])).view(uv.shape[:-1] + (3,))
    return {"color": color, "transmittance": bgT, "points": points, "points_original": pos, "points_inverse": pinv,
            "points_inverse_weights": w, "uv": uv}


def keep_of(volume, pos32):
    """The expected valid mask for float32 positions ``pos32`` [...,3] (numpy): in the cube AND the restated look-up of the cell's bit."""
    pos32 = np.asarray(pos32, np.float32)
    return O.lookup(O.pack(volume), volume.shape, pos32) & O.in_cube(pos32)
