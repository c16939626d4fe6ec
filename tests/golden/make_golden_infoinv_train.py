#!/usr/bin/env python3
"""Capture the InfoInv training golden vectors FROM THE REFERENCE ITSELF (run in the build container only).

    python tests/golden/make_golden_infoinv_train.py     # writes tests/golden/infoinv_train_{on_white,off_black}.npz

The reference InfoInv module (InfoInv/models) on CPU, in training mode, with the per-ray jitter of sample_ray and the background coin pinned the
way make_golden.capture_train pins them; the loop of InfoInv/main.py:262-330: rgb MSE + 8e-5 * density_L1, backward, torch.optim.Adam over
get_optparam_groups with the lr decay.  Stored: rgb_map of iteration 0, the gradients of the rgb loss ALONE (the L1 term is of the order of
the render gradient on toy planes and would hide a wrong scatter) and of the total loss at iteration 0 (planes only: the MLP tensors'
total-loss gradients equal their rgb-only ones), and the parameters after two steps.
Parameters come from ngf_amd.synth (checksums stored); the files hold data only.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _checksums, _import_ref, _load_params, _rays_for_case, synth  # noqa: E402


def _get(field, k):
    obj = field
    for part in k.split(".")[:-1]:
        obj = getattr(obj, part) if not part.isdigit() else obj[int(part)]
    return getattr(obj, k.split(".")[-1])


def capture(name, seed, infoinv, white_bg, with_mask, S=40, steps=2, coin=0.7):
    F = _import_ref("InfoInv")
    aabb = torch.tensor([[-1.5, -1.5, -1.5], [1.5, 1.5, 1.5]])
    grid = [12, 10, 9]
    plane_hw = ((10, 12), (9, 10), (9, 12))
    params = synth.infoinv_params(seed, plane_hw, preset="R1")
    with contextlib.redirect_stdout(io.StringIO()):
        field = F.TriPlane(aabb, grid, "cpu", near_far=[2.0, 6.0], alphaMask_thres=1e-4, distance_scale=25,
                           rayMarch_weight_thres=1e-4, step_ratio=0.5)
    _load_params(field, params)
    extra = {}
    if with_mask:
        dhw = (9, 11, 13)
        vol, bits = synth.alpha_mask_bits(seed, dhw)
        maabb = torch.tensor([[-1.45, -1.35, -1.4], [1.3, 1.5, 1.25]])
        field.alphaMask = F.AlphaGridMask("cpu", maabb, torch.from_numpy(vol.astype(np.float32)))
        extra = {"mask_bits": bits, "mask_dhw": np.array(dhw), "mask_aabb": maabb.numpy()}
    rays = _rays_for_case(seed, 96, 32)
    n = rays.shape[0]
    rgb_train = synth.hash_uniform(seed, 800, (n, 3))
    lr_factor = 0.1 ** (1 / 30000)
    opt = torch.optim.Adam(field.get_optparam_groups(0.02, 0.001), betas=(0.9, 0.99))
    names = list(params)
    out = {}
    real_rand_like, real_rand = torch.rand_like, torch.rand
    for it in range(steps):
        U = synth.hash_uniform(seed, 810 + it, (n, 1))
        torch.rand_like = lambda *a, **k: torch.from_numpy(U.copy())
        torch.rand = lambda *a, **k: torch.tensor([coin])
        try:
            o = field(torch.from_numpy(rays), is_train=True, white_bg=white_bg, N_samples=S, infoinv=infoinv)
        finally:
            torch.rand_like, torch.rand = real_rand_like, real_rand
        rgb_loss = torch.mean((o["rgb_map"] - torch.from_numpy(rgb_train)) ** 2)
        total = rgb_loss + 8e-5 * field.density_L1()
        opt.zero_grad()
        if it == 0:
            rgb_loss.backward(retain_graph=True)
            for k in names:
                out[f"grad_rgb0.{k}"] = _get(field, k).grad.numpy().copy()
            opt.zero_grad()
        total.backward()
        if it == 0:         # density_L1 touches the planes only: the total-loss gradients of the MLP tensors are the rgb-only ones (kept once)
            for k in names:
                g = _get(field, k).grad.numpy()
                if k.startswith("plane_"):
                    out[f"grad0.{k}"] = g.copy()
                else:
                    assert np.array_equal(g, out[f"grad_rgb0.{k}"]), k
            out["rgb_map0"] = o["rgb_map"].detach().numpy().copy()
            out["rgb_loss0"] = np.float64(rgb_loss.item())
            out["total_loss0"] = np.float64(total.item())
        out[f"jitter{it}"] = U[:, 0]
        opt.step()
        for g in opt.param_groups:
            g["lr"] = g["lr"] * lr_factor
    for k in names:
        out[f"after.{k}"] = _get(field, k).detach().numpy().copy()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), model="infoinv", seed=seed, preset="R1", infoinv=int(infoinv), white_bg=int(white_bg),
                        coin=np.float32(coin), S=S, steps=steps, aabb=aabb.numpy(), grid=np.array(grid), plane_hw=np.array(plane_hw),
                        near_far=np.array([2.0, 6.0], np.float32), distance_scale=np.float32(25), thr=np.float32(1e-4),
                        stepSize=field.stepSize.numpy(), rays=rays, rgb_train=rgb_train, lr_factor=np.float64(lr_factor),
                        **_checksums(params), **extra, **out)
    print(f"{name}: rays {n} S {S} rgb loss {out['rgb_loss0']:.6f} |grad_rgb plane_xy| {np.abs(out['grad_rgb0.plane_xy']).mean():.3e} "
          f"|grad plane_xy| {np.abs(out['grad0.plane_xy']).mean():.3e}")


if __name__ == "__main__":
    capture("infoinv_train_on_white", seed=91, infoinv=True, white_bg=True, with_mask=True)
    capture("infoinv_train_off_black", seed=92, infoinv=False, white_bg=False, with_mask=False)
