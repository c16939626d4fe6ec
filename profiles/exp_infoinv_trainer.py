#!/usr/bin/env python3
"""The fused InfoInv trainer (ngf_amd.infoinv_train.Trainer.step) against the drop-in loop (autograd + torch.optim.Adam, the loop of
profiles/exp_infoinv_train.py) at the reference's batch shape: 4096 rays x 884 samples, 256^2 planes, preset R1 (R2 with an argument).
Both run in ONE process on two fields built from the same parameters, in alternating blocks after a warm-up that covers the clock ramp;
prints each block's median ms per iteration (device events around the block's iterations), the median of the block medians of either
path and their spread (min .. max of the block medians).

    python profiles/exp_infoinv_trainer.py [R1|R2] [blocks] [iterations per block] [both|fused|dropin]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import ngf_amd  # noqa: F401
from ngf_amd import cases, infoinv_train, synth

preset = sys.argv[1] if len(sys.argv) > 1 else "R1"
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 5
per = int(sys.argv[3]) if len(sys.argv) > 3 else 10
which = sys.argv[4] if len(sys.argv) > 4 else "both"
dev = "cuda"
frame = synth.lookat_rays(800, 800)
pick = (synth.hash_uniform(9, 1, (4096,)) * np.float32(frame.shape[0])).astype(np.int64)
rays = torch.from_numpy(frame[pick]).to(dev)
tgt = torch.from_numpy(synth.hash_uniform(9, 2, (4096, 3))).to(dev)
g, params, step = cases.big_case("infoinv", preset)

paths = {}
if which in ("both", "dropin"):
    fa = cases.field_for_case(g, params, None, device=dev)
    fa.differentiable = True
    S = int(fa.nSamples)
    opt = torch.optim.Adam(fa.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99))

    def dropin():
        out = fa(rays, is_train=True, white_bg=True, N_samples=S, infoinv=True)
        rgb_loss = torch.mean((out["rgb_map"] - tgt) ** 2)
        total = rgb_loss + 8e-5 * fa.density_L1()
        opt.zero_grad()
        total.backward()
        opt.step()
        return rgb_loss.detach()
    paths["drop-in"] = dropin
if which in ("both", "fused"):
    fb = cases.field_for_case(g, params, None, device=dev)
    S = int(fb.nSamples)
    tr = infoinv_train.Trainer(fb, batch_size=4096, max_samples=S)

    def fused():
        return tr.step(rays, tgt, N_samples=S, white_bg=True, infoinv=True)
    paths["fused"] = fused


def block(fn, n):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    ev[0].record()
    for i in range(n):
        loss = fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in zip(ev[:-1], ev[1:])], float(loss)


for name, fn in paths.items():          # warm-up: code objects, the engines' buffers, the clock ramp
    block(fn, 30)
meds = {k: [] for k in paths}
for b in range(blocks):
    for name, fn in paths.items():
        t, loss = block(fn, per)
        meds[name].append(float(np.median(t)))
        print(f"block {b} {name:8s} median {np.median(t):8.3f} ms  (min {np.min(t):.3f}, max {np.max(t):.3f})  loss {loss:.6f}")
print(f"InfoInv training iteration, {preset}, 4096 rays x {S} samples, 256^2 planes, {blocks} alternating blocks of {per} iterations after 30 warm-up")
for name in paths:
    m = meds[name]
    print(f"  {name:8s} median of block medians {np.median(m):8.3f} ms   spread {np.min(m):.3f} .. {np.max(m):.3f} ms")
if len(paths) == 2:
    a, b = meds["drop-in"], meds["fused"]
    print(f"  drop-in - fused = {np.median(a) - np.median(b):.3f} ms; the two spreads together {np.max(a) - np.min(a) + np.max(b) - np.min(b):.3f} ms")
