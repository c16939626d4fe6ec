#!/usr/bin/env python3
"""The InfoInv tree's own loop (InfoInv/main.py:262-330) on the drop-in field with `field.differentiable = True`, at the reference's batch
shape: 4096 rays x 884 samples, 256^2 planes, preset R1 (R2 with an argument).  Prints ms per iteration (median of device-event times after
warm-up) and the split forward / loss + density_L1 / backward / Adam step, each section between two device events.

    python profiles/exp_infoinv_train.py [R1|R2] [iterations]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import ngf_amd  # noqa: F401
from ngf_amd import cases, synth

preset = sys.argv[1] if len(sys.argv) > 1 else "R1"
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10
dev = "cuda"
frame = synth.lookat_rays(800, 800)
pick = (synth.hash_uniform(9, 1, (4096,)) * np.float32(frame.shape[0])).astype(np.int64)
rays = torch.from_numpy(frame[pick]).to(dev)
tgt = torch.from_numpy(synth.hash_uniform(9, 2, (4096, 3))).to(dev)

g, params, step = cases.big_case("infoinv", preset)
f = cases.field_for_case(g, params, None, device=dev)
f.differentiable = True
S = int(f.nSamples)
opt = torch.optim.Adam(f.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99))
SECTIONS = ("forward", "loss", "backward", "step")
times = {k: [] for k in SECTIONS + ("total",)}
for i in range(3 + iters):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    ev[0].record()
    out = f(rays, is_train=True, white_bg=True, N_samples=S, infoinv=True)
    ev[1].record()
    rgb_loss = torch.mean((out["rgb_map"] - tgt) ** 2)
    total = rgb_loss + 8e-5 * f.density_L1()
    opt.zero_grad()
    ev[2].record()
    total.backward()
    ev[3].record()
    opt.step()
    ev[4].record()
    torch.cuda.synchronize()
    if i >= 3:
        for k, a, b in zip(SECTIONS, ev[:-1], ev[1:]):
            times[k].append(a.elapsed_time(b))
        times["total"].append(ev[0].elapsed_time(ev[4]))
eng = f._ii_engine
print(f"InfoInv training loop, {preset}, 4096 rays x {S} samples, 256^2 planes, torch.optim.Adam, {iters} iterations after 3 warm-up")
print(f"engine buffers {eng.bytes / 2**30:.2f} GiB; loss {float(rgb_loss.detach()):.6f}")
for k in SECTIONS + ("total",):
    print(f"  {k:9s} median {np.median(times[k]):8.3f} ms   (min {np.min(times[k]):.3f}, max {np.max(times[k]):.3f})")
