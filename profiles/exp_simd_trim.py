#!/usr/bin/env python3
"""Level-3 launches through several builds of the library in ONE process, alternating: ROUNDS rounds of REP launches per build (median ms per round),
the way profiles/r05_level3_ablations.txt was made.  Prints; the tables of profiles/r11_simd_trim.txt are its output.

    python profiles/exp_simd_trim.py plain=<path/libngf_hip.so> nomask=<path> nocollect=<path>
    SHAPES="R2 S884mask S884ball n160000 n80000 n40000 level2" ROUNDS=3 python profiles/exp_simd_trim.py parent=<path> new=<path>

Builds: make -C neural-gauge-fields_amd/csrc exp NAME=<n> DEFS=<d>, or the libngf_hip.so of another checkout.  Every build renders its own handle
(ngf_amd._lib.library(path)); outputs are compared with the first build's (reported, not asserted: the timing-only builds differ).
SHAPES (default "frame"): frame = 800 x 800, S = 192, preset R1 | R2 = the same, preset R2 | S884mask / S884ball = S = 884 through the field's own
updateAlphaMask((256,)*3) / a ball of radius 0.8 (profiles/workload.py) | n<rays> = that many rays of the R1 frame from row 200 | level2 = the R1 frame at level 2
| unequal / unequalS884ball = the frame / the ball shape with the yz gauge plane cropped to 256 x 248: gauge planes of unequal sizes, the GaugeAny<> instantiations."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import ngf_amd  # noqa: F401
from ngf_amd import _lib, synth, triplane
from ngf_amd.cases import big_case, field_for_case

builds = [a.split("=", 1) for a in sys.argv[1:]]
ROUNDS, REP = int(os.environ.get("ROUNDS", "5")), int(os.environ.get("REP", "20"))
full = torch.from_numpy(synth.lookat_rays(800, 800)).cuda()


def make(shape):
    """-> (field, rays, call keywords), created inside the current library"""
    g, params, step = big_case("triplane", "R2" if shape == "R2" else "R1")
    if shape.startswith("unequal"):
        params = dict(params)
        params["gauge_yz"] = np.ascontiguousarray(params["gauge_yz"][:, :, :, :-8])
        shape = shape[len("unequal"):]
    f = field_for_case(g, params, None, device="cuda", bake=True, bake_color=shape != "level2")
    rays, kw = full, dict(iteration=30001, row_width=800, white_bg=True, N_samples=192)
    if shape.startswith("S884"):
        kw["N_samples"] = -1
        if shape == "S884mask":
            f.updateAlphaMask((256, 256, 256))
        else:
            ax = torch.linspace(-1.5, 1.5, 128)
            zz, yy, xx = torch.meshgrid(ax, ax, ax, indexing="ij")
            f.alphaMask = triplane.AlphaGridMask("cuda", torch.tensor(np.asarray(g["aabb"], np.float32)), ((xx ** 2 + yy ** 2 + zz ** 2) < 0.8 ** 2).float().cuda())
            f.invalidate()
    if shape.startswith("n"):
        rays = full[200 * 800:200 * 800 + int(shape[1:])].contiguous()
    return f, rays, kw


for shape in os.environ.get("SHAPES", "frame").split():
    fields, outs, waves = {}, {}, {}
    for name, path in builds:
        with _lib.library(path) as L, torch.no_grad():
            fields[name] = make(shape)
            f, rays, kw = fields[name]
            for _ in range(3):
                outs[name] = f(rays, **kw)
            torch.cuda.synchronize()
            waves[name] = L.ngf_debug_get(b"last_waves")
    med = {name: [] for name, _ in builds}
    for r in range(ROUNDS):
        for name, path in builds:
            f, rays, kw = fields[name]
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REP)]
            with _lib.library(path), torch.no_grad():
                for a, b in ev:
                    a.record(); f(rays, **kw); b.record()
                torch.cuda.synchronize()
            med[name].append(float(np.median([a.elapsed_time(b) for a, b in ev])))
    first = builds[0][0]
    for name, path in builds:
        m = np.array(med[name])
        same = bool(torch.equal(outs[name]["rgb_map"], outs[first]["rgb_map"]) and torch.equal(outs[name]["depth_map"], outs[first]["depth_map"]))
        print(f"{shape:<9} {name:<10} waves {waves[name]:>2}  median {np.median(m):.4f} ms  spread {m.max() - m.min():.4f}  rounds {' '.join(f'{v:.4f}' for v in m)}  "
              f"vs {first}: {np.median(m) - np.median(np.array(med[first])):+.4f} ms  same pixels: {same}", flush=True)
    for name, path in builds:
        with _lib.library(path):
            fields[name][0].release()
    del fields, outs
