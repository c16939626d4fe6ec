#!/usr/bin/env python3
"""The inverse gauge on the GPU: ngf_uv_inverse_map against uvmapping.InverseNetwork in fp32 torch, same device, same
points, same process.

    python profiles/uv_inverse.py [--out profiles/uv_inverse.txt]

Method: time between two device events around ONE call, median of 9 after 3 warm-up calls, at n = 40 962 (the vertices of icosphere 6), 2^18
and 2^20 points, both primitives; min and max of the nine stand beside the median (the run-to-run spread).  Rate = 2 MAC / time; the fraction
is of 157.3 TFLOP/s, the fp32 matrix peak the project measures against (sections 4.8, 4.11).  Then cycle_error over 2^20 points and
coordinate_deformation(icosphere_division=6 / side=203) end to end: wall clock around the call with a device synchronisation (median of 5),
and the device's share as the event time of the same call."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ngf_amd  # noqa: E402,F401
from ngf_amd import mesh, synth, uvmapping  # noqa: E402

PEAK = 157.3e12
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def events(fn, reps=9, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def wall(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    w, d = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        w.append((time.perf_counter() - t0) * 1e3)
        d.append(a.elapsed_time(b))
    k = int(np.argsort(w)[len(w) // 2])
    return w[k], d[k]


def make_net(prim):
    net = uvmapping.NeuTex(primitive_type=prim, sample_num=64, device="cuda")
    params = dict(synth.uvmapping_params(61, prim))
    params.update(synth.inverse_gauge_params(71, prim))
    net.load_params(params)
    return net


def points(prim, n):
    if prim == "sphere" and n == 40962:
        return torch.from_numpy(mesh.icosphere(6)[0]).cuda()
    g = torch.Generator(device="cuda").manual_seed(n)
    if prim == "square":
        return torch.rand((n, 2), device="cuda", generator=g) * 2 - 1
    return torch.nn.functional.normalize(torch.randn((n, 3), device="cuda", generator=g), dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uv_inverse.txt"))
    args = ap.parse_args()
    prop = torch.cuda.get_device_properties(0)
    say(f"device: {prop.name}, {prop.multi_processor_count} CUs; torch {torch.__version__}")
    say("kernel: ngf_uv_inverse_map (fp32 MFMA, 16 points per wave pass, 4 waves per block, one block per CU); eager: uvmapping.InverseNetwork, fp32 torch")
    say(f"{'prim':7s}{'n':>9s} | {'hip ms (min .. max)':>26s} {'TFLOP/s':>8s} {'of peak':>8s} | {'eager ms (min .. max)':>26s} {'TFLOP/s':>8s} {'of peak':>8s} | {'eager/hip':>9s} | max|hip - eager|")
    for prim in ("sphere", "square"):
        net = make_net(prim)
        D = net.inverse_gauge.input_point_dim
        mac = 64 * D + 64 * 512 + 2 * 512 * 512 + 512 * 3
        for n in (40962, 1 << 18, 1 << 20):
            uv = points(prim, n)
            with torch.no_grad():
                diff = float((net.inverse_map(uv) - net.inverse_gauge.map(uv)).abs().max())
                h = events(lambda: net.inverse_map(uv))
                e = events(lambda: net.inverse_gauge.map(uv))
            fl = 2.0 * mac * n
            say(f"{prim:7s}{n:9d} | {h[0]:9.3f} ({h[1]:7.3f} .. {h[2]:7.3f}) {fl / h[0] / 1e9:8.1f} {fl / (h[0] * 1e-3) / PEAK:8.3f} | "
                f"{e[0]:9.3f} ({e[1]:7.3f} .. {e[2]:7.3f}) {fl / e[0] / 1e9:8.1f} {fl / (e[0] * 1e-3) / PEAK:8.3f} | {e[0] / h[0]:9.2f} | {diff:.2e}")
            if n == 1 << 20:
                slower = h[1] > e[2]
                say(f"        requirement at 2^20 (hip not slower than eager beyond the spread): hip min {h[1]:.3f} ms vs eager max {e[2]:.3f} ms -> "
                    f"{'MISSED' if slower else 'met'}")
        xyz = torch.rand((1 << 20, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)) * 2 - 1
        c = events(lambda: net.cycle_error(xyz))
        say(f"{prim:7s} cycle_error over 2^20 points: {c[0]:.3f} ms ({c[1]:.3f} .. {c[2]:.3f}) -- the gauge query, the inverse map and the reduction")
        kw = {"icosphere_division": 6} if prim == "sphere" else {"side": 203}
        w, _ = wall(lambda: net.coordinate_deformation(**kw))
        tv = mesh.icosphere(6)[0] if prim == "sphere" else mesh.square_template(203)[0]
        t = torch.from_numpy(tv).cuda()
        d = events(lambda: (net.inverse_map(t), net.texture_colors(t, (0, 0, 1)), mesh.atlas_coords(t, prim, 512 if prim == "sphere" else None)), reps=5, warm=2)
        say(f"{prim:7s} coordinate_deformation({', '.join(f'{k}={v}' for k, v in kw.items())}), {len(tv)} vertices, no file: wall {w:.2f} ms; device {d[0]:.2f} ms "
            f"(event time of its three device stages on a resident template), host {w - d[0]:.2f} ms (the template in numpy, its upload, the launches)")
        net.release()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
