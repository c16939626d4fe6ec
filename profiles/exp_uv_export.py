"""UV-Mapping (NeuTex) texture export on one GPU: net_texture.export_textures(R) through the HIP kernel (ngf_uv_texture_eval) against eager torch
running the same nn.Sequential modules on the same GPU and the same points (tests/uv_export_eager.texture_forward), for the sphere (6 R^2
points) and the square (R^2 points) model, in view and diffuse mode.  Clocks are ramped with a second of the workload itself, every shape is
warmed up, and the two sides alternate in blocks; a block is timed with a host clock around a device synchronise.

    python profiles/exp_uv_export.py [--res 512] [--iters 40] [--block 5] [--out profiles/uv_export.txt]

Three times per case: `export` is the exporter as a user calls it (sample points cached on the device by the first call), `kernel` the
ngf_uv_texture_eval launch alone between two device events, `eager` the torch modules.  The floor is 2 x MACs over the fp32 matrix peak
(157.3 TFLOP/s: 256 CUs x 256 FLOP/clk x 2.4 GHz); the fraction of peak is that floor over the kernel time."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ngf_amd  # noqa: E402,F401
import uv_export_eager as E  # noqa: E402

PEAK = 157.3e12


def macs(prim, diffuse):
    first = (63 if prim == "sphere" else 42) * 256
    block1 = first + 5 * 256 * 256 + 256 * 3
    return block1 if diffuse else block1 + 295 * 256 + 3 * 256 * 256 + 256 * 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--block", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uv_export.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_uv_export.py measures on the GPU; no device found")
    dev, R = "cuda:0", a.res
    lines = [f"# export_textures({R}) on {torch.cuda.get_device_name(0)}; ms are medians of {a.iters // a.block} blocks of {a.block} calls (min..max of the blocks)"]
    for prim in ("sphere", "square"):
        net = E.make_net(prim, dev)
        kind = "cube" if prim == "sphere" else "sq"
        pts = E.build_points(kind, R).to(dev)
        n = pts.numel() // pts.shape[-1]
        for viewdir in ([0.0, 0.0, 1.0], None):
            diffuse = viewdir is None
            view = None if diffuse else torch.tensor(viewdir, device=dev)

            def export():
                return net.net_texture.export_textures(R, viewdir)

            def kernel():
                return net.texture_colors(pts, view, diffuse=diffuse)

            @torch.no_grad()
            def eager():
                return E.texture_forward(net.net_texture, pts, view)

            got, want = export(), eager()
            diff = float((got - want).abs().max())
            t_end = time.perf_counter() + 1.0                    # clock ramp: a second of the workload itself
            while time.perf_counter() < t_end:
                kernel()
                torch.cuda.synchronize()
            for f in (export, kernel, eager):
                for _ in range(3):
                    f()
            torch.cuda.synchronize()
            ms = {"export": [], "kernel": [], "eager": []}
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            for _ in range(a.iters // a.block):
                for name, f in (("export", export), ("eager", eager)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.block):
                        f()
                    torch.cuda.synchronize()
                    ms[name].append((time.perf_counter() - t0) * 1e3 / a.block)
                ev[0].record()
                for _ in range(a.block):
                    kernel()
                ev[1].record()
                torch.cuda.synchronize()
                ms["kernel"].append(ev[0].elapsed_time(ev[1]) / a.block)
            flop = 2.0 * macs(prim, diffuse) * n
            floor = flop / PEAK * 1e3
            med = {k: float(np.median(v)) for k, v in ms.items()}
            lines.append(f"{prim} {'diffuse' if diffuse else 'view'}: {n} points, {flop / 1e12:.3f} TFLOP, matrix floor {floor:.2f} ms; "
                         + "; ".join(f"{k} {med[k]:.2f} ms ({min(v):.2f}..{max(v):.2f})" for k, v in ms.items())
                         + f"; kernel at {floor / med['kernel']:.3f} of the fp32 matrix peak ({flop / med['kernel'] / 1e9:.1f} TFLOP/s); "
                         f"eager / export = {med['eager'] / med['export']:.2f}x; max|hip - eager| = {diff:.2e}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
