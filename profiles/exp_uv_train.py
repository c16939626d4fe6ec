"""UV-Mapping (NeuTex) training step on one GPU: the HIP engine (net.differentiable = True) against the eager fp32 torch restatement of the same
loop (tests/uv_train_eager.py) -- forward, compute_loss (weights 1/1/1/0), zero_grad, backward, Adam(lr 1e-4) -- alternated in blocks after a
warm-up.  Shapes: dtu_train.sh (1 camera, a 24 x 24 ray patch, S = 64, P = 2500) for square and sphere, and 4096 rays (square).

    python profiles/exp_uv_train.py [--iters 200] [--block 20] [--only hip|eager] [--shape NAME]   # appends to profiles/uv_train.txt

The achieved rate counts 2 x MACs of the forward (gauge on every sample, geometry + texture on the in-cube ones) x 3 (forward + data and weight
gradients; the first layers need no data gradient, ignored) over the HIP step's wall time."""
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
import uv_train_eager as E  # noqa: E402

SHAPES = {"dtu_square": ("square", 576), "dtu_sphere": ("sphere", 576), "rays4096_square": ("square", 4096)}
MAC_GAUGE = 63 * 64 + 64 * 128 + 2 * 128 * 128 + 128 * 3
MAC_GEO = 63 * 256 + 10 * 256 * 256 + 256
MAC_TEX = 63 * 256 + 5 * 256 * 256 + 256 * 3 + 295 * 256 + 3 * 256 * 256 + 256 * 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--only", default=None)
    ap.add_argument("--shape", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uv_train.txt"))
    a = ap.parse_args()
    dev = "cuda:0"
    lines = []
    for name, (prim, R) in SHAPES.items():
        if a.shape and name != a.shape:
            continue
        S, P = 64, 2500
        params = E.model_params(81, prim)
        b = E.batch(81, prim, R=R, S=S, P=P)
        t = lambda k: torch.from_numpy(b[k]).to(dev)          # noqa: E731
        cam, rd, U, tp, gt, gtt = (t(k) for k in ("campos", "raydir", "U", "template", "gt_image", "gt_trans"))
        nets, opts = {}, {}
        for kind in ("hip", "eager"):
            if a.only and kind != a.only:
                continue
            n = E.make_net(params, prim, S, dev)
            n.differentiable = kind == "hip"
            nets[kind], opts[kind] = n, torch.optim.Adam(list(n.parameters()), lr=1e-4)

        def step(kind):
            n = nets[kind]
            out = n(cam, rd, None, jitter_u=U, template_points=tp) if kind == "hip" else E.forward(n, cam, rd, None, U, tp)
            loss = E.compute_loss(out, gt, gtt)
            opts[kind].zero_grad()
            loss.backward()
            opts[kind].step()

        for kind in nets:
            for _ in range(5):
                step(kind)
        torch.cuda.synchronize()
        ms = {k: [] for k in nets}
        done = 0
        while done < a.iters:
            for kind in nets:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.block):
                    step(kind)
                torch.cuda.synchronize()
                ms[kind].append((time.perf_counter() - t0) * 1e3 / a.block)
            done += a.block
        with torch.no_grad():
            from ngf_amd.uv_train import _UvRender  # noqa: F401
            _, _, valid = E.cube_ray_generation(cam, rd, S, U)
            nv = int(valid.sum())
        flop = 2.0 * 3 * (R * S * MAC_GAUGE + nv * (MAC_GEO + MAC_TEX))
        parts = [f"{name}: rays {R} S {S} P {P} in-cube samples {nv} of {R * S}"]
        for kind, v in ms.items():
            med = float(np.median(v))
            parts.append(f"{kind} {med:.3f} ms/iter (blocks {min(v):.3f}..{max(v):.3f})")
        if "hip" in ms:
            parts.append(f"{flop / 1e12:.3f} TFLOP/step -> {flop / (float(np.median(ms['hip'])) * 1e-3) / 1e12:.1f} TFLOP/s over the HIP step")
        if "hip" in nets:
            parts.append(f"engine {nets['hip']._uv_engine.bytes / 2**20:.0f} MiB")
        lines.append("; ".join(parts))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
