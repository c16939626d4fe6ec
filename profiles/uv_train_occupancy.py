"""NeuTex training through the occupancy grid on one GPU: what an iteration costs with and without a mask in the trainer
(net.occupancy_in_training), at the two shapes of section 4.7 -- the DTU batch (576 rays x 64 samples, P = 2500) and
4096 rays x 64 samples, square model, the weights, rays and loop of profiles/exp_uv_train.py: forward, compute_loss (weights 1/1/1/0),
zero_grad, backward, torch.optim.Adam(lr 1e-4).step().

    python profiles/uv_train_occupancy.py [--blocks 12] [--block 10] [--parent-lib PATH] [--shape NAME] [--out profiles/uv_train_occupancy.txt]

Conditions, each with its own model and optimiser, timed ALTERNATELY in one process (a block of `block` iterations of each per round, `blocks`
rounds, after a second of the workload to ramp the clocks and five warm iterations of each); a block is timed on the host clock between two
synchronisations; figures are the median of the block means (min .. max), and the spread of (b) is the yardstick for every difference:
  (a) the PARENT commit's libngf_hip.so (--parent-lib), through the same Python;
  (b) this library, the switch off;
  (c) an all-ones 128^3 mask: the look-up and the second form of the two kernels alone, every in-cube sample kept;
  (d) a 128^3 ball that fills 8 % of the cube (tests/uv_occupancy_ref.py: ball_mask): the object in empty space;
  (e) an all-zeros mask: nothing kept -- the floor left by the gauge network on every sample, batch-sized grids and the launch count.
The kept share is ngf_uv_train_counts of the last forward."""
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
from ngf_amd import _lib, uv_train  # noqa: E402
import uv_occupancy_ref as O  # noqa: E402
import uv_train_eager as E  # noqa: E402

SHAPES = {"dtu_square": ("square", 576), "rays4096_square": ("square", 4096)}
S, P = 64, 2500
NEW = ("ngf_uv_trainer_set_occupancy", "ngf_uv_train_counts", "ngf_uv_train_kept")


class _Absent:
    """Stands where the parent library lacks an entry point, so that uv_train._bind can set its argtypes; condition (a) installs no mask and
    asks for no counts, so it is never called (calling it raises)."""
    argtypes = None


def parent_library(path):
    L = _lib._load(os.path.abspath(path))
    for s in NEW:
        if not hasattr(L, s):
            setattr(L, s, _Absent())
    uv_train._bind(L)
    return os.path.abspath(path)


def fmt(ts):
    return f"{np.median(ts):8.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--shape", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uv_train_occupancy.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("uv_train_occupancy.py measures on the GPU; no device found")
    dev = "cuda:0"
    cells = (128, 128, 128)
    ball = O.ball_mask(cells)
    masks = {"(c) all-ones 128^3": np.ones(cells, bool), "(d) ball, 8 % of the cube": ball, "(e) all-zeros 128^3": np.zeros(cells, bool)}
    parent = parent_library(a.parent_lib) if a.parent_lib else None
    lines = [f"# NeuTex training through the occupancy grid on {torch.cuda.get_device_name(0)}: forward + backward + Adam per iteration, {a.block} iterations per "
             f"block, {a.blocks} blocks per condition alternating, host clock between synchronisations; median of the block means (min .. max)",
             f"# ball mask: {100 * ball.mean():.2f} % of the 128^3 cells"]
    for name, (prim, R) in SHAPES.items():
        if a.shape and name != a.shape:
            continue
        params = E.model_params(81, prim)
        b = E.batch(81, prim, R=R, S=S, P=P)
        t = lambda k: torch.from_numpy(b[k]).to(dev)          # noqa: E731
        cam, rd, U, tp, gt, gtt = (t(k) for k in ("campos", "raydir", "U", "template", "gt_image", "gt_trans"))
        conds = ([("(a) the parent commit's library", None, parent)] if parent else []) + [("(b) this library, switch off", None, None)]
        conds += [(k, v, None) for k, v in masks.items()]
        nets, opts = {}, {}
        for cname, mask, _ in conds:
            n = E.make_net(params, prim, S, dev)
            n.differentiable = True
            if mask is not None:
                n.set_occupancy(mask)
                n.occupancy_in_training = True
            nets[cname], opts[cname] = n, torch.optim.Adam(list(n.parameters()), lr=1e-4)

        def step(cname):
            n = nets[cname]
            out = n(cam, rd, None, jitter_u=U, template_points=tp)
            loss = E.compute_loss(out, gt, gtt)
            opts[cname].zero_grad()
            loss.backward()
            opts[cname].step()

        def run(cname, lib, k):
            if lib is None:
                for _ in range(k):
                    step(cname)
            else:
                with _lib.library(lib):          # (the engine is created inside: it keeps the library it was built on)
                    for _ in range(k):
                        step(cname)

        t_end = time.perf_counter() + 1.0
        while time.perf_counter() < t_end:          # ramp the clocks with the workload itself
            run(conds[-4][0], None, 1)
            torch.cuda.synchronize()
        for cname, _, lib in conds:
            run(cname, lib, 5)
        torch.cuda.synchronize()
        ms = {c[0]: [] for c in conds}
        for _ in range(a.blocks):
            for cname, _, lib in conds:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(cname, lib, a.block)
                torch.cuda.synchronize()
                ms[cname].append((time.perf_counter() - t0) * 1e3 / a.block)
        bname = "(b) this library, switch off"
        base = float(np.median(ms[bname]))
        spread = (max(ms[bname]) - min(ms[bname])) / base
        lines.append(f"{name}: {R} rays x {S} samples, P {P}   (run-to-run spread of (b): {100 * spread:.2f} % of its median; engine "
                     f"{nets[bname].grad_engine.bytes / 2**20:.0f} MiB)")
        for cname, _, lib in conds:
            if lib is None:
                inc, kept = nets[cname].grad_engine.counts()
                share = f"in-cube {inc:>7d} of {R * S}  kept {kept:>7d} ({100.0 * kept / max(inc, 1):5.1f} % of the in-cube samples)"
            else:
                share = "(no counts: the parent has no ngf_uv_train_counts)"
            lines.append(f"  {cname:<34s} {fmt(ms[cname])}  x{np.median(ms[cname]) / base:5.3f} of (b)   {share}")
        print("\n".join(lines[-len(conds) - 1:]), flush=True)
        for n in nets.values():
            n.release_grad_engine()
            n.release()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
