#!/usr/bin/env python3
"""Training NeuTex's inverse gauge on the GPU: the HIP forward + backward (ngf_uv_inverse_train_*) against eager fp32
torch forward + backward of uvmapping.InverseNetwork, same device, same points, same process.

    python profiles/uv_inverse_train.py [--out profiles/uv_inverse_train.txt] [--skip-iteration]

Method: time between two device events, median of 11 after 3 warm-up rounds, min and max beside it (the run-to-run spread), at 2500 (the
template of the origin loss), 36 864 (the DTU batch's samples) and 2^18 points, sphere.  Through the C ABI: the forward call; the backward call
cut after the dX chain (ngf_debug_uv_inverse_train_dx); the whole backward (dX chain, five dW launches and their reductions); dW + reduce is the difference
of the two medians.  "total" is one forward and one backward between the same two events, d_uv asked for, gradients left in the engine -- eager
torch is timed the same way: forward, then torch.autograd.grad of sum(xyz * d_xyz) w.r.t. uv and the ten tensors.  Rates count 2 x 558 784 MAC
per point and pass (forward, dX, dW) against 157.3 TFLOP/s, the fp32 matrix peak the project measures against.
Then the W_INV DTU-batch iteration of profiles/exp_uv_train.py's loop (576 rays, S = 64, P = 2500, Adam) with inverse_gauge.differentiable on
and off in one process, alternated in blocks: wall clock per iteration."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ngf_amd  # noqa: E402,F401
from ngf_amd import _lib, synth, uvmapping  # noqa: E402
from ngf_amd.uv_inverse_train import InverseGrad  # noqa: E402

PEAK = 157.3e12
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def events(fn, reps=11, warm=3):
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


def fmt(t):
    return f"{t[0]:8.3f} ({t[1]:7.3f} .. {t[2]:7.3f})"


def make_net(prim):
    net = uvmapping.NeuTex(primitive_type=prim, sample_num=64, device="cuda")
    params = dict(synth.uvmapping_params(61, prim))
    params.update(synth.inverse_gauge_params(71, prim))
    net.load_params(params)
    return net


def kernels(prim="sphere"):
    net = make_net(prim)
    gauge = net.inverse_gauge
    D = gauge.input_point_dim
    mac = 64 * D + 64 * 512 + 2 * 512 * 512 + 512 * 3
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    say(f"{'n':>8s} | {'forward ms (min .. max)':>28s} {'peak':>5s} | {'dX chain':>28s} {'peak':>5s} | {'backward (dX + dW)':>28s} | {'dW+reduce':>9s} {'peak':>5s} | "
        f"{'hip total':>28s} {'peak':>5s} | {'eager total':>28s} {'peak':>5s} | eager/hip | engine MiB")
    for n in (2500, 36864, 1 << 18):
        g = torch.Generator(device="cuda").manual_seed(n)
        uv = torch.nn.functional.normalize(torch.randn((n, D), device="cuda", generator=g), dim=-1).contiguous()
        d_xyz = torch.randn((n, 3), device="cuda", generator=g).contiguous()
        eng = InverseGrad(gauge, n)
        xyz, d_uv = torch.empty((n, 3), device="cuda"), torch.empty((n, D), device="cuda")
        tk = C.c_int64(0)

        def fwd():
            _lib.check(L.ngf_uv_inverse_train_forward(eng._h, uv.data_ptr(), n, xyz.data_ptr(), C.byref(tk), st))

        def bwd():
            _lib.check(L.ngf_uv_inverse_train_backward(eng._h, tk.value, d_xyz.data_ptr(), d_uv.data_ptr(), st))

        def both():
            fwd()
            bwd()

        eng.sync()
        f = events(fwd)
        dx = events(lambda: _lib.check(L.ngf_debug_uv_inverse_train_dx(eng._h, tk.value, d_xyz.data_ptr(), d_uv.data_ptr(), st)))
        b = events(bwd)
        tot = events(both)
        params = list(gauge.inverse_network.parameters())

        def eager():
            u = uv.detach().requires_grad_(True)
            out = gauge.inverse_network(u)
            torch.autograd.grad((out * d_xyz).sum(), [u] + params)

        e = events(eager)
        fl = 2.0 * mac * n
        dw = b[0] - dx[0]
        pk = lambda ms, k=1: f"{k * fl / (ms * 1e-3) / PEAK:5.2f}"          # noqa: E731
        say(f"{n:8d} | {fmt(f)} {pk(f[0])} | {fmt(dx)} {pk(dx[0])} | {fmt(b)} | {dw:9.3f} {pk(dw)} | {fmt(tot)} {pk(tot[0], 3)} | {fmt(e)} {pk(e[0], 3)} | "
            f"{e[0] / tot[0]:9.2f} | {eng.bytes / 2**20:8.1f}")
        if n >= 36864:
            gap, spread = e[0] - tot[0], max(tot[2] - tot[1], e[2] - e[1])
            say(f"         acceptance at {n}: eager - hip = {gap:.3f} ms against the larger run-to-run spread {spread:.3f} ms -> {'met' if gap > spread else 'NOT REACHED'}")
        eng.release()
    net.release()


def iteration(iters, block):
    import uv_train_eager as E
    prim, R, S, P = "sphere", 576, 64, 2500
    W_INV = (1.0, 1.0, 1.0, 1.0)
    params = E.model_params(81, prim)
    b = E.batch(81, prim, R=R, S=S, P=P)
    t = lambda k: torch.from_numpy(b[k]).cuda()          # noqa: E731
    cam, rd, U, tp, gt, gtt = (t(k) for k in ("campos", "raydir", "U", "template", "gt_image", "gt_trans"))
    nets, opts = {}, {}
    for kind in ("inverse on kernels", "inverse in torch"):
        n = E.make_net(params, prim, S, "cuda")
        n.differentiable = True
        n.inverse_gauge.differentiable = kind == "inverse on kernels"
        nets[kind], opts[kind] = n, torch.optim.Adam(list(n.parameters()), lr=1e-4)

    def step(kind):
        out = nets[kind](cam, rd, None, jitter_u=U, template_points=tp)
        loss = E.compute_loss(out, gt, gtt, W_INV)
        opts[kind].zero_grad()
        loss.backward()
        opts[kind].step()

    for kind in nets:
        for _ in range(5):
            step(kind)
    torch.cuda.synchronize()
    ms = {k: [] for k in nets}
    for _ in range(max(1, iters // block)):
        for kind in nets:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(block):
                step(kind)
            torch.cuda.synchronize()
            ms[kind].append((time.perf_counter() - t0) * 1e3 / block)
    say(f"W_INV DTU-batch iteration ({prim}, {R} rays, S {S}, P {P}; render engine on in both; torch.optim.Adam), wall clock per iteration, blocks of {block}:")
    for kind, v in ms.items():
        say(f"    {kind:20s} {float(np.median(v)):.3f} ms/iter (blocks {min(v):.3f} .. {max(v):.3f})")
    eng = nets["inverse on kernels"].inverse_gauge.inverse_grad_engines()
    say(f"    engines: template {eng[0].max_rays} points {eng[0].bytes / 2**20:.1f} MiB, uv {eng[1].max_rays} points {eng[1].bytes / 2**20:.1f} MiB; "
        f"forwards per iteration {eng[0].forwards / (5 + len(ms['inverse on kernels']) * block):.2f} / {eng[1].forwards / (5 + len(ms['inverse on kernels']) * block):.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uv_inverse_train.txt"))
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--skip-iteration", action="store_true")
    args = ap.parse_args()
    prop = torch.cuda.get_device_properties(0)
    say(f"device: {prop.name}, {prop.multi_processor_count} CUs; torch {torch.__version__}")
    kernels()
    if not args.skip_iteration:
        iteration(args.iters, args.block)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
