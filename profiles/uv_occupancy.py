"""NeuTex occupancy grid on one GPU: what the render kernel costs with and without a mask, on the UV frame of bench.py (DTU camera 0 of the
800 x 600 frame, the 96 rows through the object = 76 800 rays, S = 64, synth.uvmapping_params(5, "sphere")), for the fp32 and the split-bf16 kernel.

    python profiles/uv_occupancy.py [--rounds 7] [--parent-lib PATH] [--out profiles/uv_occupancy.txt]

Four conditions, timed ALTERNATELY (one launch of each per round, `rounds` rounds, after a second of the workload to ramp the clocks and one
warm launch of each): no mask; an all-ones 128^3 mask (the look-up's own cost); a hand-made ball that fills 8 % of the cube (the object in empty
space); build_occupancy(128) at the lattice's median sigma (the synthetic weights give a density that is noise at the lattice's scale: half the
corners are hot, so nearly every cell is -- this condition shows the build and the install, not a saving).  A launch is timed between two device events; figures are medians (min .. max), and the spread of the no-mask
launches is the yardstick for every difference.  `stats` are the kernel's counters: samples evaluated, 16-sample passes run; the pass fill is
samples / (16 passes).  --parent-lib: a build of the PARENT commit's libngf_hip.so; its no-mask launch (same weights, same rays, raw C ABI) joins
the rounds, so the instantiations without the look-up can be compared across the commits in one process."""
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
from ngf_amd import rays as nrays  # noqa: E402
import uv_occupancy_ref as O  # noqa: E402

S = 64


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def host_ms(fn, iters=3):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def fmt(ts):
    return f"{np.median(ts):8.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


class ParentRender:
    """The parent commit's library through the raw C ABI: ngf_uv_create on the model's tensors, ngf_uv_render_batch on the frame."""

    def __init__(self, path, net, cam, dirs, U):
        self.L = C.CDLL(os.path.abspath(path))
        self.L.ngf_uv_create.argtypes = [C.POINTER(_lib.UvDesc), C.POINTER(C.c_void_p), C.c_void_p]
        self.L.ngf_uv_destroy.argtypes = [C.c_void_p]
        self.L.ngf_uv_render_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        dev = dirs.device
        d = _lib.UvDesc()
        d.sphere, d.flags = int(net.primitive_type != "square"), _lib.UV_F_SPLIT_BF16 if net.split_bf16 else 0
        self.keep = []
        for i, lin in enumerate(net.layers()):
            w, b = lin.weight.detach().to(dev, torch.float32).contiguous(), lin.bias.detach().to(dev, torch.float32).contiguous()
            self.keep += [w, b]
            d.w[i], d.b[i] = w.data_ptr(), b.data_ptr()
        self.h = C.c_void_p()
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert self.L.ngf_uv_create(C.byref(d), C.byref(self.h), st) == 0
        self.cam, self.dirs, self.U = cam.to(dev).contiguous(), dirs.contiguous(), U.contiguous()
        n = dirs.shape[1]
        self.color, self.trans = torch.empty((1, n, 3), device=dev), torch.empty((1, n), device=dev)

    def __call__(self):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = self.L.ngf_uv_render_batch(self.h, self.cam.data_ptr(), self.dirs.data_ptr(), None, self.U.data_ptr(), 1, self.dirs.shape[1], S, self.color.data_ptr(),
                                        self.trans.data_ptr(), None, None, None, st)
        assert rc == 0

    def close(self):
        self.L.ngf_uv_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uv_occupancy.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("uv_occupancy.py measures on the GPU; no device found")
    dev = "cuda:0"
    v0 = synth.DTU_VIEW0
    dirs = nrays.generate_rays_dtu(600, 800, v0["focal"], v0["princpt"], v0["rot"], rows=(252, 348), device=dev)[None]
    cam = torch.tensor(v0["campos"], dtype=torch.float32)[None]
    n = dirs.shape[1]
    U = torch.from_numpy(synth.hash_uniform(5, 77, (1, n, S))).to(dev)
    params = synth.uvmapping_params(5, "sphere")
    ball = O.ball_mask((128, 128, 128))
    lines = [f"# NeuTex occupancy grid on {torch.cuda.get_device_name(0)}: {n} rays x {S} samples (bench.py's UV frame), one launch per condition and round, "
             f"{a.rounds} rounds alternating, device events; median (min .. max)",
             f"# ball mask: {100 * ball.mean():.2f} % of the 128^3 cells"]
    for split in (False, True):
        net = uvmapping.NeuTex(primitive_type="sphere", sample_num=S, device=dev, split_bf16=split)
        net.load_params(params)
        render = lambda **kw: net(cam, dirs, None, jitter_u=U, **kw)          # noqa: E731
        t_end = time.perf_counter() + 1.0
        while time.perf_counter() < t_end:          # ramp the clocks with the workload itself
            render()
            torch.cuda.synchronize()
        # build_occupancy(128) at the lattice's median, and its two parts
        cells = (128, 128, 128)
        step = (np.float32(2.0) / np.asarray(cells, np.float32)).astype(np.float32)
        lattice = lambda: net._lattice((129, 129, 129), np.full(3, -1.0, np.float32), step, clip=False)          # noqa: E731
        sigma = lattice()
        thr = float(sigma.median())
        t_lat = host_ms(lattice)
        t_red = host_ms(lambda: net._occupancy_reduce(sigma, cells, thr, 1))
        t_all = host_ms(lambda: net.build_occupancy(128, threshold=thr, dilate=1))
        built = net.build_occupancy(128, threshold=thr, dilate=1)
        built_pair, built_frac = (built.bits.clone(), built.shape), built.fraction()
        conds = [("no mask", None), ("all-ones 128^3", np.ones(cells, bool)), ("ball, 8 % of the cube", ball), (f"build_occupancy(128) at the median sigma {thr:.4f}", built_pair)]
        parent = ParentRender(a.parent_lib, net, cam, dirs, U) if a.parent_lib else None
        frames, stats, times = {}, {}, {c[0]: [] for c in conds}
        t_parent = []
        for r in range(-1, a.rounds):          # round -1: the warm launches, the frames and the counters
            for name, mask in conds:
                net.set_occupancy(mask)
                if r < 0:
                    out = render(collect_stats=True)
                    frames[name], stats[name] = out["color"].clone(), tuple(int(x) for x in net.last_stats[:2].cpu())
                else:
                    times[name].append(timed(render))
            if parent is not None:
                parent() if r < 0 else t_parent.append(timed(parent))
        net.set_occupancy(None)
        base = float(np.median(times["no mask"]))
        spread = (max(times["no mask"]) - min(times["no mask"])) / base
        lines.append(f"{'split-bf16' if split else 'fp32'} kernel   (run-to-run spread of the no-mask launches: {100 * spread:.2f} % of their median)")
        for name, _ in conds:
            smp, pas = stats[name]
            fill = smp / (16.0 * pas) if pas else 0.0
            lines.append(f"  {name:<52s} {fmt(times[name])}  x{np.median(times[name]) / base:5.3f} of no mask   {n / np.median(times[name]) / 1e3:7.3f} Mray/s   "
                         f"samples {smp:>9d}  passes {pas:>8d}  pass fill {fill:.3f}")
        if parent is not None:
            lines.append(f"  {'no mask, the parent commit library':<52s} {fmt(t_parent)}  x{np.median(t_parent) / base:5.3f} of no mask")
            same = torch.equal(parent.color, frames["no mask"])
            lines.append(f"    the parent's frame and this commit's no-mask frame: {'the same bits' if same else 'DIFFERENT bits'}")
            parent.close()
        mse = float(((frames[conds[3][0]] - frames["no mask"]).double() ** 2).mean())
        psnr = float("inf") if mse == 0 else -10.0 * np.log10(mse)
        lines.append(f"  all-ones frame == no-mask frame: {torch.equal(frames['all-ones 128^3'], frames['no mask'])};  PSNR of the build_occupancy frame against the no-mask frame: {psnr:.2f} dB "
                     f"(occupied {100 * built_frac:.1f} % of the cells: the synthetic density is noise at the scale of a cell, so nearly every cell has a corner above the median)")
        lines.append(f"  build_occupancy(128): {t_all:.2f} ms = lattice 129^3 {t_lat:.2f} ms + reduction {t_red:.3f} ms (+ install), host clock around a synchronise, median of 3")
        net.release()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
