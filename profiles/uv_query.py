"""UV-Mapping (NeuTex) point queries and the UV-textured mesh export on one GPU: NeuTex.density_lattice / query / export_mesh through the HIP
kernels (ngf_uv_density_lattice, ngf_uv_query) against eager fp32 torch running the same nn modules on the same GPU, the same points, in the same
process (tests/uv_query_eager.py).  Clocks are ramped with a second of the workload itself; a kernel is timed between two device events, eager
torch and the mesh steps with a host clock around a device synchronise; every figure is a median.

    python profiles/uv_query.py [--iters 9] [--out profiles/uv_query.txt]

The floor of a launch is 2 x MACs over the fp32 matrix peak (157.3 TFLOP/s: 256 CUs x 256 FLOP/clk x 2.4 GHz); `of peak` is that floor over the
measured time.  The yardstick is the texture export's kernel (profiles/uv_export.txt: 0.89 of the peak), built from the same blocks."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ngf_amd  # noqa: E402,F401
from ngf_amd import evalout, mesh, synth  # noqa: E402
import uv_export_eager as E  # noqa: E402
import uv_query_eager as Q  # noqa: E402

PEAK = 157.3e12
GEO = 63 * 256 + 10 * 256 * 256 + 256


def macs(prim, want, diffuse=False):
    D = 3 if prim == "sphere" else 2
    m = GEO if "sigma" in want else 0
    if "uv" in want or "rgb" in want:
        m += 63 * 64 + 64 * 128 + 2 * 128 * 128 + 128 * D
    if "rgb" in want:
        block1 = 21 * D * 256 + 5 * 256 * 256 + 256 * 3
        m += block1 if diffuse else block1 + 295 * 256 + 3 * 256 * 256 + 256 * 3
    return m


def device_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def host_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), out


@torch.no_grad()
def eager(net, pts, view, want, diffuse=False, chunk=1 << 19):
    """The same networks in eager fp32 torch on the device, 2^19 points at a time (the activations of more do not fit comfortably)."""
    out = []
    for i in range(0, pts.shape[0], chunk):
        p = pts[i:i + chunk]
        r = []
        if "sigma" in want:
            r.append(Q.density(net, p))
        if "uv" in want or "rgb" in want:
            uv = Q.gauge(net, p)
            r.append(uv)
            if "rgb" in want:
                r.append(E.texture_forward(net.net_texture, uv, None if diffuse else view[i:i + chunk]))
        out.append(r)
    return out


def line(label, ms, lo, hi, n, m, eager_ms=None):
    s = f"  {label:<44s} {ms:9.3f} ms ({lo:.3f} .. {hi:.3f})  {2 * m * n / (ms * 1e-3) / 1e12:6.1f} TFLOP/s  {2 * m * n / PEAK / (ms * 1e-3):5.2f} of peak"
    if eager_ms is not None:
        s += f"   eager torch {eager_ms:9.2f} ms (x{eager_ms / ms:.1f})"
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uv_query.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("uv_query.py measures on the GPU; no device found")
    dev = "cuda:0"
    lines = [f"# NeuTex point queries on {torch.cuda.get_device_name(0)}; kernel ms are medians of {a.iters} launches between device events (min .. max); "
             f"eager torch: fp32 modules, same device, same points, host clock around a synchronise, median of 3"]
    for prim in ("sphere", "square"):
        net = Q.make_net(prim, dev)
        t_end = time.perf_counter() + 1.0
        while time.perf_counter() < t_end:                      # ramp the clocks with the workload itself
            net.density_lattice(128)
            torch.cuda.synchronize()
        lines.append(f"{prim} model")
        for R in ((128, 256) if prim == "sphere" else (128,)):          # (the geometry network does not know the primitive: 256^3 once)
            ms, lo, hi = device_ms(lambda: net.density_lattice(R), a.iters if R < 200 else max(3, a.iters // 3))
            vol, lo32, step = net.density_lattice(R)
            pts = torch.from_numpy(Q.lattice_points(lo32, step, (R, R, R)).reshape(-1, 3)).to(dev)
            e_ms, _ = host_ms(lambda: eager(net, pts, None, ("sigma",)), 3 if R < 200 else 1)
            lines.append(line(f"density_lattice({R}): {R ** 3} points", ms, lo, hi, R ** 3, GEO, e_ms))
            del pts, vol
        n = 1 << 20
        xyz = torch.from_numpy((synth.hash_uniform(7, 1, (n, 3)) * np.float32(2) - np.float32(1))).to(dev)
        v = synth.hash_normal(7, 2, (n, 3)).astype(np.float64)
        view = torch.from_numpy((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)).to(dev)
        for want, diffuse in ((("sigma",), False), (("uv",), False), (("sigma", "uv"), False), (("uv", "rgb"), False), (("uv", "rgb"), True),
                              (("sigma", "uv", "rgb"), False), (("sigma", "uv", "rgb"), True)):
            ms, lo, hi = device_ms(lambda: net.query(xyz, view, want=want, diffuse=diffuse), a.iters)
            e_ms, _ = host_ms(lambda: eager(net, xyz, view, want, diffuse), 3)
            lines.append(line(f"query 2^20: {' + '.join(want)}{' (diffuse)' if diffuse else ''}", ms, lo, hi, n, macs(prim, want, diffuse), e_ms))
        # export_mesh(256, texture_resolution=512), step by step as export_mesh runs them.  The synthetic weights give a density that is noise at
        # the lattice's scale, so the level is set where about 1 lattice point in 200 lies above it: a mesh of a size a trained model gives.
        R, TR = 256, 512
        vol, lo32, step = net.density_lattice(R)
        level = float(torch.quantile(vol.reshape(-1)[::97].contiguous(), 0.995))
        t_lat, (vol, lo32, step) = host_ms(lambda: net.density_lattice(R), 3)
        t_mc, (verts, faces) = host_ms(lambda: mesh.marching_cubes(vol, level, spacing=step.tolist(), origin=lo32.tolist()), 3)
        t_uv, uv = host_ms(lambda: net.query(verts, want=("uv",))["uv"], 3)
        sphere = prim == "sphere"
        t_st, st = host_ms(lambda: mesh.atlas_coords(uv, prim, TR if sphere else None), 3)

        def atlas():
            tex = net.net_texture._export_sphere(TR, None) if sphere else net.net_texture._export_square(TR, None)
            return evalout.to_uint8((tex ** (1 / 2.2)).clamp(0, 1).contiguous()).cpu().numpy()

        t_tex, image = host_ms(atlas, 3)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "m.obj")
            t0 = time.perf_counter()
            st_file, fvt = mesh.unwrap_seam(faces, st) if sphere else (st, None)
            mesh.write_obj(path, verts, faces, st_file, fvt, texture=image)
            t_file = (time.perf_counter() - t0) * 1e3
            size = sum(os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp))
            t0 = time.perf_counter()
            net.export_mesh(path, level=level, resolution=R, texture_resolution=TR)
            torch.cuda.synchronize()
            t_all = (time.perf_counter() - t0) * 1e3
        lines.append(f"  export_mesh(256, texture_resolution=512) at level {level:.4f}: {verts.shape[0]} vertices, {faces.shape[0]} triangles, files {size / 1e6:.1f} MB")
        lines.append(f"    lattice {t_lat:.2f} ms | marching cubes {t_mc:.2f} ms | vertex uv {t_uv:.3f} ms | atlas_coords {t_st:.3f} ms | atlas image {t_tex:.2f} ms | "
                     f"seam + files (host) {t_file:.1f} ms | the whole call {t_all:.1f} ms")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
