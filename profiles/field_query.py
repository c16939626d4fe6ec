"""Point queries: device time of ngf_field_query over 2^20 uniform in-box points with per-point directions -- sigma only,
sigma + rgb, sigma + rgb + coords -- on the 256^2 R1 TriPlane field at level 3 and on the InfoInv R1 field, beside the two calls the library
already had on the same points in the same process: ngf_field_alpha, and ngf_field_decode_rgb on the query's own coordinates.  Every launch is
timed by its own pair of device events; the configurations of a field alternate launch by launch and the table gives each one's median.  Then
the whole Base.export_mesh(256^3) of a ball-shaped TriPlane field (the field of profiles/exp_mesh_export.py) with and without colors=True, host
clock to synchronise.

    python profiles/field_query.py [--out profiles/field_query.txt] [--log2n 20] [--reps 30] [--grid 256]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ngf_amd  # noqa: E402,F401
from ngf_amd import _lib, synth  # noqa: E402
from ngf_amd.cases import big_case, field_for_case  # noqa: E402

DEV = "cuda:0"


def ball_field(res=256):
    g = {"model": np.array("triplane"), "aabb": np.array([[-1.5] * 3, [1.5] * 3], np.float32), "grid": np.array([256] * 3),
         "near_far": np.array([2.0, 6.0], np.float32), "step_ratio": np.float32(0.5), "distance_scale": np.float32(25), "thr": np.float32(1e-4)}
    p = synth.triplane_params(5, ((res, res),) * 3, (8, 8), preset="R0")
    u = np.linspace(-1.0, 1.0, res)
    quad = (14.0 / 3 - 20.0 * (u[None, :] ** 2 + u[:, None] ** 2) / 2).astype(np.float32)
    w = np.zeros((1, 48), np.float32)
    for k, name in enumerate(("xy", "yz", "xz")):
        p[f"plane_{name}"][0, 0] = quad
        p[f"gauge_{name}"][:] = 0
        w[0, 16 * k] = 1
    p["density_decoder.weight"] = w
    p["density_decoder.bias"] = np.zeros((1,), np.float32)
    return field_for_case(g, p, None, device=DEV, bake=True, bake_color=True)


def medians(configs, reps, warm=5):
    """{name: median ms}: every launch between its own two events, the configurations alternating."""
    for _ in range(warm):
        for _, fn in configs:
            fn()
    torch.cuda.synchronize()
    ev = {name: [] for name, _ in configs}
    for _ in range(reps):
        for name, fn in configs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            ev[name].append((a, b))
    torch.cuda.synchronize()
    return {name: statistics.median(a.elapsed_time(b) for a, b in pairs) for name, pairs in ev.items()}


def one_field(title, f, mode, n, reps, say):
    L, h = _lib.lib(), f.handle()
    gen = torch.Generator(device=DEV).manual_seed(1)
    lo, hi = f.aabb[0].to(DEV), f.aabb[1].to(DEV)
    pts = (lo + (hi - lo) * torch.rand((n, 3), device=DEV, generator=gen)).clamp(lo, hi).contiguous()
    dirs = torch.nn.functional.normalize(torch.randn((n, 3), device=DEV, generator=gen), dim=-1).contiguous()
    sig, rgb, co = torch.empty((n,), device=DEV), torch.empty((n, 3), device=DEV), torch.empty((n, 6), device=DEV)
    alpha, rgb2 = torch.empty((n,), device=DEV), torch.empty((n, 3), device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def query(s, r, c):
        return lambda: _lib.check(L.ngf_field_query(h, pts.data_ptr(), n, mode, dirs.data_ptr() if r is not None else None, 3, 0,
                                                    None if s is None else s.data_ptr(), None if r is None else r.data_ptr(),
                                                    None if c is None else c.data_ptr(), st))

    query(sig, rgb, co)()           # the coordinates ngf_field_decode_rgb is timed on
    torch.cuda.synchronize()
    configs = [("query: sigma", query(sig, None, None)),
               ("query: sigma + rgb", query(sig, rgb, None)),
               ("query: sigma + rgb + coords", query(sig, rgb, co)),
               ("ngf_field_alpha", lambda: _lib.check(L.ngf_field_alpha(h, pts.data_ptr(), n, mode, C.c_float(float(f.stepSize)), alpha.data_ptr(), st))),
               ("ngf_field_decode_rgb (query's coords)", lambda: _lib.check(L.ngf_field_decode_rgb(h, co.data_ptr(), dirs.data_ptr(), n, mode, rgb2.data_ptr(), st)))]
    t = medians(configs, reps)
    torch.cuda.synchronize()
    same = torch.equal(rgb.view(torch.int32), rgb2.view(torch.int32))
    say(f"{title}: {n} in-box points, median of {reps} launches each (ms; Mpoint/s)")
    for name, _ in configs:
        say(f"  {name:40s} {t[name]:8.3f} ms   {n / t[name] / 1e3:9.1f}")
    two = t["ngf_field_alpha"] + t["ngf_field_decode_rgb (query's coords)"]
    say(f"  {'alpha + decode_rgb, the two calls':40s} {two:8.3f} ms   -> sigma + rgb in one query is x{t['query: sigma + rgb'] / two:.2f} of that"
        f" (decode_rgb's colours are the query's bits: {same})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--grid", type=int, default=256)
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("field_query.py: the table is a median of at least 20 launches")
    if not torch.cuda.is_available():
        raise SystemExit("field_query.py measures on the GPU; no device found")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n = 1 << a.log2n
    say(f"point queries on {torch.cuda.get_device_name(0)} (device events around every launch)")
    g, params, _ = big_case("triplane", "R1")
    one_field("TriPlane R1, 256^2 planes, level 3", field_for_case(g, params, None, device=DEV, bake=True, bake_color=True), 1, n, a.reps, say)
    g, params, _ = big_case("infoinv", "R1")
    one_field("InfoInv R1, 256^2 planes", field_for_case(g, params, None, device=DEV), 1, n, a.reps, say)

    f, G = ball_field(), a.grid
    runs = {"export_mesh": lambda: f.export_mesh(level=0.005, gridSize=(G, G, G)),
            "export_mesh(colors=True)": lambda: f.export_mesh(level=0.005, gridSize=(G, G, G), colors=True)}
    nv = int(runs["export_mesh(colors=True)"]()[0].shape[0])
    t = {k: [] for k in runs}
    for _ in range(2):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    for _ in range(7):
        for k, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[k].append((time.perf_counter() - t0) * 1e3)
    m = {k: statistics.median(v) for k, v in t.items()}
    say(f"Base.export_mesh({G}^3) of a ball-shaped TriPlane field at level 3, {nv} vertices, host clock to synchronise, median of 7 alternating calls:")
    say(f"  without colours {m['export_mesh']:.2f} ms, with colors=True {m['export_mesh(colors=True)']:.2f} ms "
        f"(+{m['export_mesh(colors=True)'] - m['export_mesh']:.2f} ms: the normals, one query of {nv} points, to_uint8)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
