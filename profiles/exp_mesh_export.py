"""Mesh export: device time of ngf_mesh_count and ngf_mesh_emit at 256^3 on (a) the dense alpha of an object-like field
(a TriPlane field whose density is a ball) and (b) a checkerboard volume, where every lattice edge carries a vertex and every cell is cut; each
beside the time its bytes would take at the achievable HBM rate (6.3 TB/s, MI355X); then the whole Base.export_mesh(256^3) and the share of it
that is getDenseAlpha.  There is no host baseline: skimage is not installed, so nothing here compares with a CPU marching cubes.

    python profiles/exp_mesh_export.py [--out profiles/mesh_export.txt] [--grid 256] [--reps 20]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ngf_amd  # noqa: E402,F401
from ngf_amd import _lib, synth  # noqa: E402
from ngf_amd.cases import field_for_case  # noqa: E402

HBM = 6.3e12      # bytes / s, achievable (float4 copy)
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
    return field_for_case(g, p, None, device=DEV)


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps      # ms


def passes(vol, level, reps, say):
    L = _lib.lib()
    n = vol.numel()
    nbytes = L.ngf_mesh_workspace_bytes(*vol.shape)
    work = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    counts = torch.empty((2,), dtype=torch.int64, device=DEV)
    dims, strides = (C.c_int32 * 3)(*vol.shape), (C.c_int64 * 3)(*vol.stride())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    org, sp = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)

    def count():
        _lib.check(L.ngf_mesh_count(vol.data_ptr(), dims, strides, C.c_float(level), work.data_ptr(), nbytes, counts.data_ptr(), stream))

    count()
    nv, nt = counts.tolist()
    verts = torch.empty((nv, 3), device=DEV)
    nrm = torch.empty((nv, 3), device=DEV)
    faces = torch.empty((nt, 3), dtype=torch.int32, device=DEV)

    def emit(flags):
        _lib.check(L.ngf_mesh_emit(vol.data_ptr(), dims, strides, C.c_float(level), org, sp, flags, work.data_ptr(), nbytes, nv, nt, verts.data_ptr(),
                                   nrm.data_ptr(), faces.data_ptr(), stream))

    blocks = (n + 255) // 256
    # bytes each pass must move once (the re-reads of neighbouring lattice points are cache traffic and not counted)
    b_count = 4 * n + 2 * n + 8 * blocks + (2 * n + 8 * blocks + 4 * n)             # count: volume in, cell words out; apply: cell words in, first-vertex out
    # emit: cell words in; the volume and the first-vertex words only where a point carries vertices or a cell triangles (taken as 8 B per vertex
    # and 4 B per face index, an estimate: neighbours share cache lines); vertices and faces out
    b_emit = 2 * n + 8 * blocks + 8 * nv + 12 * nt + 12 * nv + 12 * nt
    say(f"  {n} lattice points, workspace {nbytes / n:.3f} B per point, {nv} vertices, {nt} triangles")
    for name, fn, nbytes_moved in (("count (count + scan + apply)", count, b_count), ("emit", lambda: emit(0), b_emit),
                                   ("emit with normals", lambda: emit(_lib.MESH_NORMALS), b_emit + 12 * nv)):
        ms = timed(fn, reps)
        floor = nbytes_moved / HBM * 1e3
        say(f"  {name:30s} {ms:8.3f} ms   {nbytes_moved / 1e6:9.1f} MB   at 6.3 TB/s {floor:7.3f} ms   x{ms / floor:5.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_mesh_export.py measures on the GPU; no device found")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    G = a.grid
    say(f"mesh export at {G}^3 on {torch.cuda.get_device_name(0)} (emit includes its one stream wait for the two counts; times are device events over {a.reps} calls)")
    f = ball_field()
    alpha, _ = f.getDenseAlpha((G, G, G))
    say("dense alpha of a ball-shaped TriPlane field, level 0.005:")
    passes(alpha, 0.005, a.reps, say)
    i = torch.arange(G, device=DEV)
    checker = ((i[:, None, None] + i[None, :, None] + i[None, None, :]) % 2).float().contiguous()
    say("checkerboard volume (every edge carries a vertex, every cell is cut), level 0.5:")
    passes(checker, 0.5, max(a.reps // 4, 3), say)
    say("the dense alpha again in updateAlphaMask's [gz,gy,gx] layout (strides reversed: count classifies by 16 x 16 tiles first):")
    passes(alpha.permute(2, 1, 0).contiguous().permute(2, 1, 0), 0.005, a.reps, say)

    def whole():
        f.export_mesh(level=0.005, gridSize=(G, G, G))

    def dense():
        f.getDenseAlpha((G, G, G))

    for fn in (whole, dense):
        fn()
    torch.cuda.synchronize()
    t = {}
    for name, fn in (("export_mesh", whole), ("getDenseAlpha", dense)):
        t0 = time.perf_counter()
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        t[name] = (time.perf_counter() - t0) / 5 * 1e3
    say(f"Base.export_mesh({G}^3), host clock to synchronise: {t['export_mesh']:.2f} ms, of which getDenseAlpha (lattice points built by torch + "
        f"one alpha launch) {t['getDenseAlpha']:.2f} ms = {100 * t['getDenseAlpha'] / t['export_mesh']:.0f} %")
    say("no host baseline: skimage is not installed here, nothing was compared with a CPU marching cubes")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
