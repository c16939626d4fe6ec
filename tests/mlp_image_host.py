"""The CPU harness of the MLP image builders (csrc/ngf_mlp_image.hpp): synthetic weights, the stand-alone program tests/host/mlp_image_main.cpp
compiled with the host compiler, and what it wrote.  Shared by tests/test_mlp_image_cpu.py and tests/golden/make_golden_mlp_images.py."""
import os
import shutil
import subprocess

import numpy as np

import ngf_amd  # noqa: F401
from ngf_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-gauge-fields_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "host", "mlp_image_main.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "mlp_images.npz")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g"]
CONFIGS = ("tri_fp32", "tri_bake", "tri_bake_bf16", "tri_bf16", "tri_nofold", "ii_fp32", "ii_bf16")

# (name, shape) in the order the program reads them; F = 144 (TriPlane) / 216 (InfoInv), the only sizes ngf_field_create accepts
TENSORS = {
    "tri": (("basis", (144, 144)), ("w1p", (64, 144)), ("w1", (64, 159)), ("b1", (64,)), ("w2", (64, 64)), ("b2", (64,)), ("w3", (3, 64)), ("b3", (3,)),
            ("dw1", (48,)), ("db1", (1,))),
    "ii": (("w1p", (64, 216)), ("w1", (64, 231)), ("b1", (64,)), ("w2", (64, 64)), ("b2", (64,)), ("w3", (3, 64)), ("b3", (3,)),
           ("dw1", (32, 72)), ("db1", (32,)), ("dw2", (32, 32)), ("db2", (32,)), ("dw3", (32,)), ("db3", (1,))),
}
# bit patterns that exercise the bf16 rounding of the 3-term split: a tie that rounds down to even and one that rounds up to even, a carry into the
# exponent, a value whose mid and lo parts are zero (1.5), two fp32 denormals, negative zero
SPECIALS = np.array([0x3F808000, 0x3F818000, 0x3FFFFFFF, 0x3FC00000, 0x00012345, 0x80400000, 0x80000000], dtype=np.uint32).view(np.float32)


def _distinct(seed, n):
    """n finite float32 values, no two equal: |v| in slot i of n disjoint intervals of [0.25, 1.25), slots and signs from the hash generators."""
    slot = np.empty(n, dtype=np.int64)
    slot[np.argsort(synth.hash_uniform(seed, 1, (n,)), kind="stable")] = np.arange(n)
    mag = 0.25 + (slot + 0.5 * synth.hash_uniform(seed, 0, (n,)).astype(np.float64)) / n
    v = (np.where(synth.hash_uniform(seed, 2, (n,)) < 0.5, -mag, mag)).astype(np.float32)
    assert np.isfinite(v).all() and np.unique(v).size == n
    return v


def weights():
    """{model: {name: float32 array}}.  w1p is just another random [64][F] array: the builders only place it."""
    out = {}
    for seed, (model, tensors) in enumerate(TENSORS.items(), start=1):
        flat = _distinct(seed, sum(int(np.prod(s)) for _, s in tensors))
        at, W = 0, {}
        for name, shape in tensors:
            n = int(np.prod(shape))
            W[name] = flat[at:at + n].reshape(shape).copy()
            at += n
        F = W["w1p"].shape[1]
        k = SPECIALS.size
        # every matrix that is split: a run in the plane part, one across the view columns (entries 8..14 of the 15), one in layer 2
        W["w1p"][3, 5:5 + k] = SPECIALS
        W["w1"][7, F + 8:F + 8 + k] = SPECIALS
        W["w1"][9, 2:2 + k] = SPECIALS
        W["w2"][11, 30:30 + k] = SPECIALS
        if model == "ii":
            W["dw1"][5, 64:64 + k] = SPECIALS
            W["dw2"][6, 10:10 + k] = SPECIALS
        out[model] = W
    return out


def weights_bytes():
    W = weights()
    return b"".join(W[m][name].astype("<f4").tobytes() for m, tensors in TENSORS.items() for name, _ in tensors)


def compiler():
    for cxx in ("g++", "/opt/rocm/llvm/bin/clang++", "clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    raise RuntimeError("no host C++ compiler (g++ or clang++) found")


def _links_and_runs(cxx, flags, workdir):
    src, exe = os.path.join(workdir, "probe.cpp"), os.path.join(workdir, "probe")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    if subprocess.run([cxx, *flags, src, "-o", exe], capture_output=True).returncode != 0:
        return False
    return subprocess.run([exe], capture_output=True).returncode == 0


def compile_program(workdir, flags=None, source=SOURCE):
    """Compiles the stand-alone program ``source`` (tests/host/*.cpp) into workdir; returns (path, flags used).  flags = None: the sanitizer
    build, or -- only where a one-line probe with those flags does not link and run on this machine -- the same without sanitizers."""
    cxx = compiler()
    if flags is None:
        flags = SANITIZE if _links_and_runs(cxx, SANITIZE, workdir) else ["-O1", "-g"]
    exe = os.path.join(workdir, os.path.splitext(os.path.basename(source))[0])
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, source, "-o", exe], check=True)
    return exe, flags


def run_program(exe, workdir, time_reps=0):
    """Runs the program on weights_bytes(); returns ({name.img / name.pack: uint32 words}, {config: [(section, offset, count)]}, {config: best us})."""
    wpath, outdir = os.path.join(workdir, "weights.f32"), os.path.join(workdir, "out")
    os.makedirs(outdir, exist_ok=True)
    with open(wpath, "wb") as f:
        f.write(weights_bytes())
    r = subprocess.run([exe, wpath, outdir] + (["--time", str(time_reps)] if time_reps else []), capture_output=True, text=True)
    assert r.returncode == 0, f"{exe} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}"
    sections, times = {c: [] for c in CONFIGS}, {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "section":
            sections[w[1]].append((w[2], int(w[3]), int(w[4])))
        elif w[0] == "time":
            times[w[1]] = float(w[2])
    words = {fn: np.fromfile(os.path.join(outdir, fn), dtype="<u4") for fn in sorted(os.listdir(outdir))}
    return words, sections, times
