"""The cases, inputs, float64 references and error bounds of the InfoInv trainer's weight-gradient products (ngf_debug_ii_product, include/ngf.h),
in numpy only: tests/test_gpu_ii_product.py runs them on the GPU, tests/test_infoinv_train_edges_cpu.py checks on the CPU that the bound can see
a defect.

A case is a dict: form "mfma" (ii_mm_kernel + ii_mm_reduce_kernel, the fused step) or "fp64" (ii_xty_kernel + ii_xty_reduce_kernel, the autograd
path), the widths M (delta rows) and N (input rows), the static row count `rows`, the optional device row count `dev` (min(rows, dev) rows are
summed) and the leading dimension ld = rows + 3.  X is [M][ld], Y is [N][ld]: the summed index is the fast one.

The bounds are derived, not measured.  With u = 2^-24 and gamma_n = n u / (1 - n u), any order of summing n fp32 products satisfies
|s - s64| <= gamma_n sum |x| |y| (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  m = min(rows, dev) rows:
  mfma  gw    gamma_(min(m, 1024) + 4) (|X|^T |Y|) + u |C64|: an fp32 sum of at most kIiMmSub = 1024 products in any order (+ 4 of slack for the
              fp64 adds of the sub-sums and of the chunks, each 2^-53 relative), then one rounding to float
        gw64  the same without the rounding to float
        gb    gamma_(nz + 1) sum |X|, nz = ceil(m / 8192) chunks: fp64 sums, one rounding to float
        accumulate  out = fl(previous + fl(s)): one more rounding, u (|previous| + |C64|) (1 + 2^-20) (gw64: 2^-53 in place of u)
  fp64  gw, gb  u |C64| + m 2^-53 (|X|^T |Y|): the product of two floats is exact in fp64, m fp64 adds, one rounding to float
        gw64  m 2^-53 (|X|^T |Y|)
With m = 0: exactly +0 without `accumulate` and bit-unchanged contents with it (tests/test_gpu_ii_product.py asserts the bits)."""
import numpy as np

from ngf_amd import synth

U = 2.0 ** -24
U64 = 2.0 ** -53
MM_K, MM_SUB, MM_CHUNK = 32, 1024, 8192          # kIiMmK, kIiMmSub, kIiMmChunk (ngf_infoinv_fused.hpp)
XTY_STAGE, XTY_CHUNK = 64, 4096                  # the LDS stage and kIiChunk (ngf_infoinv_train.hpp)
SENTINEL = 0x7FC5A5A5                            # the bits of every output word before a call (a NaN that no kernel computes)
SENTINEL64 = (SENTINEL << 32) | SENTINEL

SHAPES = [(32, 72), (32, 32), (1, 32), (64, 231), (64, 64), (3, 64)]          # the trainer's six products (M, N)
NARROW, WIDE, MID = [(1, 32), (3, 64)], (64, 231), [(32, 72), (32, 32), (64, 64)]
ROWS = [1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 16385]
DEV = (8193, [0, 1, 33, 8192, 8193, 20000])
FORMS = ("mfma", "fp64")

# case index -> input seed, where the unit normals of 7000 + index could not show a dropped last row (tests/test_infoinv_train_edges_cpu.py).
# The risk is M = 1 at thousands of rows: the last row contributes x[0][m - 1] * y[:][m - 1] alone, against an mfma bound of gamma_1028 times a
# sum of m products.  At the seeds below every case shows it, so the table is empty.
RESEED = {}


def gamma(n):
    return n * U / (1.0 - n * U)


def _case(form, shape, rows, dev=None):
    return {"form": form, "M": shape[0], "N": shape[1], "rows": rows, "dev": dev, "ld": rows + 3}


def cases():
    """Every row count occurs with a 1- or 3-wide M and with (64, 231), in both forms; the other three shapes take turns
    (tests/test_infoinv_train_edges_cpu.py asserts the coverage)."""
    c = []
    for form in FORMS:
        for i, r in enumerate(ROWS):
            c.append(_case(form, NARROW[i % 2], r))
            c.append(_case(form, WIDE, r))
            c.append(_case(form, MID[i % 3], r))
        for i, d in enumerate(DEV[1]):
            shape = SHAPES[(i + (0 if form == "mfma" else 3)) % 6]
            c.append(_case(form, shape, DEV[0], dev=d))
            if shape != WIDE and d in (0, 20000):          # no rows, and a count above the launch: on the widest product too
                c.append(_case(form, WIDE, DEV[0], dev=d))
    for i, k in enumerate(c):
        k["seed"] = RESEED.get(i, 7000 + i)
        k["id"] = "{}-{}".format(i, case_name(k))
    return c


def case_name(c):
    return "{form}-m{M}-n{N}-r{rows}".format(**c) + ("" if c["dev"] is None else "-dev{}".format(c["dev"]))


def eff_rows(c):
    return c["rows"] if c["dev"] is None else min(c["rows"], c["dev"])


def n_chunks(c, rows=None):
    """chunks of the launch (the scratch the entry asks for) or, with `rows`, the chunks that hold rows"""
    per = MM_CHUNK if c["form"] == "mfma" else XTY_CHUNK
    return ((c["rows"] if rows is None else rows) + per - 1) // per


def scratch_elems(c):
    """(doubles of part, doubles of partb) the launch needs"""
    nz = n_chunks(c)
    return (nz * c["M"] * c["N"], nz * c["M"]) if c["form"] == "mfma" else (nz * c["M"] * (c["N"] + 1), 0)


def inputs(c):
    """float32 x [M, ld], y [N, ld]: unit normals; the rows from min(rows, dev) on and the padding up to ld are NaN, so a kernel that
    reads them shows it.  prev_*: the known contents the `accumulate` run starts from."""
    s, m = c["seed"], eff_rows(c)
    x = synth.hash_normal(s, 1, (c["M"], c["ld"])).astype(np.float32)
    y = synth.hash_normal(s, 2, (c["N"], c["ld"])).astype(np.float32)
    x[:, m:] = np.nan
    y[:, m:] = np.nan
    return {"x": x, "y": y,
            "prev_gw": (synth.hash_normal(s, 3, (c["M"], c["N"])) * np.float32(3)).astype(np.float32),
            "prev_gb": (synth.hash_normal(s, 4, (c["M"],)) * np.float32(3)).astype(np.float32),
            "prev_gw64": (synth.hash_normal(s, 5, (c["M"], c["N"])).astype(np.float64) * 3.0 + 2.0 ** -30)}


def reference(c, d, drop_row=False, accumulate=False):
    """{output name: (float64 value, bound)} of gw [M, N], gw64 [M, N] and gb [M].  drop_row: the sum without its last row (the defect the CPU
    test shows the bound can see).  accumulate (mfma): on top of d["prev_*"]."""
    m = eff_rows(c)
    K = max(m - (1 if drop_row else 0), 0)
    X, Y = np.asarray(d["x"][:, :K], np.float64), np.asarray(d["y"][:, :K], np.float64)
    C, A = X @ Y.T, np.abs(X) @ np.abs(Y).T
    B, Ab = X.sum(1), np.abs(X).sum(1)
    if c["form"] == "mfma":
        g = gamma(min(m, MM_SUB) + 4)
        out = {"gw": (C, g * A + U * np.abs(C)), "gw64": (C, g * A), "gb": (B, gamma(n_chunks(c, m) + 1) * Ab)}
        if accumulate:
            slack = 1.0 + 2.0 ** -20
            for k, u in (("gw", U), ("gw64", U64), ("gb", U)):
                p = np.asarray(d["prev_" + k], np.float64)
                v, b = out[k]
                out[k] = (p + v, b + u * slack * (np.abs(p) + np.abs(v) + b))          # + b: the sum that is added is itself off by b
        return out
    assert not accumulate
    return {"gw": (C, U * np.abs(C) + m * U64 * A), "gw64": (C, m * U64 * A), "gb": (B, U * np.abs(B) + m * U64 * Ab)}
