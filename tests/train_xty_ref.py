"""The cases, inputs, float64 references and error bounds of the TriPlane trainer's weight-gradient products (ngf_debug_train_xty, include/ngf.h:
one launch of xty_all_kernel through the step's own set-up code), in numpy only: tests/test_gpu_train_xty.py runs them on the GPU,
tests/test_triplane_train_edges_cpu.py checks on the CPU that the bound can see a defect.

A case is a dict: the static row count `rows` (as a function of G = 2 x the device's CU count, the cap of the grid), the optional device row
count `dev` (min(rows, dev) rows are summed) and `cancel` (the rows come in pairs +x, -x against one y: every product sums to exactly zero).
The operands are sample-major: D1 [rows][64], D2 [rows][64], D3 [rows][16], F [rows][144], H1 [rows][64], H2 [rows][64], V [rows][16].

The bounds are derived, not measured.  With u = 2^-24 and gamma_n = n u / (1 - n u), a sum of fp32 products taken along any tree of depth n
satisfies |s - s64| <= gamma_n sum |x| |y| (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  With m = min(rows, dev) rows
in ceil(m / 32) k-chunks and W = min(ceil(rows / 32), G) workgroups, a workgroup sums at most 32 ceil(chunks / W) products into its accumulators
(in the matrix unit's order) and the W workgroups add their sums to the output one after the other (float atomics, any order) on top of what it
held: a depth of 32 ceil(chunks / W) + min(W, chunks) + 1, over sum |x| |y| + |previous|."""
import numpy as np

from ngf_amd import synth

U = 2.0 ** -24
CH = 32                                          # rows per k-chunk of xty_block
SENTINEL = 0x7FC5A5A5                            # the bits of every word behind a buffer (a NaN that no kernel computes)
# operand -> (columns of the buffer, columns that hold data)
OPERANDS = {"D1": (64, 64), "D2": (64, 64), "D3": (16, 3), "F": (144, 144), "H1": (64, 64), "H2": (64, 64), "V": (16, 15)}
# output -> (delta operand, input operand); gW1: the 15 view columns 144..158 of the [64][159] tensor
PRODUCTS = {"M": ("D1", "F"), "gW2": ("D2", "H1"), "gW1": ("D1", "V"), "gW3": ("D3", "H2")}
OUT_SHAPES = {"M": (64, 144), "gW2": (64, 64), "gW1": (64, 15), "gW3": (3, 64)}
SURPLUS = 3                                      # NaN rows behind the last row of every operand

ROWS = (("1", lambda G: 1), ("31", lambda G: 31), ("32", lambda G: 32), ("33", lambda G: 33), ("63", lambda G: 63), ("64", lambda G: 64),
        ("65", lambda G: 65), ("32G-1", lambda G: 32 * G - 1), ("32G", lambda G: 32 * G), ("32G+1", lambda G: 32 * G + 1),
        ("32G+33", lambda G: 32 * G + 33), ("64G+1", lambda G: 64 * G + 1))
DEV_ROWS = ("32G+33", lambda G: 32 * G + 33)     # the launch of the rows_dev cases: a second lap of one workgroup
DEV = (("0", lambda r: 0), ("1", lambda r: 1), ("17", lambda r: 17), ("rows", lambda r: r), ("above", lambda r: r + 5))


def gamma(n):
    return n * U / (1.0 - n * U)


def names():
    """the case ids, which do not depend on the device"""
    return [f"r{n}" for n, _ in ROWS] + [f"r{DEV_ROWS[0]}-dev{n}" for n, _ in DEV] + ["r32G-cancel"]


def cases(G):
    c = [{"id": f"r{n}", "rows": fn(G), "dev": None, "cancel": False} for n, fn in ROWS]
    r = DEV_ROWS[1](G)
    c += [{"id": f"r{DEV_ROWS[0]}-dev{n}", "rows": r, "dev": fn(r), "cancel": False} for n, fn in DEV]
    c.append({"id": "r32G-cancel", "rows": 32 * G, "dev": None, "cancel": True})
    for i, k in enumerate(c):
        k["seed"], k["G"] = 9000 + i, G
    assert [k["id"] for k in c] == names()
    return c


def eff_rows(c):
    return c["rows"] if c["dev"] is None else min(c["rows"], c["dev"])


def depth(c):
    m = eff_rows(c)
    chunks, W = -(-m // CH), min(-(-c["rows"] // CH), c["G"])
    return CH * -(-chunks // W) + min(W, chunks) + 1


def inputs(c):
    """float32 operands [rows + SURPLUS][columns]: unit normals in the data columns; NaN in the rows from min(rows, dev) on, and in column 15 of
    D3 and V (the layout's pad); zeros in columns 3..14 of D3, as the colour backward writes them.  prev_*: the known contents of the outputs
    (gW1: of the 15 view columns)."""
    s, m, n = c["seed"], eff_rows(c), c["rows"] + SURPLUS
    d = {}
    for i, (k, (cols, used)) in enumerate(OPERANDS.items()):
        a = np.zeros((n, cols), np.float32)
        a[:, :used] = synth.hash_normal(s, 1 + i, (n, used))
        if c["cancel"] and k.startswith("D"):
            a[1:m:2] = -a[0:m - 1:2]
        if c["cancel"] and not k.startswith("D"):
            a[1:m:2] = a[0:m - 1:2]
        a[m:] = np.nan
        d[k] = a
    d["D3"][:, 15] = np.nan
    d["V"][:, 15] = np.nan
    for i, (k, shape) in enumerate(OUT_SHAPES.items()):
        d["prev_" + k] = (synth.hash_normal(s, 20 + i, shape) * np.float32(3)).astype(np.float32)
    return d


def reference(c, d, drop_row=False):
    """{output: (float64 value, bound)} on top of d["prev_*"].  drop_row: the sum without its last row (the defect the CPU test shows the bound
    can see)."""
    m = eff_rows(c)
    K = max(m - (1 if drop_row else 0), 0)
    g = gamma(depth(c))
    out = {}
    for k, (x, y) in PRODUCTS.items():
        mo, no = OUT_SHAPES[k]
        X, Y = np.asarray(d[x][:K, :mo], np.float64), np.asarray(d[y][:K, :no], np.float64)
        p = np.asarray(d["prev_" + k], np.float64)
        out[k] = (p + X.T @ Y, g * (np.abs(X).T @ np.abs(Y) + np.abs(p)) if m > 0 else np.zeros_like(p))
    return out
