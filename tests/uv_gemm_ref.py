"""The cases, inputs, float64 references and error bounds of the UV-Mapping trainer's layer GEMM (ngf_debug_uvt_gemm, include/ngf.h), in numpy
only: tests/test_gpu_uv_train_gemm.py runs them on the GPU, tests/test_uv_train_edges_cpu.py checks on the CPU that the bound can see a defect.

A case is a dict: form "fwd" (Z = act(X W^T + b)), "dx" (dX = (dZ W [+ add]) [x act'(aux)]) or "dw" (dW, db = dZ^T X over 1024-row chunks), the
layer's widths and leading dimensions, the static row count `rows` and the optional device row count `dev` (min(rows, dev) rows are computed).

The bound is derived, not measured.  With u = 2^-24 and gamma_n = n u / (1 - n u), any order of summing n fp32 products and addends satisfies
|C - C64| <= gamma_n (|A| |B| + |bias| + |add|) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1): n = K + 4 for the two
unsplit forms (K products, bias or add, the LeakyReLU factor and slack), min(K, 1024) + nz + 4 for dW (a chunk, then nz chunks), nz + 1 over
sum |dZ| for db (fp64 chunk sums rounded once, then nz chunks)."""
import numpy as np

from ngf_amd import synth

U = 2.0 ** -24
CHUNK = 1024
SLOPE = np.float32(0.2)
NONE, RELU, LEAKY = 0, 1, 2
SENTINEL = 0x7FC5A5A5            # the bits of every output word before a call (a NaN that no kernel computes)

ROWS = [1, 15, 16, 17, 63, 64, 65, 130]
FWD_K = [(63, 64), (42, 64), (295, 296), (256, 256), (128, 128)]
FWD_N = [(256, 256), (256, 296), (128, 128), (64, 64), (3, 4), (2, 4), (1, 1)]
FWD_DEV = (200, [0, 1, 65, 200, 4000])
DX_K = [(1, 1), (2, 4), (3, 4), (128, 128), (256, 256)]
DX_N = [(42, 64), (63, 64), (64, 64), (128, 128), (256, 256)]
DW_ROWS = [1, 15, 17, 1023, 1024, 1025, 2049]
DW_OUT = [(1, 1), (3, 4), (64, 64), (256, 256)]
DW_IN = [(42, 64), (63, 64), (295, 296), (256, 256)]
DW_DEV = (2049, [0, 1, 1024, 1025])


# case index -> input seed, where the unit normals of 9000 + index cannot show a defect (tests/test_uv_train_edges_cpu.py): ReLU leaves the
# whole last row of case 2 (two units wide) at zero, so a missing row would equal the reference
RESEED = {2: 9502}


def gamma(n):
    return n * U / (1.0 - n * U)


def _fwd(K, N, rows, act, dev=None):
    return {"form": "fwd", "in": K[0], "ld_x": K[1], "out": N[0], "ld_z": N[1], "rows": rows, "dev": dev, "act": act}


def _dx(K, N, rows, act, add, dev=None, inn=None):
    inn = inn or N
    return {"form": "dx", "out": K[0], "ld_z": K[1], "n_dx": N[0], "ld_dx": N[1], "in": inn[0], "ld_x": inn[1], "rows": rows, "dev": dev,
            "act": act, "add": bool(add)}


def _dw(out, inn, rows, dev=None):
    return {"form": "dw", "out": out[0], "ld_z": out[1], "in": inn[0], "ld_x": inn[1], "rows": rows, "dev": dev}


def cases():
    """Every listed value of every axis occurs, and every row count occurs with a 1- to 3-wide side and with a 256-wide side
    (tests/test_uv_train_edges_cpu.py asserts both)."""
    c = []
    narrow, wide, mid = FWD_N[4:], FWD_N[:2], FWD_N[2:4]
    for i, r in enumerate(ROWS):
        c.append(_fwd(FWD_K[i % 5], narrow[i % 3], r, i % 3))
        c.append(_fwd(FWD_K[(i + 2) % 5], wide[i % 2], r, (i + 1) % 3))
    for i, r in enumerate([17, 65, 130, 1]):
        c.append(_fwd(FWD_K[(i + 4) % 5], mid[i % 2], r, (i + 2) % 3))
    for i, d in enumerate(FWD_DEV[1]):
        c.append(_fwd(FWD_K[i % 5], [FWD_N[0], FWD_N[4], FWD_N[1], FWD_N[6], FWD_N[3]][i], FWD_DEV[0], (i + 1) % 3, dev=d))
    for i, r in enumerate(ROWS):
        c.append(_dx(DX_K[i % 3], DX_N[i % 5], r, i % 3, i % 2))
        if i % 2:
            c.append(_dx(DX_K[4], DX_N[(i + 3) % 5], r, (i + 1) % 3, (i + 1) % 2))
        else:
            c.append(_dx(DX_K[3], DX_N[4], r, (i + 1) % 3, (i + 1) % 2))
    c.append(_dx(DX_K[4], DX_N[4], 65, NONE, 0, inn=(295, 296)))          # block2.0: its first 256 input columns only
    c.append(_dx(DX_K[4], DX_N[4], 65, LEAKY, 1, inn=(295, 296)))
    for i, d in enumerate([0, 65, 4000]):
        c.append(_dx(DX_K[[2, 4, 0][i]], DX_N[[4, 1, 3][i]], 200, [RELU, LEAKY, NONE][i], i % 2, dev=d))
    for i, r in enumerate(DW_ROWS):
        c.append(_dw(DW_OUT[i % 2], DW_IN[i % 4], r))
        c.append(_dw(DW_OUT[3], DW_IN[(i + 1) % 4], r) if i % 2 == 0 else _dw(DW_OUT[2], DW_IN[3], r))
    for i, d in enumerate(DW_DEV[1]):
        c.append(_dw([DW_OUT[3], DW_OUT[1], DW_OUT[2], DW_OUT[0]][i], DW_IN[(i + 2) % 4], DW_DEV[0], dev=d))
    for i, k in enumerate(c):
        k["seed"] = RESEED.get(i, 9000 + i)
        k["id"] = "{}-{}".format(i, case_name(k))
    return c


def case_name(c):
    dev = "" if c["dev"] is None else "-dev{}".format(c["dev"])
    if c["form"] == "fwd":
        return "fwd-k{in}.{ld_x}-n{out}.{ld_z}-r{rows}-a{act}".format(**c) + dev
    if c["form"] == "dx":
        return "dx-k{out}.{ld_z}-n{n_dx}.{ld_dx}-in{in}-r{rows}-a{act}-add{add:d}".format(**c) + dev
    return "dw-o{out}.{ld_z}-i{in}.{ld_x}-r{rows}".format(**c) + dev


def eff_rows(c):
    return c["rows"] if c["dev"] is None else min(c["rows"], c["dev"])


def n_chunks(rows):
    return (rows + CHUNK - 1) // CHUNK


def _padded(seed, stream, rows, cols, ld, m):
    """[rows, ld] unit normals; the columns from `cols` on and the rows from `m` on are NaN: a kernel that reads them shows it."""
    a = synth.hash_normal(seed, stream, (rows, ld)).astype(np.float32)
    a[:, cols:] = np.nan
    a[m:] = np.nan
    return a


def inputs(c):
    """float32 arrays of the call, in the layouts the entry takes."""
    s, rows, m = c["seed"], c["rows"], eff_rows(c)
    d = {"w": synth.hash_normal(s, 1, (c["out"], c["in"])).astype(np.float32)}
    if c["form"] == "fwd":
        d["x"] = _padded(s, 2, rows, c["in"], c["ld_x"], m)
        d["b"] = synth.hash_normal(s, 3, (c["out"],)).astype(np.float32)
    elif c["form"] == "dx":
        d["dz"] = _padded(s, 2, rows, c["out"], c["ld_z"], m)
        if c["act"] != NONE:
            x = _padded(s, 4, rows, c["n_dx"], c["ld_x"], m)          # aux: about half <= 0, some exact zeros of either sign
            if m > 0:
                x[0, 0::7] = np.where(np.isnan(x[0, 0::7]), np.nan, 0.0)
                x[m - 1, 1::5] = np.where(np.isnan(x[m - 1, 1::5]), np.nan, -0.0)
            d["x"] = x
        if c["add"]:
            d["add"] = _padded(s, 5, rows, c["n_dx"], c["ld_dx"], m)
    else:
        d["dz"] = _padded(s, 2, rows, c["out"], c["ld_z"], m)
        d["x"] = _padded(s, 4, rows, c["in"], c["ld_x"], m)
    return d


def act64(x, act):
    if act == RELU:
        return np.where(x > 0, x, 0.0)
    if act == LEAKY:
        return np.where(x > 0, x, np.float64(SLOPE) * x)
    return x


def dact64(y, act):
    if act == RELU:
        return np.where(y > 0, 1.0, 0.0)
    if act == LEAKY:
        return np.where(y > 0, 1.0, np.float64(SLOPE))
    return np.ones_like(y)


def reference(c, d, drop_k=False):
    """{output name: (float64 value, bound)} over the region the call computes: z [m, out], dx [m, n_dx], or gw [out, in] and gb [out].
    drop_k: the product with the last index of the summed dimension left out (the defect the CPU test shows the bound can see)."""
    m = eff_rows(c)
    f = lambda a: np.asarray(a, np.float64)          # noqa: E731
    if c["form"] == "fwd":
        K = c["in"] - (1 if drop_k else 0)
        X, W, b = f(d["x"][:m, :K]), f(d["w"][:, :K]), f(d["b"])
        z = act64(X @ W.T + b, c["act"])
        return {"z": (z, gamma(c["in"] + 4) * (np.abs(X) @ np.abs(W).T + np.abs(b)))}
    if c["form"] == "dx":
        K = c["out"] - (1 if drop_k else 0)
        Z, W = f(d["dz"][:m, :K]), f(d["w"][:K, :c["n_dx"]])
        add = f(d["add"][:m, :c["n_dx"]]) if c["add"] else np.zeros((m, c["n_dx"]))
        mask = dact64(f(d["x"][:m, :c["n_dx"]]), c["act"]) if c["act"] != NONE else 1.0
        return {"dx": ((Z @ W + add) * mask, gamma(c["out"] + 4) * (np.abs(Z) @ np.abs(W) + np.abs(add)))}
    K = max(m - (1 if drop_k else 0), 0)
    Z, X = f(d["dz"][:K, :c["out"]]), f(d["x"][:K, :c["in"]])
    nz = n_chunks(m)
    return {"gw": (Z.T @ X, gamma(min(m, CHUNK) + nz + 4) * (np.abs(Z).T @ np.abs(X))),
            "gb": (Z.sum(0), gamma(nz + 1) * np.abs(Z).sum(0))}
