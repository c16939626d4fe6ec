"""Helpers of the mesh-export tests: a numpy restatement of csrc/ngf_mesh.hpp (same definitions, same output order, and in float32 the same
operations in the same order, so vertices compare bit for bit), an edge-use counter, Euler characteristic, signed volume and a PLY reader.
The case table comes from the package (ngf_amd.mesh_table)."""
import collections

import numpy as np

import ngf_amd  # noqa: F401
from ngf_amd import mesh_table as T

TRI = np.full((256, 3 * T.MAX_TRIS), -1, dtype=np.int64)
for _c, _t in enumerate(T.TRIS):
    _flat = [e for tri in _t for e in tri]
    TRI[_c, :len(_flat)] = _flat
TRI_COUNT = np.array(T.TRI_COUNT, dtype=np.int64)
EDGE_AXIS = np.array(T.EDGE_AXIS, dtype=np.int64)
EDGE_BASE = np.array(T.EDGE_BASE, dtype=np.int64)
_POP3 = np.array([0, 1, 1, 2, 1, 2, 2, 3], dtype=np.int64)


def _gradient(v, spacing, dtype):
    """[3,gx,gy,gz]: central differences, one-sided at the border, 0 along a flat axis, per unit of world length."""
    g = np.zeros((3,) + v.shape, dtype=dtype)
    for a in range(3):
        d = v.shape[a]
        if d == 1:
            continue
        x = np.moveaxis(v, a, 0)
        out = np.moveaxis(g[a], a, 0)
        sp = dtype(spacing[a])
        out[0] = (x[1] - x[0]) / sp
        out[-1] = (x[-1] - x[-2]) / sp
        if d > 2:
            out[1:-1] = (x[2:] - x[:-2]) / (dtype(2) * sp)
    return g


def marching_cubes_ref(vol, level, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), normals=False, flip=False, dtype=np.float32):
    """(verts [nv,3] dtype, faces [nt,3] int32[, normals [nv,3] dtype]) of a numpy volume [gx,gy,gz] (float32 values).  ``dtype`` is the
    precision of the interpolation and the normals; the classification always compares the float32 values with the float32 level."""
    vol = np.asarray(vol, dtype=np.float32)
    level = np.float32(level)
    spacing = [np.float32(s) for s in spacing]
    origin = [np.float32(o) for o in origin]
    gx, gy, gz = vol.shape
    empty = (np.zeros((0, 3), dtype), np.zeros((0, 3), np.int32)) + ((np.zeros((0, 3), dtype),) if normals else ())
    if min(vol.shape) == 1:
        return empty
    with np.errstate(all='ignore'):
        inside = vol >= level
        mask = np.zeros(vol.shape, dtype=np.int64)
        mask[:-1] |= (inside[:-1] != inside[1:]).astype(np.int64)
        mask[:, :-1] |= (inside[:, :-1] != inside[:, 1:]).astype(np.int64) << 1
        mask[:, :, :-1] |= (inside[:, :, :-1] != inside[:, :, 1:]).astype(np.int64) << 2
        mask = mask.reshape(-1)
        count = _POP3[mask]
        first = np.cumsum(count) - count
        nv = int(count.sum())
        step = (gy * gz, gz, 1)
        v = vol.astype(dtype)
        flat = v.reshape(-1)
        idx = np.stack(np.unravel_index(np.arange(vol.size), vol.shape), 0)
        verts = np.zeros((nv, 3), dtype)
        nrm = np.zeros((nv, 3), dtype)
        grad = _gradient(v, spacing, dtype).reshape(3, -1) if normals else None
        for a in range(3):
            p = np.nonzero(mask >> a & 1)[0]
            at = first[p] + _POP3[mask[p] & ((1 << a) - 1)]
            v0, v1 = flat[p], flat[p + step[a]]
            t = (dtype(level) - v0) / (v1 - v0)
            t = np.where((t >= 0) & (t <= 1), t, dtype(0.5))
            for b in range(3):
                verts[at, b] = dtype(origin[b]) + (idx[b][p].astype(dtype) + (t if b == a else dtype(0))) * dtype(spacing[b])
            if normals:
                g0, g1 = grad[:, p], grad[:, p + step[a]]
                g = g0 + t * (g1 - g0)
                length = np.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
                ok = (length > 0) & np.isfinite(length)
                nrm[at] = np.where(ok, -g / np.where(ok, length, 1), dtype(0)).T
        # faces: cells in point order, a cell's triangles in table order
        c = inside.astype(np.int64)
        case = (c[:-1, :-1, :-1] | c[1:, :-1, :-1] << 1 | c[:-1, 1:, :-1] << 2 | c[1:, 1:, :-1] << 3 |
                c[:-1, :-1, 1:] << 4 | c[1:, :-1, 1:] << 5 | c[:-1, 1:, 1:] << 6 | c[1:, 1:, 1:] << 7)
        cell_p = (np.arange(vol.size).reshape(vol.shape)[:-1, :-1, :-1]).reshape(-1)
        case = case.reshape(-1)
        keep = TRI_COUNT[case] > 0
        cell_p, case = cell_p[keep], case[keep]
        rows = TRI[case]
        valid = rows >= 0
        e = rows[valid]
        owner = np.broadcast_to(cell_p[:, None], rows.shape)[valid]
        a = EDGE_AXIS[e]
        base = EDGE_BASE[e]
        owner = owner + (base & 1) * step[0] + (base >> 1 & 1) * step[1] + (base >> 2) * step[2]
        faces = (first[owner] + _POP3[mask[owner] & ((1 << a) - 1)]).reshape(-1, 3).astype(np.int32)
    if flip:
        faces = faces[:, ::-1].copy()
    return (verts, faces, nrm) if normals else (verts, faces)


def edge_uses(faces):
    """Counter of the directed mesh edges (a, b) over all triangles."""
    f = np.asarray(faces, dtype=np.int64)
    pairs = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    return collections.Counter(map(tuple, pairs.tolist()))


def closed_and_oriented(faces):
    """Every directed edge exactly once and its reverse exactly once: a closed surface with one consistent orientation."""
    uses = edge_uses(faces)
    return all(n == 1 and uses.get((b, a), 0) == 1 for (a, b), n in uses.items())


def euler_characteristic(faces):
    f = np.asarray(faces, dtype=np.int64)
    uses = edge_uses(f)
    edges = {(min(a, b), max(a, b)) for a, b in uses}
    return len(np.unique(f)) - len(edges) + f.shape[0]


def signed_volume(verts, faces):
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    return float(np.einsum('ij,ij->i', v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def read_ply(path):
    """(verts float32 [nv,3], faces int32 [nt,3]) of a binary little-endian PLY with x y z floats and a uchar/int vertex_indices list."""
    with open(path, 'rb') as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode('ascii').split('\n')
    assert lines[0] == 'ply' and lines[1] == 'format binary_little_endian 1.0', lines[:2]
    nv = int([ln for ln in lines if ln.startswith('element vertex')][0].split()[-1])
    nt = int([ln for ln in lines if ln.startswith('element face')][0].split()[-1])
    props = [ln for ln in lines if ln.startswith('property')]
    assert props == ['property float x', 'property float y', 'property float z', 'property list uchar int vertex_indices'], props
    verts = np.frombuffer(data, dtype='<f4', count=3 * nv, offset=end).reshape(nv, 3)
    rec = np.frombuffer(data, dtype=[('n', 'u1'), ('i', '<i4', (3,))], count=nt, offset=end + 12 * nv)
    assert end + 12 * nv + 13 * nt == len(data) and (rec['n'] == 3).all()
    return verts.copy(), rec['i'].copy()


def ball(shape, radius, centre=None, spacing=(1.0, 1.0, 1.0)):
    """r - |p - centre| on the lattice index * spacing, float32 (inside the ball: positive)."""
    ax = [np.arange(n, dtype=np.float64) * s for n, s in zip(shape, spacing)]
    centre = [(n - 1) * s / 2 for n, s in zip(shape, spacing)] if centre is None else centre
    x, y, z = np.meshgrid(*[a - c for a, c in zip(ax, centre)], indexing='ij')
    return (radius - np.sqrt(x * x + y * y + z * z)).astype(np.float32)
