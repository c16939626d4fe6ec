"""Host-only restatements of the NeuTex occupancy grid (include/ngf.h: ngf_uv_occupancy_*; csrc/ngf_uv_occupancy.hpp) for
tests/test_uv_occupancy_cpu.py and tests/test_gpu_uv_occupancy.py: the look-up of a point, the reduction of a density lattice to the packed mask,
mask builders, and what the render tests need of a batch (float32 positions, the samples too close to a cell boundary to pin).  numpy and CPU
torch only; every float32 step is rounded separately.

Grid: nx x ny x nz cells over [-1,1]^3, cell (cx,cy,cz) at linear index (cx ny + cy) nz + cz, bits packed like np.packbits."""
import numpy as np
import torch

import uv_render_ref as R
import uv_train_eager as E
from ngf_amd import synth

F = np.float32
EPS = F(2.0 ** -24)
LOOKUP_SHAPES = ((1, 1, 1), (2, 3, 5), (7, 8, 9), (16, 16, 16), (33, 17, 8))
REDUCE_SHAPES = ((1, 1, 1), (2, 3, 5), (9, 8, 7), (16, 16, 16), (33, 17, 8))
RENDER_S = (64, 65, 129)
RENDER_GRIDS = ((5, 7, 16), (16, 16, 16))          # the random mask's grid and the ball's
BOUNDARY_MARGIN = 1e-5                              # a sample at least this far (float64) from every cell boundary has a pinned decision
NEAR_LIMIT = 0.005                                  # samples nearer than that: at most this share of the in-cube samples


# ---- bits --------------------------------------------------------------------------------------------------------------------------------------
def pack(volume):
    """bool / uint8 [nx,ny,nz] -> the packed image, (cells + 7) // 8 bytes, tail bits 0."""
    return np.packbits(np.asarray(volume).reshape(-1) != 0)


def unpack(bits, shape):
    n = int(np.prod(shape))
    return np.unpackbits(np.asarray(bits, np.uint8))[:n].astype(bool).reshape(shape)


# ---- the look-up -------------------------------------------------------------------------------------------------------------------------------
def cell(p, n):
    """min(int(floorf((p + 1.0f) * h)), n - 1) with h = (float)n * 0.5f; p float32 [...], finite.  The add and the multiply round separately."""
    p = np.asarray(p, F)
    h = F(n) * F(0.5)
    s = (p + F(1.0)).astype(F)
    t = (s * h).astype(F)
    return np.minimum(np.floor(t).astype(np.int64), n - 1)


def in_cube(xyz):
    """The render's strict test: -1 < p_k < 1 on every axis (NaN fails it)."""
    xyz = np.asarray(xyz, F)
    with np.errstate(invalid="ignore"):
        return ((xyz > F(-1.0)) & (xyz < F(1.0))).all(-1)


def lookup(bits, shape, xyz):
    """bool [...]: the point is in the cube and its cell's bit is set.  Only in-cube points index the image."""
    xyz = np.asarray(xyz, F)
    ok = in_cube(xyz)
    out = np.zeros(xyz.shape[:-1], bool)
    q = xyz[ok]
    idx = (cell(q[:, 0], shape[0]) * shape[1] + cell(q[:, 1], shape[1])) * shape[2] + cell(q[:, 2], shape[2])
    assert idx.size == 0 or (idx.min() >= 0 and idx.max() < int(np.prod(shape)))
    b = np.asarray(bits, np.uint8)
    out[ok] = ((b[idx >> 3] >> (7 - (idx & 7))) & 1).astype(bool)
    return out


def special_values(n):
    """The coordinates at which the look-up of an axis of n cells can go wrong: both faces and their float32 neighbours inside, 0, every cell
    edge -1 + 2 i / n (as float32) with its float32 neighbours, NaN."""
    edges = (F(-1.0) + F(2.0) * np.arange(1, n, dtype=F) / F(n)).astype(F)
    near = np.concatenate([edges, np.nextafter(edges, F(-2.0)), np.nextafter(edges, F(2.0))]) if n > 1 else np.zeros(0, F)
    base = np.array([-1.0, -1.0 + 2.0 ** -24, 0.0, 1.0 - 2.0 ** -24, 1.0, np.nan], F)
    assert base[1] > F(-1.0) and base[3] < F(1.0)
    return np.concatenate([base, near]).astype(F)


def special_points(shape, seed=77):
    """Every special value on every axis, the other two coordinates random inside the cube."""
    pts = []
    for k in range(3):
        v = special_values(shape[k])
        p = (synth.hash_uniform(seed + k, 900, (v.shape[0], 3)) * F(1.9) - F(0.95)).astype(F)
        p[:, k] = v
        pts.append(p)
    return np.concatenate(pts)


# ---- lattice -> mask ---------------------------------------------------------------------------------------------------------------------------
def hot_cells(sigma, threshold):
    """sigma float32 [(nx+1),(ny+1),(nz+1)] -> bool [nx,ny,nz]: not (max of the cell's 8 corners <= threshold); the max propagates NaN."""
    s = np.asarray(sigma, F)
    m = None
    with np.errstate(invalid="ignore"):
        for a in (0, 1):
            for b in (0, 1):
                for c in (0, 1):
                    v = s[a:s.shape[0] - 1 + a, b:s.shape[1] - 1 + b, c:s.shape[2] - 1 + c]
                    m = v if m is None else np.maximum(m, v)
        return ~(m <= F(threshold))


def dilate_cells(hot, dilate):
    """occupied = some cell within Chebyshev distance ``dilate``, inside the grid, is hot."""
    nx, ny, nz = hot.shape
    pad = np.zeros((nx + 2 * dilate, ny + 2 * dilate, nz + 2 * dilate), bool)
    pad[dilate:dilate + nx, dilate:dilate + ny, dilate:dilate + nz] = hot
    out = np.zeros_like(hot)
    for a in range(2 * dilate + 1):
        for b in range(2 * dilate + 1):
            for c in range(2 * dilate + 1):
                out |= pad[a:a + nx, b:b + ny, c:c + nz]
    return out


def from_lattice(sigma, threshold, dilate):
    """The packed mask of ngf_uv_occupancy_from_lattice."""
    return pack(dilate_cells(hot_cells(sigma, threshold), dilate))


# ---- mask builders -----------------------------------------------------------------------------------------------------------------------------
def random_mask(shape, seed=41, keep=0.5):
    return synth.hash_uniform(seed, 910, tuple(shape)) < F(keep)


def checkerboard(shape):
    i, j, k = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    return ((i + j + k) % 2).astype(bool)


def ball_mask(shape, radius=0.535, centre=(0.0, 0.0, 0.0)):
    """Cells whose centre lies within ``radius`` of ``centre``; a ball of radius 0.535 fills 8 % of the cube."""
    ax = [(-1.0 + (2.0 * np.arange(n) + 1.0) / n) - c for n, c in zip(shape, centre)]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    return x * x + y * y + z * z <= radius * radius


def single_cell(shape, at):
    v = np.zeros(shape, bool)
    v[tuple(at)] = True
    return v


def smooth_density_params(seed, prim):
    """synth.uvmapping_params with the geometry network's first layer cut down to the coordinates and the lowest positional frequency: a density
    that varies at the scale of the cube, as a trained object's does.  (The seeded density is noise at the scale of a cell: its median as threshold
    with dilate 1 leaves no cell of an (8, 9, 10) grid empty.  This one leaves about 6 % empty.)"""
    p = dict(synth.uvmapping_params(seed, prim))
    w = np.array(p["net_geometry_decoder.block.0.weight"]).copy()
    keep = np.zeros(63, bool)          # inputs: x (3), sin(x_d 2^f) d-major (30), cos (30)
    keep[:3] = keep[3:33:10] = keep[33:63:10] = True
    w[:, ~keep] = 0
    p["net_geometry_decoder.block.0.weight"] = w
    return p


# ---- render batches ----------------------------------------------------------------------------------------------------------------------------
def render_batches(prim, S):
    """The batches of the render tests: 37 pool rays (odd: the last ray is unpaired; 3 rays miss), and an edge batch of 2 cameras.
    -> [(name, campos [N,3], raydir [N,R,3], U [N,R,S])]"""
    cam, rd, U = R.pool_rays(prim, S, R.SEED, R=37)
    b = E.edge_batch(R.SEED, prim, S, R=9, n_cams=2)
    return [("pool37", cam, rd, U), ("edge2x9", b["campos"], b["raydir"], b["U"])]


def render_masks():
    """[(name, bool volume)]: a random (5,7,16) mask with keep 0.5 and a ball in a (16,16,16) grid."""
    return [("random", random_mask(RENDER_GRIDS[0])), ("ball", ball_mask(RENDER_GRIDS[1], radius=0.7))]


def positions(campos, raydir, U, dtype):
    """E.cube_ray_generation in ``dtype`` -> (pos [N,R,S,3], valid [N,R,S] bool) as numpy."""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)          # noqa: E731
    pos, _, valid = E.cube_ray_generation(t(campos), t(raydir), U.shape[-1], t(U))
    return pos.numpy(), valid.bool().numpy()


def near_boundary(pos64, shape, margin=BOUNDARY_MARGIN):
    """bool [...]: the float64 position is nearer than ``margin`` to a cell boundary -1 + 2 i / n of some axis."""
    near = np.zeros(pos64.shape[:-1], bool)
    for k in range(3):
        t = (pos64[..., k] + 1.0) * shape[k] / 2.0
        near |= np.abs(t - np.rint(t)) * 2.0 / shape[k] < margin
    return near


def cells64(pos64, shape):
    return np.stack([np.minimum(np.floor((pos64[..., k] + 1.0) * shape[k] / 2.0).astype(np.int64), shape[k] - 1) for k in range(3)], -1)


def decisions(campos, raydir, U, volume):
    """What the masked render must decide for a batch: ``keep`` [N,R,S] = in-cube (float32) and restatement(p32), ``pinned`` [N,R,S] = in-cube
    samples whose float64 position keeps BOUNDARY_MARGIN from every cell boundary, ``valid`` [N,R,S] = the float64 in-cube mask."""
    p32, v32 = positions(campos, raydir, U, torch.float32)
    p64, v64 = positions(campos, raydir, U, torch.float64)
    assert np.array_equal(v32, v64), "the batch keeps its samples off the faces: float32 and float64 agree on the in-cube mask"
    keep = lookup(pack(volume), volume.shape, p32) & v32
    pinned = v64 & ~near_boundary(p64, volume.shape)
    return keep, pinned, v64, p32, p64
