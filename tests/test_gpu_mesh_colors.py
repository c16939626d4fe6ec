"""GPU tests of the coloured mesh export (Base.export_mesh(colors=...), DESIGN.md sections 4.9 / 4.10): the geometry is the uncoloured call's,
the colours are the point query's at the vertices seen along -normal (or along one shared direction), and the PLY carries them."""
import numpy as np
import pytest
import torch

import ngf_amd  # noqa: F401
from ngf_amd import evalout, synth
from helpers import field_for_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BALL_A, BALL_C, PLANE_RES = 14.0, 20.0, 64
GRID, LEVEL = (24, 20, 28), 0.005


def ball_field():
    """The ball of tests/test_gpu_mesh.py: a TriPlane field whose density pre-activation is a - c |p|^2 in normalised coordinates (one density
    channel per plane, weight 1 on those three channels, zero gauge planes).  Its colour planes are the preset's seeded noise."""
    g = {"model": np.array("triplane"), "aabb": np.array([[-1.5] * 3, [1.5] * 3], np.float32), "grid": np.array([32] * 3),
         "near_far": np.array([2.0, 6.0], np.float32), "step_ratio": np.float32(0.5), "distance_scale": np.float32(25), "thr": np.float32(1e-4)}
    p = synth.triplane_params(5, ((PLANE_RES, PLANE_RES),) * 3, (8, 8), preset="R0")
    u = np.linspace(-1.0, 1.0, PLANE_RES)
    quad = (BALL_A / 3 - BALL_C * (u[None, :] ** 2 + u[:, None] ** 2) / 2).astype(np.float32)
    w = np.zeros((1, 48), np.float32)
    for k, name in enumerate(("xy", "yz", "xz")):
        p[f"plane_{name}"][0, 0] = quad
        p[f"gauge_{name}"][:] = 0
        w[0, 16 * k] = 1
    p["density_decoder.weight"] = w
    p["density_decoder.bias"] = np.zeros((1,), np.float32)
    return field_for_case(g, p, None, device=DEV)


def read_ply(path):
    """(vertex property names in file order, dict of per-vertex arrays, faces) of a binary little-endian PLY with float / uchar vertex properties."""
    raw = open(path, 'rb').read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode('ascii').splitlines()
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    counts, props, element = {}, [], None
    for ln in lines[2:-1]:
        w = ln.split()
        if w[0] == "element":
            element, counts[w[1]] = w[1], int(w[2])
        elif element == "vertex":
            props.append((w[2], {"float": "<f4", "uchar": "u1"}[w[1]]))
        else:
            assert ln == "property list uchar int vertex_indices"
    vdt, fdt = np.dtype(props), np.dtype([('n', 'u1'), ('i', '<i4', (3,))])
    body = raw[end:]
    assert len(body) == counts["vertex"] * vdt.itemsize + counts["face"] * fdt.itemsize
    v = np.frombuffer(body, dtype=vdt, count=counts["vertex"])
    f = np.frombuffer(body, dtype=fdt, count=counts["face"], offset=counts["vertex"] * vdt.itemsize)
    return [p[0] for p in props], {p[0]: v[p[0]] for p in props}, f['i']


def _bits(t):
    return t.contiguous().view(torch.int32)


def _view_dirs(normals):
    """Every vertex is seen along -normal; a zero normal gives (0, 0, -1)."""
    zero = (normals == 0).all(-1, keepdim=True)
    return torch.where(zero, torch.tensor([0.0, 0.0, -1.0], device=normals.device), -normals)


@pytest.fixture(scope="module")
def ball():
    f = ball_field()
    plain = f.export_mesh(level=LEVEL, gridSize=GRID)
    plain_n = f.export_mesh(level=LEVEL, gridSize=GRID, normals=True)
    return f, plain, plain_n


def test_colours_leave_the_geometry_alone(ball):
    f, plain, plain_n = ball
    out = f.export_mesh(level=LEVEL, gridSize=GRID, colors=True)
    assert len(plain) == 2 and len(out) == 3
    v, fc, col = out
    assert v.shape[0] > 100 and torch.equal(_bits(v), _bits(plain[0])) and torch.equal(fc, plain[1])
    assert col.dtype == torch.uint8 and col.shape == (v.shape[0], 3) and col.device == v.device
    out_n = f.export_mesh(level=LEVEL, gridSize=GRID, normals=True, colors=True)
    assert len(out_n) == 4
    assert torch.equal(_bits(out_n[0]), _bits(plain[0])) and torch.equal(out_n[1], plain[1]) and torch.equal(_bits(out_n[2]), _bits(plain_n[2]))
    assert torch.equal(out_n[3], col)                          # the colours do not depend on whether the normals are returned


def test_colours_are_the_query_at_the_vertices_seen_along_minus_normal(ball):
    f, plain, plain_n = ball
    v, fc, nrm, col = f.export_mesh(level=LEVEL, gridSize=GRID, normals=True, colors=True)
    want = evalout.to_uint8(f.query(v, _view_dirs(nrm))['rgb'])
    assert torch.equal(col, want)
    assert len(torch.unique(col.view(-1, 3), dim=0)) > 1       # seeded noise in the colour planes: the colours vary
    # color_kw reaches the query: the gauge planes of this field are zero, so iteration = -1 (gauge off) gives the same colours
    other = f.export_mesh(level=LEVEL, gridSize=GRID, colors=True, color_kw={"iteration": -1})[-1]
    assert torch.equal(other, evalout.to_uint8(f.query(v, _view_dirs(nrm), iteration=-1)['rgb']))
    with pytest.raises(TypeError):
        f.export_mesh(level=LEVEL, gridSize=GRID, colors=True, color_kw={"infoinv": True})


def test_one_shared_direction(ball):
    f, plain, _ = ball
    v, fc, col = f.export_mesh(level=LEVEL, gridSize=GRID, colors=(0, 0, 1))
    assert torch.equal(_bits(v), _bits(plain[0])) and torch.equal(fc, plain[1])
    assert torch.equal(col, evalout.to_uint8(f.query(v, torch.tensor([0.0, 0.0, 1.0]))['rgb']))
    assert torch.equal(col, evalout.to_uint8(f.query(v, torch.tensor([0.0, 0.0, 1.0], device=DEV).expand(v.shape[0], 3))['rgb']))
    with pytest.raises(ValueError):
        f.export_mesh(level=LEVEL, gridSize=GRID, colors=(0, 1))


def test_the_ply_carries_normals_and_colours(ball, tmp_path):
    f, plain, _ = ball
    path = str(tmp_path / "c.ply")
    v, fc, col = f.export_mesh(path, level=LEVEL, gridSize=GRID, colors=True)
    names, pv, pf = read_ply(path)
    assert names == ["x", "y", "z", "red", "green", "blue"]
    assert np.array_equal(np.stack([pv["x"], pv["y"], pv["z"]], 1).view(np.uint32), v.cpu().numpy().view(np.uint32))
    assert np.array_equal(np.stack([pv["red"], pv["green"], pv["blue"]], 1), col.cpu().numpy()) and np.array_equal(pf, fc.cpu().numpy())
    v, fc, nrm, col = f.export_mesh(path, level=LEVEL, gridSize=GRID, normals=True, colors=True)
    names, pv, pf = read_ply(path)
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert np.array_equal(np.stack([pv["x"], pv["y"], pv["z"]], 1).view(np.uint32), v.cpu().numpy().view(np.uint32))
    assert np.array_equal(np.stack([pv["nx"], pv["ny"], pv["nz"]], 1).view(np.uint32), nrm.cpu().numpy().view(np.uint32))
    assert np.array_equal(np.stack([pv["red"], pv["green"], pv["blue"]], 1), col.cpu().numpy()) and np.array_equal(pf, fc.cpu().numpy())
    # without colours the file is what it was: x y z only, also with normals=True
    plain_path = str(tmp_path / "p.ply")
    f.export_mesh(plain_path, level=LEVEL, gridSize=GRID, normals=True)
    names, pv, pf = read_ply(plain_path)
    assert names == ["x", "y", "z"] and np.array_equal(pf, plain[1].cpu().numpy())


@pytest.mark.parametrize("infoinv", [False, True])
def test_an_infoinv_field_exports_colours_with_its_switch(infoinv):
    g = {"model": np.array("infoinv"), "aabb": np.array([[-1.5, -1.0, -1.25], [1.5, 1.0, 1.25]], np.float32), "grid": np.array([32] * 3),
         "near_far": np.array([2.0, 6.0], np.float32), "step_ratio": np.float32(0.5), "distance_scale": np.float32(25), "thr": np.float32(1e-4)}
    f = field_for_case(g, synth.infoinv_params(7, ((32, 32),) * 3, preset="R1"), None, device=DEV)
    grid = (12, 10, 14)
    alpha, _ = f.getDenseAlpha(grid, infoinv=infoinv)
    lo, hi = float(alpha.min()), float(alpha.max())
    assert lo < hi
    level = 0.5 * (lo + hi)
    plain = f.export_mesh(level=level, gridSize=grid, infoinv=infoinv)
    v, fc, nrm, col = f.export_mesh(level=level, gridSize=grid, normals=True, colors=True, infoinv=infoinv)
    assert v.shape[0] > 0 and torch.equal(_bits(v), _bits(plain[0])) and torch.equal(fc, plain[1])       # infoinv= reached the alpha ...
    want = evalout.to_uint8(f.query(v, _view_dirs(nrm), infoinv=infoinv)['rgb'])
    assert torch.equal(col, want)                                                                          # ... and the colours
    other = evalout.to_uint8(f.query(v, _view_dirs(nrm), infoinv=not infoinv)['rgb'])
    assert not torch.equal(col, other)                      # the switch matters for this field
    # an explicit color_kw wins over the alpha's keywords
    col2 = f.export_mesh(level=level, gridSize=grid, colors=True, color_kw={"infoinv": not infoinv}, infoinv=infoinv)[-1]
    assert torch.equal(col2, other)
