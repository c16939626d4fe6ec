"""CPU-side checks of the point-query boundary (ngf_field_query) and of the PLY writer with vertex normals and colours: the symbol is
exported and bound, the argument checks that need no GPU answer, and ``mesh.write_ply`` round-trips through a reader written here and still
writes the bytes it wrote before the optional arguments existed."""
import ctypes as C
import inspect

import numpy as np
import pytest

import ngf_amd  # noqa: F401
from ngf_amd import _lib, fieldbase, infoinv, mesh, triplane

NGF_E_ARG = 1


def test_query_symbol_is_exported_and_bound():
    assert "ngf_field_query" in _lib.SYMBOLS and _lib.QUERY_NO_MASK == 1
    for which in ("product", "exp"):
        with _lib.library(which) as L:
            fn = L.ngf_field_query
            assert fn.argtypes == [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]
            assert fn.restype is C.c_int


def test_query_refuses_a_null_handle_and_names_itself():
    L = _lib.lib()
    assert L.ngf_field_query(None, None, 0, 0, None, 3, 0, None, None, None, None) == NGF_E_ARG
    assert b"ngf_field_query" in L.ngf_last_error()
    buf = (C.c_float * 6)()
    assert L.ngf_field_query(None, C.addressof(buf), 1, 0, None, 3, 0, C.addressof(buf), None, None, None) == NGF_E_ARG
    assert b"ngf_field_query" in L.ngf_last_error()


def test_query_signature_and_cpu_refusal():
    sig = inspect.signature(fieldbase.Base.query)
    assert list(sig.parameters) == ["self", "xyz", "viewdirs", "use_mask", "want_coords", "kw"]
    assert sig.parameters["viewdirs"].default is None and sig.parameters["use_mask"].default is True and sig.parameters["want_coords"].default is False
    assert sig.parameters["use_mask"].kind is inspect.Parameter.KEYWORD_ONLY
    esig = inspect.signature(fieldbase.Base.export_mesh)
    assert list(esig.parameters) == ["self", "path", "level", "gridSize", "normals", "flip", "colors", "color_kw", "kw"]
    assert esig.parameters["colors"].default is None and esig.parameters["color_kw"].default is None
    import torch
    aabb = torch.tensor([[-1.5] * 3, [1.5] * 3])
    f = triplane.TriPlane(aabb, [16] * 3, "cpu", step_ratio=0.5)
    g = infoinv.TriPlane(aabb, [16] * 3, "cpu", step_ratio=0.5)
    with pytest.raises(RuntimeError, match="GPU only"):
        f.query(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="GPU only"):
        g.query(torch.zeros(4, 3), infoinv=False)
    with pytest.raises(TypeError):          # unknown keywords, as _alpha_mode
        f.query(torch.zeros(4, 3), infoinv=True)
    with pytest.raises(TypeError):
        g.query(torch.zeros(4, 3), iteration=3)
    assert f._query_mode() == 1 and f._query_mode(iteration=-1) == 0 and g._query_mode() == 1 and g._query_mode(infoinv=False) == 0


# ---- PLY -------------------------------------------------------------------------------------------------------------------------------------
def _write_ply_before(path, verts, faces):
    """The writer as it was before it took normals and colours, restated."""
    v = np.ascontiguousarray(np.asarray(verts, dtype='<f4').reshape(-1, 3))
    f = np.asarray(faces, dtype='<i4').reshape(-1, 3)
    rec = np.empty((f.shape[0],), dtype=[('n', 'u1'), ('i', '<i4', (3,))])
    rec['n'] = 3
    rec['i'] = f
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {v.shape[0]}\nproperty float x\nproperty float y\nproperty float z\n"
              f"element face {f.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, 'wb') as fh:
        fh.write(header.encode('ascii'))
        fh.write(v.tobytes())
        fh.write(rec.tobytes())


def read_ply(path):
    """A reader for the files write_ply makes: returns (property names of the vertex element in file order, dict of arrays, faces)."""
    raw = open(path, 'rb').read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode('ascii').splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = nf = None
    props, element = [], None
    for ln in lines[2:-1]:
        w = ln.split()
        if w[0] == "element":
            element = w[1]
            if element == "vertex":
                nv = int(w[2])
            else:
                assert element == "face"
                nf = int(w[2])
        elif w[0] == "property" and element == "vertex":
            props.append((w[2], {"float": "<f4", "uchar": "u1"}[w[1]]))
        else:
            assert ln == "property list uchar int vertex_indices" and element == "face"
    vdt = np.dtype(props)
    body = raw[end:]
    v = np.frombuffer(body, dtype=vdt, count=nv)
    fdt = np.dtype([('n', 'u1'), ('i', '<i4', (3,))])
    f = np.frombuffer(body, dtype=fdt, count=nf, offset=nv * vdt.itemsize)
    assert len(body) == nv * vdt.itemsize + nf * fdt.itemsize and (f['n'] == 3).all()
    return [p[0] for p in props], {p[0]: v[p[0]] for p in props}, f['i']


def _mesh_arrays():
    rng = np.random.default_rng(5)
    verts = rng.standard_normal((7, 3)).astype(np.float32)
    faces = rng.integers(0, 7, (5, 3)).astype(np.int32)
    normals = rng.standard_normal((7, 3)).astype(np.float32)
    colors = rng.integers(0, 256, (7, 3)).astype(np.uint8)
    colors[0] = (0, 255, 128)
    return verts, faces, normals, colors


@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("with_colors", [False, True])
def test_write_ply_round_trips(tmp_path, with_normals, with_colors):
    verts, faces, normals, colors = _mesh_arrays()
    p = str(tmp_path / "m.ply")
    mesh.write_ply(p, verts, faces, normals=normals if with_normals else None, colors=colors if with_colors else None)
    names, v, f = read_ply(p)
    want = ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else []) + (["red", "green", "blue"] if with_colors else [])
    assert names == want                                   # floats first, then the uchar colours
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1).view(np.uint32), verts.view(np.uint32))
    if with_normals:
        assert np.array_equal(np.stack([v["nx"], v["ny"], v["nz"]], 1).view(np.uint32), normals.view(np.uint32))
    if with_colors:
        got = np.stack([v["red"], v["green"], v["blue"]], 1)
        assert got.dtype == np.uint8 and np.array_equal(got, colors)
    assert np.array_equal(f, faces)
    # the bytes: header, then 12 [+ 12] [+ 3] bytes per vertex, then 13 per face
    raw = open(p, 'rb').read()
    body = raw[raw.index(b"end_header\n") + 11:]
    per = 12 + (12 if with_normals else 0) + (3 if with_colors else 0)
    assert len(body) == 7 * per + 5 * 13
    assert body[:12] == verts[0].astype('<f4').tobytes()
    if with_colors:
        assert body[per - 3:per] == bytes([0, 255, 128])


def test_write_ply_without_the_new_arguments_writes_the_old_bytes(tmp_path):
    verts, faces, _, _ = _mesh_arrays()
    a, b, c = str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), str(tmp_path / "c.ply")
    _write_ply_before(a, verts, faces)
    mesh.write_ply(b, verts, faces)
    mesh.write_ply(c, verts, faces, normals=None, colors=None)
    assert open(a, 'rb').read() == open(b, 'rb').read() == open(c, 'rb').read()
    e = str(tmp_path / "e.ply")                            # an empty mesh too
    _write_ply_before(e, np.zeros((0, 3)), np.zeros((0, 3)))
    mesh.write_ply(b, np.zeros((0, 3)), np.zeros((0, 3)))
    assert open(e, 'rb').read() == open(b, 'rb').read()


def test_write_ply_refuses_mismatched_attributes(tmp_path):
    verts, faces, normals, colors = _mesh_arrays()
    with pytest.raises(ValueError):
        mesh.write_ply(str(tmp_path / "x.ply"), verts, faces, normals=normals[:3])
    with pytest.raises(ValueError):
        mesh.write_ply(str(tmp_path / "x.ply"), verts, faces, colors=colors.astype(np.float32))
