"""Mesh export on the GPU: marching cubes over a dense float volume (csrc/ngf_mesh.hip), the reference's
``convert_sdf_samples_to_ply`` (TriPlane/utils.py:179-239) on top of it, and a binary PLY writer in numpy (there is no ``plyfile``).  For NeuTex
(uvmapping.NeuTex.export_mesh): ``atlas_coords`` (gauge uv -> OBJ texture coordinates in the exported atlas), ``unwrap_seam`` and ``write_obj``;
``icosphere`` and ``square_template`` are the atlas templates of NeuTex.coordinate_deformation (numpy, on the host).

The triangulation is the table of ``ngf_amd.mesh_table``: the usual one-vertex-per-crossing-edge definition, closed and consistently
oriented, but NOT skimage's Lewiner tables -- vertex and face ORDER (and the split of a cell's polygons into triangles) differ from
``skimage.measure.marching_cubes``."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib


def _check_volume(volume):
    if not torch.is_tensor(volume) or volume.dim() != 3:
        raise ValueError("marching_cubes wants a 3-D tensor [gx,gy,gz]")
    if volume.device.type != 'cuda':
        raise RuntimeError("ngf_amd.mesh runs on the GPU only (a CUDA/HIP tensor); there is no CPU path")
    return volume if volume.dtype == torch.float32 else volume.float()


@torch.no_grad()
def marching_cubes(volume, level, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), normals=False, flip=False):
    """Iso-surface of ``volume`` [gx,gy,gz] (a CUDA tensor of any strides; never copied or transposed) at ``level``.

    Returns ``(verts [nv,3] float32, faces [nt,3] int32)`` -- plus ``normals [nv,3]`` with ``normals=True`` -- on the volume's device.  Lattice point
    (i,j,k) sits at ``origin + (i,j,k) * spacing``; a point is inside iff ``v >= level`` and triangle normals point to the outside (low) side;
    ``flip=True`` reverses every triangle.  The arrays are a function of the volume alone (two calls are bit-identical).  One host
    synchronisation: the two counts come back before the outputs are allocated."""
    vol = _check_volume(volume)
    dev = vol.device
    L = _lib.lib()
    dims = (C.c_int32 * 3)(*vol.shape)
    strides = (C.c_int64 * 3)(*vol.stride())
    sp = (C.c_float * 3)(*[float(s) for s in spacing])
    org = (C.c_float * 3)(*[float(o) for o in origin])
    level = float(level)
    nbytes = L.ngf_mesh_workspace_bytes(*vol.shape)
    if nbytes < 0:
        raise ValueError(f"marching_cubes: a volume of {tuple(vol.shape)} is refused (no empty axis, and 3 * points must stay below 2^31)")
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        work = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
        counts = torch.empty((2,), device=dev, dtype=torch.int64)
        _lib.check(L.ngf_mesh_count(vol.data_ptr(), dims, strides, C.c_float(level), work.data_ptr(), nbytes, counts.data_ptr(), stream))
        nv, nt = (int(x) for x in counts.tolist())
        verts = torch.empty((nv, 3), device=dev, dtype=torch.float32)
        faces = torch.empty((nt, 3), device=dev, dtype=torch.int32)
        nrm = torch.empty((nv, 3), device=dev, dtype=torch.float32) if normals else None
        flags = (_lib.MESH_FLIP if flip else 0) | (_lib.MESH_NORMALS if normals else 0)
        _lib.check(L.ngf_mesh_emit(vol.data_ptr(), dims, strides, C.c_float(level), org, sp, flags, work.data_ptr(), nbytes, nv, nt,
                                   verts.data_ptr(), None if nrm is None else nrm.data_ptr(), faces.data_ptr(), stream))
    return (verts, faces, nrm) if normals else (verts, faces)


def write_ply(path, verts, faces, normals=None, colors=None):
    """Binary little-endian PLY: vertex ``x y z [nx ny nz] [red green blue]`` -- the floats first (float32), then the uchar colours -- and face
    ``vertex_indices`` as a list (uchar count) of int32.  ``normals`` [nv,3] float and ``colors`` [nv,3] uint8 are optional; without them the
    file is the plain ``x y z`` one."""
    v = np.ascontiguousarray(np.asarray(verts, dtype='<f4').reshape(-1, 3))
    f = np.asarray(faces, dtype='<i4').reshape(-1, 3)
    rec = np.empty((f.shape[0],), dtype=[('n', 'u1'), ('i', '<i4', (3,))])
    rec['n'] = 3
    rec['i'] = f
    props = "property float x\nproperty float y\nproperty float z\n"
    fields = [('p', '<f4', (3,))]
    if normals is not None:
        props += "property float nx\nproperty float ny\nproperty float nz\n"
        fields.append(('n', '<f4', (3,)))
    if colors is not None:
        props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
        fields.append(('c', 'u1', (3,)))
    vrec = np.empty((v.shape[0],), dtype=fields)          # packed: 12 [+ 12] [+ 3] bytes per vertex
    vrec['p'] = v
    if normals is not None:
        nn = np.asarray(normals, dtype='<f4').reshape(-1, 3)
        if nn.shape != v.shape:
            raise ValueError(f"write_ply: normals {nn.shape} do not match the {v.shape[0]} vertices")
        vrec['n'] = nn
    if colors is not None:
        cc = np.asarray(colors)
        if cc.dtype != np.uint8 or cc.reshape(-1, 3).shape != v.shape:
            raise ValueError(f"write_ply: colors must be uint8 [{v.shape[0]},3], got {cc.dtype} {cc.shape}")
        vrec['c'] = cc.reshape(-1, 3)
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {v.shape[0]}\n" + props +
              f"element face {f.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, 'wb') as fh:
        fh.write(header.encode('ascii'))
        fh.write(vrec.tobytes())
        fh.write(rec.tobytes())


def atlas_coords(uv, primitive_type, resolution=None):
    """OBJ texture coordinates ``[..., 2]`` = (s left to right, t bottom to top) of gauge outputs ``uv`` [..., 2|3] in the atlas image the
    NeuTex exporters write -- defined by those images: a point the exporter evaluates maps to the centre of the texel that holds its colour.

    square  (``_export_square(R)`` [R,R,3], row i <-> uv_0, column j <-> uv_1):  s = (uv_1 + 1) / 2,  t = 1 - (uv_0 + 1) / 2
    sphere  (``_export_sphere(R)`` [R,2R,3], equirectangular, rows flipped; the image depends on R through its half-texel offset, hence
            ``resolution``): for the unit vector (a, b, c), y = acos(-b), x = atan2(-a, -c),
            s = ((x - pi) mod 2 pi) / (2 pi) + 0.5 / (2R),  t = y / pi + 0.5 / R

    A tensor or an array, evaluated in its own dtype and (for a tensor) on its own device; s of the sphere lies in [0.5/(2R), 1 + 0.5/(2R)):
    see ``unwrap_seam`` for the triangles that cross the image's left edge."""
    was_tensor = torch.is_tensor(uv)
    q = uv if was_tensor else torch.as_tensor(np.asarray(uv))
    if not q.is_floating_point():
        q = q.float()
    if primitive_type == 'square':
        if q.shape[-1] not in (2, 3):
            raise ValueError(f"atlas_coords: square uv must be [..., 2] (or [..., 3], z ignored), got {tuple(q.shape)}")
        st = torch.stack([(q[..., 1] + 1) / 2, 1 - (q[..., 0] + 1) / 2], dim=-1)
    elif primitive_type == 'sphere':
        if q.shape[-1] != 3:
            raise ValueError(f"atlas_coords: sphere uv must be [..., 3], got {tuple(q.shape)}")
        if resolution is None or int(resolution) < 1:
            raise ValueError("atlas_coords: the sphere atlas needs the resolution R of its [R,2R] image")
        R = int(resolution)
        y = torch.acos((-q[..., 1]).clamp(-1, 1))
        x = torch.atan2(-q[..., 0], -q[..., 2])
        s = torch.remainder(x - np.pi, 2 * np.pi) / (2 * np.pi) + 0.5 / (2 * R)
        st = torch.stack([s, y / np.pi + 0.5 / R], dim=-1)
    else:
        raise ValueError(f"Unknown primitive type {primitive_type}")
    return st if was_tensor else st.numpy()


def unwrap_seam(faces, st):
    """Per-corner texture indices for an atlas that is periodic in s (the sphere's): in each triangle a corner whose s lies more than 0.5 below
    the triangle's largest s takes a duplicate of its coordinates with s + 1 (one duplicate per vertex, shared by every triangle that needs it),
    so a triangle that fits in half a turn spans at most 0.5 in s instead of running backwards across the whole image; a renderer needs the
    texture's repeat wrap mode (the default of the common ones) for the s > 1 corners.  (At EXACTLY half a turn the rule can leave a wider span.)  Returns ``(st_ext [nv + nd, 2], faces_vt [nt,3] int32)``
    as numpy arrays; triangles that need nothing keep the vertices' own indices."""
    f = (faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)).astype(np.int64).reshape(-1, 3)
    st = st.detach().cpu().numpy() if torch.is_tensor(st) else np.asarray(st)
    st = st.reshape(-1, 2)
    s = st[f, 0]
    low = s < s.max(axis=1, keepdims=True) - 0.5
    ids, inv = np.unique(f[low], return_inverse=True)
    dup = st[ids].copy()
    dup[:, 0] += 1
    faces_vt = f.copy()
    faces_vt[low] = st.shape[0] + inv.reshape(-1)
    return np.concatenate([st, dup], axis=0), faces_vt.astype(np.int32)


def write_obj(path, verts, faces, st, faces_vt=None, texture=None, normals=None):
    """Wavefront OBJ with texture coordinates: ``path`` (``v`` / ``vt`` [/ ``vn``] lines in ``%.9g``, which round-trips a float32, and
    ``f v/vt[/vn]`` corners, 1-based), its material file (``path`` with the extension ``.mtl``) and, when ``texture`` -- a uint8 [H,W,3] array,
    row 0 on top -- is given, the image as ``.png`` next to them, named by the material's ``map_Kd``.  ``faces_vt`` [nt,3] are the corners'
    indices into ``st`` (default: the vertex indices); ``normals`` [nv,3] are per vertex.  An empty mesh gives a valid file with no elements."""
    import os

    def host(a, dtype):
        return np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=dtype)

    v = host(verts, np.float32).reshape(-1, 3)
    f = host(faces, np.int64).reshape(-1, 3)
    vt = host(st, np.float32).reshape(-1, 2)
    fv = f if faces_vt is None else host(faces_vt, np.int64).reshape(-1, 3)
    if fv.shape != f.shape:
        raise ValueError(f"write_obj: faces_vt {fv.shape} does not match faces {f.shape}")
    if f.size and (f.min() < 0 or f.max() >= v.shape[0] or fv.min() < 0 or fv.max() >= vt.shape[0]):
        raise ValueError("write_obj: a face index points outside verts / st")
    vn = None
    if normals is not None:
        vn = host(normals, np.float32).reshape(-1, 3)
        if vn.shape != v.shape:
            raise ValueError(f"write_obj: normals {vn.shape} do not match the {v.shape[0]} vertices")
    stem = os.path.splitext(path)[0]
    name = os.path.basename(stem)
    if texture is not None:
        from PIL import Image
        img = np.asarray(texture)
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"write_obj: texture must be uint8 [H,W,3], got {img.dtype} {img.shape}")
        Image.fromarray(np.ascontiguousarray(img)).save(stem + ".png")
    with open(stem + ".mtl", "w") as fh:
        fh.write("newmtl atlas\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\n")
        if texture is not None:
            fh.write(f"map_Kd {name}.png\n")
    def rows(fmt, a, chunk=1 << 16):
        # one formatting call per 65 536 rows (the format repeated, the block's numbers as one flat tuple): 2.5x faster than a call per row
        return [(fmt * len(a[i:i + chunk])) % tuple(a[i:i + chunk].ravel().tolist()) for i in range(0, len(a), chunk)]

    parts = [f"mtllib {name}.mtl\nusemtl atlas\n"] + rows("v %.9g %.9g %.9g\n", v) + rows("vt %.9g %.9g\n", vt)
    if vn is not None:
        parts += rows("vn %.9g %.9g %.9g\n", vn)
        parts += rows("f %d/%d/%d %d/%d/%d %d/%d/%d\n", np.stack([f + 1, fv + 1, f + 1], axis=-1).reshape(-1, 9))
    else:
        parts += rows("f %d/%d %d/%d %d/%d\n", np.stack([f + 1, fv + 1], axis=-1).reshape(-1, 6))
    with open(path, "w") as fh:
        fh.write("".join(parts))


# --- the atlas templates of NeuTex.coordinate_deformation (uvmapping.py) ------------------------------------------------
_ICO_FACES = ((0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
              (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1))


def icosphere(division):
    """The unit icosphere: an icosahedron subdivided ``division`` times 4-to-1, every level normalised to the sphere (in float64; the result is
    rounded to float32 once).  Returns ``(verts float32 [10 * 4^d + 2, 3], faces int64 [20 * 4^d, 3])`` as numpy arrays, closed, faces
    counter-clockwise seen from outside.

    The order is this project's own (there is no trimesh here to match).  Level 0: the twelve vertices (-1,t,0) (1,t,0) (-1,-t,0) (1,-t,0)
    (0,-1,t) (0,1,t) (0,-1,-t) (0,1,-t) (t,0,-1) (t,0,1) (-t,0,-1) (-t,0,1), t the golden ratio, normalised, and the twenty faces of
    ``_ICO_FACES``.  A level keeps the vertices it has and appends one midpoint per edge, the edges in ascending order of (smaller end, larger
    end); face (a, b, c) becomes, in place and in this order, (a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)."""
    d = int(division)
    if d < 0:
        raise ValueError(f"icosphere: division must be >= 0, got {division}")
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = np.array([(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
                  (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)], dtype=np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    f = np.array(_ICO_FACES, dtype=np.int64)
    for _ in range(d):
        nv = v.shape[0]
        ends = np.stack([f, np.roll(f, -1, axis=1)], axis=-1)          # [F, 3, 2]: edges ab, bc, ca
        lo, hi = ends.min(-1), ends.max(-1)
        key, inv = np.unique(lo * nv + hi, return_inverse=True)
        mid = v[key // nv] + v[key % nv]
        v = np.concatenate([v, mid / np.linalg.norm(mid, axis=1, keepdims=True)], axis=0)
        m = nv + inv.reshape(-1, 3)                                    # ab, bc, ca of every face
        a, b, c, ab, bc, ca = f[:, 0], f[:, 1], f[:, 2], m[:, 0], m[:, 1], m[:, 2]
        f = np.stack([a, ab, ca, b, bc, ab, c, ca, bc, ab, bc, ca], axis=-1).reshape(-1, 3)
    return v.astype(np.float32), np.ascontiguousarray(f)


def square_template(side):
    """The regular grid of the reference's SquareTemplate.get_regular_points (gauge_fields.py:139-143) as a mesh: ``(verts float32 [side^2, 2],
    faces int64 [2 (side - 1)^2, 3])`` as numpy arrays.  Vertex i * side + j is (u_i, u_j) with u = ``np.linspace(-1, 1, side)`` (float64,
    rounded to float32 once, as the reference's ``torch.FloatTensor(uv)`` rounds it); cell (i, j), cells in row-major order, gives the two
    triangles ((i,j), (i+1,j), (i+1,j+1)) and ((i,j), (i+1,j+1), (i,j+1)), both of positive area in the (u_0, u_1) plane."""
    side = int(side)
    if side < 2:
        raise ValueError(f"square_template: side must be >= 2, got {side}")
    uv = np.stack(np.meshgrid(*([np.linspace(-1, 1, side)] * 2), indexing="ij"), axis=-1).reshape((-1, 2))
    i, j = np.meshgrid(np.arange(side - 1, dtype=np.int64), np.arange(side - 1, dtype=np.int64), indexing="ij")
    p00, p10, p11, p01 = i * side + j, (i + 1) * side + j, (i + 1) * side + j + 1, i * side + j + 1
    faces = np.stack([p00, p10, p11, p00, p11, p01], axis=-1).reshape(-1, 3)
    return uv.astype(np.float32), np.ascontiguousarray(faces)


def mesh_points(verts, bbox, offset=None, scale=None):
    """The point arithmetic of convert_sdf_samples_to_ply (TriPlane/utils.py:206-217), literally: bbox[0] + verts per column into an
    array of verts' dtype, then ``/ scale``, then ``- offset``."""
    pts = np.zeros_like(verts)
    pts[:, 0] = bbox[0, 0] + verts[:, 0]
    pts[:, 1] = bbox[0, 1] + verts[:, 1]
    pts[:, 2] = bbox[0, 2] + verts[:, 2]
    if scale is not None:
        pts = pts / scale
    if offset is not None:
        pts = pts - offset
    return pts


def convert_sdf_samples_to_ply(pytorch_3d_sdf_tensor, ply_filename_out, bbox, level=0.5, offset=None, scale=None):
    """TriPlane/utils.py:179-239 with the marching cubes on the GPU: spacing ``(bbox[1] - bbox[0]) / shape`` (the reference's own: shape, not
    shape - 1), vertices in voxel units times that spacing, faces reversed, then bbox[0] added, ``/ scale``, ``- offset``, and a binary PLY.
    ``bbox`` is indexed ``[row, column]`` like the reference's (a numpy array or a tensor).  Returns ``(mesh_points, faces)`` as numpy arrays."""
    bbox = bbox.detach().cpu().numpy() if torch.is_tensor(bbox) else np.asarray(bbox)
    voxel_size = list((bbox[1] - bbox[0]) / np.array(pytorch_3d_sdf_tensor.shape))
    verts, faces = marching_cubes(pytorch_3d_sdf_tensor, level, spacing=voxel_size, flip=True)
    verts, faces = verts.cpu().numpy(), faces.cpu().numpy()
    pts = mesh_points(verts, bbox, offset, scale)
    print("saving mesh to %s" % (ply_filename_out))
    write_ply(ply_filename_out, pts, faces)
    return pts, faces
