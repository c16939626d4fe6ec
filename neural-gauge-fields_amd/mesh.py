"""Mesh export on the GPU: marching cubes over a dense float volume (csrc/ngf_mesh.hip), the reference's
``convert_sdf_samples_to_ply`` (TriPlane/utils.py:179-239) on top of it, and a binary PLY writer in numpy (there is no ``plyfile``).

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
