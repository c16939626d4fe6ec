"""``NeuTex`` -- drop-in for the colour path of the reference's UV-Mapping model (UV-Mapping/model/model.py:11-59).

Same sub-module and parameter names as the reference (``net_geometry_decoder.block.*``,
``gauge_transform.encoder.*``, ``net_texture.{block1,color1,block2}.*``, ``inverse_gauge.inverse_network.*``) so its
``{epoch}_net_NeuTex.pth`` checkpoints load with ``strict=True`` (``load_params`` keeps ``strict=False`` for parameter sets without
the inverse network).
``forward`` returns the reference's ``color`` / ``transmittance`` outputs; the three MLPs, the cube ray generation
and the ray march run in one HIP kernel (include/ngf.h: ngf_uv_render).

The reference jitters the segment lengths with ``torch.rand`` even at test time (model.py:30); pass ``jitter_u``
([N,R,S] uniforms) for reproducible output, otherwise they are drawn on the device.

Texture export: ``net.net_texture.export_textures`` / ``_export_cube`` / ``_export_sphere`` / ``_export_square`` (decoder.py:123-179) and the
general ``NeuTex.texture_colors`` run the texture MLP on explicit points in a HIP kernel of their own (include/ngf.h: ngf_uv_texture_eval);
``merge_cube_to_single_texture`` (util.py:286-312) lays a cube export out as the cross image the reference's test driver saves.

Point queries: ``NeuTex.query`` (density, gauge uv, colour at world points), ``NeuTex.density_lattice`` and ``NeuTex.export_mesh`` (an OBJ whose
``vt`` coordinates map the exported atlas onto the marching-cubes surface) run the three MLPs on explicit points in a HIP kernel of their own
(include/ngf.h: ngf_uv_query, ngf_uv_density_lattice).

Occupancy grid: ``NeuTex.build_occupancy`` reduces a density lattice to one bit per cell on the device and installs it; the render kernel then
evaluates only the in-cube samples whose cell is occupied (include/ngf.h: ngf_uv_occupancy_from_lattice, ngf_uv_set_occupancy; DESIGN.md section
4.14).  Opt-in: the masked frame is the reference's frame with sigma set to 0 in empty cells.  ``set_occupancy`` / ``occupancy`` / ``occupied`` /
``occupancy_state`` / ``load_occupancy`` are the rest of the surface.

Inverse gauge: ``NeuTex.inverse_map`` (template point -> world point), ``NeuTex.cycle_error`` and ``NeuTex.coordinate_deformation`` (the
reference's deformed-template mesh, model.py:383-418) run ``inverse_gauge.inverse_network`` in a HIP kernel of its own (include/ngf.h:
ngf_uv_inverse_map).  They build no graph.  With ``net.inverse_gauge.differentiable = True`` (an attribute, never saved),
grad enabled and the parameters on a GPU, ``InverseGauge.forward`` and ``InverseGauge.map`` -- the origin loss's template points and
``points_inverse`` -- run the same network forwards and backwards on HIP kernels too (uv_inverse_train.py, include/ngf.h:
ngf_uv_inverse_trainer_*); otherwise they are plain torch.

Training: with ``net.differentiable = True`` (an attribute, never saved) and grad enabled, ``forward`` returns the reference's training dict
with a graph over every parameter (uv_train.py, include/ngf.h: ngf_uv_trainer_*).  Off, or under ``torch.no_grad()``, it is the eval path.
With ``net.occupancy_in_training = True`` as well (an attribute, never saved) it trains through the installed occupancy mask: empty cells are
neither evaluated nor given a gradient (include/ngf.h: ngf_uv_trainer_set_occupancy).
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _engine, _lib


def _seq(dims, act):
    layers = []
    for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        layers.append(nn.Linear(a, b))
        if i < len(dims) - 2 or act[1]:
            layers.append(act[0]())
    return nn.Sequential(*layers)


class GeometryMlpDecoder(nn.Module):
    """decoder.py:201-217 (parameter container; evaluated inside the kernel)."""

    def __init__(self, pos_freqs=10, hidden_size=256, num_layers=10):
        super().__init__()
        if (pos_freqs, hidden_size, num_layers) != (10, 256, 10):
            raise ValueError("the gfx950 kernel implements GeometryMlpDecoder(10, 256, 10) (model.py:16)")
        dims = [3 + 6 * pos_freqs] + [hidden_size] * (num_layers + 1) + [1]
        self.block = _seq(dims, (nn.ReLU, False))


class GaugeNetwork(nn.Module):
    """gauge_fields.py:8-34."""

    def __init__(self, input_dim, output_dim, mid_size=64, hidden_size=128, num_layers=2):
        super().__init__()
        self.linear1 = nn.Linear(input_dim + 2 * input_dim * 10, mid_size)
        self.linear2 = nn.Linear(mid_size, hidden_size)
        self.linear_list = nn.ModuleList([nn.Linear(hidden_size, hidden_size) for _ in range(num_layers)])
        self.last_linear = nn.Linear(hidden_size, output_dim)


class GaugeTransform(nn.Module):
    """gauge_fields.py:49-58."""

    def __init__(self, primitive_type):
        super().__init__()
        self.output_dim = 2 if primitive_type == 'square' else 3
        self.encoder = GaugeNetwork(3, self.output_dim)


# --- the sample points of the texture exporters (decoder.py:123-170), built as the reference builds them so that they are its points bit for bit:
# float64 numpy grids rounded to float32 once, the cube faces normalised in float32 on the CPU.  A few MB per export, not the hot path.
def _cell_centres(resolution):
    """generate_grid(2, R) (util.py:13-16): [R,R,2] cell centres in (-1,1), 'ij' order, float64."""
    a = np.arange(resolution)
    grid = np.stack(np.meshgrid(a, a, indexing="ij"), axis=-1)
    return (2 * grid + 1) / resolution - 1


def export_square_points(resolution):
    """[R,R,2] float32: the points of ``_export_square``; texel [i,j] is evaluated at uv = (centre i, centre j)."""
    return torch.tensor(_cell_centres(resolution)).float()


def export_cube_points(resolution):
    """[6,R,R,3] float32: the points of ``_export_cube`` -- convert_cube_uv_to_xyz (util.py:134-164) of the cell centres per face."""
    vc, uc = export_square_points(resolution).unbind(-1)
    one = torch.ones_like(uc)
    faces = ((one, vc, -uc), (-one, vc, uc), (uc, one, -vc), (uc, -one, vc), (uc, vc, one), (-uc, vc, -one))
    return torch.stack([F.normalize(torch.stack(f, dim=-1), dim=-1) for f in faces], dim=0)


def export_sphere_points(resolution):
    """[R,2R,3] float32: the equirectangular directions of ``_export_sphere``, before its final ``flip(0)``."""
    grid = np.stack(np.meshgrid(np.arange(2 * resolution), np.arange(resolution), indexing="xy"), axis=-1)
    grid = grid / np.array([2 * resolution, resolution]) * np.array([2 * np.pi, np.pi]) + np.array([np.pi, 0])
    x, y = grid[..., 0], grid[..., 1]
    return torch.tensor(np.stack([-np.sin(x) * np.sin(y), -np.cos(y), -np.cos(x) * np.sin(y)], -1)).float()


def merge_cube_to_single_texture(cube, flip=True, rotate=True):
    """util.py:286-312: a [6,R,R,C] cube export laid out as a [3R,4R,C] cross (unused cells 1); pure indexing on ``cube``'s device."""
    assert cube.shape[0] == 6 and cube.shape[1] == cube.shape[2]
    res = cube.shape[1]
    result = torch.ones((3 * res, 4 * res, cube.shape[-1]), dtype=cube.dtype, device=cube.device)
    if flip:
        cube = cube.flip(1)
    row = [0, 5, 1, 4] if rotate else [1, 4, 0, 5]
    for k, face in enumerate(row):
        result[res:2 * res, k * res:(k + 1) * res] = cube[face]
    result[:res, res:2 * res] = cube[2].flip(0, 1) if rotate else cube[2]
    result[2 * res:, res:2 * res] = cube[3].flip(0, 1) if rotate else cube[3]
    return result


class TextureMlpDecoder(nn.Module):
    """decoder.py:11-58: the MLPs; ``cubemap_`` / ``cubemap_mode_`` (texture editing) are plain attributes as in the
    reference and are pushed to the device by NeuTex.set_target_texture.  The exporters (decoder.py:123-179) are thin callers of the owning
    NeuTex's ``texture_colors``: the MLP runs in the HIP kernel behind it, on the owner's handle (``_owner``: a weak reference set by
    NeuTex.__init__, a plain attribute -- no parameter, buffer or state-dict key)."""

    def __init__(self, uv_dim, width=256):
        super().__init__()
        self.cubemap_ = None
        self.cubemap_mode_ = 0
        self.uv_dim = uv_dim
        self._owner = None
        self._points = {}                # kind -> (resolution, device, points): the last export's sample points stay on the device
        self.block1 = _seq([uv_dim + 20 * uv_dim] + [width] * 6, (lambda: nn.LeakyReLU(0.2), True))
        self.color1 = nn.Linear(width, 3)
        self.block2 = _seq([width + 3 + 36] + [width] * 4 + [3], (lambda: nn.LeakyReLU(0.2), False))

    def __getstate__(self):              # (a weak reference does not pickle; NeuTex.__setstate__ restores it)
        d = self.__dict__.copy()
        d["_owner"], d["_points"] = None, {}
        return d

    def _net(self):
        net = self._owner() if self._owner is not None else None
        if net is None:
            raise RuntimeError("this TextureMlpDecoder belongs to no live NeuTex: the exporters run on the owning model's GPU handle (keep the model alive)")
        if torch.device(net.device).type != 'cuda':
            raise RuntimeError("ngf_amd NeuTex exports textures on the GPU only (device='cuda'); there is no CPU path")
        return net

    def _export(self, kind, build, resolution, viewdir):
        net = self._net()
        dev = torch.device(net.device)
        hit = self._points.get(kind)
        if hit is None or hit[0] != int(resolution) or hit[1] != dev:
            hit = (int(resolution), dev, build(int(resolution)).to(dev))
            self._points[kind] = hit
        return net.texture_colors(hit[2], viewdir, diffuse=viewdir is None)

    def _export_cube(self, resolution, viewdir):
        """[6,R,R,3]; ``viewdir`` a 3-vector (used as given, not normalised) or None for the diffuse texture sigmoid(color1)."""
        return self._export("cube", export_cube_points, resolution, viewdir)

    def _export_sphere(self, resolution, viewdir):
        """[R,2R,3] equirectangular."""
        return self._export("sphere", export_sphere_points, resolution, viewdir).flip(0)

    def _export_square(self, resolution, viewdir):
        """[R,R,3], indexed [i <-> uv[...,0], j <-> uv[...,1]] as the reference's (the transpose of what sample_square reads back)."""
        return self._export("square", export_square_points, resolution, viewdir)

    def export_textures(self, resolution=512, viewdir=[0, 0, 1]):
        return self._export_cube(resolution, viewdir) if self.uv_dim == 3 else self._export_square(resolution, viewdir)


class InverseNetwork(nn.Module):
    """gauge_fields.py:78-119 (modified AtlasNet core): template point (2|3) -> 64 -> 512 -> 512 -> 512 -> xyz, ReLU.  This module is the
    torch path of training (the template points of the origin loss, ``points_inverse``); with ``InverseGauge.differentiable`` set the same
    weights train through HIP kernels (uv_inverse_train.py), and without a graph they run in one through ``NeuTex.inverse_map``."""

    def __init__(self, input_point_dim, mid_size=64, hidden_size=512, num_layers=2):
        super().__init__()
        self.input_size = input_point_dim
        self.linear1 = nn.Linear(input_point_dim, mid_size)
        self.linear2 = nn.Linear(mid_size, hidden_size)
        self.linear_list = nn.ModuleList([nn.Linear(hidden_size, hidden_size) for _ in range(num_layers)])
        self.last_linear = nn.Linear(hidden_size, 3)

    def forward(self, x):
        x = F.relu(self.linear1(x))
        x = F.relu(self.linear2(x))
        for lin in self.linear_list:
            x = F.relu(lin(x))
        return self.last_linear(x)


# the launch shape of ngf_uv_inverse_map (csrc/ngf_uv_inverse.hpp: kUvInvTilePoints, kUvInvWaves; tests/test_uv_inverse_cpu.py compares): a wave
# pass takes 16 points, a block has four waves, the grid is capped at the CU count -- one full grid of passes is their product
INVERSE_TILE_POINTS, INVERSE_WAVES_PER_BLOCK = 16, 4


class InverseGauge(nn.Module):
    """gauge_fields.py:164-207.  ``forward(template_points=None)`` -> (input points [P,D], output points [1,1,P,3]); the points are drawn as
    SquareTemplate / SphereTemplate.get_random_points do, on the parameters' device.  ``map(uv)`` [..., D] -> [..., 3]: the reference's
    ``uv.view(input_shape, -1, D)`` raises in torch, so the evident intent -- the network on the flattened points -- is what runs here."""

    def __init__(self, num_points_per_primitive, primitive_type="square"):
        super().__init__()
        if primitive_type not in ("square", "sphere"):
            raise ValueError(f"Unknown primitive type {primitive_type}")
        self.primitive_type = primitive_type
        self.input_point_dim = 2 if primitive_type == "square" else 3
        self.num_points_per_primitive = int(num_points_per_primitive)
        self.inverse_network = InverseNetwork(self.input_point_dim)

    def layers(self):
        """The five Linear layers of the inverse network in the order of ngf_uv_inverse_desc (the one list: NeuTex.inverse_layers() and
        uv_inverse_train.inverse_params() are built on it)."""
        n = self.inverse_network
        return [n.linear1, n.linear2, n.linear_list[0], n.linear_list[1], n.last_linear]

    def random_points(self, n):
        dev = self.inverse_network.linear1.weight.device
        with torch.no_grad():
            if self.primitive_type == "square":
                return torch.rand((n, 2), device=dev) * 2 - 1
            return F.normalize(torch.randn((n, 3), device=dev) * 2 - 1, dim=-1)

    def forward(self, template_points=None):
        pts = self.random_points(self.num_points_per_primitive) if template_points is None else template_points
        if self._on_kernels() and pts.numel():          # (an empty batch is torch's: same empty result, same graph, no engine)
            return pts, self._map_hip('_template_engine', pts).view(1, 1, -1, 3)
        return pts, self.inverse_network(pts.unsqueeze(0)).unsqueeze(1).contiguous()

    def map(self, uv):
        assert uv.shape[-1] == self.input_point_dim
        if self._on_kernels() and uv.numel():
            return self._map_hip('_map_engine', uv).view(uv.shape[:-1] + (3,))
        out = self.inverse_network(uv.reshape(-1, self.input_point_dim))
        return out.view(uv.shape[:-1] + (3,))

    # --- training on the HIP kernels (uv_inverse_train.py) ---------------------------------------------------
    differentiable = False          # training switch, as NeuTex.differentiable: a plain attribute, never saved
    _template_engine = None         # one engine per call site: the template points of ``forward`` and the uv of ``map`` meet in one
    _map_engine = None              # iteration, and a shared engine would make each other's tickets stale (a third forward per step)

    def _on_kernels(self):
        """``differentiable`` set, grad enabled and the parameters on a GPU; else ``forward`` and ``map`` are the torch code above."""
        return self.differentiable and torch.is_grad_enabled() and self.inverse_network.linear1.weight.is_cuda

    def _inverse_engine(self, attr, n):
        from .uv_inverse_train import InverseGrad, inverse_params
        return _engine.grad_engine(self, attr, InverseGrad, inverse_params(self), int(n), 1)

    def _map_hip(self, attr, pts):
        from .uv_inverse_train import _InverseMap
        dev = self.inverse_network.linear1.weight.device
        x = pts.to(dev, torch.float32).reshape(-1, self.input_point_dim).contiguous()
        eng = self._inverse_engine(attr, x.shape[0])
        return _InverseMap.apply(self, attr, eng, x, *eng.params)

    def inverse_grad_engines(self):
        """The training engines (uv_inverse_train.InverseGrad: max_rays = points, bytes, forwards) of ``forward`` and ``map``, or None each."""
        return self._template_engine, self._map_engine

    def release_inverse_grad_engines(self):
        """Free both engines' per-point buffers (the next differentiable call builds a new one)."""
        _engine.release_engine(self, '_template_engine')
        _engine.release_engine(self, '_map_engine')

    def __getstate__(self):              # engines are not state: not pickled, not deep-copied (they are not in state_dict either)
        d = self.__dict__.copy()
        d.pop('_template_engine', None)
        d.pop('_map_engine', None)
        return d

    def __del__(self):
        try:
            self.release_inverse_grad_engines()
        except Exception:
            pass


def lattice_axes(resolution, lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0)):
    """``(res, lo, step)`` of NeuTex.density_lattice: ``resolution`` an int or a triple (at least 2 per axis), ``step = (hi - lo) / (n - 1)`` in
    float32.  The last point must REACH hi (at hi = 1 the clip then zeroes that slab and an iso-surface closes): where the rounded step falls
    short -- ``lo + float32(n - 1) * step`` lands an ulp inside for 137 of the sizes up to 1024, 42 the first -- it is taken one ulp longer."""
    res = (int(resolution),) * 3 if np.ndim(resolution) == 0 else tuple(int(r) for r in resolution)
    if len(res) != 3 or min(res) < 2:
        raise ValueError(f"resolution must be an int or a triple, at least 2 per axis, got {resolution!r}")
    lo32, hi32 = np.asarray(lo, dtype=np.float32).reshape(3), np.asarray(hi, dtype=np.float32).reshape(3)
    last = np.asarray(res, dtype=np.float32) - np.float32(1)
    step = (hi32 - lo32) / last
    top = lo32 + last * step          # (float32: the product rounded, then the sum -- the kernel's arithmetic)
    short = np.where(step > 0, top < hi32, top > hi32)
    step = np.where(short, np.nextafter(step, np.copysign(np.float32(np.inf), step)), step)
    assert step.dtype == np.float32
    return res, lo32, step


OCCUPANCY_MAX_AXIS, OCCUPANCY_MAX_DILATE = 1024, 2          # csrc/ngf_uv_occupancy.hpp: kUvOccMaxAxis, kUvOccMaxDilate


def _occupancy_shape(shape):
    """``shape`` as a triple of cell counts, each 1 .. 1024 (an int means a cube)."""
    res = (int(shape),) * 3 if np.ndim(shape) == 0 else tuple(int(r) for r in shape)
    if len(res) != 3 or min(res) < 1 or max(res) > OCCUPANCY_MAX_AXIS:
        raise ValueError(f"an occupancy grid has three axes of 1 .. {OCCUPANCY_MAX_AXIS} cells, got {shape!r}")
    return res


class Occupancy:
    """The occupancy grid of a NeuTex (``NeuTex.occupancy``): ``shape`` = (nx, ny, nz) cells over the cube [-1,1]^3, ``bits`` = the packed mask on
    the model's device (uint8, ``np.packbits`` order over the C-ordered cells, tail bits 0), ``threshold`` / ``dilate`` = what ``build_occupancy``
    built it with (None for a mask that was set or loaded)."""

    def __init__(self, bits, shape, threshold=None, dilate=None):
        self.bits, self.shape, self.threshold, self.dilate = bits, tuple(shape), threshold, dilate

    @property
    def cells(self):
        return self.shape[0] * self.shape[1] * self.shape[2]

    def volume(self):
        """The mask as a bool volume [nx,ny,nz] on the bits' device."""
        shifts = torch.arange(7, -1, -1, device=self.bits.device, dtype=torch.int32)
        flat = ((self.bits.to(torch.int32)[:, None] >> shifts) & 1).reshape(-1)[:self.cells]
        return flat.bool().view(self.shape)

    def fraction(self):
        """Occupied cells / all cells."""
        return float(self.volume().sum().item()) / self.cells


class NeuTex(nn.Module):
    def __init__(self, opt=None, primitive_type=None, sample_num=None, device='cuda', split_bf16=False, points_per_primitive=None):
        super().__init__()
        self.opt = opt
        self.split_bf16 = bool(split_bf16)          # NGF_UV_F_SPLIT_BF16: 256-unit layers as 3-term split bf16 MFMA products (opt-in)
        self.primitive_type = primitive_type or getattr(opt, 'primitive_type', 'square')
        self.sample_num = int(sample_num or getattr(opt, 'sample_num', 64))
        self.device = device
        self.net_geometry_decoder = GeometryMlpDecoder(pos_freqs=10, hidden_size=256, num_layers=10)
        self.gauge_transform = GaugeTransform(self.primitive_type)
        self.net_texture = TextureMlpDecoder(2 if self.primitive_type == 'square' else 3)
        self.net_texture._owner = weakref.ref(self)
        ppp = points_per_primitive if points_per_primitive is not None else getattr(opt, 'points_per_primitive', None)
        self.inverse_gauge = InverseGauge(2500 if ppp is None else int(ppp), self.primitive_type)
        self.differentiable = False          # training switch (uv_train.py): an attribute, not a parameter or buffer; never saved
        self._uv_engine = None
        self._handle = None
        self._key = None
        self._inv_handle = None
        self._inv_key = None
        self._occ = None                     # the occupancy grid (an Occupancy): the user's, not a buffer -- see build_occupancy
        self.to(device)

    def layers(self):
        """The 29 Linear layers in the order of ngf_uv_desc."""
        g = [m for m in self.net_geometry_decoder.block if isinstance(m, nn.Linear)]
        e = self.gauge_transform.encoder
        ga = [e.linear1, e.linear2, e.linear_list[0], e.linear_list[1], e.last_linear]
        t1 = [m for m in self.net_texture.block1 if isinstance(m, nn.Linear)]
        t2 = [m for m in self.net_texture.block2 if isinstance(m, nn.Linear)]
        out = g + ga + t1 + [self.net_texture.color1] + t2
        assert len(out) == _lib.UV_LAYERS
        return out

    def load_params(self, params: dict):
        sd = {k: torch.as_tensor(v) for k, v in params.items()}
        self.load_state_dict(sd, strict=False)
        self.to(self.device)

    # --- texture editing (decoder.py:52-58, 79-121): net_texture.cubemap_ / cubemap_mode_ -------------------------------
    def set_target_texture(self, cubemap, mode=0):
        """``net_texture.cubemap_ = cubemap; net_texture.cubemap_mode_ = mode`` of the reference: a [6,R,R,C] cube map
        (sphere) or an [H,W,C] image (square), values in [0,1], C = 3 or 4 (what load_cube_from_single_texture /
        load_square return, util.py:240-275); ``None`` switches editing off."""
        self.net_texture.cubemap_ = None if cubemap is None else torch.as_tensor(cubemap, dtype=torch.float32)
        self.net_texture.cubemap_mode_ = int(mode)
        if self._handle is not None:
            self._push_texture()

    def _push_texture(self):
        t = getattr(self.net_texture, "cubemap_", None)
        dev = torch.device(self.device)
        with torch.cuda.device(dev):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            if t is None:
                _lib.check(_lib.lib().ngf_uv_set_texture(self._handle, None, 0, 0, 0, 0, 0, st))
                return
            t = t.to(dev, torch.float32).contiguous()
            faces = 6 if t.dim() == 4 else 1
            H, W, Cn = (t.shape[1], t.shape[2], t.shape[3]) if t.dim() == 4 else tuple(t.shape)
            _lib.check(_lib.lib().ngf_uv_set_texture(self._handle, t.data_ptr(), faces, int(H), int(W), int(Cn), int(self.net_texture.cubemap_mode_), st))
            torch.cuda.current_stream().synchronize()        # the library copied from `t`; it may be freed now

    @torch.no_grad()
    def texture_edit(self, uv, original_color):
        """The edit stage alone (decoder.py:95-121): uv [n,3] (gauge output; z ignored for square models), original_color
        = color1 + color2 [n,3] -> [n,3]."""
        dev = torch.device(self.device)
        uv = uv.to(dev, torch.float32).contiguous()
        oc = original_color.to(dev, torch.float32).contiguous()
        out = torch.empty_like(oc)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().ngf_uv_texture_edit(self.handle(), uv.data_ptr(), oc.data_ptr(), uv.shape[0], out.data_ptr(),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return out

    @torch.no_grad()
    def texture_colors(self, uv, view_dir=None, diffuse=False):
        """TextureMlpDecoder.forward (decoder.py:56-121) on explicit points: uv [..., D] (D = 3; a square model also takes D = 2 and ignores z)
        and ``view_dir``, one 3-vector shared by all points or [..., 3] per point, used as given -> [..., 3] on the model's device:
        ``(softplus(color1) + color2).clamp(min=0)``, through the edit stage when a target texture is set.  ``diffuse=True`` is the exporters'
        viewdir=None branch, ``sigmoid(color1(block1(uv)))``: no view direction, no edit stage."""
        dev = torch.device(self.device)
        if dev.type != 'cuda':
            raise RuntimeError("ngf_amd NeuTex exports textures on the GPU only (device='cuda'); there is no CPU path")
        uv = torch.as_tensor(uv)
        D = uv.shape[-1]
        if D != 3 and not (D == 2 and self.primitive_type == 'square'):
            raise ValueError(f"uv must be [..., 3]{' or [..., 2]' if self.primitive_type == 'square' else ''}, got {tuple(uv.shape)}")
        lead = tuple(uv.shape[:-1])
        pts = uv.detach().to(dev, torch.float32).reshape(-1, D)
        if D == 2:
            pts = torch.cat([pts, pts.new_zeros((pts.shape[0], 1))], dim=-1)
        pts = pts.contiguous()
        n = pts.shape[0]
        view, stride = None, 0
        if not diffuse:
            if view_dir is None:
                raise ValueError("texture_colors needs a view direction unless diffuse=True")
            view = torch.as_tensor(view_dir).detach().to(dev, torch.float32)
            if view.shape[-1] != 3:
                raise ValueError(f"view_dir must be a 3-vector or [..., 3], got {tuple(view.shape)}")
            if view.numel() == 3:
                view = view.reshape(3).contiguous()
            else:
                view, stride = view.expand(lead + (3,)).reshape(-1, 3).contiguous(), 3
        out = torch.empty((n, 3), device=dev)
        if n:
            h = self.handle()
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().ngf_uv_texture_eval(h, pts.data_ptr(), None if view is None else view.data_ptr(), stride, n,
                                                          _lib.UV_TEX_DIFFUSE if diffuse else 0, out.data_ptr(),
                                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return out.view(lead + (3,))

    # --- point queries and the UV-textured mesh (include/ngf.h: ngf_uv_query, ngf_uv_density_lattice) ------------------
    def _gpu(self, what):
        dev = torch.device(self.device)
        if dev.type != 'cuda':
            raise RuntimeError(f"ngf_amd NeuTex {what} on the GPU only (device='cuda'); there is no CPU path")
        return dev

    @torch.no_grad()
    def query(self, xyz, viewdirs=None, *, want=('sigma', 'uv', 'rgb'), diffuse=False, clip=True):
        """The model at world points ``xyz`` [..., 3]: a dict with the entries named in ``want`` --
        ``sigma`` [...]: ``net_geometry_decoder(pts)["density"]``, exactly 0 outside the open cube (-1,1)^3 unless ``clip=False``;
        ``uv`` [..., D] (D = 3 sphere, 2 square): ``gauge_transform(pts)``; ``rgb`` [..., 3]: ``net_texture(uv, viewdirs)`` at that uv, with
        ``viewdirs`` one 3-vector or [..., 3], used as given, or ``diffuse=True`` for the exporters' viewdir=None colour -- bit for bit
        ``texture_colors(uv, viewdirs)``.  A part that is not wanted does not run (``uv`` alone costs 6 % of the three).  fp32 whatever the
        model's ``split_bf16``; a point's values do not depend on the other points or on the other entries of ``want``."""
        dev = self._gpu("answers point queries")
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or any(w not in ('sigma', 'uv', 'rgb') for w in want):
            raise ValueError(f"want must name some of 'sigma', 'uv', 'rgb', got {want!r}")
        xyz = torch.as_tensor(xyz)
        if xyz.shape[-1] != 3:
            raise ValueError(f"xyz must be [..., 3], got {tuple(xyz.shape)}")
        lead = tuple(xyz.shape[:-1])
        pts = xyz.detach().to(dev, torch.float32).reshape(-1, 3).contiguous()
        n = pts.shape[0]
        view, stride = None, 0
        if 'rgb' in want and not diffuse:
            if viewdirs is None:
                raise ValueError("query needs viewdirs for 'rgb' unless diffuse=True")
            view = torch.as_tensor(viewdirs).detach().to(dev, torch.float32)
            if view.shape[-1] != 3:
                raise ValueError(f"viewdirs must be a 3-vector or [..., 3], got {tuple(view.shape)}")
            if view.numel() == 3:
                view = view.reshape(3).contiguous()
            else:
                view, stride = view.expand(lead + (3,)).reshape(-1, 3).contiguous(), 3
        sigma = torch.empty((n,), device=dev) if 'sigma' in want else None
        uv = torch.empty((n, 3), device=dev) if 'uv' in want else None
        rgb = torch.empty((n, 3), device=dev) if 'rgb' in want else None
        if n:
            h = self.handle()
            flags = (_lib.UV_TEX_DIFFUSE if diffuse else 0) | (0 if clip else _lib.UV_QUERY_NO_CLIP)
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().ngf_uv_query(h, pts.data_ptr(), n, None if view is None else view.data_ptr(), stride, flags,
                                                   None if sigma is None else sigma.data_ptr(), None if uv is None else uv.data_ptr(),
                                                   None if rgb is None else rgb.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        out = {}
        if sigma is not None:
            out['sigma'] = sigma.view(lead)
        if uv is not None:
            D = 2 if self.primitive_type == 'square' else 3
            out['uv'] = uv[:, :D].reshape(lead + (D,))
        if rgb is not None:
            out['rgb'] = rgb.view(lead + (3,))
        return out

    @torch.no_grad()
    def density_lattice(self, resolution, lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), clip=True):
        """The density on the lattice of ``resolution`` (an int or a triple, >= 2 per axis) points from ``lo`` to ``hi``: ``(volume [nx,ny,nz],
        lo, step)`` with ``step = (hi - lo) / (n - 1)`` in float32 (numpy arrays; an ulp longer where the last point would stop short of hi) and ``volume[i,j,k]`` the density at ``lo + (i,j,k) * step``,
        every product and every sum rounded to float32 -- the layout and spacing ``mesh.marching_cubes`` takes.  The kernel generates the
        points; with ``clip`` a lattice that reaches the faces of the cube is 0 there (``query``'s clip), so an iso-surface closes."""
        res, lo32, step = lattice_axes(resolution, lo, hi)
        return self._lattice(res, lo32, step, clip), lo32, step

    def _lattice(self, res, lo32, step, clip):
        """ngf_uv_density_lattice on ``res`` points per axis from ``lo32`` in steps of ``step`` (float32 triples) -> the volume on the device."""
        dev = self._gpu("evaluates density lattices")
        vol = torch.empty(res, device=dev)
        h = self.handle()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().ngf_uv_density_lattice(h, (C.c_float * 3)(*lo32.tolist()), (C.c_float * 3)(*step.tolist()), res[0], res[1], res[2],
                                                         0 if clip else _lib.UV_QUERY_NO_CLIP, vol.data_ptr(),
                                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return vol

    # --- the occupancy grid: the render skips empty space (include/ngf.h: ngf_uv_occupancy_*, ngf_uv_set_occupancy) ------
    @property
    def occupancy(self):
        """None when no mask is installed, else the ``Occupancy`` (``shape``, ``bits``, ``threshold``, ``dilate``, ``fraction()``, ``volume()``)."""
        return self._occ

    @torch.no_grad()
    def build_occupancy(self, resolution=128, alpha_thres=1e-3, threshold=None, dilate=1):
        """Build the occupancy grid from the model's own density, install it and return it.  ``resolution``: cells per axis, an int or a triple
        (1 .. 1024 each).  The density is evaluated on the cells' corners -- ``(n + 1)`` points per axis from -1 in steps of ``float32(2 / n)``,
        not clipped -- and a cell is occupied iff some cell within Chebyshev distance ``dilate`` (0, 1 or 2) of it has a corner with
        ``not (sigma <= threshold)``.  With ``threshold=None`` the sigma threshold is ``float32(-log1p(-alpha_thres) / (2 / sample_num))``: the
        density whose opacity over one nominal segment is ``alpha_thres`` (the fields' ``alphaMask_thres``).  Lattice and reduction run on the device.

        With a mask installed the eval render evaluates a sample only where it is in the cube AND its cell is occupied; every other sample
        contributes what an out-of-cube sample does (opacity 0, colour 0, zeros in the debug outputs).  The masked frame is therefore, by
        definition, the reference's frame with sigma set to 0 in empty cells -- NOT the reference's frame, which is why the mask is opt-in.
        An evaluated sample's density and colour are the same bits as without a mask.

        The mask belongs to the user: it is not rebuilt when a parameter changes (call ``build_occupancy`` again after training), it survives a
        rebuild of the handle and pickling, and it is no buffer (``state_dict`` does not hold it: ``occupancy_state`` / ``load_occupancy``).
        ``query``, ``density_lattice`` and the texture calls ignore it, and so does the differentiable path (``differentiable = True`` with grad
        enabled) unless ``occupancy_in_training`` is set.

        Training through the mask (``net.occupancy_in_training = True``, off by default): the differentiable forward
        then evaluates the geometry and texture networks only on the in-cube samples of occupied cells -- the eval render's decision on the same
        batch -- and every other sample has sigma 0, blend weight exactly 0 and no gradient into those networks (the gauge network still runs
        on every sample: ``uv`` does not depend on the mask).  The mask is still never rebuilt behind the user's back.  A cell masked empty
        gets no gradient, so its density cannot rise again by training alone: build the mask after a warm-up, and rebuild it every so often.
        ``build_occupancy`` evaluates the WHOLE lattice, masked cells included, so cells can come back."""
        dev = self._gpu("builds occupancy grids")
        n = _occupancy_shape(resolution)
        dilate = int(dilate)
        if not 0 <= dilate <= OCCUPANCY_MAX_DILATE:
            raise ValueError(f"dilate must be 0 .. {OCCUPANCY_MAX_DILATE}, got {dilate}")
        if threshold is None:
            if not 0.0 <= float(alpha_thres) < 1.0:
                raise ValueError(f"alpha_thres must be in [0, 1), got {alpha_thres!r}")
            threshold = -np.log1p(-float(alpha_thres)) / (2.0 / self.sample_num)
        threshold = float(np.float32(threshold))
        if np.isnan(threshold):
            raise ValueError("the occupancy threshold is NaN")
        step = (np.float32(2.0) / np.asarray(n, dtype=np.float32)).astype(np.float32)
        sigma = self._lattice(tuple(k + 1 for k in n), np.full(3, -1.0, np.float32), step, clip=False)
        bits = self._occupancy_reduce(sigma, n, threshold, dilate)
        self._occ = Occupancy(bits, n, threshold, dilate)
        if self._handle is not None:
            self._push_occupancy()
        return self._occ

    def _occupancy_reduce(self, sigma, n, threshold, dilate):
        """ngf_uv_occupancy_from_lattice: the float32 lattice [(nx+1),(ny+1),(nz+1)] on the device -> the packed bits on the device."""
        dev = sigma.device
        L = _lib.lib()
        bits = torch.empty(((n[0] * n[1] * n[2] + 7) // 8,), dtype=torch.uint8, device=dev)
        need = int(L.ngf_uv_occupancy_workspace_bytes(n[0], n[1], n[2]))
        if need < 0:
            _lib.check(-need)
        ws = torch.empty((need,), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(L.ngf_uv_occupancy_from_lattice(sigma.data_ptr(), n[0], n[1], n[2], threshold, dilate, bits.data_ptr(), ws.data_ptr(), need,
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.current_stream().synchronize()          # (the workspace may be freed now)
        return bits

    def set_occupancy(self, mask):
        """Install a mask: ``None`` (off), a bool or uint8 volume [nx,ny,nz] (tensor or numpy; non-zero = occupied), or a ``(packed_bits, shape)``
        pair -- ``np.packbits`` of the C-ordered cells, ``(nx ny nz + 7) // 8`` bytes with the tail bits 0.  See ``build_occupancy`` for what a
        mask does to the render."""
        if mask is None:
            self._occ = None
        else:
            if isinstance(mask, tuple) and len(mask) == 2:
                packed, shape = mask
                shape = _occupancy_shape(shape)
                packed = packed.detach().cpu().numpy() if torch.is_tensor(packed) else np.asarray(packed)
                cells = shape[0] * shape[1] * shape[2]
                if packed.dtype != np.uint8 or packed.ndim != 1 or packed.shape[0] != (cells + 7) // 8:
                    raise ValueError(f"the packed bits of a {shape} grid are {(cells + 7) // 8} uint8 values, got {packed.dtype} {packed.shape}")
                if cells % 8 and int(packed[-1]) & ((1 << (8 - cells % 8)) - 1):
                    raise ValueError("the tail bits of the last byte must be 0")
            else:
                vol = mask.detach().cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)
                if vol.ndim != 3 or vol.dtype not in (np.bool_, np.uint8):
                    raise ValueError(f"a mask is a bool or uint8 volume [nx,ny,nz] or a (packed_bits, shape) pair, got {vol.dtype} {vol.shape}")
                shape = _occupancy_shape(vol.shape)
                packed = np.packbits(vol.reshape(-1) != 0)
            self._occ = Occupancy(torch.from_numpy(np.ascontiguousarray(packed)).to(torch.device(self.device)), shape)
        if self._handle is not None:
            self._push_occupancy()
        return self._occ

    def _push_occupancy(self):
        """The mask -> the handle (beside _push_texture: after every rebuild of the handle, and when the mask changes)."""
        dev = torch.device(self.device)
        with torch.cuda.device(dev):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            if self._occ is None:
                _lib.check(_lib.lib().ngf_uv_set_occupancy(self._handle, None, 0, 0, 0, st))
                return
            self._occ.bits = self._occ.bits.to(dev).contiguous()
            n = self._occ.shape
            _lib.check(_lib.lib().ngf_uv_set_occupancy(self._handle, self._occ.bits.data_ptr(), n[0], n[1], n[2], st))
            torch.cuda.current_stream().synchronize()          # the library copied the bits

    @torch.no_grad()
    def occupied(self, xyz):
        """bool [...] for world points ``xyz`` [..., 3]: the point passes the render's strict in-cube test and its cell's bit is set -- the
        render kernel's own look-up, cell ``min(int(floor((p + 1) * n / 2)), n - 1)`` per axis in float32."""
        dev = self._gpu("looks up occupancy")
        if self._occ is None:
            raise RuntimeError("no occupancy mask is installed (build_occupancy / set_occupancy)")
        xyz = torch.as_tensor(xyz)
        if xyz.shape[-1] != 3:
            raise ValueError(f"xyz must be [..., 3], got {tuple(xyz.shape)}")
        lead = tuple(xyz.shape[:-1])
        pts = xyz.detach().to(dev, torch.float32).reshape(-1, 3).contiguous()
        out = torch.zeros((pts.shape[0],), dtype=torch.uint8, device=dev)
        if pts.shape[0]:
            h = self.handle()
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().ngf_uv_occupancy_lookup(h, pts.data_ptr(), pts.shape[0], out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return out.bool().view(lead)

    def occupancy_state(self):
        """The mask as a dict for a checkpoint, shaped like the fields' ``alphaMask.*`` keys: ``'occupancy.shape'`` (3 ints) and
        ``'occupancy.mask'`` (``np.packbits`` of the cells); empty without a mask.  Not buffers: ``state_dict`` is unchanged."""
        if self._occ is None:
            return {}
        return {'occupancy.shape': np.asarray(self._occ.shape, np.int64), 'occupancy.mask': self._occ.bits.detach().cpu().numpy().copy()}

    def load_occupancy(self, state):
        """Install the mask of an ``occupancy_state()`` dict (a dict without the keys switches the mask off)."""
        has = [k in state for k in ('occupancy.shape', 'occupancy.mask')]
        if not any(has):
            return self.set_occupancy(None)
        if not all(has):
            raise ValueError("an occupancy state holds both 'occupancy.shape' and 'occupancy.mask'")
        shape = np.asarray(state['occupancy.shape']).reshape(-1)
        if shape.shape[0] != 3:
            raise ValueError(f"'occupancy.shape' holds three cell counts, got {shape.tolist()}")
        mask = state['occupancy.mask']
        mask = mask.detach().cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)
        return self.set_occupancy((mask.reshape(-1), tuple(int(s) for s in shape)))

    @torch.no_grad()
    def export_mesh(self, path=None, *, level, resolution=256, viewdir=None, texture_resolution=512, normals=False, flip=False):
        """The model's surface with its texture atlas mapped onto it -- what UV-Mapping/test.py:39-55 sketches: ``density_lattice(resolution)``,
        marching cubes at ``level`` (no default: NeuTex densities have no natural scale), the gauge at the vertices, ``mesh.atlas_coords`` of
        it.  Returns ``(verts [nv,3], faces [nt,3] int32, st [nv,2])`` on the device.  With ``path`` also writes ``path`` (OBJ; the sphere's
        seam triangles get per-corner coordinates, ``mesh.unwrap_seam``), its ``.mtl`` and the atlas as ``.png``: ``_export_sphere`` /
        ``_export_square`` at ``texture_resolution`` for ``viewdir`` (None: the diffuse texture) ``** (1/2.2)``, clamped, as 8-bit (test.py:60-88)."""
        from . import mesh
        self._gpu("exports meshes")
        vol, lo, step = self.density_lattice(resolution)
        got = mesh.marching_cubes(vol, level, spacing=step.tolist(), origin=lo.tolist(), normals=normals, flip=flip)
        verts, faces = got[0], got[1]
        sphere = self.primitive_type != 'square'
        uv = self.query(verts, want=('uv',))['uv']
        st = mesh.atlas_coords(uv, self.primitive_type, texture_resolution if sphere else None)
        if path is not None:
            self._write_atlas_obj(path, verts, faces, st, viewdir, texture_resolution, got[2] if normals else None)
        return verts, faces, st

    def _write_atlas_obj(self, path, verts, faces, st, viewdir, texture_resolution, normals=None):
        """``path`` (OBJ), its ``.mtl`` and the atlas ``.png`` for a mesh whose texture coordinates ``st`` are ``mesh.atlas_coords`` at
        ``texture_resolution``: the exporter's image for ``viewdir`` (None: diffuse) ``** (1/2.2)``, clamped, 8-bit; the sphere's seam unwrapped."""
        from . import evalout, mesh
        sphere = self.primitive_type != 'square'
        tex = self.net_texture._export_sphere(texture_resolution, viewdir) if sphere else self.net_texture._export_square(texture_resolution, viewdir)
        image = evalout.to_uint8((tex ** (1 / 2.2)).clamp(0, 1).contiguous()).cpu().numpy()
        st_file, faces_vt = mesh.unwrap_seam(faces, st) if sphere else (st, None)
        mesh.write_obj(path, verts, faces, st_file, faces_vt, texture=image, normals=normals)

    # --- the inverse gauge on the GPU (include/ngf.h: ngf_uv_inverse_map) -------------------------------------------
    def inverse_layers(self):
        """The five Linear layers of the inverse network in the order of ngf_uv_inverse_desc."""
        return self.inverse_gauge.layers()

    def inverse_handle(self):
        """The packed inverse network (ngf_uv_inverse), rebuilt when a parameter of it was written in place or replaced -- ``handle()``'s key."""
        key = tuple((t.data_ptr(), t._version) for lin in self.inverse_layers() for t in (lin.weight, lin.bias))
        if self._inv_handle is not None and key == self._inv_key:
            return self._inv_handle
        dev = self._gpu("runs the inverse gauge")
        keep = [t.detach().to(dev, torch.float32).contiguous() for lin in self.inverse_layers() for t in (lin.weight, lin.bias)]
        d = _lib.uv_inverse_desc(self.inverse_gauge.input_point_dim, keep)
        out = C.c_void_p()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().ngf_uv_inverse_create(C.byref(d), C.byref(out), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        self._release_inverse()
        self._inv_handle, self._inv_key = out, key
        return out

    @torch.no_grad()
    def inverse_map(self, uv):
        """``inverse_gauge.map(uv)`` without a graph, in a HIP kernel: template points ``uv`` [..., D] (D = 2 square, 3 sphere), used as given
        -- on the template or off it -- -> world points [..., 3] on the model's device.  fp32 on the matrix pipe; a point's value does not
        depend on the other points, on their number or on its place among them."""
        dev = self._gpu("runs the inverse gauge")
        uv = torch.as_tensor(uv)
        D = self.inverse_gauge.input_point_dim
        if uv.dim() < 1 or uv.shape[-1] != D:
            raise ValueError(f"uv must be [..., {D}] for a {self.primitive_type} model, got {tuple(uv.shape)}")
        lead = tuple(uv.shape[:-1])
        pts = uv.detach().to(dev, torch.float32).reshape(-1, D).contiguous()
        n = pts.shape[0]
        out = torch.empty((n, 3), device=dev)
        if n:
            h = self.inverse_handle()
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().ngf_uv_inverse_map(h, pts.data_ptr(), n, out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return out.view(lead + (3,))

    @torch.no_grad()
    def cycle_error(self, xyz):
        """``|inverse_map(gauge(xyz)) - xyz|^2`` [...] at world points ``xyz`` [..., 3]: the quantity behind the reference's
        ``loss_inverse_mapping`` (without its weights), as two launches -- ``query(xyz, want='uv')``, then ``inverse_map``."""
        dev = self._gpu("runs the inverse gauge")
        xyz = torch.as_tensor(xyz).detach().to(dev, torch.float32)
        back = self.inverse_map(self.query(xyz, want=('uv',))['uv'])
        return ((back - xyz) ** 2).sum(-1)

    @torch.no_grad()
    def coordinate_deformation(self, path=None, *, viewdir=(0, 0, 1), icosphere_division=6, side=257, texture_resolution=512):
        """model.py:383-418 made runnable: the atlas template -- ``mesh.icosphere(icosphere_division)`` for a sphere model,
        ``mesh.square_template(side)`` for a square model -- pushed through the inverse gauge.  Returns ``(verts [nv,3] = inverse_map(template),
        faces [nt,3] int64, colors [nv,3] = texture_colors(template, viewdir), raw as the reference returns them, st [nv,2] =
        mesh.atlas_coords(template))`` on the device.  With ``path`` also writes the OBJ, its ``.mtl`` and the atlas ``.png`` as ``export_mesh``
        does.  (The reference's square branch takes trimesh's Loop-subdivided box, whose vertices this project cannot restate without
        trimesh; the regular grid of SquareTemplate.get_regular_points is the template here.)"""
        from . import mesh
        dev = self._gpu("deforms templates")
        sphere = self.primitive_type != 'square'
        tv, tf = mesh.icosphere(icosphere_division) if sphere else mesh.square_template(side)
        template, faces = torch.from_numpy(tv).to(dev), torch.from_numpy(tf).to(dev)
        verts = self.inverse_map(template)
        colors = self.texture_colors(template, viewdir)
        st = mesh.atlas_coords(template, self.primitive_type, texture_resolution if sphere else None)
        if path is not None:
            self._write_atlas_obj(path, verts, faces, st, viewdir, texture_resolution)
        return verts, faces, colors, st

    def __getstate__(self):              # handles and engines are not state: not pickled, not deep-copied; the occupancy mask is (its bits are a tensor)
        d = self.__dict__.copy()
        for k in ('_handle', '_key', '_inv_handle', '_inv_key', '_uv_engine'):
            d[k] = None
        d.pop('occupancy_in_training', None)          # a training switch, not state
        return d

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault('_occ', None)
        self.net_texture._owner = weakref.ref(self)

    def release(self):
        if self._handle is not None:
            _lib.lib().ngf_uv_destroy(self._handle)
            self._handle, self._key = None, None
        self._release_inverse()
        self.inverse_gauge.release_inverse_grad_engines()

    def _release_inverse(self):
        if getattr(self, '_inv_handle', None) is not None:
            _lib.lib().ngf_uv_inverse_destroy(self._inv_handle)
            self._inv_handle, self._inv_key = None, None

    def __del__(self):
        try:
            self.release()
            self.release_grad_engine()
        except Exception:
            pass

    def handle(self):
        key = tuple((t.data_ptr(), t._version) for lin in self.layers() for t in (lin.weight, lin.bias))     # the 29 render layers only
        if self._handle is not None and key == self._key:
            return self._handle
        dev = torch.device(self.device)
        if dev.type != 'cuda':
            raise RuntimeError("ngf_amd NeuTex renders on the GPU only (device='cuda'); there is no CPU path")
        d = _lib.UvDesc()
        d.sphere = int(self.primitive_type != 'square')
        d.flags = _lib.UV_F_SPLIT_BF16 if self.split_bf16 else 0
        keep = []
        for i, lin in enumerate(self.layers()):
            w = lin.weight.detach().to(dev, torch.float32).contiguous()
            b = lin.bias.detach().to(dev, torch.float32).contiguous()
            keep += [w, b]
            d.w[i], d.b[i] = w.data_ptr(), b.data_ptr()
        out = C.c_void_p()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().ngf_uv_create(C.byref(d), C.byref(out), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        if self._handle is not None:          # (the render handle alone: the inverse network's has its own key)
            _lib.lib().ngf_uv_destroy(self._handle)
        self._handle, self._key = out, key
        self._push_texture()
        if self._occ is not None:
            self._push_occupancy()
        return out

    # --- training (uv_train.py) ---------------------------------------------------------------------------------------------------
    occupancy_in_training = False          # train through the installed occupancy mask: a plain attribute like
                                           # ``differentiable`` -- never saved, not in state_dict, not pickled

    def _uv_grad_engine(self, nrays, S):
        """The training engine for this batch shape, holding the mask training goes through: ``occupancy`` with ``occupancy_in_training`` set,
        else none.  The engine is told only when that object changed since it was last told; a rebuilt engine is told again."""
        from .uv_train import UvGrad, train_params
        eng = _engine.grad_engine(self, '_uv_engine', UvGrad, train_params(self), nrays, S)
        eng.set_occupancy(self._occ if self.occupancy_in_training else None)
        return eng

    @property
    def grad_engine(self):
        """The training engine (uv_train.UvGrad: max_rays, max_samples, bytes) of the last differentiable forward, or None."""
        return self._uv_engine

    def release_grad_engine(self):
        """Free the training engine's per-sample buffers (the next differentiable forward builds a new one)."""
        _engine.release_engine(self, '_uv_engine')

    def _train_forward(self, camera_position, ray_direction, background_color, jitter_u, template_points):
        from .uv_train import TrainOutput, _UvRender, train_params
        if self.split_bf16:
            raise RuntimeError("UV-Mapping training is fp32: construct the NeuTex with split_bf16=False to train it")
        if getattr(self.net_texture, "cubemap_", None) is not None:
            raise RuntimeError("UV-Mapping training does not support texture editing: clear it with set_target_texture(None)")
        params = train_params(self)
        dev = params[0].device
        if dev.type != 'cuda':
            raise RuntimeError("a differentiable NeuTex renders on the GPU only (device='cuda'); there is no CPU path")
        rd = ray_direction.detach().to(dev, torch.float32).contiguous()
        N, R = rd.shape[0], rd.shape[1]
        S = self.sample_num
        U = (torch.rand((N, R, S), device=dev) if jitter_u is None else jitter_u).detach().to(dev, torch.float32).contiguous()
        if tuple(U.shape) != (N, R, S):
            raise ValueError(f"jitter_u must be [N,R,S] = [{N},{R},{S}]")
        cam = camera_position.detach().to(dev, torch.float32).contiguous()
        bg = None if background_color is None else background_color.detach().to(dev, torch.float32).contiguous()
        if tuple(cam.shape) != (N, 3) or (bg is not None and tuple(bg.shape) != (N, 3)):
            raise ValueError(f"camera_position / background_color must be [N,3] with N = {N}")
        eng = self._uv_grad_engine(N * R, S)
        color, trans, uv, weight, pos = _UvRender.apply(self, eng, cam, rd, bg, U, *params)
        _, points_3d = self.inverse_gauge(None if template_points is None else template_points.to(dev, torch.float32))
        points = points_3d.view(points_3d.shape[0], -1, points_3d.shape[-1]).permute(0, 2, 1)
        return TrainOutput(self, uv, points=points, color=color, transmittance=trans, points_original=pos, points_inverse_weights=weight, uv=uv)

    def forward(self, camera_position=None, ray_direction=None, background_color=None, jitter_u=None, debug=False, collect_stats=False,
                template_points=None):
        """model.py:27: camera_position [N,3], ray_direction [N,R,3] (normalised), background_color [N,3] or None.  With ``differentiable`` set
        and grad enabled: the training dict (color, transmittance, points, points_original, points_inverse_weights, uv, lazy points_inverse).
        With an occupancy mask installed (``build_occupancy``) the eval path skips the samples of empty cells: the frame is the reference's with
        sigma set to 0 there, and ``collect_stats`` counts the samples evaluated and the passes run.  The differentiable path ignores the mask
        unless ``occupancy_in_training`` is set; then it trains through the installed mask as it stands -- the same samples the eval path would
        evaluate, no gradient for a cell masked empty -- and never rebuilds it: ``build_occupancy`` after a warm-up and again every so often
        (it evaluates the whole lattice, so cells can come back).  ``grad_engine.counts()`` / ``grad_engine.kept_mask()`` tell what the last
        forward kept.  A backward that has to render its batch again (another forward ran in between) after the mask was changed raises."""
        if self.differentiable and torch.is_grad_enabled():
            if debug or collect_stats:
                raise ValueError("debug / collect_stats belong to the eval path (torch.no_grad() or differentiable = False)")
            return self._train_forward(camera_position, ray_direction, background_color, jitter_u, template_points)
        return self._eval_forward(camera_position, ray_direction, background_color, jitter_u, debug, collect_stats)

    @torch.no_grad()
    def _eval_forward(self, camera_position, ray_direction, background_color, jitter_u, debug, collect_stats):
        dev = torch.device(self.device)
        N, R = ray_direction.shape[0], ray_direction.shape[1]
        S = self.sample_num
        rd = ray_direction.to(dev, torch.float32).contiguous()
        if jitter_u is None:
            jitter_u = torch.rand((N, R, S), device=dev)
        U = jitter_u.to(dev, torch.float32).contiguous()
        color = torch.empty((N, R, 3), device=dev)
        trans = torch.empty((N, R), device=dev)
        dbg_s = torch.zeros((N, R, S), device=dev) if debug else None
        dbg_c = torch.zeros((N, R, S, 3), device=dev) if debug else None
        stats = torch.zeros(16, dtype=torch.int64, device=dev) if collect_stats else None
        h = self.handle()
        # camera positions / backgrounds travel as device tensors ([N,3] in HBM): no `.cpu()`, so a chunked caller (the reference
        # renders 1024 rays per call, UV-Mapping/test.py:108-114) never synchronises, and the N cameras of a batch are ONE launch
        cam = camera_position.detach().to(dev, torch.float32).contiguous()
        bg = None if background_color is None else background_color.detach().to(dev, torch.float32).contiguous()
        if tuple(cam.shape) != (N, 3) or (bg is not None and tuple(bg.shape) != (N, 3)):
            raise ValueError(f"camera_position / background_color must be [N,3] with N = {N}")
        if S <= 0:
            raise RuntimeError(f"NeuTex renders with sample_num > 0, got {S}")
        with torch.cuda.device(dev):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            if N * R > 0:          # (the tensors of an empty batch have no storage: the library would take their null pointers for missing arguments)
                _lib.check(_lib.lib().ngf_uv_render_batch(
                    h, cam.data_ptr(), rd.data_ptr(), None if bg is None else bg.data_ptr(), U.data_ptr(), N, R, S, color.data_ptr(), trans.data_ptr(),
                    None if dbg_s is None else dbg_s.data_ptr(), None if dbg_c is None else dbg_c.data_ptr(),
                    None if stats is None else stats.data_ptr(), st))
        out = {"color": color, "transmittance": trans}
        if collect_stats:
            self.last_stats = stats
        if debug:
            out["sigma"], out["point_color"] = dbg_s, dbg_c
        return out
