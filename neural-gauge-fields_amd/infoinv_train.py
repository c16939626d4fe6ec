"""The differentiable training-mode forward of the InfoInv field: ``field(rays, is_train=True, infoinv=...)`` under autograd, as the InfoInv tree's own
loop uses it (InfoInv/main.py:262-330) -- torch's loss, ``8e-5 * field.density_L1()``, ``total_loss.backward()``, ``torch.optim.Adam``.

``InfoInvGrad`` is the device engine (include/ngf.h, ngf_infoinv_trainer_*): ``forward`` renders the batch with the trainer's kernels and keeps its
per-sample buffers, ``backward`` takes d loss / d rgb_map and returns the gradients of the sixteen parameters in their reference layouts.
``_InfoInvRender`` is the torch.autograd.Function around it; ``infoinv.TriPlane`` owns one engine per field when ``field.differentiable`` is set."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

PARAM_NAMES = ('plane_xy', 'plane_yz', 'plane_xz',
               'density_decoder.mlp.0.weight', 'density_decoder.mlp.0.bias', 'density_decoder.mlp.2.weight', 'density_decoder.mlp.2.bias',
               'density_decoder.mlp.4.weight', 'density_decoder.mlp.4.bias',
               'rgb_decoder.basis.weight', 'rgb_decoder.mlp.0.weight', 'rgb_decoder.mlp.0.bias', 'rgb_decoder.mlp.2.weight',
               'rgb_decoder.mlp.2.bias', 'rgb_decoder.mlp.4.weight', 'rgb_decoder.mlp.4.bias')
NPARAMS = len(PARAM_NAMES)


class InfoInvTrainDesc(C.Structure):
    _fields_ = [
        ("aabb", C.c_float * 6), ("near_", C.c_float), ("far_", C.c_float), ("step", C.c_float), ("distance_scale", C.c_float),
        ("weight_thres", C.c_float),
        ("plane", C.c_void_p * 3), ("plane_h", C.c_int32 * 3), ("plane_w", C.c_int32 * 3),
        ("dens_w1", C.c_void_p), ("dens_b1", C.c_void_p), ("dens_w2", C.c_void_p), ("dens_b2", C.c_void_p), ("dens_w3", C.c_void_p),
        ("dens_b3", C.c_void_p),
        ("basis", C.c_void_p), ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p), ("w3", C.c_void_p),
        ("b3", C.c_void_p),
        ("mask_bits", C.c_void_p), ("mask_d", C.c_int32), ("mask_h", C.c_int32), ("mask_w", C.c_int32), ("mask_aabb", C.c_float * 6),
        ("max_rays", C.c_int64), ("max_samples", C.c_int32),
    ]


def _bind(L):
    if getattr(L, "_ngf_infoinv_bound", False):
        return
    L.ngf_infoinv_trainer_create.argtypes = [C.POINTER(InfoInvTrainDesc), C.POINTER(C.c_void_p), C.c_void_p]
    L.ngf_infoinv_trainer_destroy.argtypes = [C.c_void_p]
    L.ngf_infoinv_trainer_bytes.argtypes = [C.c_void_p]
    L.ngf_infoinv_trainer_bytes.restype = C.c_int64
    L.ngf_sizeof_infoinv_train_desc.restype = C.c_int32
    L.ngf_infoinv_train_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                            C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]
    L.ngf_infoinv_train_backward_grad.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.ngf_infoinv_train_get_grads.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.ngf_infoinv_train_params_changed.argtypes = [C.c_void_p]
    if L.ngf_sizeof_infoinv_train_desc() != C.sizeof(InfoInvTrainDesc):
        raise RuntimeError("libngf_hip.so ABI mismatch (ngf_infoinv_train_desc layout)")
    L._ngf_infoinv_bound = True


def train_params(field):
    """The sixteen parameter tensors in the trainer's `which` order (PARAM_NAMES)."""
    d, r = field.density_decoder.mlp, field.rgb_decoder
    return [field.plane_xy, field.plane_yz, field.plane_xz, d[0].weight, d[0].bias, d[2].weight, d[2].bias, d[4].weight, d[4].bias,
            r.basis.weight, r.mlp[0].weight, r.mlp[0].bias, r.mlp[2].weight, r.mlp[2].bias, r.mlp[4].weight, r.mlp[4].bias]


def _field_key(f, params):
    """What the engine was built from, without a device-to-host copy: tensors by (pointer, version) -- the mask's aabb included, its values are
    read only when an engine is (re)built -- and the field's aabb through Base._aabb_host (cached per tensor version).  stepSize is a host tensor."""
    m = None
    if f.alphaMask is not None:
        vol, ab = f.alphaMask.alpha_volume, f.alphaMask.aabb
        m = (id(f.alphaMask), vol.data_ptr(), vol._version, ab.data_ptr(), ab._version)
    return (tuple((p.data_ptr(), tuple(p.shape)) for p in params), m, f._aabb_host(), tuple(float(v) for v in f.near_far),
            float(f.stepSize), float(f.distance_scale), float(f.rayMarch_weight_thres))


class InfoInvGrad:
    """Device engine of one InfoInv field for batches of up to max_rays x max_samples (per-sample buffers ~4 KB per pair)."""

    def __init__(self, field, max_rays, max_samples):
        self.field = field
        self.dev = torch.device(field.device)
        if self.dev.type != "cuda":
            raise RuntimeError("a differentiable InfoInv field(..., is_train=True) renders on the GPU only (device='cuda'); there is no CPU path")
        self.L = _lib.lib()
        _bind(self.L)
        self.params = train_params(field)
        if self.params[0].is_cuda:
            self.dev = self.params[0].device          # 'cuda' -> 'cuda:k': where the parameters live
        for name, p in zip(PARAM_NAMES, self.params):
            if not (p.is_cuda and p.device == self.dev and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError(f"InfoInv training needs contiguous float32 parameters on {self.dev}: {name} is {p.dtype} on {p.device}")
        self.max_rays, self.max_samples = int(max_rays), int(max_samples)
        d = InfoInvTrainDesc()
        ptr = [p.data_ptr() for p in self.params]
        for k in range(3):
            d.plane[k] = ptr[k]
            d.plane_h[k], d.plane_w[k] = int(self.params[k].shape[2]), int(self.params[k].shape[3])
        (d.dens_w1, d.dens_b1, d.dens_w2, d.dens_b2, d.dens_w3, d.dens_b3) = ptr[3:9]
        (d.basis, d.w1, d.b1, d.w2, d.b2, d.w3, d.b3) = ptr[9:16]
        d.aabb = (C.c_float * 6)(*field._aabb_host())
        d.near_, d.far_ = float(field.near_far[0]), float(field.near_far[1])
        d.step = float(field.stepSize)
        d.distance_scale = float(field.distance_scale)
        d.weight_thres = float(field.rayMarch_weight_thres)
        self._keep = []
        if field.alphaMask is not None:
            bits = field.alphaMask.packed_bits_device().to(self.dev)
            self._keep.append(bits)
            d.mask_bits = bits.data_ptr()
            shp = field.alphaMask.alpha_volume.shape
            d.mask_d, d.mask_h, d.mask_w = int(shp[-3]), int(shp[-2]), int(shp[-1])
            d.mask_aabb = (C.c_float * 6)(*field.alphaMask.aabb.reshape(-1).tolist())
        d.max_rays, d.max_samples = self.max_rays, self.max_samples
        out = C.c_void_p()
        with torch.cuda.device(self.dev):
            _lib.check(self.L.ngf_infoinv_trainer_create(C.byref(d), C.byref(out), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        self._h = out
        self.key = _field_key(field, self.params)
        self._versions = None                   # the first forward packs the planes

    @property
    def bytes(self) -> int:
        return int(self.L.ngf_infoinv_trainer_bytes(self._h)) if self._h is not None else 0

    def fits(self, n, S, params):
        return n <= self.max_rays and S <= self.max_samples and self.key == _field_key(self.field, params)

    def release(self):
        if getattr(self, "_h", None) is not None:
            self.L.ngf_infoinv_trainer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def forward(self, rays, jitter, S, white_bg, infoinv):
        """-> (rgb_map [n,3], depth_map [n], ticket).  The packed planes follow torch's in-place version counters (optimizer.step(),
        load_state_dict); ``field.invalidate()`` marks them stale for writes that bypass the counters."""
        v = tuple(int(p._version) for p in self.params[:3])
        if v != self._versions or getattr(self.field, "_grad_stale", False):
            _lib.check(self.L.ngf_infoinv_train_params_changed(self._h))
            self._versions = v
            self.field._grad_stale = False
        n = rays.shape[0]
        rgb = torch.empty((n, 3), device=self.dev, dtype=torch.float32)
        depth = torch.empty((n,), device=self.dev, dtype=torch.float32)
        ticket = C.c_int64(0)
        with torch.cuda.device(self.dev):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(self.L.ngf_infoinv_train_forward(self._h, rays.data_ptr(), jitter.data_ptr(), n, int(S), int(bool(white_bg)),
                                                        int(bool(infoinv)), rgb.data_ptr(), depth.data_ptr(), C.byref(ticket), st))
        return rgb, depth, int(ticket.value)

    def backward(self, ticket, d_rgb, want):
        """``want[k]``: return parameter k's gradient (else None).  None = the ticket is stale (another forward used the buffers)."""
        with torch.cuda.device(self.dev):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            rc = self.L.ngf_infoinv_train_backward_grad(self._h, int(ticket), d_rgb.data_ptr(), st)
            if rc == _lib.E_STALE:
                return None
            _lib.check(rc)
            grads = [torch.empty_like(self.params[k]) if want[k] else None for k in range(NPARAMS)]
            ptrs = (C.c_void_p * NPARAMS)(*[None if g is None else g.data_ptr() for g in grads])
            _lib.check(self.L.ngf_infoinv_train_get_grads(self._h, ptrs, st))
        return grads


class _InfoInvRender(torch.autograd.Function):
    """``rgb_map, depth_map = field(rays, is_train=True, infoinv=...)`` as one autograd node over the sixteen parameters.  depth_map is not
    differentiable (the reference computes it under torch.no_grad(), InfoInv/models/FieldBase.py:274-276)."""

    @staticmethod
    def forward(ctx, field, eng, rays, jitter, S, white_bg, infoinv, *params):
        rgb, depth, ticket = eng.forward(rays, jitter, S, white_bg, infoinv)
        ctx.field, ctx.engine, ctx.ticket = field, eng, ticket
        ctx.cfg = (int(S), bool(white_bg), bool(infoinv))
        ctx.save_for_backward(rays, jitter, *params)          # saved tensors: autograd refuses a backward after an in-place write to any of them
        ctx.mark_non_differentiable(depth)
        return rgb, depth

    @staticmethod
    def backward(ctx, d_rgb, _d_depth):
        saved = ctx.saved_tensors
        rays, jitter = saved[0], saved[1]
        S, white_bg, infoinv = ctx.cfg
        eng = ctx.engine
        if getattr(ctx.field, '_ii_engine', None) is not eng or eng._h is None:
            eng = ctx.field._infoinv_grad_engine(rays.shape[0], S)
        if any(a.data_ptr() != b.data_ptr() or a.shape != b.shape for a, b in zip(saved[2:], eng.params)):
            raise RuntimeError("the field's parameter tensors were re-allocated between forward and backward")
        d = d_rgb.to(dtype=torch.float32).contiguous()
        want = [bool(w) for w in ctx.needs_input_grad[7:]]
        grads = eng.backward(ctx.ticket, d, want) if eng is ctx.engine else None
        if grads is None:           # another forward went through the engine since (or it is a new one): render this batch again, then its backward
            _, _, ticket = eng.forward(rays, jitter, S, white_bg, infoinv)
            grads = eng.backward(ticket, d, want)
            if grads is None:
                raise RuntimeError(_lib.lib().ngf_last_error().decode())
        return (None,) * 7 + tuple(grads)
