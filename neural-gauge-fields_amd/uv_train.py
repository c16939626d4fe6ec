"""The differentiable training-mode forward of the UV-Mapping (NeuTex) model: ``net(campos, raydir, background_color)`` under autograd, as the
reference's own loop uses it (UV-Mapping/train.py:138-141, model.py:300-356) -- torch's losses, ``loss_total.backward()``, ``torch.optim.Adam``.

``UvGrad`` is the device engine (include/ngf.h, ngf_uv_trainer_*): ``forward`` renders the batch with the trainer's kernels and keeps every layer's
activations, ``backward`` takes d loss / d (color, transmittance, uv, blend weight) and returns the gradients of the 58 render-layer tensors in
their reference layouts.  ``_UvRender`` is the torch.autograd.Function around it; ``uvmapping.NeuTex`` owns one engine when ``net.differentiable``
is set.  The inverse network (``inverse_gauge``) stays plain torch: it sees the template points and, with an inverse-mapping loss, ``uv``."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

NPARAMS = 2 * _lib.UV_LAYERS


class UvTrainDesc(C.Structure):
    _fields_ = [("sphere", C.c_int32), ("flags", C.c_int32), ("w", C.c_void_p * _lib.UV_LAYERS), ("b", C.c_void_p * _lib.UV_LAYERS),
                ("max_rays", C.c_int64), ("max_samples", C.c_int32), ("pad_", C.c_int32)]


class UvtGemmArgs(C.Structure):
    """ngf_uvt_gemm_args (include/ngf.h): one layer-sized GEMM of the trainer on caller-owned buffers, a test aid."""
    _fields_ = [("size", C.c_int32), ("form", C.c_int32), ("in_", C.c_int32), ("out", C.c_int32), ("act", C.c_int32), ("n_dx", C.c_int32),
                ("rows", C.c_int64), ("rows_dev", C.c_void_p), ("x", C.c_void_p), ("ld_x", C.c_int64), ("w", C.c_void_p), ("b", C.c_void_p),
                ("z", C.c_void_p), ("ld_z", C.c_int64), ("dx", C.c_void_p), ("ld_dx", C.c_int64), ("add", C.c_void_p), ("ld_add", C.c_int64),
                ("part", C.c_void_p), ("partb", C.c_void_p), ("part_elems", C.c_int64), ("partb_elems", C.c_int64),
                ("gw", C.c_void_p), ("gb", C.c_void_p)]


GEMM_FORWARD, GEMM_DX, GEMM_DW = 0, 1, 2


def debug_gemm(form, stream=None, **kw):
    """ngf_debug_uvt_gemm: keyword = field of UvtGemmArgs; a torch tensor is passed as its data pointer (``part`` / ``partb`` also set
    their element counts).  Returns the library's return code: 0, or 1 with ngf_last_error() set."""
    L = _lib.lib()
    _bind(L)
    a = UvtGemmArgs()
    a.size, a.form = C.sizeof(UvtGemmArgs), int(form)
    for k, v in kw.items():
        if isinstance(v, torch.Tensor):
            if k in ("part", "partb"):
                setattr(a, k + "_elems", v.numel())
            v = v.data_ptr()
        setattr(a, k, v)
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    return L.ngf_debug_uvt_gemm(C.byref(a), C.c_void_p(st))


def _bind(L):
    if getattr(L, "_ngf_uv_train_bound", False):
        return
    L.ngf_debug_uvt_gemm.argtypes = [C.POINTER(UvtGemmArgs), C.c_void_p]
    L.ngf_uv_trainer_create.argtypes = [C.POINTER(UvTrainDesc), C.POINTER(C.c_void_p), C.c_void_p]
    L.ngf_uv_trainer_destroy.argtypes = [C.c_void_p]
    L.ngf_uv_trainer_bytes.argtypes = [C.c_void_p]
    L.ngf_uv_trainer_bytes.restype = C.c_int64
    L.ngf_sizeof_uv_train_desc.restype = C.c_int32
    L.ngf_uv_train_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]
    L.ngf_uv_train_backward.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ngf_uv_train_get_grads.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.ngf_uv_train_params_changed.argtypes = [C.c_void_p]
    if L.ngf_sizeof_uv_train_desc() != C.sizeof(UvTrainDesc):
        raise RuntimeError("libngf_hip.so ABI mismatch (ngf_uv_train_desc layout)")
    L._ngf_uv_train_bound = True


def train_params(net):
    """The 58 render-layer tensors in the trainer's slot order: weight, bias of each layer of ``net.layers()``."""
    out = []
    for lin in net.layers():
        out += [lin.weight, lin.bias]
    return out


class UvGrad:
    """Device engine of one NeuTex for batches of up to max_rays x max_samples (about 27 KB of per-sample buffers per (ray, sample) pair)."""

    def __init__(self, net, max_rays, max_samples):
        self.net = net
        self.L = _lib.lib()
        _bind(self.L)
        self.params = train_params(net)
        self.dev = self.params[0].device
        if self.dev.type != "cuda":
            raise RuntimeError("a differentiable NeuTex renders on the GPU only (device='cuda'); there is no CPU path")
        for p in self.params:
            if not (p.is_cuda and p.device == self.dev and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError(f"UV-Mapping training needs contiguous float32 parameters on {self.dev}: one is {p.dtype} on {p.device}")
        self.max_rays, self.max_samples = int(max_rays), int(max_samples)
        d = UvTrainDesc()
        d.sphere = int(net.primitive_type != 'square')
        d.flags = 0
        for i in range(_lib.UV_LAYERS):
            d.w[i], d.b[i] = self.params[2 * i].data_ptr(), self.params[2 * i + 1].data_ptr()
        d.max_rays, d.max_samples = self.max_rays, self.max_samples
        out = C.c_void_p()
        with torch.cuda.device(self.dev):
            _lib.check(self.L.ngf_uv_trainer_create(C.byref(d), C.byref(out), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        self._h = out
        self.key = self._key(self.params)
        self._versions = None

    @staticmethod
    def _key(params):
        return tuple((p.data_ptr(), tuple(p.shape)) for p in params)

    @property
    def bytes(self) -> int:
        return int(self.L.ngf_uv_trainer_bytes(self._h)) if self._h is not None else 0

    def fits(self, nrays, S, params):
        return nrays <= self.max_rays and S <= self.max_samples and self.key == self._key(params)

    def release(self):
        if getattr(self, "_h", None) is not None:
            self.L.ngf_uv_trainer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def forward(self, cam, rd, bg, U):
        """-> (color [N,R,3], trans [N,R], uv [N,R,S,D], weight [N,R,S], ray_pos [N,R,S,3], ticket).  The weights are read in place; a change of
        any tensor's version (optimizer.step(), load_state_dict) is reported to the trainer (it packs nothing today, the call is its contract)."""
        v = tuple(int(p._version) for p in self.params)
        if v != self._versions:
            _lib.check(self.L.ngf_uv_train_params_changed(self._h))
            self._versions = v
        N, R, S = U.shape
        D = 2 if self.net.primitive_type == 'square' else 3
        f = dict(device=self.dev, dtype=torch.float32)
        color, trans = torch.empty((N, R, 3), **f), torch.empty((N, R), **f)
        uv, weight, pos = torch.empty((N, R, S, D), **f), torch.empty((N, R, S), **f), torch.empty((N, R, S, 3), **f)
        ticket = C.c_int64(0)
        with torch.cuda.device(self.dev):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(self.L.ngf_uv_train_forward(self._h, cam.data_ptr(), rd.data_ptr(), None if bg is None else bg.data_ptr(), U.data_ptr(), N, R, S,
                                                   color.data_ptr(), trans.data_ptr(), uv.data_ptr(), weight.data_ptr(), pos.data_ptr(),
                                                   C.byref(ticket), st))
        return color, trans, uv, weight, pos, int(ticket.value)

    def backward(self, ticket, d_color, d_trans, d_uv, d_weight, want):
        """``want[k]``: return tensor k's gradient (else None).  None = the ticket is stale (another forward used the buffers)."""
        with torch.cuda.device(self.dev):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            rc = self.L.ngf_uv_train_backward(self._h, int(ticket), d_color.data_ptr(), d_trans.data_ptr(),
                                              None if d_uv is None else d_uv.data_ptr(), None if d_weight is None else d_weight.data_ptr(), st)
            if rc == _lib.E_STALE:
                return None
            _lib.check(rc)
            grads = [torch.empty_like(self.params[k]) if want[k] else None for k in range(NPARAMS)]
            ptrs = (C.c_void_p * NPARAMS)(*[None if g is None else g.data_ptr() for g in grads])
            _lib.check(self.L.ngf_uv_train_get_grads(self._h, ptrs, st))
        return grads


def _grad_or_zeros(g, like):
    return torch.zeros_like(like) if g is None else g.to(dtype=torch.float32).contiguous()


class _UvRender(torch.autograd.Function):
    """``color, transmittance, uv, blend_weight, ray_pos`` of NeuTex.forward as one autograd node over the 58 render-layer tensors.  ray_pos
    (``points_original``) carries no gradient, as in the reference (cube_ray_generation runs under torch.no_grad(), renderer.py:90)."""

    @staticmethod
    def forward(ctx, net, eng, cam, rd, bg, U, *params):
        color, trans, uv, weight, pos, ticket = eng.forward(cam, rd, bg, U)
        ctx.net, ctx.engine, ctx.ticket = net, eng, ticket
        ctx.has_bg = bg is not None
        ctx.save_for_backward(cam, rd, U, *(() if bg is None else (bg,)), *params)
        ctx.mark_non_differentiable(pos)
        return color, trans, uv, weight, pos

    @staticmethod
    def backward(ctx, d_color, d_trans, d_uv, d_weight, _d_pos):
        saved = ctx.saved_tensors
        cam, rd, U = saved[0], saved[1], saved[2]
        bg = saved[3] if ctx.has_bg else None
        params = saved[4 if ctx.has_bg else 3:]
        N, R, S = U.shape
        eng = ctx.engine
        if getattr(ctx.net, '_uv_engine', None) is not eng or eng._h is None:
            eng = ctx.net._uv_grad_engine(N * R, S)
        if any(a.data_ptr() != b.data_ptr() or a.shape != b.shape for a, b in zip(params, eng.params)):
            raise RuntimeError("the model's parameter tensors were re-allocated between forward and backward")
        dev = eng.dev
        f = dict(device=dev, dtype=torch.float32)
        dc = _grad_or_zeros(d_color, torch.empty((N, R, 3), **f))
        dt = _grad_or_zeros(d_trans, torch.empty((N, R), **f))
        du = None if d_uv is None else d_uv.to(dtype=torch.float32).contiguous()
        dw = None if d_weight is None else d_weight.to(dtype=torch.float32).contiguous()
        want = [bool(w) for w in ctx.needs_input_grad[6:]]
        grads = eng.backward(ctx.ticket, dc, dt, du, dw, want) if eng is ctx.engine else None
        if grads is None:           # another forward went through the engine since (or it is a new one): render this batch again, then its backward
            *_, ticket = eng.forward(cam, rd, bg, U)
            grads = eng.backward(ticket, dc, dt, du, dw, want)
            if grads is None:
                raise RuntimeError(_lib.lib().ngf_last_error().decode())
        return (None,) * 6 + tuple(grads)


class TrainOutput(dict):
    """The reference's output dict (model.py:27-59); ``points_inverse`` = inverse_gauge.map(uv) is computed on first access only."""

    def __init__(self, net, uv, /, **kw):
        super().__init__(**kw)
        self._net, self._uv = net, uv

    def __missing__(self, key):
        if key != "points_inverse":
            raise KeyError(key)
        v = self._net.inverse_gauge.map(self._uv)
        self[key] = v
        return v
