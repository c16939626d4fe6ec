"""The differentiable training-mode forward of the UV-Mapping (NeuTex) model: ``net(campos, raydir, background_color)`` under autograd, as the
reference's own loop uses it (UV-Mapping/train.py:138-141, model.py:300-356) -- torch's losses, ``loss_total.backward()``, ``torch.optim.Adam``.

``UvGrad`` is the device engine (include/ngf.h, ngf_uv_trainer_*): ``forward`` renders the batch with the trainer's kernels and keeps every layer's
activations, ``backward`` takes d loss / d (color, transmittance, uv, blend weight) and returns the gradients of the 58 render-layer tensors in
their reference layouts.  ``_UvRender`` is the torch.autograd.Function around it; ``uvmapping.NeuTex`` owns one engine when ``net.differentiable``
is set.  The inverse network (``inverse_gauge``) sees the template points and, with an inverse-mapping loss, ``uv``: plain torch by default,
its own HIP forward and backward with ``net.inverse_gauge.differentiable = True`` (uv_inverse_train.py)."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._engine import GradEngine, on_stream, replay

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
    L.ngf_uv_trainer_set_occupancy.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    L.ngf_uv_train_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]
    L.ngf_uv_train_kept.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    if L.ngf_sizeof_uv_train_desc() != C.sizeof(UvTrainDesc):
        raise RuntimeError("libngf_hip.so ABI mismatch (ngf_uv_train_desc layout)")
    L._ngf_uv_train_bound = True


def train_params(net):
    """The 58 render-layer tensors in the trainer's slot order: weight, bias of each layer of ``net.layers()``."""
    out = []
    for lin in net.layers():
        out += [lin.weight, lin.bias]
    return out


class UvGrad(GradEngine):
    """Device engine of one NeuTex for batches of up to max_rays x max_samples (about 27 KB of per-sample buffers per (ray, sample) pair)."""
    DESTROY, BYTES, PARAMS_CHANGED, GET_GRADS = "ngf_uv_trainer_destroy", "ngf_uv_trainer_bytes", "ngf_uv_train_params_changed", "ngf_uv_train_get_grads"
    # STALE: every tensor.  The weights are read in place; a change of any tensor's version (optimizer.step(), load_state_dict) is reported to
    # the trainer (it packs nothing today, the call is its contract).  A NeuTex has no ``_grad_stale``.
    FIELD_STALE = False
    GROWS_FROM_RELEASED = False

    def __init__(self, net, max_rays, max_samples):
        params = train_params(net)
        dev = params[0].device
        if dev.type != "cuda":
            raise RuntimeError("a differentiable NeuTex renders on the GPU only (device='cuda'); there is no CPU path")
        super().__init__(net, dev, params, max_rays, max_samples)
        _bind(self.L)
        self.net = net
        for p in params:
            if not (p.is_cuda and p.device == dev and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError(f"UV-Mapping training needs contiguous float32 parameters on {dev}: one is {p.dtype} on {p.device}")
        d = UvTrainDesc()
        d.sphere = int(net.primitive_type != 'square')
        d.flags = 0
        for i in range(_lib.UV_LAYERS):
            d.w[i], d.b[i] = params[2 * i].data_ptr(), params[2 * i + 1].data_ptr()
        d.max_rays, d.max_samples = self.max_rays, self.max_samples
        out = C.c_void_p()
        with on_stream(dev) as st:
            _lib.check(self.L.ngf_uv_trainer_create(C.byref(d), C.byref(out), st))
        self._h = out
        self.key = self._key(params)
        self.occupancy = None       # the uvmapping.Occupancy whose bits the trainer holds a copy of (set_occupancy), or None
        self._shape = None          # (N, R, S) of the last forward

    @staticmethod
    def _key(params):
        return tuple((p.data_ptr(), tuple(p.shape)) for p in params)

    def set_occupancy(self, occ):
        """Train through the mask ``occ`` (a uvmapping.Occupancy; None = off) from the next forward on: only the in-cube samples of occupied
        cells are evaluated (include/ngf.h: ngf_uv_trainer_set_occupancy).  The library copies the bits; an object that is already the
        engine's is not pushed again."""
        if occ is self.occupancy:
            return
        with on_stream(self.dev) as st:
            if occ is None:
                _lib.check(self.L.ngf_uv_trainer_set_occupancy(self._h, None, 0, 0, 0, st))
            else:
                bits = occ.bits.to(self.dev).contiguous()
                n = occ.shape
                _lib.check(self.L.ngf_uv_trainer_set_occupancy(self._h, bits.data_ptr(), n[0], n[1], n[2], st))
                torch.cuda.current_stream(self.dev).synchronize()          # (still inside on_stream: the stream the copy went to) `bits` may go now
        self.occupancy = occ

    def counts(self):
        """``(in_cube, kept)`` of the last forward: its in-cube samples and those of them it evaluated (equal without a mask).  Synchronises."""
        out = (C.c_int64 * 2)()
        with on_stream(self.dev) as st:
            _lib.check(self.L.ngf_uv_train_counts(self._h, out, st))
        return int(out[0]), int(out[1])

    def kept_mask(self):
        """bool [N,R,S]: the samples the last forward evaluated."""
        if self._shape is None:
            raise RuntimeError("the engine has run no forward")
        out = torch.empty(self._shape, dtype=torch.uint8, device=self.dev)
        with on_stream(self.dev) as st:
            _lib.check(self.L.ngf_uv_train_kept(self._h, out.data_ptr(), st))
        return out.bool()

    def forward(self, cam, rd, bg, U):
        """-> (color [N,R,3], trans [N,R], uv [N,R,S,D], weight [N,R,S], ray_pos [N,R,S,3], ticket)."""
        self.sync()
        N, R, S = U.shape
        self._shape = (N, R, S)
        D = 2 if self.net.primitive_type == 'square' else 3
        f = dict(device=self.dev, dtype=torch.float32)
        color, trans = torch.empty((N, R, 3), **f), torch.empty((N, R), **f)
        uv, weight, pos = torch.empty((N, R, S, D), **f), torch.empty((N, R, S), **f), torch.empty((N, R, S, 3), **f)
        ticket = C.c_int64(0)
        with on_stream(self.dev) as st:
            _lib.check(self.L.ngf_uv_train_forward(self._h, cam.data_ptr(), rd.data_ptr(), None if bg is None else bg.data_ptr(), U.data_ptr(), N, R, S,
                                                   color.data_ptr(), trans.data_ptr(), uv.data_ptr(), weight.data_ptr(), pos.data_ptr(),
                                                   C.byref(ticket), st))
        return color, trans, uv, weight, pos, int(ticket.value)

    def backward(self, ticket, d_color, d_trans, d_uv, d_weight, want):
        """``want[k]``: return tensor k's gradient (else None).  None = the ticket is stale (another forward used the buffers)."""
        with on_stream(self.dev) as st:
            rc = self.L.ngf_uv_train_backward(self._h, int(ticket), d_color.data_ptr(), d_trans.data_ptr(),
                                              None if d_uv is None else d_uv.data_ptr(), None if d_weight is None else d_weight.data_ptr(), st)
            return self._grads(rc, want, st)


def _f32(g):
    return None if g is None else g.to(dtype=torch.float32).contiguous()


class _UvRender(torch.autograd.Function):
    """``color, transmittance, uv, blend_weight, ray_pos`` of NeuTex.forward as one autograd node over the 58 render-layer tensors.  ray_pos
    (``points_original``) carries no gradient, as in the reference (cube_ray_generation runs under torch.no_grad(), renderer.py:90)."""

    @staticmethod
    def forward(ctx, net, eng, cam, rd, bg, U, *params):
        color, trans, uv, weight, pos, ticket = eng.forward(cam, rd, bg, U)
        ctx.net, ctx.engine, ctx.ticket = net, eng, ticket
        ctx.occupancy = getattr(eng, "occupancy", None)          # the mask this forward trained through (the Occupancy object, or None)
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
        f = dict(device=U.device, dtype=torch.float32)      # the library reads d color and d transmittance unconditionally
        dc = torch.zeros((N, R, 3), **f) if d_color is None else _f32(d_color)
        dt = torch.zeros((N, R), **f) if d_trans is None else _f32(d_trans)

        def same_mask(eng):          # before the batch is rendered again: through the mask of the forward, or not at all
            if getattr(eng, "occupancy", None) is not ctx.occupancy:
                raise RuntimeError("the occupancy mask this forward trained through is no longer the one in the training engine (another forward "
                                   "ran after the mask was changed): its backward would render the batch again through a different mask and "
                                   "differentiate a different function.  Call backward before the next forward, or keep the mask until then")

        grads = replay(ctx.net, '_uv_engine', lambda: ctx.net._uv_grad_engine(N * R, S), ctx.engine, ctx.ticket, params, (cam, rd, bg, U),
                       (dc, dt, _f32(d_uv), _f32(d_weight)), [bool(w) for w in ctx.needs_input_grad[6:]], whose="model", before_rerender=same_mask)
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
