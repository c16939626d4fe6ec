"""NeuTex's inverse gauge under autograd on the project's own kernels (include/ngf.h: ngf_uv_inverse_trainer_*).

``InverseGrad`` is the device engine for up to ``max_rays`` points (``max_samples`` is 1: the engine interface counts rays x samples): ``forward``
runs ``inverse_gauge.inverse_network`` at template points with the bits of ``NeuTex.inverse_map`` and keeps the hidden layers' outputs,
``backward`` takes d loss / d xyz and returns d loss / d uv (when asked) and the gradients of the ten tensors in their reference layouts.
``_InverseMap`` is the torch.autograd.Function around it.  ``uvmapping.InverseGauge`` owns one engine per call site when
``inverse_gauge.differentiable`` is set: the template points of the origin loss and the ``uv`` of ``points_inverse`` go through different engines,
so neither makes the other's ticket stale."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._engine import GradEngine, on_stream, replay

NPARAMS = 2 * _lib.UV_INVERSE_LAYERS


def _bind(L):
    if getattr(L, "_ngf_uv_inverse_train_bound", False):
        return
    L.ngf_uv_inverse_trainer_create.argtypes = [C.POINTER(_lib.UvInverseDesc), C.c_int64, C.POINTER(C.c_void_p), C.c_void_p]
    L.ngf_uv_inverse_trainer_destroy.argtypes = [C.c_void_p]
    L.ngf_uv_inverse_trainer_bytes.argtypes = [C.c_void_p]
    L.ngf_uv_inverse_trainer_bytes.restype = C.c_int64
    L.ngf_uv_inverse_train_params_changed.argtypes = [C.c_void_p]
    L.ngf_uv_inverse_train_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]
    L.ngf_uv_inverse_train_backward.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ngf_debug_uv_inverse_train_dx.argtypes = L.ngf_uv_inverse_train_backward.argtypes
    L.ngf_uv_inverse_train_get_grads.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L._ngf_uv_inverse_train_bound = True


def inverse_params(gauge):
    """The ten tensors in the trainer's slot order: weight, bias of each of ``gauge.layers()``."""
    return [t for lin in gauge.layers() for t in (lin.weight, lin.bias)]


class InverseGrad(GradEngine):
    """Device engine of one InverseGauge for batches of up to ``max_rays`` points (about 12.8 KB of kept outputs and dZ per point)."""
    DESTROY, BYTES = "ngf_uv_inverse_trainer_destroy", "ngf_uv_inverse_trainer_bytes"
    PARAMS_CHANGED, GET_GRADS = "ngf_uv_inverse_train_params_changed", "ngf_uv_inverse_train_get_grads"
    # STALE: every tensor -- a change of any version counter (optimizer.step(), load_state_dict, an in-place write) has the trainer pack the
    # weights again, on the device, at the next forward.  An InverseGauge has no ``_grad_stale``.
    FIELD_STALE = False
    GROWS_FROM_RELEASED = False

    def __init__(self, gauge, max_rays, max_samples=1):
        params = inverse_params(gauge)
        dev = params[0].device
        if dev.type != "cuda":
            raise RuntimeError("a differentiable InverseGauge runs on the GPU only (device='cuda'); on the CPU it is plain torch")
        for p in params:
            if not (p.is_cuda and p.device == dev and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError(f"inverse-gauge training needs contiguous float32 parameters on {dev}: one is {p.dtype} on {p.device}")
        super().__init__(gauge, dev, params, max_rays, 1)
        _bind(self.L)
        self.dim = int(gauge.input_point_dim)
        self.forwards = 0               # launches of the training forward (a stale ticket shows as one more than the calls made)
        d = _lib.uv_inverse_desc(self.dim, params)
        out = C.c_void_p()
        with on_stream(dev) as st:
            _lib.check(self.L.ngf_uv_inverse_trainer_create(C.byref(d), self.max_rays, C.byref(out), st))
        self._h = out
        self.key = self._key(params)

    @staticmethod
    def _key(params):
        return tuple((p.data_ptr(), tuple(p.shape)) for p in params)

    def forward(self, uv):
        """uv [n, D] (contiguous float32 on the engine's device) -> (xyz [n, 3], ticket)."""
        self.sync()
        n = uv.shape[0]
        xyz = torch.empty((n, 3), device=self.dev, dtype=torch.float32)
        ticket = C.c_int64(0)
        with on_stream(self.dev) as st:
            _lib.check(self.L.ngf_uv_inverse_train_forward(self._h, uv.data_ptr(), n, xyz.data_ptr(), C.byref(ticket), st))
        self.forwards += 1
        return xyz, int(ticket.value)

    def backward(self, ticket, d_xyz, want_uv, want):
        """-> (d_uv [n, D] or None, the ten gradients with None where ``want[k]`` is false); None = the ticket is stale."""
        n = d_xyz.shape[0]
        d_uv = torch.empty((n, self.dim), device=self.dev, dtype=torch.float32) if want_uv else None
        with on_stream(self.dev) as st:
            rc = self.L.ngf_uv_inverse_train_backward(self._h, int(ticket), d_xyz.data_ptr(), None if d_uv is None else d_uv.data_ptr(), st)
            grads = self._grads(rc, want, st)
        return None if grads is None else (d_uv, grads)


class _InverseMap(torch.autograd.Function):
    """``xyz = inverse_network(uv)`` as one autograd node over ``(uv, *params)``.  ``attr`` names the engine slot of the gauge this call site
    uses."""

    @staticmethod
    def forward(ctx, gauge, attr, eng, uv, *params):
        xyz, ticket = eng.forward(uv)
        ctx.gauge, ctx.attr, ctx.engine, ctx.ticket = gauge, attr, eng, ticket
        ctx.save_for_backward(uv, *params)
        return xyz

    @staticmethod
    def backward(ctx, d_xyz):
        uv, *params = ctx.saved_tensors
        n = uv.shape[0]
        d = d_xyz.to(dtype=torch.float32).contiguous()
        want_uv = bool(ctx.needs_input_grad[3])
        d_uv, grads = replay(ctx.gauge, ctx.attr, lambda: ctx.gauge._inverse_engine(ctx.attr, n), ctx.engine, ctx.ticket, params, (uv,),
                             (d, want_uv), [bool(w) for w in ctx.needs_input_grad[4:]], whose="inverse gauge")
        return (None, None, None, d_uv) + tuple(grads)
