"""The differentiable training-mode forward of the InfoInv field: ``field(rays, is_train=True, infoinv=...)`` under autograd, as the InfoInv tree's own
loop uses it (InfoInv/main.py:262-330) -- torch's loss, ``8e-5 * field.density_L1()``, ``total_loss.backward()``, ``torch.optim.Adam``.

``InfoInvGrad`` is the device engine (include/ngf.h, ngf_infoinv_trainer_*): ``forward`` renders the batch with the trainer's kernels and keeps its
per-sample buffers, ``backward`` takes d loss / d rgb_map and returns the gradients of the sixteen parameters in their reference layouts.
``_InfoInvRender`` is the torch.autograd.Function around it; ``infoinv.TriPlane`` owns one engine per field when ``field.differentiable`` is set.

``Trainer`` is the fused form of the same loop body on the same engine: one call per iteration, the rgb loss and Adam inside the library, the weight
gradients on the matrix pipe (ngf_infoinv_train_step_backward / _adam_all); ``fit`` is the lifecycle loop of InfoInv/main.py:243-336 around it."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._engine import GradEngine, TrainerBase, fill_geometry, on_stream, rays_per_chunk, replay

L1_REG_WEIGHT = 8e-5            # InfoInv/main.py:259
MAX_PAIRS = 1 << 22             # default of ``field.grad_max_pairs``: the (ray, sample) pairs one engine holds, ~16 GB of per-sample buffers
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


class IiProductArgs(C.Structure):
    """ngf_ii_product_args (include/ngf.h): one weight-gradient product of the trainer on caller-owned buffers, a test aid."""
    _fields_ = [("size", C.c_int32), ("form", C.c_int32), ("m", C.c_int32), ("n", C.c_int32), ("accumulate", C.c_int32), ("pad_", C.c_int32),
                ("rows", C.c_int64), ("ld", C.c_int64), ("rows_dev", C.c_void_p), ("x", C.c_void_p), ("y", C.c_void_p),
                ("part", C.c_void_p), ("partb", C.c_void_p), ("part_elems", C.c_int64), ("partb_elems", C.c_int64),
                ("gw", C.c_void_p), ("gb", C.c_void_p), ("gw64", C.c_void_p)]


PRODUCT_MFMA, PRODUCT_FP64 = 0, 1


def debug_product(form, stream=None, **kw):
    """ngf_debug_ii_product: keyword = field of IiProductArgs; a torch tensor is passed as its data pointer (``part`` / ``partb`` also set
    their element counts).  Returns the library's return code: 0, or 1 with ngf_last_error() set."""
    L = _lib.lib()
    _bind(L)
    a = IiProductArgs()
    a.size, a.form = C.sizeof(IiProductArgs), int(form)
    for k, v in kw.items():
        if isinstance(v, torch.Tensor):
            if k in ("part", "partb"):
                setattr(a, k + "_elems", v.numel())
            v = v.data_ptr()
        setattr(a, k, v)
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    return L.ngf_debug_ii_product(C.byref(a), C.c_void_p(st))


def _bind(L):
    if getattr(L, "_ngf_infoinv_bound", False):
        return
    L.ngf_debug_ii_product.argtypes = [C.POINTER(IiProductArgs), C.c_void_p]
    L.ngf_debug_ii_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]
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
    L.ngf_infoinv_train_step_backward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                                  C.c_void_p]
    L.ngf_infoinv_train_set_moments.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.ngf_infoinv_train_adam_all.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]
    L.ngf_infoinv_train_get_grad.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.ngf_infoinv_train_adam_ext.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float,
                                             C.c_void_p]
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


class InfoInvGrad(GradEngine):
    """Device engine of one InfoInv field for batches of up to max_rays x max_samples (per-sample buffers ~4 KB per pair)."""
    DESTROY, BYTES = "ngf_infoinv_trainer_destroy", "ngf_infoinv_trainer_bytes"
    PARAMS_CHANGED, GET_GRADS = "ngf_infoinv_train_params_changed", "ngf_infoinv_train_get_grads"
    STALE = slice(0, 3)             # the planes: the trainer keeps channel-last copies of them

    def __init__(self, field, max_rays, max_samples):
        dev = torch.device(field.device)
        if dev.type != "cuda":
            raise RuntimeError("a differentiable InfoInv field(..., is_train=True) renders on the GPU only (device='cuda'); there is no CPU path")
        params = train_params(field)
        if params[0].is_cuda:
            dev = params[0].device                    # 'cuda' -> 'cuda:k': where the parameters live
        super().__init__(field, dev, params, max_rays, max_samples)
        _bind(self.L)
        for name, p in zip(PARAM_NAMES, params):
            if not (p.is_cuda and p.device == dev and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError(f"InfoInv training needs contiguous float32 parameters on {dev}: {name} is {p.dtype} on {p.device}")
        d = InfoInvTrainDesc()
        ptr = [p.data_ptr() for p in params]
        for k in range(3):
            d.plane[k] = ptr[k]
            d.plane_h[k], d.plane_w[k] = int(params[k].shape[2]), int(params[k].shape[3])
        (d.dens_w1, d.dens_b1, d.dens_w2, d.dens_b2, d.dens_w3, d.dens_b3) = ptr[3:9]
        (d.basis, d.w1, d.b1, d.w2, d.b2, d.w3, d.b3) = ptr[9:16]
        self._keep = fill_geometry(d, field, dev, float(field.rayMarch_weight_thres))
        d.max_rays, d.max_samples = self.max_rays, self.max_samples
        out = C.c_void_p()
        with on_stream(dev) as st:
            _lib.check(self.L.ngf_infoinv_trainer_create(C.byref(d), C.byref(out), st))
        self._h = out
        self.key = self._key(params)
        self.repacks = 0                        # how often the packed planes were marked stale (ngf_infoinv_train_params_changed)
        self._moments_owner = None              # the Trainer whose Adam moments the handle holds
        self.adam_ext = self.L.ngf_infoinv_train_adam_ext      # what ngf_amd.optim.Adam calls for this engine's parameters
        from . import optim
        optim.register(field, params)           # ngf_amd.optim.Adam finds the engine behind a parameter (fused update, no re-pack)

    def _key(self, params):
        return _field_key(self.field, params)

    def sync_planes(self):
        """``GradEngine.sync``, counted: the first forward packs the planes, later ones when a version counter moved or the field was invalidated."""
        self.repacks += self.sync()

    def forward(self, rays, jitter, S, white_bg, infoinv):
        """-> (rgb_map [n,3], depth_map [n], ticket); see ``sync_planes`` for when the planes are packed again."""
        self.sync_planes()
        n = rays.shape[0]
        rgb = torch.empty((n, 3), device=self.dev, dtype=torch.float32)
        depth = torch.empty((n,), device=self.dev, dtype=torch.float32)
        ticket = C.c_int64(0)
        with on_stream(self.dev) as st:
            _lib.check(self.L.ngf_infoinv_train_forward(self._h, rays.data_ptr(), jitter.data_ptr(), n, int(S), int(bool(white_bg)),
                                                        int(bool(infoinv)), rgb.data_ptr(), depth.data_ptr(), C.byref(ticket), st))
        return rgb, depth, int(ticket.value)

    def counts(self):
        """(valid samples, active samples) of the rays the engine's buffers hold (ngf_debug_ii_counts, a test aid; waits for the stream)."""
        out = (C.c_int64 * 2)()
        with on_stream(self.dev) as st:
            _lib.check(self.L.ngf_debug_ii_counts(self._h, out, st))
        return int(out[0]), int(out[1])

    def backward(self, ticket, d_rgb, want):
        """``want[k]``: return parameter k's gradient (else None).  None = the ticket is stale (another forward used the buffers)."""
        with on_stream(self.dev) as st:
            return self._grads(self.L.ngf_infoinv_train_backward_grad(self._h, int(ticket), d_rgb.data_ptr(), st), want, st)


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
        grads = replay(ctx.field, '_ii_engine', lambda: ctx.field._infoinv_grad_engine(rays.shape[0], S), ctx.engine, ctx.ticket, saved[2:],
                       (rays, jitter, S, white_bg, infoinv), (d_rgb.to(dtype=torch.float32).contiguous(),),
                       [bool(w) for w in ctx.needs_input_grad[7:]])
        return (None,) * 7 + tuple(grads)


class Trainer(TrainerBase):
    """Adam state + the fused training step of one InfoInv field (the body of InfoInv/main.py:262-330):

        output = field(rays_train, is_train=True, white_bg=white_bg, N_samples=nSamples, infoinv=infoinv)
        total_loss = mean((rgb_map - rgb_train)**2) + L1_reg_weight * field.density_L1()
        optimizer.zero_grad(); total_loss.backward(); optimizer.step()          # Adam(get_optparam_groups, betas=(0.9, 0.99))
        for g in optimizer.param_groups: g['lr'] *= lr_factor

    ``step(rays_train, rgb_train)`` does that in two library calls on the field's differentiable engine (the autograd path keeps working on the
    same field); the nn.Parameters are updated in place.  Arguments as ``ngf_amd.train.Trainer``; learning rates per InfoInv/models/Field.py:27-37:
    the three planes at ``lr_init``, both decoders at ``lr_basis``.  There is no CPU path."""
    NAMES = PARAM_NAMES
    GET_GRAD = "ngf_infoinv_train_get_grad"

    def __init__(self, field, batch_size=4096, max_samples=None, lr_init=0.02, lr_basis=1e-3, lr_decay_iters=-1, lr_decay_target_ratio=0.1,
                 n_iters=30000, L1_reg_weight=L1_REG_WEIGHT, betas=(0.9, 0.99), eps=1e-8, frozen=(), state_from=None):
        if torch.device(field.device).type != "cuda":
            raise RuntimeError("ngf_amd.infoinv_train.Trainer runs on the GPU only (device='cuda'); there is no CPU path")
        self.L = _lib.lib()
        _bind(self.L)
        super().__init__(field, train_params(field), [lr_init] * 3 + [lr_basis] * (NPARAMS - 3), batch_size, max_samples, lr_decay_iters,
                         lr_decay_target_ratio, n_iters, L1_reg_weight, betas, eps, frozen, state_from)
        self._eng = None
        self._have_grads = False
        self._shape_key = _field_key(field, self.params)
        self._engine(self.batch_size, self.max_samples)

    def _engine(self, n, S):
        """The field's engine, sized for one ray chunk of the batch; this trainer's moments are the ones its handle updates."""
        f = self.field
        per = rays_per_chunk(f, S, MAX_PAIRS)      # the autograd path's rule (infoinv.TriPlane._render_train_infoinv)
        eng = getattr(f, '_ii_engine', None)
        if eng is not None and eng._h is not None and n > per and eng.max_rays > per:
            f.release_grad_engine()                 # built for more pairs than grad_max_pairs allows now: the library chunks by the engine's size
        eng = f._infoinv_grad_engine(min(int(n), per), S)
        if eng is not self._eng or eng._moments_owner is not self:
            m = (C.c_void_p * NPARAMS)(*[t.data_ptr() for t in self.exp_avg])
            v = (C.c_void_p * NPARAMS)(*[t.data_ptr() for t in self.exp_avg_sq])
            _lib.check(self.L.ngf_infoinv_train_set_moments(eng._h, m, v))
            eng._moments_owner = self
            if eng is not self._eng:
                self._have_grads = False
            self._eng = eng
        return eng

    def release(self):
        """Free the engine's device buffers if this trainer's engine is still the field's; the moments stay (``state_from=``)."""
        eng, self._eng = getattr(self, "_eng", None), None
        if eng is not None and getattr(self.field, '_ii_engine', None) is eng:
            self.field.release_grad_engine()

    def params_changed(self):
        """Tell the trainer that plane values were written by something that bumps no version counter (``.data`` writes, raw pointers): the
        channel-last copies are rebuilt at the next ``backward``.  In-place torch ops and ``load_state_dict`` are seen without it."""
        self.field._grad_stale = True

    @torch.no_grad()
    def backward(self, rays_train, rgb_train, N_samples=-1, white_bg=True, infoinv=True, jitter=None, coin=None, keep_loss=False):
        """forward(is_train=True) + backward of the rgb MSE; returns the rgb loss as a 0-dim float64 device tensor.  ``jitter`` [n] and ``coin``
        (a float in [0,1)) replace torch.rand_like / torch.rand((1,)) for parity tests.  A batch of more than ``field.grad_max_pairs`` pairs is
        worked through in ray chunks whose gradients add up; nothing is truncated.

        ALIASING: by default the returned tensor is a VIEW of the trainer's persistent loss buffer -- the next ``backward`` overwrites it in
        place.  Read it (``.item()``) before the next step, or pass ``keep_loss=True`` for a fresh tensor per step."""
        if _field_key(self.field, train_params(self.field)) != self._shape_key:
            raise RuntimeError("the field's parameters, alpha mask or geometry were re-allocated (load / a new mask): build a new Trainer")
        rays, tgt, n, S, jitter, white = self._batch(rays_train, rgb_train, N_samples, white_bg, jitter, coin)
        jitter = jitter.reshape(n)
        eng = self._engine(n, S)
        eng.sync_planes()
        with on_stream(eng.dev) as st:
            _lib.check(self.L.ngf_infoinv_train_step_backward(eng._h, rays.data_ptr(), tgt.data_ptr(), jitter.data_ptr(), n, S, int(white),
                                                              int(bool(infoinv)), self._loss.data_ptr(), st))
        self._have_grads = True
        return self._loss_out(keep_loss)

    def _grad_handle(self):
        if self._eng is None or self._eng._h is None or not self._have_grads:
            raise RuntimeError("gradient() needs a backward() first")
        return self._eng._h, self._eng.dev

    @torch.no_grad()
    def optimizer_step(self):
        """optimizer.step() + the lr decay of main.py:298-299.  Frozen parameters get no update and their step counters stay.  One update per
        ``backward``.  A differentiable forward of the same field under autograd between ``backward`` and this call goes through the same
        engine and retires the gradients: the library then refuses the update (a RuntimeError from this call) -- run ``backward`` again."""
        eng = self._eng
        if eng is None or eng._h is None or not self._have_grads or getattr(self.field, '_ii_engine', None) is not eng:
            raise RuntimeError("optimizer_step() needs a backward() first")
        if eng._moments_owner is not self:
            raise RuntimeError("another Trainer used this field's engine since the backward: run backward() again")
        counts, lrs, _ = self._advance()
        with on_stream(eng.dev) as st:
            _lib.check(self.L.ngf_infoinv_train_adam_all(eng._h, counts, lrs, float(self.betas[0]), float(self.betas[1]), float(self.eps),
                                                         float(self.l1), st))
        self._have_grads = False         # one update per backward: a second optimizer_step() raises instead of applying the gradients again
        self.field.invalidate()          # parameters changed behind torch's back: the eval image is re-packed on the next render ...
        self.field._grad_stale = False   # ... but the engine's packed planes were written by the Adam pass itself
        self._decay()


def fit(field, allrays, allrgbs, args, white_bg=True, infoinv=True, on_iteration=None):
    """The optimisation loop of InfoInv/main.py:243-336 on top of ``Trainer`` -- no dataset, logging or checkpoint code (those stay with the
    caller; ``on_iteration(iteration, rgb_loss)`` is the hook for them).  The InfoInv loop has no ``shrink`` and no up-sampling.

    ``args``: the reference's namespace: batch_size, n_iters, lr_init, lr_basis, lr_decay_iters, lr_decay_target_ratio, update_AlphaMask_list,
    nSamples, step_ratio.  Returns the per-iteration PSNR list."""
    from . import geometry
    from .train import SimpleSampler
    dev = torch.device(field.device)
    mask_list = list(args.update_AlphaMask_list or [])
    nSamples = min(int(args.nSamples), geometry.cal_n_samples([int(v) for v in field.gridSize], args.step_ratio))
    allrays, allrgbs = field.filtering_rays(allrays, allrgbs, bbox_only=True)
    sampler = SimpleSampler(allrays.shape[0], args.batch_size)

    def new_trainer(state_from=None, l1=L1_REG_WEIGHT):
        return Trainer(field, batch_size=args.batch_size, max_samples=nSamples, lr_init=args.lr_init, lr_basis=args.lr_basis,
                       lr_decay_iters=args.lr_decay_iters, lr_decay_target_ratio=args.lr_decay_target_ratio, n_iters=args.n_iters,
                       L1_reg_weight=l1, state_from=state_from)

    l1 = L1_REG_WEIGHT
    trainer = new_trainer()
    PSNRs = []
    for iteration in range(args.n_iters):
        ids = sampler.nextids()
        rays_train, rgb_train = allrays[ids].to(dev), allrgbs[ids].to(dev)
        rgb_loss = trainer.step(rays_train, rgb_train, N_samples=nSamples, white_bg=white_bg, infoinv=infoinv).item()
        PSNRs.append(-10.0 * np.log(rgb_loss) / np.log(10.0))
        if on_iteration is not None:
            on_iteration(iteration, rgb_loss)
        if iteration in mask_list:
            field.updateAlphaMask((256, 256, 256), infoinv=infoinv)
            if iteration == mask_list[0]:
                l1 = 4e-5                                                    # main.py:328
                allrays, allrgbs = field.filtering_rays(allrays, allrgbs)
                sampler = SimpleSampler(allrgbs.shape[0], args.batch_size)
            old = trainer
            trainer = new_trainer(state_from=old, l1=l1)                     # new mask -> new device image
            old.release()
    trainer.release()
    return PSNRs
