"""What the three training paths share above the C ABI (train.py: TriPlane, infoinv_train.py: InfoInv, uv_train.py: UV-Mapping / NeuTex): the
engine behind a differentiable forward (``GradEngine``) and the get-or-grow rule of the one a model keeps (``grad_engine``), the backward of the
autograd nodes (``replay``), descriptor fields and the ray-chunking forward of the two plane fields (``fill_geometry``, ``render_train``), and the
Adam bookkeeping of the fused trainers (``TrainerBase``).  Each module keeps its descriptor, the arguments of its library calls and its node."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib


class on_stream(torch.cuda.device):
    """``with on_stream(dev) as st:`` -- ``dev`` is the current device inside, ``st`` its current stream as the library's calls take it."""

    def __enter__(self):
        super().__enter__()
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Handle:
    """An object that owns one library handle ``_h`` of ``self.L``; ``DESTROY`` names the C entry point that frees it."""
    DESTROY = None
    _h = None

    def release(self):
        if self._h is not None:
            getattr(self.L, self.DESTROY)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class GradEngine(Handle):
    """The device side of a differentiable forward for batches of up to ``max_rays`` x ``max_samples``.  A subclass names its C entry points, fills
    its descriptor, creates ``_h`` and sets ``key`` (what ``_key`` gives for the tensors it was built from); ``forward`` and the arguments of its
    backward call are its own."""
    BYTES = PARAMS_CHANGED = GET_GRADS = None
    STALE = slice(None)             # the slice of ``params`` whose torch version counters mark the trainer's packed copies stale
    FIELD_STALE = True              # ``field._grad_stale`` (Base.invalidate: writes that bump no counter) marks them stale as well
    GROWS_FROM_RELEASED = True      # grad_engine: a released engine still left in the model's attribute counts towards its successor's shape

    def __init__(self, field, dev, params, max_rays, max_samples):
        self.field, self.dev, self.params = field, dev, params
        self.max_rays, self.max_samples = int(max_rays), int(max_samples)
        self.L = _lib.lib()
        self._versions = None       # the first forward reports the parameters

    def _key(self, params):
        raise NotImplementedError

    @property
    def bytes(self) -> int:
        return int(getattr(self.L, self.BYTES)(self._h)) if self._h is not None else 0

    def fits(self, n, S, params):
        return n <= self.max_rays and S <= self.max_samples and self.key == self._key(params)

    def sync(self):
        """Tell the trainer (params_changed) when a version counter moved since the last look -- optimizer.step(), load_state_dict -- or the field
        was invalidated.  The library's own Adam writes the packed copies itself and bumps nothing.  True = it was told."""
        v = tuple(int(p._version) for p in self.params[self.STALE])
        if v != self._versions or (self.FIELD_STALE and getattr(self.field, "_grad_stale", False)):
            _lib.check(getattr(self.L, self.PARAMS_CHANGED)(self._h))
            self._versions = v
            if self.FIELD_STALE:
                self.field._grad_stale = False
            return True
        return False

    def _grads(self, rc, want, st):
        """The tail of ``backward`` (inside its ``on_stream``), ``rc`` the backward call's answer: None = the ticket is stale (NGF_E_STALE: another
        forward used the buffers); every other failure raises (a HIP / launch failure must not be retried away).  ``want[k]``: return parameter
        k's gradient (else None), all of them in one call."""
        if rc == _lib.E_STALE:
            return None
        _lib.check(rc)
        grads = [torch.empty_like(p) if w else None for p, w in zip(self.params, want)]
        ptrs = (C.c_void_p * len(grads))(*[None if g is None else g.data_ptr() for g in grads])
        _lib.check(getattr(self.L, self.GET_GRADS)(self._h, ptrs, st))
        return grads


def grad_engine(model, attr, cls, params, n, S):
    """The engine ``model`` keeps in ``attr``, fit for ``n`` rays x ``S`` samples of ``params``; anything else is released and replaced by a
    ``cls(model, rays, samples)`` for the larger of both shapes, so alternating batch shapes settle on one engine."""
    eng = getattr(model, attr, None)
    if eng is not None and eng._h is not None and eng.fits(n, S, params):
        return eng
    n, S = int(n), int(S)
    if eng is not None:
        if eng._h is not None or cls.GROWS_FROM_RELEASED:
            n, S = max(n, eng.max_rays), max(S, eng.max_samples)
        eng.release()
        setattr(model, attr, None)
    eng = cls(model, n, S)
    setattr(model, attr, eng)
    return eng


def release_engine(model, attr):
    eng = getattr(model, attr, None)
    if eng is not None:
        eng.release()
        setattr(model, attr, None)


def replay(model, attr, engine, first, ticket, saved, inputs, d, want, whose="field", before_rerender=None):
    """The gradients of one autograd node: ``first`` / ``ticket`` are the engine and ticket of its forward, ``saved`` the parameter tensors it saw,
    ``inputs`` the arguments of ``forward``, ``d`` the incoming gradients of ``backward``.  The engine is the model's CURRENT one: that of the
    forward (the common case: its identity is the whole check), unless a larger batch or a re-allocation had it rebuilt in between (``engine()``
    gets it).  After another forward through the engine (a stale ticket), or on a new engine, the batch is rendered again, then its backward;
    ``before_rerender(eng)`` is called first then: the place to refuse when the engine no longer holds the state the forward ran with
    (uv_train.py: the occupancy mask)."""
    eng = first
    if getattr(model, attr, None) is not eng or eng._h is None:
        eng = engine()
    if any(a.data_ptr() != b.data_ptr() or a.shape != b.shape for a, b in zip(saved, eng.params)):
        raise RuntimeError(f"the {whose}'s parameter tensors were re-allocated between forward and backward")
    grads = eng.backward(ticket, *d, want) if eng is first else None
    if grads is None:
        if before_rerender is not None:
            before_rerender(eng)
        *_, ticket = eng.forward(*inputs)
        grads = eng.backward(ticket, *d, want)
        if grads is None:
            raise RuntimeError(_lib.lib().ngf_last_error().decode())
    return grads


def fill_geometry(d, f, dev, weight_thres):
    """The fields ngf_train_desc and ngf_infoinv_train_desc share: ray geometry, the march's constants and the alpha mask.  Returns the tensors the
    descriptor points into (the packed mask bits): keep them for as long as the handle lives."""
    d.aabb = (C.c_float * 6)(*f._aabb_host())
    d.near_, d.far_ = float(f.near_far[0]), float(f.near_far[1])
    d.step = float(f.stepSize)
    d.distance_scale = float(f.distance_scale)
    d.weight_thres = weight_thres
    keep = []
    if f.alphaMask is not None:
        bits = f.alphaMask.packed_bits_device().to(dev)
        keep.append(bits)
        d.mask_bits = bits.data_ptr()
        shp = f.alphaMask.alpha_volume.shape
        d.mask_d, d.mask_h, d.mask_w = int(shp[-3]), int(shp[-2]), int(shp[-1])
        d.mask_aabb = (C.c_float * 6)(*f.alphaMask.aabb.reshape(-1).tolist())
    return keep


def rays_per_chunk(field, S, default):
    """At most ``field.grad_max_pairs`` (``default`` when unset) (ray, sample) pairs go through an engine at once."""
    return max(1, max(int(getattr(field, 'grad_max_pairs', default)), int(S)) // int(S))


def render_train(field, rays_chunk, white_bg, N_samples, flag, jitter, coin, default_pairs, engine, fn):
    """``forward(is_train=True)`` with gradients: the random draws of ``_render`` (jitter: torch.rand_like of sample_ray, FieldBase.py:128-130; the
    background coin: FieldBase.py:299), then one autograd node ``fn`` over the parameters of ``engine(rays, samples)``.  The engine keeps buffers
    per (ray, sample) pair, so a call beyond ``grad_max_pairs`` pairs is cut into ray chunks, one node each: the engine holds ONE chunk and the
    backward renders every chunk but the last again (what two forwards before one backward always did) -- bounded memory for twice the forward."""
    dev = torch.device(field.device)
    rays = rays_chunk.detach().to(device=dev, dtype=torch.float32).contiguous()
    if rays.dim() != 2 or rays.shape[1] != 6:
        raise ValueError(f"rays_chunk must be [n,6], got {tuple(rays.shape)}")
    n = rays.shape[0]
    if n == 0:
        raise ValueError("a differentiable forward needs at least one ray")
    S = int(N_samples) if N_samples > 0 else int(field.nSamples)
    jitter = torch.rand((n,), device=dev) if jitter is None else jitter.detach().to(device=dev, dtype=torch.float32).reshape(n).contiguous()
    white = bool(white_bg or ((torch.rand((1,)) if coin is None else torch.tensor([float(coin)])) < 0.5))
    per = rays_per_chunk(field, S, default_pairs)
    if n <= per:
        eng = engine(n, S)
        rgb, depth = fn.apply(field, eng, rays, jitter, S, white, bool(flag), *eng.params)
        return {'rgb_map': rgb, 'depth_map': depth}
    outs = []
    for a in range(0, n, per):
        r, j = rays[a:a + per], jitter[a:a + per]
        eng = engine(r.shape[0], S)
        outs.append(fn.apply(field, eng, r, j, S, white, bool(flag), *eng.params))
    return {'rgb_map': torch.cat([o[0] for o in outs], 0), 'depth_map': torch.cat([o[1] for o in outs], 0)}


class TrainerBase:
    """Adam state of a fused ``Trainer`` -- moments in the parameters' layouts, one step counter per parameter as torch.optim.Adam keeps them,
    learning rates and their decay -- and the parts of an iteration that do not depend on the model.  A subclass sets ``self.L``, names its
    parameters (``NAMES``) and its single-gradient call (``GET_GRAD``), and writes ``backward`` and ``optimizer_step`` around its library calls."""
    NAMES = ()
    GET_GRAD = None
    EMPTY_OK = False                # a batch without rays passes the batch check

    def __init__(self, field, params, lr, batch_size, max_samples, lr_decay_iters, lr_decay_target_ratio, n_iters, L1_reg_weight, betas, eps,
                 frozen, state_from):
        self.field, self.params = field, params
        self.dev = torch.device(field.device)
        self.exp_avg = [torch.zeros_like(p) for p in params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in params]
        self.steps = [0] * len(params)              # torch.optim.Adam keeps one step counter per parameter
        self.frozen = set(self.NAMES.index(k) if isinstance(k, str) else int(k) for k in frozen)      # parameters optimizer_step leaves alone
        self.lr = lr
        self.lr_factor = lr_decay_target_ratio ** (1 / (lr_decay_iters if lr_decay_iters > 0 else n_iters))
        self.betas, self.eps, self.l1 = betas, eps, L1_reg_weight
        self.batch_size = int(batch_size)
        self.max_samples = int(max_samples if max_samples is not None else field.nSamples)
        if state_from is not None:                  # carry the optimiser state of parameters that kept their shape
            for k in range(len(params)):
                if state_from.exp_avg[k].shape == self.exp_avg[k].shape:
                    self.exp_avg[k].copy_(state_from.exp_avg[k])
                    self.exp_avg_sq[k].copy_(state_from.exp_avg_sq[k])
                    self.steps[k] = state_from.steps[k]
            self.lr = list(state_from.lr)
        self._loss = torch.zeros((2,), dtype=torch.float64, device=self.dev)      # [sum of squared residuals, their mean]

    def _batch(self, rays_train, rgb_train, N_samples, white_bg, jitter, coin):
        """-> (rays [n,6], targets [n,3], n, S, jitter, white background) of one ``backward``: checked, float32, contiguous, on the device;
        ``jitter`` and ``coin`` (a float in [0,1)) replace torch.rand_like (FieldBase.py:128-130) / torch.rand((1,)) (FieldBase.py:299)."""
        rays = rays_train.to(device=self.dev, dtype=torch.float32).contiguous()
        tgt = rgb_train.to(device=self.dev, dtype=torch.float32).contiguous()
        n = rays.shape[0]
        if rays.dim() != 2 or rays.shape[1] != 6 or tuple(tgt.shape) != (n, 3) or (n == 0 and not self.EMPTY_OK):
            raise ValueError(f"rays_train must be [n,6] and rgb_train [n,3]{'' if self.EMPTY_OK else ' with n > 0'}, "
                             f"got {tuple(rays.shape)} / {tuple(tgt.shape)}")
        S = int(N_samples) if N_samples > 0 else int(self.field.nSamples)
        if jitter is None:
            jitter = torch.rand((n,), device=self.dev)
        jitter = jitter.to(device=self.dev, dtype=torch.float32).contiguous()
        white = bool(white_bg or ((float(torch.rand((1,))) if coin is None else float(coin)) < 0.5))
        return rays, tgt, n, S, jitter, white

    def _loss_out(self, keep_loss):
        """The rgb loss of the last ``backward``: a VIEW of the persistent loss buffer (the step's last kernel writes the mean there; a torch op
        here would be one more launch per step) that the next ``backward`` overwrites, or with ``keep_loss`` a fresh tensor."""
        return self._loss[1].clone() if keep_loss else self._loss[1]

    def _skipped(self, k):
        """Parameter k has no gradient this step (torch.optim skips parameters whose .grad is None); frozen ones are skipped anyway."""
        return False

    def _advance(self):
        """The per-parameter arrays of one Adam call: step counts (0 = skipped; a skipped parameter keeps its counter), learning rates, and the
        indices that are updated."""
        n = len(self.params)
        counts, idx = (C.c_int32 * n)(), []
        for k in range(n):
            if k in self.frozen or self._skipped(k):
                continue
            self.steps[k] += 1
            counts[k] = self.steps[k]
            idx.append(k)
        return counts, (C.c_float * n)(*[float(x) for x in self.lr]), idx

    def _decay(self):
        self.lr = [x * self.lr_factor for x in self.lr]                # main.py:298-299

    def _grad_handle(self):
        """(handle, device) ``gradient`` reads from."""
        return self._h, self.dev

    @torch.no_grad()
    def gradient(self, which) -> torch.Tensor:
        """The gradient of one parameter (index or state_dict name) in its reference layout, after ``backward``.
        Planes exclude the L1 term (it is added inside the Adam kernel)."""
        k = self.NAMES.index(which) if isinstance(which, str) else int(which)
        h, dev = self._grad_handle()
        out = torch.empty_like(self.params[k])
        with on_stream(dev) as st:
            _lib.check(getattr(self.L, self.GET_GRAD)(h, k, out.data_ptr(), st))
        return out

    def step(self, *args, **kw):
        """One iteration: ``backward(...)`` + ``optimizer_step()``.  Returns the rgb loss (0-dim float64 device tensor; ``.item()`` for PSNR) -- a
        view of the trainer's loss buffer that the next step overwrites unless ``keep_loss=True`` (see ``backward``)."""
        loss = self.backward(*args, **kw)
        self.optimizer_step()
        return loss
