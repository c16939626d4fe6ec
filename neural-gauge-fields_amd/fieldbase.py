"""Drop-in counterparts of the reference's ``Base`` / ``AlphaGridMask`` (TriPlane/models/FieldBase.py:22-116,
251-312; InfoInv/models/FieldBase.py) and ``renderer`` (TriPlane/main.py:60-71).

Same constructor arguments, attribute and parameter names, checkpoint dictionary and ``forward``
signature; ``forward`` hands the whole ray batch to the gfx950 library (include/ngf.h) in ONE launch
instead of running ~40 ATen ops per chunk.  PyTorch is used for device memory, streams and the
``nn.Module`` / ``state_dict`` plumbing only.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _engine, _lib, geometry


class AlphaGridMask(torch.nn.Module):
    """Occupancy volume container (FieldBase.py:22-40); the kernel consumes its np.packbits image."""

    def __init__(self, device, aabb, alpha_volume):
        super().__init__()
        self.device = device
        self.aabb = aabb.to(self.device)
        self.aabbSize = self.aabb[1] - self.aabb[0]
        self.invgridSize = 1.0 / self.aabbSize * 2
        self.alpha_volume = alpha_volume.view(1, 1, *alpha_volume.shape[-3:])
        self.gridSize = torch.LongTensor([alpha_volume.shape[-1], alpha_volume.shape[-2], alpha_volume.shape[-3]]).to(self.device)

    def packed_bits(self) -> np.ndarray:
        """The checkpoint image (FieldBase.py:104-108), on the host."""
        return np.packbits(self.alpha_volume.bool().cpu().numpy().reshape(-1))

    def packed_bits_device(self) -> torch.Tensor:
        """The same bytes built on the device (ngf_pack_mask_bits) -- what the render handle consumes."""
        vol = self.alpha_volume
        if not vol.is_cuda:
            return torch.from_numpy(self.packed_bits())
        v = vol.to(torch.float32).contiguous().view(-1)
        bits = torch.empty(((v.numel() + 7) // 8,), dtype=torch.uint8, device=v.device)
        with torch.cuda.device(v.device):
            _lib.check(_lib.lib().ngf_pack_mask_bits(v.data_ptr(), v.numel(), bits.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return bits


class Base(torch.nn.Module):
    MODEL = _lib.MODEL_TRIPLANE
    PLANE_C = 64
    DENS_DIM = 16

    def __init__(self, aabb, gridSize, device, alphaMask=None, near_far=[2.0, 6.0], alphaMask_thres=0.001,
                 distance_scale=25, rayMarch_weight_thres=0.0001, step_ratio=2.0, gauge_start=0, bake_density=None,
                 bake_color=None, no_fold=False, split_bf16=False):
        super().__init__()
        self.aabb = aabb if torch.is_tensor(aabb) else torch.tensor(aabb, dtype=torch.float32)
        self.alphaMask = alphaMask
        self.device = device
        self.alphaMask_thres = alphaMask_thres
        self.distance_scale = distance_scale
        self.rayMarch_weight_thres = rayMarch_weight_thres
        self.near_far = near_far
        self.step_ratio = step_ratio
        # Optimisation levels of the TriPlane render: 0 = no_fold (rgb_decoder as written), 1 = layer 1 pre-composed with
        # `basis` + per-ray view fold, 2 = level 1 + density_decoder folded into 1-channel planes (bake_density: Linear(48,1) commutes with
        # bilinear interpolation, fp64 accumulate at pack time, |d sigma| <= 2e-6 relative), 3 = level 2 + layer 1 folded into 64-channel
        # pre-activation planes (bake_color) -- both halves of SURVEY section 7's fold (iii).  LEVEL 3 IS THE DEFAULT since round 4 (its
        # gather became quad-coalesced: 87 -> 142 Mray/s on the R1 frame, level 2: 83).  Every level is parity-tested against the oracle and
        # the reference's golden pixels with the same tolerances; bake_color=False gives level 2, bake_density=False level 1.
        # bake_density=None (the default) resolves to level 2 unless the un-composed level 0 is asked for: NGF_F_NO_FOLD excludes the
        # NGF_F_BAKE_* flags (ngf_field_create rejects the combination), so TriPlane(..., no_fold=True) alone must give level 0.
        self.no_fold = bool(no_fold)                # NGF_F_NO_FOLD (TriPlane): rgb_decoder exactly as written, for measurements
        if self.no_fold and (bake_density or bake_color):
            raise ValueError("no_fold=True is the un-composed formulation (level 0): it excludes bake_density / bake_color")
        self.bake_density = (not self.no_fold) if bake_density is None else bool(bake_density)      # NGF_F_BAKE_DENSITY (TriPlane)
        # NGF_F_BAKE_COLOR (TriPlane): on by default where it applies -- on top of the baked density, and not with the bf16 split (which works
        # on the pre-composed layer 1, ngf_field_create rejects the combination)
        self.bake_color = (self.bake_density and not self.no_fold and not bool(split_bf16)) if bake_color is None else bool(bake_color)
        self.split_bf16 = bool(split_bf16)          # NGF_F_SPLIT_BF16 (TriPlane): colour MLP on bf16 MFMA with 3-term split operands
        self._handle = None
        self._handle_key = None
        self.last_stats = None
        self.init_para(gridSize)
        self.init_model(device=device, gauge_start=gauge_start)

    # --- init_para (FieldBase.py:63-74): same attributes, arithmetic restated in geometry.py ------
    def init_para(self, gridSize):
        aabb = self.aabb.detach().cpu().numpy().astype(np.float32)
        self.aabbSize = self.aabb[1] - self.aabb[0]
        self.invaabbSize = 2.0 / self.aabbSize
        self.gridSize = torch.LongTensor([int(g) for g in gridSize]).to(self.device)
        self.units = self.aabbSize.to(self.device) / (self.gridSize - 1)
        step = geometry.step_size(aabb, [int(g) for g in gridSize], self.step_ratio)
        self.stepSize = torch.tensor(step, dtype=torch.float32)
        self.aabbDiag = torch.sqrt(torch.sum(torch.square(self.aabbSize)))
        self.nSamples = geometry.n_samples(aabb, step)
        self._handle_key = None

    def init_model(self, device=None, gauge_start=0):
        raise NotImplementedError

    # --- checkpoint format (FieldBase.py:94-116) ---------------------------------------------------
    def save(self, path):
        kwargs = {'aabb': self.aabb, 'gridSize': self.gridSize.tolist(), 'alphaMask_thres': self.alphaMask_thres,
                  'distance_scale': self.distance_scale, 'rayMarch_weight_thres': self.rayMarch_weight_thres,
                  'near_far': self.near_far, 'step_ratio': self.step_ratio}
        ckpt = {'kwargs': kwargs, 'state_dict': self.state_dict()}
        if self.alphaMask is not None:
            alpha_volume = self.alphaMask.alpha_volume.bool().cpu().numpy()
            ckpt.update({'alphaMask.shape': alpha_volume.shape})
            ckpt.update({'alphaMask.mask': np.packbits(alpha_volume.reshape(-1))})
            ckpt.update({'alphaMask.aabb': self.alphaMask.aabb.cpu()})
        torch.save(ckpt, path)

    def load(self, ckpt):
        if 'alphaMask.aabb' in ckpt.keys():
            length = int(np.prod(ckpt['alphaMask.shape']))
            vol = torch.from_numpy(np.unpackbits(ckpt['alphaMask.mask'])[:length].reshape(ckpt['alphaMask.shape']))
            self.alphaMask = AlphaGridMask(self.device, ckpt['alphaMask.aabb'].to(self.device), vol.float().to(self.device))
        sd = ckpt['state_dict']
        # planes of a trained checkpoint were up-sampled / shrunk (Field.py:108-132): size them from the
        # state_dict (the reference's own loader raises a size mismatch here)
        for name in ('plane_xy', 'plane_yz', 'plane_xz', 'gauge_xy', 'gauge_yz', 'gauge_xz'):
            if name in sd and hasattr(self, name) and getattr(self, name).shape != sd[name].shape:
                setattr(self, name, torch.nn.Parameter(torch.empty_like(sd[name], device=self.device)))
        self.load_state_dict(sd)
        self._handle_key = None

    def load_params(self, params: dict):
        """Assign parameters from a dict of numpy arrays keyed by state_dict names (test / bench plumbing)."""
        sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()}
        self.load({'state_dict': sd})

    # --- the HIP handle ----------------------------------------------------------------------------
    def _aabb_host(self):
        """The six floats of ``self.aabb`` on the host, fetched once per (tensor, version).  The reference's drivers keep aabb on the GPU
        (``scene_bbox.to(device)``, TriPlane/main.py:211): ``aabb.tolist()`` in the per-call handle key was then a device-to-host copy plus a
        stream synchronisation in front of EVERY render call and every training step -- nothing could be enqueued behind a running launch."""
        a = self.aabb
        key = (id(a), a.data_ptr(), a._version)
        c = getattr(self, '_aabb_cache', None)
        if c is None or c[0] != key:
            c = (key, tuple(float(v) for v in a.detach().reshape(-1).tolist()))
            self._aabb_cache = c
        return c[1]

    def _param_key(self):
        ps = [(n, p.data_ptr(), p._version, tuple(p.shape)) for n, p in self.named_parameters()]
        if getattr(self, 'check_params', False):
            ps.append(tuple(float(p.detach().double().sum()) + float(p.detach().double().abs().sum()) for p in self.parameters()))
        m = None if self.alphaMask is None else (self.alphaMask.alpha_volume.data_ptr(), self.alphaMask.alpha_volume._version)
        return (tuple(ps), m, float(self.stepSize), self._aabb_host(), self.bake_density, self.bake_color, self.no_fold, self.split_bf16,
                tuple(self.near_far), float(self.distance_scale), float(self.rayMarch_weight_thres))

    # --- differentiable training-mode forward (FieldBase.py:251-312 under autograd; the loop of TriPlane/main.py:272-296) ------------------
    def _render_grad_engine(self, n, S):
        """The device trainer behind ``forward(is_train=True)`` with autograd on (ngf_amd.train.RenderGrad); rebuilt when the batch outgrows it
        or the parameter tensors were re-allocated (up_sampling / shrink / load).  One key computation per call (the loop of main.py:272-296 pays
        it once per iteration: ``_render_train`` takes the parameter list from the engine, the backward checks the engine's identity)."""
        from . import train
        return _engine.grad_engine(self, '_grad_engine', train.RenderGrad, train._train_params(self), n, S)

    def _wants_grad(self, is_train):
        if not (is_train and torch.is_grad_enabled()):
            return False
        slots = getattr(self, '_tp_slots', None)          # the fifteen parameters without walking the module tree (train._train_params)
        if slots is not None:
            return any(m._parameters[a].requires_grad for m, a in slots)
        return any(p.requires_grad for p in self.parameters())

    def _render_train(self, rays_chunk, white_bg, N_samples, gauge_on, jitter=None, coin=None):
        """``forward(is_train=True)`` with gradients (``_engine.render_train``): one torch.autograd.Function over the fifteen parameters.  The
        reference's loop works unchanged on the result: ``loss(out['rgb_map'], ...) + w * field.density_L1()``, ``.backward()``,
        ``torch.optim.Adam(field.get_optparam_groups(...)).step()`` (TriPlane/main.py:272-296).
        Memory: the engine keeps per-(ray, sample) buffers (136 B per pair) and activation rows for a third of the pairs (2.4 KB each) --
        3.4 GiB at the reference's 4096 x 884 batch; the default ``grad_max_pairs`` of 2^24 is 4.6 batches of that size, ~16 GiB."""
        from . import train
        return _engine.render_train(self, rays_chunk, white_bg, N_samples, gauge_on, jitter, coin, 1 << 24, self._render_grad_engine,
                                    train._TrainRender)

    def invalidate(self):
        """Force the packed device image to be rebuilt at the next call.  The handle is rebuilt automatically when a parameter
        tensor is replaced or modified through autograd-tracked in-place ops (optimizer.step(), load_state_dict, up_sampling,
        shrink: they bump ``Parameter._version``).  Writes that bypass the version counter -- ``param.data.mul_(...)``, raw
        pointer writes from another library -- are invisible to it: call ``invalidate()`` after them, or set
        ``field.check_params = True`` (debug: the key then carries a device-side checksum of every parameter, one sync per call)."""
        self._handle_key = None
        self._grad_stale = True           # the differentiable forward's packed plane copies as well (train.RenderGrad.forward)

    def _fill_desc(self, d: _lib.FieldDesc, keep: list):
        raise NotImplementedError

    def release(self, trim=False):
        """Destroy the packed device image.  The library waits for the streams the handle was used on (on the handle's own device) and parks
        its buffers for the next ``handle()`` of the same shapes; ``trim=True`` also returns the parked buffers to the driver (after
        up_sampling / shrink the old sizes never match again, and torch's caching allocator cannot see memory this pool holds)."""
        if self._handle is not None:
            _lib.lib().ngf_field_destroy(self._handle)
            self._handle = None
            self._handle_key = None
            self._handle_shapes = None
        if trim:
            _lib.lib().ngf_pool_trim()

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def handle(self):
        """(Re)build the packed device image when parameters changed since the last call."""
        key = self._param_key()
        if self._handle is not None and key == self._handle_key:
            return self._handle
        L = _lib.lib()
        dev = torch.device(self.device)
        if dev.type != 'cuda':
            raise RuntimeError("ngf_amd fields render on the GPU only (device='cuda'); there is no CPU path")
        d = _lib.FieldDesc()
        keep = []
        d.model, d.plane_c, d.dens_dim = self.MODEL, self.PLANE_C, self.DENS_DIM
        d.flags = _lib.F_SPLIT_BF16 if self.split_bf16 else 0
        if self.MODEL == _lib.MODEL_TRIPLANE:
            d.flags = ((_lib.F_BAKE_DENSITY if self.bake_density else 0) | (_lib.F_BAKE_COLOR if self.bake_color else 0) |
                       (_lib.F_NO_FOLD if self.no_fold else 0) | (_lib.F_SPLIT_BF16 if self.split_bf16 else 0))

        def dp(t):
            t = t.detach().to(device=dev, dtype=torch.float32).contiguous()
            keep.append(t)
            return t.data_ptr()

        for k, name in enumerate(('plane_xy', 'plane_yz', 'plane_xz')):
            pl = getattr(self, name)
            d.plane[k] = dp(pl)
            d.plane_h[k], d.plane_w[k] = pl.shape[2], pl.shape[3]
        self._fill_desc(d, dp)
        rd = self.rgb_decoder
        d.basis = dp(rd.basis.weight)
        d.w1, d.b1 = dp(rd.mlp[0].weight), dp(rd.mlp[0].bias)
        d.w2, d.b2 = dp(rd.mlp[2].weight), dp(rd.mlp[2].bias)
        d.w3, d.b3 = dp(rd.mlp[4].weight), dp(rd.mlp[4].bias)
        d.aabb = (C.c_float * 6)(*self._aabb_host())
        d.near_, d.far_ = float(self.near_far[0]), float(self.near_far[1])
        d.step = float(self.stepSize)
        d.distance_scale = float(self.distance_scale)
        d.weight_thres = float(np.float32(self.rayMarch_weight_thres))
        if self.alphaMask is not None:
            bits = self.alphaMask.packed_bits_device().to(dev)
            keep.append(bits)
            d.mask_bits = bits.data_ptr()
            shp = self.alphaMask.alpha_volume.shape
            d.mask_d, d.mask_h, d.mask_w = int(shp[-3]), int(shp[-2]), int(shp[-1])
            d.mask_aabb = (C.c_float * 6)(*self.alphaMask.aabb.reshape(-1).tolist())
        # the old image goes first: its buffers are what the new one is built in (same shapes after a parameter update -- exact-size reuse from
        # the library's pool, no second image resident; other shapes after up_sampling / shrink / a new mask -- the stale sizes go back to the driver)
        shapes = (tuple(int(x) for x in d.plane_h), tuple(int(x) for x in d.plane_w), tuple(int(x) for x in d.gauge_h), tuple(int(x) for x in d.gauge_w),
                  int(d.flags), int(d.mask_d), int(d.mask_h), int(d.mask_w))
        old = getattr(self, '_handle_shapes', None)
        self.release(trim=old is not None and old != shapes)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            out = C.c_void_p()
            _lib.check(L.ngf_field_create(C.byref(d), C.byref(out), C.c_void_p(stream)))
        self._handle, self._handle_key, self._handle_shapes = out, key, shapes
        return out

    def _mode(self, **kw) -> int:
        raise NotImplementedError

    # --- Base.forward (FieldBase.py:251-312) ---------------------------------------------------------
    @torch.no_grad()
    def _render(self, rays_chunk, white_bg, is_train, N_samples, mode, collect_stats=False, out=None, jitter=None, coin=None, row_width=0):
        """``jitter`` [n] and ``coin`` (a float in [0,1)) replace the torch.rand_like of sample_ray (FieldBase.py:128-130) and the
        torch.rand((1,)) of the random background (FieldBase.py:299) in training mode -- parity tests against captured reference forwards.
        ``row_width`` > 0: the ray list is an image with that many rays per row (ngf_field_render_image: the same pixels, the launch walks the image
        in screen-space blocks; ``renderer(..., row_width=W)`` / ``evalout.evaluation`` pass it)."""
        dev = torch.device(self.device)
        rays = rays_chunk.to(device=dev, dtype=torch.float32).contiguous()
        if rays.dim() != 2 or rays.shape[1] != 6:
            raise ValueError(f"rays_chunk must be [n,6], got {tuple(rays.shape)}")
        n = rays.shape[0]
        S = int(N_samples) if N_samples > 0 else int(self.nSamples)
        h = self.handle()
        if out is not None:
            rgb, depth = out                      # caller-provided device buffers ([n,3], [n], contiguous float32)
            assert rgb.is_contiguous() and depth.is_contiguous() and rgb.shape == (n, 3) and depth.shape == (n,)
        else:
            rgb = torch.empty((n, 3), device=dev, dtype=torch.float32)
            depth = torch.empty((n,), device=dev, dtype=torch.float32)
        if n == 0:
            return {'rgb_map': rgb, 'depth_map': depth}
        if is_train:
            jitter = torch.rand((n,), device=dev) if jitter is None else jitter.to(device=dev, dtype=torch.float32).reshape(n).contiguous()
        else:
            jitter = None
        if not (white_bg or (is_train and (torch.rand((1,)) if coin is None else torch.tensor([float(coin)])) < 0.5)):
            white_bg = False
        else:
            white_bg = True
        stats = torch.zeros(16, dtype=torch.int64, device=dev) if collect_stats else None   # [4:] = section cycles under the profile knob
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            _lib.check(_lib.lib().ngf_field_render_image(
                h, rays.data_ptr(), n, int(row_width or 0), S, int(white_bg), int(mode), None if jitter is None else jitter.data_ptr(),
                rgb.data_ptr(), depth.data_ptr(), None if stats is None else stats.data_ptr(), C.c_void_p(stream)))
        if collect_stats:
            self.last_stats = stats
        return {'rgb_map': rgb, 'depth_map': depth}

    # --- model management on top of the march's device code ---------------------------------
    def _alpha_mode(self, **kw) -> int:
        """Kernel mode of compute_alpha: TriPlane runs it with the gauge OFF (iteration=-1, FieldBase.py:154); the InfoInv tree
        passes infoinv=True/False down to compute_density (InfoInv/models/FieldBase.py:140-156)."""
        if kw:
            raise TypeError(f"unexpected keyword arguments {sorted(kw)}")
        return 0

    @torch.no_grad()
    def compute_alpha(self, xyz_locs, length=1, **kw):
        """FieldBase.py:140-159 (InfoInv: compute_alpha(xyz_locs, length=1, infoinv=True)): alpha = 1 - exp(-sigma * length) at
        world-space points [..., 3]."""
        mode = self._alpha_mode(**kw)
        dev = torch.device(self.device)
        pts = xyz_locs.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
        out = torch.empty((pts.shape[0],), device=dev, dtype=torch.float32)
        if pts.shape[0]:
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().ngf_field_alpha(self.handle(), pts.data_ptr(), pts.shape[0], int(mode),
                                                      C.c_float(float(length)), out.data_ptr(),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return out.view(xyz_locs.shape[:-1])

    @torch.no_grad()
    def getDenseAlpha(self, gridSize=None, **kw):
        """FieldBase.py:161-178 (InfoInv: getDenseAlpha(gridSize=None, infoinv=True)): alpha on the [gx,gy,gz] lattice of the
        aabb (one launch instead of gx slices)."""
        gridSize = self.gridSize.tolist() if gridSize is None else [int(g) for g in gridSize]
        dev = torch.device(self.device)
        samples = torch.stack(torch.meshgrid(torch.linspace(0, 1, gridSize[0]), torch.linspace(0, 1, gridSize[1]),
                                             torch.linspace(0, 1, gridSize[2]), indexing='ij'), -1).to(dev)
        aabb = self.aabb.to(dev)
        dense_xyz = aabb[0] * (1 - samples) + aabb[1] * samples
        alpha = self.compute_alpha(dense_xyz.view(-1, 3), float(self.stepSize), **kw).view(gridSize)
        return alpha, dense_xyz

    @torch.no_grad()
    def updateAlphaMask(self, gridSize=(200, 200, 200), **kw):
        """FieldBase.py:180-216 (InfoInv: updateAlphaMask(gridSize, infoinv=True), InfoInv/models/FieldBase.py:180-193, called as
        field.updateAlphaMask(tuple(reso_mask), infoinv=infoinv) by InfoInv/main.py:325) with getDenseAlpha :161-178 inside: dense alpha on the lattice, clamp, 3x3x3 max-pool,
        threshold, new AlphaGridMask, and the aabb of the occupied lattice points -- one C-ABI call
        (ngf_field_alpha_mask_build); only the three torch.linspace vectors are made on the host, like the reference makes
        its lattice, so the points are bit-identical to dense_xyz."""
        mode = self._alpha_mode(**kw)
        gx, gy, gz = (int(g) for g in gridSize)
        dev = torch.device(self.device)
        lin = [torch.linspace(0, 1, g).to(dev) for g in (gx, gy, gz)]
        alpha = torch.empty((gz, gy, gx), device=dev, dtype=torch.float32)
        vol = torch.empty((gz, gy, gx), device=dev, dtype=torch.float32)
        new_aabb = torch.empty((2, 3), device=dev, dtype=torch.float32)
        count = torch.zeros((1,), device=dev, dtype=torch.int64)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().ngf_field_alpha_mask_build(
                self.handle(), int(mode), lin[0].data_ptr(), lin[1].data_ptr(), lin[2].data_ptr(), gx, gy, gz,
                C.c_float(float(self.stepSize)), C.c_float(float(self.alphaMask_thres)), alpha.data_ptr(), vol.data_ptr(),
                new_aabb.data_ptr(), count.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        if int(count.item()) == 0:            # the reference fails here too (amin of an empty tensor); it also prints this total
            raise RuntimeError("updateAlphaMask: no voxel reaches alphaMask_thres")
        self.last_dense_alpha = alpha         # [gz,gy,gx]: alpha.clamp(0,1).transpose(0,2) of the reference, before the pool
        self.alphaMask = AlphaGridMask(self.device, self.aabb, vol)
        self._handle_key = None
        return new_aabb

    def _query_mode(self, **kw) -> int:
        raise NotImplementedError

    @torch.no_grad()
    def query(self, xyz, viewdirs=None, *, use_mask=True, want_coords=False, **kw):
        """Density, colour and gauge-shifted plane coordinates at world-space points ``xyz`` [..., 3] in one launch (ngf_field_query): what the
        reference's module answers with compute_gauge / compute_density / compute_rgb (TriPlane/models/Field.py:53-105).

        ``viewdirs`` is [..., 3] like ``xyz`` or a single 3-vector shared by every point; directions are used as given, not normalised.  ``kw`` is
        ``iteration=0`` for TriPlane (forward's rule, the gauge is applied iff iteration >= gauge_start) and ``infoinv=True`` for InfoInv.
        Returns a dict: ``'sigma'`` [...] (feature2density of the density; 0 outside the aabb and, with an alpha mask and ``use_mask``, where the
        mask is empty), ``'rgb'`` [..., 3] when ``viewdirs`` is given (sigmoid of the decoder's output; no mask, no weight threshold; 0 outside the
        aabb) and ``'coords'`` [..., 6] = (t_xy, t_yz, t_xz) with ``want_coords`` (0 outside the aabb).  Runs under ``torch.no_grad()``: the
        result is NOT differentiable.  GPU only."""
        mode = self._query_mode(**kw)
        dev = torch.device(self.device)
        if dev.type != 'cuda':
            raise RuntimeError("ngf_amd fields answer queries on the GPU only (device='cuda'); there is no CPU path")
        if xyz.shape[-1] != 3:
            raise ValueError(f"xyz must be [..., 3], got {tuple(xyz.shape)}")
        shape = tuple(xyz.shape[:-1])
        pts = xyz.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
        n = pts.shape[0]
        dirs, stride = None, 0
        if viewdirs is not None:
            dirs = torch.as_tensor(viewdirs).to(device=dev, dtype=torch.float32)
            if tuple(dirs.shape) == (3,) and shape != ():
                stride = 0                       # one direction for every point
            elif tuple(dirs.shape) == shape + (3,):
                stride = 3
            else:
                raise ValueError(f"viewdirs must be {shape + (3,)} like xyz or a single 3-vector, got {tuple(dirs.shape)}")
            dirs = dirs.reshape(-1, 3).contiguous()
        out = {'sigma': torch.empty((n,), device=dev, dtype=torch.float32)}
        if dirs is not None:
            out['rgb'] = torch.empty((n, 3), device=dev, dtype=torch.float32)
        if want_coords:
            out['coords'] = torch.empty((n, 6), device=dev, dtype=torch.float32)
        if n:
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().ngf_field_query(
                    self.handle(), pts.data_ptr(), n, int(mode), None if dirs is None else dirs.data_ptr(), stride,
                    0 if use_mask else _lib.QUERY_NO_MASK, out['sigma'].data_ptr(), out['rgb'].data_ptr() if dirs is not None else None,
                    out['coords'].data_ptr() if want_coords else None, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return {k: v.view(shape + tuple(v.shape[1:])) for k, v in out.items()}

    @torch.no_grad()
    def export_mesh(self, path=None, level=0.005, gridSize=None, normals=False, flip=False, colors=None, color_kw=None, **kw):
        """The reference's --export_mesh (TriPlane/main.py:400-401, whose mesh(args) is not defined there): getDenseAlpha(gridSize, **kw) -- InfoInv's
        infoinv= passes through -- then marching cubes at ``level`` on the device (ngf_amd.mesh), with the vertices on the lattice the alpha
        was sampled on, aabb[0] + index * (aabb[1] - aabb[0]) / (n - 1).  Returns (verts, faces[, normals]) as device tensors and writes a binary
        PLY when ``path`` is given.

        ``colors``: None (no colours: the call above), True (every vertex is seen along ``-normal``; the vertex normals are computed whether or
        not they are returned, and a zero normal gives the direction (0, 0, -1)) or one direction ``(dx, dy, dz)`` shared by all vertices.  The
        colours are ``query(verts, dirs, **color_kw)['rgb']`` through ``evalout.to_uint8`` (clamp, times 255, truncate); ``color_kw`` defaults to
        ``kw`` for InfoInv (``infoinv=`` reaches the alpha and the colour alike) and to ``{}`` for TriPlane.  They come back as a uint8 [nv, 3]
        device tensor, the LAST element of the returned tuple, and go into the PLY as ``red green blue`` (with the normals when ``normals``)."""
        from . import mesh
        if torch.device(self.device).type != 'cuda':
            raise RuntimeError("ngf_amd fields export meshes on the GPU only (device='cuda'); there is no CPU path")
        alpha, _ = self.getDenseAlpha(gridSize, **kw)
        lo, hi = np.asarray(self._aabb_host(), dtype=np.float32).reshape(2, 3)
        steps = np.maximum(np.asarray(alpha.shape, dtype=np.float32) - np.float32(1), np.float32(1))
        if colors is None:
            out = mesh.marching_cubes(alpha, level, spacing=(hi - lo) / steps, origin=lo, normals=normals, flip=flip)
            if path is not None:
                mesh.write_ply(path, out[0].cpu().numpy(), out[1].cpu().numpy())
            return out
        from . import evalout
        by_normal = colors is True
        res = mesh.marching_cubes(alpha, level, spacing=(hi - lo) / steps, origin=lo, normals=normals or by_normal, flip=flip)
        verts, faces = res[0], res[1]
        if by_normal:
            zero = (res[2] == 0).all(dim=-1, keepdim=True)
            dirs = torch.where(zero, torch.tensor([0.0, 0.0, -1.0], device=verts.device), -res[2])
        else:
            dirs = torch.tensor([float(c) for c in colors], dtype=torch.float32)
            if tuple(dirs.shape) != (3,):
                raise ValueError("colors must be None, True or one direction (dx, dy, dz)")
        if color_kw is None:
            color_kw = dict(kw) if self.MODEL == _lib.MODEL_INFOINV else {}
        if verts.shape[0]:
            rgb8 = evalout.to_uint8(self.query(verts, dirs, **color_kw)['rgb'])
        else:
            rgb8 = torch.empty((0, 3), device=verts.device, dtype=torch.uint8)
        out = (verts, faces, res[2], rgb8) if normals else (verts, faces, rgb8)
        if path is not None:
            mesh.write_ply(path, verts.cpu().numpy(), faces.cpu().numpy(), normals=res[2].cpu().numpy() if normals else None,
                           colors=rgb8.cpu().numpy())
        return out

    @torch.no_grad()
    def filtering_rays(self, all_rays, all_rgbs, N_samples=256, chunk=10240 * 5, bbox_only=False):
        """FieldBase.py:218-246: drop rays that miss the box (bbox_only) or never touch an occupied voxel."""
        dev = torch.device(self.device)
        shape = all_rgbs.shape[:-1]
        rays = all_rays.reshape(-1, all_rays.shape[-1]).to(device=dev, dtype=torch.float32).contiguous()
        if not bbox_only and self.alphaMask is None:
            raise RuntimeError("filtering_rays(bbox_only=False) needs an alpha mask (updateAlphaMask)")
        flags = torch.empty((rays.shape[0],), device=dev, dtype=torch.uint8)
        if rays.shape[0]:
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().ngf_field_ray_filter(self.handle(), rays.data_ptr(), rays.shape[0], 0 if bbox_only else int(N_samples),
                                                           flags.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        keep = flags.bool()
        keep = keep.view(shape).to(all_rays.device)
        return all_rays[keep], all_rgbs[keep]

    @torch.no_grad()
    def march(self, rays, N_samples, mode=1):
        """Per-sample (sigma, weight) [n,S] -- parity-test hook (sample_ray .. raw2alpha)."""
        dev = torch.device(self.device)
        rays = rays.to(device=dev, dtype=torch.float32).contiguous()
        n, S = rays.shape[0], int(N_samples)
        sigma = torch.empty((n, S), device=dev)
        weight = torch.empty((n, S), device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().ngf_field_march(self.handle(), rays.data_ptr(), n, S, int(mode), None, sigma.data_ptr(),
                                                  weight.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return sigma, weight

    @torch.no_grad()
    def decode_rgb(self, coords, dirs, mode=1):
        """compute_rgb for explicit samples: coords [n,6] = (t_xy, t_yz, t_xz), dirs [n,3] -- parity-test hook."""
        dev = torch.device(self.device)
        coords = coords.to(device=dev, dtype=torch.float32).contiguous()
        dirs = dirs.to(device=dev, dtype=torch.float32).contiguous()
        out = torch.empty((coords.shape[0], 3), device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().ngf_field_decode_rgb(self.handle(), coords.data_ptr(), dirs.data_ptr(), coords.shape[0],
                                                       int(mode), out.data_ptr(),
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return out


class rgb_decoder(torch.nn.Module):
    """Parameter container with the reference's names (networks.py:12-32); evaluated inside the kernel."""

    def __init__(self, feat_dim, view_pe=6, middle_dim=128):
        super().__init__()
        if view_pe != 2 or middle_dim != 64:
            raise ValueError("the gfx950 kernel implements rgb_decoder(view_pe=2, middle_dim=64) (Field.py:28)")
        self.input_dim = feat_dim + 3 + 2 * view_pe * 3
        self.view_pe = view_pe
        self.basis = torch.nn.Linear(feat_dim, feat_dim, bias=False)
        self.mlp = torch.nn.Sequential(torch.nn.Linear(self.input_dim, middle_dim), torch.nn.ReLU(inplace=True),
                                       torch.nn.Linear(middle_dim, middle_dim), torch.nn.ReLU(inplace=True),
                                       torch.nn.Linear(middle_dim, 3))
        torch.nn.init.constant_(self.mlp[-1].bias, 0)


class density_decoder(torch.nn.Module):
    """InfoInv density MLP container (InfoInv/models/networks.py:34-54)."""

    def __init__(self, feat_dim, middle_dim=32):
        super().__init__()
        self.input_dim = feat_dim
        self.mlp = torch.nn.Sequential(torch.nn.Linear(feat_dim, middle_dim), torch.nn.ReLU(inplace=True),
                                       torch.nn.Linear(middle_dim, middle_dim), torch.nn.ReLU(inplace=True),
                                       torch.nn.Linear(middle_dim, 1))
        torch.nn.init.constant_(self.mlp[-1].bias, 0)


def renderer(rays, field, chunk=1024, N_samples=-1, white_bg=True, is_train=False, device='cuda', **field_kw):
    """TriPlane/main.py:60-71 (InfoInv/main.py:61-72).  ``chunk`` existed to bound the reference's
    [chunk, S, C] intermediates; the fused kernel has none, so the whole batch goes down in one launch
    (``chunk`` is accepted and ignored).  Extra keyword arguments (``infoinv=...``) reach the field; ``row_width=W`` tells the launch that ``rays``
    is an H x W image in row-major order (evaluation's ``samples.view(-1, 6)``, main.py:88-94): the same pixels from a screen-space tile order."""
    kw = dict(field_kw)
    if 'infoinv' not in kw and 'iteration' not in kw and field.MODEL == _lib.MODEL_TRIPLANE:
        kw['iteration'] = 30001
    out = field(rays.to(device), is_train=is_train, white_bg=white_bg, N_samples=N_samples, **kw)
    return out['rgb_map'], out['depth_map']
