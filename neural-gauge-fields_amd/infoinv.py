"""``TriPlane`` of the InfoInv tree (InfoInv/models/Field.py:10-89): no gauge, 96-channel planes,
plane features modulated by a sinusoidal encoding of the position, density MLP 72-32-32-1.  With ``field.differentiable = True`` a
training-mode forward under autograd is differentiable (ngf_amd.infoinv_train): the InfoInv tree's own loop (InfoInv/main.py:262-330) runs on it."""
from __future__ import annotations

import torch

from . import _engine, _lib
from .fieldbase import AlphaGridMask, Base, density_decoder, renderer, rgb_decoder  # noqa: F401
from .triplane import _DensityL1


class TriPlane(Base):
    MODEL = _lib.MODEL_INFOINV
    PLANE_C = 96
    DENS_DIM = 24

    def __init__(self, aabb, gridSize, device, **kargs):
        kargs.pop('gauge_start', None)
        super().__init__(aabb, gridSize, device, **kargs)
        # Opt-in switch of the differentiable training-mode forward (not a constructor argument: save() keeps the reference's kwargs).  False
        # keeps the NotImplementedError of a forward that autograd would record.
        self.differentiable = False

    def init_model(self, res=256, dim=96, scale=0.1, device=None, gauge_start=0):
        for name in ('plane_xy', 'plane_yz', 'plane_xz'):
            setattr(self, name, torch.nn.Parameter(scale * torch.randn((1, dim, res, res), device=device)))
        self.density_dim = 24
        self.rgb_dim = dim - self.density_dim
        self.density_decoder = density_decoder(feat_dim=self.density_dim * 3, middle_dim=32).to(device)
        self.rgb_decoder = rgb_decoder(feat_dim=self.rgb_dim * 3, view_pe=2, middle_dim=64).to(device)

    def get_optparam_groups(self, lr_init_spatialxyz=0.02, lr_init_network=0.001):
        return [{'params': self.plane_xy, 'lr': lr_init_spatialxyz}, {'params': self.plane_yz, 'lr': lr_init_spatialxyz},
                {'params': self.plane_xz, 'lr': lr_init_spatialxyz},
                {'params': self.rgb_decoder.parameters(), 'lr': lr_init_network},
                {'params': self.density_decoder.parameters(), 'lr': lr_init_network}]

    def _fill_desc(self, d, dp):
        m = self.density_decoder.mlp
        d.dens_w1, d.dens_b1 = dp(m[0].weight), dp(m[0].bias)
        d.dens_w2, d.dens_b2 = dp(m[2].weight), dp(m[2].bias)
        d.dens_w3, d.dens_b3 = dp(m[4].weight), dp(m[4].bias)

    def _alpha_mode(self, infoinv=True) -> int:
        """compute_alpha / getDenseAlpha / updateAlphaMask(..., infoinv=True) of InfoInv/models/FieldBase.py:140,161,180."""
        return int(bool(infoinv))

    def _query_mode(self, infoinv=True) -> int:
        """Kernel mode of ``query``: the infoinv= switch of compute_density / compute_rgb (InfoInv/models/Field.py:63,83)."""
        return int(bool(infoinv))

    def density_L1(self):
        """InfoInv/models/Field.py:107-110: mean|plane_xy| + mean|plane_yz| + mean|plane_xz|, differentiable.  On the device ngf_planes_l1 /
        ngf_planes_l1_backward (triplane._DensityL1, any plane size); anything else is the reference's torch expression."""
        planes = (self.plane_xy, self.plane_yz, self.plane_xz)
        if all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.data_ptr() % 16 == 0 and p.numel() > 0 for p in planes):
            return _DensityL1.apply(*planes)
        return torch.mean(torch.abs(self.plane_xy)) + torch.mean(torch.abs(self.plane_yz)) + torch.mean(torch.abs(self.plane_xz))

    def _infoinv_grad_engine(self, n, S):
        """The device trainer behind a differentiable forward (ngf_amd.infoinv_train.InfoInvGrad); rebuilt when the batch outgrows it or a
        parameter tensor / the alpha mask / the geometry was replaced."""
        from . import infoinv_train
        return _engine.grad_engine(self, '_ii_engine', infoinv_train.InfoInvGrad, infoinv_train.train_params(self), n, S)

    def release_grad_engine(self):
        """Free the differentiable forward's device buffers (about 3.5 KB per (ray, sample) pair of the largest batch seen, up to ~15 GB at the default
        ``grad_max_pairs``); the next differentiable forward builds the engine again.  A pending backward of an earlier forward re-renders its batch."""
        _engine.release_engine(self, '_ii_engine')

    def _render_train_infoinv(self, rays_chunk, white_bg, N_samples, infoinv, jitter=None, coin=None):
        """``forward(is_train=True)`` with gradients (``_engine.render_train``; the background coin: FieldBase.py:270): one torch.autograd.Function
        over the sixteen parameters per ray chunk of at most ``grad_max_pairs`` (ray, sample) pairs (default 2^22, ~16 GB of per-sample buffers)."""
        from . import infoinv_train
        return _engine.render_train(self, rays_chunk, white_bg, N_samples, infoinv, jitter, coin, infoinv_train.MAX_PAIRS,
                                    self._infoinv_grad_engine, infoinv_train._InfoInvRender)

    def forward(self, rays_chunk, white_bg=True, is_train=False, N_samples=-1, infoinv=True, collect_stats=False, out=None, jitter=None, coin=None, row_width=0):
        """InfoInv/models/FieldBase.py:228.  A call that the reference would record for autograd (is_train=True, grad enabled, parameters
        requiring gradients) returns a differentiable rgb_map when ``self.differentiable`` is set (the InfoInv training loop); without the switch
        it raises instead of returning pixels without a graph -- a loss built on them would otherwise only train its regularisers."""
        if self._wants_grad(is_train):
            if not getattr(self, 'differentiable', False):
                raise NotImplementedError("ngf_amd.infoinv.TriPlane: a training-mode forward under autograd needs the opt-in "
                                          "`field.differentiable = True` (the differentiable InfoInv forward, DESIGN.md section 4.6); or call it "
                                          "under torch.no_grad() for a training-mode render")
            return self._render_train_infoinv(rays_chunk, white_bg, N_samples, infoinv, jitter=jitter, coin=coin)
        return self._render(rays_chunk, white_bg, is_train, N_samples, mode=int(bool(infoinv)), collect_stats=collect_stats, out=out, jitter=jitter, coin=coin, row_width=row_width)
