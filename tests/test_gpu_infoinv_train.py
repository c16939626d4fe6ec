"""GPU: the InfoInv tree's own training loop (InfoInv/main.py:262-330) on the drop-in field with the opt-in ``field.differentiable = True``:
``field(rays_train, is_train=True, infoinv=...)`` is differentiable, ``density_L1`` exists, ``total_loss.backward()`` and ``torch.optim.Adam``
(or ngf_amd.optim.Adam) run unchanged.  Checked against what the reference module itself produced (tests/golden/infoinv_train_*.npz,
make_golden_infoinv_train.py): rgb_map, the gradients of the rgb loss alone and of the total loss, the parameters after two Adam steps.
C ABI: ngf_infoinv_train_forward / ngf_infoinv_train_backward_grad."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import field_for_case  # noqa: E402
import ngf_amd  # noqa: E402,F401
from ngf_amd import infoinv_train, synth  # noqa: E402
from oracle import train as otrain  # noqa: E402

pytestmark = pytest.mark.gpu
GRAD_TOL = 1e-4
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ["infoinv_train_on_white", "infoinv_train_off_black"]


def rel(a, b):
    return float(np.abs(a - b).max()) / max(float(np.abs(b).max()), 1e-30)


def load(name):
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
    plane_hw = tuple(tuple(int(v) for v in hw) for hw in g["plane_hw"])
    params = synth.infoinv_params(int(g["seed"]), plane_hw, preset=str(g["preset"]))
    for k, v in params.items():
        v64 = v.astype(np.float64).reshape(-1)
        chk = np.array([v64.sum(), np.abs(v64).sum(), v64[:: max(1, v64.size // 7)][:7].sum()])
        assert np.array_equal(chk, g["chk." + k]), f"synth regenerated different parameters for {k}"
    g.setdefault("step_ratio", np.float32(0.5))
    mask = (g["mask_bits"], tuple(int(v) for v in g["mask_dhw"]), g["mask_aabb"]) if "mask_bits" in g else None
    return g, params, mask


def make_field(name, differentiable=True):
    g, params, mask = load(name)
    f = field_for_case(g, params, mask)
    f.differentiable = differentiable
    return g, params, f


def _adam(which):
    from ngf_amd import optim
    return {"torch": torch.optim.Adam, "ngf": optim.Adam}[which]


def _forward(f, g, rays, it=0):
    return f(rays, is_train=True, white_bg=bool(int(g["white_bg"])), N_samples=int(g["S"]), infoinv=bool(int(g["infoinv"])),
             jitter=torch.from_numpy(g[f"jitter{it}"]), coin=float(g["coin"]))


@pytest.mark.parametrize("opt", ["torch", "ngf"])
@pytest.mark.parametrize("case", CASES)
def test_the_infoinv_training_loop_runs_unchanged_and_matches_the_reference(case, opt):
    """InfoInv/main.py:262-330 with the opt-in line; only the two random draws of the forward are pinned (jitter=, coin=)."""
    g, params, field = make_field(case)
    nSamples = int(g["S"])
    infoinv = bool(int(g["infoinv"]))
    rays_train, rgb_train = torch.from_numpy(g["rays"]).cuda(), torch.from_numpy(g["rgb_train"]).cuda()
    grad_vars = field.get_optparam_groups(0.02, 1e-3)
    optimizer = _adam(opt)(grad_vars, betas=(0.9, 0.99))
    lr_factor = float(g["lr_factor"])
    L1_reg_weight = 8e-5
    for iteration in range(int(g["steps"])):
        output = field(rays_train, is_train=True, white_bg=bool(int(g["white_bg"])), N_samples=nSamples, infoinv=infoinv,
                       jitter=torch.from_numpy(g[f"jitter{iteration}"]), coin=float(g["coin"]))
        rgb_map = output['rgb_map']
        assert rgb_map.requires_grad and not output['depth_map'].requires_grad
        rgb_loss = torch.mean((rgb_map - rgb_train) ** 2)
        total_loss = rgb_loss
        if iteration == 0:
            np.testing.assert_allclose(rgb_map.detach().cpu().numpy(), g["rgb_map0"], rtol=1e-4, atol=2e-6)
            # the rgb loss alone: on toy planes the L1 term is of the order of the render gradient and would hide a wrong scatter
            optimizer.zero_grad()
            rgb_loss.backward(retain_graph=True)
            sd = dict(field.named_parameters())
            for name in infoinv_train.PARAM_NAMES:
                got = sd[name].grad.cpu().numpy()
                assert rel(got, g[f"grad_rgb0.{name}"]) < GRAD_TOL, ("rgb", name, rel(got, g[f"grad_rgb0.{name}"]))
        if L1_reg_weight > 0:
            loss_reg_L1 = field.density_L1()
            total_loss += L1_reg_weight * loss_reg_L1
        optimizer.zero_grad()
        total_loss.backward()
        if iteration == 0:
            assert abs(float(total_loss.detach()) - float(g["total_loss0"])) < 2e-6
            sd = dict(field.named_parameters())
            for name in infoinv_train.PARAM_NAMES:
                want = g[f"grad0.{name}"] if name.startswith("plane_") else g[f"grad_rgb0.{name}"]
                got = sd[name].grad.cpu().numpy()
                assert rel(got, want) < GRAD_TOL, ("total", name, rel(got, want))
        optimizer.step()
        for param_group in optimizer.param_groups:
            param_group['lr'] = param_group['lr'] * lr_factor
    sd = field.state_dict()
    for name in infoinv_train.PARAM_NAMES:
        d = np.abs(sd[name].cpu().numpy() - g[f"after.{name}"])
        assert not np.array_equal(sd[name].cpu().numpy(), params[name])
        assert np.median(d) < 1e-5 and np.mean(d > 1e-3) < 0.02, (name, float(np.median(d)), float(np.mean(d > 1e-3)))
    # an eval render after the steps sees the updated parameters
    with torch.no_grad():
        out = field(rays_train, N_samples=nSamples, infoinv=infoinv)
        fresh = field_for_case(g, {k: v.cpu().numpy() for k, v in field.state_dict().items()},
                               load(case)[2])(rays_train, N_samples=nSamples, infoinv=infoinv)
    assert torch.isfinite(out["rgb_map"]).all() and not out["rgb_map"].requires_grad
    assert torch.equal(out["rgb_map"], fresh["rgb_map"])


def test_the_default_field_still_raises_and_graphless_calls_build_no_graph():
    g, _, f = make_field(CASES[0], differentiable=False)
    rays = torch.from_numpy(g["rays"]).cuda()
    with pytest.raises(NotImplementedError, match="differentiable"):
        _forward(f, g, rays)
    f.differentiable = True
    with torch.no_grad():
        out = _forward(f, g, rays)
    assert not out["rgb_map"].requires_grad
    out = f(rays, is_train=False, N_samples=int(g["S"]))
    assert not out["rgb_map"].requires_grad
    assert getattr(f, "_ii_engine", None) is None
    assert "differentiable" not in f.state_dict()


def test_frozen_parameters_get_no_grad():
    g, _, f = make_field(CASES[1])
    f.rgb_decoder.basis.weight.requires_grad_(False)
    f.plane_yz.requires_grad_(False)
    out = _forward(f, g, torch.from_numpy(g["rays"]).cuda())
    out["rgb_map"].sum().backward()
    assert f.rgb_decoder.basis.weight.grad is None and f.plane_yz.grad is None
    assert f.plane_xy.grad is not None and f.density_decoder.mlp[0].weight.grad is not None


def test_inplace_write_between_forward_and_backward_is_refused():
    g, _, f = make_field(CASES[0])
    out = _forward(f, g, torch.from_numpy(g["rays"]).cuda())
    with torch.no_grad():
        f.density_decoder.mlp[2].weight.mul_(1.5)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out["rgb_map"].sum().backward()


def test_a_second_forward_before_the_backward_does_not_mix_batches():
    g, _, f = make_field(CASES[0])
    rays = torch.from_numpy(g["rays"]).cuda()
    tgt = torch.from_numpy(g["rgb_train"]).cuda()
    out = _forward(f, g, rays)
    torch.mean((out["rgb_map"] - tgt) ** 2).backward()
    want = [p.grad.clone() for p in infoinv_train.train_params(f)]
    f.zero_grad()
    out = _forward(f, g, rays)
    other = f(rays[:40].flip(0), is_train=True, white_bg=False, N_samples=int(g["S"]), infoinv=False,
              jitter=torch.from_numpy(g["jitter1"][:40]), coin=0.7)          # another batch through the same engine before the first one's backward
    torch.mean((out["rgb_map"] - tgt) ** 2).backward()
    for p, w in zip(infoinv_train.train_params(f), want):
        assert torch.equal(p.grad, w)
    assert other["rgb_map"].requires_grad


def test_two_backwards_of_one_batch_are_bit_identical():
    g, _, f = make_field(CASES[1])
    out = _forward(f, g, torch.from_numpy(g["rays"]).cuda())
    loss = torch.mean((out["rgb_map"] - torch.from_numpy(g["rgb_train"]).cuda()) ** 2)
    loss.backward(retain_graph=True)
    first = [p.grad.clone() for p in infoinv_train.train_params(f)]
    f.zero_grad()
    loss.backward()
    for p, w in zip(infoinv_train.train_params(f), first):
        assert torch.equal(p.grad, w)


def test_density_l1_matches_torch_on_the_device():
    g, _, f = make_field(CASES[0])
    l1 = f.density_L1()
    l1.backward()
    planes = [p.detach().clone().requires_grad_(True) for p in (f.plane_xy, f.plane_yz, f.plane_xz)]
    want = torch.mean(torch.abs(planes[0])) + torch.mean(torch.abs(planes[1])) + torch.mean(torch.abs(planes[2]))
    want.backward()
    assert abs(float(l1.detach()) - float(want.detach())) < 1e-6 * float(want.detach())
    for p, q in zip((f.plane_xy, f.plane_yz, f.plane_xz), planes):
        assert torch.allclose(p.grad, q.grad, rtol=1e-6, atol=0)


def test_large_batches_are_chunked_not_truncated():
    g, _, f = make_field(CASES[1])
    rays = torch.from_numpy(g["rays"]).cuda()
    tgt = torch.from_numpy(g["rgb_train"]).cuda()
    out = _forward(f, g, rays)
    torch.mean((out["rgb_map"] - tgt) ** 2).backward()
    want_rgb, want = out["rgb_map"].detach().clone(), [p.grad.clone() for p in infoinv_train.train_params(f)]
    f.zero_grad()
    f.grad_max_pairs = 50 * int(g["S"])                      # three chunks of <= 50 rays
    out = _forward(f, g, rays)
    torch.mean((out["rgb_map"] - tgt) ** 2).backward()
    assert torch.equal(out["rgb_map"].detach(), want_rgb)
    for name, p, w in zip(infoinv_train.PARAM_NAMES, infoinv_train.train_params(f), want):
        assert rel(p.grad.cpu().numpy(), w.cpu().numpy()) < 1e-5, name


class _EagerInfoInv(otrain.EagerTrainer):
    """oracle/train.EagerTrainer (autograd through the eager port of the reference's operators) on the InfoInv model: the port's InfoInv pieces
    (EagerField._sigma / _rgb with the PE modulation on or off, no gauge in _coords) under the trainer's training-mode forward."""

    def __init__(self, params, g, step, modulate):
        super().__init__(params, g["aabb"], step, g["near_far"], float(g["distance_scale"]), float(g["thr"]))
        self.infoinv_model, self.dd, self.modulate = True, 24, bool(modulate)

    def _sigma(self, c, modulate):
        return super()._sigma(c, self.modulate)

    def _rgb(self, c, dirs, modulate):
        return super()._rgb(c, dirs, self.modulate)


ODD_HW = ((131, 97), (101, 131), (101, 97))          # per axis: x 97, y 131, z 101 -- plane_xy [Ny,Nx], plane_yz [Nz,Ny], plane_xz [Nz,Nx]


@pytest.mark.parametrize("preset,hw,infoinv,white", [("R1", None, True, True), ("R2", None, True, False), ("R1", ODD_HW, False, True)],
                         ids=["R1-256-on-white", "R2-256-on-black", "R1-odd-off-white"])
def test_full_size_batch_matches_autograd_of_the_eager_port(preset, hw, infoinv, white):
    """256^2 planes (and one odd, rectangular per-axis size), 2048 random rays of the 800x800 frame, S = 192: rgb_map and every gradient of the
    rgb loss against autograd of the eager port on the host.  R2 is the dense-active preset (most samples reach the colour MLP)."""
    from ngf_amd import cases
    g, params, step = cases.big_case("infoinv", preset)
    if hw is not None:
        params = synth.infoinv_params(3, hw, preset=preset)
    f = field_for_case(g, params, None)
    f.differentiable = True
    n, S = 2048, 192
    frame = synth.lookat_rays(800, 800)
    pick = (synth.hash_uniform(21, 1, (n,)) * np.float32(frame.shape[0])).astype(np.int64)
    rays_np = frame[pick]
    tgt_np = synth.hash_uniform(21, 2, (n, 3))
    jit_np = synth.hash_uniform(21, 3, (n,))
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    orc = _EagerInfoInv(params, g, step, infoinv)
    rgb_ref, aux = orc.forward_train(torch.from_numpy(rays_np), S, torch.from_numpy(jit_np), white, 0)
    torch.mean((rgb_ref - torch.from_numpy(tgt_np)) ** 2).backward()
    n_active = int(aux["active"].sum())
    assert n_active > 5000, n_active                    # the colour path is exercised

    out = f(torch.from_numpy(rays_np).cuda(), is_train=True, white_bg=white, N_samples=S, infoinv=infoinv, jitter=torch.from_numpy(jit_np),
            coin=0.7)
    np.testing.assert_allclose(out["rgb_map"].detach().cpu().numpy(), rgb_ref.detach().numpy(), rtol=1e-4, atol=2e-6)
    torch.mean((out["rgb_map"] - torch.from_numpy(tgt_np).cuda()) ** 2).backward()
    sd = dict(f.named_parameters())
    # R1 and the odd size: every entry at GRAD_TOL.  R2 (390 k active samples, 25 M colour pre-activations) is ill-conditioned in the forward's
    # rounding: the same eager port run in float64 moves the float32 port's basis gradient by 9e-4 (entry- and norm-wise), its plane gradients by
    # up to 1e-2 entry-wise.  Against the float32 port this kernel's basis gradient is 1.4e-4 off: R2 is held at 1e-3, below that spread.
    tol = 1e-3 if preset == "R2" else GRAD_TOL
    for name in infoinv_train.PARAM_NAMES:
        got, want = sd[name].grad.cpu().numpy(), orc.p[name].grad.numpy()
        l2 = float(np.linalg.norm((got - want).ravel()) / max(np.linalg.norm(want.ravel()), 1e-30))
        assert rel(got, want) < tol and l2 < tol, (name, rel(got, want), l2)


def test_non_finite_upstream_gradients_reach_the_planes_as_nan():
    """A NaN in d loss / d rgb_map must not come out of the fixed-point plane scatter as finite numbers."""
    g, _, f = make_field(CASES[1])
    out = _forward(f, g, torch.from_numpy(g["rays"]).cuda())
    up = torch.ones_like(out["rgb_map"])
    up[:, 1] = float("nan")
    out["rgb_map"].backward(up)
    for p in (f.plane_xy, f.plane_yz, f.plane_xz):
        assert not torch.isfinite(p.grad).all()
