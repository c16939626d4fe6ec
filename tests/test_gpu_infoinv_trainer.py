"""GPU: the fused InfoInv trainer (ngf_amd.infoinv_train.Trainer / fit): one call per iteration of InfoInv/main.py:262-330 with the rgb loss, the
weight gradients on the matrix pipe and Adam inside the library.  Checked against what the reference module itself produced
(tests/golden/infoinv_train_*.npz), against autograd of the eager port at full batch size, and against the drop-in autograd loop on the same
field.  Every tolerance is the one tests/test_gpu_infoinv_train.py applies to the same quantity (imported from there, or restated next to
the line it restates).  Every random draw is pinned (jitter=, coin=)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import field_for_case  # noqa: E402
import ngf_amd  # noqa: E402,F401
from ngf_amd import infoinv_train, synth  # noqa: E402
from test_gpu_infoinv_train import CASES, GRAD_TOL, ODD_HW, _EagerInfoInv, load, make_field, rel  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = infoinv_train.PARAM_NAMES


def _batch(g):
    return torch.from_numpy(g["rays"]).cuda(), torch.from_numpy(g["rgb_train"]).cuda()


def _cfg(g, it=0):
    return dict(N_samples=int(g["S"]), white_bg=bool(int(g["white_bg"])), infoinv=bool(int(g["infoinv"])),
                jitter=torch.from_numpy(g[f"jitter{it}"]), coin=float(g["coin"]))


def _trainer(f, g, **kw):
    return infoinv_train.Trainer(f, batch_size=int(g["rays"].shape[0]), max_samples=int(g["S"]), **kw)


def _close(got, want, tag):
    """The criterion of test_the_infoinv_training_loop_runs_unchanged_and_matches_the_reference for parameters after Adam steps."""
    d = np.abs(got - want)
    print(tag, "median |d|", float(np.median(d)), "share > 1e-3", float(np.mean(d > 1e-3)))
    assert np.median(d) < 1e-5 and np.mean(d > 1e-3) < 0.02, (tag, float(np.median(d)), float(np.mean(d > 1e-3)))


def _state(f):
    return {k: v.detach().cpu().numpy() for k, v in f.state_dict().items()}


@pytest.mark.parametrize("case", CASES)
def test_backward_gives_the_reference_gradients_and_loss(case):
    g, _, f = make_field(case)
    rays, tgt = _batch(g)
    tr = _trainer(f, g)
    loss = tr.backward(rays, tgt, **_cfg(g))
    for name in NAMES:
        got = tr.gradient(name).cpu().numpy()
        print(case, name, "rel", rel(got, g[f"grad_rgb0.{name}"]))
        assert rel(got, g[f"grad_rgb0.{name}"]) < GRAD_TOL, (name, rel(got, g[f"grad_rgb0.{name}"]))
    want = float(np.mean((g["rgb_map0"].astype(np.float64) - g["rgb_train"].astype(np.float64)) ** 2))
    print(case, "loss", float(loss), want)
    assert loss.dtype == torch.float64 and loss.dim() == 0 and abs(float(loss) - want) < 2e-6


@pytest.mark.parametrize("case", CASES)
def test_steps_give_the_reference_parameters_and_the_eval_render_sees_them(case):
    g, params, f = make_field(case)
    rays, tgt = _batch(g)
    tr = _trainer(f, g, lr_init=0.02, lr_basis=1e-3, L1_reg_weight=8e-5)
    tr.lr_factor = float(g["lr_factor"])
    for it in range(int(g["steps"])):
        tr.step(rays, tgt, **_cfg(g, it))
    sd = _state(f)
    for name in NAMES:
        assert not np.array_equal(sd[name], params[name]), name
        _close(sd[name], g[f"after.{name}"], (case, name))
    S, infoinv = int(g["S"]), bool(int(g["infoinv"]))
    with torch.no_grad():
        out = f(rays, N_samples=S, infoinv=infoinv)
        fresh = field_for_case(g, sd, load(case)[2])(rays, N_samples=S, infoinv=infoinv)
    assert torch.isfinite(out["rgb_map"]).all()
    assert torch.equal(out["rgb_map"], fresh["rgb_map"])


@pytest.mark.parametrize("preset,hw,infoinv,white", [("R1", None, True, True), ("R2", None, True, False), ("R1", ODD_HW, False, True)],
                         ids=["R1-256-on-white", "R2-256-on-black", "R1-odd-off-white"])
def test_full_size_batch_matches_autograd_of_the_eager_port(preset, hw, infoinv, white):
    """The comparison of test_gpu_infoinv_train.test_full_size_batch_matches_autograd_of_the_eager_port on the fused path: 2048 rays x 192
    samples, so the products run over several chunks and many fp32 sub-sums.  1e-4 for R1, 1e-3 for R2 (see that test for why)."""
    from ngf_amd import cases
    g, params, step = cases.big_case("infoinv", preset)
    if hw is not None:
        params = synth.infoinv_params(3, hw, preset=preset)
    f = field_for_case(g, params, None)
    n, S = 2048, 192
    frame = synth.lookat_rays(800, 800)
    pick = (synth.hash_uniform(21, 1, (n,)) * np.float32(frame.shape[0])).astype(np.int64)
    rays_np = frame[pick]
    tgt_np = synth.hash_uniform(21, 2, (n, 3))
    jit_np = synth.hash_uniform(21, 3, (n,))
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    orc = _EagerInfoInv(params, g, step, infoinv)
    rgb_ref, aux = orc.forward_train(torch.from_numpy(rays_np), S, torch.from_numpy(jit_np), white, 0)
    loss_ref = torch.mean((rgb_ref - torch.from_numpy(tgt_np)) ** 2)
    loss_ref.backward()
    assert int(aux["active"].sum()) > 5000

    tr = infoinv_train.Trainer(f, batch_size=n, max_samples=S)
    loss = tr.backward(torch.from_numpy(rays_np), torch.from_numpy(tgt_np), N_samples=S, white_bg=white, infoinv=infoinv,
                       jitter=torch.from_numpy(jit_np), coin=0.7)
    assert abs(float(loss) - float(loss_ref.detach())) < 2e-6
    tol = 1e-3 if preset == "R2" else GRAD_TOL
    for name in NAMES:
        got, want = tr.gradient(name).cpu().numpy(), orc.p[name].grad.numpy()
        l2 = float(np.linalg.norm((got - want).ravel()) / max(np.linalg.norm(want.ravel()), 1e-30))
        print(preset, name, "rel", rel(got, want), "l2", l2)
        assert rel(got, want) < tol and l2 < tol, (name, rel(got, want), l2)


def test_one_fused_step_agrees_with_one_iteration_of_the_drop_in_loop():
    case = CASES[0]
    g, _, fa = make_field(case)
    _, _, fb = make_field(case)
    rays, tgt = _batch(g)
    c = _cfg(g)
    _trainer(fa, g).step(rays, tgt, **c)
    opt = torch.optim.Adam(fb.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99))
    out = fb(rays, is_train=True, **c)
    total = torch.mean((out["rgb_map"] - tgt) ** 2) + 8e-5 * fb.density_L1()
    opt.zero_grad()
    total.backward()
    opt.step()
    sa, sb = _state(fa), _state(fb)
    for name in NAMES:
        _close(sa[name], sb[name], name)


def test_two_trainers_from_one_state_are_bit_identical():
    case = CASES[1]
    g, _, fa = make_field(case)
    _, _, fb = make_field(case)
    rays, tgt = _batch(g)
    ta, tb = _trainer(fa, g), _trainer(fb, g)
    for it in range(3):
        c = _cfg(g, it % int(g["steps"]))
        la, lb = ta.step(rays, tgt, keep_loss=True, **c), tb.step(rays, tgt, keep_loss=True, **c)
        assert torch.equal(la, lb)
    for k, name in enumerate(NAMES):
        assert torch.equal(ta.params[k], tb.params[k]), name
        assert torch.equal(ta.exp_avg[k], tb.exp_avg[k]) and torch.equal(ta.exp_avg_sq[k], tb.exp_avg_sq[k]), name
        assert float(ta.exp_avg_sq[k].abs().max()) > 0, name


def test_library_adam_follows_torch_adam_step_for_step_on_an_infoinv_field():
    """The pattern of test_gpu_autograd.test_fused_adam_follows_torch_adam_step_for_step: both optimisers get the same gradient tensors, the
    parameters and the state agree after every step; the differentiable engine's packed planes are never marked stale."""
    from ngf_amd import optim
    case = CASES[0]
    g, _, fa = make_field(case)
    _, _, fb = make_field(case)
    rays, tgt = _batch(g)
    S = int(g["S"])
    oa = torch.optim.Adam(fa.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99))
    ob = optim.Adam(fb.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99))
    for it in range(4):
        jit = torch.from_numpy(synth.hash_uniform(77, it, (rays.shape[0],)))
        for f, o in ((fa, oa), (fb, ob)):
            out = f(rays, is_train=True, white_bg=True, N_samples=S, infoinv=True, jitter=jit)
            total = torch.mean((out["rgb_map"] - tgt) ** 2) + 8e-5 * f.density_L1()
            o.zero_grad()
            total.backward()
            if f is fb:
                for (na, pa), (nb, pb) in zip(fa.named_parameters(), fb.named_parameters()):
                    assert float((pa.grad - pb.grad).abs().max()) <= 2e-3 * max(float(pa.grad.abs().max()), 1e-30), na
                    pb.grad.copy_(pa.grad)
            o.step()
            for gr in o.param_groups:
                gr['lr'] = gr['lr'] * 0.999
        for (na, pa), (nb, pb) in zip(fa.named_parameters(), fb.named_parameters()):
            d = float((pa.detach() - pb.detach()).abs().max())
            assert d <= 1e-6 * max(float(pa.detach().abs().max()), 1e-3) + 1e-8, (it, na, d)
            sa, sb = oa.state[pa], ob.state[pb]
            assert float(sa['step']) == float(sb['step']) == it + 1
            assert float((sa['exp_avg'] - sb['exp_avg']).abs().max()) <= 1e-5 * max(float(sa['exp_avg'].abs().max()), 1e-12), (it, na)
            assert float((sa['exp_avg_sq'] - sb['exp_avg_sq']).abs().max()) <= 1e-5 * max(float(sa['exp_avg_sq'].abs().max()), 1e-20), (it, na)
    # torch's in-place update bumps the version counters: its engine packs before every forward.  The library's wrote the packed copies itself:
    # one pack (the first forward), and the next forward renders the current parameters
    assert fa._ii_engine.repacks == 4 and fb._ii_engine.repacks == 1
    jit = torch.from_numpy(synth.hash_uniform(77, 99, (rays.shape[0],)))
    with torch.no_grad():
        got = fb(rays, is_train=True, white_bg=True, N_samples=S, infoinv=True, jitter=jit)["rgb_map"]
    fresh = field_for_case(g, _state(fb), load(case)[2])
    fresh.differentiable = True
    with torch.no_grad():
        want = fresh(rays, is_train=True, white_bg=True, N_samples=S, infoinv=True, jitter=jit)["rgb_map"]
    assert fb._ii_engine.repacks == 1
    assert torch.equal(got, want)


def test_frozen_parameters_get_no_update_and_their_counters_stay():
    g, params, f = make_field(CASES[0])
    rays, tgt = _batch(g)
    frozen = (1, "rgb_decoder.basis.weight", 8)
    tr = _trainer(f, g, frozen=frozen)
    tr.step(rays, tgt, **_cfg(g))
    tr.step(rays, tgt, **_cfg(g, 1))
    idx = {1, NAMES.index("rgb_decoder.basis.weight"), 8}
    sd = _state(f)
    for k, name in enumerate(NAMES):
        if k in idx:
            assert np.array_equal(sd[name], params[name]) and tr.steps[k] == 0, name
            assert float(tr.exp_avg[k].abs().max()) == 0 and float(tr.exp_avg_sq[k].abs().max()) == 0, name
        else:
            assert not np.array_equal(sd[name], params[name]) and tr.steps[k] == 2, name


def test_state_from_carries_the_moments_and_the_counters():
    case = CASES[1]
    g, _, fa = make_field(case)
    _, _, fb = make_field(case)
    rays, tgt = _batch(g)
    ta = _trainer(fa, g)
    tb = _trainer(fb, g)
    ta.step(rays, tgt, **_cfg(g))
    tb.step(rays, tgt, **_cfg(g))
    tb2 = _trainer(fb, g, state_from=tb)
    assert tb2.steps == tb.steps == [1] * 16 and tb2.lr == tb.lr
    for k in range(16):
        assert torch.equal(tb2.exp_avg[k], tb.exp_avg[k]) and tb2.exp_avg[k].data_ptr() != tb.exp_avg[k].data_ptr()
    ta.step(rays, tgt, **_cfg(g, 1))
    tb2.step(rays, tgt, **_cfg(g, 1))
    for k, name in enumerate(NAMES):
        assert torch.equal(ta.params[k], tb2.params[k]), name
        assert torch.equal(ta.exp_avg[k], tb2.exp_avg[k]) and torch.equal(ta.exp_avg_sq[k], tb2.exp_avg_sq[k]), name


def test_a_batch_above_grad_max_pairs_is_chunked_not_truncated():
    case = CASES[1]
    g, _, fa = make_field(case)
    _, _, fb = make_field(case)
    rays, tgt = _batch(g)
    fb.grad_max_pairs = 50 * int(g["S"])                     # ray chunks of <= 50 rays
    assert rays.shape[0] > 100
    ta, tb = _trainer(fa, g), _trainer(fb, g)
    la = ta.step(rays, tgt, keep_loss=True, **_cfg(g))
    lb = tb.step(rays, tgt, keep_loss=True, **_cfg(g))
    assert fb._ii_engine.max_rays == 50 and fa._ii_engine.max_rays == rays.shape[0]
    assert abs(float(la) - float(lb)) < 1e-12
    sa, sb = _state(fa), _state(fb)
    for name in NAMES:
        _close(sb[name], sa[name], name)


def test_a_non_finite_target_gives_nan_planes_not_wrapped_values():
    g, _, f = make_field(CASES[1])
    rays, tgt = _batch(g)
    tgt = tgt.clone()
    tgt[:, 1] = float("nan")
    tr = _trainer(f, g)
    loss = tr.step(rays, tgt, **_cfg(g))
    assert not np.isfinite(float(loss))
    for p in (f.plane_xy, f.plane_yz, f.plane_xz):
        assert torch.isnan(p).all()


def test_a_reallocated_parameter_asks_for_a_new_trainer_and_an_inplace_write_is_seen():
    g, params, f = make_field(CASES[0])
    rays, tgt = _batch(g)
    tr = _trainer(f, g)
    tr.step(rays, tgt, **_cfg(g))
    with pytest.raises(RuntimeError, match="backward"):
        tr.optimizer_step()                                  # one update per backward
    with torch.no_grad():
        f.plane_xy.mul_(0.5)                                 # an in-place write from outside: seen through the version counter
    before = f._ii_engine.repacks
    tr.backward(rays, tgt, **_cfg(g))
    assert f._ii_engine.repacks == before + 1
    f.plane_yz = torch.nn.Parameter(f.plane_yz.detach().clone())          # a new tensor, as load / up-sampling leave behind
    with pytest.raises(RuntimeError, match="new Trainer"):
        tr.backward(rays, tgt, **_cfg(g))
    tr2 = _trainer(f, g, state_from=tr)
    assert np.isfinite(float(tr2.step(rays, tgt, **_cfg(g))))


def test_fit_runs_end_to_end_on_a_toy_field():
    g, _, f = make_field(CASES[0])
    rays, tgt = torch.from_numpy(g["rays"]), torch.from_numpy(g["rgb_train"])
    allrays, allrgbs = rays.repeat(4, 1), tgt.repeat(4, 1)
    args = types.SimpleNamespace(batch_size=64, n_iters=24, lr_init=0.02, lr_basis=1e-3, lr_decay_iters=-1, lr_decay_target_ratio=0.1,
                                 update_AlphaMask_list=[10], nSamples=int(g["S"]), step_ratio=float(g["step_ratio"]))
    np.random.seed(5)
    torch.manual_seed(5)
    seen = []
    psnr = infoinv_train.fit(f, allrays, allrgbs, args, white_bg=bool(int(g["white_bg"])), infoinv=bool(int(g["infoinv"])),
                             on_iteration=lambda it, loss: seen.append(it))
    assert len(psnr) == 24 and seen == list(range(24)) and all(np.isfinite(p) for p in psnr), psnr
    assert f.alphaMask is not None
    with torch.no_grad():
        out = f(rays.cuda(), N_samples=int(g["S"]), infoinv=bool(int(g["infoinv"])))
    assert torch.isfinite(out["rgb_map"]).all()
