"""GPU checks of InfoInv training at the batch edges that tests/test_gpu_infoinv_train.py and tests/test_gpu_infoinv_trainer.py never reach, on
the toy planes of their fixtures (12 x 10 x 9 grid): an exact active count of 0, 1, 31, 32, 33 and 1025 (the k-step and the fp32-to-fp64
hand-over of the colour products), a batch without one valid sample, one ray, ragged 256-thread ray blocks, two and three rays per
ii_prefix_kernel thread, a short last chunk of both product kernels in a real batch, an alpha mask with the PE modulation off on white and on on
black, softplus arguments on both sides of ATen's threshold of 20, the fused step cut into ray chunks, a small batch after a large one on the same
engine, and one Adam step on planes of 63, 64, 65 and 130 texels per row.

Both HIP paths run on every case: the autograd path (``field.differentiable = True``) and ``Trainer.backward`` + ``Trainer.gradient`` of the
fused path, against tests/infoinv_train_eager.py in fp64 (the truth) and fp32 (the yardstick), under the criterion of
tests/test_gpu_uv_train_edges.py: three seeds (model and batch); the loss within 1e-5 relative of fp64; per tensor, over the three gradients
stacked, e_hip <= max(4 e_torch32, 1e-5); where the fp64 gradient of a tensor is exactly zero on all three seeds the HIP gradient must be
exactly zero too; rgb_map within max(2e-6, 4 e_torch32) of fp64.  Batches come from E.edge_batch: rays picked by their fp64 counts, every
sample 1e-5 away from the box faces and every weight 2 % away from the threshold, so fp32 and fp64 agree on the valid and the active set;
every case asserts both counts against the engine (ngf_debug_ii_counts)."""
import numpy as np
import pytest
import torch

import infoinv_train_eager as E
from ngf_amd import infoinv_train, synth
from ngf_amd.cases import field_for_case
from oracle import train as otrain

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = infoinv_train.PARAM_NAMES
EDGE = E.edge_cases()
PIX_TOL = 2e-6
HIP = ("auto", "fused")
L1 = 8e-5


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.asarray(a)).to(DEV, dtype)


def _field(params, g=None, masked=False):
    g0, _, mask = E.toy()
    f = field_for_case(g or g0, params, mask if masked else None, device=DEV)
    f.differentiable = True
    return f


def _auto(f, b, white, counts=True):
    """the autograd path -> (rgb_map, loss, gradients, (valid, active) of the engine)"""
    f.zero_grad()
    out = f(_t(b["rays"]), is_train=True, white_bg=white, N_samples=b["S"], infoinv=b["infoinv"], jitter=_t(b["jitter"]), coin=0.7)
    loss = torch.mean((out["rgb_map"] - _t(b["rgb_train"])) ** 2)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in f.named_parameters()}
    assert set(grads) == set(NAMES)
    return out["rgb_map"].detach().clone(), float(loss.detach().double()), grads, f._ii_engine.counts() if counts else None


def _fused(f, b, white, counts=True, trainer=None):
    """Trainer.backward + Trainer.gradient -> (None, loss, gradients, (valid, active) of the engine)"""
    tr = trainer or infoinv_train.Trainer(f, batch_size=len(b["rays"]), max_samples=b["S"])
    loss = tr.backward(_t(b["rays"]), _t(b["rgb_train"]), N_samples=b["S"], white_bg=white, infoinv=b["infoinv"], jitter=_t(b["jitter"]), coin=0.7,
                       keep_loss=True)
    grads = {k: tr.gradient(k).clone() for k in NAMES}
    return None, float(loss), grads, f._ii_engine.counts() if counts else None


def _eager(b, white, dtype, g=None):
    g0, _, mask = E.toy()
    e = E.Eager(b["params"], g or g0, dtype, DEV, mask if b["masked"] else None)
    rgb, loss, grads, aux = e.gradients(_t(b["rays"], dtype), _t(b["rgb_train"], dtype), b["S"], _t(b["jitter"], dtype), white, b["infoinv"])
    return rgb, loss, grads, (int(aux["valid"].sum()), int(aux["active"].sum()))


def _three(make, white, g=None, hip=None):
    """make(seed) -> batch; the three seeds on both HIP paths, fp32 torch and fp64 torch -> [{run: (rgb_map, loss, gradients, counts)}]"""
    res = []
    for seed in E.EDGE_SEEDS:
        b = make(seed)
        f = _field(b["params"], g, b["masked"])
        r = {"batch": b, "auto": _auto(f, b, white)}
        r["fused"] = _fused(f, b, white)
        for name, fn in (hip or {}).items():
            r[name] = fn(b, white)
        f.release_grad_engine()
        r["t32"], r["t64"] = _eager(b, white, torch.float32, g), _eager(b, white, torch.float64, g)
        want = (int(b["valid"].sum()), int(b["active"].sum()))
        for k in ("auto", "fused", "t32", "t64"):
            assert r[k][3] == want, (seed, k, r[k][3], want)
        res.append(r)
    return res


def _stack_err(res, name, k):
    num = sum(float(torch.linalg.norm(r[name][2][k].double() - r["t64"][2][k])) ** 2 for r in res)
    den = sum(float(torch.linalg.norm(r["t64"][2][k])) ** 2 for r in res)
    return (num / den) ** 0.5 if den > 0 else None


def _group(k):
    return "planes" if k.startswith("plane_") else k.split(".")[0]


def _check(res, label, paths=HIP):
    """the criterion over the three seeds stacked, on every HIP path; prints e_hip / e_torch32 per path and tensor group"""
    bad = {}
    for r in res:
        l64 = r["t64"][1]
        for p in paths:
            assert abs(r[p][1] - l64) <= 1e-5 * max(1.0, abs(l64)), (label, p, r[p][1], l64)
        e_t = float((r["t32"][0].double() - r["t64"][0]).abs().max())
        e_h = float((r["auto"][0].double() - r["t64"][0]).abs().max())
        print(f"ii_edges {label} rgb_map: hip {e_h:.2e} fp32 torch {e_t:.2e} of fp64")
        assert e_h <= max(PIX_TOL, 4 * e_t), (label, "rgb_map", e_h, e_t)
    for p in paths:
        worst = {}
        for k in NAMES:
            gh = [r[p][2][k] for r in res]
            assert all(bool(torch.isfinite(g).all()) for g in gh), (label, p, k)
            e_h, e_t = _stack_err(res, p, k), _stack_err(res, "t32", k)
            if e_h is None:          # the fp64 gradient is exactly zero on every seed
                assert all(bool((g == 0).all()) for g in gh), (label, p, k, "fp64 is exactly zero, HIP is not")
                continue
            if not e_h <= max(4 * e_t, 1e-5):
                bad[(p, k)] = (e_h, e_t)
            grp = _group(k)
            if grp not in worst or e_h / max(e_t, 1e-30) > worst[grp][0] / max(worst[grp][1], 1e-30):
                worst[grp] = (e_h, e_t, k)
        for grp, (e_h, e_t, k) in sorted(worst.items()):
            print(f"ii_edges {label} {p} {grp}: e_hip {e_h:.3e} e_torch32 {e_t:.3e} ({k})")
    assert not bad, (label, bad)


def _case(name):
    kw, white = EDGE[name]
    return _three(lambda seed: E.edge_batch(seed, **kw), white), white


@pytest.mark.parametrize("bg", ["white", "black"])
def test_no_active_sample(bg):
    res, white = _case(f"active0-{bg}")
    _check(res, f"active0-{bg}")
    for r in res:
        assert r["auto"][3][1] == 0 and r["auto"][3][0] > len(r["batch"]["rays"])
        for p in HIP:
            assert all(bool((r[p][2][k] == 0).all()) for k in E.COLOUR), p          # no row reaches the colour products
            dens = [bool((r[p][2][k] != 0).any()) for k in E.DENSITY]
            # black: nothing reaches the pixels.  white: 1 - sum of the weights does, through the density alone
            assert (all(dens) if white else not any(dens)), (p, bg, dens)
        assert all(bool((r["t64"][2][k] == 0).all()) for k in E.COLOUR)
        if not white:
            assert bool((r["auto"][0] == 0).all())


@pytest.mark.parametrize("bg", ["white", "black"])
def test_no_valid_sample_at_all(bg):
    res, white = _case(f"novalid-{bg}")
    _check(res, f"novalid-{bg}")
    for r in res:
        assert r["auto"][3] == (0, 0)
        assert bool((r["auto"][0] == (1.0 if white else 0.0)).all())          # the background
        for p in HIP:
            assert all(bool((r[p][2][k] == 0).all()) for k in NAMES), p
    # a following optimizer_step: finite parameters that moved by the L1 term only
    b = res[0]["batch"]
    f = _field(b["params"])
    tr = infoinv_train.Trainer(f, batch_size=len(b["rays"]), max_samples=b["S"], L1_reg_weight=L1)
    before = [p.detach().clone() for p in tr.params]
    lrs = list(tr.lr)
    _fused(f, b, white, trainer=tr)
    tr.optimizer_step()
    for k, name in enumerate(NAMES):
        now = tr.params[k].detach()
        assert bool(torch.isfinite(now).all()), name
        if k >= 3:
            assert torch.equal(now, before[k]), name          # a zero gradient: m = v = 0 and a step of 0 / (0 + eps)
            continue
        gk = L1 * torch.sign(before[k]) / before[k].numel()
        want, m, v = otrain.adam_update(before[k], gk, torch.zeros_like(gk), torch.zeros_like(gk), 1, lrs[k])
        err = float((now - want).abs().max())
        assert err < 2e-6 * max(1.0, float(before[k].abs().max())) + 1e-3 * lrs[k], (name, err)
        assert not torch.equal(now, before[k]), name
    f.release_grad_engine()


@pytest.mark.parametrize("active", E.EDGE_ACTIVE)
def test_an_exact_active_count_at_the_edges_of_the_colour_products(active):
    res, _ = _case(f"active{active}")
    for r in res:
        assert r["auto"][3][1] == active and r["fused"][3][1] == active
    _check(res, f"active{active}")


@pytest.mark.parametrize("R,S", E.EDGE_RAYS, ids=[f"{R}x{S}" for R, S in E.EDGE_RAYS])
def test_ray_and_sample_counts_at_the_edges_of_the_ray_kernels_and_the_chunks(R, S):
    res, _ = _case(f"rays{R}x{S}")
    assert res[0]["auto"][0].shape == (R, 3)
    _check(res, f"rays{R}x{S}")


@pytest.mark.parametrize("case", ["mask-off-white", "mask-on-black"])
def test_an_alpha_mask_with_the_other_switches(case):
    res, _ = _case(case)
    _check(res, case)


def test_softplus_arguments_on_both_sides_of_the_threshold():
    made = {seed: E.softplus_case(seed) for seed in E.EDGE_SEEDS}
    for seed, (_, _, _, s) in made.items():
        print(f"ii_edges softplus seed {seed}: {s}")
        assert 0.1 <= s["above"] <= 0.9 and s["gap"] > 1e-4, (seed, s)
    g = made[E.EDGE_SEEDS[0]][1]
    res = _three(lambda seed: made[seed][2], True, g=g)
    _check(res, "softplus")


def test_the_fused_step_in_ray_chunks_gradient_by_gradient():
    kw, white = EDGE["chunks"]
    per = 50          # 128 rays: chunks of 50, 50 and 28

    def chunked(b, wh):
        f = _field(b["params"])
        f.grad_max_pairs = per * b["S"]
        out = _fused(f, b, wh, counts=False)
        assert f._ii_engine.max_rays == per and len(b["rays"]) == 128
        f.release_grad_engine()
        return out

    res = _three(lambda seed: E.edge_batch(seed, **kw), white, hip={"chunked": chunked})
    _check(res, "chunks", paths=("auto", "fused", "chunked"))
    for r in res:
        assert abs(r["chunked"][1] - r["fused"][1]) < 1e-12
        for k in NAMES:          # the bound of test_large_batches_are_chunked_not_truncated, on every gradient
            a, c = r["fused"][2][k], r["chunked"][2][k]
            d = float((a - c).abs().max()) / max(float(a.abs().max()), 1e-30)
            assert d < 1e-5, (k, d)


@pytest.mark.parametrize("path", HIP)
def test_a_small_batch_after_the_largest_one_reads_none_of_its_rows(path):
    seed = E.EDGE_SEEDS[0]
    big = E.edge_batch(seed, E.EDGE_S, R=2051)
    small = E.edge_batch(seed, 7, active=33)
    run = _auto if path == "auto" else _fused
    f = _field(small["params"])
    fresh = run(f, small, True)
    f.release_grad_engine()
    assert getattr(f, "_ii_engine", None) is None
    f = _field(small["params"])
    run(f, big, True)
    after = [run(f, small, True)]
    eng = f._ii_engine
    assert (eng.max_rays, eng.max_samples) == (2051, E.EDGE_S)
    # once more, now that the engine no longer grows: the large batch's rows are in the very buffers the small one uses
    run(f, big, True)
    after.append(run(f, small, True))
    assert f._ii_engine is eng
    f.release_grad_engine()
    for got in after:
        assert got[3] == fresh[3] == (int(small["valid"].sum()), 33)
        assert got[1] == fresh[1]
        if path == "auto":
            assert torch.equal(got[0], fresh[0])
        assert all(torch.equal(got[2][k], fresh[2][k]) for k in NAMES), [k for k in NAMES if not torch.equal(got[2][k], fresh[2][k])]


# (Nx, Ny, Nz): plane_xy [Ny, Nx], plane_yz [Nz, Ny], plane_xz [Nz, Nx] -- rows of 63, 64, 65 and 130 texels, heights 2, 3 and 70 among them
ADAM_GRIDS = ((63, 64, 2), (65, 130, 70), (64, 65, 3))


def _adam_case(grid):
    g0, _, _ = E.toy()
    g = dict(g0, grid=np.asarray(grid, np.int64))
    nx, ny, nz = grid
    hw = ((ny, nx), (nz, ny), (nz, nx))
    fx = dict(np.load(E.GOLDEN + "/infoinv_train_off_black.npz", allow_pickle=False))
    b = {"rays": fx["rays"], "jitter": fx["jitter0"], "rgb_train": fx["rgb_train"], "S": E.EDGE_S, "infoinv": True, "masked": False,
         "params": synth.infoinv_params(500 + nx, hw, preset="R1")}
    return g, hw, b


def _check_adam(name, now, m, v, before, gk, lr):
    want, wm, wv = otrain.adam_update(before, gk, torch.zeros_like(gk), torch.zeros_like(gk), 1, lr)
    err = float((now - want).abs().max())
    assert err < 2e-6 * max(1.0, float(before.abs().max())) + 1e-3 * lr, (name, err)
    assert torch.allclose(m, wm, rtol=1e-5, atol=1e-12) and torch.allclose(v, wv, rtol=1e-5, atol=1e-20), name
    assert not torch.equal(now, before), name


def _next_forward_is_that_of_a_fresh_engine(f, g, b):
    """a differentiable forward through the engine whose packed planes the Adam pass wrote (no re-pack), against a field built from the state"""
    eng, packs = f._ii_engine, f._ii_engine.repacks
    got = _auto(f, b, True, counts=False)
    assert f._ii_engine is eng and eng.repacks == packs
    fresh_f = _field({k: v.detach().cpu().numpy() for k, v in f.state_dict().items()}, g)
    want = _auto(fresh_f, b, True, counts=False)
    assert torch.equal(got[0], want[0]) and got[1] == want[1]
    assert all(torch.equal(got[2][k], want[2][k]) for k in NAMES)
    fresh_f.release_grad_engine()


@pytest.mark.parametrize("grid", ADAM_GRIDS, ids=["x".join(str(v) for v in gr) for gr in ADAM_GRIDS])
def test_one_fused_adam_step_on_odd_plane_widths_element_by_element(grid):
    g, hw, b = _adam_case(grid)
    f = _field(b["params"], g)
    assert [tuple(p.shape[2:]) for p in (f.plane_xy, f.plane_yz, f.plane_xz)] == list(hw)
    tr = infoinv_train.Trainer(f, batch_size=len(b["rays"]), max_samples=b["S"], L1_reg_weight=L1)
    before = [p.detach().clone() for p in tr.params]
    lrs = list(tr.lr)
    _, _, grads, cnt = _fused(f, b, True, trainer=tr)
    assert cnt[1] > 0
    tr.optimizer_step()
    for k, name in enumerate(NAMES):
        gk = grads[name]
        assert bool((gk != 0).any()), name
        if k < 3:
            gk = gk + L1 * torch.sign(before[k]) / before[k].numel()
        _check_adam(name, tr.params[k].detach(), tr.exp_avg[k], tr.exp_avg_sq[k], before[k], gk, lrs[k])
    _next_forward_is_that_of_a_fresh_engine(f, g, b)
    f.release_grad_engine()


@pytest.mark.parametrize("grid", ADAM_GRIDS, ids=["x".join(str(v) for v in gr) for gr in ADAM_GRIDS])
def test_one_library_adam_step_through_the_optimizer_on_odd_plane_widths(grid):
    from ngf_amd import optim
    g, hw, b = _adam_case(grid)
    f = _field(b["params"], g)
    opt = optim.Adam(f.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99))
    out = f(_t(b["rays"]), is_train=True, white_bg=True, N_samples=b["S"], infoinv=True, jitter=_t(b["jitter"]), coin=0.7)
    total = torch.mean((out["rgb_map"] - _t(b["rgb_train"])) ** 2) + L1 * f.density_L1()
    opt.zero_grad()
    total.backward()
    params = dict(f.named_parameters())
    before = {k: p.detach().clone() for k, p in params.items()}
    grads = {k: p.grad.detach().clone() for k, p in params.items()}
    opt.step()
    assert f._ii_engine.repacks == 1
    for k, name in enumerate(NAMES):
        st = opt.state[params[name]]
        assert float(st["step"]) == 1
        _check_adam(name, params[name].detach(), st["exp_avg"], st["exp_avg_sq"], before[name], grads[name], 0.02 if k < 3 else 1e-3)
    _next_forward_is_that_of_a_fresh_engine(f, g, b)
    f.release_grad_engine()
