"""GPU checks of NeuTex training through the occupancy grid (``net.occupancy_in_training``; csrc/ngf_uv_train.hpp: the OCC forms of
uvt_rays_kernel and uvt_compact_kernel; include/ngf.h: ngf_uv_trainer_set_occupancy, ngf_uv_train_counts, ngf_uv_train_kept; DESIGN.md
section 4.15).

With the switch on a sample is valid iff it is in the cube and its cell is occupied; every other sample is what an out-of-cube sample is.  The
expected valid mask ``keep`` of a case is the restated look-up (tests/uv_occupancy_ref.py, exact for a given float32 point:
test_gpu_uv_occupancy.py::test_lookup_equals_the_restatement) on the library's OWN float32 ``points_original``, and the same ``keep`` goes to the
fp32 and fp64 torch restatements (tests/uv_train_occ_eager.py), so all three differentiate the same function.  The criteria are those of
tests/test_gpu_uv_train_edges.py, imported from there: per tensor e_hip <= max(4 e_torch32, 1e-5) over three seeds stacked, losses within 1e-5
relative of fp64, the forward within max(2e-5, 4 e_torch32), the trainer within 2e-5 of the eval kernel (which applies the same mask), blend
weights within 1e-4.  Batches: E.edge_batch(seed, prim, S=23, V=...) over E.EDGE_SEEDS, background [[0.2, 0.5, 0.8]]; the masks and what they
keep are listed in tests/uv_train_occ_eager.py and pinned on the CPU by tests/test_uv_train_occupancy_cpu.py.

Caveat of the comparison with the eval render's debug output (test 3): "the eval path evaluated the sample" is read as sigma != 0.  A kept
sample's sigma is softplus(raw) = log1p(exp(raw)), exactly 0 only for raw below about -103; the seeded models' raw densities stay within a few
units of 0 (the test asserts that every kept sample has sigma > 0, so it cannot pass by that accident)."""
import numpy as np
import pytest
import torch

import test_gpu_uv_train_edges as TE
import uv_occupancy_ref as O
import uv_train_eager as E
import uv_train_occ_eager as EO

pytestmark = pytest.mark.gpu
DEV = TE.DEV
S = EO.S
OUTPUTS = ("color", "transmittance", "points", "points_original", "points_inverse_weights", "uv")
PRIMS = ("square", "sphere")


def _args(b, dtype=torch.float32):
    return tuple(TE._t(b[k], dtype) for k in ("campos", "raydir", "U", "template")) + (TE._t(EO.BG1, dtype),)


def _backwards(net, out, b, dtype=torch.float32):
    """A backward per loss set of one forward -> ({tag: loss}, {tag: gradients})."""
    losses, grads = {}, {}
    for tag, w in TE.LOSSES:
        net.zero_grad()
        loss = E.compute_loss(out, TE._t(b["gt_image"], dtype), TE._t(b["gt_trans"], dtype), w)
        loss.backward(retain_graph=True)
        losses[tag], grads[tag] = float(loss.detach()), TE._grads(net)
    return losses, grads


def _hip_forward(net, b):
    cam, rd, U, tp, bg = _args(b)
    net.sample_num = U.shape[-1]
    net.differentiable = True
    return net(cam, rd, bg, jitter_u=U, template_points=tp)


def _detached(out):
    return {k: out[k].detach().clone() for k in OUTPUTS}


def _hip(net, b, backward=True):
    """One differentiable forward of ``net`` as it stands (mask, switch) -> outputs, counts, kept mask, and with ``backward`` the losses and
    gradients of both loss sets."""
    out = _hip_forward(net, b)
    eng = net.grad_engine
    r = {"out": _detached(out), "counts": eng.counts(), "kept": eng.kept_mask().cpu().numpy()}
    if backward:
        r["losses"], r["grads"] = _backwards(net, out, b)
    return r


def _torch(params, prim, b, dtype, keep):
    net = E.make_net(params, prim, S, DEV, dtype)
    cam, rd, U, tp, bg = _args(b, dtype)
    out = EO.forward(net, cam, rd, bg, U, tp, torch.from_numpy(keep).to(DEV))
    losses, grads = _backwards(net, out, b, dtype)
    return _detached(out), losses, grads


def _same(a, b):
    return a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


def _same_grads(ga, gb):
    return all(set(ga[tag]) == set(gb[tag]) and all(torch.equal(ga[tag][k], gb[tag][k]) for k in ga[tag]) for tag, _ in TE.LOSSES)


def _render_layers(grads):
    render = [k for k in grads if not k.startswith("inverse_gauge.")]
    assert len(render) == 58
    return render


def _case(prim, V, vol):
    """The three seeds of a case on HIP (switch on, mask ``vol``), fp32 torch and fp64 torch, in the layout TE._check_* take; every per-case
    assertion of the issue's list is made here."""
    res = []
    for seed in E.EDGE_SEEDS:
        params, b = E.model_params(seed, prim), E.edge_batch(seed, prim, S, V=V)
        net = E.make_net(params, prim, S, DEV)
        net.set_occupancy(vol)
        net.occupancy_in_training = False
        off = _hip(net, b, backward=False)                      # the switch off: what uv must equal, bit for bit
        assert off["counts"] == (V, V)
        net.occupancy_in_training = True
        h = _hip(net, b)
        pos = h["out"]["points_original"].cpu().numpy()
        keep = EO.keep_of(vol, pos)
        assert int(O.in_cube(pos).sum()) == V
        assert h["counts"] == (V, int(keep.sum())), (seed, h["counts"], int(keep.sum()))
        assert np.array_equal(h["kept"], keep), (seed, int((h["kept"] != keep).sum()))
        w = h["out"]["points_inverse_weights"].cpu().numpy()
        assert not w[~keep].any()                              # exactly 0 off keep
        assert _same(h["out"]["uv"], off["out"]["uv"]) and _same(h["out"]["points_original"], off["out"]["points_original"])
        cam, rd, U, _, bg = _args(b)
        with torch.no_grad():
            ev = net(cam, rd, bg, jitter_u=U)                  # the eval kernel, through the same mask
        h["out"].update(eval_color=ev["color"], eval_transmittance=ev["transmittance"])
        net.release_grad_engine()
        net.release()
        r = {"batch": b, "keep": keep, "hip": (h["out"], h["losses"], h["grads"])}
        r["t32"] = _torch(params, prim, b, torch.float32, keep)
        r["t64"] = _torch(params, prim, b, torch.float64, keep)
        res.append(r)
    return res


# ---- 1. gradients and forward against fp64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prim", PRIMS)
@pytest.mark.parametrize("case", EO.CASES, ids=lambda c: c[0])
def test_gradients_and_forward_through_a_mask_against_fp64(case, prim):
    name, V, make = case
    res = _case(prim, V, make())
    kept = [int(r["keep"].sum()) for r in res]
    print(f"uv_train_occupancy {name} {prim}: kept {kept} of {V}")
    assert all(0 < k < V for k in kept)
    TE._check_forward(res, f"occ {name} {prim}")
    TE._check_gradients(res, f"occ {name} {prim}")


# ---- 2. everything masked ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prim", PRIMS)
def test_everything_masked_leaves_the_background_and_no_gradient(prim):
    name, V, make = EO.EMPTY_CASE
    res = _case(prim, V, make())
    tone = torch.pow(TE._t(EO.BG1, torch.float64) + 1e-5, 1 / 2.2).clamp(0, 1)
    for r in res:
        out, grads = r["hip"][0], r["hip"][2]
        assert not r["keep"].any()                             # (_case: counts() == (17, 0), kept_mask() all False)
        assert bool((out["transmittance"] == 1).all()) and bool((out["points_inverse_weights"] == 0).all())
        assert float((out["color"].double() - tone[:, None, :]).abs().max()) < 1e-6
        for tag, _ in TE.LOSSES:
            assert all(bool((grads[tag][k] == 0).all()) and bool((r["t64"][2][tag][k] == 0).all()) for k in _render_layers(grads[tag])), tag
    TE._check_forward(res, f"occ {name} {prim}")
    TE._check_gradients(res, f"occ {name} {prim}")


# ---- 3. agreement with the eval render -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prim", PRIMS)
@pytest.mark.parametrize("case", EO.CASES[:2], ids=lambda c: c[0])
def test_the_trainer_and_the_eval_render_evaluate_the_same_samples(case, prim):
    name, V, make = case
    vol = make()
    for seed in E.EDGE_SEEDS:
        b = E.edge_batch(seed, prim, S, V=V)
        net = E.make_net(E.model_params(seed, prim), prim, S, DEV)
        net.set_occupancy(vol)
        net.occupancy_in_training = True
        h = _hip(net, b, backward=False)
        cam, rd, U, _, bg = _args(b)
        with torch.no_grad():
            ev = net(cam, rd, bg, jitter_u=U, debug=True)
        for k in ("color", "transmittance"):
            d = float((h["out"][k] - ev[k]).abs().max())
            print(f"uv_train_occupancy {name} {prim} seed {seed} {k}: trainer - eval render {d:.2e}")
            assert d < TE.PIX_TOL, (name, seed, k, d)
        sigma = ev["sigma"].cpu().numpy()
        assert (sigma[h["kept"]] > 0).all()                   # the caveat of the module docstring does not apply here
        assert np.array_equal(sigma != 0, h["kept"]), (name, seed, int(((sigma != 0) != h["kept"]).sum()))
        assert 0 < h["counts"][1] < h["counts"][0] == V
        net.release_grad_engine()
        net.release()


# ---- 4. / 5. what changes nothing ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prim", PRIMS)
def test_an_all_ones_mask_and_a_mask_with_the_switch_off_change_nothing(prim):
    seed, V = E.EDGE_SEEDS[0], 2049
    b = E.edge_batch(seed, prim, S, V=V)
    net = E.make_net(E.model_params(seed, prim), prim, S, DEV)
    plain = _hip(net, b)
    assert plain["counts"] == (V, V) and int(plain["kept"].sum()) == V
    runs = {}
    net.occupancy_in_training = True
    net.set_occupancy(np.ones((5, 7, 16), bool))               # the look-up runs and keeps every in-cube sample
    runs["all ones, switch on"] = _hip(net, b)
    assert net.grad_engine.occupancy is net.occupancy
    net.occupancy_in_training = False
    net.set_occupancy(O.checkerboard((8, 8, 8)))               # a mask that would drop half of them, not consulted
    runs["checkerboard, switch off"] = _hip(net, b)
    assert net.grad_engine.occupancy is None
    for name, r in runs.items():
        assert r["counts"] == (V, V) and np.array_equal(r["kept"], plain["kept"]), name
        assert all(_same(r["out"][k], plain["out"][k]) for k in OUTPUTS), name
        assert r["losses"] == plain["losses"] and _same_grads(r["grads"], plain["grads"]), name
        assert len(_render_layers(r["grads"]["l0"])) == 58
    net.release_grad_engine()
    net.release()


# ---- 6. mask lifetime ----------------------------------------------------------------------------------------------------------------------------
def _masked_net(prim="sphere", seed=E.EDGE_SEEDS[0], V=2049, params=None):
    b = E.edge_batch(seed, prim, S, V=V)
    net = E.make_net(E.model_params(seed, prim) if params is None else params, prim, S, DEV)
    net.occupancy_in_training = True
    return net, b


def test_a_mask_set_between_forward_and_backward_does_not_touch_that_backward():
    net, b = _masked_net()
    net.set_occupancy(O.checkerboard((8, 8, 8)))
    ref = _hip(net, b)
    out = _hip_forward(net, b)
    eng = net.grad_engine
    other = net.set_occupancy(O.ball_mask((16, 16, 16), radius=0.7))
    eng.set_occupancy(other)                                   # into the trainer itself: its next forward would use it
    assert eng.occupancy is other
    losses, grads = _backwards(net, out, b)
    assert losses == ref["losses"] and _same_grads(grads, ref["grads"])
    # (d) two backward passes of one masked forward: _backwards ran both loss sets on one graph; once more, the same bits
    again = _backwards(net, out, b)
    assert again[0] == losses and _same_grads(again[1], grads)
    net.release_grad_engine()
    net.release()


def test_a_backward_that_must_render_again_through_another_mask_raises():
    net, b = _masked_net()

    def grads_of(out, **kw):
        net.zero_grad()
        E.compute_loss(out, TE._t(b["gt_image"]), TE._t(b["gt_trans"]), TE.W_DEFAULT).backward(**kw)
        return TE._grads(net)

    net.set_occupancy(O.checkerboard((8, 8, 8)))
    first = _hip_forward(net, b)
    same = _hip_forward(net, b)                                # the first forward's ticket is stale now, the mask is still its own:
    g_first = grads_of(first, retain_graph=True)               # its backward renders the batch again through that mask
    g_same = grads_of(same)
    assert all(torch.equal(g_first[k], g_same[k]) for k in g_first)
    _hip_forward(net, b)
    net.set_occupancy(O.ball_mask((16, 16, 16), radius=0.7))
    second = _hip_forward(net, b)                              # the engine now holds the ball
    with pytest.raises(RuntimeError, match="occupancy mask"):
        grads_of(first)
    g_second = grads_of(second)                                # the second forward is whole
    assert all(bool(torch.isfinite(g).all()) for g in g_second.values()) and not torch.equal(g_second[E.DENSITY_BIAS], g_first[E.DENSITY_BIAS])
    net.release_grad_engine()
    net.release()


def test_build_occupancy_between_iterations_and_an_engine_rebuild_keep_the_mask_current():
    prim, seed = "sphere", E.EDGE_SEEDS[0]
    net, b = _masked_net(prim, seed, params={**E.model_params(seed, prim), **O.smooth_density_params(seed, prim)})
    V = 2049

    def check(tag):
        h = _hip(net, b)
        keep = EO.keep_of(net.occupancy.volume().cpu().numpy(), h["out"]["points_original"].cpu().numpy())
        assert h["counts"] == (V, int(keep.sum())) and np.array_equal(h["kept"], keep), (tag, h["counts"], int(keep.sum()))
        assert net.grad_engine.occupancy is net.occupancy
        print(f"uv_train_occupancy {tag}: kept {h['counts'][1]} of {V}, {net.occupancy.fraction():.3f} of the cells occupied")
        return h

    sigma = net.density_lattice((9, 10, 11), clip=False)[0]
    first = net.build_occupancy((8, 9, 10), threshold=float(sigma.median()), dilate=1)
    one = check("first mask")
    assert 0 < one["counts"][1] < V
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    opt.step()                                                 # an iteration: the parameters move, the mask does not
    assert net.occupancy is first
    # (c) a new mask between two iterations, from the density as it is now: the next forward trains through it
    sigma = net.density_lattice((9, 10, 11), clip=False)[0]
    second = net.build_occupancy((8, 9, 10), threshold=float(sigma.quantile(0.75)), dilate=0)
    assert second is not first
    two = check("second mask")
    assert 0 < two["counts"][1] < one["counts"][1]
    # (e) a released engine: the next forward builds a new one, which gets the mask again
    net.release_grad_engine()
    assert net.grad_engine is None
    three = check("after release_grad_engine")
    assert three["counts"] == two["counts"] and np.array_equal(three["kept"], two["kept"])
    # an engine grown for a larger batch as well
    eng = net.grad_engine
    big = E.edge_batch(seed, prim, S, R=eng.max_rays + 5)
    _hip(net, big, backward=False)
    assert net.grad_engine is not eng and net.grad_engine.occupancy is second
    four = check("after the engine grew")
    assert four["counts"] == two["counts"] and np.array_equal(four["kept"], two["kept"])
    net.release_grad_engine()
    net.release()


# ---- 7. refusals on a live trainer ---------------------------------------------------------------------------------------------------------------
def test_a_live_trainer_refuses_a_bad_axis_and_counts_before_a_forward():
    import ctypes as C
    net, b = _masked_net(V=17)
    eng = net._uv_grad_engine(b["raydir"].shape[1], S)         # a fresh engine: no forward yet
    L, st = eng.L, C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    with pytest.raises(RuntimeError, match="no forward"):
        eng.counts()
    with pytest.raises(RuntimeError, match="no forward"):
        eng.kept_mask()
    out = torch.zeros(8, dtype=torch.uint8, device=DEV)
    assert L.ngf_uv_train_kept(eng._h, out.data_ptr(), st) == 1 and b"no forward" in L.ngf_last_error()
    bits = torch.full((1 << 14,), 0xFF, dtype=torch.uint8, device=DEV)
    for bad in ((0, 4, 4), (4, 1025, 4), (4, 4, -1)):
        assert L.ngf_uv_trainer_set_occupancy(eng._h, bits.data_ptr(), *bad, st) == 1 and b"every axis" in L.ngf_last_error(), bad
    assert L.ngf_uv_trainer_set_occupancy(eng._h, None, 0, 0, 0, st) == 0          # NULL switches the mask off whatever the axes say
    out2 = (C.c_int64 * 2)()
    assert L.ngf_uv_train_counts(eng._h, None, st) == 1 and L.ngf_uv_train_counts(eng._h, out2, st) == 1
    # the refusals left the trainer whole and without a mask: a forward keeps every in-cube sample
    net.occupancy_in_training = False
    h = _hip(net, b, backward=False)
    assert net.grad_engine is eng and h["counts"] == (17, 17) and not out.any()
    net.release_grad_engine()
    net.release()
