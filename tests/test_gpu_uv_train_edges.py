"""GPU checks of UV-Mapping (NeuTex) training at the batch edges that tests/test_gpu_uv_train.py never reaches: an exact in-cube count V at the
1024-row split-K chunk edges (and 0 and 1), ray counts that make uvt_scan_kernel take one, two and three rays per thread and leave the
256-thread ray kernels a ragged last block, three cameras with three backgrounds in the backward, a small batch after a large one on the same
engine, and softplus arguments on both sides of torch's threshold of 20.

``net.differentiable = True`` against tests/uv_train_eager.py in fp64 (the truth) and fp32 (the yardstick), under the criterion of
tests/test_gpu_uv_train.py: the loss within 1e-5 relative of fp64, per tensor e_hip <= max(4 e_torch32, 1e-5), the forward as in
test_forward_matches_eval_kernel_and_restatement_two_cameras_short_rays (but for the finding below).  One change: every case runs on three seeds
(model and batch) and a tensor's e is taken over the three gradients stacked -- a dozen in-cube samples give fp32 torch a lucky or unlucky draw,
and a ratio of two such draws is no test.  Where the fp64 gradient of a tensor is exactly zero on all three, the HIP gradient must be exactly
zero too.  Both loss sets run on every case (two backwards of one forward).  Batches come from E.edge_batch: rays picked by their fp64 in-cube
counts, every sample at least 1e-5 away from the cube's faces, so fp32 and fp64 agree on which samples count; every case asserts the count of the
returned points_original.

Finding (measured on an MI355X).  |trainer - eval kernel| < 2e-5 on colour and transmittance holds in every case at
S = 23 and S = 24 (largest 1.56e-5), at one ray, at 257 rays on the square and at three cameras on the square (1.91e-5).  At S = 5 it does not
hold in the EVAL_FINDING cases: 2.17e-4 against 2e-5 at 1025 and 2051 rays on the sphere (square: 2.77e-5), 7.80e-5 at 257 rays on the sphere,
1.37e-4 at three cameras on the sphere.  A segment is 0.4 long there and fp32 torch itself is 6.1e-3 (three cameras: 2.1e-2) off fp64 on the same
pixels; the slope of the tone map at a dark pixel, d/dx (x + 1e-5)^(1/2.2), is about 240.  Both kernels are fp32 and neither is the truth, so in
those cases alone the eval kernel is held to what fp32 torch does, max(2e-5, 4 e_torch32) of fp64, as the trainer is in every case.

points_original."""
import numpy as np
import pytest
import torch

import uv_train_eager as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PIX_TOL = 2e-5
W_DEFAULT, W_INV = (1.0, 1.0, 1.0, 0.0), (1.0, 1.0, 1.0, 1.0)
LOSSES = (("l0", W_DEFAULT), ("l1", W_INV))
BG1 = np.array([[0.2, 0.5, 0.8]], np.float32)
BG3 = np.array([[0.2, 0.5, 0.8], [0.9, 0.1, 0.3], [0.05, 0.7, 0.45]], np.float32)
# the cases of the finding in the module docstring: the trainer's forward and the eval kernel are more than PIX_TOL apart
EVAL_FINDING = {(257, "sphere"), (1025, "square"), (1025, "sphere"), (2051, "square"), (2051, "sphere"), ("cams", "sphere")}
RUNS = (("hip", torch.float32, True), ("t32", torch.float32, False), ("t64", torch.float64, False))


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.asarray(a)).to(DEV, dtype)


def _grads(net):
    return {k: p.grad.detach().double().clone() for k, p in net.named_parameters()}


def _in_cube(pos):
    return int(((pos > -1.0) & (pos < 1.0)).all(-1).sum())


def _one(net, b, S, dtype, hip, bg, keep_engine=False):
    """One forward and a backward per loss set -> (outputs, {tag: loss}, {tag: gradients})."""
    net.sample_num = S
    net.differentiable = hip
    cam, rd, U, tp = (_t(b[k], dtype) for k in ("campos", "raydir", "U", "template"))
    bgt = None if bg is None else _t(bg, dtype)
    out = net(cam, rd, bgt, jitter_u=U, template_points=tp) if hip else E.forward(net, cam, rd, bgt, U, tp)
    losses, grads = {}, {}
    for tag, w in LOSSES:
        net.zero_grad()
        loss = E.compute_loss(out, _t(b["gt_image"], dtype), _t(b["gt_trans"], dtype), w)
        loss.backward(retain_graph=True)
        losses[tag], grads[tag] = float(loss.detach()), _grads(net)
    keep = {k: out[k].detach() for k in ("color", "transmittance", "points", "points_original", "points_inverse_weights", "uv")}
    if hip:
        with torch.no_grad():
            ev = net(cam, rd, bgt, jitter_u=U)          # the eval kernel on the same batch
        keep.update(eval_color=ev["color"], eval_transmittance=ev["transmittance"])
        if not keep_engine:
            net.release_grad_engine()
    return keep, losses, grads


def _three(prim, S, make, bg):
    """make(seed) -> (params, batch); runs the three seeds on HIP, fp32 torch and fp64 torch."""
    res = []
    for seed in E.EDGE_SEEDS:
        params, b = make(seed)
        r = {"batch": b}
        for name, dtype, hip in RUNS:
            r[name] = _one(E.make_net(params, prim, S, DEV, dtype), b, S, dtype, hip, bg)
        if "counts" in b:
            assert _in_cube(r["hip"][0]["points_original"]) == int(b["counts"].sum())
        res.append(r)
    return res


def _stack_err(res, name, tag, k):
    num = sum(float(torch.linalg.norm(r[name][2][tag][k] - r["t64"][2][tag][k])) ** 2 for r in res)
    den = sum(float(torch.linalg.norm(r["t64"][2][tag][k])) ** 2 for r in res)
    return (num / den) ** 0.5 if den > 0 else None


def _check_gradients(res, label):
    """The criterion over the three seeds stacked; prints e_hip / e_torch32 per tensor group -> the worst ratio of the case."""
    bad, worst = {}, {}
    for r in res:
        for tag, _ in LOSSES:
            l64 = r["t64"][1][tag]
            assert abs(r["hip"][1][tag] - l64) <= 1e-5 * max(1.0, abs(l64)), (label, tag, r["hip"][1][tag], l64)
    for tag, _ in LOSSES:
        for k in res[0]["t64"][2][tag]:
            gh = [r["hip"][2][tag][k] for r in res]
            assert all(bool(torch.isfinite(g).all()) for g in gh), (label, tag, k)
            e_h, e_t = _stack_err(res, "hip", tag, k), _stack_err(res, "t32", tag, k)
            if e_h is None:          # the fp64 gradient is exactly zero on every seed
                assert all(bool((g == 0).all()) for g in gh), (label, tag, k, "fp64 is exactly zero, HIP is not")
                continue
            if not e_h <= max(4 * e_t, 1e-5):
                bad[(tag, k)] = (e_h, e_t)
            grp = k.split(".")[0]
            if grp not in worst or e_h / max(e_t, 1e-30) > worst[grp][0] / max(worst[grp][1], 1e-30):
                worst[grp] = (e_h, e_t, tag, k)
    for grp, (e_h, e_t, tag, k) in sorted(worst.items()):
        print(f"uv_edges {label} {grp}: e_hip {e_h:.3e} e_torch32 {e_t:.3e} ({tag} {k})")
    assert not bad, (label, bad)


def _check_forward(res, label, eval_finding=False):
    """The forward tolerances of test_forward_matches_eval_kernel_and_restatement_two_cameras_short_rays: the trainer against the eval kernel
    (2e-5) and against fp32 and fp64 torch.  eval_finding: the cases named in the module docstring, where the eval kernel is held to the
    trainer's own yardstick instead."""
    for r in res:
        out, ref, ref64 = r["hip"][0], r["t32"][0], r["t64"][0]
        for k in ("color", "transmittance"):
            e_t32 = float((ref[k].double() - ref64[k]).abs().max())
            e_hip = float((out[k].double() - ref64[k]).abs().max())
            e_ev = float((out["eval_" + k].double() - ref64[k]).abs().max())
            d_ev = float((out[k] - out["eval_" + k]).abs().max())
            print(f"uv_edges {label} {k}: trainer {e_hip:.2e} eval kernel {e_ev:.2e} fp32 torch {e_t32:.2e} of fp64; trainer - eval {d_ev:.2e}")
            if eval_finding:
                assert e_ev < max(PIX_TOL, 4 * e_t32), (label, k, "eval kernel", e_ev, e_t32)
            else:
                assert d_ev < PIX_TOL, (label, k, "against the eval kernel", d_ev)
            assert e_hip < max(PIX_TOL, 4 * e_t32), (label, k, e_hip, e_t32)
        assert out["points_original"].shape == ref["points_original"].shape
        assert torch.allclose(out["points_original"], ref["points_original"], rtol=0, atol=1e-6), label
        # every ray and sample: the tensors are compared whole, never a sample of them
        e_w = float((out["points_inverse_weights"] - ref["points_inverse_weights"]).abs().max())
        assert e_w < 1e-4, (label, "points_inverse_weights", e_w)
        e_uv = float((ref["uv"].double() - ref64["uv"]).abs().max())
        e_uv_hip = float((out["uv"].double() - ref64["uv"]).abs().max())
        assert e_uv_hip < max(1e-4, 4 * e_uv), (label, "uv", e_uv_hip, e_uv)
        assert torch.allclose(out["points"], ref["points"], rtol=1e-5, atol=1e-6), label
        print(f"uv_edges {label} forward: weights {e_w:.2e} uv {e_uv_hip:.2e} (fp32 torch {e_uv:.2e})")


@pytest.mark.parametrize("prim", ["square", "sphere"])
@pytest.mark.parametrize("V", E.EDGE_V)
def test_an_exact_in_cube_count_at_the_chunk_edges(V, prim):
    S = E.EDGE_V_S
    res = _three(prim, S, lambda seed: (E.model_params(seed, prim), E.edge_batch(seed, prim, S, V=V)), BG1)
    for r in res:
        assert _in_cube(r["hip"][0]["points_original"]) == V and (r["batch"]["raydir"].shape[1] * S) % 16 != 0
    _check_forward(res, f"V={V} {prim}")
    _check_gradients(res, f"V={V} {prim}")
    if V == 0:
        tone = torch.pow(_t(BG1, torch.float64) + 1e-5, 1 / 2.2).clamp(0, 1)
        for r in res:
            out, render = r["hip"][0], [k for k in r["hip"][2]["l1"] if not k.startswith("inverse_gauge.")]
            assert len(render) == 58
            for tag, _ in LOSSES:
                assert all(bool((r["t64"][2][tag][k] == 0).all()) and bool((r["hip"][2][tag][k] == 0).all()) for k in render), tag
            assert bool((out["transmittance"] == 1).all()) and bool((out["points_inverse_weights"] == 0).all())
            assert float((out["color"].double() - tone[:, None, :]).abs().max()) < 1e-6


@pytest.mark.parametrize("prim", ["square", "sphere"])
@pytest.mark.parametrize("R", E.EDGE_RAYS)
def test_ray_counts_past_one_scan_thread_each_and_ragged_ray_blocks(R, prim):
    S = E.EDGE_RAYS_S
    res = _three(prim, S, lambda seed: (E.model_params(seed, prim), E.edge_batch(seed, prim, S, R=R)), BG1)
    assert res[0]["hip"][0]["points_inverse_weights"].shape == (1, R, S) and res[0]["hip"][0]["uv"].shape[:3] == (1, R, S)
    _check_forward(res, f"R={R} {prim}", eval_finding=(R, prim) in EVAL_FINDING)
    _check_gradients(res, f"R={R} {prim}")


@pytest.mark.parametrize("prim", ["square", "sphere"])
def test_three_cameras_with_three_backgrounds(prim):
    n, R = E.EDGE_CAMS
    S = E.EDGE_RAYS_S
    res = _three(prim, S, lambda seed: (E.model_params(seed, prim), E.edge_batch(seed, prim, S, R=R, n_cams=n)), BG3)
    for r in res:
        # the background reaches the picture: every camera has rays that see it, and the three differ
        assert (r["hip"][0]["transmittance"].amax(1) > 0.5).all()
    _check_forward(res, f"cams={n}x{R} {prim}", eval_finding=("cams", prim) in EVAL_FINDING)
    _check_gradients(res, f"cams={n}x{R} {prim}")


@pytest.mark.parametrize("prim", ["square", "sphere"])
def test_a_small_batch_after_a_large_one_reads_none_of_its_rows(prim):
    seed = E.EDGE_SEEDS[0]
    params = E.model_params(seed, prim)
    big = E.edge_batch(seed, prim, E.EDGE_RAYS_S, R=E.EDGE_RAYS[-1])
    small = E.edge_batch(seed, prim, E.EDGE_V_S, V=17)
    net = E.make_net(params, prim, E.EDGE_V_S, DEV)
    net.differentiable = True
    fresh = _one(net, small, E.EDGE_V_S, torch.float32, True, BG1)          # releases its engine
    assert net.grad_engine is None
    _one(net, big, E.EDGE_RAYS_S, torch.float32, True, BG1, keep_engine=True)
    after = [_one(net, small, E.EDGE_V_S, torch.float32, True, BG1, keep_engine=True)]
    eng = net.grad_engine
    assert (eng.max_rays, eng.max_samples) == (E.EDGE_RAYS[-1], E.EDGE_V_S)
    # once more, now that the engine no longer grows: the large batch's rows are in the very buffers the small one uses
    _one(net, big, E.EDGE_RAYS_S, torch.float32, True, BG1, keep_engine=True)
    after.append(_one(net, small, E.EDGE_V_S, torch.float32, True, BG1, keep_engine=True))
    assert net.grad_engine is eng
    net.release_grad_engine()
    for got in after:
        for k in fresh[0]:
            assert torch.equal(got[0][k], fresh[0][k]), k
        for tag, _ in LOSSES:
            assert got[1][tag] == fresh[1][tag]
            assert len(fresh[2][tag]) == 58 + 10          # the render layers and the inverse network
            assert all(torch.equal(got[2][tag][k], fresh[2][tag][k]) for k in fresh[2][tag]), tag


@pytest.mark.parametrize("which", ["density", "color1"])
def test_softplus_arguments_on_both_sides_of_the_threshold(which):
    S = 24
    stats = {}

    def make(seed):
        params, b, stats[seed] = E.softplus_case(seed, which, S=S)
        return params, b

    res = _three("square", S, make, None)
    for seed, s in stats.items():
        assert 0.1 <= s["above"] <= 0.9 and s["gap"] > 1e-4, (seed, s)
        if which == "color1":
            assert s["unclamped"] >= 0.5, (seed, s)
        print(f"uv_edges softplus {which} seed {seed}: {s}")
    _check_forward(res, f"softplus {which}")
    _check_gradients(res, f"softplus {which}")
