"""CPU checks behind tests/test_gpu_uv_render_edges.py: what that module feeds the NeuTex render kernel, and what it holds it to, is checked
here before a GPU sees it.  The C oracle, never compared with anything above 64 samples per ray before, against the fp64 eager forward at 65,
128 and 200 samples; the float32 compositing chain inside the rounding bound B(S) of float64 compositing at every sample count the GPU module
uses; the ray batches reach the pair totals and the geometries they promise; the expected work counters on a mask written by hand."""
import numpy as np
import pytest
import torch

import ngf_amd  # noqa: F401
import uv_render_ref as R
import uv_train_eager as E

BG = np.array([0.2, 0.5, 0.8], np.float32)


def _eager(seed, prim, cam, rd, U, bg, dtype):
    net = E.make_net(E.model_params(seed, prim), prim, U.shape[-1], "cpu", dtype)
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)          # noqa: E731
    with torch.no_grad():
        o = E.forward(net, t(cam), t(rd), None if bg is None else t(bg)[None], t(U), t(R.template(prim)), extras=True)
    return o["color"].double().numpy(), o["transmittance"].double().numpy(), o["valid"].numpy()


@pytest.mark.parametrize("prim", ["sphere", "square"])
@pytest.mark.parametrize("S", [65, 128, 200])
def test_the_oracle_above_one_chunk_matches_fp64(S, prim):
    seed = R.MODEL_SEEDS[prim == "square"]
    cam, rd, U = R.pool_rays(prim, S, R.SEED, R=23)
    c64, t64, v64 = _eager(seed, prim, cam, rd, U, BG, torch.float64)
    c32, t32, _ = _eager(seed, prim, cam, rd, U, BG, torch.float32)
    o = R.oracle_render(seed, prim, cam, rd, U, BG)
    assert np.array_equal(o["valid"], v64) and np.array_equal(v64, R.valid64(cam, rd, U))
    assert v64.sum() > 5 * S and (v64.sum(-1) == 0).sum() == 3
    for name, got, ref32, ref64 in (("colour", o["color"], c32, c64), ("transmittance", o["trans"], t32, t64)):
        e_o, e_t = float(np.abs(got - ref64).max()), float(np.abs(ref32 - ref64).max())
        print(f"S={S} {prim} {name}: oracle {e_o:.2e} fp32 torch {e_t:.2e} of fp64")
        assert e_o < max(2e-5, 4 * e_t), (name, e_o, e_t)


@pytest.mark.parametrize("S", sorted(set(R.CHUNK_S + R.PAIR_S + R.GEOMETRY_S)))
def test_float32_compositing_stays_inside_the_rounding_bound(S):
    prim = ("sphere", "square")[S % 2]
    seed = R.MODEL_SEEDS[S % 2]
    cam, rd, U = R.pool_rays(prim, S, R.SEED, R=23)
    o = R.oracle_render(seed, prim, cam, rd, U, BG)
    sigma, col, valid = o["sigma"][0], o["col"][0], o["valid"][0]
    B = R.bound(S, col[valid].max())
    lin64, c64, T64 = R.composite64(sigma, col, valid, U[0], BG)
    lin32, c32, T32 = R.composite32(sigma, col, valid, U[0], BG)
    e_lin, e_T = float(np.abs(lin32 - lin64).max()), float(np.abs(T32 - T64).max())
    print(f"S={S}: |composite32 - composite64| colour {e_lin:.2e} T {e_T:.2e}, B(S) {B:.2e}")
    assert e_lin <= B and e_T <= B
    # the float32 chain is the oracle's own: the same transmittance to an ulp of expf, the same pixel to a few of powf
    assert float(np.abs(T32 - o["trans"][0]).max()) < 1e-6 and float(np.abs(c32 - o["color"][0]).max()) < 2e-6
    # and the bound can see a defect: a sample dropped, and a transmittance that restarts at the chunk edge
    hit = valid.sum(-1) > 0
    drop = valid.copy()
    drop[np.arange(len(drop)), np.argmax(valid, -1)] = False
    lin_d, _, T_d = R.composite64(sigma, col, drop, U[0], BG)
    assert (np.abs(lin_d - lin64)[hit].max(-1) > B).mean() > 0.5 and (np.abs(T_d - T64)[hit] > B).mean() > 0.5
    if S > R.CHUNK:
        tail = valid.copy()
        tail[:, :R.CHUNK] = False
        assert (np.abs(R.composite64(sigma, col, tail, U[0], BG)[2] - T64)[hit] > B).mean() > 0.5


@pytest.mark.parametrize("S", R.PAIR_S)
def test_the_paired_batches_reach_every_total(S):
    cam, rd, U = R.paired_rays(S, R.pair_targets(S))
    assert rd.shape[1] == 2 * len(R.PAIR_TARGETS + R.PAIR_EXTRA)
    o = R.oracle_render(R.MODEL_SEEDS[0], "sphere", cam, rd, U)
    assert np.array_equal(o["valid"], R.valid64(cam, rd, U))          # the pool's margin: fp32 and fp64 agree
    totals = R.pair_chunk_totals(o["valid"], S)
    assert set(R.PAIR_TARGETS) <= set(totals.reshape(-1).tolist()), totals
    assert all(t in totals[k] for k, t in enumerate(R.pair_targets(S)))
    both = [k for k, t in enumerate(totals) if 16 < t.max() < 128]
    assert all(o["valid"][0, 2 * k].any() and o["valid"][0, 2 * k + 1].any() for k in both)          # the list crosses from ray 0 to ray 1


@pytest.mark.parametrize("S", R.GEOMETRY_S)
def test_the_geometry_batches_hold_what_they_promise(S):
    got = {}
    for kind in R.GEOMETRY_KINDS:
        cam, rd, U = R.geometry_rays(kind, S)
        valid = R.oracle_render(R.MODEL_SEEDS[0], "sphere", cam, rd, U)["valid"]
        got[kind] = (cam, rd, valid, valid.sum(-1), R.slab_hits(cam, rd))
        assert rd.shape[0] * rd.shape[1] >= 4 and np.allclose(np.linalg.norm(rd, axis=-1), 1.0, atol=1e-6), kind
    _, _, _, n, hits = got["miss"]
    assert (~hits).sum() >= 4 and (n[~hits] == 0).all()           # the slab test fails: t0 = 0, and (the cube is convex) no sample is in it
    assert (hits & (n == 0)).sum() >= 2                           # the cube behind the camera: t0 = 0 by the clamp
    assert (n == 0).sum() >= 4 and (n > 0).sum() >= 4             # both rays with no in-cube sample and rays with some
    assert ((n.reshape(-1)[:-1] == 0) & (n.reshape(-1)[1:] > 0)).any()
    cam, _, _, n, hits = got["inside"]
    assert (np.abs(cam) < 1).all() and hits.all() and (n > 0).all() and (n < S).all()
    cam, rd, valid, n, hits = got["axis"]
    assert not (np.abs(cam) == 1).any() and ((rd == 0).sum(-1) >= 1).all() and np.signbit(rd[rd == 0]).any()
    for axis in range(3):
        for sign in (1.0, -1.0):
            assert ((rd[0, :, axis] == sign) & ((rd[0] == 0).sum(-1) == 2)).any()
    assert ((rd == 0).sum(-1) == 1).sum() >= 4 and (n[0] == S).any() and (n[0] == 0).any() and (n[1] > 0).all()
    _, _, valid, n, _ = got["diagonal"]
    assert valid.all() and valid.shape[1] % 2 == 0 and valid.shape[1] >= 4
    _, _, _, n, hits = got["graze"]
    assert (n == 0).any() and ((n >= 1) & (n <= 4)).any() and n.max() <= 8 and hits.any() and not hits.all()


def test_the_expected_counters_on_a_mask_written_by_hand():
    S = 70                                   # a chunk of 64 and one of 6
    v = np.zeros((5, S), bool)
    v[0, :17] = True                         # pair 0, chunk 0: 17 + 4 = 21 -> 2 passes
    v[1, 60:] = True                         #         chunk 1:  0 + 6      -> 1
    v[3, :] = True                           # pair 1 (ray 2 has nothing): 64 -> 4, 6 -> 1
    v[4, :65] = True                         # the unpaired last ray: 64 -> 4, 1 -> 1
    assert R.pair_chunk_totals(v, S).tolist() == [[21, 6], [64, 6], [64, 1]]
    assert R.expected_stats(v, S) == (17 + 10 + 70 + 65, 2 + 1 + 4 + 1 + 4 + 1)
    assert R.expected_stats(v[None], S) == R.expected_stats(v, S)          # [N,R,S]: the launch's rays in order
    assert R.expected_stats(np.zeros((3, 64), bool), 64) == (0, 0)
    assert R.expected_stats(np.ones((2, 64), bool), 64) == (128, 8) and R.expected_stats(np.ones((1, 1), bool), 1) == (1, 1)
