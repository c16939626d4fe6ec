"""Point queries on the GPU (Base.query / ngf_field_query): density, colour and gauge-shifted plane coordinates at world-space points.

Reference-pinned part: the sample points of the first 8 rays of every golden case are rebuilt in numpy fp32 as p = o + d * z (a separate multiply
and add, like the reference's sample_ray), queried with the ray's direction, and compared with the reference's own per-sample intermediates
(i_valid, i_sigma, i_coords, i_rgb at i_rgb_mask) at every optimisation level the per-sample tests of test_gpu_parity.py run, plus level 3.

Edge part: batch sizes around the 16-point pass and the 64-point wave, one workgroup walking many tiles, permutations, hostile points (NaN, inf,
3e38, just outside the box), the shared-direction form, consistency with compute_alpha / decode_rgb, determinism across streams, and the
argument refusals of the C entry point."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import field_for_case, load_case

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TRIPLANE = ["triplane_r1_gauge", "triplane_r2_nogauge", "triplane_r1_mask", "triplane_r0"]
INFOINV = ["infoinv_r1_on", "infoinv_r1_off", "infoinv_r1_mask"]
LEVELS = {"level1": {}, "level2": {"bake": True}, "level3": {"bake": True, "bake_color": True}, "no_fold": {"no_fold": True},
          "split_bf16": {"split_bf16": True}}
PINNED = [(n, lv) for n in TRIPLANE for lv in LEVELS] + [(n, lv) for n in INFOINV for lv in ("level1", "split_bf16")]
# colour bound per sample: the criterion of test_per_sample_colours_match_the_reference; level 3 has no per-sample bound of its own and takes the
# pixel bound every level meets (test_render_matches_oracle_and_reference): a pixel of a one-sample opaque ray IS that sample's colour
RGB_BOUND = {"level1": 5e-6, "level2": 5e-6, "no_fold": 5e-6, "split_bf16": 5e-6, "level3": 2e-5}


def _mode(g):
    if "gauge_on" in g:
        return {"iteration": 30001 if int(g["gauge_on"]) else -1}
    return {"infoinv": bool(int(g["infoinv"]))}


def _kernel_mode(g):
    return int(g["gauge_on"]) if "gauge_on" in g else int(g["infoinv"])


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """Two query results, bit for bit."""
    return a.keys() == b.keys() and all(a[k].shape == b[k].shape and torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


def _rows(r, idx):
    return {k: v[idx] for k, v in r.items()}


def _sample_points(g):
    """The sample points of the first 8 rays in fp32, p = o + d * z with the product rounded before the sum, and the rays' directions per point."""
    o, d = g["rays"][:8, None, :3].astype(np.float32), g["rays"][:8, None, 3:6].astype(np.float32)
    z = g["i_z"][..., None].astype(np.float32)
    prod = (d * z).astype(np.float32)
    p = (o + prod).astype(np.float32)
    dirs = np.ascontiguousarray(np.broadcast_to(d, p.shape)).astype(np.float32)
    a = g["aabb"].astype(np.float32)
    in_box = ((p >= a[0]) & (p <= a[1])).all(-1)
    return p, dirs, in_box


@pytest.mark.parametrize("name,level", PINNED)
def test_query_matches_the_reference_per_sample(name, level):
    g, params, step, mask = load_case(name)
    f = field_for_case(g, params, mask, **LEVELS[level])
    p, dirs, in_box = _sample_points(g)
    valid, m = g["i_valid"], g["i_rgb_mask"]
    if mask is None:
        assert np.array_equal(in_box, valid)                 # the rebuilt points reproduce the reference's in-box test
    else:
        assert not (valid & ~in_box).any()                   # a superset: the reference's valid also went through its alpha mask
    assert 250 <= int(in_box.sum()) <= 330
    r = f.query(torch.from_numpy(p), torch.from_numpy(dirs), want_coords=True, **_mode(g))
    sigma, rgb, coords = (r[k].cpu().numpy() for k in ("sigma", "rgb", "coords"))
    assert sigma.shape == valid.shape and rgb.shape == valid.shape + (3,) and coords.shape == valid.shape + (6,)

    # 1. zero pattern
    assert np.array_equal(sigma == 0, ~valid)
    assert not rgb[~in_box].any() and not coords[~in_box].any()
    if mask is not None:
        r_nm = f.query(torch.from_numpy(p), use_mask=False, **_mode(g))
        assert set(r_nm) == {"sigma"}
        s_nm = r_nm["sigma"].cpu().numpy()
        assert np.array_equal(s_nm == 0, ~in_box)
        assert np.array_equal(s_nm[valid].view(np.uint32), sigma[valid].view(np.uint32))       # the mask only zeroes

    # 2. sigma
    np.testing.assert_allclose(sigma, g["i_sigma"], rtol=2e-5, atol=1e-9)

    # 3. colour at the reference's active samples
    if m.any():
        assert not (m & ~in_box).any()
        e_rgb = float(np.abs(rgb[m] - g["i_rgb"][m]).max())
        print(f"{name} {level}: {int(m.sum())} coloured samples, max |rgb - reference| = {e_rgb:.3e} (bound {RGB_BOUND[level]:.0e})")
        assert e_rgb < RGB_BOUND[level], e_rgb
        assert int(m.sum()) >= 20
    else:
        assert name == "triplane_r0" and not g["i_rgb"].any()         # the literal random-init preset has no active sample
    assert np.isfinite(rgb).all() and (rgb >= 0).all() and (rgb <= 1).all()

    # 4. coordinates at the reference's valid samples
    if "gauge_on" in g and int(g["gauge_on"]):
        e_c = float(np.abs(coords[valid] - g["i_coords"][valid]).max())
        print(f"{name} {level}: max |coords - reference| = {e_c:.3e} (bound 2e-6: ~13 fp32 roundings at magnitude <= 2)")
        assert e_c <= 2e-6, e_c
    else:
        assert np.array_equal(coords[valid].view(np.uint32), g["i_coords"][valid].view(np.uint32))


# ---- edges -----------------------------------------------------------------------------------------------------------------------------------
EDGE = ["triplane_r1_gauge", "triplane_r1_mask", "infoinv_r1_on"]
EDGE_FLAGS = {"triplane_r1_gauge": {"bake": True, "bake_color": True}, "triplane_r1_mask": {}, "infoinv_r1_on": {}}


@functools.lru_cache(maxsize=None)
def _edge_field(name):
    g, params, step, mask = load_case(name)
    return g, field_for_case(g, params, mask, **EDGE_FLAGS[name])


@functools.lru_cache(maxsize=None)
def _edge_points(name, n=1000):
    """n seeded points in a box 10 % larger than the aabb (about a quarter of them outside) and unit directions, on the device."""
    g, f = _edge_field(name)
    rng = np.random.default_rng(11)
    a = g["aabb"].astype(np.float32)
    c, h = (a[0] + a[1]) / 2, (a[1] - a[0]) / 2
    pts = (c + h * rng.uniform(-1.1, 1.1, (n, 3))).astype(np.float32)
    dirs = rng.standard_normal((n, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    return torch.from_numpy(pts).cuda(), torch.from_numpy(dirs).cuda()


def _q(name, pts, dirs, **kw):
    g, f = _edge_field(name)
    return f.query(pts, dirs, want_coords=True, **_mode(g), **kw)


@pytest.mark.parametrize("name", EDGE)
def test_batch_sizes_and_one_workgroup_walking_many_tiles(name):
    from ngf_amd._lib import knobs
    pts, dirs = _edge_points(name)
    full = _q(name, pts, dirs)
    assert full["sigma"].shape == (1000,) and full["rgb"].shape == (1000, 3) and full["coords"].shape == (1000, 6)
    assert int((full["coords"] != 0).any(-1).sum()) > 100 and int((full["coords"] == 0).all(-1).sum()) > 100      # both kinds of point are in the batch
    for n in (0, 1, 15, 16, 17, 63, 64, 65, 255, 257):
        part = _q(name, pts[:n], dirs[:n])
        assert part["sigma"].shape == (n,) and part["rgb"].shape == (n, 3) and part["coords"].shape == (n, 6)
        assert _same(part, _rows(full, slice(0, n))), n
    with knobs(grid=1):                                     # restored on exit, also when the block raises
        one = _q(name, pts, dirs)
    assert _same(one, full)


@pytest.mark.parametrize("name", EDGE)
def test_a_permutation_of_the_points_permutes_the_outputs(name):
    pts, dirs = _edge_points(name)
    full = _q(name, pts, dirs)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(pts.shape[0])).cuda()
    shuffled = _q(name, pts[perm], dirs[perm])
    back = {k: torch.empty_like(v) for k, v in shuffled.items()}
    for k in back:
        back[k][perm] = shuffled[k]
    assert _same(back, full)


def _hostile(a):
    """(points, inside flags): corners, face centres and interior points of the box, and points that are outside in every way there is."""
    a0, a1 = a[0].astype(np.float32), a[1].astype(np.float32)
    c = ((a0 + a1) / 2).astype(np.float32)
    inside = [np.where([(k >> j) & 1 for j in range(3)], a1, a0) for k in range(8)]                  # the eight corners: inside by the <= test
    for ax in range(3):
        for b in (a0, a1):
            q = c.copy(); q[ax] = b[ax]; inside.append(q)                                            # face centres
    rng = np.random.default_rng(9)
    h = (a1 - a0) / 2
    inside += list((c + h * rng.uniform(-0.9, 0.9, (50, 3))).astype(np.float32))
    outside = []
    for ax in range(3):
        q = c.copy(); q[ax] = np.nextafter(a1[ax], np.float32(np.inf)); outside.append(q)            # just outside
        q = c.copy(); q[ax] = np.nextafter(a0[ax], np.float32(-np.inf)); outside.append(q)
        for v in (1e6, -1e6, 3e38, -3e38, np.nan, np.inf, -np.inf):
            q = c.copy(); q[ax] = np.float32(v); outside.append(q)
    q = a1.copy(); q[0] = np.nextafter(a1[0], np.float32(np.inf)); outside.append(q)                 # a corner, one component a step out
    outside += [np.full(3, np.nan, np.float32), np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32), np.full(3, 3e38, np.float32)]
    outside += list((c + h * rng.uniform(1.01, 4.0, (len(inside) - len(outside), 3)) * rng.choice([-1, 1], (len(inside) - len(outside), 3))).astype(np.float32))
    assert len(inside) == len(outside) == 64
    # mixed waves, then a pass of 16 and a whole wave of outside points, then a tail of inside points
    order = []
    for k in range(24):
        order += [("i", k), ("o", k)]
    order += [("o", k) for k in range(24, 40)] + [("i", k) for k in range(24, 40)]                 # rows 48-63: the last pass of wave 0 holds no inside point
    order += [("o", k) for k in range(40, 64)] + [("o", k) for k in range(0, 24)]                  # rows 80-127
    order += [("o", k) for k in range(64)] + [("i", k) for k in range(40, 64)]                     # rows 128-191: a whole wave of outside points
    pts = np.stack([inside[k] if w == "i" else outside[k] for w, k in order]).astype(np.float32)
    flag = np.array([w == "i" for w, _ in order])
    return pts, flag


@pytest.mark.parametrize("name", EDGE)
def test_hostile_points_give_exact_zeros_and_do_not_disturb_their_neighbours(name):
    g, f = _edge_field(name)
    pts, inside = _hostile(g["aabb"])
    assert inside.sum() * 2 <= len(pts)
    rng = np.random.default_rng(4)
    dirs = rng.standard_normal(pts.shape).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    bad = np.flatnonzero(~inside)[::3]
    dirs[bad] = np.nan                                        # a direction nobody may read
    P, D = torch.from_numpy(pts).cuda(), torch.from_numpy(dirs).cuda()
    r = _q(name, P, D, use_mask=False)
    ins = torch.from_numpy(inside).cuda()
    for k, v in r.items():
        assert not torch.isnan(v).any(), k
        assert int(torch.count_nonzero(v[~ins])) == 0, k      # exact zeros outside
    assert bool((r["coords"][ins] != 0).any(-1).all())        # corners and face centres count as inside: they have coordinates
    alone = _q(name, P[ins], D[ins], use_mask=False)
    assert _same(_rows(r, ins), alone)
    # the same with the alpha mask in force (a no-op for the fields without one) and with one shared direction
    rm = _q(name, P, D)
    assert _same(_rows(rm, ins), _q(name, P[ins], D[ins])) and all(int(torch.count_nonzero(v[~ins])) == 0 for v in rm.values())


@pytest.mark.parametrize("name", EDGE)
def test_one_shared_direction_equals_its_broadcast(name):
    pts, _ = _edge_points(name)
    d = torch.tensor([0.3, -0.5, 0.8124038], device="cuda")
    a = _q(name, pts[:333], d)
    b = _q(name, pts[:333], d.expand(333, 3))
    assert _same(a, b)
    g, f = _edge_field(name)
    with pytest.raises(ValueError):
        f.query(pts[:8], torch.zeros(4, 3, device="cuda"), **_mode(g))
    # [..., 3] in, [...] out
    r = f.query(pts[:12].view(3, 4, 3), d, **_mode(g))
    assert set(r) == {"sigma", "rgb"} and r["sigma"].shape == (3, 4) and r["rgb"].shape == (3, 4, 3)
    assert torch.equal(_bits(r["sigma"].reshape(-1)), _bits(a["sigma"][:12]))


@pytest.mark.parametrize("name", EDGE)
def test_query_agrees_with_compute_alpha_and_decode_rgb(name):
    g, f = _edge_field(name)
    pts, dirs = _edge_points(name)
    r = _q(name, pts, dirs)
    inb = ((pts >= f.aabb[0].cuda()) & (pts <= f.aabb[1].cuda())).all(-1)
    assert 100 < int(inb.sum()) < 1000
    p, d = pts[inb], dirs[inb]
    sigma, rgb, coords = r["sigma"][inb], r["rgb"][inb], r["coords"][inb]
    length = float(f.stepSize)
    akw = {} if "gauge_on" in g else _mode(g)
    if "gauge_on" in g:                                       # compute_alpha runs TriPlane with the gauge off
        sigma = f.query(p, iteration=-1)["sigma"]
    alpha = f.compute_alpha(p, length, **akw)
    assert torch.equal(alpha == 0, sigma == 0)
    want = 1.0 - np.exp(-sigma.cpu().numpy().astype(np.float64) * length)
    err = np.abs(alpha.cpu().numpy() - want)
    print(f"{name}: max |compute_alpha - (1 - exp(-sigma * length))| = {err.max():.3e}")
    np.testing.assert_allclose(alpha.cpu().numpy(), want, rtol=1e-6, atol=1e-7)
    again = f.decode_rgb(coords, d, mode=_kernel_mode(g))
    e = float((again - rgb).abs().max())
    print(f"{name}: decode_rgb at the query's coordinates: max difference {e:.3e}, bit-identical: {torch.equal(_bits(again), _bits(rgb))}")
    assert e < RGB_BOUND["level3" if EDGE_FLAGS[name].get("bake_color") else "level1"]


@pytest.mark.parametrize("name", EDGE)
def test_two_calls_one_of_them_on_a_side_stream_are_bit_identical(name):
    pts, dirs = _edge_points(name)
    a = _q(name, pts, dirs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b = _q(name, pts, dirs)
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert _same(a, b)


def test_sigma_only_and_coords_only_calls():
    """The calls that need no colour stage (and, for InfoInv coordinates, no MLP at all) return the rows of the full call."""
    from ngf_amd import _lib
    for name in EDGE:
        g, f = _edge_field(name)
        pts, dirs = _edge_points(name)
        full = _q(name, pts, dirs)
        assert torch.equal(_bits(f.query(pts, **_mode(g))["sigma"]), _bits(full["sigma"]))
        co = torch.full((pts.shape[0], 6), 7.0, device="cuda")
        _lib.check(_lib.lib().ngf_field_query(f.handle(), pts.data_ptr(), pts.shape[0], _kernel_mode(g), None, 3, 0, None, None, co.data_ptr(),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        assert torch.equal(_bits(co), _bits(full["coords"]))


@pytest.mark.parametrize("level", ["level2", "level3", "split_bf16_baked"])
def test_equal_square_gauge_planes_take_the_shared_axis_density_side(level):
    """The golden cases have 12 x 14 gauge planes (the GaugeAny density side at levels 2 and 3).  Three square gauge planes of one size take the
    shared-axis set-up instead: same operations per axis, so the coordinates are the bits of the level-1 kernel's (which sets every plane's cell
    up on its own); sigma moves by the baked density planes' rounding only (|d sigma| <= 2e-6 relative, inside the 2e-5 of the sigma check)."""
    from ngf_amd import synth
    g, _, _, _ = load_case("triplane_r1_gauge")
    plane_hw = tuple(tuple(int(v) for v in hw) for hw in g["plane_hw"])
    params = synth.triplane_params(int(g["seed"]), plane_hw, (12, 12), preset=str(g["preset"]), gauge_std=float(g["gauge_std"]))
    flags = {"level2": {"bake": True}, "level3": {"bake": True, "bake_color": True}, "split_bf16_baked": {"bake": True, "bake_color": True, "split_bf16": True}}[level]
    base, f = field_for_case(g, params, None), field_for_case(g, params, None, **flags)
    pts, dirs = _edge_points("triplane_r1_gauge")
    a = base.query(pts, dirs, want_coords=True, iteration=30001)
    b = f.query(pts, dirs, want_coords=True, iteration=30001)
    assert int((a["coords"] != 0).any(-1).sum()) > 100
    assert torch.equal(_bits(a["coords"]), _bits(b["coords"]))
    assert torch.equal(a["sigma"] == 0, b["sigma"] == 0)
    np.testing.assert_allclose(b["sigma"].cpu().numpy(), a["sigma"].cpu().numpy(), rtol=2e-5, atol=1e-9)
    e = float((a["rgb"] - b["rgb"]).abs().max())
    print(f"{level}: max |rgb - level 1's| = {e:.3e}")
    assert e < RGB_BOUND["level1"] + RGB_BOUND["level3"]    # two levels, each within its per-sample bound of the reference
    inb = pts[(a["coords"] != 0).any(-1)]                    # compute_alpha has no box test of its own: in-box points only
    alpha = f.compute_alpha(inb, float(f.stepSize))
    want = 1.0 - np.exp(-f.query(inb, iteration=-1)["sigma"].cpu().numpy().astype(np.float64) * float(f.stepSize))
    np.testing.assert_allclose(alpha.cpu().numpy(), want, rtol=1e-6, atol=1e-7)


def test_argument_refusals_with_a_live_handle():
    from ngf_amd import _lib
    g, f = _edge_field("triplane_r1_gauge")
    pts, dirs = _edge_points("triplane_r1_gauge")
    L, h = _lib.lib(), f.handle()
    n = 64
    sig = torch.full((n,), 7.0, device="cuda")
    rgb = torch.full((n, 3), 7.0, device="cuda")
    X, D, S, R = pts.data_ptr(), dirs.data_ptr(), sig.data_ptr(), rgb.data_ptr()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bad = {
        "null handle": (None, X, n, 1, D, 3, 0, S, R, None, st),
        "null xyz": (h, None, n, 1, D, 3, 0, S, R, None, st),
        "negative n": (h, X, -1, 1, D, 3, 0, S, R, None, st),
        "dir_stride 1": (h, X, n, 1, D, 1, 0, S, R, None, st),
        "dir_stride 6": (h, X, n, 1, D, 6, 0, S, R, None, st),
        "unknown flag": (h, X, n, 1, D, 3, 2, S, R, None, st),
        "rgb without dirs": (h, X, n, 1, None, 3, 0, S, R, None, st),
        "no output": (h, X, n, 1, D, 3, 0, None, None, None, st),
    }
    for what, args in bad.items():
        assert L.ngf_field_query(*args) == 1, what
        assert b"ngf_field_query" in L.ngf_last_error(), what
    torch.cuda.synchronize()
    assert bool((sig == 7).all()) and bool((rgb == 7).all())          # refused before anything ran
    assert L.ngf_field_query(h, X, 0, 1, D, 3, 0, S, R, None, st) == 0          # n == 0 is fine
    assert L.ngf_field_query(h, X, n, 1, D, 3, _lib.QUERY_NO_MASK, S, R, None, st) == 0
    torch.cuda.synchronize()
    assert bool((sig != 7).all())
