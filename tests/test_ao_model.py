"""The numpy model of the ambient-occlusion stage (tests/ao_model.py) against the CPU oracle, no GPU: it is deterministic, a sample depends
on (seed, path, depth, s) only, the directions are unit vectors of the hemisphere, and on scenes whose answer is known on paper -- an open
sky, a closed box, the foot of a long wall -- the oracle's any-hit trace of its rays gives that answer."""
import numpy as np
import pytest

import ao_model as am
import bounce_model as bm
from helpers import build_oracle

BIAS = 1e-3
SEED = 0xA0
S_BIG = 4096
MARGIN = 4.0 * np.sqrt(0.25 / S_BIG)  # 4 sigma of a binomial with p = 1/2 over S_BIG samples: 0.031


def quad(a, b, c, d):
    return np.array([np.concatenate([a, b, c]), np.concatenate([a, c, d])], np.float32)


def scene_of(oracle, soups):
    o = oracle.Scene()
    for verts in soups:
        o.add_instance(o.add_blas(verts), None, 0)
    return o.build()


def one_hit(oracle, o, origin, direction):
    rays = oracle.make_rays(np.array([origin], np.float64), np.array([direction], np.float64))
    hits = o.trace(rays)
    assert hits["hit"][0] == 1
    return rays, hits


FLOOR = quad((-2000, 0, -2000), (-2000, 0, 2000), (2000, 0, 2000), (2000, 0, -2000))


@pytest.fixture(scope="module")
def world(oracle):
    import raycore_jl_amd as rc
    cfg = rc.scenes.config_c3(lon=16, bands=9, lattice=(3, 3, 2))
    o = build_oracle(oracle, cfg)
    rays = rc.scenes.c3_primary_rays(cfg, 320, 200)[:63_997]
    hits = o.trace(rays, nthreads=16)
    lit = hits["hit"] == 1
    assert lit.sum() >= 1000 and (~lit).sum() >= 1000
    return o, rays, hits, lit


def test_deterministic_and_dummy_on_misses(world):
    o, rays, hits, lit = world
    a = am.ao_rays(o, rays, hits, 3, seed=SEED, depth=1, bias=BIAS, max_dist=2.5)
    b = am.ao_rays(o, rays, hits, 3, seed=SEED, depth=1, bias=BIAS, max_dist=2.5)
    assert a.dtype == bm.RAY_DT and len(a) == len(rays) * 3 and a.tobytes() == b.tobytes()
    a = a.reshape(len(rays), 3)
    assert np.all(a["tmax"][lit] == np.float32(2.5)) and np.all(a["tmin"] == 0)
    assert np.all(a["tmax"][~lit] == 0) and np.all(a["d"][~lit] == (0, 0, 1)) and np.all(a["o"][~lit] == 0)  # the dummy ray
    p, nrm = o.hit_points(rays[lit], hits[lit])
    assert np.array_equal(a["o"][lit][:, 0], p + nrm * np.float32(BIAS))  # the bounce stage's origin, the same for every sample
    assert np.array_equal(a["o"][lit][:, 0], a["o"][lit][:, 2])
    assert not np.array_equal(a["d"][lit][:, 0], a["d"][lit][:, 1])


def test_a_sample_depends_on_seed_path_depth_and_s_only(world):
    o, rays, hits, lit = world
    n = len(rays)
    base = am.ao_rays(o, rays, hits, 5, seed=SEED, depth=2, bias=BIAS).reshape(n, 5)
    # not on `samples`: the first three of five are the three of three
    three = am.ao_rays(o, rays, hits, 3, seed=SEED, depth=2, bias=BIAS).reshape(n, 3)
    assert three.tobytes() == np.ascontiguousarray(base[:, :3]).tobytes()
    # not on n or the slot: a permuted sub-queue with its path ids draws the same rays for the same path
    perm = np.random.default_rng(3).permutation(n)[:20_011]
    sub = am.ao_rays(o, rays[perm], hits[perm], 5, seed=SEED, depth=2, bias=BIAS, path_in=perm.astype(np.uint32)).reshape(len(perm), 5)
    assert sub.tobytes() == np.ascontiguousarray(base[perm]).tobytes()
    # path_base shifts the path: slot i with base 7 is path i + 7
    by_base = am.ao_rays(o, rays, hits, 5, seed=SEED, depth=2, bias=BIAS, path_base=7)
    by_ids = am.ao_rays(o, rays, hits, 5, seed=SEED, depth=2, bias=BIAS, path_in=np.arange(7, n + 7, dtype=np.uint32))
    assert by_base.tobytes() == by_ids.tobytes() and by_base.tobytes() != base.tobytes()
    # and each of seed, path, depth changes the directions of the hit slots
    for other in (dict(seed=SEED + 1, depth=2), dict(seed=SEED, depth=3), dict(seed=SEED, depth=2, path_base=7)):
        d = am.ao_rays(o, rays, hits, 5, bias=BIAS, **other).reshape(n, 5)["d"][lit]
        assert (d != base["d"][lit]).any(axis=2).mean() > 0.99, other


def test_counter_layout_is_spelled_out():
    """counter = (lo32 path, hi32 path, s, 0x414F0000 | depth), key = (lo32 seed, hi32 seed); the bounce stage's tag gives other numbers."""
    for path, s, depth, seed in ((0, 0, 0, 0), (63996, 4, 1, 0x5AD0), ((7 << 32) | 12345, 65535, 65535, 0xC0FFEE1234567890)):
        got = am.uniforms(np.array([path], np.uint64), s, depth, seed)
        r = bm.philox4x32_10(path & 0xFFFFFFFF, path >> 32, s, 0x414F0000 | depth, seed & 0xFFFFFFFF, seed >> 32)
        want = [bm.u32_to_unit(r[k]).reshape(-1)[0] for k in range(2)]
        assert [float(g[0]) for g in got] == [float(w) for w in want]
        assert all(0.0 <= float(g[0]) < 1.0 for g in got)
        b = bm.bounce_uniforms(np.array([path], np.uint64), s, depth, seed)
        assert (float(b[0][0]), float(b[1][0])) != (float(got[0][0]), float(got[1][0]))


def test_directions_are_unit_vectors_of_the_hemisphere():
    g = np.random.default_rng(11)
    k = 10_000
    nrm = g.normal(size=(k, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    nrm = bm.normalize3(nrm)  # unit in float32, as a hit frame's normal is
    d = am.directions(nrm, np.arange(k, dtype=np.uint64) * np.uint64(7919), g.integers(0, 65536, k), 3, SEED)
    assert d.dtype == np.float32 and d.shape == (k, 3)
    dots = np.einsum("ij,ij->i", d.astype(np.float64), nrm.astype(np.float64))
    assert dots.min() >= 0.0, dots.min()
    norms = np.linalg.norm(d.astype(np.float64), axis=1)
    assert np.abs(norms - 1.0).max() < 1e-5, np.abs(norms - 1.0).max()
    assert abs(dots.mean() - 2.0 / 3.0) < 0.01  # cosine-weighted: E[cos] = 2/3 (uniform over the hemisphere would give 1/2)


def test_open_sky_is_fully_visible(oracle):
    o = scene_of(oracle, [FLOOR])
    rays, hits = one_hit(oracle, o, (0.3, 5, 0.2), (0, -1, 0))
    counts, ar = am.expected_counts(o, rays, hits, S_BIG, seed=SEED, bias=BIAS)
    assert counts.shape == (1,) and counts[0] == S_BIG
    assert np.all(ar["d"][:, 1] >= 0) and np.all(np.isinf(ar["tmax"]))  # the normal faces the ray: up


def test_closed_box_is_fully_occluded_and_a_short_reach_opens_it(oracle):
    import raycore_jl_amd as rc
    o = scene_of(oracle, [rc.scenes.box_room((-1, -1, -1), (1, 1, 1), 1)])
    rays, hits = one_hit(oracle, o, (0.05, 0, -0.03), (0, -1, 0))  # the floor point (0.05, -1, -0.03): the nearest other wall is 0.95 away
    counts, _ = am.expected_counts(o, rays, hits, S_BIG, seed=SEED, bias=BIAS)
    assert counts[0] == 0
    counts, _ = am.expected_counts(o, rays, hits, S_BIG, seed=SEED, bias=BIAS, max_dist=0.9)  # shorter than the way to any wall
    assert counts[0] == S_BIG
    counts, _ = am.expected_counts(o, rays, hits, S_BIG, seed=SEED, bias=BIAS, max_dist=1.5)  # reaches the side walls, not the ceiling
    assert 0 < counts[0] < S_BIG


def test_foot_of_a_long_wall_sees_half(oracle):
    """A floor point 1e-3 from a wall 4000 long and 2000 tall, max_dist = 1: the half of the cosine-weighted hemisphere that leans toward
    the wall is blocked, but for the directions within about 1e-3 of parallel (a fraction of the order of 1e-3)."""
    wall = quad((0, -1, -2000), (0, 2000, -2000), (0, 2000, 2000), (0, -1, 2000))
    o = scene_of(oracle, [FLOOR, wall])
    rays, hits = one_hit(oracle, o, (1e-3, 5, 0.2), (0, -1, 0))
    for seed in (SEED, SEED + 1):
        counts, ar = am.expected_counts(o, rays, hits, S_BIG, seed=seed, bias=BIAS, max_dist=1.0)
        frac = counts[0] / S_BIG
        assert abs(frac - 0.5) <= MARGIN, (seed, frac)
        away = int((ar["d"][:, 0] >= 0).sum())  # the samples that lean away from the wall are the visible ones, the near-parallel few aside
        assert 0 <= int(counts[0]) - away <= 16, (seed, counts[0], away)
