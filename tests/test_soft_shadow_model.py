"""The numpy model of the soft-shadow stage (tests/soft_shadow_model.py) against the CPU oracle, no GPU: with one sample its rays are the
oracle's shadow rays bit for bit, with radius 0 every target is the light itself, and the Philox counter layout is pinned by literals."""
import numpy as np
import pytest

import bounce_model as bm
import soft_shadow_model as sm
from helpers import build_oracle

LIGHTS = np.array([[10, 10, 10], [-4, 6, 3], [3, 2.5, -6]], np.float32)
RADII = np.array([1.0, 0.5, 1.0], np.float32)
BIAS = 1e-3
N_RAYS = 63_997


@pytest.fixture(scope="module")
def world(oracle):
    import raycore_jl_amd as rc
    cfg = rc.scenes.config_c3(lon=16, bands=9, lattice=(7, 7, 6))
    o = build_oracle(oracle, cfg)
    rays = rc.scenes.c3_primary_rays(cfg, 320, 200)[:N_RAYS]
    hits = o.trace(rays, nthreads=16)
    lit = hits["hit"] == 1
    assert lit.sum() >= 1000 and (~lit).sum() >= 1000
    return o, rays, hits, lit


@pytest.mark.parametrize("l", [0, 1, 2])
def test_one_sample_is_the_oracles_shadow_ray(world, l):
    o, rays, hits, lit = world
    want = o.shadow_rays(rays, hits, LIGHTS[l], BIAS)
    got = sm.soft_shadow_rays(o, rays, hits, LIGHTS[l:l + 1], RADII[l:l + 1], 1, seed=0x50F7, bias=BIAS)
    a, b = want.view(np.uint32).reshape(-1, 8), got.view(np.uint32).reshape(-1, 8)
    same = (a == b).all(axis=1)
    assert same[lit].all(), f"light {l}: {int((~same[lit]).sum())} of {int(lit.sum())} hit slots differ"
    assert np.all(got["tmax"][~lit] == 0) and np.all(got["d"][~lit] == (0, 0, 1)) and np.all(got["o"][~lit] == 0)  # the dummy ray


def test_radius_zero_targets_are_the_light(world):
    o, rays, hits, lit = world
    idx = np.nonzero(lit)[0]
    p, _ = o.hit_points(rays[idx], hits[idx])
    for l in range(3):
        for s in range(3):
            t = sm.targets(p, LIGHTS[l], 0.0, 3, idx.astype(np.uint64), l, s, 0, 0x50F7)
            assert t.dtype == np.float32
            assert np.array_equal(t.view(np.uint32), np.broadcast_to(LIGHTS[l], t.shape).view(np.uint32)), (l, s)
    # and so the three rays of a (hit, light) pair are the one-sample ray
    one = sm.soft_shadow_rays(o, rays, hits, LIGHTS, np.zeros(3, np.float32), 1, bias=BIAS).view(np.uint32).reshape(N_RAYS, 3, 1, 8)
    three = sm.soft_shadow_rays(o, rays, hits, LIGHTS, np.zeros(3, np.float32), 3, seed=9, bias=BIAS).view(np.uint32).reshape(N_RAYS, 3, 3, 8)
    assert np.array_equal(three[lit], np.broadcast_to(one[lit], three[lit].shape))


# counter = (lo32 path, hi32 path, s | depth << 16, 0x53460000 | l), key = (lo32 seed, hi32 seed); (r0, r1, r2) as float32 bit patterns
PINNED = [((0, 0, 0, 0, 0), (1046774876, 1061751545, 1045932352)),
          ((63996, 2, 4, 1, 0x5AD0), (1058927786, 1051015882, 1053518774)),
          (((7 << 32) | 12345, 65535, 65535, 65535, 0xC0FFEE1234567890), (1056803478, 1051718900, 1049821070))]


@pytest.mark.parametrize("args,want", PINNED)
def test_philox_counter_layout(args, want):
    path, l, s, depth, seed = args
    got = sm.uniforms(np.array([path], np.uint64), l, s, depth, seed)
    assert tuple(int(x[0].view(np.uint32)) for x in got) == want
    # spelled out word by word, independent of sm.uniforms
    r = bm.philox4x32_10(path & 0xFFFFFFFF, path >> 32, s | (depth << 16), 0x53460000 | l, seed & 0xFFFFFFFF, seed >> 32)
    assert tuple(int(bm.u32_to_unit(r[k]).reshape(-1)[0].view(np.uint32)) for k in range(3)) == want
    assert all(0.0 <= float(x[0]) < 1.0 for x in got)
