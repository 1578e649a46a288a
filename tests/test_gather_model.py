"""The numpy model of the final gather (tests/gather_model.py) against the CPU oracle, no GPU: its open counts are the ambient-occlusion
model's, with x = 1 every sample of a lit slot is either a counted hit or an escape, the sums are additive in x, a sample does not depend
on `samples`, and metadata outside 1..N adds nothing."""
import numpy as np
import pytest

import ao_model as am
import gather_model as gm
from helpers import build_oracle
from scene_kit import distinct_x

BIAS = 1e-3
SEED = 0xA0
N_RAYS = 63_997  # the GPU tests' frame
S = 5
DISTANCES = (np.inf, 1.0)


@pytest.fixture(scope="module")
def world(oracle):
    import raycore_jl_amd as rc
    cfg = rc.scenes.config_c3(lon=16, bands=9, lattice=(3, 3, 2))
    o = build_oracle(oracle, cfg)
    rays = rc.scenes.c3_primary_rays(cfg, 320, 200)[:N_RAYS]
    hits = o.trace(rays, nthreads=16)
    lit = hits["hit"] == 1
    assert lit.sum() >= 1000 and (~lit).sum() >= 1000
    tables = {d: gm.sample_table(o, rays, hits, S, seed=SEED, bias=BIAS, max_dist=d)[:2] for d in DISTANCES}
    for t in tables.values():
        for a in t:
            a.setflags(write=False)
    return o, rays, hits, lit, tables


@pytest.mark.parametrize("max_dist", DISTANCES)
def test_open_counts_are_ambient_occlusions(world, max_dist):
    """closest-hit and any-hit agree on whether a ray of t_min = 0 hits: the escaped samples are the visible samples."""
    o, rays, hits, lit, tables = world
    meta, escaped = tables[max_dist]
    want, _ = am.expected_counts(o, rays, hits, S, seed=SEED, bias=BIAS, max_dist=max_dist)
    n = len(o.blas_prims)
    _, opened = gm.reduce(meta, escaped, np.zeros(n, np.uint32))
    assert opened.dtype == np.uint32 and np.array_equal(opened, want)
    assert 0 < opened[lit].sum() < lit.sum() * S and not opened[~lit].any()


@pytest.mark.parametrize("max_dist", DISTANCES)
def test_ones_and_open_partition_the_samples(world, max_dist):
    o, rays, hits, lit, tables = world
    meta, escaped = tables[max_dist]
    prim_meta = o.blas_prims["meta"]
    n = len(prim_meta)
    assert prim_meta.min() >= 1 and prim_meta.max() <= n  # all metadata in range: every hit is counted
    sums, opened = gm.reduce(meta, escaped, np.ones(n, np.uint32), miss_value=0)
    assert sums.dtype == np.uint64
    assert np.all(sums[lit] + opened[lit] == S)
    assert not sums[~lit].any() and not opened[~lit].any()
    # with miss_value = 1 the escapes are counted in the sums too
    sums1, _ = gm.reduce(meta, escaped, np.ones(n, np.uint32), miss_value=1)
    assert np.all(sums1[lit] == S)
    assert (sums[lit] > 0).sum() >= 100 and (opened[lit] > 0).sum() >= 100


def test_additive_in_x_and_in_the_miss_value(world):
    o, rays, hits, lit, tables = world
    meta, escaped = tables[np.inf]
    n = len(o.blas_prims)
    g = np.random.default_rng(2)
    a, b = g.integers(0, 1 << 31, n, dtype=np.uint32), g.integers(0, 1 << 31, n, dtype=np.uint32)
    sa, _ = gm.reduce(meta, escaped, a, miss_value=11)
    sb, _ = gm.reduce(meta, escaped, b, miss_value=31)
    sab, _ = gm.reduce(meta, escaped, a + b, miss_value=42)
    assert np.array_equal(sa + sb, sab) and sab.max() > 0
    top, opened = gm.reduce(meta, escaped, np.full(n, gm.U32_MAX, np.uint32), miss_value=gm.U32_MAX)
    assert np.all(top[lit] == np.uint64(S * gm.U32_MAX)) and top.max() >= 1 << 32  # the sums pass 32 bits
    # a wrong primitive shows: distinct x gives other sums than a rotation of it
    x = distinct_x(n)
    assert not np.array_equal(gm.reduce(meta, escaped, x)[0], gm.reduce(meta, escaped, np.roll(x, 1))[0])


def test_a_sample_does_not_depend_on_samples(world):
    o, rays, hits, lit, tables = world
    meta, escaped = tables[1.0]
    x = distinct_x(len(o.blas_prims))
    for k in (1, 2):
        m_k, e_k, _ = gm.sample_table(o, rays, hits, k, seed=SEED, bias=BIAS, max_dist=1.0)
        assert np.array_equal(m_k, meta[:, :k]) and np.array_equal(e_k, escaped[:, :k])
        assert all(np.array_equal(p, q) for p, q in zip(gm.reduce(m_k, e_k, x, 9), gm.reduce(meta, escaped, x, 9, samples=k)))
    # the per-sample contributions add up to the full sum
    per = [gm.reduce(meta[:, s:s + 1], escaped[:, s:s + 1], x, 9)[0] for s in range(S)]
    assert np.array_equal(np.sum(per, axis=0, dtype=np.uint64), gm.reduce(meta, escaped, x, 9)[0])


def test_metadata_outside_the_range_adds_nothing(world):
    """The rule is about len(x) = N: read with a shorter x, hits on metadata above it are dropped -- neither counted nor open."""
    o, rays, hits, lit, tables = world
    meta, escaped = tables[np.inf]
    n = len(o.blas_prims)
    half = n // 2
    s_full, open_full = gm.reduce(meta, escaped, np.ones(n, np.uint32))
    s_half, open_half = gm.reduce(meta, escaped, np.ones(half, np.uint32))
    assert np.array_equal(open_full, open_half)
    dropped = ((meta > half).sum(axis=1)).astype(np.uint64)
    assert dropped.sum() > 0 and np.array_equal(s_half + dropped, s_full)
    table = np.array([[0, n + 50, 3, -1]], np.int64)  # metadata 0 and N + 50: nothing; 3: x[2]; no hit and not escaped: nothing
    esc = np.zeros((1, 4), bool)
    x = distinct_x(n)
    assert gm.reduce(table, esc, x, miss_value=7)[0][0] == x[2] and gm.reduce(table, esc, x, miss_value=7)[1][0] == 0
