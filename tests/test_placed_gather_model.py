"""The numpy model of the placed final gather (tests/placed_gather_model.py) against what it must say on a scene small enough to read by
eye -- two instances of ONE mesh that carry different values -- and against the metadata model (tests/gather_model.py) it must reduce to
when the field is one per metadata.  CPU only: the rays are traced by the oracle."""
import numpy as np
import pytest

import gather_model as gm
import placed_gather_model as pg
import placed_vf_model as pm
from helpers import build_oracle, random_rays
from scene_kit import distinct_x, scenes_module

S, SEED, BIAS = 8, 7, 1e-3


class Rc:
    """What the scene makers read of the product module: its scene generators (pure numpy)."""
    scenes = scenes_module()


@pytest.fixture(scope="module")
def plates(oracle):
    """The two plates, P = 16, both instances with metadata 1..8, seen from z = 0.5: 16 rays straight down and 16 straight up over the
    4 x 4 grid of cell centres; (scene, rays, hits, placed table, metadata table)."""
    o = build_oracle(oracle, pm.plates_cfg(Rc))
    c = (np.arange(4) + 0.5) / 4
    org = np.array([(x, y, 0.5) for x in c for y in c])
    rays = Rc.scenes.make_rays(np.concatenate([org, org]), np.concatenate([np.tile([0.0, 0, -1], (16, 1)), np.tile([0.0, 0, 1], (16, 1))]))
    hits = o.trace(rays, nthreads=4)
    assert hits["hit"].all() and (hits["instance_id"][:16] == 0).all() and (hits["instance_id"][16:] == 1).all()
    b, escaped, gr = pg.sample_table(o, rays, hits, S, seed=SEED, bias=BIAS, nthreads=4)
    meta, escaped_m, _ = gm.sample_table(o, rays, hits, S, seed=SEED, bias=BIAS, nthreads=4)
    assert np.array_equal(escaped, escaped_m) and np.array_equal(b >= 0, meta >= 1)
    return o, rays, hits, b, escaped, meta


def test_plates_sums_name_the_placed_primitives_hit(plates):
    o, rays, hits, b, escaped, meta = plates
    assert np.array_equal(pm.bases(o), [0, 8, 16])
    on0, on1, esc = int(((b >= 0) & (b < 8)).sum()), int((b >= 8).sum()), int(escaped.sum())
    print(f"plates: {esc} samples escape, {on0} land on instance 0, {on1} on instance 1")
    assert on0 > 0 and on1 > 0 and esc > 0 and on0 + on1 + esc == 32 * S  # every primary ray hit: every sample is live
    # a plate's samples leave on its lit side: the lower plate's land on the upper one and the other way round
    assert (b[:16][b[:16] >= 0] >= 8).all() and (b[16:][b[16:] >= 0] < 8).all()
    x = (np.uint32(1) << np.arange(16, dtype=np.uint32))
    sums, opened = pg.reduce(b, escaped, x)
    assert np.array_equal(opened, escaped.sum(axis=1))
    # bit q of a slot's sum, written from the table and not through reduce(): how often each placed primitive was hit, shifted to its bit
    times = np.stack([np.bincount(row[row >= 0], minlength=16) for row in b])
    assert np.array_equal(sums, (times.astype(np.uint64) << np.arange(16, dtype=np.uint64)).sum(axis=1))
    once = times.max(axis=1) <= 1
    assert once.sum() >= 8  # where no primitive is hit twice the sum IS the set of placed primitives hit
    for i in np.nonzero(once)[0]:
        assert {q for q in range(16) if int(sums[i]) >> q & 1} == set(b[i][b[i] >= 0].tolist())
    assert np.array_equal(pg.expected(o, rays, hits, x, S, seed=SEED, bias=BIAS, nthreads=4)[0], sums)


def test_plates_no_field_per_metadata_gives_these_sums(plates):
    """Both instances carry metadata 1..8: the metadata model cannot tell the ceiling from the floor."""
    o, rays, hits, b, escaped, meta = plates
    x = (np.uint32(1) << np.arange(16, dtype=np.uint32))
    sums = pg.reduce(b, escaped, x)[0]
    g = np.random.default_rng(3)
    for x8 in (x[:8], x[8:], x[:8] | x[8:], g.integers(0, 1 << 32, 8, dtype=np.uint32), np.zeros(8, np.uint32)):
        assert not np.array_equal(gm.reduce(meta, escaped, x8)[0], sums)
    # ANY 8-word x: the metadata sums are A @ x with A[i, m - 1] = how often slot i's samples hit metadata m.  The placed sums do not lie
    # in A's column space (the least-squares residual is far above the float64 rounding of values below 2^16 * 8), so no x reproduces them
    A = np.stack([np.bincount(row[row >= 1] - 1, minlength=8) for row in meta]).astype(np.float64)
    want = sums.astype(np.float64)
    best = np.linalg.lstsq(A, want, rcond=None)[0]
    assert np.abs(A @ best - want).max() > 1.0
    # ... while the lifted field does reduce to the metadata model, word for word
    x8 = distinct_x(8, with_max=True)
    got, want = pg.reduce(b, escaped, pg.lift(o, x8), 5), gm.reduce(meta, escaped, x8, 5)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_hit_indices_of_hits_and_misses(plates):
    o, rays, hits, *_ = plates
    away = Rc.scenes.make_rays(np.array([[0.5, 0.5, 0.5], [5.0, 5.0, 0.5]]), np.array([[1.0, 0, 0], [0, 0, -1.0]]))
    both = np.concatenate([hits, o.trace(away, nthreads=1)])
    q = pg.hit_indices(o, both)
    assert q.dtype == np.uint32 and (q[-2:] == pg.INVALID).all() and (q[:16] < 8).all() and ((q[16:32] >= 8) & (q[16:32] < 16)).all()
    inst, flat = pm.placed_index(o)
    assert np.array_equal(inst[q[:32]], hits["instance_id"]) and np.array_equal(flat[q[:32]], hits["primitive_id"])


def lifted_equals_metadata(o, rays, samples, seed):
    hits = o.trace(rays, nthreads=8)
    assert 0 < hits["hit"].sum() < len(hits)
    n_prims = len(o.blas_prims)
    assert o.blas_prims["meta"].min() >= 1 and o.blas_prims["meta"].max() <= n_prims
    x = distinct_x(n_prims, salt=5, with_max=True)
    b, escaped, _ = pg.sample_table(o, rays, hits, samples, seed=seed, bias=BIAS, nthreads=8)
    meta, escaped_m, _ = gm.sample_table(o, rays, hits, samples, seed=seed, bias=BIAS, nthreads=8)
    assert (b >= 0).sum() >= 100 and escaped.sum() >= 100 and np.array_equal(escaped, escaped_m)
    assert len(np.unique(pm.placed_index(o)[0][b[b >= 0]])) >= 2  # samples land on more than one instance
    for miss in (0, pg.U32_MAX):
        got, want = pg.reduce(b, escaped, pg.lift(o, x), miss), gm.reduce(meta, escaped, x, miss)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[0].max() >= 1 << 32


def test_lift_reduces_to_the_metadata_model_on_the_mixed_scene(oracle):
    o = build_oracle(oracle, pm.mixed_cfg(Rc))
    lifted_equals_metadata(o, random_rays(Rc, 1024, 11, -2.9, 2.9), 4, 3)


def test_lift_reduces_to_the_metadata_model_on_c3(oracle):
    cfg = Rc.scenes.config_c3(lon=16, bands=9, lattice=(7, 7, 6))  # (the dense lattice: samples reach the neighbouring spheres)
    o = build_oracle(oracle, cfg)
    assert len(o.blas_prims) == 256 and pm.bases(o)[-1] == 294 * 256  # one BLAS under 294 instances: every x word is read through many instances
    lifted_equals_metadata(o, Rc.scenes.c3_primary_rays(cfg, 160, 100), 5, 0xA0)
