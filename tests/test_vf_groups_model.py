"""CPU checks of the grouped, sampled view-factor job through its numpy model (tests/vf_groups_model.py) and the oracle:

1. the model's ray: uniform = the oracle's view_factor_ray bit for bit; cosine = the same origins, directions in the normal's hemisphere;
2. the model's trace-and-count path against the oracle's matrix: uniform sampling gives P diag(w) M P^T exactly;
3. the analytic cube: cosine sampling gives the form factors between the walls of the unit cube, uniform sampling does not;
4. form_factor_weights and the float arithmetic of form_factors on the model's integers.

Integer comparisons are np.array_equal."""
import numpy as np
import pytest

import vf_groups_model as model
from api_kit import rc  # noqa: F401
from helpers import build_oracle
from scene_kit import room_cfg


@pytest.fixture(scope="module")
def room(rc, oracle):
    return build_oracle(oracle, room_cfg(rc))


def cube_cfg(rc):
    verts = rc.scenes.box_room((0, 0, 0), (1, 1, 1), 2)
    return {"blas": [(verts, np.arange(1, len(verts) + 1, dtype=np.uint32))], "instances": [(1, rc.scenes.IDENTITY3x4[None], np.zeros(1, np.uint32))]}


CUBE_R, CUBE_SEED = 4096, 5
SIGMA = np.sqrt(0.2 * 0.8 / 32768)  # the binomial error of a wall's 8 x 4096 rays at p = 0.2


@pytest.fixture(scope="module")
def cube_counts(rc, oracle):
    """(cosine matrix, cosine escaped, uniform matrix) of the unit cube's walls, R = 4096, seed 5: traced once, read-only."""
    o = build_oracle(oracle, cube_cfg(rc))
    assert len(o.blas_prims) == 48
    groups = model.wall_groups(0, 2)
    out = []
    for sampling in ("cosine", "uniform"):
        m, esc, unc = model.Traced(o, CUBE_R, CUBE_SEED, sampling).count(groups, 6)
        assert not esc.any() and int(m.sum(dtype=np.uint64)) + int(unc.sum(dtype=np.uint64)) == 48 * CUBE_R
        m.setflags(write=False)
        out.append(m)
    return out[0], out[1]


# ---- 1. the ray model ------------------------------------------------------------------------------------------------------------------
def test_uniform_rays_are_the_oracles(room):
    prims = room.blas_prims
    idx = np.array([0, 1, 2, 63, 64, 191, 4095, 100000], np.uint64)
    for src in (0, 1, 77, 143, 144, 191):
        for seed in (0, 77, (1 << 63) + 12345):
            got = model.sampled_rays(prims, src, idx, seed, "uniform")
            want = np.array([room.view_factor_ray(src, int(i), seed) for i in idx])
            assert got.tobytes() == want.tobytes(), (src, seed)


def test_cosine_rays_share_the_origins_and_stay_in_the_hemisphere(room):
    prims = room.blas_prims
    idx = np.arange(0, 512, dtype=np.uint64)
    for src in (0, 1, 77, 143, 144, 191):
        uni, cos = model.sampled_rays(prims, src, idx, 77, "uniform"), model.sampled_rays(prims, src, idx, 77, "cosine")
        for f in ("o", "tmin", "tmax"):
            assert cos[f].tobytes() == uni[f].tobytes(), (src, f)
        assert (cos["tmin"] == 0).all() and np.isinf(cos["tmax"]).all()
        assert cos["d"].tobytes() != uni["d"].tobytes()
        tri = prims["v"][src]
        normal = model.bm.normalize3(model.bm.cross3(tri[1] - tri[0], tri[2] - tri[0]))
        dots = model.bm.dot3(cos["d"], np.broadcast_to(normal, cos["d"].shape))
        assert (dots >= 0).all(), (src, float(dots.min()))
        lengths = np.linalg.norm(cos["d"].astype(np.float64), axis=1)
        assert np.abs(lengths - 1).max() < 1e-6  # (not renormalised: unit up to float32 rounding)
        # cosine-weighted: the mean of cos(theta) is 2/3 (uniform: 1/2); 512 samples, sd of cos(theta) = sqrt(1/18), 6 sd
        assert abs(float(dots.mean()) - 2 / 3) < 6 * np.sqrt(1 / 18 / 512)


# ---- 2. the model's grouped matrix against the oracle's matrix -------------------------------------------------------------------------
def test_uniform_counts_are_the_grouped_reference_matrix(room):
    n, R, seed = 192, 192, 77
    M = room.view_factors(R, seed=seed, nthreads=8)
    traced = model.Traced(room, R, seed, "uniform")
    rng = np.random.default_rng(1)
    walls = model.wall_groups(144, 2)
    excluded = walls.copy()
    excluded[walls == 3] = model.U32_MAX   # one wall left out, as source and as target
    weights = rng.integers(0, 1 << 32, n, dtype=np.uint32)
    weights[:3] = (model.U32_MAX, 0, 1)
    for what, groups, G in (("identity", np.arange(n, dtype=np.uint32), n), ("walls + sphere", walls, 7), ("one group", np.zeros(n, np.uint32), 1),
                            ("an excluded group", excluded, 7)):
        for w in (None, weights):
            matrix, esc, unc = traced.count(groups, G, w)
            assert matrix.dtype == np.uint64 and matrix.shape == (G, G)
            assert np.array_equal(matrix, model.grouped_from_matrix(M, groups, G, w)), what
            assert not esc.any(), what  # the room is closed
            ww = np.ones(n, np.uint64) if w is None else w.astype(np.uint64)
            per_group = np.array([int(ww[groups == g].sum(dtype=np.uint64)) for g in range(G)], dtype=object) * R
            rows = np.array([sum(int(v) for v in row) for row in matrix], dtype=object) + np.array([int(v) for v in unc], dtype=object)
            assert (rows == per_group).all(), what
            if what != "an excluded group":
                assert not unc.any(), what  # every ray of the closed room is counted: rows sum to R * sum(w)
    ident, _, _ = traced.count(np.arange(n, dtype=np.uint32), n)
    assert np.array_equal(ident, np.asarray(M).astype(np.uint64))
    seven, _, _ = traced.count(walls, 7)
    assert seven[6, 6] == 0 and (seven[6, :6] > 0).all() and (seven[:6, 6] > 0).all()  # a convex sphere never sees itself


# ---- 3. the analytic cube ----------------------------------------------------------------------------------------------------------------
def wall_pairs():
    return [(a, b, "opposite" if a // 2 == b // 2 else "adjacent") for a in range(6) for b in range(6) if a != b]


def test_cosine_sampling_gives_the_cubes_form_factors(cube_counts):
    cosine, uniform = cube_counts
    F = cosine.astype(np.float64) / (8 * CUBE_R)
    assert not np.diag(cosine).any()  # a flat wall never sees itself
    worst = {"opposite": 0.0, "adjacent": 0.0}
    for a, b, kind in wall_pairs():
        want = model.F_OPPOSITE if kind == "opposite" else model.F_ADJACENT
        worst[kind] = max(worst[kind], abs(F[a, b] - want) / SIGMA)
    print(f"cosine: worst opposite {worst['opposite']:.2f} sigma, worst adjacent {worst['adjacent']:.2f} sigma; rows sum to {F.sum(axis=1)}")
    assert worst["opposite"] <= 4 and worst["adjacent"] <= 4
    assert (cosine.sum(axis=1) == 8 * CUBE_R).all()  # closed, and no ray lands on its own wall
    # the sampling parameter is observable: the reference's uniform rays miss the opposite-wall value by far
    U = uniform.astype(np.float64) / (8 * CUBE_R)
    off = min(abs(U[a, b] - model.F_OPPOSITE) / SIGMA for a, b, kind in wall_pairs() if kind == "opposite")
    print(f"uniform: opposite walls {sorted(set(np.round([U[a, b] for a, b, k in wall_pairs() if k == 'opposite'], 4)))}, at least {off:.1f} sigma off")
    assert off > 10


# ---- 4. form_factor_weights and form_factors' arithmetic -----------------------------------------------------------------------------------
def test_form_factor_weights(rc):
    rng = np.random.default_rng(2)
    for areas, R in ((rng.random(1000) + 0.01, 10000), (np.array([1e-9, 3.0, 0.0, 2.5e6]), 1), (np.full(48, 0.125), 4096),
                     (rng.random(200000) * 1e-3, (1 << 32) - 1), (np.array([7.0]), 123)):
        w = rc.form_factor_weights(areas, R)
        assert w.dtype == np.uint32 and w.shape == areas.shape
        total = sum(int(v) for v in w)
        assert R * total < 1 << 63 and int(w.max()) <= (1 << 32) - 1
        # the scale is the largest: one of the two bounds is reached to within the floor's step per entry and float rounding
        s = int(w.max()) / areas.max()
        assert int(w.max()) >= (1 << 32) - 2 or R * (total + len(w) + 1) * (1 + 2.0 ** -40) >= 1 << 63
        # proportional within one step
        assert (np.abs(w.astype(np.float64) - areas * s) <= 1 + areas * s * 2.0 ** -40).all()
        assert (w[areas == 0] == 0).all()
    for bad in (np.array([1.0, -1.0]), np.array([np.nan]), np.zeros(3), np.ones((2, 2)), np.array([np.inf, 1.0])):
        with pytest.raises(ValueError, match="areas"):
            rc.form_factor_weights(bad, 10)
    for bad in (0, -1, 1 << 32, 2.5, True):
        with pytest.raises(ValueError, match="rays_per_triangle"):
            rc.form_factor_weights(np.ones(3), bad)


def test_form_factors_arithmetic_reproduces_the_cube(rc, oracle, cube_counts):
    """Equal areas: every weight is 2^32 - 1, the integers are the unweighted ones times that, and the quotients are test 3's."""
    cosine, _ = cube_counts
    groups = model.wall_groups(0, 2)
    w = rc.form_factor_weights(np.full(48, 0.125), CUBE_R)
    assert (w == model.U32_MAX).all()
    o = build_oracle(oracle, cube_cfg(rc))
    matrix, esc, _ = model.Traced(o, CUBE_R, CUBE_SEED, "cosine").count(groups, 6, w)
    assert np.array_equal(matrix, cosine * np.uint64(model.U32_MAX))
    F, E = rc.form_factors_from_counts(matrix, esc, groups, w, CUBE_R)
    assert F.dtype == np.float64 and F.shape == (6, 6) and E.shape == (6,) and not E.any()
    assert np.abs(F - cosine.astype(np.float64) / (8 * CUBE_R)).max() < 1e-15
    for a, b, kind in wall_pairs():
        assert abs(F[a, b] - (model.F_OPPOSITE if kind == "opposite" else model.F_ADJACENT)) <= 4 * SIGMA
    # a group without weight gives zeros, not a division by zero
    F2, E2 = rc.form_factors_from_counts(np.zeros((2, 2), np.uint64), np.zeros(2, np.uint64), np.zeros(48, np.uint32), w, CUBE_R)
    assert not F2.any() and not E2.any()
