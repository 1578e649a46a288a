"""The numpy model of the point-source illumination (tests/point_source_model.py), no GPU: the stratification of its uniforms, both
mappings at u = 1, the unit length and the equal-area strata of the isotropic directions, the hemisphere of the Lambertian ones, what
first_source does, and a furnace on the CPU oracle -- a lamp inside a closed sphere loses no ray."""
import numpy as np
import pytest

import bounce_model as bm
import point_source_model as pm
from helpers import build_oracle
from scene_kit import single_cfg

F32 = np.float32
GRIDS = (13, 24, 64)
SEED = 5
AXIS = (0.3, 0.2, 1.0)
LAMP = (0.25, -0.05, 0.2)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("key", [0, 3, 0xFFFFFFFF])
def test_every_cell_holds_its_sample(grid, key):
    """(u1, u2) of cell (a, b) lies in [a/G, (a+1)/G] x [b/G, (b+1)/G]: the bounds are the f32 quotients the definition itself forms."""
    u1, u2 = pm.stratified_uniforms(grid, key, SEED)
    assert u1.dtype == F32 and u2.dtype == F32 and len(u1) == grid * grid
    cell = np.arange(grid * grid)
    a, b = (cell // grid).astype(F32), (cell % grid).astype(F32)
    g = F32(grid)
    assert (u1 >= a / g).all() and (u1 <= (a + F32(1)) / g).all()
    assert (u2 >= b / g).all() and (u2 <= (b + F32(1)) / g).all()
    assert u1.min() >= 0 and u1.max() <= 1 and u2.min() >= 0 and u2.max() <= 1
    # jittered, not the cell centres, and the two coordinates are different draws
    assert len(np.unique(u1 * g - a)) > grid * grid // 2 and not np.array_equal(u1 * g - a, u2 * g - b)


def test_u_equal_to_one_is_handled_in_both_mappings():
    one, half = np.array([1.0], F32), np.array([0.5], F32)
    d = pm.isotropic_dir(one, half)
    assert d.shape == (1, 3) and d[0, 0] == 0 and d[0, 1] == 0 and d[0, 2] == -1  # u1 = 1: the south pole, (0, 0, -1)
    # u2 = 1: phi = 2 * Float32(pi) lies a rounding above 2 pi; sincos_f64's reduction takes it (k = 4, |r| < 1e-6)
    phi = (F32(2) * bm.PI_F32) * F32(1)
    s, c = bm.sincos_f64(np.array([phi], np.float64))
    assert abs(s[0] - np.sin(np.float64(phi))) < 1e-15 and abs(c[0] - np.cos(np.float64(phi))) < 1e-15
    d = pm.isotropic_dir(half, one)
    assert np.isfinite(d).all() and abs(np.linalg.norm(d.astype(np.float64)) - 1) < 1e-6 and d[0, 0] > 0.999
    # the Lambertian mapping: the concentric disk at its corner and on its rim
    for u1, u2 in ((1.0, 1.0), (1.0, 0.5), (0.5, 1.0), (1.0, 0.0), (0.0, 1.0)):
        d = pm.lambertian_dir(AXIS, np.array([u1], F32), np.array([u2], F32))
        assert np.isfinite(d).all() and abs(np.linalg.norm(d.astype(np.float64)) - 1) < 1e-6, (u1, u2, d)


@pytest.mark.parametrize("grid", GRIDS)
def test_isotropic_directions_are_unit_and_equal_area(grid):
    u1, u2 = pm.stratified_uniforms(grid, 0, SEED)
    d = pm.isotropic_dir(u1, u2).astype(np.float64)
    dev = np.abs(np.linalg.norm(d, axis=1) - 1).max()
    print(f"grid {grid}: largest deviation from unit length {dev:.3g}")
    assert dev < 1e-6
    # z = 1 - 2 u1 is uniform in area: each of the G strata in z holds exactly G rays (stratum a: 1 - 2 (a + 1) / G <= z <= 1 - 2 a / G)
    strata = np.clip(np.floor((1.0 - d[:, 2]) * 0.5 * grid).astype(np.int64), 0, grid - 1)
    strata_by_cell = np.arange(grid * grid) // grid
    edge = np.abs((1.0 - d[:, 2]) * 0.5 * grid - np.round((1.0 - d[:, 2]) * 0.5 * grid)) < 1e-4  # (a sample on a stratum's edge may round either way)
    assert np.array_equal(strata[~edge], strata_by_cell[~edge])
    assert np.array_equal(np.bincount(strata_by_cell, minlength=grid), np.full(grid, grid))
    assert (np.abs(np.bincount(strata, minlength=grid) - grid) <= edge.sum()).all()
    # ... and in azimuth: cell (a, b) lies in sector b of G
    az = np.mod(np.arctan2(d[:, 1], d[:, 0]), 2 * np.pi) / (2 * np.pi) * grid
    near = np.abs(az - np.round(az)) < 1e-3
    assert np.array_equal(np.floor(az[~near]).astype(np.int64), (np.arange(grid * grid) % grid)[~near])


@pytest.mark.parametrize("grid", GRIDS)
def test_lambertian_directions_fill_the_hemisphere_about_the_axis(grid):
    u1, u2 = pm.stratified_uniforms(grid, 1, SEED)
    d = pm.lambertian_dir(AXIS, u1, u2).astype(np.float64)
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-6
    n = np.asarray(AXIS, np.float64) / np.linalg.norm(AXIS)
    cos = d @ n
    assert cos.min() >= -1e-6
    assert abs(cos.mean() - 2.0 / 3.0) < 0.5 / grid  # cosine-weighted: E[cos] = 2/3 (stratified: the error falls like 1/G^2)


def test_first_source_offsets_the_key_only():
    src = pm.make_sources([LAMP, (0, 0, 0), LAMP], [(0, 0, 0), AXIS, (0, 0, 0)])
    whole = pm.point_source_rays(src, 13, SEED)
    tail = pm.point_source_rays(src[1:], 13, SEED, first_source=1)
    assert whole[169:].tobytes() == tail.tobytes()
    assert pm.point_source_rays(src[1:], 13, SEED)[:169].tobytes() != tail[:169].tobytes()
    # the same lamp under another key draws other samples; another seed likewise
    assert whole[:169].tobytes() != whole[338:].tobytes()
    assert pm.point_source_rays(src[:1], 13, SEED + 1).tobytes() != whole[:169].tobytes()
    # position, t_min and t_max are copied
    s2 = pm.make_sources([LAMP], None, t_min=0.125, t_max=0.75)
    r = pm.point_source_rays(s2, 13, SEED)
    assert (r["o"] == np.asarray(LAMP, F32)).all() and (r["tmin"] == F32(0.125)).all() and (r["tmax"] == F32(0.75)).all()
    assert np.array_equal(r["d"], whole[:169]["d"])
    # a negative zero axis is isotropic too
    s3 = pm.make_sources([LAMP], [(-0.0, 0.0, -0.0)])
    assert pm.point_source_rays(s3, 13, SEED).tobytes() == whole[:169].tobytes()


@pytest.mark.parametrize("grid", GRIDS)
def test_furnace_on_the_oracle(oracle, grid):
    """A lamp inside a closed sphere: all grid^2 rays of either kind hit, none escapes, none is dropped."""
    import raycore_jl_amd as rc
    o = build_oracle(oracle, single_cfg(rc))
    src = pm.make_sources([LAMP, LAMP], [(0, 0, 0), AXIS])
    counts, escaped, dropped = pm.expected_counts(o, src, grid, SEED)
    assert counts.shape == (2, len(o.blas_prims)) and counts.dtype == np.uint32
    assert not escaped.any() and not dropped.any()
    assert (counts.sum(axis=1) == grid * grid).all()
    assert not np.array_equal(counts[0], counts[1])
    # the Lambertian lamp lights only what lies in front of it
    tri = o.blas_prims["v"].astype(np.float64).mean(axis=1)
    behind = (tri - np.asarray(LAMP)) @ np.asarray(AXIS) < -0.25
    assert behind.any() and not counts[1][o.blas_prims["meta"][behind] - 1].any() and counts[0][o.blas_prims["meta"][behind] - 1].any()
