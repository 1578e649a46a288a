"""The numpy model of the placed products (tests/placed_products_model.py) against the matrix it must be the product of, against the
ray budget of every source, and against the analytic form factor of two opposed plates.  CPU only: the rays are traced by the oracle."""
import numpy as np
import pytest

import placed_products_model as model
import placed_vf_model as placed
import vf_groups_model as sibling
from helpers import build_oracle
from scene_kit import full_range_x, scenes_module

PLATES_RAYS, PLATES_SEED = 4096, 5  # the job of tests/test_placed_vf_model.py's plates
SIGMA = np.sqrt(0.2 * 0.8 / 32768)  # the binomial error of a form factor of 0.2 from 8 x 4096 rays, as derived there


class Rc:
    """What the scene makers of the model read of the product module: its scene generators (pure numpy)."""
    scenes = scenes_module()


@pytest.fixture(scope="module")
def plates(oracle):
    return build_oracle(oracle, placed.plates_cfg(Rc))


@pytest.mark.parametrize("sampling", placed.SAMPLINGS)
def test_products_are_the_matrix_times_x(plates, sampling):
    R = 96
    traced = placed.Traced(plates, R, 7, sampling)
    assert traced.n == 16
    Mp, escapes = model.matrix(traced)
    assert Mp.shape == (16, 16) and Mp.any() and not np.diag(Mp).any()
    for x in (full_range_x(16, 1), np.full(16, model.U32_MAX, np.uint32), np.ones(16, np.uint32)):
        mx, mtx, escaped, _ = model.products(traced, x)
        x64 = x.astype(np.uint64)
        with np.errstate(over="ignore"):
            assert np.array_equal(mx, Mp @ x64) and np.array_equal(mtx, Mp.T @ x64)
        assert mx.dtype == mtx.dtype == escaped.dtype == np.uint64 and np.array_equal(escaped, escapes)
    assert (model.products(traced, np.full(16, model.U32_MAX, np.uint32))[0] > model.U32_MAX).any()  # the sums carry past 32 bits
    # x = None is x = 1, and every ray of a source is a counted hit, an escape or a hit on the source itself
    ones = model.products(traced, np.ones(16, np.uint32))
    none = model.products(traced, None)
    for got, want in zip(none, ones):
        assert np.array_equal(got, want)
    mx, mtx, escaped, self_hits = none
    assert np.array_equal(mx + escaped + self_hits, np.full(16, R, np.uint64))
    assert np.array_equal(mx, Mp.sum(axis=1, dtype=np.uint64)) and np.array_equal(mtx, Mp.sum(axis=0, dtype=np.uint64))
    assert int(mx.sum()) == int(mtx.sum()) and escaped.any()


def test_the_lower_plates_form_factor(plates):
    traced = placed.Traced(plates, PLATES_RAYS, PLATES_SEED, "cosine")
    mx, mtx, escaped, self_hits = model.products(traced, None)
    F = float(mx[:8].sum()) / (8 * PLATES_RAYS)  # the lower plate looks up: every counted hit of its rays is on the upper plate
    print("plates: sum(mx[lower]) / (8 R) = %.6f, analytic %.6f, 4 sigma = %.6f" % (F, sibling.F_OPPOSITE, 4 * SIGMA))
    assert abs(F - sibling.F_OPPOSITE) <= 4 * SIGMA
    assert int(mx[:8].sum()) == int(mtx[8:].sum()) and not self_hits.any()
    assert np.array_equal(mx + escaped, np.full(16, PLATES_RAYS, np.uint64))


def test_bounces_in_python_integers(plates):
    R = 96
    Mp, _ = model.matrix(placed.Traced(plates, R, 7, "cosine"))
    e = np.arange(16, dtype=np.uint32) * 1000 + 5
    rho = np.full(16, 32768, np.uint32)
    assert np.array_equal(model.bounces(Mp, R, e, rho, 0), e)
    one = model.bounces(Mp, R, e, rho, 1)
    want = e.astype(np.uint64) + ((((Mp @ e.astype(np.uint64)) // np.uint64(R)) * np.uint64(32768)) >> np.uint64(16))
    assert np.array_equal(one, want.astype(np.uint32)) and (one != e).any()
    top = e.copy()
    top[3] = model.U32_MAX - 1
    rho1 = np.full(16, 65536, np.uint32)
    assert Mp[3].any() and model.bounces(Mp, R, top, rho1, 2)[3] == model.U32_MAX  # saturates
