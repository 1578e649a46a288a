"""The numpy model of the view-factor products and of the integer bounce iteration (tests/vf_products_model.py), held against the
oracle's matrix of the room scene: the model is what the GPU tests compare the device with, so its own identities are checked here,
without a device."""
import numpy as np
import pytest

import vf_products_model as model
from helpers import build_oracle
from scene_kit import room_cfg

R, SEED = 192, 77
U32_MAX = model.U32_MAX


@pytest.fixture(scope="module")
def M(oracle):
    import raycore_jl_amd as rc
    m = build_oracle(oracle, room_cfg(rc)).view_factors(R, seed=SEED, nthreads=8)
    m.setflags(write=False)
    return m


def test_room_is_closed_and_hot(M):
    """What the GPU tests rely on: N = 192, every ray is counted, and one column takes far more than its share."""
    n = M.shape[0]
    assert M.shape == (192, 192) and M.dtype == np.uint32
    assert (M.sum(axis=1, dtype=np.uint64) == R).all()
    assert int(M.sum(axis=0, dtype=np.uint64).max()) == 1018 and R * n == 36864


def test_products_of_ones_are_the_row_and_column_sums(M):
    mx, mtx = model.products(M, np.ones(M.shape[0], np.uint32))
    assert mx.dtype == mtx.dtype == np.uint64
    assert np.array_equal(mx, M.sum(axis=1, dtype=np.uint64)) and np.array_equal(mtx, M.sum(axis=0, dtype=np.uint64))


def test_products_are_linear_and_wrap(M):
    rng = np.random.default_rng(5)
    n = M.shape[0]
    x, y = rng.integers(0, 1 << 31, n, dtype=np.uint32), rng.integers(0, 1 << 31, n, dtype=np.uint32)
    for a, b, ab in zip(model.products(M, x), model.products(M, y), model.products(M, x + y)):
        assert np.array_equal(a + b, ab)
    mx3, _ = model.products(M, (3 * (x >> 2)).astype(np.uint32))
    assert np.array_equal(mx3, 3 * model.products(M, x >> 2)[0])
    # against Python integers, and modulo 2^64 where a sum passes it
    full = rng.integers(0, 1 << 32, n, dtype=np.uint32)
    mx, mtx = model.products(M, full)
    assert [int(v) for v in mx] == [sum(int(m) * int(v) for m, v in zip(row, full)) for row in M]
    assert [int(v) for v in mtx] == [sum(int(m) * int(v) for m, v in zip(col, full)) for col in M.T]
    big = np.full((2, 2), U32_MAX, np.uint32)
    want = (2 * U32_MAX * U32_MAX) % (1 << 64)
    assert [int(v) for v in model.products(big * np.uint64(1 << 31), np.full(2, U32_MAX, np.uint32))[0]] == [(want << 31) % (1 << 64)] * 2


def test_bounces_without_reflectance_return_the_emission(M):
    rng = np.random.default_rng(6)
    n = M.shape[0]
    e = rng.integers(0, 1 << 32, n, dtype=np.uint32)
    for k in (0, 1, 4):
        assert np.array_equal(model.bounces(M, R, e, np.zeros(n, np.uint32), k), e)
    assert np.array_equal(model.bounces(M, R, e, np.full(n, 65536, np.uint32), 0), e)


def test_bounces_are_monotone_in_k(M):
    rng = np.random.default_rng(7)
    n = M.shape[0]
    e = rng.integers(0, 1 << 20, n, dtype=np.uint32)
    rho = rng.integers(0, 65537, n, dtype=np.uint32)
    xs = [model.bounces(M, R, e, rho, k) for k in range(5)]
    for a, b in zip(xs, xs[1:]):
        assert (b >= a).all()
    assert (xs[4] > xs[0]).any()
    # one step by hand
    mx = model.products(M, e)[0]
    assert np.array_equal(xs[1], e + ((mx // np.uint64(R)) * rho.astype(np.uint64) >> np.uint64(16)).astype(np.uint32))


def test_bounces_saturate(M):
    n = M.shape[0]
    e = np.full(n, U32_MAX - 5, np.uint32)
    x = model.bounces(M, R, e, np.full(n, 65536, np.uint32), 3)
    assert (x == U32_MAX).all()
    e[1:] = 0
    x = model.bounces(M, R, e, np.full(n, 65536, np.uint32), 2)
    assert x[0] >= U32_MAX - 5 and x.max() <= U32_MAX and (x[1:] < U32_MAX).all()
