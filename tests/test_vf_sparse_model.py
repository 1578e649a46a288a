"""The numpy model of the sparse view-factor matrix (tests/vf_sparse_model.py) against the dense model of the products
(tests/vf_products_model.py): the GPU tests compare the device with it, so its own identities are checked here, without a device."""
import numpy as np
import pytest

import vf_products_model as dense
import vf_sparse_model as model

U32_MAX = model.U32_MAX


def random_matrix(rng, n, density, top=1 << 32):
    M = rng.integers(1, top, (n, n), dtype=np.uint64).astype(np.uint32)
    M[rng.random((n, n)) >= density] = 0
    return M


def matrices():
    rng = np.random.default_rng(41)
    out = {"dense": random_matrix(rng, 17, 1.0), "half": random_matrix(rng, 33, 0.5), "thin": random_matrix(rng, 64, 0.03),
           "zero": np.zeros((5, 5), np.uint32), "one": np.array([[7]], np.uint32)}
    holes = random_matrix(rng, 40, 0.3)
    holes[[0, 7, 8, 39]] = 0  # empty rows at the front, in the middle (two in a row) and at the end
    holes[:, 3] = 0
    out["holes"] = holes
    out["top"] = np.where(random_matrix(rng, 9, 0.6) != 0, U32_MAX, 0).astype(np.uint32)
    return out


MATRICES = matrices()


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_csr_round_trip_is_canonical(name):
    M = MATRICES[name]
    n = M.shape[0]
    csr = model.csr_from_dense(M)
    row_ptr, cols, vals = csr
    assert model.is_canonical(csr, n)
    assert row_ptr.dtype == np.uint64 and cols.dtype == vals.dtype == np.uint32
    assert int(row_ptr[-1]) == len(cols) == len(vals) == np.count_nonzero(M)
    assert np.array_equal(np.diff(row_ptr.astype(np.int64)), (M != 0).sum(axis=1))
    assert np.array_equal(model.densify(csr, n), M)


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_spmv_equals_the_dense_products(name):
    M = MATRICES[name]
    n = M.shape[0]
    csr = model.csr_from_dense(M)
    rng = np.random.default_rng(42)
    for x in (rng.integers(0, 1 << 32, n, dtype=np.uint32), np.ones(n, np.uint32), np.full(n, U32_MAX, np.uint32), np.zeros(n, np.uint32)):
        mx, mtx = model.spmv(csr, x)
        w_mx, w_mtx = dense.products(M, x)
        assert mx.dtype == mtx.dtype == np.uint64
        assert np.array_equal(mx, w_mx) and np.array_equal(mtx, w_mtx)


def test_spmv_wraps_modulo_2_64():
    M = np.full((3, 3), U32_MAX, np.uint32)
    x = np.full(3, U32_MAX, np.uint32)
    mx, mtx = model.spmv(model.csr_from_dense(M), x)
    want = (3 * U32_MAX * U32_MAX) % (1 << 64)
    assert 3 * U32_MAX * U32_MAX >= 1 << 64
    assert [int(v) for v in mx] == [want] * 3 and [int(v) for v in mtx] == [want] * 3


def test_row_blocks_add_up():
    M = MATRICES["holes"]
    n = M.shape[0]
    x = np.random.default_rng(43).integers(0, 1 << 32, n, dtype=np.uint32)
    w_mx, w_mtx = dense.products(M, x)
    mx, mtx = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    parts = []
    for r0, r1 in ((0, 9), (9, 9), (9, 31), (31, n)):
        block = model.csr_from_dense(M[r0:r1])
        assert model.is_canonical(block, n) and int(block[0][0]) == 0
        a, b = model.spmv(block, x, row_offset=r0)
        assert not a[:r0].any() and not a[r1:].any()
        mx += a
        mtx += b
        parts.append(block)
    assert np.array_equal(mx, w_mx) and np.array_equal(mtx, w_mtx)
    # the blocks concatenate into the whole
    whole = model.csr_from_dense(M)
    assert np.array_equal(np.concatenate([p[1] for p in parts]), whole[1]) and np.array_equal(np.concatenate([p[2] for p in parts]), whole[2])
    ptr, base = [np.zeros(1, np.uint64)], 0
    for p in parts:
        ptr.append(p[0][1:] + np.uint64(base))
        base += int(p[0][-1])
    assert np.array_equal(np.concatenate(ptr), whole[0])


def test_is_canonical_rejects_what_is_not():
    M = MATRICES["half"]
    n = M.shape[0]
    row_ptr, cols, vals = model.csr_from_dense(M)
    assert model.is_canonical((row_ptr, cols, vals), n)
    k = int(row_ptr[3])  # the first entry of row 3, which has at least two
    assert int(row_ptr[4]) - k >= 2
    swapped = cols.copy()
    swapped[[k, k + 1]] = swapped[[k + 1, k]]
    assert not model.is_canonical((row_ptr, swapped, vals), n)
    same = cols.copy()
    same[k + 1] = same[k]
    assert not model.is_canonical((row_ptr, same, vals), n)
    zero = vals.copy()
    zero[k] = 0
    assert not model.is_canonical((row_ptr, cols, zero), n)
    assert not model.is_canonical((row_ptr + np.uint64(1), cols, vals), n)
    assert not model.is_canonical((row_ptr[:-1], cols, vals), n)
    assert not model.is_canonical((row_ptr, cols, vals), int(cols.max()))
    assert not model.is_canonical((row_ptr, cols[:-1], vals[:-1]), n)
    assert not model.is_canonical((row_ptr.astype(np.int64), cols, vals), n)
    # a column that falls from one row to the next is fine: order is per row
    two = (np.array([0, 1, 2], np.uint64), np.array([5, 2], np.uint32), np.array([1, 1], np.uint32))
    assert model.is_canonical(two, 6)
    # trailing empty rows: their row_ptr equals the number of entries
    tail = (np.array([0, 2, 2, 2], np.uint64), np.array([1, 4], np.uint32), np.array([3, 9], np.uint32))
    assert model.is_canonical(tail, 5) and np.array_equal(model.densify(tail, 5)[1:], np.zeros((2, 5), np.uint32))
