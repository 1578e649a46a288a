"""A numpy restatement of the sparse view-factor matrix (rc_view_factors_sparse*, rc_view_factor_sparse_products_device).

A CSR block is the triple (row_ptr uint64, cols uint32, vals uint32): entries row_ptr[r] .. row_ptr[r + 1] - 1 belong to row r.  It is
CANONICAL when row_ptr starts at 0, never decreases and ends at the number of entries, the columns of a row are strictly ascending and
every value is at least 1 -- then the triple is a function of the matrix alone.  The products wrap modulo 2^64 like the device's u64 adds."""
import numpy as np

U32_MAX = (1 << 32) - 1


def csr_from_dense(M):
    """The canonical CSR of a dense unsigned matrix."""
    M = np.asarray(M)
    nz = M != 0
    row_ptr = np.zeros(M.shape[0] + 1, np.uint64)
    row_ptr[1:] = np.cumsum(nz.sum(axis=1, dtype=np.uint64), dtype=np.uint64)
    r, c = np.nonzero(nz)  # row-major: rows ascending, columns ascending within a row
    return row_ptr, c.astype(np.uint32), M[r, c].astype(np.uint32)


def densify(csr, n_cols):
    """The dense uint32 matrix of a CSR block; duplicate (row, column) entries add (a canonical block has none)."""
    row_ptr, cols, vals = csr
    rows = len(row_ptr) - 1
    M = np.zeros((rows, n_cols), np.uint32)
    r = np.repeat(np.arange(rows), np.diff(row_ptr.astype(np.int64)))
    np.add.at(M, (r, cols.astype(np.int64)), vals)
    return M


def is_canonical(csr, n_cols):
    row_ptr, cols, vals = csr
    if row_ptr.dtype != np.uint64 or cols.dtype != np.uint32 or vals.dtype != np.uint32:
        return False
    if len(row_ptr) < 1 or int(row_ptr[0]) != 0 or int(row_ptr[-1]) != len(cols) or len(cols) != len(vals):
        return False
    p = row_ptr.astype(np.int64)
    if (np.diff(p) < 0).any() or (len(vals) and int(vals.min()) < 1) or (len(cols) and int(cols.max()) >= n_cols):
        return False
    ascending = np.ones(len(cols), bool)
    ascending[1:] = cols[1:] > cols[:-1]
    ascending[p[:-1][p[:-1] < len(cols)]] = True  # the first entry of a row has no predecessor
    return bool(ascending.all())


def spmv(csr, x, row_offset=0):
    """(mx, mtx), uint64 vectors of len(x): mx[row_offset + r] = sum_k vals[k] x[cols[k]], mtx[cols[k]] += vals[k] x[row_offset + r],
    modulo 2^64."""
    row_ptr, cols, vals = csr
    x64 = np.asarray(x).astype(np.uint64)
    rows = len(row_ptr) - 1
    r = np.repeat(np.arange(rows), np.diff(row_ptr.astype(np.int64)))
    mx, mtx = np.zeros(len(x64), np.uint64), np.zeros(len(x64), np.uint64)
    v64, c = vals.astype(np.uint64), cols.astype(np.int64)
    with np.errstate(over="ignore"):
        np.add.at(mx, row_offset + r, v64 * x64[c])
        np.add.at(mtx, c, v64 * x64[row_offset + r])
    return mx, mtx
