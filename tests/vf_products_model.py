"""A numpy restatement of the view-factor products and of the integer bounce iteration (rc_view_factor_products*, view_factor_bounces).

M is the oracle's view-factor matrix as a [src_meta - 1, hit_meta - 1] array (what view_factors returns).  Everything is integer
arithmetic: the products wrap modulo 2^64 like the device's u64 adds, the bounce rule saturates at 2^32 - 1."""
import numpy as np

U32_MAX = (1 << 32) - 1


def products(M, x):
    """(M @ x, M.T @ x) in uint64 arithmetic, which wraps modulo 2^64."""
    M64 = np.asarray(M).astype(np.uint64)
    x64 = np.asarray(x).astype(np.uint64)
    with np.errstate(over="ignore"):
        return M64 @ x64, M64.T @ x64


def bounces(M, R, e, rho, k):
    """x_0 = e, x_{j+1}[i] = min(2^32 - 1, e[i] + (((M x_j)[i] // R) * rho[i] >> 16)), k times; rho is 16.16 fixed point in 0..65536.
    Python integers: (M x)[i] <= R * (2^32 - 1) needs no 64-bit wrap for R < 2^31, and none is modelled."""
    rows = [[int(v) for v in row] for row in np.asarray(M)]
    e = [int(v) for v in e]
    rho = [int(v) for v in rho]
    assert all(0 <= v <= U32_MAX for v in e) and all(0 <= r <= 65536 for r in rho) and len(e) == len(rho) == len(rows)
    x = list(e)
    for _ in range(k):
        mx = [sum(m * v for m, v in zip(row, x) if m) for row in rows]
        x = [min(U32_MAX, e[i] + (((mx[i] // R) * rho[i]) >> 16)) for i in range(len(e))]
    return np.array(x, dtype=np.uint64).astype(np.uint32)
