"""A numpy restatement of the placed products and of the integer bounce iteration over placed primitives
(rc_placed_view_factor_products_device, placed_view_factor_bounces; include/raycore_mi355x.h, "Radiosity between instances").

The items (a, hit, b) come from tests/placed_vf_model.py's Traced, which shoots the model's placed rays through the ORACLE.  The rule is
applied here in u64 that wraps modulo 2^64 like the device's adds: a hit with b != a adds x[b] to mx[a] and x[a] to mtx[b], a miss adds 1
to escaped[a], a hit on the source itself adds nothing.  No metadata takes part.  The bounce iteration is restated in Python integers."""
import numpy as np

U32_MAX = (1 << 32) - 1


def products(traced, x=None):
    """(mx, mtx, escaped, self_hits) of a Traced job, uint64 of length P.  x: P u32, or None for x = 1."""
    n = traced.n
    a, hit, b = traced.a, traced.hit, traced.b
    x64 = np.ones(n, np.uint64) if x is None else np.asarray(x).astype(np.uint64)
    assert len(x64) == n
    counted = hit & (b != a)
    mx, mtx, escaped, self_hits = (np.zeros(n, np.uint64) for _ in range(4))
    with np.errstate(over="ignore"):
        np.add.at(mx, a[counted], x64[b[counted]])
        np.add.at(mtx, b[counted], x64[a[counted]])
    np.add.at(escaped, a[~hit], np.uint64(1))
    np.add.at(self_hits, a[hit & (b == a)], np.uint64(1))
    return mx, mtx, escaped, self_hits


def matrix(traced):
    """Mp (P, P) uint64: Mp[a, b] = the rays of placed primitive a that hit placed primitive b != a -- Traced.count with every placed
    primitive its own group -- and the escapes (P,)."""
    Mp, escaped, _ = traced.count(np.arange(traced.n, dtype=np.uint32), traced.n)
    return Mp, escaped


def bounces(Mp, R, e, rho, k):
    """x_0 = e, x_{j+1}[q] = min(2^32 - 1, e[q] + (((Mp x_j)[q] // R) * rho[q] >> 16)), k times, in Python integers; rho is 16.16 fixed
    point in 0..65536.  (Mp x)[q] <= R * (2^32 - 1) needs no 64-bit wrap for R < 2^31, and none is modelled."""
    rows = [[(j, int(v)) for j, v in enumerate(row) if v] for row in np.asarray(Mp)]
    e = [int(v) for v in e]
    rho = [int(v) for v in rho]
    assert all(0 <= v <= U32_MAX for v in e) and all(0 <= r <= 65536 for r in rho) and len(e) == len(rho) == len(rows)
    x = list(e)
    for _ in range(k):
        mx = [sum(m * x[j] for j, m in row) for row in rows]
        x = [min(U32_MAX, e[q] + (((mx[q] // R) * rho[q]) >> 16)) for q in range(len(e))]
    return np.array(x, dtype=np.uint64).astype(np.uint32)
