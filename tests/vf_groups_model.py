"""A numpy restatement of the sampled view-factor ray and of the grouped counting rule (rc_view_factor_sampled_rays_device,
rc_view_factor_groups_device, include/raycore_mi355x.h).

The ray composes tests/bounce_model.py: view_factor_ray (the reference's uniform ray, checked against the oracle's own), philox4x32_10,
u32_to_unit and cosine_hemisphere.  The rays are traced by the ORACLE (Scene.trace); the counting rule is applied here, in integers that
wrap modulo 2^64 like the device's u64 adds.  `prims` is the oracle's flat primitive array (Scene.blas_prims): a hit's primitive_id
indexes it."""
import numpy as np

import bounce_model as bm

F32 = np.float32
U32_MAX = (1 << 32) - 1
SAMPLINGS = ("uniform", "cosine")


def sampled_rays(prims, src, ray_idx, seed=0, sampling="uniform"):
    """The rays of flat source primitive `src` for the ray indices `ray_idx`.  Both samplings share the Philox draw -- counter (ray_idx,
    src, 0, 0), key = seed -> r1, r2, xi1, xi2 -- and the origin; "cosine" replaces the direction by the bounce stage's cosine-weighted
    one about the triangle's unit normal from (xi1, xi2), not renormalised."""
    assert sampling in SAMPLINGS
    ray_idx = np.asarray(ray_idx, np.uint64)
    out = bm.view_factor_ray(prims, src, ray_idx, seed)
    if sampling == "uniform":
        return out
    tri = prims["v"][src].astype(F32)
    normal = bm.normalize3(bm.cross3(tri[1] - tri[0], tri[2] - tri[0]))
    r = bm.philox4x32_10(ray_idx, np.uint64(src), 0, 0, int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    d, _ = bm.cosine_hemisphere(np.ascontiguousarray(np.broadcast_to(normal, (len(ray_idx), 3))), bm.u32_to_unit(r[2]), bm.u32_to_unit(r[3]))
    out["d"] = d
    return out


def all_rays(prims, rays_per_triangle, seed, sampling, src=None, rays=None):
    """The rays of the work items of one job in the device's order: item w = source src[0] + w // n_ray, ray rays[0] + w % n_ray."""
    s0, s1 = (0, len(prims)) if src is None else src
    r0, r1 = (0, rays_per_triangle) if rays is None else rays
    idx = np.arange(r0, r1, dtype=np.uint64)
    parts = [sampled_rays(prims, s, idx, seed, sampling) for s in range(s0, s1)]
    return np.concatenate(parts) if parts else np.zeros(0, bm.RAY_DT), np.repeat(np.arange(s0, s1, dtype=np.int64), len(idx))


class Traced:
    """One job's rays traced by the oracle, once: per work item the source's metadata `a`, whether it hit, and the hit's metadata `b`
    (0 on a miss).  count() applies the rule to them for any grouping."""

    def __init__(self, scene, rays_per_triangle, seed, sampling, src=None, rays=None, nthreads=8):
        prims = scene.blas_prims
        self.n = len(prims)
        r, source = all_rays(prims, rays_per_triangle, seed, sampling, src, rays)
        hits = scene.trace(r, nthreads=nthreads)
        self.hit = hits["hit"] == 1
        self.a = prims["meta"][source].astype(np.int64)
        self.b = np.zeros(len(r), np.int64)
        self.b[self.hit] = prims["meta"][hits["primitive_id"][self.hit]]

    def count(self, groups, n_groups, weights=None, escaped=True):
        return count(self.a, self.hit, self.b, self.n, groups, n_groups, weights, escaped)


def count(a, hit, b, n, groups, n_groups, weights=None, escaped=True):
    """The rule of rc_view_factor_groups_device on traced items: (matrix (G, G) u64, escaped (G,) u64, uncounted (G,) u64).  `uncounted`
    is the weight of a group's rays that add nothing although their source counts: hits on the source's own metadata, on metadata outside
    1..N or on an excluded group -- and the misses when escaped is False."""
    G = int(n_groups)
    groups = np.asarray(groups, np.int64)
    assert len(groups) == n and 1 <= G <= 65535
    w = np.ones(n, np.uint64) if weights is None else np.asarray(weights).astype(np.uint64)
    src_ok = (a >= 1) & (a <= n)
    ga = np.where(src_ok, groups[np.clip(a - 1, 0, n - 1)], G)
    src_ok &= ga < G
    wa = np.where(src_ok, w[np.clip(a - 1, 0, n - 1)], 0).astype(np.uint64)
    hit_ok = hit & (b >= 1) & (b <= n) & (b != a)
    gb = np.where(hit_ok, groups[np.clip(b - 1, 0, n - 1)], G)
    hit_ok &= gb < G
    matrix, esc, unc = np.zeros(G * G, np.uint64), np.zeros(G, np.uint64), np.zeros(G, np.uint64)
    with np.errstate(over="ignore"):
        m = src_ok & hit_ok
        np.add.at(matrix, ga[m] * G + gb[m], wa[m])
        m = src_ok & ~hit & bool(escaped)
        np.add.at(esc, ga[m], wa[m])
        m = src_ok & ~hit_ok & ~(~hit & bool(escaped))
        np.add.at(unc, ga[m], wa[m])
    return matrix.reshape(G, G), esc, unc


def grouped_from_matrix(M, groups, n_groups, weights=None):
    """P diag(w) M P^T in u64 (wrapping): what the uniform sampling must give for the reference's matrix M[src_meta - 1, hit_meta - 1]."""
    n, G = len(M), int(n_groups)
    groups = np.asarray(groups, np.int64)
    w = np.ones(n, np.uint64) if weights is None else np.asarray(weights).astype(np.uint64)
    keep = groups < G
    P = np.zeros((G, n), np.uint64)
    P[groups[keep], np.nonzero(keep)[0]] = 1
    with np.errstate(over="ignore"):
        return P @ (w[:, None] * np.asarray(M).astype(np.uint64)) @ P.T


def wall_groups(n_before, k):
    """The groups of n_before leading primitives (one group, number 6) followed by scenes.box_room(lo, hi, k): wall = axis * 2 + side."""
    per = 2 * k * k
    return np.concatenate([np.full(n_before, 6, np.uint32), np.repeat(np.arange(6, dtype=np.uint32), per)])


# The unit cube's form factors between whole walls (closed forms for identical, directly opposed / perpendicular unit squares):
F_OPPOSITE, F_ADJACENT = 0.199825, 0.200044
