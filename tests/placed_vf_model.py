"""A numpy restatement of the placed-primitive index space, the placed view-factor ray and the placed counting rule
(rc_placed_primitive_bases, rc_placed_triangles_device, rc_placed_view_factor_rays_device, rc_placed_view_factor_groups_device,
include/raycore_mi355x.h).

The ray composes tests/bounce_model.py -- philox4x32_10, u32_to_unit, cosine_hemisphere, orthogonal_basis, acos_f64, sincos_f64 -- and
restates the uniform direction, with the source's instance in the third word of the Philox counter.  The world triangle is float32, one
IEEE operation at a time in the order of oracle/rc_oracle.c's rco_transform_point (numpy never fuses a * b + c).  The rays are traced by the
ORACLE (Scene.trace); the rule is applied here, in integers that wrap modulo 2^64 like the device's u64 adds.  No metadata takes part."""
import numpy as np

import bounce_model as bm

F32 = np.float32
U32_MAX = (1 << 32) - 1
SAMPLINGS = ("uniform", "cosine")


def prim_counts(scene):
    """Per instance, in the instance array's order: (the primitive count of its BLAS, its first flat primitive)."""
    offs = scene.blas_descs["primitives_offset"].astype(np.int64)
    ends = np.append(offs[1:], len(scene.blas_prims))
    b = scene.instances["blas_index"].astype(np.int64) - 1
    return (ends - offs)[b], offs[b]


def bases(scene):
    """base: n_inst + 1 uint32, the exclusive prefix sum of the instances' primitive counts; base[-1] = P."""
    counts, _ = prim_counts(scene)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)


def placed_index(scene):
    """Per placed primitive q: (instance i, flat primitive index)."""
    counts, offs = prim_counts(scene)
    inst = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    base = bases(scene).astype(np.int64)
    return inst, offs[inst] + (np.arange(int(base[-1]), dtype=np.int64) - base[inst])


def world_triangles(scene):
    """(P, 3, 3) float32: p_k = transform_point(T_i, v_k), per row ((m0 * x + m1 * y) + m2 * z) + m3, T_i the instance's forward transform."""
    inst, flat = placed_index(scene)
    m = scene.instances["transform"].astype(F32).reshape(-1, 3, 4)[inst]  # (P, row, column)
    v = scene.blas_prims["v"].astype(F32)[flat]                           # (P, vertex, xyz)
    out = np.empty_like(v)
    for k in range(3):
        x, y, z = (v[:, k, c][:, None] for c in range(3))
        out[:, k, :] = ((m[:, :, 0] * x + m[:, :, 1] * y) + m[:, :, 2] * z) + m[:, :, 3]
    return out


def sampled_rays(tri, flat, inst, ray_idx, seed=0, sampling="uniform"):
    """The placed rays of n items: per item (or one for all) the world triangle `tri` ((n, 3, 3) or (3, 3) float32), the flat primitive
    index `flat` and the instance `inst`, and the ray index `ray_idx` (n): the per-triangle family's ray of the world triangle with the
    Philox counter (ray_idx, flat, inst, 0)."""
    assert sampling in SAMPLINGS
    ray_idx = np.asarray(ray_idx, np.uint64)
    n = len(ray_idx)
    tri = np.broadcast_to(np.asarray(tri, F32), (n, 3, 3))
    p1, p2, p3 = (np.ascontiguousarray(tri[:, j]) for j in range(3))
    normal = bm.normalize3(bm.cross3(p2 - p1, p3 - p1))
    r = bm.philox4x32_10(ray_idx, np.asarray(flat, np.uint64), np.asarray(inst, np.uint64), 0, int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    r1, r2, xi1, xi2 = (bm.u32_to_unit(x) for x in r)
    sq = np.sqrt(r1)
    wu, wv, ww = F32(1) - sq, sq * (F32(1) - r2), sq * r2
    pt = (p1 * wu[:, None] + p2 * wv[:, None]) + p3 * ww[:, None]
    out = np.zeros(n, bm.RAY_DT)
    out["o"] = pt + normal * F32(0.01)
    out["tmax"] = np.inf
    if sampling == "cosine":
        out["d"], _ = bm.cosine_hemisphere(np.ascontiguousarray(normal), xi1, xi2)
        return out
    bu, bv = bm.orthogonal_basis(normal)
    theta = bm.acos_f64(xi1.astype(np.float64)).astype(F32)
    phi = (F32(2) * bm.PI_F32) * xi2
    st, ct = bm.sincos_f64(theta.astype(np.float64))
    sp, cp = bm.sincos_f64(phi.astype(np.float64))
    st, ct, sp, cp = (x.astype(F32) for x in (st, ct, sp, cp))
    out["d"] = (bu * (st * cp)[:, None] + bv * (st * sp)[:, None]) + normal * ct[:, None]
    return out


def placed_rays(scene, q, ray_idx, seed=0, sampling="uniform"):
    """sampled_rays for placed primitive q of an oracle scene."""
    inst, flat = placed_index(scene)
    return sampled_rays(world_triangles(scene)[q], flat[q], inst[q], ray_idx, seed, sampling)


class Traced:
    """One job's rays traced by the oracle, once: per work item (placed primitive placed[0] + w // n_ray, ray rays[0] + w % n_ray) the
    source `a`, whether it hit, and the placed primitive `b` that was hit (-1 on a miss).  count() applies the rule for any grouping."""

    def __init__(self, scene, rays_per_triangle, seed, sampling, placed=None, rays=None, nthreads=8):
        base = bases(scene).astype(np.int64)
        self.base, self.n = base, int(base[-1])
        inst, flat = placed_index(scene)
        tris = world_triangles(scene)
        _, offs = prim_counts(scene)
        q0, q1 = (0, self.n) if placed is None else placed
        r0, r1 = (0, rays_per_triangle) if rays is None else rays
        q0, q1 = min(q0, self.n), min(q1, self.n)
        n_ray = max(r1 - r0, 0)
        self.a = np.repeat(np.arange(q0, max(q1, q0), dtype=np.int64), n_ray)
        idx = np.tile(np.arange(r0, r0 + n_ray, dtype=np.uint64), max(q1 - q0, 0))
        self.rays = sampled_rays(tris[self.a], flat[self.a], inst[self.a], idx, seed, sampling)
        hits = scene.trace(self.rays, nthreads=nthreads)
        self.hit = hits["hit"] == 1
        self.b = placed_hits(hits, base, offs)

    def count(self, groups, n_groups, weights=None, escaped=True):
        return count(self.a, self.hit, self.b, self.n, groups, n_groups, weights, escaped)


def placed_hits(hits, base, prims_offset):
    """b per hit record: base[instance_id] + (primitive_id - the instance's first flat primitive); -1 where nothing was hit."""
    hit = hits["hit"] == 1
    b = np.full(len(hits), -1, np.int64)
    i = hits["instance_id"][hit].astype(np.int64)
    b[hit] = np.asarray(base, np.int64)[i] + (hits["primitive_id"][hit].astype(np.int64) - np.asarray(prims_offset, np.int64)[i])
    return b


def count(a, hit, b, n, groups, n_groups, weights=None, escaped=True):
    """The rule of rc_placed_view_factor_groups_device on traced items: (matrix (G, G) u64, escaped (G,) u64, uncounted (G,) u64).
    `uncounted` is the weight of a group's rays that add nothing although their source counts: hits on the source itself or on an
    excluded group -- and the misses when escaped is False."""
    G = int(n_groups)
    groups = np.asarray(groups, np.int64)
    assert len(groups) == n and 1 <= G <= 65535
    w = np.ones(n, np.uint64) if weights is None else np.asarray(weights).astype(np.uint64)
    ga = groups[a]
    src_ok = ga < G
    wa = np.where(src_ok, w[a], 0).astype(np.uint64)
    hit_ok = hit & (b != a)
    gb = np.where(hit_ok, groups[np.clip(b, 0, n - 1)], G)
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


# ---- the scenes of the tests ---------------------------------------------------------------------------------------------------------
def square(k=2):
    """The unit square in z = 0 split k x k, 2 k^2 triangles, normal +z; (n, 9) float32."""
    s = np.linspace(0.0, 1.0, k + 1)
    out = []
    for i in range(k):
        for j in range(k):
            a, b, c, d = (s[i], s[j], 0), (s[i + 1], s[j], 0), (s[i + 1], s[j + 1], 0), (s[i], s[j + 1], 0)
            out += [a + b + c, a + c + d]
    return np.asarray(out, F32)


def upper_plate(z):
    """Turned 180 degrees about x (y -> -y, z -> -z: the normal points down) and moved so that it covers the unit square at height z."""
    return np.array([1, 0, 0, 0, 0, -1, 0, 1, 0, 0, -1, z], F32)


def plates_cfg(rc, z=1.0):
    """One BLAS, the 8-triangle square, pushed twice: at identity, and turned 180 degrees about x and lifted to height z.  P = 16."""
    verts = square()
    xf = np.stack([rc.scenes.IDENTITY3x4, upper_plate(z)])
    return {"blas": [(verts, np.arange(1, 9, dtype=np.uint32))], "instances": [(1, xf, np.arange(2, dtype=np.uint32))]}


def mixed_cfg(rc):
    """Irregular bases, a mirror and a bent normal: BLAS 1 = the 8-triangle square, BLAS 2 = fan_sphere(12, 7) (144 triangles), BLAS 3 = an
    open room at identity; instances in the order A, B, A, B, B, A, B, room.  One B is scaled by (1, 0.5, 2) and rotated, one A is
    mirrored (det < 0).  Every instance is pushed by itself, so the instance array keeps this order."""
    sc = rc.scenes
    room = sc.box_room((-3, -3, -3), (3, 3, 3), 2)[:-8]

    def xf(lin, t):
        return np.concatenate([np.asarray(lin, np.float64), np.asarray(t, np.float64)[:, None]], axis=1).astype(F32).reshape(12)

    c, s = np.cos(0.7), np.sin(0.7)
    rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    placed = [(1, xf(np.eye(3), (-1.5, -1.5, -2.0))),
              (2, xf(np.eye(3), (1.2, 0.0, 0.0))),
              (1, xf(np.diag([-1.0, 1.0, 1.0]) * 1.5, (0.5, -2.0, 1.0))),                 # mirrored: det < 0
              (2, xf(rot @ np.diag([1.0, 0.5, 2.0]), (-1.2, 0.5, 0.3))),                  # non-uniform scale, rotated
              (2, xf(np.eye(3) * 0.6, (0.0, -1.5, -1.0))),
              (1, xf(np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]]), (-2.0, 2.0, 0.0))),
              (2, xf(np.eye(3), (0.3, 1.6, 1.4))),
              (3, sc.IDENTITY3x4)]
    blas = [(square(), np.arange(1, 9, dtype=np.uint32)), (sc.fan_sphere(12, 7), np.arange(1, 145, dtype=np.uint32)),
            (room, np.arange(1, len(room) + 1, dtype=np.uint32))]
    return {"blas": blas, "instances": [(b, x[None], np.array([k], np.uint32)) for k, (b, x) in enumerate(placed)]}
