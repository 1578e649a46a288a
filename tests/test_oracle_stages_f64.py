"""An independent check of the oracle's wavefront stages (hit_points, shadow_rays, reflection_rays).  The oracle's hit_frame is a
line-for-line twin of the device function, so a shared mistake -- the wrong matrix for the normal, the primitive or the instance picked
by the wrong index -- passes every bit-for-bit comparison.  Here the stages are restated in float64 numpy in ANOTHER formulation:

  * the triangle of a hit is looked up in the test's own bookkeeping (instance position -> geometry -> input faces); the flat primitive
    array only has to name one of THAT geometry's triangles;
  * the world normal is the normalised cross product of the TRANSFORMED edges, A (v1 - v0) x A (v2 - v0), flipped to face the ray origin:
    no inverse matrix anywhere;
  * the hit point must be o + t d and lie on the world-space plane of the transformed triangle;
  * shadow origin / direction / t_max follow from those; the reflection from the float64 interpolation of the input mesh's normals.

Geometry with well-shaped triangles (fan spheres as soups, bumpy grid meshes), several geometries per scene, instances from the fuzz's
hostile_transform kinds 0 (rotation x scale), 1 (mirror) and 2 (shear + anisotropic scale), rays aimed as the fuzz aims them.  Slots with
|n . d| < 1e-4 are skipped: there the flip is decided by rounding.

The bound on the normal is set by measurement and proved to discriminate: the mutant "forward 3x3 applied to the local normal" (computed
here, in numpy) is indistinguishable under rotations and mirrors and wrong under shear.

Measured on these inputs (x86-64, the oracle as committed):
  family        hits    skipped   worst |n_oracle - n_f64|   mutant |n_mutant - n_f64| (median)   worst plane distance / tolerance
  kinds 0 / 1   10 273  0         1.43e-7                    2.2e-8 (no deviation)                0.045
  kind 2        25 385  0         2.61e-7                    0.777                                0.059
NORMAL_BOUND = 4e-6: above 4 x the worst case of either family, below 1/1000 of the mutant's median on the shear family."""
import numpy as np

from scene_kit import grid_mesh, hostile_transform, scenes_module


NORMAL_BOUND = 4e-6
EPS = 2.0 ** -24           # half an ulp of 1.0f: the relative error of one correctly rounded float32 operation
BIAS = 0.05
LIGHT = np.array([1.5, 4.0, -2.5], np.float32)
N_RAYS = 30_000


def geometries(sc):
    """[(kind, verts or (v, f, nrm, uv))]: four geometries with distinct triangles; soups carry metadata 1..n."""
    a = sc.fan_sphere(12, 7, radius=0.5)
    b = sc.fan_sphere(9, 5, centre=(0.2, -0.1, 0.3), radius=0.8)
    v1, f1, n1, uv1 = grid_mesh(7, seed=21)
    v2, f2, n2, _ = grid_mesh(4, seed=22, with_uv=False)
    return [("soup", a), ("mesh", (v1 - np.float32(0.5), f1, n1, uv1)), ("soup", b), ("mesh", (v2 * np.float32(1.5), f2, n2, None))]


def build(po, sc, kinds, seed):
    """An oracle scene of the four geometries, 5 instances each with transforms of the given kinds -> (scene, per-instance A (3x4 f64),
    per-instance geometry index, per-geometry faces (F, 3, 3) f32, per-geometry corner normals (F, 3, 3) f64, per-geometry lookup)."""
    g = np.random.default_rng(seed)
    s = po.Scene()
    faces, normals, lookup = [], [], []
    for kind, geo in geometries(sc):
        if kind == "soup":
            tri = np.asarray(geo, np.float32).reshape(-1, 3, 3)
            s.add_blas(tri.reshape(-1, 9), np.arange(1, len(tri) + 1, dtype=np.uint32))
            t64 = tri.astype(np.float64)
            n = np.cross(t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0])
            n /= np.linalg.norm(n, axis=1, keepdims=True)
            cn = np.repeat(n[:, None, :], 3, axis=1)       # a soup triangle's corner normals: its geometric normal (build_triangle)
        else:
            v, f, nrm, uv = geo
            s.add_mesh(v, f, nrm, uv)
            tri, cn = v[f], nrm[f].astype(np.float64)
        faces.append(tri)
        normals.append(cn)
        lookup.append({t.tobytes(): k for k, t in enumerate(tri)})
        assert len(lookup[-1]) == len(tri)
    assert len(set().union(*[set(d) for d in lookup])) == sum(len(d) for d in lookup), "the geometries share no triangle"
    xforms, geo_of = [], []
    order = g.permutation(np.repeat(np.arange(len(faces)), 5))  # instances of the geometries interleaved
    for k, b in enumerate(order):
        x = hostile_transform(g, int(kinds[k % len(kinds)]))
        s.add_instance(int(b) + 1, x, 1000 + 7 * k)
        xforms.append(x.astype(np.float64).reshape(3, 4))
        geo_of.append(int(b))
    return s.build(), np.array(xforms), np.array(geo_of), faces, normals, lookup


def fuzz_rays(sc, seed, n):
    g = np.random.default_rng(seed)
    org = g.uniform(-5, 5, size=(n, 3))
    tgt = g.uniform(-3.5, 3.5, size=(n, 3))
    d = tgt - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return sc.make_rays(org, d)


def unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def norm(a):
    return np.linalg.norm(a, axis=-1)


def check_family(po, kinds, seed, what):
    sc = scenes_module()
    s, A, geo_of, faces, normals, lookup = build(po, sc, kinds, seed)
    rays = fuzz_rays(sc, seed + 1, N_RAYS)
    hits = s.trace(rays, nthreads=8)
    idx = np.nonzero(hits["hit"] == 1)[0]
    prims = s.blas_prims
    # ---- the hit's triangle, by the test's own bookkeeping -------------------------------------------------------------------
    inst = hits["instance_id"][idx].astype(np.int64)
    assert inst.max() < len(A)
    assert np.array_equal(hits["instance_custom_index"][idx], 1000 + 7 * inst), f"{what}: instance_id does not name the instance's position"
    gi = geo_of[inst]
    face = np.empty(len(idx), np.int64)
    for j, (i, b) in enumerate(zip(idx, gi)):
        key = prims["v"][hits["primitive_id"][i]].tobytes()
        assert key in lookup[b], f"{what}: ray {i}: flat primitive {hits['primitive_id'][i]} is no triangle of geometry {b}, which instance {inst[j]} instantiates"
        face[j] = lookup[b][key]
        assert prims["meta"][hits["primitive_id"][i]] == face[j] + 1
    tri = np.stack([faces[b][k] for b, k in zip(gi, face)]).astype(np.float64)       # (H, 3, 3) local
    cn = np.stack([normals[b][k] for b, k in zip(gi, face)])                         # (H, 3, 3) corner normals
    M, T = A[inst][:, :, :3], A[inst][:, :, 3]
    w = np.einsum("hij,hkj->hki", M, tri) + T[:, None, :]                            # world-space corners
    e1, e2 = w[:, 1] - w[:, 0], w[:, 2] - w[:, 0]
    o, d, t = rays["o"][idx].astype(np.float64), rays["d"][idx].astype(np.float64), hits["t"][idx].astype(np.float64)
    u, v = hits["bary_u"][idx].astype(np.float64), hits["bary_v"][idx].astype(np.float64)
    n64 = unit(np.cross(e1, e2))
    nd = np.einsum("hi,hi->h", n64, d)
    n64 = np.where((nd > 0)[:, None], -n64, n64)
    keep = np.abs(nd) >= 1e-4
    skipped = 1.0 - keep.mean()
    assert skipped < 0.01, f"{what}: {skipped:.2%} of the hits are grazing"
    # ---- hit_points -----------------------------------------------------------------------------------------------------------
    pts, nrm = s.hit_points(rays, hits)
    assert not pts[hits["hit"] == 0].any() and not nrm[hits["hit"] == 0].any()
    p64 = o + t[:, None] * d
    mag = norm(o) + np.abs(t)
    # o + d * t in float32: one product and one sum per component, each within EPS of its result
    assert np.all(norm(pts[idx] - p64) <= 4 * EPS * mag), f"{what}: hit point is not o + t d"
    # ... and on the triangle's plane: t is within 1e-5 relative of the true distance (BASELINE north star, with the floor of a tenth of
    # the scene's diagonal test_oracle_independent_f64 uses), and a point moved by dt along the unit d leaves the plane by at most dt
    wb = s.world_bound
    floor = 0.1 * float(np.linalg.norm(np.asarray(wb[3:], np.float64) - np.asarray(wb[:3], np.float64)))
    plane_tol = 1e-5 * np.maximum(np.abs(t), floor) + 4 * EPS * mag
    plane = np.abs(np.einsum("hi,hi->h", pts[idx] - w[:, 0], n64))
    assert np.all(plane <= plane_tol), f"{what}: hit point off its triangle's plane by {np.max(plane / plane_tol):.3g} tolerances"
    # the same point from the barycentrics: the hit names this triangle, not a coplanar neighbour
    bary = w[:, 0] + u[:, None] * e1 + v[:, None] * e2
    size = np.maximum(norm(e1), norm(e2))
    assert np.all(norm(bary - p64)[keep] <= plane_tol[keep] / np.abs(nd[keep]) + 1e-3 * size[keep]), f"{what}: o + t d is not the barycentric point"
    dev = norm(nrm[idx] - n64)[keep]
    local_n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    mutant = unit(np.einsum("hij,hj->hi", M, local_n))                               # the wrong matrix: forward instead of inverse-transpose
    mutant = np.where((np.einsum("hi,hi->h", mutant, d) > 0)[:, None], -mutant, mutant)
    mdev = norm(mutant - n64)[keep]
    flipped = int((nd > 0).sum())
    # ---- shadow_rays ------------------------------------------------------------------------------------------------------------
    sr = s.shadow_rays(rays, hits, LIGHT, BIAS)
    miss = hits["hit"] == 0
    assert np.all(sr["tmax"][miss] == 0) and np.all(sr["d"][miss] == (0, 0, 1)) and not sr["o"][miss].any()
    o_s64 = p64 + BIAS * n64
    lv = LIGHT.astype(np.float64) - o_s64
    dist = norm(lv)
    k = keep
    # origin: the point's roundings, the normal's bound scaled by the bias, and the product's and the sum's own roundings
    tol_o = 4 * EPS * mag + BIAS * NORMAL_BOUND + 4 * EPS * (mag + BIAS)
    assert np.all(norm(sr["o"][idx] - o_s64)[k] <= tol_o[k]), f"{what}: shadow origin"
    assert np.all(sr["tmin"][idx] == 0)
    # light - origin rounds once per component; the dot product, square root and the three divisions a few EPS of their results
    tol_lv = tol_o + 2 * EPS * (norm(LIGHT.astype(np.float64)) + norm(o_s64))
    assert np.all(np.abs(sr["tmax"][idx] - dist)[k] <= (tol_lv + 8 * EPS * dist)[k]), f"{what}: shadow t_max"
    assert np.all(norm(sr["d"][idx] - lv / dist[:, None])[k] <= (2 * tol_lv / dist + 8 * EPS)[k]), f"{what}: shadow direction"
    # ---- reflection_rays ------------------------------------------------------------------------------------------------------
    rr = s.reflection_rays(rays, hits, BIAS)
    assert np.all(rr["tmax"][miss] == 0) and np.all(rr["d"][miss] == (0, 0, 1))
    b = np.stack([1.0 - u - v, u, v], axis=1)
    summed = np.einsum("hk,hki->hi", b, cn)
    sn64 = unit(summed)
    # float32 interpolation: each term and each partial sum rounds; relative to the sum that is the conditioning sum |b_k n_k| / |sum|.
    # A soup's corner normals are the float32 normalised cross product of its float32 edges (well-shaped triangles: a few EPS more)
    cond = np.einsum("hk,hk->h", np.abs(b), norm(cn)) / norm(summed)
    tol_n = 16 * EPS * cond
    rd64 = d - 2.0 * np.einsum("hi,hi->h", d, sn64)[:, None] * sn64
    assert np.all(norm(rr["d"][idx] - rd64) <= 6 * tol_n + 8 * EPS), f"{what}: reflected direction"
    assert np.all(norm(rr["o"][idx] - (p64 + BIAS * sn64)) <= 4 * EPS * mag + BIAS * tol_n + 4 * EPS * (mag + BIAS)), f"{what}: reflection origin"
    assert np.all(rr["tmin"][idx] == 0) and np.all(np.isinf(rr["tmax"][idx]))
    sa, _ = s.shading_attributes(hits)
    assert np.all(norm(sa[idx] - sn64) <= tol_n), f"{what}: interpolated shading normal"
    print(f"{what}: {len(idx)} hits ({flipped} flipped), {skipped:.3%} skipped, worst normal deviation {dev.max():.3g}, mutant median {np.median(mdev):.3g}, "
          f"worst plane distance {np.max(plane / plane_tol):.3g} tolerances")
    return len(idx), flipped, float(dev.max()), float(np.median(mdev))


def test_rotations_and_mirrors(oracle):
    """Kinds 0 and 1: the oracle's normal is within NORMAL_BOUND of the float64 one.  The wrong-matrix mutant does not deviate here (a
    scaled orthogonal matrix and its inverse-transpose give the same direction): this family does not discriminate, the next one does."""
    n, flipped, worst, mutant = check_family(oracle, (0, 1), 101, "kinds 0 / 1")
    assert n >= 1000 and 100 <= flipped <= n - 100
    assert 4 * worst <= NORMAL_BOUND
    assert mutant <= NORMAL_BOUND


def test_shear(oracle):
    """Kind 2: both sides of the bound -- the oracle at most a quarter of it, the mutant's median at least 1000 times it."""
    n, flipped, worst, mutant = check_family(oracle, (2,), 202, "kind 2")
    assert n >= 1000 and 100 <= flipped <= n - 100
    assert 4 * worst <= NORMAL_BOUND <= mutant / 1000
