"""numpy restatement of the diffuse bounce stage (rc_bounce_rays_device, include/raycore_mi355x.h).

Philox4x32-10 and the f64 sampler trig are vectorised ports of the oracle's own primitives (rco_philox4x32_10, rco_sincos_f64,
rco_acos_f64); tests/test_bounce_model.py checks the ports against them.  The hit frame (p, n) comes from the oracle's Scene.hit_points.
Everything else -- concentric disk, get_orthogonal_basis, the final combination -- is float32, one IEEE operation at a time, in the
order the header states (no contraction: numpy never fuses a*b+c)."""
import ctypes as C

import numpy as np

from oracle.pyoracle import HIT_DT, RAY_DT

F32 = np.float32
PI_F32 = F32(np.pi)  # Float32(pi) = 3.1415927f
TAG = 0x424E0000
INVALID_ID = 0xFFFFFFFF


def oracle_primitives(po):
    """The oracle library with the scalar primitives' signatures set (pyoracle sets only some of them)."""
    L = po.lib()
    L.rco_philox4x32_10.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.rco_sincos_f64.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.rco_sincos_f64.restype = None
    L.rco_acos_f64.argtypes = [C.c_double]
    L.rco_acos_f64.restype = C.c_double
    return L


# ---- ports of the oracle's primitives ----------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al. 2011) over arrays of u32 counters; key words broadcast."""
    M = np.uint64(0xFFFFFFFF)
    c = [np.asarray(x, np.uint64) & M for x in (c0, c1, c2, c3)]
    c0, c1, c2, c3 = np.broadcast_arrays(*c)
    k0 = np.uint64(int(k0) & 0xFFFFFFFF)
    k1 = np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & M, n2, p0 & M
        k0 = (k0 + np.uint64(0x9E3779B9)) & M
        k1 = (k1 + np.uint64(0xBB67AE85)) & M
    return [x.astype(np.uint32) for x in (c0, c1, c2, c3)]


def u32_to_unit(x):
    return (np.asarray(x, np.uint32) >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)


def sincos_f64(x):
    """rc_sincos_f64: fdlibm kernels after a one-step pi/2 reduction (the cast to int truncates, as C's does)."""
    x = np.asarray(x, np.float64)
    pio2_hi, pio2_lo, two_over_pi = 1.57079632679489655800e+00, 6.12323399573676603587e-17, 6.36619772367581382433e-01
    k = (x * two_over_pi + 0.5).astype(np.int64)
    kd = k.astype(np.float64)
    r = (x - kd * pio2_hi) - kd * pio2_lo
    z = r * r
    sp = 8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)))
    ks = r + (z * r) * (-1.66666666666666324348e-01 + z * sp)
    cp = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 + z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))))
    kc = 1.0 - (0.5 * z - z * cp)
    q = k & 3
    s = np.select([q == 0, q == 1, q == 2], [ks, kc, -ks], -kc)
    c = np.select([q == 0, q == 1, q == 2], [kc, -ks, -kc], ks)
    return s, c


def acos_f64(x):
    """rc_acos_f64 on [0, 1) (both fdlibm branches evaluated, the right one selected)."""
    x = np.asarray(x, np.float64)
    pio2_hi, pio2_lo = 1.57079632679489655800e+00, 6.12323399573676603587e-17
    pS0, pS1, pS2 = 1.66666666666666657415e-01, -3.25565818622400915405e-01, 2.01212532134862925881e-01
    pS3, pS4, pS5 = -4.00555345006794114027e-02, 7.91534994289814532176e-04, 3.47933107596021167570e-05
    qS1, qS2, qS3, qS4 = -2.40339491173441421878e+00, 2.02094576023350569471e+00, -6.88283971605453293030e-01, 7.70381505559019352791e-02
    z = x * x
    p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))))
    q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)))
    small = pio2_hi - (x - (pio2_lo - x * (p / q)))
    z = (1.0 - x) * 0.5
    s = np.sqrt(z)
    df = (s.view(np.uint64) & np.uint64(0xFFFFFFFF00000000)).view(np.float64)
    c = (z - df * df) / (s + df)
    p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))))
    q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)))
    w = (p / q) * s + c
    big = 2.0 * (df + w)
    return np.where(x < 0.5, small, big)


# ---- float32 vector helpers (rc_device.h order) -----------------------------------------------------------------------------
def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def normalize3(a):
    n = np.sqrt(dot3(a, a))
    return a / n[..., None]


def orthogonal_basis(normal):
    """get_orthogonal_basis (src/math.jl:143-156): (u, v); argmin keeps the first minimum on ties."""
    normal = np.asarray(normal, F32)
    n = normalize3(normal)
    a = np.abs(normal)
    mi = np.zeros(len(normal), np.int64)
    mv = a[:, 0].copy()
    for j in (1, 2):
        lt = a[:, j] < mv
        mi[lt] = j
        mv[lt] = a[lt, j]
    cand = np.eye(3, dtype=F32)[mi]
    bv = normalize3(cross3(n, cand))
    bu = normalize3(cross3(bv, n))
    return bu, bv


def concentric_disk(u1, u2):
    """concentric_sample_disk (src/math.jl:1-14): (dx, dy) float32; cos / sin through sincos_f64 rounded once."""
    u1, u2 = np.asarray(u1, F32), np.asarray(u2, F32)
    ox, oy = F32(2) * u1 - F32(1), F32(2) * u2 - F32(1)
    zero = (ox == 0) & (oy == 0)
    first = np.abs(ox) > np.abs(oy)
    with np.errstate(divide="ignore", invalid="ignore"):
        th1 = ((oy / ox) * PI_F32) / F32(4)
        th2 = PI_F32 / F32(2) - ((ox / oy) * PI_F32) / F32(4)
    r = np.where(first, ox, oy)
    theta = np.where(first, th1, th2)
    theta = np.where(zero, F32(0), theta).astype(F32)
    s, c = sincos_f64(theta.astype(np.float64))
    dx = np.where(zero, F32(0), r * c.astype(F32)).astype(F32)
    dy = np.where(zero, F32(0), r * s.astype(F32)).astype(F32)
    return dx, dy, theta


def cosine_hemisphere(n, u1, u2):
    """cosine_sample_hemisphere about the (unit) normals n, combined (u*dx + v*dy) + n*z without renormalising."""
    n = np.asarray(n, F32)
    dx, dy, _ = concentric_disk(u1, u2)
    z = np.sqrt(np.maximum(F32(0), (F32(1) - dx * dx) - dy * dy))
    bu, bv = orthogonal_basis(n)
    return (bu * dx[:, None] + bv * dy[:, None]) + n * z[:, None], z


def bounce_uniforms(path, k, bounce, seed):
    path = np.asarray(path, np.uint64)
    r = philox4x32_10(path & np.uint64(0xFFFFFFFF), path >> np.uint64(32), np.asarray(k, np.uint64), np.uint64(TAG | int(bounce)),
                      int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    return u32_to_unit(r[0]), u32_to_unit(r[1])


def sources(n_out, src=None, count=None, wrap=False, first=0):
    """(s, k, live) per output slot first .. first + n_out - 1: slot-aligned, live-first queue or round robin (count is the device count
    word's value)."""
    i = np.arange(first, first + n_out, dtype=np.int64)
    if src is None:
        return i, np.zeros(n_out, np.int64), np.ones(n_out, bool)
    src = np.asarray(src, np.int64)
    if count == 0:
        return np.zeros(n_out, np.int64), np.zeros(n_out, np.int64), np.zeros(n_out, bool)
    if wrap:
        return src[i % count], i // count, np.ones(n_out, bool)
    live = i < count
    s = np.zeros(n_out, np.int64)
    s[live] = src[i[live]]
    return s, np.zeros(n_out, np.int64), live


def bounce_rays(scene, rays, hits, n_out, seed=0, bounce=0, bias=1e-3, src=None, count=None, wrap=False, path_in=None, path_base=0, first=0):
    """The stage's output for output slots first .. first + n_out - 1: (RAY_DT array, u32 path ids).  `scene` is an oracle Scene (for
    the hit frames)."""
    rays = np.ascontiguousarray(rays, RAY_DT)
    hits = np.ascontiguousarray(hits, HIT_DT)
    s, k, live = sources(n_out, src, count, wrap, first)
    live &= hits["hit"][s] != 0
    out = np.zeros(n_out, RAY_DT)
    out["d"] = (0, 0, 1)
    out["tmax"] = -1
    path_ids = np.full(n_out, INVALID_ID, np.uint32)
    idx = np.nonzero(live)[0]
    if len(idx) == 0:
        return out, path_ids
    ss = s[idx]
    path = np.uint64(path_base) + (np.asarray(path_in, np.uint64)[ss] if path_in is not None else ss.astype(np.uint64))
    p, nrm = scene.hit_points(rays[ss], hits[ss])
    u1, u2 = bounce_uniforms(path, k[idx], bounce, seed)
    d, _ = cosine_hemisphere(nrm, u1, u2)
    out["o"][idx] = p + nrm * F32(bias)
    out["tmin"][idx] = 0
    out["d"][idx] = d
    out["tmax"][idx] = np.inf
    path_ids[idx] = (path & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return out, path_ids


def view_factor_ray(prims, src, ray_idx, seed=0):
    """The ray view_factors! shoots for (source primitive, ray index) (rco_view_factor_ray), for arrays of ray indices: the pieces it
    shares with the bounce (basis, Philox, u32_to_unit, sincos_f64) restated."""
    tri = prims["v"][src].astype(F32)
    ray_idx = np.asarray(ray_idx, np.uint64)
    p1, p2, p3 = (np.broadcast_to(tri[j], (len(ray_idx), 3)) for j in range(3))
    normal = normalize3(cross3(p2 - p1, p3 - p1))
    bu, bv = orthogonal_basis(normal)
    r = philox4x32_10(ray_idx, np.uint64(src), 0, 0, int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    r1, r2, xi1, xi2 = (u32_to_unit(x) for x in r)
    sq = np.sqrt(r1)
    wu, wv, ww = F32(1) - sq, sq * (F32(1) - r2), sq * r2
    pt = (p1 * wu[:, None] + p2 * wv[:, None]) + p3 * ww[:, None]
    o = pt + normal * F32(0.01)
    theta = acos_f64(xi1.astype(np.float64)).astype(F32)
    phi = (F32(2) * PI_F32) * xi2
    st, ct = sincos_f64(theta.astype(np.float64))
    sp, cp = sincos_f64(phi.astype(np.float64))
    st, ct, sp, cp = (x.astype(F32) for x in (st, ct, sp, cp))
    xl, yl, zl = st * cp, st * sp, ct
    d = (bu * xl[:, None] + bv * yl[:, None]) + normal * zl[:, None]
    out = np.zeros(len(ray_idx), RAY_DT)
    out["o"] = o
    out["d"] = d
    out["tmax"] = np.inf
    return out
