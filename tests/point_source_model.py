"""numpy restatement of the point-source illumination calls (rc_point_source_rays_device, rc_get_illumination_points_device,
include/raycore_mi355x.h), built on bounce_model's ports of the oracle's primitives.

A source is one RAY_DT record: o = the lamp's position, d = its axis (all three components zero, either sign: isotropic; anything else:
Lambertian about normalize3(d)), t_min and t_max copied into every ray.  Source k shoots grid^2 rays, cell = a * grid + b:
    rnd = Philox4x32-10(counter = (cell, first_source + k, 0, 0x50530000), key = (lo32 seed, hi32 seed))
    u1 = ((float)a + u32_to_unit(rnd[0])) / (float)grid,  u2 = ((float)b + u32_to_unit(rnd[1])) / (float)grid
    isotropic:  z = 1 - 2 u1;  s = sqrt(max(0, 1 - z z));  phi = (2 * Float32(pi)) * u2;  dir = (s cos phi, s sin phi, z)
    Lambertian: dir = cosine_hemisphere(normalize3(d), u1, u2)
everything float32, one IEEE operation at a time in the order the header states (numpy never fuses a*b+c); sin / cos through sincos_f64,
rounded once.  The expected counts come from these rays, the oracle's closest-hit trace and a bincount by the oracle's metadata."""
import numpy as np

import bounce_model as bm
from oracle.pyoracle import RAY_DT

F32 = np.float32
TAG = 0x50530000


def make_sources(points, axes=None, t_min=0.0, t_max=np.inf):
    p = np.asarray(points, F32).reshape(-1, 3)
    src = np.zeros(len(p), RAY_DT)
    src["o"] = p
    if axes is not None:
        src["d"] = np.asarray(axes, F32).reshape(-1, 3)
    src["tmin"] = t_min
    src["tmax"] = t_max
    return src


def stratified_uniforms(grid, key_source, seed=0):
    """(u1, u2) float32 of the grid^2 cells of the source with Philox counter word `key_source` (= first_source + k), in cell order."""
    G = int(grid)
    cell = np.arange(G * G, dtype=np.uint64)
    a, b = cell // np.uint64(G), cell % np.uint64(G)
    r = bm.philox4x32_10(cell, np.uint64(int(key_source) & 0xFFFFFFFF), 0, TAG, int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    xi1, xi2 = bm.u32_to_unit(r[0]), bm.u32_to_unit(r[1])
    u1 = (a.astype(F32) + xi1) / F32(G)
    u2 = (b.astype(F32) + xi2) / F32(G)
    return u1.astype(F32), u2.astype(F32)


def isotropic_dir(u1, u2):
    u1, u2 = np.asarray(u1, F32), np.asarray(u2, F32)
    z = F32(1) - F32(2) * u1
    s = np.sqrt(np.maximum(F32(0), F32(1) - z * z))
    phi = (F32(2) * bm.PI_F32) * u2
    sn, cs = bm.sincos_f64(phi.astype(np.float64))
    return np.stack([s * cs.astype(F32), s * sn.astype(F32), z], axis=-1).astype(F32)


def lambertian_dir(axis, u1, u2):
    u1, u2 = np.asarray(u1, F32), np.asarray(u2, F32)
    n = bm.normalize3(np.broadcast_to(np.asarray(axis, F32), (len(u1), 3)).copy())
    d, _ = bm.cosine_hemisphere(n, u1, u2)
    return d.astype(F32)


def is_isotropic(source):
    d = np.asarray(source["d"], F32)
    return bool((d == 0).all())


def source_dirs(source, u1, u2):
    with np.errstate(invalid="ignore", divide="ignore"):
        return isotropic_dir(u1, u2) if is_isotropic(source) else lambertian_dir(source["d"], u1, u2)


def point_source_rays(sources, grid, seed=0, first_source=0):
    """The stage's output: len(sources) * grid^2 RAY_DT rays, source k's at k * grid^2 in cell order."""
    sources = np.ascontiguousarray(sources, RAY_DT)
    cells = int(grid) * int(grid)
    out = np.zeros(len(sources) * cells, RAY_DT)
    for k, src in enumerate(sources):
        u1, u2 = stratified_uniforms(grid, first_source + k, seed)
        rows = out[k * cells:(k + 1) * cells]
        rows["o"] = src["o"]
        rows["tmin"] = src["tmin"]
        rows["d"] = source_dirs(src, u1, u2)
        rows["tmax"] = src["tmax"]
    return out


def counts_of(prim_meta, hits, n_sources, grid, n_prims=None):
    """(counts (S, N) uint32, escaped (S,) uint32, dropped (S,) uint32) of closest-hit records of the stage's rays, whoever traced them:
    a bincount by metadata - 1 per source; metadata outside 1..N is dropped; a ray without a hit has escaped."""
    prim_meta = np.asarray(prim_meta, np.int64)
    N = len(prim_meta) if n_prims is None else int(n_prims)
    cells = int(grid) * int(grid)
    counts = np.zeros((n_sources, N), np.uint32)
    escaped = np.zeros(n_sources, np.uint32)
    dropped = np.zeros(n_sources, np.uint32)
    for k in range(n_sources):
        h = hits[k * cells:(k + 1) * cells]
        struck = h["hit"] != 0
        meta = prim_meta[h["primitive_id"][struck]]
        valid = (meta >= 1) & (meta <= N)
        counts[k] = np.bincount(meta[valid] - 1, minlength=N).astype(np.uint32)
        escaped[k] = int((~struck).sum())
        dropped[k] = int((~valid).sum())
    return counts, escaped, dropped


def expected_counts(scene, sources, grid, seed=0, first_source=0, nthreads=8):
    """(counts, escaped, dropped) from the model's rays and the oracle alone."""
    rays = point_source_rays(sources, grid, seed, first_source)
    hits = scene.trace(rays, mode="closest", nthreads=nthreads)
    return counts_of(scene.blas_prims["meta"], hits, len(sources), grid)
