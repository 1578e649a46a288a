"""numpy float32 restatement of the ambient-occlusion stage (rc_ambient_occlusion_rays_device, include/raycore_mi355x.h): `samples`
cosine-weighted rays of length max_dist over the hemisphere of every hit.

The direction is bounce_model's cosine_hemisphere of two uniforms from bounce_model's philox4x32_10 / u32_to_unit, counter
(lo32 path, hi32 path, s, 0x414F0000 | depth), key = seed; the hit frame (p, n) comes from the oracle's Scene.hit_points; the ray is
o = p + n * bias, t_min = 0, d, t_max = max_dist.  Everything is float32, one IEEE operation at a time, left to right (numpy never fuses
a*b+c).  The expected counts come from the oracle's any-hit trace of these rays, the t_max > 0 gate and a sum over the samples."""
import numpy as np

from bounce_model import F32, cosine_hemisphere, philox4x32_10, u32_to_unit
from oracle.pyoracle import HIT_DT, RAY_DT

TAG = 0x414F0000


def uniforms(path, s, depth, seed):
    """(u1, u2) of sample s on `path`: counter (lo32 path, hi32 path, s, TAG | depth), key = seed."""
    path = np.asarray(path, np.uint64)
    r = philox4x32_10(path & np.uint64(0xFFFFFFFF), path >> np.uint64(32), np.asarray(s, np.uint64), np.uint64(TAG | int(depth)),
                      int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    return u32_to_unit(r[0]), u32_to_unit(r[1])


def directions(nrm, path, s, depth, seed):
    """The cosine-weighted direction of sample s per row of the (unit) normals nrm (k, 3), not renormalised."""
    u1, u2 = uniforms(path, s, depth, seed)
    with np.errstate(divide="ignore", invalid="ignore"):  # (a NaN normal gives a NaN direction, silently)
        d, _ = cosine_hemisphere(nrm, u1, u2)
    return d.astype(F32)


def ao_rays(scene, rays, hits, samples, seed=0, depth=0, bias=1e-3, max_dist=np.inf, path_in=None, path_base=0):
    """The stage's n * samples rays (RAY_DT), slot i * samples + s; miss slots hold the dummy ray (d = (0,0,1), t_max = 0)."""
    rays = np.ascontiguousarray(rays, RAY_DT)
    hits = np.ascontiguousarray(hits, HIT_DT)
    n, S = len(rays), int(samples)
    out = np.zeros((n, S), RAY_DT)
    out["d"] = (0, 0, 1)
    idx = np.nonzero(hits["hit"] != 0)[0]
    if len(idx) == 0:
        return out.reshape(-1)
    path = np.uint64(path_base) + (np.asarray(path_in, np.uint64)[idx] if path_in is not None else idx.astype(np.uint64))
    p, nrm = scene.hit_points(rays[idx], hits[idx])
    with np.errstate(invalid="ignore"):
        o = p + nrm * F32(bias)
    for s in range(S):
        out["o"][idx, s] = o
        out["d"][idx, s] = directions(nrm, path, s, depth, seed)
        out["tmax"][idx, s] = F32(max_dist)
    return out.reshape(-1)


def counts_of(hits, ao_rays, ao_hits, samples):
    """(n,) u32: per hit the samples with hits[i].hit && ray.t_max > 0 && !any_hit(ray).hit."""
    n = len(hits)
    with np.errstate(invalid="ignore"):
        seen = np.repeat(hits["hit"] != 0, samples) & (ao_rays["tmax"] > 0) & (ao_hits["hit"] == 0)
    return seen.reshape(n, samples).sum(axis=1).astype(np.uint32)


def expected_counts(scene, rays, hits, samples, seed=0, depth=0, bias=1e-3, max_dist=np.inf, path_in=None, path_base=0, nthreads=16):
    """The model's rays traced by the oracle alone (mode="any"), gated and summed: ((n,) u32 counts, the rays)."""
    ar = ao_rays(scene, rays, hits, samples, seed, depth, bias, max_dist, path_in, path_base)
    ah = scene.trace(ar, mode="any", nthreads=nthreads)
    return counts_of(np.ascontiguousarray(hits, HIT_DT), ar, ah, int(samples)), ar
