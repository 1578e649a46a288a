"""numpy float32 restatement of the soft-shadow stage (rc_soft_shadow_rays_device, include/raycore_mi355x.h): the sampled area-light
target of compute_light (docs/src/raytracing-core.jl:61-81) with Philox in place of rand(Vec3f), and the shadow ray toward it.

The target is built from bounce_model's philox4x32_10, u32_to_unit and dot3; the hit frame (p, n) comes from the oracle's
Scene.hit_points; the ray is o = p + n * bias, lv = target - o, dist = sqrt(dot3(lv, lv)), d = lv / dist.  Everything is float32, one
IEEE operation at a time, left to right (numpy never fuses a*b+c).  The expected counts come from the oracle's any-hit trace of these
rays, the t_max > 0 gate and a sum over the samples."""
import numpy as np

from bounce_model import F32, dot3, philox4x32_10, u32_to_unit
from oracle.pyoracle import HIT_DT, RAY_DT

TAG = 0x53460000


def uniforms(path, l, s, depth, seed):
    """(r0, r1, r2) of sample s of light l on `path`: counter (lo32 path, hi32 path, s | depth << 16, TAG | l), key = seed."""
    path = np.asarray(path, np.uint64)
    r = philox4x32_10(path & np.uint64(0xFFFFFFFF), path >> np.uint64(32), np.asarray(s, np.uint64) | np.uint64(int(depth) << 16),
                      np.uint64(TAG) | np.asarray(l, np.uint64), int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    return u32_to_unit(r[0]), u32_to_unit(r[1]), u32_to_unit(r[2])


def targets(p, light, radius, samples, path, l, s, depth, seed):
    """The sampled target per row of p (k, 3) for light `light` (3,) of index l and sample indices s (k,) or a scalar."""
    p = np.asarray(p, F32)
    light = np.asarray(light, F32)
    if samples == 1:
        return np.broadcast_to(light, p.shape).copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        lv = light[None, :] - p
        light_dir = lv / np.sqrt(dot3(lv, lv))[:, None]
        r = uniforms(path, l, s, depth, seed)
        off = np.stack([(rk * F32(2) - F32(1)) * F32(radius) for rk in r], axis=-1).astype(F32)
        off = off - light_dir * dot3(off, light_dir)[:, None]
        return (light[None, :] + off).astype(F32)


def shadow_ray_to(p, nrm, target, bias):
    """(o, d, t_max) of the shadow ray from the biased hit point toward target."""
    with np.errstate(divide="ignore", invalid="ignore"):
        o = p + nrm * F32(bias)
        lv = target - o
        dist = np.sqrt(dot3(lv, lv))
        return o, lv / dist[:, None], dist


def soft_shadow_rays(scene, rays, hits, lights, radii, samples, seed=0, depth=0, bias=1e-3, path_in=None, path_base=0):
    """The stage's n * L * samples rays (RAY_DT), slot (i * L + l) * samples + s; miss slots hold the dummy ray (d = (0,0,1), t_max = 0)."""
    rays = np.ascontiguousarray(rays, RAY_DT)
    hits = np.ascontiguousarray(hits, HIT_DT)
    lights = np.asarray(lights, F32).reshape(-1, 3)
    radii = np.asarray(radii, F32).reshape(-1)
    n, L, S = len(rays), len(lights), int(samples)
    out = np.zeros((n, L, S), RAY_DT)
    out["d"] = (0, 0, 1)
    idx = np.nonzero(hits["hit"] != 0)[0]
    if len(idx) == 0:
        return out.reshape(-1)
    path = np.uint64(path_base) + (np.asarray(path_in, np.uint64)[idx] if path_in is not None else idx.astype(np.uint64))
    p, nrm = scene.hit_points(rays[idx], hits[idx])
    for l in range(L):
        for s in range(S):
            t = targets(p, lights[l], radii[l], S, path, l, s, depth, seed)
            o, d, dist = shadow_ray_to(p, nrm, t, bias)
            out["o"][idx, l, s] = o
            out["d"][idx, l, s] = d
            out["tmax"][idx, l, s] = dist
    return out.reshape(-1)


def counts_of(hits, shadow_rays, shadow_hits, n_lights, samples):
    """(n, L) u32: per (hit, light) the samples with hits[i].hit && ray.t_max > 0 && !any_hit(ray).hit."""
    n = len(hits)
    with np.errstate(invalid="ignore"):
        seen = (np.repeat(hits["hit"] != 0, n_lights * samples) & (shadow_rays["tmax"] > 0) & (shadow_hits["hit"] == 0))
    return seen.reshape(n, n_lights, samples).sum(axis=2).astype(np.uint32)


def expected_counts(scene, rays, hits, lights, radii, samples, seed=0, depth=0, bias=1e-3, path_in=None, path_base=0, nthreads=16):
    """The model's rays traced by the oracle alone (mode="any"), gated and summed: ((n, L) u32 counts, the rays)."""
    lights = np.asarray(lights, F32).reshape(-1, 3)
    sr = soft_shadow_rays(scene, rays, hits, lights, radii, samples, seed, depth, bias, path_in, path_base)
    sh = scene.trace(sr, mode="any", nthreads=nthreads)
    return counts_of(np.ascontiguousarray(hits, HIT_DT), sr, sh, len(lights), int(samples)), sr
