"""numpy restatement of the final gather (rc_final_gather_device, include/raycore_mi355x.h), from ao_model's rays and the CPU oracle only.

The rays are ao_model.ao_rays -- the ambient-occlusion stage's, sample s of slot i at i * samples + s --, traced by the oracle for the
CLOSEST hit; the hit's metadata is prims["meta"][primitive_id] of the oracle's flat primitive array.  Per sample, with
live = hits[i].hit && ray.t_max > 0 and N = the number of primitives:
    live && H.hit && 1 <= m <= N :  sums[i] += x[m - 1]
    live && H.hit, m outside 1..N:  nothing                              (get_illumination's rule, src/kernels.jl:123)
    live && !H.hit               :  sums[i] += miss_value, open[i] += 1
sums are uint64 modulo 2^64, open uint32."""
import numpy as np

import ao_model as am
from oracle.pyoracle import HIT_DT

U32_MAX = (1 << 32) - 1


def sample_table(scene, rays, hits, samples, seed=0, depth=0, bias=1e-3, max_dist=np.inf, path_in=None, path_base=0, nthreads=16):
    """What every sample met, from the oracle alone: (meta, escaped, gather_rays) with meta (n, samples) int64 -- the metadata of the
    closest hit of a live sample, -1 where there is none -- and escaped (n, samples) bool, a live sample that hit nothing."""
    hits = np.ascontiguousarray(hits, HIT_DT)
    n, S = len(hits), int(samples)
    gr = am.ao_rays(scene, rays, hits, S, seed, depth, bias, max_dist, path_in, path_base)
    gh = scene.trace(gr, mode="closest", nthreads=nthreads)
    return sample_table_of(scene.blas_prims["meta"], hits, gr, gh, S) + (gr,)


def sample_table_of(prim_meta, hits, gather_rays, gather_hits, samples):
    """(meta, escaped) of stored rays and their closest-hit records, whoever traced them (the composed path's host reduction)."""
    n, S = len(hits), int(samples)
    with np.errstate(invalid="ignore"):
        live = np.repeat(hits["hit"] != 0, S) & (gather_rays["tmax"] > 0)
    struck = live & (gather_hits["hit"] != 0)
    meta = np.full(n * S, -1, np.int64)
    meta[struck] = np.asarray(prim_meta, np.int64)[gather_hits["primitive_id"][struck]]
    return meta.reshape(n, S), (live & (gather_hits["hit"] == 0)).reshape(n, S)


def reduce(meta, escaped, x, miss_value=0, samples=None):
    """(sums uint64 (n,), open uint32 (n,)) of the first `samples` columns of a sample table under the rule above; len(x) = N."""
    x = np.asarray(x, np.uint32)
    S = meta.shape[1] if samples is None else int(samples)
    meta, escaped = meta[:, :S], escaped[:, :S]
    counted = (meta >= 1) & (meta <= len(x))
    value = np.zeros(meta.shape, np.uint64)
    value[counted] = x[meta[counted] - 1]
    value[escaped] = np.uint64(miss_value)
    return value.sum(axis=1, dtype=np.uint64), escaped.sum(axis=1).astype(np.uint32)


def expected(scene, rays, hits, x, samples, miss_value=0, **kw):
    """(sums, open) of the model's rays traced by the oracle alone."""
    meta, escaped, _ = sample_table(scene, rays, hits, samples, **kw)
    return reduce(meta, escaped, x, miss_value)
