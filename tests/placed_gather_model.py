"""numpy restatement of the placed final gather (rc_placed_final_gather_device, rc_placed_hit_indices_device, include/raycore_mi355x.h),
from existing pieces only: ao_model's rays, the CPU oracle's closest-hit trace, and placed_vf_model's index space (placed_hits, bases,
prim_counts).

The rays are ao_model.ao_rays -- sample s of slot i at i * samples + s --, traced by the oracle for the CLOSEST hit; the placed primitive of
a hit is b = base[instance_id] + (primitive_id - the instance's first flat primitive).  Per sample, with live = hits[i].hit &&
ray.t_max > 0 and P = the number of placed primitives:
    live && H.hit  :  sums[i] += x[b]                       (every hit is counted: b < P always; no metadata takes part)
    live && !H.hit :  sums[i] += miss_value, open[i] += 1
sums are uint64 modulo 2^64, open uint32."""
import numpy as np

import ao_model as am
import placed_vf_model as pm
from oracle.pyoracle import HIT_DT

U32_MAX = (1 << 32) - 1
INVALID = U32_MAX  # RC_INVALID_ID


def sample_table(scene, rays, hits, samples, seed=0, depth=0, bias=1e-3, max_dist=np.inf, path_in=None, path_base=0, nthreads=16):
    """What every sample met, from the oracle alone: (b, escaped, gather_rays) with b (n, samples) int64 -- the placed primitive of the
    closest hit of a live sample, -1 where there is none -- and escaped (n, samples) bool, a live sample that hit nothing."""
    hits = np.ascontiguousarray(hits, HIT_DT)
    S = int(samples)
    gr = am.ao_rays(scene, rays, hits, S, seed, depth, bias, max_dist, path_in, path_base)
    gh = scene.trace(gr, mode="closest", nthreads=nthreads)
    return sample_table_of(pm.bases(scene), pm.prim_counts(scene)[1], hits, gr, gh, S) + (gr,)


def sample_table_of(base, prims_offset, hits, gather_rays, gather_hits, samples):
    """(b, escaped) of stored rays and their closest-hit records, whoever traced them (the composed path's host reduction).  base /
    prims_offset: placed_vf_model.bases and the second result of placed_vf_model.prim_counts."""
    n, S = len(hits), int(samples)
    with np.errstate(invalid="ignore"):
        live = np.repeat(hits["hit"] != 0, S) & (gather_rays["tmax"] > 0)
    struck = live & (gather_hits["hit"] != 0)
    b = np.where(struck, pm.placed_hits(gather_hits, base, prims_offset), -1)
    return b.reshape(n, S), (live & (gather_hits["hit"] == 0)).reshape(n, S)


def reduce(b, escaped, x, miss_value=0, samples=None):
    """(sums uint64 (n,), open uint32 (n,)) of the first `samples` columns of a sample table under the rule above; len(x) = P."""
    x = np.asarray(x, np.uint32)
    S = b.shape[1] if samples is None else int(samples)
    b, escaped = b[:, :S], escaped[:, :S]
    assert b.max(initial=-1) < len(x)
    value = np.zeros(b.shape, np.uint64)
    value[b >= 0] = x[b[b >= 0]]
    value[escaped] = np.uint64(miss_value)
    return value.sum(axis=1, dtype=np.uint64), escaped.sum(axis=1).astype(np.uint32)


def expected(scene, rays, hits, x, samples, miss_value=0, **kw):
    """(sums, open) of the model's rays traced by the oracle alone."""
    b, escaped, _ = sample_table(scene, rays, hits, samples, **kw)
    return reduce(b, escaped, x, miss_value)


def hit_indices(scene, hits):
    """rc_placed_hit_indices_device on hit records: (n,) uint32, the placed primitive of a hit, RC_INVALID_ID for a miss."""
    b = pm.placed_hits(np.ascontiguousarray(hits, HIT_DT), pm.bases(scene), pm.prim_counts(scene)[1])
    return np.where(b >= 0, b, INVALID).astype(np.uint32)


def lift(scene, x_meta):
    """A field per metadata carried to the placed index space: x_placed[q] = x_meta[meta(flat(q)) - 1].  Needs metadata in 1..len(x_meta)."""
    x_meta = np.asarray(x_meta, np.uint32)
    _, flat = pm.placed_index(scene)
    meta = scene.blas_prims["meta"].astype(np.int64)[flat]
    assert meta.min() >= 1 and meta.max() <= len(x_meta)
    return x_meta[meta - 1]
