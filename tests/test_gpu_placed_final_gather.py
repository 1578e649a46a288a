"""rc_placed_final_gather_device and rc_placed_hit_indices_device on the GPU: the sum of a field per PLACED primitive over the closest hits of
all hits x hemisphere samples in one traversal launch, word for word against the numpy model (tests/placed_gather_model.py: ao_model's
rays, the CPU oracle's closest-hit trace, placed_vf_model's index space), in the three kernel shapes the launcher dispatches and for an
unbounded and a short reach; against the product's own composed path (rc_ambient_occlusion_rays_device + closest-hit trace +
rc_placed_hit_indices_device + a host lookup, also with the entry cull on); against rc_final_gather_device with the field lifted from
metadata; on irregular bases with a mirror and a non-uniform scale; on two plates of ONE mesh that carry different values; accumulation and
path ids; empty work and bad arguments; a captured call whose x is exchanged between replays; behind a device-side transform update; two
streams at once; as a stage of WavefrontPaths; and through the host calls.

Every integer comparison is exact and covers every slot.  The worlds are the final-gather file's: C3 with 16 x 9 fan spheres on the
lattices (3,3,2) and (7,7,6) -- ONE 256-triangle BLAS under 18 and 294 instances, P = 4608 and 75 264, so every instance reads its own
stretch of x where the metadata gather reads one stretch through all of them -- and 63 997 rays, so n * S ends inside a chunk."""
import numpy as np
import pytest

import bounce_model as bm
import gather_model as gm
import placed_gather_model as pg
import placed_vf_model as pm
from gpu_kit import POISON, check_words, dev, finish, poisoned, words_of, zeroed
from gpu_kit import rc  # noqa: F401
from helpers import build_oracle, build_product, random_rays
from scene_kit import distinct_x
from worlds import C3World, three_shapes

pytestmark = pytest.mark.gpu

BIAS = 1e-3
N_RAYS = 63_997  # 320 x 200 less three: n * S ends inside a 128-item chunk for S = 2 and 5 (remainders 122 and 113)
SEED = 0xA0
S_MAX = 5
DISTANCES = (np.inf, 1.0)
U32_MAX = pg.U32_MAX


def check(outs, want, what):
    """outs: (sums tensor, open tensor or None) of a call; want: (sums u64, open u32) of the model."""
    for out, w, dtype, name in ((outs[0], want[0], np.uint64, "sums"), (outs[1], want[1], np.uint32, "open")):
        if out is not None:
            check_words(out, w, dtype, f"{what} ({name})")


def run_gather(t, d_rays, d_hits, n, samples, d_x, outs=None, with_open=True, miss_value=0, max_dist=np.inf, seed=SEED, depth=0, d_path_in=None,
               path_base=0, stream=None, placed=True):
    """One call into zeroed, guarded outputs (or into `outs`); returns (sums tensor, open tensor or None).  placed=False: the metadata
    gather with the same arguments."""
    if outs is None:
        outs = (zeroed(n, 8), zeroed(n, 4) if with_open else None)
    call = t.placed_final_gather_device if placed else t.final_gather_device
    call(d_rays.data_ptr(), d_hits.data_ptr(), n, samples, d_x.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr() if outs[1] is not None else None,
         miss_value=miss_value, max_dist=max_dist, seed=seed, depth=depth, bias=BIAS, d_path_in=d_path_in, path_base=path_base, stream=stream)
    return outs


class Tables:
    """The oracle's sample tables of one scene, computed once per argument set and read-only: (b, escaped), (n, samples) each."""

    def __init__(self, o, s_max):
        self.o, self.s_max, self._tables = o, s_max, {}
        self.base, self.offs = pm.bases(o), pm.prim_counts(o)[1]
        self.P = int(self.base[-1])

    def table_of(self, rays, hits, own, max_dist=np.inf, seed=SEED, depth=0, path_in=None, path_base=0):
        key = (float(max_dist), seed, depth, None if path_in is None else np.asarray(path_in).tobytes(), path_base, own)
        if key not in self._tables:
            b, escaped, _ = pg.sample_table(self.o, rays, hits, self.s_max, seed=seed, depth=depth, bias=BIAS, max_dist=max_dist, path_in=path_in,
                                            path_base=path_base)
            b.setflags(write=False)
            escaped.setflags(write=False)
            self._tables[key] = (b, escaped)
        return self._tables[key]


class World(C3World):
    def __init__(self, rc, oracle, lattice, kernel=None):
        super().__init__(rc, oracle, lattice, kernel)
        self.tables = Tables(self.o, S_MAX)
        self.P = self.tables.P
        n_inst = self.t.n_instances()
        assert self.P == 256 * n_inst and np.array_equal(self.t.placed_primitive_bases(), self.tables.base)
        self.x = distinct_x(self.P, with_max=True)
        inst_of = np.repeat(np.arange(n_inst), 256)
        own = self.hits["instance_id"].astype(np.int64)
        # a degenerate input cannot pass -- all from the oracle alone, before anything is compared: at both reaches enough slots with a
        # sample that lands on ANOTHER instance than the slot's own; at the unbounded reach enough slots whose samples land on two or more
        # instances; enough slots with both a hit and an escape; sums that pass 2^32; and a reach that matters
        for dist in DISTANCES:
            b, escaped = self.table(max_dist=dist)
            struck = b >= 0
            inst = np.where(struck, inst_of[np.clip(b, 0, self.P - 1)], -1)
            other = int((struck & (inst != own[:, None])).any(axis=1).sum())
            assert other >= 100, (lattice, dist, other)
            if dist == np.inf:
                lo, hi = np.where(struck, inst, n_inst).min(axis=1), inst.max(axis=1)
                several = int((struck.any(axis=1) & (lo != hi)).sum())
                assert several >= 100, (lattice, several)
            mixed = int((struck.any(axis=1) & escaped.any(axis=1)).sum())
            assert mixed >= 100, (lattice, dist, mixed)
            assert self.want(S_MAX, max_dist=dist)[0].max() >= 1 << 32
            assert (b[~self.lit] == -1).all() and not escaped[~self.lit].any()
        assert not np.array_equal(self.want(S_MAX, max_dist=DISTANCES[0])[0], self.want(S_MAX, max_dist=DISTANCES[1])[0])
        self.d_x = dev(self.x)

    def table(self, rays=None, hits=None, **kw):
        r, h = (self.rays, self.hits) if rays is None else (rays, hits)
        return self.tables.table_of(r, h, rays is None, **kw)

    def want(self, samples, x=None, miss_value=0, **kw):
        assert samples <= S_MAX
        b, escaped = self.table(**kw)
        return pg.reduce(b, escaped, self.x if x is None else x, miss_value, samples)

    def fused(self, samples, d_x=None, **kw):
        return run_gather(self.t, self.d_rays, self.d_hits, N_RAYS, samples, self.d_x if d_x is None else d_x, **kw)


@pytest.fixture(scope="module")
def worlds(rc, oracle):
    yield from three_shapes(World, rc, oracle)


# ---- 1: every word against the model, in the three shapes, for both reaches and both ends of miss_value -----------------------------------
@pytest.mark.parametrize("shape", ["lds", "partial", "plain"])
@pytest.mark.parametrize("max_dist", DISTANCES)
@pytest.mark.parametrize("samples", [1, 2, 5])
def test_sums_and_open_equal_the_models(worlds, shape, max_dist, samples):
    w = worlds[shape]
    for miss_value in (0, U32_MAX):
        outs = w.fused(samples, miss_value=miss_value, max_dist=max_dist)
        finish(w.t)
        want = w.want(samples, miss_value=miss_value, max_dist=max_dist)
        check(outs, want, f"{shape} S={samples} max_dist={max_dist} miss_value={miss_value}")
        sums, opened = words_of(outs[0], N_RAYS, np.uint64), words_of(outs[1], N_RAYS, np.uint32)
        assert not sums[~w.lit].any() and not opened[~w.lit].any(), "a slot whose primary ray missed gathered something"
        assert opened.max() <= samples and 0 < opened.sum() < w.lit.sum() * samples


# ---- 2: the product's own composed path, with and without the entry cull; the hit-index stage against the model -----------------------------
@pytest.mark.parametrize("shape", ["lds", "partial", "plain"])
def test_composed_product_path_gives_the_same_words(worlds, shape):
    import torch
    w = worlds[shape]
    t, n, S, dist, miss = w.t, N_RAYS, S_MAX, 1.0, 12345
    total = n * S
    before = t.get_option("entry_cull")
    try:
        for cull in (before, 2):
            t.set_option("entry_cull", cull)
            d_gr, d_gh, d_q = poisoned(total * 32), poisoned(total * 32), poisoned(total * 4)
            t.ambient_occlusion_rays_device(w.d_rays.data_ptr(), w.d_hits.data_ptr(), n, S, d_gr.data_ptr(), max_dist=dist, seed=SEED, bias=BIAS)
            t.trace_device(d_gr.data_ptr(), d_gh.data_ptr(), total, mode="closest")
            t.placed_hit_indices_device(d_gh.data_ptr(), total, d_q.data_ptr())
            outs = w.fused(S, miss_value=miss, max_dist=dist)
            torch.cuda.synchronize()
            stored = d_gr.cpu().numpy()[:total * 32].view(bm.RAY_DT)
            traced = d_gh.cpu().numpy()[:total * 32].view(bm.HIT_DT)
            q = words_of(d_q, total, np.uint32)
            # the stage against placed_hits, for the hit and the miss records of the sample trace
            assert np.array_equal(q, pg.hit_indices(w.o, traced)), f"{shape} entry_cull={cull}: rc_placed_hit_indices_device differs from placed_hits"
            # (both kinds of record are there: the World's guard has >= 100 slots with a sample on another instance at this reach)
            assert (q == pg.INVALID).sum() >= 1000 and (q != pg.INVALID).sum() >= 100 and q[q != pg.INVALID].max() < w.P
            # the composed path: the stage's indices, looked up and summed on the host
            with np.errstate(invalid="ignore"):
                live = np.repeat(w.hits["hit"] != 0, S) & (stored["tmax"] > 0)
            struck = live & (q != pg.INVALID)
            value = np.zeros(total, np.uint64)
            value[struck] = w.x[q[struck]]
            escaped = live & (traced["hit"] == 0)
            value[escaped] = miss
            composed = (value.reshape(n, S).sum(axis=1, dtype=np.uint64), escaped.reshape(n, S).sum(axis=1).astype(np.uint32))
            check(outs, composed, f"{shape} entry_cull={cull} against the composed path")
            check(outs, w.want(S, miss_value=miss, max_dist=dist), f"{shape} entry_cull={cull} against the model")
    finally:
        t.set_option("entry_cull", before)


# ---- 3: the lift identity: a field per metadata carried to the placed space gives the metadata gather's words; open is ambient occlusion's -
@pytest.mark.parametrize("shape", ["lds", "partial", "plain"])
def test_lifted_field_gives_the_metadata_gathers_words(worlds, shape):
    w = worlds[shape]
    x_meta = distinct_x(256, salt=7, with_max=True)
    lifted = pg.lift(w.o, x_meta)
    assert len(lifted) == w.P and np.array_equal(lifted[:256], lifted[256:512])
    d_meta, d_lifted = dev(x_meta), dev(lifted)
    for dist in DISTANCES:
        counts = zeroed(N_RAYS, 4)
        w.t.ambient_occlusion_device(w.d_rays.data_ptr(), w.d_hits.data_ptr(), N_RAYS, S_MAX, counts.data_ptr(), max_dist=dist, seed=SEED, bias=BIAS)
        meta_outs = w.fused(S_MAX, d_x=d_meta, miss_value=3, max_dist=dist, placed=False)
        outs = w.fused(S_MAX, d_x=d_lifted, miss_value=3, max_dist=dist)
        alone = w.fused(S_MAX, d_x=d_lifted, miss_value=3, max_dist=dist, with_open=False)
        finish(w.t)
        sums, opened = words_of(outs[0], N_RAYS, np.uint64), words_of(outs[1], N_RAYS, np.uint32)
        assert np.array_equal(sums, words_of(meta_outs[0], N_RAYS, np.uint64)), f"{shape} max_dist={dist}: sums differ from rc_final_gather_device's"
        assert np.array_equal(opened, words_of(meta_outs[1], N_RAYS, np.uint32)), f"{shape} max_dist={dist}: open differs from rc_final_gather_device's"
        assert np.array_equal(opened, words_of(counts, N_RAYS, np.uint32)), f"{shape} max_dist={dist}: open differs from rc_ambient_occlusion_device's counts"
        assert opened.any() and sums.max() >= 1 << 32
        assert np.array_equal(words_of(alone[0], N_RAYS, np.uint64), sums), "d_open = NULL changed the sums"
        check(outs, w.want(S_MAX, x=lifted, miss_value=3, max_dist=dist), f"{shape} max_dist={dist} against the model")


# ---- 4: irregular bases, a mirror and a non-uniform scale -----------------------------------------------------------------------------------
def test_irregular_bases_mirror_and_scale(rc, oracle):
    cfg = pm.mixed_cfg(rc)
    t, o = build_product(rc, cfg), build_oracle(oracle, cfg)
    try:
        base = pm.bases(o)
        assert np.array_equal(base, [0, 8, 152, 160, 304, 448, 456, 600, 640]) and np.array_equal(t.placed_primitive_bases(), base)
        n, S = 4096, 4
        rays = random_rays(rc, n, 11, -2.9, 2.9)
        hits = o.trace(rays, nthreads=8)
        assert 1000 <= hits["hit"].sum()
        x = distinct_x(640, salt=13, with_max=True)
        d_rays, d_hits, d_x = dev(rays), dev(hits), dev(x)
        for dist in DISTANCES:
            b, escaped, _ = pg.sample_table(o, rays, hits, S, seed=SEED, bias=BIAS, max_dist=dist, nthreads=8)
            if dist == np.inf:  # every one of the eight instances receives sample hits: a base indexed by BLAS, custom index or flat offset shows
                per_instance = np.bincount(np.searchsorted(base, b[b >= 0], side="right") - 1, minlength=8)
                assert per_instance.min() >= 10, per_instance
            for kernel in (3, 5):
                t.set_option("kernel", kernel)
                outs = run_gather(t, d_rays, d_hits, n, S, d_x, miss_value=9, max_dist=dist)
                finish(t)
                check(outs, pg.reduce(b, escaped, x, 9), f"mixed scene, kernel {kernel}, max_dist={dist}")
        d_q = poisoned(n * 4)
        t.placed_hit_indices_device(d_hits.data_ptr(), n, d_q.data_ptr())
        finish(t)
        check_words(d_q, pg.hit_indices(o, hits), np.uint32, "rc_placed_hit_indices_device on the primary hits of the mixed scene")
    finally:
        t.free()


# ---- 5: two plates of ONE mesh: fields that agree on every metadata value and differ per instance ---------------------------------------------
def test_two_instances_of_one_mesh_carry_different_values(rc, oracle):
    cfg = pm.plates_cfg(rc)
    t, o = build_product(rc, cfg), build_oracle(oracle, cfg)
    try:
        c = np.arange(16) / 16
        org = np.array([(u + 0.023, v + 0.038, 0.5) for u in c for v in c])  # (off the cells' centres: no ray through a triangle's edge)
        rays = rc.scenes.make_rays(np.concatenate([org, org]), np.concatenate([np.tile([0.0, 0, -1], (256, 1)), np.tile([0.0, 0, 1], (256, 1))]))
        hits = o.trace(rays, nthreads=4)
        n, S = len(rays), 5
        assert hits["hit"].all() and set(hits["instance_id"].tolist()) == {0, 1}
        b, escaped, _ = pg.sample_table(o, rays, hits, S, seed=SEED, bias=BIAS, nthreads=4)
        assert ((b >= 0) & (b < 8)).sum() >= 100 and (b >= 8).sum() >= 100 and escaped.sum() >= 100
        floor_lit = np.concatenate([np.full(8, 1000, np.uint32), np.zeros(8, np.uint32)])    # per metadata both fields hold {1000, 0}:
        ceiling_lit = np.concatenate([np.zeros(8, np.uint32), np.full(8, 1000, np.uint32)])  # no metadata field separates them
        d_rays, d_hits = dev(rays), dev(hits)
        got = []
        for x in (floor_lit, ceiling_lit):
            outs = run_gather(t, d_rays, d_hits, n, S, dev(x), miss_value=1)
            finish(t)
            check(outs, pg.reduce(b, escaped, x, 1), "plates")
            got.append(words_of(outs[0], n, np.uint64).copy())
        assert not np.array_equal(got[0], got[1])
        assert got[0][:256].max() <= S and got[0][256:].max() >= 1000  # the lit floor is seen from the ceiling only, and the other way round
        assert got[1][256:].max() <= S and got[1][:256].max() >= 1000
    finally:
        t.free()


# ---- 6: accumulation over depths, and samples keyed by path ids -----------------------------------------------------------------------------
def test_accumulation_and_path_ids(worlds):
    w = worlds["lds"]
    outs = w.fused(2, depth=0, seed=SEED, miss_value=5)
    w.fused(2, outs=outs, depth=1, seed=SEED + 1, miss_value=5)
    finish(w.t)
    d0, d1 = w.want(2, depth=0, miss_value=5), w.want(2, depth=1, seed=SEED + 1, miss_value=5)
    assert not np.array_equal(d0[0], d1[0])  # another seed and depth draw other samples
    check(outs, (d0[0] + d1[0], d0[1] + d1[1]), "seed, depth 0 + seed + 1, depth 1 into one pair of buffers")
    # a permuted, compacted queue: the lit slots only, shuffled, each with its path id -- the result is the permuted result
    lit = np.nonzero(w.lit)[0]
    perm = np.random.default_rng(5).permutation(lit).astype(np.uint32)
    k = len(perm)
    assert perm.min() >= 3  # (perm - 3 below stays a u32)
    q_rays, q_hits, q_paths = dev(w.rays[perm]), dev(w.hits[perm]), dev(perm)  # (held: the launches read them after the calls return)
    outs = run_gather(w.t, q_rays, q_hits, k, 2, w.d_x, d_path_in=q_paths.data_ptr(), miss_value=5)
    finish(w.t)
    check(outs, tuple(a[perm] for a in d0), "a compacted queue with d_path_in")
    shifted = dev(perm - np.uint32(3))
    outs = run_gather(w.t, q_rays, q_hits, k, 2, w.d_x, d_path_in=shifted.data_ptr(), path_base=3, miss_value=5)
    finish(w.t)
    check(outs, tuple(a[perm] for a in d0), "d_path_in - 3 with path_base = 3")


# ---- 7: empty work and refusals -----------------------------------------------------------------------------------------------------------
def test_empty_work_and_argument_checks(rc, worlds):
    import torch
    from raycore_jl_amd._capi import lib
    w = worlds["lds"]
    f, g, h = lib().rc_placed_final_gather_device, lib().rc_placed_hit_indices_device, w.t._h
    out, opened, idx = poisoned(4096), poisoned(4096), poisoned(4096)
    r, hh, xp, op, pp, qp = w.d_rays.data_ptr(), w.d_hits.data_ptr(), w.d_x.data_ptr(), out.data_ptr(), opened.data_ptr(), idx.data_ptr()
    INV, NS = 1, 6

    def call(scene=h, rays=r, hits=hh, n=16, samples=4, max_dist=np.inf, depth=0, x=xp, o=op, p=pp):
        return f(scene, rays, hits, n, samples, max_dist, SEED, depth, None, 0, BIAS, x, 7, o, p, None)

    def untouched():
        torch.cuda.synchronize()
        return bool((out == POISON).all()) and bool((opened == POISON).all()) and bool((idx == POISON).all())

    assert call(n=0) == 0 and call(samples=0) == 0
    assert call(rays=None, hits=None, n=0, x=None, o=None, p=None) == 0  # no work: nothing is read
    assert call(rays=None, hits=None, samples=0, x=None, o=None, p=None) == 0
    assert g(h, hh, 0, qp, None) == 0
    assert untouched(), "a call without work wrote to an output"
    assert call(scene=None) == INV
    assert call(rays=None) == INV
    assert call(hits=None) == INV
    assert call(x=None) == INV
    assert call(o=None) == INV
    assert call(n=1 << 30, samples=4) == INV               # n * samples == 2^32
    assert call(n=(1 << 32) // 5 + 1, samples=5) == INV    # the first n past it for S = 5
    assert call(n=1 << 63, samples=2) == INV               # (a product that wraps in 64 bits)
    assert call(n=1 << 32, samples=1) == INV
    assert call(samples=65536) == INV
    assert call(depth=65536) == INV
    for bad in (0.0, -0.0, -1.0, -np.inf, np.nan):
        assert call(max_dist=bad) == INV, bad
    assert g(None, hh, 16, qp, None) == INV and g(h, None, 16, qp, None) == INV and g(h, hh, 16, None, None) == INV
    assert g(h, None, 0, qp, None) == INV and g(h, hh, 0, None, None) == INV  # rc_hit_points_device's rule: NULL is refused with n == 0 too
    assert untouched(), "a refused call wrote to an output"
    u = build_product(rc, rc.scenes.config_c1())
    u.push_instances(1, rc.scenes.IDENTITY3x4[None], np.zeros(1, np.uint32))  # a pending mutation
    assert call(scene=u._h) == NS and g(u._h, hh, 16, qp, None) == NS
    u.free()
    assert untouched()


# ---- 8: captured, with x overwritten in place between replays -----------------------------------------------------------------------------
def test_captured_call_follows_the_new_x(worlds):
    import torch
    w = worlds["partial"]
    t, S = w.t, 2
    s = torch.cuda.Stream()
    d_x = dev(w.x)  # the captured call's own buffer
    outs = (zeroed(N_RAYS, 8), zeroed(N_RAYS, 4))

    def launch():
        run_gather(t, w.d_rays, w.d_hits, N_RAYS, S, d_x, outs=outs, miss_value=9, stream=s.cuda_stream)

    torch.cuda.synchronize()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launch()  # the eager call the capture needs
    torch.cuda.synchronize()
    check(outs, w.want(S, miss_value=9), "eager call")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launch()
    x2 = distinct_x(w.P, salt=11, with_max=True)
    assert not np.array_equal(w.want(S, x=x2, miss_value=9)[0], w.want(S, miss_value=9)[0])
    for x, what in ((w.x, "replay"), (x2, "replay after x was overwritten in place")):
        d_x.copy_(dev(x))  # in place: the graph holds the tensor's address
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            outs[0][:N_RAYS * 8] = 0  # the call accumulates: zeroed in the graph's stream before each replay
            outs[1][:N_RAYS * 4] = 0
            g.replay()
        torch.cuda.synchronize()
        check(outs, w.want(S, x=x, miss_value=9), what)
    t.wait_for_gpu()
    del g
    torch.cuda.synchronize()
    t.set_option("release_captures", 1)  # the graph is gone: hand its captured launch back
    assert t.get_option("release_captures") == 0


# ---- 9: behind a device-side transform update and refit on the same stream, no host wait ---------------------------------------------------
def test_follows_a_device_side_update(rc, oracle, worlds):
    import torch
    w = worlds["lds"]
    cfg = dict(w.cfg)
    b, xf, ids = cfg["instances"][0]
    moved = np.array(xf, np.float32).reshape(len(xf), 3, 4).copy()
    moved[:, :, 3] += np.random.default_rng(8).uniform(-0.3, 0.3, size=(len(xf), 3)).astype(np.float32)
    moved = moved.reshape(len(xf), 12)
    cfg2 = dict(cfg, instances=[(b, moved, ids)])
    t, o2 = build_product(rc, cfg), build_oracle(oracle, cfg2)  # the product starts from the old transforms, the oracle has the new ones
    try:
        hits2 = o2.trace(w.rays, nthreads=16)  # the moved scene's primary hits
        lit2 = hits2["hit"] == 1
        assert lit2.sum() >= 1000 and not np.array_equal(hits2["hit"], w.hits["hit"])
        assert np.array_equal(pm.bases(o2), w.tables.base)  # a move keeps every base
        b2, escaped2, _ = pg.sample_table(o2, w.rays, hits2, 2, seed=SEED, bias=BIAS)
        want = pg.reduce(b2, escaped2, w.x, 4)
        old = pg.sample_table(w.o, w.rays, hits2, 2, seed=SEED, bias=BIAS)[:2]  # (the same records gathered in the scene before the move)
        assert not np.array_equal(pg.reduce(*old, w.x, 4)[0], want[0])
        s = torch.cuda.Stream()
        d_xf, d_hits2 = torch.from_numpy(moved).cuda(), dev(hits2)
        outs = (zeroed(N_RAYS, 8), zeroed(N_RAYS, 4))
        d_q = poisoned(N_RAYS * 4)
        torch.cuda.synchronize()
        t.update_transforms_device(t.handles[0], d_xf, stream=s.cuda_stream)
        t.refit_device_async(stream=s.cuda_stream)
        run_gather(t, w.d_rays, d_hits2, N_RAYS, 2, w.d_x, outs=outs, miss_value=4, stream=s.cuda_stream)
        t.placed_hit_indices_device(d_hits2.data_ptr(), N_RAYS, d_q.data_ptr(), stream=s.cuda_stream)
        finish(t)
        check(outs, want, "behind update_transforms_device + refit_device_async")
        check_words(d_q, pg.hit_indices(o2, hits2), np.uint32, "rc_placed_hit_indices_device behind the update")
    finally:
        t.free()


# ---- 10: two streams at once, a different x on each -----------------------------------------------------------------------------------------
def test_two_streams_at_once(worlds):
    import torch
    w = worlds["lds"]
    xs, S = (w.x, distinct_x(w.P, salt=21, with_max=True)), 2
    d_xs = [dev(x) for x in xs]
    streams = [torch.cuda.Stream() for _ in xs]
    outs = [[(zeroed(N_RAYS, 8), zeroed(N_RAYS, 4)) for _ in range(3)] for _ in xs]
    torch.cuda.synchronize()  # the buffers are filled on the current stream: done before the other streams write them
    for rep in range(3):  # enqueued alternately, never waited for in between
        for k in range(2):
            w.fused(S, d_x=d_xs[k], outs=outs[k][rep], miss_value=k, stream=streams[k].cuda_stream)
    finish(w.t)
    assert not np.array_equal(w.want(S, x=xs[0])[0], w.want(S, x=xs[1])[0])
    for k in range(2):
        for rep in range(3):
            check(outs[k][rep], w.want(S, x=xs[k], miss_value=k), f"stream {k} launch {rep}")


# ---- 11: the placed final-gather stage of WavefrontPaths ------------------------------------------------------------------------------------
def test_wavefront_placed_final_gather(rc, worlds):
    import torch
    w = worlds["partial"]  # (the dense lattice: enough paths survive the first bounce)
    t, cfg = w.t, w.cfg
    width, height, spp, depth, seed, S, dist, miss = 64, 48, 2, 2, 0x5AD0, 4, 2.0, 77
    cam = rc.wavefront.lookat_camera(cfg["eye"], cfg["lattice_centre"], width, height, 45.0)
    n = width * height * spp
    s = torch.cuda.Stream()
    d_x = torch.from_numpy(w.x.view(np.int32).copy()).cuda()
    x_meta = distinct_x(256, salt=3, with_max=True)
    d_meta = torch.from_numpy(x_meta.view(np.int32).copy()).cuda()
    wf = rc.wavefront.WavefrontPaths(t, width, height, spp, depth, cam, cfg["light"], seed=seed)
    assert wf.gather_placed is False and wf.gather_samples == 0
    n_buffers = len(wf.buffers())
    for bad in (w.x, d_x.to(torch.int64), d_x[:100], d_x.cpu(), d_meta):  # (d_meta: n_primitives words, not P)
        with pytest.raises(ValueError):
            wf.with_placed_final_gather(bad, S)
    with pytest.raises(ValueError):
        wf.with_final_gather(d_x, S)  # P words where the metadata stage wants n_primitives
    assert wf.with_placed_final_gather(d_x, 0) is wf and wf.gather_sums == [] and wf.gather_placed is False and len(wf.buffers()) == n_buffers
    assert wf.with_placed_final_gather(d_x, S, dist, miss) is wf
    assert (wf.gather_samples, wf.gather_distance, wf.gather_miss, wf.gather_placed) == (S, dist, miss, True) and wf.gather_x is d_x
    assert len(wf.gather_sums) == len(wf.gather_open) == depth
    assert all(c.numel() == n and c.dtype == torch.int64 for c in wf.gather_sums) and all(c.numel() == n and c.dtype == torch.int32 for c in wf.gather_open)
    assert wf.traced_rays() == n * 2 * depth + n * S * depth
    assert len(wf.buffers()) == n_buffers + 2 * depth + 1 and all(any(c is b for b in wf.buffers()) for c in wf.gather_sums + wf.gather_open + [d_x])

    def check_frame(what, model, x):
        live = []
        for b in range(depth):
            rays, hits = wf.rays[b].cpu().numpy().view(bm.RAY_DT), wf.hits[b].cpu().numpy().view(bm.HIT_DT)
            paths = wf.path_ids[b].cpu().numpy().view(np.uint32)
            want = model.expected(w.o, rays, hits, x, S, miss, seed=seed, depth=b, bias=wf.bias, max_dist=dist, path_in=paths)
            got = (wf.gather_sums[b].cpu().numpy().view(np.uint64), wf.gather_open[b].cpu().numpy().view(np.uint32))
            for g, wnt, name in zip(got, want, ("sums", "open")):
                bad = np.nonzero(g != wnt)[0]
                assert len(bad) == 0, f"{what} depth {b}: {len(bad)} {name} differ, first {bad[:5]}: got {g[bad[:5]]} want {wnt[bad[:5]]}"
            lit = hits["hit"] == 1
            assert 0 < got[1][lit].sum() < lit.sum() * S and got[0].max() >= 1 << 32, (what, b)
            live.append(int(lit.sum()))
        return live

    s.wait_stream(torch.cuda.current_stream())
    wf.run(s)  # (not made current: the frame zeroes its sums on the stream it is given)
    torch.cuda.synchronize()
    live = check_frame("eager, placed", pg, w.x)
    assert live[0] >= 1000 and live[1] >= 20, live
    # one gather stage per frame, the last switch wins: to the metadata stage and back
    wf.with_final_gather(d_meta, S, dist, miss)
    assert wf.gather_placed is False and wf.gather_x is d_meta
    wf.run(s)
    torch.cuda.synchronize()
    assert check_frame("eager, metadata", gm, x_meta) == live
    wf.with_placed_final_gather(d_x, S, dist, miss)
    assert wf.gather_placed is True
    wf.run(s)
    torch.cuda.synchronize()
    assert check_frame("eager, placed again", pg, w.x) == live
    wf.capture(s)
    for c in wf.gather_sums + wf.gather_open:
        c.fill_(0x7B)  # the replayed frame zeroes them itself
    x2 = distinct_x(w.P, salt=31, with_max=True)
    d_x.copy_(torch.from_numpy(x2.view(np.int32).copy()).cuda())  # held by reference: the replay reads the new solution
    torch.cuda.synchronize()
    wf.replay()
    torch.cuda.synchronize()
    assert check_frame("replay with a new x", pg, x2) == live
    with pytest.raises(rc.RaycoreError):
        wf.with_placed_final_gather(d_x, 0)  # a captured frame keeps its stages
    t.wait_for_gpu()
    del wf
    torch.cuda.synchronize()
    t.set_option("release_captures", 1)
    assert t.get_option("release_captures") == 0


# ---- 12: the host calls ----------------------------------------------------------------------------------------------------------------------
def test_host_placed_final_gather_and_hit_indices(rc, worlds):
    w = worlds["lds"]
    for dist in DISTANCES:
        sums, opened = rc.placed_final_gather(w.t, w.rays, w.hits, w.x, S_MAX, max_dist=dist, miss_value=17, seed=SEED, bias=BIAS)
        assert sums.dtype == np.uint64 and opened.dtype == np.uint32 and sums.shape == opened.shape == (N_RAYS,)
        want = w.want(S_MAX, miss_value=17, max_dist=dist)
        assert np.array_equal(sums, want[0]) and np.array_equal(opened, want[1])
        assert np.array_equal(opened, rc.ambient_occlusion(w.t, w.rays, w.hits, S_MAX, max_dist=dist, seed=SEED, bias=BIAS))
    sums, opened = rc.placed_final_gather(w.t, w.rays[:0], w.hits[:0], w.x, 4)
    assert sums.shape == opened.shape == (0,)
    with pytest.raises(ValueError):
        rc.placed_final_gather(w.t, w.rays, w.hits[:5], w.x, 4)
    with pytest.raises(ValueError, match="placed primitive"):
        rc.placed_final_gather(w.t, w.rays, w.hits, w.x[:-1], 4)  # one value per placed primitive
    with pytest.raises(ValueError, match="placed primitive"):
        rc.placed_final_gather(w.t, w.rays, w.hits, w.x[:256], 4)  # (a field per metadata is not one)
    assert rc.placed_primitive_count(w.t) == w.P
    q = rc.placed_hit_indices(w.t, w.hits)
    assert q.dtype == np.uint32 and q.shape == (N_RAYS,) and np.array_equal(q, pg.hit_indices(w.o, w.hits))
    assert (q[~w.lit] == pg.INVALID).all() and q[w.lit].max() < w.P
    assert rc.placed_hit_indices(w.t, w.hits[:0]).shape == (0,)


def test_host_placed_irradiance(rc, worlds):
    """The one float case.  placed_irradiance() quantises b and the sky with floor under one scale (irradiance_scale, unchanged), so every
    sample's value is its float value less at most one step, 1 / scale = max(max b, sky) / (2^32 - 1); the mean of S such values is the
    float mean less at most one step.  The float mean itself is computed here in float64 from the model's sample table; its own rounding
    (S additions of values <= 4: below 1e-14) is far inside the step (about 9e-10), so the bound asserted is the step alone."""
    w = worlds["lds"]
    g = np.random.default_rng(17)
    b = g.uniform(0.0, 3.0, w.P)
    b[:4] = (0.0, 3.0, 1.5, 1e-12)
    for sky, dist in ((4.0, np.inf), (0.25, 1.0), (0.0, np.inf)):
        scale = (2 ** 32 - 1) / max(b.max(), sky)
        step = 1.0 / scale
        idx, escaped = w.table(max_dist=dist)
        value = np.where(escaped, sky, 0.0)
        value[idx >= 0] = b[idx[idx >= 0]]
        want = value.sum(axis=1) / S_MAX
        got, opened = rc.placed_irradiance(w.t, w.rays, w.hits, b, S_MAX, sky=sky, max_dist=dist, seed=SEED, bias=BIAS, return_open=True)
        assert got.dtype == np.float64 and got.shape == (N_RAYS,)
        err = want - got
        print(f"placed_irradiance sky={sky} max_dist={dist}: step {step:.3e}, error min {err.min():.3e} max {err.max():.3e}")
        assert np.all(np.abs(err) <= step), (sky, dist, float(np.abs(err).max()), step)
        assert not got[~w.lit].any() and got[w.lit].max() > 0.5
        assert np.array_equal(opened, w.want(S_MAX, max_dist=dist)[1])
        assert np.array_equal(got, rc.placed_irradiance(w.t, w.rays, w.hits, b, S_MAX, sky=sky, max_dist=dist, seed=SEED, bias=BIAS))
