"""rc_final_gather_device on the GPU: the sum of a per-primitive field over the closest hits of all hits x hemisphere samples in one
traversal launch, word for word against the numpy model (tests/gather_model.py: ao_model's rays, the CPU oracle's closest-hit trace, the
oracle's metadata), in the three kernel shapes the launcher dispatches (top level in LDS, partial LDS, plain) and for an unbounded and a
short reach; against the product's own composed path (rc_ambient_occlusion_rays_device + closest-hit trace + a host reduction, also with
the entry cull on); its open counts against rc_ambient_occlusion_device; a furnace; accumulation and path ids; metadata with gaps,
duplicates, 0 and N + 50; empty work and bad arguments; a captured call whose inputs are exchanged between replays; two streams at once;
behind a device-side transform update; as a stage of WavefrontPaths; on a hostile scene with NaN hit frames; and through the host calls.

Every integer comparison is exact and covers every slot.  The worlds are the ambient-occlusion file's: C3 with 16 x 9 fan spheres on the
lattices (3,3,2) and (7,7,6) -- ONE 256-triangle BLAS under 18 and 294 instances, so every case on them is also the instanced case: the
same x word is read through many instances -- and 63 997 rays, so n * S ends inside a chunk."""
import numpy as np
import pytest

import bounce_model as bm
import gather_model as gm
from gpu_kit import POISON, check_words, dev, finish, poisoned, words_of, zeroed
from gpu_kit import rc  # noqa: F401
from helpers import build_oracle, build_product
from scene_kit import distinct_x, meta, room_cfg
from worlds import C3World, three_shapes

pytestmark = pytest.mark.gpu

BIAS = 1e-3
N_RAYS = 63_997  # 320 x 200 less three: n * S ends inside a 128-item chunk for S = 2 and 5 (remainders 122 and 113)
SEED = 0xA0
S_MAX = 5
DISTANCES = (np.inf, 1.0)
U32_MAX = gm.U32_MAX


def check(outs, want, what):
    """outs: (sums tensor, open tensor or None) of a call; want: (sums u64, open u32) of the model."""
    for out, w, dtype, name in ((outs[0], want[0], np.uint64, "sums"), (outs[1], want[1], np.uint32, "open")):
        if out is not None:
            check_words(out, w, dtype, f"{what} ({name})")


def run_gather(t, d_rays, d_hits, n, samples, d_x, outs=None, with_open=True, miss_value=0, max_dist=np.inf, seed=SEED, depth=0, d_path_in=None,
               path_base=0, stream=None):
    """One call into zeroed, guarded outputs (or into `outs`); returns (sums tensor, open tensor or None)."""
    if outs is None:
        outs = (zeroed(n, 8), zeroed(n, 4) if with_open else None)
    t.final_gather_device(d_rays.data_ptr(), d_hits.data_ptr(), n, samples, d_x.data_ptr(), outs[0].data_ptr(),
                          outs[1].data_ptr() if outs[1] is not None else None, miss_value=miss_value, max_dist=max_dist, seed=seed, depth=depth,
                          bias=BIAS, d_path_in=d_path_in, path_base=path_base, stream=stream)
    return outs


class World(C3World):
    def __init__(self, rc, oracle, lattice, kernel=None):
        super().__init__(rc, oracle, lattice, kernel)
        self.prim_meta = self.o.blas_prims["meta"]
        self.n_prims = len(self.prim_meta)
        assert self.n_prims == self.t.n_primitives() == 256 and self.prim_meta.min() >= 1 and self.prim_meta.max() <= self.n_prims
        self.x = distinct_x(self.n_prims, with_max=True)
        self._tables = {}
        # a degenerate input cannot pass -- all from the oracle alone, before anything is compared: (enough hits and misses;) at the
        # unbounded reach enough slots whose samples land on two or more different primitives' metadata; at either reach enough slots
        # with a sample that hits and a sample that escapes; sums that pass 2^32; and a reach that matters
        for dist in DISTANCES:
            meta, escaped = self.table(max_dist=dist)
            mixed = int(((meta >= 1).any(axis=1) & escaped.any(axis=1)).sum())
            assert mixed >= 100, (lattice, dist, mixed)
            if dist == np.inf:
                srt = np.sort(np.where(meta >= 1, meta, 0), axis=1)  # (distinct positive values per row = the steps of the sorted row, a leading 0 aside)
                several = int((((np.diff(srt, axis=1) != 0) & (srt[:, :-1] != 0)).sum(axis=1) >= 1).sum())
                assert several >= 100, (lattice, several)
            assert self.want(S_MAX, max_dist=dist)[0].max() >= 1 << 32
            assert (meta[~self.lit] == -1).all() and not escaped[~self.lit].any()
        assert not np.array_equal(self.want(S_MAX, max_dist=DISTANCES[0])[0], self.want(S_MAX, max_dist=DISTANCES[1])[0])
        self.d_x = dev(self.x)

    def table(self, max_dist=np.inf, seed=SEED, depth=0, path_in=None, path_base=0, rays=None, hits=None):
        """(meta, escaped), (n, S_MAX) each, from the oracle alone; computed once per argument set and read-only.  A sample does not
        depend on `samples`, so every S <= S_MAX reads the first S columns."""
        key = (float(max_dist), seed, depth, None if path_in is None else np.asarray(path_in).tobytes(), path_base, rays is None)
        if key not in self._tables:
            r, h = (self.rays, self.hits) if rays is None else (rays, hits)
            meta, escaped, _ = gm.sample_table(self.o, r, h, S_MAX, seed=seed, depth=depth, bias=BIAS, max_dist=max_dist, path_in=path_in, path_base=path_base)
            meta.setflags(write=False)
            escaped.setflags(write=False)
            self._tables[key] = (meta, escaped)
        return self._tables[key]

    def want(self, samples, x=None, miss_value=0, **kw):
        assert samples <= S_MAX
        meta, escaped = self.table(**kw)
        return gm.reduce(meta, escaped, self.x if x is None else x, miss_value, samples)

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


# ---- 2: the product's own composed path, with and without the entry cull -----------------------------------------------------------------
@pytest.mark.parametrize("shape", ["lds", "partial", "plain"])
def test_composed_product_path_gives_the_same_words(worlds, shape):
    import torch
    w = worlds[shape]
    t, n, S, dist, miss = w.t, N_RAYS, S_MAX, 1.0, 12345
    total = n * S
    prim_meta = t.adapt().all_blas_prims["meta"]
    before = t.get_option("entry_cull")
    try:
        for cull in (before, 2):
            t.set_option("entry_cull", cull)
            d_gr, d_gh = poisoned(total * 32), poisoned(total * 32)
            t.ambient_occlusion_rays_device(w.d_rays.data_ptr(), w.d_hits.data_ptr(), n, S, d_gr.data_ptr(), max_dist=dist, seed=SEED, bias=BIAS)
            t.trace_device(d_gr.data_ptr(), d_gh.data_ptr(), total, mode="closest")
            outs = w.fused(S, miss_value=miss, max_dist=dist)
            torch.cuda.synchronize()
            stored = d_gr.cpu().numpy()[:total * 32].view(bm.RAY_DT)
            table = gm.sample_table_of(prim_meta, w.hits, stored, d_gh.cpu().numpy()[:total * 32].view(bm.HIT_DT), S)
            check(outs, gm.reduce(*table, w.x, miss), f"{shape} entry_cull={cull} against the composed path")
            check(outs, w.want(S, miss_value=miss, max_dist=dist), f"{shape} entry_cull={cull} against the model")
    finally:
        t.set_option("entry_cull", before)


# ---- 3: open is ambient occlusion's count; without d_open the sums are the same -------------------------------------------------------------
@pytest.mark.parametrize("shape", ["lds", "partial", "plain"])
def test_open_is_ambient_occlusion_and_optional(worlds, shape):
    w = worlds[shape]
    for dist in DISTANCES:
        counts = zeroed(N_RAYS, 4)
        w.t.ambient_occlusion_device(w.d_rays.data_ptr(), w.d_hits.data_ptr(), N_RAYS, S_MAX, counts.data_ptr(), max_dist=dist, seed=SEED, bias=BIAS)
        outs = w.fused(S_MAX, miss_value=3, max_dist=dist)
        alone = w.fused(S_MAX, miss_value=3, max_dist=dist, with_open=False)
        finish(w.t)
        ao = words_of(counts, N_RAYS, np.uint32)
        assert np.array_equal(words_of(outs[1], N_RAYS, np.uint32), ao), f"{shape} max_dist={dist}: open differs from rc_ambient_occlusion_device's counts"
        assert ao.any()
        assert np.array_equal(words_of(alone[0], N_RAYS, np.uint64), words_of(outs[0], N_RAYS, np.uint64)), "d_open = NULL changed the sums"
        check(alone, w.want(S_MAX, miss_value=3, max_dist=dist), f"{shape} max_dist={dist} without d_open")


# ---- 4, 6: a closed room -- the furnace, and metadata with gaps, duplicates, 0 and N + 50 -------------------------------------------------


class Room:
    """The closed room of tests/test_gpu_view_factor_products.py (a sphere inside a box, 192 triangles, one instance) seen from 6007 points
    inside it: every primary ray hits, and so does every sample."""

    def __init__(self, rc, oracle, metadata=None):
        cfg = room_cfg(rc, metadata)
        self.t, self.o = build_product(rc, cfg), build_oracle(oracle, cfg)
        self.n_prims = self.t.n_primitives()
        assert self.n_prims == 192
        g = np.random.default_rng(0xF0)
        org = g.uniform(-1.4, 1.4, size=(9000, 3))
        org = org[np.linalg.norm(org, axis=1) > 0.6][:6007]
        assert len(org) == 6007
        d = g.normal(size=(len(org), 3))
        self.rays = rc.scenes.make_rays(org, d / np.linalg.norm(d, axis=1, keepdims=True))
        self.hits = self.o.trace(self.rays, nthreads=8)
        self.n = len(self.rays)
        assert self.hits["hit"].all()
        self.meta, self.escaped, _ = gm.sample_table(self.o, self.rays, self.hits, S_MAX, seed=SEED, bias=BIAS, nthreads=8)
        assert not self.escaped.any() and (self.meta >= 0).all()  # closed: every sample of every slot hits
        self.d_rays, self.d_hits = dev(self.rays), dev(self.hits)


@pytest.mark.parametrize("kernel", [3, 5, 6])
def test_furnace(rc, oracle, kernel):
    """x = c everywhere inside a closed room: every sample brings c home, whatever it hits -- sums == S * c and open == 0, exactly."""
    r = Room(rc, oracle)
    try:
        assert (r.meta >= 1).all() and (r.meta <= r.n_prims).all()
        r.t.set_option("kernel", kernel)
        for c in (1, 0xDEADBEEF, U32_MAX):
            d_c = dev(np.full(r.n_prims, c, np.uint32))
            outs = run_gather(r.t, r.d_rays, r.d_hits, r.n, S_MAX, d_c)
            finish(r.t)
            assert (words_of(outs[0], r.n, np.uint64) == np.uint64(S_MAX * c)).all(), c
            assert not words_of(outs[1], r.n, np.uint32).any()
    finally:
        r.t.free()


def test_metadata_gaps_duplicates_and_out_of_range(rc, oracle):
    r = Room(rc, oracle, meta)
    try:
        n = r.n_prims
        assert (r.meta == 0).sum() >= 100 and (r.meta == n + 50).sum() >= 10 and (r.meta == 7).sum() >= 100  # samples that land on each kind
        x = distinct_x(n, salt=3, with_max=True)
        want = gm.reduce(r.meta, r.escaped, x, 99)
        dropped = ((r.meta == 0) | (r.meta == n + 50)).sum(axis=1)
        ones = gm.reduce(r.meta, r.escaped, np.ones(n, np.uint32))[0]
        assert np.array_equal(ones + dropped.astype(np.uint64), np.full(r.n, S_MAX, np.uint64)) and not want[1].any()
        d_x = dev(x)
        for kernel in (3, 5, 6):
            r.t.set_option("kernel", kernel)
            outs = run_gather(r.t, r.d_rays, r.d_hits, r.n, S_MAX, d_x, miss_value=99)
            finish(r.t)
            check(outs, want, f"kernel {kernel}")
    finally:
        r.t.free()


# ---- 5: accumulation over depths, and samples keyed by path ids -----------------------------------------------------------------------------
def test_accumulation_and_path_ids(worlds):
    w = worlds["lds"]
    outs = w.fused(2, depth=0, miss_value=5)
    w.fused(2, outs=outs, depth=1, miss_value=5)
    finish(w.t)
    d0, d1 = w.want(2, depth=0, miss_value=5), w.want(2, depth=1, miss_value=5)
    assert not np.array_equal(d0[0], d1[0])  # another depth draws other samples
    check(outs, (d0[0] + d1[0], d0[1] + d1[1]), "depth 0 + depth 1 into one pair of buffers")
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
    based = w.want(2, path_base=7, miss_value=5)
    assert not np.array_equal(based[0], d0[0])
    outs = w.fused(2, path_base=7, miss_value=5)
    finish(w.t)
    check(outs, based, "path_base = 7")


# ---- 7: empty work and refusals -----------------------------------------------------------------------------------------------------------
def test_empty_work_and_argument_checks(rc, worlds):
    import torch
    from raycore_jl_amd._capi import lib
    w = worlds["lds"]
    f, h = lib().rc_final_gather_device, w.t._h
    out, opened = poisoned(4096), poisoned(4096)
    r, hh, xp, op, pp = w.d_rays.data_ptr(), w.d_hits.data_ptr(), w.d_x.data_ptr(), out.data_ptr(), opened.data_ptr()
    INV, NS = 1, 6

    def call(scene=h, rays=r, hits=hh, n=16, samples=4, max_dist=np.inf, depth=0, x=xp, o=op, p=pp):
        return f(scene, rays, hits, n, samples, max_dist, SEED, depth, None, 0, BIAS, x, 7, o, p, None)

    def untouched():
        torch.cuda.synchronize()
        return bool((out == POISON).all()) and bool((opened == POISON).all())

    assert call(n=0) == 0 and call(samples=0) == 0
    assert call(rays=None, hits=None, n=0, x=None, o=None, p=None) == 0  # no work: nothing is read
    assert call(rays=None, hits=None, samples=0, x=None, o=None, p=None) == 0
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
    assert untouched(), "a refused call wrote to an output"
    u = build_product(rc, rc.scenes.config_c1())
    u.push_instances(1, rc.scenes.IDENTITY3x4[None], np.zeros(1, np.uint32))  # a pending mutation
    assert call(scene=u._h) == NS
    u.free()
    assert untouched()


# ---- 8: captured, with x, the rays and the hits exchanged in place between replays ---------------------------------------------------------
def test_captured_call_follows_its_inputs(worlds):
    import torch
    w = worlds["partial"]
    t, S = w.t, 2
    s = torch.cuda.Stream()
    d_rays, d_hits, d_x = dev(w.rays), dev(w.hits), dev(w.x)  # the captured call's own buffers
    outs = (zeroed(N_RAYS, 8), zeroed(N_RAYS, 4))

    def launch():
        run_gather(t, d_rays, d_hits, N_RAYS, S, d_x, outs=outs, miss_value=9, stream=s.cuda_stream)

    torch.cuda.synchronize()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launch()  # the eager call the capture needs
    torch.cuda.synchronize()
    check(outs, w.want(S, miss_value=9), "eager call")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launch()
    rays2, hits2 = np.ascontiguousarray(w.rays[::-1]), np.ascontiguousarray(w.hits[::-1])  # another frame: the same view, slots reversed
    x2 = distinct_x(w.n_prims, salt=11, with_max=True)
    want2 = w.want(S, x=x2, miss_value=9, rays=rays2, hits=hits2)
    assert not np.array_equal(want2[0], w.want(S, miss_value=9)[0]) and not np.array_equal(want2[0], w.want(S, x=x2, miss_value=9)[0][::-1])
    for rays, hits, x, want, what in ((w.rays, w.hits, w.x, w.want(S, miss_value=9), "replay"),
                                      (rays2, hits2, x2, want2, "replay after x, the rays and the hits were overwritten in place")):
        d_rays.copy_(dev(rays))  # in place: the graph holds the tensors' addresses
        d_hits.copy_(dev(hits))
        d_x.copy_(dev(x))
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            outs[0][:N_RAYS * 8] = 0  # the call accumulates: zeroed in the graph's stream before each replay
            outs[1][:N_RAYS * 4] = 0
            g.replay()
        torch.cuda.synchronize()
        check(outs, want, what)
    t.wait_for_gpu()
    del g
    torch.cuda.synchronize()
    t.set_option("release_captures", 1)  # the graph is gone: hand its captured launch back
    assert t.get_option("release_captures") == 0


# ---- 9: two streams at once, a different x on each -----------------------------------------------------------------------------------------
def test_two_streams_at_once(worlds):
    import torch
    w = worlds["lds"]
    xs, S = (w.x, distinct_x(w.n_prims, salt=21, with_max=True)), 2
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


# ---- 10: behind a device-side transform update and refit on the same stream, no host wait ---------------------------------------------------
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
        meta2, escaped2, _ = gm.sample_table(o2, w.rays, hits2, 2, seed=SEED, bias=BIAS)
        want = gm.reduce(meta2, escaped2, w.x, 4)
        old = gm.sample_table(w.o, w.rays, hits2, 2, seed=SEED, bias=BIAS)[:2]  # (the same records gathered in the scene before the move)
        assert not np.array_equal(gm.reduce(*old, w.x, 4)[0], want[0])
        s = torch.cuda.Stream()
        d_xf, d_hits2 = torch.from_numpy(moved).cuda(), dev(hits2)
        outs = (zeroed(N_RAYS, 8), zeroed(N_RAYS, 4))
        torch.cuda.synchronize()
        t.update_transforms_device(t.handles[0], d_xf, stream=s.cuda_stream)
        t.refit_device_async(stream=s.cuda_stream)
        run_gather(t, w.d_rays, d_hits2, N_RAYS, 2, w.d_x, outs=outs, miss_value=4, stream=s.cuda_stream)
        finish(t)
        check(outs, want, "behind update_transforms_device + refit_device_async")
    finally:
        t.free()


# ---- 11: the final-gather stage of WavefrontPaths -----------------------------------------------------------------------------------------
def test_wavefront_final_gather(rc, worlds):
    import torch
    w = worlds["partial"]  # (the dense lattice: enough paths survive the first bounce)
    t, cfg = w.t, w.cfg
    width, height, spp, depth, seed, S, dist, miss = 64, 48, 2, 2, 0x5AD0, 4, 2.0, 77
    cam = rc.wavefront.lookat_camera(cfg["eye"], cfg["lattice_centre"], width, height, 45.0)
    n = width * height * spp
    s = torch.cuda.Stream()
    d_x = torch.from_numpy(w.x.view(np.int32).copy()).cuda()
    plain = rc.wavefront.WavefrontPaths(t, width, height, spp, depth, cam, cfg["light"], seed=seed)
    assert plain.gather_samples == 0 and plain.gather_sums == [] and plain.gather_open == [] and plain.traced_rays() == n * 2 * depth
    n_buffers = len(plain.buffers())
    assert plain.with_final_gather(d_x, 0) is plain and plain.gather_sums == [] and len(plain.buffers()) == n_buffers  # off stays off
    assert plain.traced_rays() == n * 2 * depth
    for bad in (w.x, d_x.to(torch.int64), d_x[:100], d_x.cpu()):
        with pytest.raises(ValueError):
            plain.with_final_gather(bad, S)
    del plain
    wf = rc.wavefront.WavefrontPaths(t, width, height, spp, depth, cam, cfg["light"], seed=seed).with_final_gather(d_x, S, dist, miss)
    assert (wf.gather_samples, wf.gather_distance, wf.gather_miss) == (S, dist, miss) and wf.gather_x is d_x
    assert len(wf.gather_sums) == len(wf.gather_open) == depth
    assert all(c.numel() == n and c.dtype == torch.int64 for c in wf.gather_sums) and all(c.numel() == n and c.dtype == torch.int32 for c in wf.gather_open)
    assert wf.traced_rays() == n * 2 * depth + n * S * depth
    assert len(wf.buffers()) == n_buffers + 2 * depth + 1 and all(any(c is b for b in wf.buffers()) for c in wf.gather_sums + wf.gather_open + [d_x])

    def check_frame(what, x):
        live = []
        for b in range(depth):
            rays, hits = wf.rays[b].cpu().numpy().view(bm.RAY_DT), wf.hits[b].cpu().numpy().view(bm.HIT_DT)
            paths = wf.path_ids[b].cpu().numpy().view(np.uint32)
            want = gm.expected(w.o, rays, hits, x, S, miss, seed=seed, depth=b, bias=wf.bias, max_dist=dist, path_in=paths)
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
    live = check_frame("eager", w.x)
    assert live[0] >= 1000 and live[1] >= 20, live
    wf.capture(s)
    for c in wf.gather_sums + wf.gather_open:
        c.fill_(0x7B)  # the replayed frame zeroes them itself
    x2 = distinct_x(w.n_prims, salt=31, with_max=True)
    d_x.copy_(torch.from_numpy(x2.view(np.int32).copy()).cuda())  # held by reference: the replay reads the new solution
    torch.cuda.synchronize()
    wf.replay()
    torch.cuda.synchronize()
    assert check_frame("replay with a new x", x2) == live
    with pytest.raises(rc.RaycoreError):
        wf.with_final_gather(d_x, 0)  # a captured frame keeps its stages
    t.wait_for_gpu()
    del wf
    torch.cuda.synchronize()
    t.set_option("release_captures", 1)
    assert t.get_option("release_captures") == 0


# ---- 12: a hostile scene: a singular instance among normal ones, and hit records that point at it -----------------------------------------
def test_singular_instance_and_nan_frames(rc, oracle):
    """Fused against composed on the product; the oracle only supplies the primary hits and shows that the frames are NaN."""
    import torch
    sc = rc.scenes
    g = np.random.default_rng(0xA0)
    verts = sc.fan_sphere(16, 9)
    rot, _ = np.linalg.qr(g.normal(size=(3, 3)))
    xf = []
    for k, c in enumerate(((-1.2, 0, 0), (1.2, 0.1, 0), (0, 1.3, 0.2), (0, -1.2, -0.1), (0.1, 0, 1.4))):
        m = np.eye(4)
        m[:3, :3] = rot * (0.8 + 0.1 * k)
        m[:3, 3] = c
        xf.append(m[:3].astype(np.float32).reshape(12))
    m = np.eye(4)
    m[:3, :3] = rot @ np.diag([1.0, 1.0, 0.0])  # flattened along one axis: singular, its inverse holds Inf / NaN
    m[:3, 3] = (0.1, 0.1, 0.0)
    singular = len(xf)
    xf.append(m[:3].astype(np.float32).reshape(12))
    cfg = {"blas": [(verts, None)], "instances": [(1, np.stack(xf), np.arange(len(xf), dtype=np.uint32))]}
    t, o = build_product(rc, cfg), build_oracle(oracle, cfg)
    try:
        n, S = 6007, 3
        org = g.uniform(-4, 4, size=(n, 3))
        d = g.uniform(-1.5, 1.5, size=(n, 3)) - org
        rays = sc.make_rays(org, d / np.linalg.norm(d, axis=1, keepdims=True))
        hits = o.trace(rays, nthreads=4)
        lit = np.nonzero(hits["hit"] == 1)[0]
        assert len(lit) >= 500 and n - len(lit) >= 500, len(lit)
        hits = hits.copy()
        hits["instance_id"][lit[::7]] = singular  # the same BLAS, so the records stay in range; their frames come out NaN
        _, nrm = o.hit_points(rays[lit[::7]], hits[lit[::7]])
        assert np.isnan(nrm).any(axis=1).all(), "the singular instance's frames are expected to be NaN"
        prim_meta = t.adapt().all_blas_prims["meta"]
        x = distinct_x(t.n_primitives(), salt=41, with_max=True)
        d_rays, d_hits, d_x = dev(rays), dev(hits), dev(x)
        for dist in DISTANCES:
            d_gr, d_gh = poisoned(n * S * 32), poisoned(n * S * 32)
            t.ambient_occlusion_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), n, S, d_gr.data_ptr(), max_dist=dist, seed=SEED, bias=BIAS)
            t.trace_device(d_gr.data_ptr(), d_gh.data_ptr(), n * S, mode="closest")
            outs = run_gather(t, d_rays, d_hits, n, S, d_x, miss_value=6, max_dist=dist)
            counts = zeroed(n, 4)
            t.ambient_occlusion_device(d_rays.data_ptr(), d_hits.data_ptr(), n, S, counts.data_ptr(), max_dist=dist, seed=SEED, bias=BIAS)
            finish(t)
            stored = d_gr.cpu().numpy()[:n * S * 32].view(bm.RAY_DT)
            assert np.isnan(stored["d"].reshape(n, S, 3)[lit[::7]]).any(axis=2).all()
            assert np.all(stored["tmax"].reshape(n, S)[lit] == np.float32(dist))  # t_max = max_dist > 0 also on NaN frames: no gate
            table = gm.sample_table_of(prim_meta, hits, stored, d_gh.cpu().numpy()[:n * S * 32].view(bm.HIT_DT), S)
            want = gm.reduce(*table, x, 6)
            check(outs, want, f"max_dist={dist}: fused against the composed path")
            assert np.array_equal(words_of(outs[1], n, np.uint32), words_of(counts, n, np.uint32))
            assert 0 < want[1][lit].sum() < len(lit) * S and want[0].any()
    finally:
        t.free()


# ---- 13: the host calls ----------------------------------------------------------------------------------------------------------------------
def test_host_final_gather(rc, worlds):
    w = worlds["lds"]
    for dist in DISTANCES:
        sums, opened = rc.final_gather(w.t, w.rays, w.hits, w.x, S_MAX, max_dist=dist, miss_value=17, seed=SEED, bias=BIAS)
        assert sums.dtype == np.uint64 and opened.dtype == np.uint32 and sums.shape == opened.shape == (N_RAYS,)
        want = w.want(S_MAX, miss_value=17, max_dist=dist)
        assert np.array_equal(sums, want[0]) and np.array_equal(opened, want[1])
        assert np.array_equal(opened, rc.ambient_occlusion(w.t, w.rays, w.hits, S_MAX, max_dist=dist, seed=SEED, bias=BIAS))
    sums, opened = rc.final_gather(w.t, w.rays[:0], w.hits[:0], w.x, 4)
    assert sums.shape == opened.shape == (0,)
    with pytest.raises(ValueError):
        rc.final_gather(w.t, w.rays, w.hits[:5], w.x, 4)
    with pytest.raises(ValueError):
        rc.final_gather(w.t, w.rays, w.hits, w.x[:-1], 4)  # one value per primitive


def test_host_irradiance(rc, worlds):
    """The one float case.  irradiance() quantises b and the sky with floor under one scale, so every sample's value is its float value
    less at most one step, 1 / scale = max(max b, sky) / (2^32 - 1); the mean of S such values is the float mean less at most one step.
    The float mean itself is computed here in float64 from the model's sample table; its own rounding (S additions of values <= 4: below
    1e-14) is far inside the step (about 9e-10), so the bound asserted is the step alone."""
    w = worlds["lds"]
    g = np.random.default_rng(17)
    b = g.uniform(0.0, 3.0, w.n_prims)
    b[:4] = (0.0, 3.0, 1.5, 1e-12)
    for sky, dist in ((4.0, np.inf), (0.25, 1.0), (0.0, np.inf)):
        scale = (2 ** 32 - 1) / max(b.max(), sky)
        step = 1.0 / scale
        meta, escaped = w.table(max_dist=dist)
        value = np.where(escaped, sky, 0.0)
        value[meta >= 1] = b[meta[meta >= 1] - 1]
        want = value.sum(axis=1) / S_MAX
        got, opened = rc.irradiance(w.t, w.rays, w.hits, b, S_MAX, sky=sky, max_dist=dist, seed=SEED, bias=BIAS, return_open=True)
        assert got.dtype == np.float64 and got.shape == (N_RAYS,)
        err = want - got
        print(f"irradiance sky={sky} max_dist={dist}: step {step:.3e}, error min {err.min():.3e} max {err.max():.3e}")
        assert np.all(np.abs(err) <= step), (sky, dist, float(np.abs(err).max()), step)
        assert not got[~w.lit].any() and got[w.lit].max() > 0.5
        assert np.array_equal(opened, w.want(S_MAX, max_dist=dist)[1])
        assert np.array_equal(got, rc.irradiance(w.t, w.rays, w.hits, b, S_MAX, sky=sky, max_dist=dist, seed=SEED, bias=BIAS))
