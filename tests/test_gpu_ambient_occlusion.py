"""rc_ambient_occlusion_device on the GPU: hemisphere visibility counts of all hits x samples in one traversal launch, count for count
against the numpy model's rays (tests/ao_model.py) traced by the CPU oracle, in the three kernel shapes the launcher dispatches (top level
in LDS, partial LDS, plain) and for an unbounded and a short reach; against the product's own composed path
(rc_ambient_occlusion_rays_device + any-hit trace, also with the entry cull on), whose stored rays are the model's bit for bit;
accumulating over depths, keyed by path ids, with empty work, bad arguments, a captured call whose frame is exchanged between replays, two
streams at once, as the ambient-occlusion stage of WavefrontPaths, on a hostile scene with a singular instance and NaN hit frames, and
through the host convenience.

Not tested separately: "one sample with max_dist = inf is the bounce ray of that path escaping".  The occlusion ray draws its uniforms
under a Philox tag of its own, so it is no bounce ray bit for bit; what the two share is the direction function, and that is already
pinned from both sides -- the model builds its rays with bounce_model.cosine_hemisphere, the function tests/test_gpu_bounce.py holds
rc_bounce_rays_device to, and the composed-path test below holds the device's stored occlusion rays to the model bit for bit."""
import numpy as np
import pytest

import ao_model as am
import bounce_model as bm
from gpu_kit import POISON, check_words, dev, poisoned, words_of, zeroed
from gpu_kit import rc  # noqa: F401
from helpers import assert_rays_equal, build_oracle, build_product
from worlds import C3World, three_shapes

pytestmark = pytest.mark.gpu

BIAS = 1e-3
N_RAYS = 63_997  # 320 x 200 less three: n * S ends inside a 128-item chunk for S = 2 and 5 (remainders 122 and 113)
SEED = 0xA0
S_MAX = 5
DISTANCES = (np.inf, 1.0)
DUMMY = np.array([0, 0, 0, 0, 0, 0, 1, 0], np.float32).view(np.uint32)


class World(C3World):
    def __init__(self, rc, oracle, lattice, kernel=None):
        super().__init__(rc, oracle, lattice, kernel)
        self._seen = {}
        # a degenerate input cannot pass: (enough hits and misses;) fully open, partly occluded (and, on the dense lattice, fully occluded)
        # slots; and a reach that matters -- all from the oracle alone, before anything is compared
        lit = int(self.lit.sum())
        for dist in DISTANCES:
            c = self.want(S_MAX, max_dist=dist)[self.lit]
            full, zero = int((c == S_MAX).sum()), int((c == 0).sum())
            assert full >= 100 and lit - full - zero >= 100, (lattice, dist, full, lit - full - zero, zero)
            if lattice == (7, 7, 6) and dist == np.inf:
                assert zero >= 20, zero
        assert not np.array_equal(self.want(S_MAX, max_dist=DISTANCES[0]), self.want(S_MAX, max_dist=DISTANCES[1]))

    def seen(self, max_dist=np.inf, seed=SEED, depth=0, path_in=None, path_base=0, rays=None, hits=None):
        """(n, S_MAX) bool from the oracle alone: sample s of slot i is visible -- the model's rays, oracle.trace(mode="any"), the gate.
        Computed once per argument set; a sample does not depend on `samples`, so every S <= S_MAX reads its first S columns."""
        key = (float(max_dist), seed, depth, None if path_in is None else np.asarray(path_in).tobytes(), path_base, rays is None)
        if key not in self._seen:
            r, h = (self.rays, self.hits) if rays is None else (rays, hits)
            ar = am.ao_rays(self.o, r, h, S_MAX, seed, depth, BIAS, max_dist, path_in, path_base)
            ah = self.o.trace(ar, mode="any", nthreads=16)
            v = ((np.repeat(h["hit"] != 0, S_MAX)) & (ar["tmax"] > 0) & (ah["hit"] == 0)).reshape(len(r), S_MAX)
            v.setflags(write=False)
            self._seen[key] = v
        return self._seen[key]

    def want(self, samples, **kw):
        """(n,) u32 expected counts of the first `samples` samples."""
        assert samples <= S_MAX
        return self.seen(**kw)[:, :samples].sum(axis=1).astype(np.uint32)

    def fused(self, samples, out=None, max_dist=np.inf, seed=SEED, depth=0, d_path_in=None, path_base=0, stream=None):
        """One call into a zeroed count buffer with a poisoned guard behind it (or into `out`); returns the tensor."""
        if out is None:
            out = zeroed(N_RAYS, 4)
        self.t.ambient_occlusion_device(self.d_rays.data_ptr(), self.d_hits.data_ptr(), N_RAYS, samples, out.data_ptr(), max_dist=max_dist, seed=seed,
                                        depth=depth, bias=BIAS, d_path_in=d_path_in, path_base=path_base, stream=stream)
        return out


def check(out, want, what):
    """`out`: a tensor from World.fused, `want`: (n,) counts."""
    check_words(out, want, np.uint32, what)


@pytest.fixture(scope="module")
def worlds(rc, oracle):
    yield from three_shapes(World, rc, oracle)


# ---- 1: every count against the oracle, in the three shapes, for both reaches ----------------------------------------------------------
@pytest.mark.parametrize("shape", ["lds", "partial", "plain"])
@pytest.mark.parametrize("max_dist", DISTANCES)
@pytest.mark.parametrize("samples", [1, 2, 5])
def test_counts_equal_the_oracles(worlds, shape, max_dist, samples):
    import torch
    w = worlds[shape]
    out = w.fused(samples, max_dist=max_dist)
    torch.cuda.synchronize()
    w.t.wait_for_gpu()  # (a stack overflow would be reported here)
    check(out, w.want(samples, max_dist=max_dist), f"{shape} S={samples} max_dist={max_dist}")
    got = words_of(out, N_RAYS, np.uint32)
    assert not got[~w.lit].any(), "a slot whose primary ray missed has visible samples"
    assert got.max() <= samples


# ---- 2: the product's own composed path, with and without the entry cull ----------------------------------------------------------------
@pytest.mark.parametrize("shape", ["lds", "partial", "plain"])
def test_composed_product_path_gives_the_same_counts(worlds, shape):
    import torch
    w = worlds[shape]
    t, n, S, dist = w.t, N_RAYS, S_MAX, 1.0
    total = n * S
    model_rays = am.ao_rays(w.o, w.rays, w.hits, S, SEED, 0, BIAS, dist)
    before = t.get_option("entry_cull")
    try:
        for cull in (before, 2):
            t.set_option("entry_cull", cull)
            d_ar, d_ah = poisoned(total * 32), poisoned(total * 32)
            t.ambient_occlusion_rays_device(w.d_rays.data_ptr(), w.d_hits.data_ptr(), n, S, d_ar.data_ptr(), max_dist=dist, seed=SEED, bias=BIAS)
            t.trace_device(d_ar.data_ptr(), d_ah.data_ptr(), total, mode="any")
            out = w.fused(S, max_dist=dist)
            torch.cuda.synchronize()
            raw = d_ar.cpu().numpy()
            assert np.all(raw[total * 32:] == POISON), "bytes behind the occlusion rays were written"
            stored = raw[:total * 32].view(bm.RAY_DT)
            composed = am.counts_of(w.hits, stored, d_ah.cpu().numpy()[:total * 32].view(bm.HIT_DT), S)
            check(out, composed, f"{shape} entry_cull={cull} against the composed path")
            check(out, w.want(S, max_dist=dist), f"{shape} entry_cull={cull} against the oracle")
            a, b = stored.view(np.uint32).reshape(n, S, 8), model_rays.view(np.uint32).reshape(n, S, 8)
            assert np.array_equal(a[w.lit], b[w.lit]), f"{shape}: the stored rays differ from the model's on hit slots"
            assert np.all(a[~w.lit] == DUMMY), f"{shape}: a miss slot does not hold the dummy ray"
    finally:
        t.set_option("entry_cull", before)


# ---- 4: accumulation over depths, and samples keyed by path ids ------------------------------------------------------------------------
def test_accumulation_and_path_ids(worlds):
    import torch
    w = worlds["lds"]
    out = w.fused(2, depth=0)
    w.fused(2, out=out, depth=1)
    torch.cuda.synchronize()
    d0, d1 = w.want(2, depth=0), w.want(2, depth=1)
    assert not np.array_equal(d0, d1)  # another depth draws other samples
    check(out, d0 + d1, "depth 0 + depth 1 into one buffer")
    perm = np.random.default_rng(5).permutation(N_RAYS).astype(np.uint32)
    d_perm = dev(perm)
    out = w.fused(2, d_path_in=d_perm.data_ptr(), path_base=7)
    torch.cuda.synchronize()
    keyed = w.want(2, path_in=perm, path_base=7)
    assert not np.array_equal(keyed, d0)
    check(out, keyed, "d_path_in = a permutation, path_base = 7")


# ---- 5: empty work and refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rc_ambient_occlusion_device", "rc_ambient_occlusion_rays_device"])
def test_empty_work_and_argument_checks(rc, worlds, name):
    import torch
    from raycore_jl_amd._capi import lib
    w = worlds["lds"]
    f, h = getattr(lib(), name), w.t._h
    out = poisoned(4096)
    r, hh, op = w.d_rays.data_ptr(), w.d_hits.data_ptr(), out.data_ptr()
    INV, NS = 1, 6

    def call(scene=h, rays=r, hits=hh, n=16, samples=4, max_dist=np.inf, depth=0, o=op):
        return f(scene, rays, hits, n, samples, max_dist, SEED, depth, None, 0, BIAS, o, None)

    assert call(n=0) == 0 and call(samples=0) == 0
    assert call(rays=None, hits=None, n=0, o=None) == 0  # no work: nothing is read
    assert call(rays=None, hits=None, samples=0, o=None) == 0
    torch.cuda.synchronize()
    assert bool((out == POISON).all()), "a call without work wrote to the output"
    assert call(scene=None) == INV
    assert call(rays=None) == INV
    assert call(hits=None) == INV
    assert call(o=None) == INV
    assert call(n=1 << 30, samples=4) == INV               # n * samples == 2^32
    assert call(n=(1 << 32) // 5 + 1, samples=5) == INV    # the first n past it for S = 5
    assert call(n=1 << 63, samples=2) == INV               # (a product that wraps in 64 bits)
    assert call(n=1 << 32, samples=1) == INV
    assert call(samples=65536) == INV
    assert call(depth=65536) == INV
    for bad in (0.0, -0.0, -1.0, -np.inf, np.nan):
        assert call(max_dist=bad) == INV, bad
    torch.cuda.synchronize()
    assert bool((out == POISON).all()), "a refused call wrote to the output"
    u = build_product(rc, rc.scenes.config_c1())
    u.push_instances(1, rc.scenes.IDENTITY3x4[None], np.zeros(1, np.uint32))  # a pending mutation
    assert call(scene=u._h) == NS
    u.free()
    torch.cuda.synchronize()
    assert bool((out == POISON).all())


# ---- 6: captured, with the frame exchanged in place between replays ---------------------------------------------------------------------
def test_captured_call_follows_the_frame(worlds):
    import torch
    w = worlds["partial"]
    t, S = w.t, 2
    s = torch.cuda.Stream()
    d_rays, d_hits = dev(w.rays), dev(w.hits)  # the captured call's own frame buffers
    out = zeroed(N_RAYS, 4)

    def launch():
        t.ambient_occlusion_device(d_rays.data_ptr(), d_hits.data_ptr(), N_RAYS, S, out.data_ptr(), seed=SEED, bias=BIAS, stream=s.cuda_stream)

    torch.cuda.synchronize()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launch()  # the eager call the capture needs
    torch.cuda.synchronize()
    check(out, w.want(S), "eager call")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launch()
    rays2, hits2 = np.ascontiguousarray(w.rays[::-1]), np.ascontiguousarray(w.hits[::-1])  # another frame: the same view, slots reversed
    want2 = w.want(S, rays=rays2, hits=hits2)
    assert not np.array_equal(want2, w.want(S)) and not np.array_equal(want2, w.want(S)[::-1])  # (slot = path: other samples per point)
    for rays, hits, want, what in ((w.rays, w.hits, w.want(S), "replay"), (rays2, hits2, want2, "replay after the frame was exchanged in place")):
        d_rays.copy_(dev(rays))  # in place: the graph holds the tensors' addresses
        d_hits.copy_(dev(hits))
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            out[:N_RAYS * 4] = 0  # the call accumulates: zeroed in the graph's stream before each replay
            g.replay()
        torch.cuda.synchronize()
        check(out, want, what)
    t.wait_for_gpu()
    del g
    torch.cuda.synchronize()
    t.set_option("release_captures", 1)  # the graph is gone: hand its captured launch back
    assert t.get_option("release_captures") == 0


# ---- 7: two streams at once, different seeds ---------------------------------------------------------------------------------------------
def test_two_streams_at_once(worlds):
    import torch
    w = worlds["lds"]
    seeds, S = (SEED, 0xBEEF00000001), 2
    streams = [torch.cuda.Stream() for _ in seeds]
    outs = [[zeroed(N_RAYS, 4) for _ in range(3)] for _ in seeds]
    torch.cuda.synchronize()  # the buffers are filled on the current stream: done before the other streams write them
    for rep in range(3):  # enqueued alternately, never waited for in between
        for k, seed in enumerate(seeds):
            w.fused(S, out=outs[k][rep], seed=seed, stream=streams[k].cuda_stream)
    torch.cuda.synchronize()
    w.t.wait_for_gpu()
    assert not np.array_equal(w.want(S, seed=seeds[0]), w.want(S, seed=seeds[1]))
    for k, seed in enumerate(seeds):
        for rep, out in enumerate(outs[k]):
            check(out, w.want(S, seed=seed), f"stream {k} launch {rep}")


# ---- 8: the ambient-occlusion stage of WavefrontPaths -----------------------------------------------------------------------------------
def test_wavefront_ambient_occlusion(rc, worlds):
    import torch
    w = worlds["partial"]  # (the dense lattice: enough paths survive the first bounce for the compaction comparison to mean something)
    t, cfg = w.t, w.cfg
    width, height, spp, depth, seed, S, dist = 64, 48, 2, 2, 0x5AD0, 4, 2.0
    cam = rc.wavefront.lookat_camera(cfg["eye"], cfg["lattice_centre"], width, height, 45.0)
    n = width * height * spp
    s = torch.cuda.Stream()
    plain = rc.wavefront.WavefrontPaths(t, width, height, spp, depth, cam, cfg["light"], seed=seed)
    assert plain.ao_samples == 0 and plain.ao_counts == [] and plain.traced_rays() == n * 2 * depth
    n_buffers = len(plain.buffers())
    assert plain.with_ambient_occlusion(0) is plain and plain.ao_counts == [] and len(plain.buffers()) == n_buffers  # off stays off
    del plain
    maps = {}
    for compact in (True, False):
        wf = rc.wavefront.WavefrontPaths(t, width, height, spp, depth, cam, cfg["light"], seed=seed, compact=compact).with_ambient_occlusion(S, dist)
        assert wf.ao_samples == S and wf.ao_distance == dist and len(wf.ao_counts) == depth
        assert all(c.numel() == n and c.dtype == torch.int32 for c in wf.ao_counts)
        assert wf.traced_rays() == n * 2 * depth + n * S * depth
        assert len(wf.buffers()) == n_buffers + depth and all(any(c is b for b in wf.buffers()) for c in wf.ao_counts)

        def check_frame(what):
            by_path = {}
            for b in range(depth):
                rays, hits = wf.rays[b].cpu().numpy().view(bm.RAY_DT), wf.hits[b].cpu().numpy().view(bm.HIT_DT)
                paths = wf.path_ids[b].cpu().numpy().view(np.uint32)
                want, _ = am.expected_counts(w.o, rays, hits, S, seed=seed, depth=b, bias=wf.bias, max_dist=dist, path_in=paths)
                got = wf.ao_counts[b].cpu().numpy().view(np.uint32)
                bad = np.nonzero(got != want)[0]
                assert len(bad) == 0, f"{what} depth {b}: {len(bad)} counts differ, first {bad[:5]}: got {got[bad[:5]]} want {want[bad[:5]]}"
                lit = hits["hit"] == 1
                assert 0 < got[lit].sum() < lit.sum() * S, (what, b)
                assert len(np.unique(paths[lit])) == lit.sum()
                by_path[b] = {int(p): int(c) for p, c in zip(paths[lit], got[lit])}
            return by_path

        s.wait_stream(torch.cuda.current_stream())
        wf.run(s)  # (not made current: the frame zeroes its counts on the stream it is given)
        torch.cuda.synchronize()
        eager = check_frame(f"compact={compact} eager")
        wf.capture(s)
        for c in wf.ao_counts:
            c.fill_(0x7B7B7B7B)  # the replayed frame zeroes them itself
        torch.cuda.synchronize()
        wf.replay()
        torch.cuda.synchronize()
        assert check_frame(f"compact={compact} replay") == eager
        with pytest.raises(rc.RaycoreError):
            wf.with_ambient_occlusion(0)  # a captured frame keeps its stages
        maps[compact] = eager
        t.wait_for_gpu()
        del wf
        torch.cuda.synchronize()
        t.set_option("release_captures", 1)
        assert t.get_option("release_captures") == 0
    assert maps[True] == maps[False], "compaction changed a path's occlusion counts"
    assert len(maps[True][0]) >= 1000 and len(maps[True][1]) >= 20, (len(maps[True][0]), len(maps[True][1]))  # live paths at both depths


# ---- 9: a hostile scene: a singular instance among normal ones, and hit records that point at it ---------------------------------------
def test_singular_instance_and_nan_frames(rc, oracle):
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
        for dist in DISTANCES:
            want, model_rays = am.expected_counts(o, rays, hits, S, seed=SEED, bias=BIAS, max_dist=dist, nthreads=4)
            assert np.isnan(model_rays["d"].reshape(n, S, 3)[lit[::7]]).any(axis=2).all()
            assert np.all(model_rays["tmax"].reshape(n, S)[lit] == np.float32(dist))  # t_max = max_dist > 0 also on NaN frames: no gate
            d_rays, d_hits = dev(rays), dev(hits)
            d_ar, d_ah, out = poisoned(n * S * 32), poisoned(n * S * 32), zeroed(n, 4)
            t.ambient_occlusion_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), n, S, d_ar.data_ptr(), max_dist=dist, seed=SEED, bias=BIAS)
            t.trace_device(d_ar.data_ptr(), d_ah.data_ptr(), n * S, mode="any")
            t.ambient_occlusion_device(d_rays.data_ptr(), d_hits.data_ptr(), n, S, out.data_ptr(), max_dist=dist, seed=SEED, bias=BIAS)
            torch.cuda.synchronize()
            t.wait_for_gpu()
            stored = d_ar.cpu().numpy()[:n * S * 32].view(bm.RAY_DT)
            assert_rays_equal(stored, model_rays, f"max_dist={dist}: stored rays against the model's")
            composed = am.counts_of(hits, stored, d_ah.cpu().numpy()[:n * S * 32].view(bm.HIT_DT), S)
            check(out, composed, f"max_dist={dist}: fused against the composed path")
            check(out, want, f"max_dist={dist}: fused against the oracle")
            assert 0 < want[lit].sum() < len(lit) * S
    finally:
        t.free()


# ---- 10: the host convenience ------------------------------------------------------------------------------------------------------------
def test_host_convenience(rc, worlds):
    w = worlds["lds"]
    for dist in DISTANCES:
        got = rc.ambient_occlusion(w.t, w.rays, w.hits, S_MAX, max_dist=dist, seed=SEED, bias=BIAS)
        assert got.dtype == np.uint32 and got.shape == (N_RAYS,)
        assert np.array_equal(got, w.want(S_MAX, max_dist=dist))
    assert rc.ambient_occlusion(w.t, w.rays[:0], w.hits[:0], 4).shape == (0,)
    with pytest.raises(ValueError):
        rc.ambient_occlusion(w.t, w.rays, w.hits[:5], 4)
