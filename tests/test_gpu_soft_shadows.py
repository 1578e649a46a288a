"""rc_soft_shadow_visibility_device on the GPU: area-light visibility counts of all hits x all lights x samples in one traversal launch,
count for count against the numpy model's rays (tests/soft_shadow_model.py) traced by the CPU oracle, in the three kernel shapes the
launcher dispatches (top level in LDS, partial LDS, plain); against rc_shadow_visibility_device with one sample and with radius 0;
against the product's own composed path (rc_soft_shadow_rays_device + any-hit trace, also with the entry cull on); accumulating over
depths, keyed by path ids, with empty work, bad arguments, a captured graph whose lights move and resize between replays, two streams at
once, as the soft mode of WavefrontPaths, and with a light placed exactly on a hit point."""
import numpy as np
import pytest

import bounce_model as bm
import soft_shadow_model as sm
from gpu_kit import POISON, check_words, dev, f32_tensor, poisoned, words_of, zeroed
from gpu_kit import rc  # noqa: F401
from helpers import build_product
from worlds import C3World, three_shapes

pytestmark = pytest.mark.gpu

LIGHTS = np.array([[10, 10, 10], [-4, 6, 3], [3, 2.5, -6]], np.float32)
RADII = np.array([1.0, 0.5, 1.0], np.float32)
BIAS = 1e-3
N_RAYS = 63_997  # 320 x 200 less three: with L = 3, n * L * S ends inside a 128-item chunk for S = 2 and 5 (remainders 110 and 83)
SEED = 0x50F7
DUMMY = np.array([0, 0, 0, 0, 0, 0, 1, 0], np.float32).view(np.uint32)


class World(C3World):
    def __init__(self, rc, oracle, lattice, kernel=None):
        super().__init__(rc, oracle, lattice, kernel)
        self._want = {}
        # a degenerate input cannot pass: (enough hits and misses, and) for every light fully shadowed, fully lit and penumbra slots
        c = self.want(5)[self.lit]
        for l in range(len(LIGHTS)):
            zero, full = int((c[:, l] == 0).sum()), int((c[:, l] == 5).sum())
            assert zero >= 20 and full >= 20 and len(c) - zero - full >= 20, (l, zero, full, len(c) - zero - full)

    def want(self, samples, lights=LIGHTS, radii=RADII, seed=SEED, depth=0, path_in=None, path_base=0):
        """(n, L) expected counts from the oracle alone: the model's rays, oracle.trace(mode="any"), the gate, the sum.  Computed once."""
        key = (samples, np.asarray(lights, np.float32).tobytes(), np.asarray(radii, np.float32).tobytes(), seed, depth,
               None if path_in is None else np.asarray(path_in).tobytes(), path_base)
        if key not in self._want:
            counts, _ = sm.expected_counts(self.o, self.rays, self.hits, lights, radii, samples, seed=seed, depth=depth, bias=BIAS, path_in=path_in,
                                           path_base=path_base)
            counts.setflags(write=False)
            self._want[key] = counts
        return self._want[key]

    def fused(self, lights_t, radii_t, n_lights, samples, out=None, seed=SEED, depth=0, d_path_in=None, path_base=0, stream=None):
        """One call into a zeroed count buffer with a poisoned guard behind it (or into `out`); returns the tensor."""
        if out is None:
            out = zeroed(N_RAYS * n_lights, 4)
        self.t.soft_shadow_visibility_device(self.d_rays.data_ptr(), self.d_hits.data_ptr(), N_RAYS, lights_t.data_ptr(), radii_t.data_ptr(), n_lights,
                                             samples, out.data_ptr(), seed=seed, depth=depth, bias=BIAS, d_path_in=d_path_in, path_base=path_base,
                                             stream=stream)
        return out

    def hard(self, lights_t, n_lights):
        """rc_shadow_visibility_device's bytes for the same hits and lights, (n, L)."""
        import torch
        out = poisoned(N_RAYS * n_lights)
        self.t.shadow_visibility_device(self.d_rays.data_ptr(), self.d_hits.data_ptr(), N_RAYS, lights_t.data_ptr(), n_lights, out.data_ptr(), bias=BIAS)
        torch.cuda.synchronize()
        return out.cpu().numpy()[:N_RAYS * n_lights].reshape(N_RAYS, n_lights)


def check(out, want, what):
    """`out`: a tensor from World.fused, `want`: (n, L) counts."""
    check_words(out, want, np.uint32, what)


@pytest.fixture(scope="module")
def worlds(rc, oracle):
    yield from three_shapes(World, rc, oracle)


# ---- 1: every count against the oracle, in the three shapes -------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["lds", "partial", "plain"])
@pytest.mark.parametrize("n_lights", [1, 3])
@pytest.mark.parametrize("samples", [1, 2, 5])
def test_counts_equal_the_oracles(worlds, shape, n_lights, samples):
    import torch
    w = worlds[shape]
    out = w.fused(f32_tensor(LIGHTS[:n_lights]), f32_tensor(RADII[:n_lights]), n_lights, samples)
    torch.cuda.synchronize()
    w.t.wait_for_gpu()  # (a stack overflow would be reported here)
    want = w.want(samples)[:, :n_lights]  # (a sample depends on (seed, path, depth, l, s), not on how many lights there are)
    check(out, want, f"{shape} L={n_lights} S={samples}")
    got = words_of(out, N_RAYS * n_lights, np.uint32).reshape(N_RAYS, n_lights)
    assert not got[~w.lit].any(), "a slot whose primary ray missed has visible samples"
    assert got.max() <= samples


# ---- 2, 3: one sample, and radius 0, are the hard shadow ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["lds", "partial", "plain"])
def test_one_sample_and_radius_zero_equal_the_hard_shadow_byte(worlds, shape):
    import torch
    w = worlds[shape]
    d_l = f32_tensor(LIGHTS)
    byte = w.hard(d_l, 3)
    assert 0 < byte.sum() < byte.size
    one = w.fused(d_l, f32_tensor(RADII), 3, 1)
    three = w.fused(d_l, f32_tensor(np.zeros(3, np.float32)), 3, 3)
    torch.cuda.synchronize()
    check(one, byte.astype(np.uint32), f"{shape} S=1 against rc_shadow_visibility_device")
    check(three, 3 * byte.astype(np.uint32), f"{shape} radius 0, S=3 against 3 x rc_shadow_visibility_device")


# ---- 4: the product's own composed path, with and without the entry cull ----------------------------------------------------------------
@pytest.mark.parametrize("shape", ["lds", "partial", "plain"])
def test_composed_product_path_gives_the_same_counts(worlds, shape):
    import torch
    w = worlds[shape]
    t, n, L, S = w.t, N_RAYS, 3, 5
    total = n * L * S
    d_l, d_r = f32_tensor(LIGHTS), f32_tensor(RADII)
    _, model_rays = sm.expected_counts(w.o, w.rays, w.hits, LIGHTS, RADII, S, seed=SEED, bias=BIAS)
    before = t.get_option("entry_cull")
    try:
        for cull in (before, 2):
            t.set_option("entry_cull", cull)
            d_sr, d_sh = poisoned(total * 32), poisoned(total * 32)
            t.soft_shadow_rays_device(w.d_rays.data_ptr(), w.d_hits.data_ptr(), n, d_l.data_ptr(), d_r.data_ptr(), L, S, d_sr.data_ptr(), seed=SEED,
                                      bias=BIAS)
            t.trace_device(d_sr.data_ptr(), d_sh.data_ptr(), total, mode="any")
            out = w.fused(d_l, d_r, L, S)
            torch.cuda.synchronize()
            raw = d_sr.cpu().numpy()
            assert np.all(raw[total * 32:] == POISON), "bytes behind the shadow rays were written"
            stored = raw[:total * 32].view(bm.RAY_DT)
            composed = sm.counts_of(w.hits, stored, d_sh.cpu().numpy()[:total * 32].view(bm.HIT_DT), L, S)
            check(out, composed, f"{shape} entry_cull={cull} against the composed path")
            check(out, w.want(S), f"{shape} entry_cull={cull} against the oracle")
            a, b = stored.view(np.uint32).reshape(n, L * S, 8), model_rays.view(np.uint32).reshape(n, L * S, 8)
            assert np.array_equal(a[w.lit], b[w.lit]), f"{shape}: the stored rays differ from the model's on hit slots"
            assert np.all(a[~w.lit] == DUMMY), f"{shape}: a miss slot does not hold the dummy ray"
    finally:
        t.set_option("entry_cull", before)


# ---- 5: accumulation over depths, and samples keyed by path ids ------------------------------------------------------------------------
def test_accumulation_and_path_ids(worlds):
    import torch
    w = worlds["lds"]
    d_l, d_r = f32_tensor(LIGHTS), f32_tensor(RADII)
    out = w.fused(d_l, d_r, 3, 2, depth=0)
    w.fused(d_l, d_r, 3, 2, out=out, depth=1)
    torch.cuda.synchronize()
    d0, d1 = w.want(2, depth=0), w.want(2, depth=1)
    assert not np.array_equal(d0, d1)  # another depth draws other samples
    check(out, d0 + d1, "depth 0 + depth 1 into one buffer")
    perm = np.random.default_rng(5).permutation(N_RAYS).astype(np.uint32)
    d_perm = dev(perm)
    out = w.fused(d_l, d_r, 3, 2, d_path_in=d_perm.data_ptr(), path_base=7)
    torch.cuda.synchronize()
    keyed = w.want(2, path_in=perm, path_base=7)
    assert not np.array_equal(keyed, d0)
    check(out, keyed, "d_path_in = a permutation, path_base = 7")


# ---- 6: empty work and refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rc_soft_shadow_visibility_device", "rc_soft_shadow_rays_device"])
def test_empty_work_and_argument_checks(rc, worlds, name):
    import torch
    from raycore_jl_amd._capi import lib
    w = worlds["lds"]
    f, h = getattr(lib(), name), w.t._h
    d_l, d_r = f32_tensor(LIGHTS), f32_tensor(RADII)
    out = poisoned(4096)
    r, hh, lp, rp, op = w.d_rays.data_ptr(), w.d_hits.data_ptr(), d_l.data_ptr(), d_r.data_ptr(), out.data_ptr()
    INV, NS = 1, 6

    def call(scene=h, rays=r, hits=hh, n=16, lights=lp, radii=rp, n_lights=3, samples=4, depth=0, o=op):
        return f(scene, rays, hits, n, lights, radii, n_lights, samples, SEED, depth, None, 0, BIAS, o, None)

    assert call(n=0) == 0 and call(n_lights=0) == 0 and call(samples=0) == 0
    assert call(rays=None, hits=None, n=0, lights=None, radii=None, o=None) == 0  # no work: nothing is read
    assert call(rays=None, hits=None, lights=None, radii=None, n_lights=0, o=None) == 0
    assert call(rays=None, hits=None, lights=None, radii=None, samples=0, o=None) == 0
    torch.cuda.synchronize()
    assert bool((out == POISON).all()), "a call without work wrote to the output"
    assert call(scene=None) == INV
    assert call(rays=None) == INV
    assert call(hits=None) == INV
    assert call(lights=None) == INV
    assert call(radii=None) == INV
    assert call(o=None) == INV
    assert call(n=1 << 28, n_lights=4, samples=4) == INV           # n * n_lights * samples == 2^32
    assert call(n=(1 << 32) // 15 + 1, n_lights=3, samples=5) == INV  # the first n past it for L = 3, S = 5
    assert call(n=1 << 63, n_lights=2, samples=1) == INV            # (a product that wraps in 64 bits)
    assert call(samples=65536) == INV
    assert call(depth=65536) == INV
    assert call(n_lights=65536) == INV
    torch.cuda.synchronize()
    assert bool((out == POISON).all()), "a refused call wrote to the output"
    u = build_product(rc, rc.scenes.config_c1())
    u.push_instances(1, rc.scenes.IDENTITY3x4[None], np.zeros(1, np.uint32))  # a pending mutation
    assert call(scene=u._h) == NS
    u.free()
    torch.cuda.synchronize()
    assert bool((out == POISON).all())


# ---- 7: captured, with a light that moves and a radius that changes between replays ---------------------------------------------------
def test_captured_call_follows_lights_and_radii(worlds):
    import torch
    w = worlds["partial"]
    t, L, S = w.t, 3, 2
    s = torch.cuda.Stream()
    d_l, d_r = f32_tensor(LIGHTS), f32_tensor(RADII)
    out = zeroed(N_RAYS * L, 4)
    torch.cuda.synchronize()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        w.fused(d_l, d_r, L, S, out=out, stream=s.cuda_stream)  # the eager call the capture needs
    torch.cuda.synchronize()
    check(out, w.want(S), "eager call")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        w.fused(d_l, d_r, L, S, out=out, stream=s.cuda_stream)
    moved, resized = LIGHTS.copy(), RADII.copy()
    moved[1] = (-3, 7, 2.5)
    resized[2] = 0.25
    for lights, radii, what in ((LIGHTS, RADII, "replay"), (moved, resized, "replay after a light moved and a radius changed")):
        d_l.copy_(f32_tensor(lights))  # in place: the graph holds the tensors' addresses
        d_r.copy_(f32_tensor(radii))
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            out[:N_RAYS * L * 4] = 0  # the call accumulates: zeroed in the graph's stream before each replay
            g.replay()
        torch.cuda.synchronize()
        check(out, w.want(S, lights=lights, radii=radii), what)
    assert not np.array_equal(w.want(S), w.want(S, lights=moved, radii=resized))
    t.wait_for_gpu()
    del g
    torch.cuda.synchronize()
    t.set_option("release_captures", 1)  # the graph is gone: hand its captured launch back
    assert t.get_option("release_captures") == 0


# ---- 8: two streams at once, different seeds ---------------------------------------------------------------------------------------------
def test_two_streams_at_once(worlds):
    import torch
    w = worlds["lds"]
    seeds, L, S = (SEED, 0xBEEF00000001), 3, 2
    streams = [torch.cuda.Stream() for _ in seeds]
    d_l, d_r = f32_tensor(LIGHTS), f32_tensor(RADII)
    outs = [[zeroed(N_RAYS * L, 4) for _ in range(3)] for _ in seeds]
    torch.cuda.synchronize()  # the buffers are filled on the current stream: done before the other streams write them
    for rep in range(3):  # enqueued alternately, never waited for in between
        for k, seed in enumerate(seeds):
            w.fused(d_l, d_r, L, S, out=outs[k][rep], seed=seed, stream=streams[k].cuda_stream)
    torch.cuda.synchronize()
    w.t.wait_for_gpu()
    assert not np.array_equal(w.want(S, seed=seeds[0]), w.want(S, seed=seeds[1]))
    for k, seed in enumerate(seeds):
        for rep, out in enumerate(outs[k]):
            check(out, w.want(S, seed=seed), f"stream {k} launch {rep}")


# ---- 9: the soft mode of WavefrontPaths -----------------------------------------------------------------------------------------------
def test_wavefront_soft_shadows(rc, worlds):
    import torch
    w = worlds["partial"]  # (the dense lattice: enough paths survive the first bounce for the compaction comparison to mean something)
    t, cfg = w.t, w.cfg
    width, height, spp, depth, seed, S, L = 64, 48, 2, 2, 0x5AD0, 4, 3
    cam = rc.wavefront.lookat_camera(cfg["eye"], cfg["lattice_centre"], width, height, 45.0)
    n = width * height * spp
    d_l, d_r = f32_tensor(LIGHTS), f32_tensor(RADII)
    s = torch.cuda.Stream()
    maps = {}
    for compact in (True, False):
        wf = rc.wavefront.WavefrontPaths(t, width, height, spp, depth, cam, lights=d_l, light_radii=d_r, fused_shadows=True, shadow_samples=S, seed=seed,
                                         compact=compact)
        assert wf.visible == [] and wf.shadow_rays == [] and len(wf.shadow_counts) == depth and wf.light_radii is d_r and wf.shadow_samples == S
        assert all(c.numel() == n * L and c.dtype == torch.int32 for c in wf.shadow_counts)
        assert wf.traced_rays() == n * (1 + L * S) * depth

        def check_frame(what):
            by_path = {}
            for b in range(depth):
                rays, hits = wf.rays[b].cpu().numpy().view(bm.RAY_DT), wf.hits[b].cpu().numpy().view(bm.HIT_DT)
                paths = wf.path_ids[b].cpu().numpy().view(np.uint32)
                want, _ = sm.expected_counts(w.o, rays, hits, LIGHTS, RADII, S, seed=seed, depth=b, bias=wf.bias, path_in=paths)
                got = wf.shadow_counts[b].cpu().numpy().view(np.uint32).reshape(n, L)
                bad = np.nonzero(got != want)
                assert len(bad[0]) == 0, f"{what} depth {b}: {len(bad[0])} counts differ, first {bad[0][:5]}, {bad[1][:5]}"
                lit = hits["hit"] == 1
                assert 0 < got[lit].sum() < lit.sum() * L * S, (what, b)
                assert len(np.unique(paths[lit])) == lit.sum()
                by_path[b] = {int(p): tuple(c) for p, c in zip(paths[lit], got[lit])}
            return by_path

        s.wait_stream(torch.cuda.current_stream())
        wf.run(s)  # (not made current: the frame zeroes its counts on the stream it is given)
        torch.cuda.synchronize()
        eager = check_frame(f"compact={compact} eager")
        wf.capture(s)
        for c in wf.shadow_counts:
            c.fill_(0x7B7B7B7B)  # the replayed frame zeroes them itself
        torch.cuda.synchronize()
        wf.replay()
        torch.cuda.synchronize()
        assert check_frame(f"compact={compact} replay") == eager
        maps[compact] = eager
        t.wait_for_gpu()
        del wf
        torch.cuda.synchronize()
        t.set_option("release_captures", 1)
        assert t.get_option("release_captures") == 0
    assert maps[True] == maps[False], "compaction changed a path's visibility counts"
    assert len(maps[True][0]) >= 1000 and len(maps[True][1]) >= 20, (len(maps[True][0]), len(maps[True][1]))  # live paths at both depths


# ---- 10: a light exactly on a hit point --------------------------------------------------------------------------------------------------
def test_light_on_a_hit_point_is_gated(worlds):
    import torch
    w = worlds["partial"]
    S = 2
    k = int(np.nonzero(w.lit)[0][len(np.nonzero(w.lit)[0]) // 2])
    p, _ = w.o.hit_points(w.rays[k:k + 1], w.hits[k:k + 1])
    lights = LIGHTS.copy()
    lights[1] = p[0]  # light_dir = 0 / 0 for slot k: a NaN target, a NaN t_max, gated
    want, model_rays = sm.expected_counts(w.o, w.rays, w.hits, lights, RADII, S, seed=SEED, bias=BIAS)
    assert np.isnan(model_rays["tmax"].reshape(N_RAYS, 3, S)[k, 1]).all() and want[k, 1] == 0
    assert want[w.lit, 1].sum() > 0  # the light still lights other slots
    out = w.fused(f32_tensor(lights), f32_tensor(RADII), 3, S)
    torch.cuda.synchronize()
    w.t.wait_for_gpu()
    check(out, want, "a light on a hit point")
    assert words_of(out, N_RAYS * 3, np.uint32).reshape(N_RAYS, 3)[k, 1] == 0
