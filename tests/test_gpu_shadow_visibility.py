"""rc_shadow_visibility_device on the GPU: shadow visibility of all hits x all lights in one traversal launch, byte for byte against the
CPU oracle's composed stages (trace -> shadow_rays per light -> trace any), in the three kernel shapes the launcher dispatches (top level
in LDS, partial LDS, plain), against the product's own composed path (also with the entry cull on), with empty work, bad arguments, a
captured graph whose lights move between replays, two streams at once, and as the fused mode of WavefrontPaths."""
import numpy as np
import pytest

import bounce_model as bm
from gpu_kit import POISON, check_words, f32_tensor, poisoned
from gpu_kit import rc  # noqa: F401
from helpers import build_product
from worlds import C3World, three_shapes

pytestmark = pytest.mark.gpu

LIGHTS = np.array([[10, 10, 10], [-4, 6, 3], [3, 2.5, -6], [2, 20, 2]], np.float32)
BIAS = 1e-3
N_RAYS = 63_997  # 320 x 200 less three: n * L ends in the middle of a chunk for every L used here


def oracle_visibility(o, rays, want, lights):
    """visible[n, L] from the oracle alone: its primary hits `want`, then per light shadow_rays, the reference's t_max > 0 gate and any_hit.
    On these clean worlds every hit's shadow ray passes the gate (tests/test_gpu_stage_fuzz.py has the scenes where it does not)."""
    lit = want["hit"] == 1
    vis = np.zeros((len(rays), len(lights)), np.uint8)
    for l, light in enumerate(lights):
        shadow_rays = o.shadow_rays(rays, want, light, BIAS)
        assert np.all(shadow_rays["tmax"][lit] > 0), f"light {l}: a hit slot's shadow ray has a t_max that is not > 0"
        shadow = o.trace(shadow_rays, mode="any", nthreads=16)
        vis[:, l] = lit & (shadow_rays["tmax"] > 0) & (shadow["hit"] == 0)
    return vis


class World(C3World):
    def __init__(self, rc, oracle, lattice, kernel=None):
        super().__init__(rc, oracle, lattice, kernel)
        self.visible = oracle_visibility(self.o, self.rays, self.hits, LIGHTS)
        # a degenerate input cannot pass: (enough hits and misses, and) every light both shadowed and seen
        lit = self.lit
        for l in range(len(LIGHTS)):
            seen = int(self.visible[lit, l].sum())
            assert seen >= 100 and int(lit.sum()) - seen >= 100, (l, seen, int(lit.sum()) - seen)

    def fused(self, lights_t, n_lights):
        """One call on the current stream into a poisoned buffer; returns the tensor (n * n_lights bytes + the guard)."""
        out = poisoned(N_RAYS * n_lights)
        self.t.shadow_visibility_device(self.d_rays.data_ptr(), self.d_hits.data_ptr(), N_RAYS, lights_t.data_ptr(), n_lights, out.data_ptr(), bias=BIAS)
        return out


def check(out, want, what):
    """`out`: a tensor from World.fused, `want`: (n, L) bytes."""
    check_words(out, want, np.uint8, what)


@pytest.fixture(scope="module")
def worlds(rc, oracle):
    yield from three_shapes(World, rc, oracle)


# ---- (a), (c): every byte against the oracle, in the three shapes ------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["lds", "partial", "plain"])
@pytest.mark.parametrize("n_lights", [1, 3, 4])
def test_every_byte_matches_the_oracle(worlds, shape, n_lights):
    import torch
    w = worlds[shape]
    out = w.fused(f32_tensor(LIGHTS[:n_lights]), n_lights)
    torch.cuda.synchronize()
    w.t.wait_for_gpu()  # (a stack overflow would be reported here)
    check(out, w.visible[:, :n_lights], f"{shape} L={n_lights}")
    got = out.cpu().numpy()[:N_RAYS * n_lights].reshape(N_RAYS, n_lights)
    assert not got[w.hits["hit"] == 0].any(), "a slot whose primary ray missed is lit"  # (c)
    assert set(np.unique(got)) <= {0, 1}


# ---- (b): the product's own composed path gives the same bytes, with and without the entry cull ------------------------------------
@pytest.mark.parametrize("shape", ["lds", "partial", "plain"])
def test_composed_product_path_gives_the_same_bytes(worlds, shape):
    import torch
    w = worlds[shape]
    t, n = w.t, N_RAYS
    before = t.get_option("entry_cull")
    try:
        for cull in (before, 2):
            t.set_option("entry_cull", cull)
            composed = np.zeros((n, len(LIGHTS)), np.uint8)
            for l, light in enumerate(LIGHTS):
                d_sr, d_sh = poisoned(n * 32), poisoned(n * 32)
                t.shadow_rays_device(w.d_rays.data_ptr(), w.d_hits.data_ptr(), n, light, d_sr.data_ptr(), bias=BIAS)
                t.trace_device(d_sr.data_ptr(), d_sh.data_ptr(), n, mode="any")
                torch.cuda.synchronize()
                shadow = d_sh.cpu().numpy()[:n * 32].view(bm.HIT_DT)
                composed[:, l] = (w.hits["hit"] == 1) & (shadow["hit"] == 0)
            out = w.fused(f32_tensor(LIGHTS), len(LIGHTS))
            torch.cuda.synchronize()
            check(out, composed, f"{shape} entry_cull={cull} against the composed path")
            check(out, w.visible, f"{shape} entry_cull={cull} against the oracle")
    finally:
        t.set_option("entry_cull", before)


# ---- (d): empty work and refusals -----------------------------------------------------------------------------------------------
def test_empty_work_and_argument_checks(rc, worlds):
    import torch
    from raycore_jl_amd._capi import lib
    w = worlds["lds"]
    f, h = lib().rc_shadow_visibility_device, w.t._h
    d_l = f32_tensor(LIGHTS)
    out = poisoned(N_RAYS * 4)
    r, hh, lp, op = w.d_rays.data_ptr(), w.d_hits.data_ptr(), d_l.data_ptr(), out.data_ptr()
    INV, NS = 1, 6
    assert f(h, r, hh, 0, lp, 4, BIAS, op, None) == 0        # n == 0
    assert f(h, r, hh, N_RAYS, lp, 0, BIAS, op, None) == 0   # n_lights == 0
    assert f(h, None, None, 0, None, 4, BIAS, None, None) == 0 and f(h, None, None, N_RAYS, None, 0, BIAS, None, None) == 0  # no work: nothing is read
    torch.cuda.synchronize()
    assert bool((out == POISON).all()), "a call without work wrote to the output"
    assert f(None, r, hh, N_RAYS, lp, 4, BIAS, op, None) == INV
    assert f(h, None, hh, N_RAYS, lp, 4, BIAS, op, None) == INV
    assert f(h, r, None, N_RAYS, lp, 4, BIAS, op, None) == INV
    assert f(h, r, hh, N_RAYS, None, 4, BIAS, op, None) == INV
    assert f(h, r, hh, N_RAYS, lp, 4, BIAS, None, None) == INV
    assert f(h, r, hh, 1 << 30, lp, 4, BIAS, op, None) == INV           # n * n_lights == 2^32
    assert f(h, r, hh, (1 << 32) // 3 + 1, lp, 3, BIAS, op, None) == INV  # the first n past it for L = 3
    torch.cuda.synchronize()
    assert bool((out == POISON).all()), "a refused call wrote to the output"
    u = build_product(rc, rc.scenes.config_c1())
    u.push_instances(1, rc.scenes.IDENTITY3x4[None], np.zeros(1, np.uint32))  # a pending mutation
    assert f(u._h, r, hh, 16, lp, 4, BIAS, op, None) == NS
    u.free()
    torch.cuda.synchronize()
    assert bool((out == POISON).all())


# ---- (e): captured, with lights that move between replays -------------------------------------------------------------------------
def test_captured_call_follows_the_lights(worlds):
    import torch
    w = worlds["partial"]
    t, n, L = w.t, N_RAYS, len(LIGHTS)
    s = torch.cuda.Stream()
    d_l = f32_tensor(LIGHTS)
    d_hits = poisoned(n * 32)
    out = poisoned(n * L)

    def frame():
        t.trace_device(w.d_rays.data_ptr(), d_hits.data_ptr(), n, stream=s.cuda_stream)
        t.shadow_visibility_device(w.d_rays.data_ptr(), d_hits.data_ptr(), n, d_l.data_ptr(), L, out.data_ptr(), bias=BIAS, stream=s.cuda_stream)

    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        frame()  # the eager frame the capture needs
    torch.cuda.synchronize()
    check(out, w.visible, "eager frame")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        frame()
    perm = [2, 0, 3, 1]
    for lights, cols, what in ((None, [0, 1, 2, 3], "replay"), (LIGHTS[perm], perm, "replay with permuted lights")):
        if lights is not None:
            d_l.copy_(f32_tensor(lights))  # in place: the graph holds the tensor's address
        out.fill_(POISON)
        d_hits.fill_(POISON)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check(out, w.visible[:, cols], what)
    t.wait_for_gpu()
    del g
    torch.cuda.synchronize()
    t.set_option("release_captures", 1)  # the graph is gone: hand its captured launches back
    assert t.get_option("release_captures") == 0


# ---- (f): two streams at once ------------------------------------------------------------------------------------------------------
def test_two_streams_at_once(worlds):
    import torch
    w = worlds["lds"]
    sets = ([0, 1, 2], [3, 1])
    streams = [torch.cuda.Stream() for _ in sets]
    d_ls = [f32_tensor(LIGHTS[c]) for c in sets]
    outs = [[poisoned(N_RAYS * len(c)) for _ in range(3)] for c in sets]
    torch.cuda.synchronize()  # the buffers are filled on the current stream: done before the other streams write them
    for rep in range(3):  # enqueued alternately, never waited for in between
        for k, c in enumerate(sets):
            w.t.shadow_visibility_device(w.d_rays.data_ptr(), w.d_hits.data_ptr(), N_RAYS, d_ls[k].data_ptr(), len(c), outs[k][rep].data_ptr(), bias=BIAS,
                                         stream=streams[k].cuda_stream)
    torch.cuda.synchronize()
    w.t.wait_for_gpu()
    for k, c in enumerate(sets):
        for rep, out in enumerate(outs[k]):
            check(out, w.visible[:, c], f"stream {k} launch {rep}")


# ---- (g): the fused mode of WavefrontPaths --------------------------------------------------------------------------------------
def test_wavefront_fused_shadows(rc, worlds):
    import torch
    w = worlds["lds"]
    t, cfg = w.t, w.cfg
    width, height, spp, depth, seed = 64, 48, 2, 2, 0x5AD0
    cam = rc.wavefront.lookat_camera(cfg["eye"], cfg["lattice_centre"], width, height, 45.0)
    n, L = width * height * spp, len(LIGHTS)
    want = [np.zeros((n, L), np.uint8) for _ in range(depth)]
    hit_bytes = None
    for l, light in enumerate(LIGHTS):
        wf = rc.wavefront.WavefrontPaths(t, width, height, spp, depth, cam, light, seed=seed)
        assert len(wf.shadow_rays) == depth and len(wf.shadow_hits) == depth and wf.visible == [] and wf.lights is None  # the default construction
        assert wf.traced_rays() == n * 2 * depth and len(wf.buffers()) == 5 * depth + 2
        wf.run()
        torch.cuda.synchronize()
        for b in range(depth):
            hits, shadow = wf.hits[b].cpu().numpy().view(bm.HIT_DT), wf.shadow_hits[b].cpu().numpy().view(bm.HIT_DT)
            want[b][:, l] = (hits["hit"] == 1) & (shadow["hit"] == 0)
        these = [wf.hits[b].cpu().numpy().tobytes() for b in range(depth)]
        assert hit_bytes is None or these == hit_bytes  # the paths do not depend on the light
        hit_bytes = these
        del wf
    for b in range(depth):
        assert 0 < want[b].sum() < want[b].size, b
    d_l = f32_tensor(LIGHTS)
    s = torch.cuda.Stream()
    wf = rc.wavefront.WavefrontPaths(t, width, height, spp, depth, cam, lights=d_l, fused_shadows=True, seed=seed)
    assert wf.shadow_rays == [] and wf.shadow_hits == [] and len(wf.visible) == depth and wf.lights is d_l and wf.n_lights == L
    assert all(v.numel() == n * L and v.dtype == torch.uint8 for v in wf.visible)
    assert wf.traced_rays() == n * (1 + L) * depth and len(wf.buffers()) == 4 * depth + 3

    def check_frame(cols, what):
        for b in range(depth):
            assert wf.hits[b].cpu().numpy().tobytes() == hit_bytes[b], (what, b)
            got = wf.visible[b].cpu().numpy().reshape(n, L)
            bad = np.nonzero(got != want[b][:, cols])
            assert len(bad[0]) == 0, f"{what} depth {b}: {len(bad[0])} bytes differ, first {bad[0][:5]}, {bad[1][:5]}"

    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        wf.run(s)
    torch.cuda.synchronize()
    check_frame([0, 1, 2, 3], "eager")
    wf.capture(s)
    perm = [1, 3, 0, 2]
    for lights, cols, what in ((None, [0, 1, 2, 3], "replay"), (LIGHTS[perm], perm, "replay after an in-place edit of the lights")):
        if lights is not None:
            d_l.copy_(f32_tensor(lights))
        for v in wf.visible:
            v.fill_(POISON)
        torch.cuda.synchronize()
        wf.replay()
        torch.cuda.synchronize()
        check_frame(cols, what)
    # an array is uploaded once
    wf2 = rc.wavefront.WavefrontPaths(t, width, height, spp, 1, cam, lights=LIGHTS[:2].tolist(), fused_shadows=True, seed=seed)
    assert wf2.n_lights == 2 and wf2.lights.dtype == torch.float32 and wf2.lights.is_cuda
    wf2.run()
    torch.cuda.synchronize()
    assert np.array_equal(wf2.visible[0].cpu().numpy().reshape(n, 2), want[0][:, :2])
    t.wait_for_gpu()
    del wf, wf2
    torch.cuda.synchronize()
    t.set_option("release_captures", 1)
    assert t.get_option("release_captures") == 0
