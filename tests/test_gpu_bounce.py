"""rc_bounce_rays_device (diffuse bounce rays) and the chained wavefront frame (raycore.jl_amd/wavefront.py) on the GPU, against the numpy
model of tests/bounce_model.py and the CPU oracle's stages: bit-exact rays, dead slots that miss, traces of the bounce rays, the chained
frame eager and as a graph, argument checks and two host threads."""
import threading

import numpy as np
import pytest

import bounce_model as bm
from gpu_kit import dev
from gpu_kit import rc  # noqa: F401
from helpers import assert_hits_equal, build_oracle, build_product

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def c3(rc, oracle):
    cfg = rc.scenes.config_c3()
    t, o = build_product(rc, cfg), build_oracle(oracle, cfg)
    yield cfg, t, o
    t.free()


def empty_records(n):
    import torch
    return torch.full((n * 32,), 0xAB, dtype=torch.uint8, device="cuda")  # garbage: every record must be written


def host(t, dt):
    return t.cpu().numpy().view(dt)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def assert_rays_equal(got, want, what=""):
    bad = np.nonzero(got.view(np.uint32).reshape(-1, 8) != want.view(np.uint32).reshape(-1, 8))[0]
    assert len(bad) == 0, f"{what}: {len(np.unique(bad))} rays differ, first {np.unique(bad)[:5]}: got {got[bad[:2]]} want {want[bad[:2]]}"


def primary_hits(t, cfg, width, height):
    """C3 pinhole primary rays and their device hits (the device trace is bit-exact against the oracle: tests/test_gpu_parity.py)."""
    import torch
    from raycore_jl_amd import scenes
    rays = scenes.c3_primary_rays(cfg, width, height)
    d_r, d_h = dev(rays), empty_records(len(rays))
    t.trace_device(d_r.data_ptr(), d_h.data_ptr(), len(rays))
    torch.cuda.synchronize()
    return rays, host(d_h, bm.HIT_DT).copy(), d_r, d_h


# ---- 1. bit-exact against the model -----------------------------------------------------------------------------------------
def test_slot_aligned_c1(rc, oracle):
    import torch
    cfg = rc.scenes.config_c1()
    t, o = build_product(rc, cfg), build_oracle(oracle, cfg)
    rays = o.ray_grid(cfg["viewdir"], cfg["grid"])
    hits = o.trace(rays)
    assert 0 < hits["hit"].sum() < len(rays)
    d_r, d_h, d_out = dev(rays), dev(hits), empty_records(len(rays))
    d_path = torch.full((len(rays),), 7, dtype=torch.int32, device="cuda")
    for seed, bounce, bias in ((0, 0, 1e-3), (0xDEADBEEF_00C0FFEE, 7, 0.01), (1, 65535, 0.0)):
        t.bounce_rays_device(d_r.data_ptr(), d_h.data_ptr(), len(rays), d_out.data_ptr(), seed=seed, bounce=bounce, bias=bias,
                             d_path_out=d_path.data_ptr())
        torch.cuda.synchronize()
        want, want_path = bm.bounce_rays(o, rays, hits, len(rays), seed=seed, bounce=bounce, bias=bias)
        assert_rays_equal(host(d_out, bm.RAY_DT), want, f"C1 seed {seed:#x} bounce {bounce}")
        assert np.array_equal(u32(d_path), want_path)
    got = host(d_out, bm.RAY_DT)
    live = hits["hit"] == 1
    assert np.all(got["tmax"][~live] == -1) and np.all(got["d"][~live] == (0, 0, 1)) and np.all(np.isinf(got["tmax"][live]))
    t.free()


def test_slot_aligned_c3_4mi(rc, c3):
    import torch
    cfg, t, o = c3
    rays, hits, d_r, d_h = primary_hits(t, cfg, 2048, 2048)
    n = len(rays)
    assert n == 4 * 2 ** 20 and 0 < hits["hit"].sum() < n
    d_out = empty_records(n)
    t.bounce_rays_device(d_r.data_ptr(), d_h.data_ptr(), n, d_out.data_ptr(), seed=0xC3, bounce=1)
    torch.cuda.synchronize()
    got = host(d_out, bm.RAY_DT)
    for lo in range(0, n, 1 << 20):
        want, _ = bm.bounce_rays(o, rays, hits, 1 << 20, seed=0xC3, bounce=1, first=lo)
        assert_rays_equal(got[lo:lo + (1 << 20)], want, f"C3 4 Mi slots {lo}..")


def test_compacted_and_path_ids(rc, c3):
    """A live-first queue from rc_compact_hits_device's count word (read on the device), with d_path_in / d_path_out."""
    import torch
    cfg, t, o = c3
    rays, hits, d_r, d_h = primary_hits(t, cfg, 320, 240)
    n = len(rays)
    g = np.random.default_rng(5)
    path_in = g.permutation(n).astype(np.uint32) * np.uint32(3)  # any ids
    d_pin = dev(path_in)
    d_idx = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_out, d_pout = empty_records(n), torch.zeros(n, dtype=torch.int32, device="cuda")
    t.compact_hits_device(d_h.data_ptr(), n, d_idx.data_ptr(), d_cnt.data_ptr())
    t.bounce_rays_device(d_r.data_ptr(), d_h.data_ptr(), n, d_out.data_ptr(), seed=11, bounce=2, d_src=d_idx.data_ptr(),
                         d_src_count=d_cnt.data_ptr(), d_path_in=d_pin.data_ptr(), d_path_out=d_pout.data_ptr(), path_base=5 << 32)
    torch.cuda.synchronize()
    idx = np.nonzero(hits["hit"])[0]
    c = int(d_cnt.item())
    assert c == len(idx)
    want, want_path = bm.bounce_rays(o, rays, hits, n, seed=11, bounce=2, src=idx, count=c, path_in=path_in, path_base=5 << 32)
    assert_rays_equal(host(d_out, bm.RAY_DT), want, "compacted")
    assert np.array_equal(u32(d_pout), want_path)
    assert np.array_equal(want_path[:c], path_in[idx]) and np.all(want_path[c:] == bm.INVALID_ID)  # lo32(path): the base's high part drops
    # the same path through the slot-aligned queue gets the same ray: compaction does not change a path's random numbers
    d_al = empty_records(n)
    t.bounce_rays_device(d_r.data_ptr(), d_h.data_ptr(), n, d_al.data_ptr(), seed=11, bounce=2, d_path_in=d_pin.data_ptr(), path_base=5 << 32)
    torch.cuda.synchronize()
    assert host(d_al, bm.RAY_DT)[idx].tobytes() == host(d_out, bm.RAY_DT)[:c].tobytes()


def test_wrap_c4_size_on_device(rc, c3):
    """C4's shape made on the device (wavefront.c4_bounce_rays_device: compact, then wrap = 1): all 16 Mi outputs against the model."""
    import torch
    cfg, t, o = c3
    rays, hits, d_r, d_h = primary_hits(t, cfg, 2048, 2048)
    n_rays = 16 * 2 ** 20
    d_out = empty_records(n_rays)
    idx_t, cnt_t = rc.wavefront.c4_bounce_rays_device(t, d_r.data_ptr(), d_h.data_ptr(), len(rays), n_rays, d_out.data_ptr())
    torch.cuda.synchronize()
    idx = np.nonzero(hits["hit"])[0]
    assert int(cnt_t.item()) == len(idx) and np.array_equal(u32(idx_t)[:len(idx)], idx)
    got = host(d_out, bm.RAY_DT)
    assert np.all(np.isinf(got["tmax"]))  # every slot live under wrap
    chunk = 1 << 21
    for lo in range(0, n_rays, chunk):
        want, _ = bm.bounce_rays(o, rays, hits, chunk, seed=0xC4, src=idx, count=len(idx), wrap=True, first=lo)
        assert_rays_equal(got[lo:lo + chunk], want, f"C4 wrap slots {lo}..")
    del d_out


def test_split_batches_give_the_same_bytes(rc, c3):
    import torch
    cfg, t, o = c3
    rays, hits, d_r, d_h = primary_hits(t, cfg, 256, 200)
    n, h = len(rays), 20_011
    one = empty_records(n)
    t.bounce_rays_device(d_r.data_ptr(), d_h.data_ptr(), n, one.data_ptr(), seed=3, bounce=1)
    # two calls over offset source / output pointers: path_base = the first slot's index
    two = empty_records(n)
    t.bounce_rays_device(d_r.data_ptr(), d_h.data_ptr(), h, two.data_ptr(), seed=3, bounce=1)
    t.bounce_rays_device(d_r.data_ptr() + 32 * h, d_h.data_ptr() + 32 * h, n - h, two.data_ptr() + 32 * h, seed=3, bounce=1, path_base=h)
    # the same through an offset d_path_in
    ids = dev(np.arange(n, dtype=np.uint32))
    three = empty_records(n)
    t.bounce_rays_device(d_r.data_ptr(), d_h.data_ptr(), h, three.data_ptr(), seed=3, bounce=1, d_path_in=ids.data_ptr())
    t.bounce_rays_device(d_r.data_ptr() + 32 * h, d_h.data_ptr() + 32 * h, n - h, three.data_ptr() + 32 * h, seed=3, bounce=1,
                         d_path_in=ids.data_ptr() + 4 * h)
    torch.cuda.synchronize()
    assert one.cpu().numpy().tobytes() == two.cpu().numpy().tobytes() == three.cpu().numpy().tobytes()
    want, _ = bm.bounce_rays(o, rays, hits, n, seed=3, bounce=1)
    assert_rays_equal(host(one, bm.RAY_DT), want, "split")


# ---- 2. dead slots ------------------------------------------------------------------------------------------------------------
def test_dead_slots(rc, c3):
    import torch
    cfg, t, o = c3
    rays, hits, d_r, d_h = primary_hits(t, cfg, 128, 96)
    n = len(rays)
    idx = np.nonzero(hits["hit"])[0].astype(np.uint32)
    d_idx = dev(idx)
    for count in (0, 1, len(idx) // 2):
        d_cnt = dev(np.array([count], np.uint32))
        for wrap in (False, True):
            d_out, d_pout = empty_records(n), torch.zeros(n, dtype=torch.int32, device="cuda")
            t.bounce_rays_device(d_r.data_ptr(), d_h.data_ptr(), n, d_out.data_ptr(), seed=9, d_src=d_idx.data_ptr(), d_src_count=d_cnt.data_ptr(),
                                 wrap=wrap, d_path_out=d_pout.data_ptr())
            torch.cuda.synchronize()
            want, want_path = bm.bounce_rays(o, rays, hits, n, seed=9, src=idx, count=count, wrap=wrap)
            assert_rays_equal(host(d_out, bm.RAY_DT), want, f"count {count} wrap {wrap}")
            assert np.array_equal(u32(d_pout), want_path)
            live = 0 if count == 0 else (n if wrap else count)
            got = host(d_out, bm.RAY_DT)
            assert np.sum(got["tmax"] == -1) == n - live


def test_dead_rays_miss_a_triangle_through_the_origin(rc, oracle):
    import torch
    tri = np.array([[-1, -1, 0, 1, -1, 0, 0, 1, 0], [-1, 0, -1, 1, 0, -1, 0, 0, 1]], np.float32)  # both contain the origin
    cfg = {"blas": [(tri, None)], "instances": [(1, rc.scenes.IDENTITY3x4[None], np.zeros(1, np.uint32))]}
    t, o = build_product(rc, cfg), build_oracle(oracle, cfg)
    n = 1000
    rays = oracle.make_rays(np.zeros((n, 3)), (0, 0, 1))
    hits = np.zeros(n, bm.HIT_DT)  # all misses: every slot dead
    d_r, d_h, d_out = dev(rays), dev(hits), empty_records(n)
    t.bounce_rays_device(d_r.data_ptr(), d_h.data_ptr(), n, d_out.data_ptr())
    torch.cuda.synchronize()
    dead = host(d_out, bm.RAY_DT).copy()
    assert np.all(dead["tmax"] == -1) and np.all(dead["o"] == 0) and np.all(dead["d"] == (0, 0, 1)) and np.all(dead["tmin"] == 0)
    # the shadow stage's [0, 0] dummy does reach the triangles at t = 0; [0, -1] does not
    for mode in ("closest", "any"):
        d_hh = empty_records(n)
        t.trace_device(d_out.data_ptr(), d_hh.data_ptr(), n, mode=mode)
        torch.cuda.synchronize()
        got = host(d_hh, bm.HIT_DT)
        want = o.trace(dead, mode=mode)
        assert_hits_equal(got, want, f"dead rays {mode}")
        assert not got["hit"].any()
    t.free()


# ---- 3. tracing the device-made bounce rays ----------------------------------------------------------------------------------
def test_trace_of_bounce_rays_matches_oracle(rc, c3):
    import torch
    cfg, t, o = c3
    rays, hits, d_r, d_h = primary_hits(t, cfg, 512, 512)
    n_rays = 1 << 19
    d_out = empty_records(n_rays)
    rc.wavefront.c4_bounce_rays_device(t, d_r.data_ptr(), d_h.data_ptr(), len(rays), n_rays, d_out.data_ptr())
    torch.cuda.synchronize()
    bounce = host(d_out, bm.RAY_DT).copy()
    for mode in ("closest", "any"):
        d_bh = empty_records(n_rays)
        t.trace_device(d_out.data_ptr(), d_bh.data_ptr(), n_rays, mode=mode)
        torch.cuda.synchronize()
        got = host(d_bh, bm.HIT_DT)
        want = o.trace(bounce, mode=mode, nthreads=16)
        assert_hits_equal(got, want, f"bounce rays {mode}")
        assert 0 < got["hit"].sum() < n_rays


# ---- 4. the chained frame -------------------------------------------------------------------------------------------------------
def c3_camera(rc, cfg, width, height):
    return rc.wavefront.lookat_camera(cfg["eye"], cfg["lattice_centre"], width, height, 45.0)


def frame_buffers(wf):
    out = []
    for b in range(wf.depth):
        out.append((host(wf.rays[b], bm.RAY_DT).copy(), host(wf.hits[b], bm.HIT_DT).copy(), host(wf.shadow_rays[b], bm.RAY_DT).copy(),
                    host(wf.shadow_hits[b], bm.HIT_DT).copy(), u32(wf.path_ids[b]).copy()))
    return out


def oracle_chain(o, cam, light, width, height, spp, depth, seed, bias, compact, sample=None):
    """The oracle's frame: primary_rays_lookat -> trace -> (shadow_rays -> trace any, model bounce -> trace) per depth.  `sample`: only these
    primary slots (slot-aligned mode: slot i stays on path i)."""
    from oracle import pyoracle as po
    rays = po.primary_rays_lookat(cam["pos"], cam["right"], cam["up"], cam["forward"], cam["half_width"], cam["half_height"], width, height,
                                  spp, seed, True)
    paths = np.arange(len(rays), dtype=np.uint32)
    if sample is not None:
        rays, paths = rays[sample], paths[sample]
    out = []
    for b in range(depth):
        hits = o.trace(rays, nthreads=16)
        sh = o.shadow_rays(rays, hits, light, bias)
        out.append((rays, hits, sh, o.trace(sh, mode="any", nthreads=16), paths))
        if b + 1 < depth:
            if compact:
                idx = np.nonzero(hits["hit"])[0]
                rays, paths = bm.bounce_rays(o, rays, hits, len(rays), seed=seed, bounce=b, bias=bias, src=idx, count=len(idx), path_in=paths)
            else:
                rays, paths = bm.bounce_rays(o, rays, hits, len(rays), seed=seed, bounce=b, bias=bias, path_in=paths)
    return out


def assert_frames_equal(got, want, what):
    for b, (g, w) in enumerate(zip(got, want)):
        assert_rays_equal(g[0], w[0], f"{what} rays depth {b}")
        assert_hits_equal(g[1], w[1], f"{what} hits depth {b}")
        assert_rays_equal(g[2], w[2], f"{what} shadow rays depth {b}")
        assert_hits_equal(g[3], w[3], f"{what} shadow hits depth {b}")
        assert np.array_equal(g[4], w[4]), f"{what} path ids depth {b}"


def path_records(frame):
    """(path id -> hit record) per depth, for the live slots."""
    recs = []
    for rays, hits, _, shadow_hits, paths in frame:
        live = paths != bm.INVALID_ID
        order = np.argsort(paths[live], kind="stable")
        recs.append((paths[live][order].tobytes(), hits[live][order].tobytes(), shadow_hits[live][order].tobytes(), rays[live][order].tobytes()))
    return recs


def test_wavefront_frame_small(rc, c3):
    import torch
    cfg, t, o = c3
    w, h, spp, depth = 64, 48, 2, 3
    cam, light = c3_camera(rc, cfg, w, h), cfg["light"].astype(np.float32)
    frames = {}
    for compact in (True, False):
        wf = rc.wavefront.WavefrontPaths(t, w, h, spp, depth, cam, light, seed=0x5EED, compact=compact)
        wf.run()
        torch.cuda.synchronize()
        got = frame_buffers(wf)
        assert_frames_equal(got, oracle_chain(o, cam, light, w, h, spp, depth, 0x5EED, 1e-3, compact), f"compact={compact}")
        frames[compact] = got
    assert 0 < (frames[True][2][4] != bm.INVALID_ID).sum() < w * h * spp  # some paths survive two bounces, not all
    a, b = path_records(frames[True]), path_records(frames[False])
    for d in range(depth):
        assert all(x == y for x, y in zip(a[d], b[d])), d


def test_wavefront_frame_tutorial_size(rc, c3):
    """The reference tutorial's 720 x 400 x 4 spp frame, depth 3: a strided sample of paths against the oracle chain (slot-aligned), and the
    compacted frame's (path id -> hit) records against the slot-aligned frame's, in full."""
    import torch
    cfg, t, o = c3
    w, h, spp, depth = 720, 400, 4, 3
    cam, light = c3_camera(rc, cfg, w, h), cfg["light"].astype(np.float32)
    frames = {}
    for compact in (False, True):
        wf = rc.wavefront.WavefrontPaths(t, w, h, spp, depth, cam, light, seed=0x7070, compact=compact)
        wf.run()
        torch.cuda.synchronize()
        frames[compact] = frame_buffers(wf)
        del wf
    sample = np.arange(3, w * h * spp, 7)
    want = oracle_chain(o, cam, light, w, h, spp, depth, 0x7070, 1e-3, False, sample=sample)
    got = [tuple(x[sample] for x in f) for f in frames[False]]
    assert_frames_equal(got, want, "tutorial sample")
    a, b = path_records(frames[True]), path_records(frames[False])
    for d in range(depth):
        assert all(x == y for x, y in zip(a[d], b[d])), d


# ---- 5. graph -------------------------------------------------------------------------------------------------------------------
def test_wavefront_frame_graph_replay(rc, c3):
    import torch
    cfg, t, o = c3
    w, h, spp, depth = 64, 48, 2, 3
    cam, light = c3_camera(rc, cfg, w, h), cfg["light"].astype(np.float32)
    s = torch.cuda.Stream()
    wf = rc.wavefront.WavefrontPaths(t, w, h, spp, depth, cam, light, seed=0x6A, compact=True)
    with torch.cuda.stream(s):
        wf.run(s)
    torch.cuda.synchronize()
    eager = frame_buffers(wf)
    extra = (wf.indices.cpu().numpy().tobytes(), wf.count.cpu().numpy().tobytes())
    wf.capture(s)
    for rep in range(2):
        for buf in wf.rays + wf.hits + wf.shadow_rays + wf.shadow_hits + wf.path_ids[1:]:
            buf.fill_(0x5A if buf.dtype == torch.uint8 else 12345)
        wf.count.zero_()
        torch.cuda.synchronize()
        wf.replay()
        torch.cuda.synchronize()
        got = frame_buffers(wf)
        for b in range(depth):
            for x, y in zip(got[b], eager[b]):
                assert x.tobytes() == y.tobytes(), (rep, b)
        assert (wf.indices.cpu().numpy().tobytes(), wf.count.cpu().numpy().tobytes()) == extra
    del wf
    torch.cuda.synchronize()
    t.set_option("release_captures", 1)  # the graph is gone: hand its captured launches back
    assert t.get_option("release_captures") == 0


# ---- 6. argument checks ---------------------------------------------------------------------------------------------------------
def test_argument_checks(rc, c3):
    import torch
    from raycore_jl_amd._capi import lib
    cfg, t, o = c3
    L, h = lib(), t._h
    buf = torch.zeros(64 * 32, dtype=torch.uint8, device="cuda")
    w = torch.zeros(64, dtype=torch.int32, device="cuda")
    p, q = buf.data_ptr(), w.data_ptr()
    INV, NS = 1, 6

    def call(scene=h, rays=p, hits=p, src=None, cnt=None, wrap=0, n=16, bounce=0, out=p):
        return L.rc_bounce_rays_device(scene, rays, hits, src, cnt, wrap, None, None, 0, n, 0, bounce, 1e-3, out, None)

    assert call() == 0
    assert call(scene=None) == INV
    assert call(rays=None) == INV and call(hits=None) == INV and call(out=None) == INV
    assert call(rays=None, hits=None, out=None, n=0) == 0  # n_out == 0: nothing to read or write
    assert call(src=q) == INV and call(cnt=q) == INV
    assert call(wrap=1) == INV
    assert call(src=q, cnt=q, wrap=1) == 0
    assert call(bounce=65536) == INV and call(bounce=65535) == 0
    assert call(n=1 << 32) == INV
    torch.cuda.synchronize()
    # n_out == 0 writes nothing
    buf.fill_(0x33)
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert bool((buf == 0x33).all())
    # an unsynced scene
    u = build_product(rc, rc.scenes.config_c1())
    u.push_instances(1, rc.scenes.IDENTITY3x4[None], np.zeros(1, np.uint32))  # a pending mutation
    assert L.rc_bounce_rays_device(u._h, p, p, None, None, 0, None, None, 0, 16, 0, 0, 1e-3, p, None) == NS
    u.free()


# ---- 7. two host threads ----------------------------------------------------------------------------------------------------------
def test_two_threads_two_streams(rc, c3):
    import torch
    cfg, t, o = c3
    rays, hits, d_r, d_h = primary_hits(t, cfg, 512, 384)
    n = len(rays)
    outs = {seed: empty_records(n) for seed in (101, 202)}
    errors = []

    def worker(seed):
        try:
            s = torch.cuda.Stream()
            for _ in range(20):
                t.bounce_rays_device(d_r.data_ptr(), d_h.data_ptr(), n, outs[seed].data_ptr(), seed=seed, bounce=1, stream=s.cuda_stream)
            s.synchronize()
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(e)

    th = [threading.Thread(target=worker, args=(seed,)) for seed in outs]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
    for seed, buf in outs.items():
        want, _ = bm.bounce_rays(o, rays, hits, n, seed=seed, bounce=1)
        assert_rays_equal(host(buf, bm.RAY_DT), want, f"thread seed {seed}")
