"""rc_view_factor_groups_device / rc_view_factor_sampled_rays_device: weighted view-factor counts between groups of primitives with a
choice of sampling (the reference's uniform rays, or cosine-weighted ones: form factors).

The yardstick is the numpy model of tests/vf_groups_model.py: its rays (checked against the oracle's own in tests/test_vf_groups_model.py)
traced by the ORACLE, then the counting rule of the header.  A model trace is computed once per (scene, rays, seed, sampling) and shared.
Every comparison of integers is np.array_equal; there is no tolerance.  Covered: the stage rays; the three kernel shells x both samplings
x G in {1, 7, N} x weights (2^32 - 1 among them) x waves of one, two to three and 64 sources; the identity with view_factors and the
totals; the composed path on the device; irregular metadata and excluded groups; the analytic cube; an open scene; shards onto non-zero
words and a NULL escaped; both scratch paths; two streams; a captured call that follows rewritten groups and weights; a call behind a
device-side geometry update; an instanced scene; the error codes."""
import numpy as np
import pytest

import vf_groups_model as model
from gpu_kit import dev_u32, dev_u64, u64_of
from gpu_kit import rc  # noqa: F401
from helpers import assert_rays_equal, build_oracle
from scene_kit import meta, room_cfg
from worlds import VfWorld, room_world

pytestmark = pytest.mark.gpu

U32_MAX = model.U32_MAX
RC_ERR_INVALID_ARGUMENT = 1


class World(VfWorld):
    """One scene in the product and in the oracle; the model's traces are computed once per (rays, seed, sampling, shard) and only read."""

    def __init__(self, rc, oracle, cfg):
        super().__init__(rc, oracle, cfg)
        assert self.n == len(self.o.blas_prims)
        self._traced = {}

    def traced(self, rays, seed, sampling, src=None, shard=None):
        key = (rays, seed, sampling, src, shard)
        if key not in self._traced:
            self._traced[key] = model.Traced(self.o, rays, seed, sampling, src, shard)
        return self._traced[key]

    def run(self, groups, G, rays, seed, sampling, weights=None, escaped=True, src=None, shard=None, stream=None, start=None):
        """One device call into fresh (or `start`: G * G + G given) words; returns (matrix, escaped) after a full wait."""
        import torch
        d_g = dev_u32(groups)
        d_w = dev_u32(weights) if weights is not None else None
        out = dev_u64(start) if start is not None else torch.zeros(G * G + G, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        self.t.view_factor_groups_device(d_g.data_ptr(), G, out.data_ptr(), rays, seed, sampling, d_w.data_ptr() if d_w is not None else None,
                                         out.data_ptr() + 8 * G * G if escaped else None, src=src, rays=shard, stream=stream)
        torch.cuda.synchronize()
        self.t.wait_for_gpu()  # (a stack overflow would be reported here)
        words = u64_of(out)
        return words[:G * G].reshape(G, G).copy(), words[G * G:].copy()


@pytest.fixture(scope="module")
def room(rc, oracle):
    yield from room_world(World, rc, oracle)


def room_groups(n, G):
    return {1: np.zeros(n, np.uint32), 7: model.wall_groups(144, 2), n: np.arange(n, dtype=np.uint32)}[G]


def full_range_weights(n, seed):
    w = np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint32)
    w[:3] = (U32_MAX, 0, 1 << 31)
    return w


# ---- 1. the stage rays -------------------------------------------------------------------------------------------------------------------
def test_stage_rays_equal_the_models(rc, room):
    import torch
    from raycore_jl_amd._capi import check, lib, ptr
    n_ray, first, seed = 300, 5, 99
    prims = room.o.blas_prims
    buf, ref = torch.empty(n_ray * 32, dtype=torch.uint8, device="cuda"), torch.empty(n_ray * 32, dtype=torch.uint8, device="cuda")
    idx = np.arange(first, first + n_ray, dtype=np.uint64)
    for src in (0, 1, 17, 143, 144, room.n - 1):
        for sampling in ("uniform", "cosine"):
            buf.fill_(0x55)
            room.t.view_factor_sampled_rays_device(buf.data_ptr(), src, n_ray, seed=seed, sampling=sampling, ray_begin=first)
            torch.cuda.synchronize()
            got = buf.cpu().numpy().view(rc.RAY_DT)
            assert_rays_equal(got, model.sampled_rays(prims, src, idx, seed, sampling), f"source {src}, {sampling}")
            if sampling == "uniform":
                check(lib().rc_view_factor_rays_device(room.t._h, seed, src, first, n_ray, ptr(ref.data_ptr()), None))
                torch.cuda.synchronize()
                assert got.tobytes() == ref.cpu().numpy().tobytes(), src


# ---- 2. the fused call equals the model, in every shell --------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", ["uniform", "cosine"])
@pytest.mark.parametrize("kernel", [3, 5, 6, -1])
def test_fused_call_equals_the_model(room, kernel, sampling):
    n = room.n
    top = np.full(n, U32_MAX, np.uint32)  # a wave's sum of 64 rays carries past 32 bits
    room.t.set_option("kernel", kernel)
    try:
        for rays, seed in ((192, 77), (37, 21), (1, 22)):  # a wave holds one source / two or three / 64
            traced = room.traced(rays, seed, sampling)
            for G in (1, 7, n):
                groups = room_groups(n, G)
                for weights in (None, full_range_weights(n, 1), top):
                    got = room.run(groups, G, rays, seed, sampling, weights)
                    want = traced.count(groups, G, weights)
                    what = (kernel, sampling, rays, G, None if weights is None else int(weights[5]))
                    assert got[0].dtype == np.uint64 and np.array_equal(got[0], want[0]), what
                    assert np.array_equal(got[1], want[1]), what
                    if weights is top and G < n:
                        assert got[0].max() > U32_MAX and not (got[0] % np.uint64(U32_MAX)).any(), what
        assert room.t.last_kernel_ms() > 0
    finally:
        room.t.set_option("kernel", -1)


# ---- 3. identity groups, uniform, no weights: the reference's matrix and the totals ---------------------------------------------------------
def test_identity_groups_give_view_factors_and_the_totals(rc, room):
    n = room.n
    matrix, escaped = room.run(np.arange(n, dtype=np.uint32), n, 192, 77, "uniform")
    M = rc.view_factors(room.t, 192, seed=77)
    assert M.dtype == np.uint32 and np.array_equal(matrix, M.astype(np.uint64)) and not escaped.any()
    assert np.array_equal(matrix, room.o.view_factors(192, seed=77, nthreads=8).astype(np.uint64))
    received, emitted = rc.view_factor_totals(room.t, 192, seed=77)
    assert np.array_equal(matrix.sum(axis=0, dtype=np.uint64), received) and np.array_equal(matrix.sum(axis=1, dtype=np.uint64), emitted)
    # the host-array layer
    walls = model.wall_groups(144, 2)
    got = rc.view_factor_groups(room.t, walls, 192, seed=77)
    assert got.dtype == np.uint64 and np.array_equal(got, model.grouped_from_matrix(M, walls, 7))
    w = full_range_weights(n, 2)
    got, esc = rc.view_factor_groups(room.t, walls.astype(np.int64), 192, seed=77, weights=w, sampling="cosine", n_groups=9, return_escaped=True)
    want = room.traced(192, 77, "cosine").count(walls, 9, w)
    assert got.shape == (9, 9) and np.array_equal(got, want[0]) and np.array_equal(esc, want[1]) and not got[7:].any()
    with pytest.raises(ValueError, match="one value per primitive"):
        rc.view_factor_groups(room.t, walls[:-1], 192)


# ---- 4. the composed path on the device ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", ["uniform", "cosine"])
def test_composed_path_on_the_device(rc, room, sampling):
    import torch
    t, n, rays, seed = room.t, room.n, 37, 21
    d_rays = torch.empty(n * rays * 32, dtype=torch.uint8, device="cuda")
    d_hits = torch.empty(n * rays * 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for src in range(n):
        t.view_factor_sampled_rays_device(d_rays.data_ptr() + src * rays * 32, src, rays, seed=seed, sampling=sampling)
    t.trace_device(d_rays.data_ptr(), d_hits.data_ptr(), n * rays)
    torch.cuda.synchronize()
    t.wait_for_gpu()
    hits = d_hits.cpu().numpy().view(rc.HIT_DT)
    prims = t.adapt().all_blas_prims
    hit = hits["hit"] == 1
    a = np.repeat(prims["meta"].astype(np.int64), rays)
    b = np.zeros(n * rays, np.int64)
    b[hit] = prims["meta"][hits["primitive_id"][hit]]
    walls, w = model.wall_groups(144, 2), full_range_weights(n, 3)
    want = model.count(a, hit, b, n, walls, 7, w)
    got = room.run(walls, 7, rays, seed, sampling, w)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].any()


# ---- 5. irregular metadata, excluded groups, the analytic cube ------------------------------------------------------------------------------


@pytest.mark.parametrize("sampling", ["uniform", "cosine"])
def test_irregular_metadata_and_excluded_groups(rc, oracle, sampling):
    w = World(rc, oracle, room_cfg(rc, meta))
    n = w.n
    groups = (np.arange(n, dtype=np.uint32) * 7) % 11
    groups[20:30] = U32_MAX   # excluded whatever G is
    groups[60:70] = 11        # excluded because >= G
    groups[6] = 3             # the group of the 35 triangles that share metadata 7
    weights = full_range_weights(n, 4)
    traced = w.traced(128, 5, sampling)
    want = traced.count(groups, 11, weights)
    assert want[2].any() and want[0].any()  # rays onto metadata 0 / N + 50, onto the own metadata and onto excluded groups are dropped
    for k in (3, 5, 6):
        w.t.set_option("kernel", k)
        got = w.run(groups, 11, 128, 5, sampling, weights)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), k
    w.t.free()


def test_the_analytic_cube_equals_the_model(rc, oracle):
    verts = rc.scenes.box_room((0, 0, 0), (1, 1, 1), 2)
    w = World(rc, oracle, {"blas": [(verts, np.arange(1, len(verts) + 1, dtype=np.uint32))], "instances": [(1, rc.scenes.IDENTITY3x4[None], np.zeros(1, np.uint32))]})
    groups = model.wall_groups(0, 2)
    got = w.run(groups, 6, 4096, 5, "cosine")
    want = w.traced(4096, 5, "cosine").count(groups, 6)
    assert np.array_equal(got[0], want[0]) and not got[1].any() and (got[0].sum(axis=1) == 8 * 4096).all()
    sigma = np.sqrt(0.2 * 0.8 / 32768)
    F = got[0].astype(np.float64) / (8 * 4096)
    for a in range(6):
        for b in range(6):
            if a != b:
                assert abs(F[a, b] - (model.F_OPPOSITE if a // 2 == b // 2 else model.F_ADJACENT)) <= 4 * sigma, (a, b, F[a, b])
    # form_factors: area weights (all equal here), the same quotients
    F2, esc = rc.form_factors(w.t, groups, 4096, seed=5)
    assert F2.dtype == np.float64 and np.abs(F2 - F).max() < 1e-15 and not esc.any()
    assert np.allclose(rc.primitive_areas(w.t), 0.125, rtol=0, atol=1e-12)
    w.t.free()


# ---- 6. an open scene -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", ["uniform", "cosine"])
def test_open_scene_counts_the_escapes(rc, oracle, sampling):
    sc = rc.scenes
    verts = np.concatenate([sc.fan_sphere(12, 7, centre=(0, 0, 0), radius=0.5), sc.box_room((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5), 2)[:-8]])  # one wall left out
    n = len(verts)
    w = World(rc, oracle, {"blas": [(verts, np.arange(1, n + 1, dtype=np.uint32))], "instances": [(1, sc.IDENTITY3x4[None], np.zeros(1, np.uint32))]})
    groups = model.wall_groups(144, 2)[:n].copy()
    groups[150:154] = U32_MAX  # so that some hits stay uncounted
    weights = full_range_weights(n, 5)
    rays, seed = 96, 13
    want = w.traced(rays, seed, sampling).count(groups, 7, weights)
    assert want[1].any() and want[2].any() and want[0].any()
    got = w.run(groups, 7, rays, seed, sampling, weights)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    with np.errstate(over="ignore"):
        per_group = np.array([weights[groups == g].astype(np.uint64).sum(dtype=np.uint64) for g in range(7)], dtype=np.uint64) * np.uint64(rays)
        assert np.array_equal(got[0].sum(axis=1, dtype=np.uint64) + got[1] + want[2], per_group)
    # without escaped the matrix is the same
    only = w.run(groups, 7, rays, seed, sampling, weights, escaped=False)
    assert np.array_equal(only[0], want[0]) and not only[1].any()
    w.t.free()


# ---- 7. shards onto non-zero words, NULL escaped ------------------------------------------------------------------------------------------------
def test_shards_accumulate_onto_nonzero_words(room):
    import torch
    t, n, G = room.t, room.n, 7
    groups, weights = model.wall_groups(144, 2), full_range_weights(n, 6)
    want = room.traced(96, 11, "cosine").count(groups, G, weights)
    start = np.random.default_rng(3).integers(0, 1 << 64, G * G + G, dtype=np.uint64)  # accumulation modulo 2^64
    d_g, d_w, acc = dev_u32(groups), dev_u32(weights), dev_u64(start)
    st = torch.cuda.Stream()
    for buf in (d_g, d_w, acc):
        buf.record_stream(st)
    torch.cuda.synchronize()
    for src in ((0, n // 3), (n // 3, n)):
        for shard in ((0, 31), (31, 96)):
            t.view_factor_groups_device(d_g.data_ptr(), G, acc.data_ptr(), 96, 11, "cosine", d_w.data_ptr(), acc.data_ptr() + 8 * G * G, src=src, rays=shard,
                                        stream=st.cuda_stream)
    st.synchronize()
    t.wait_for_gpu()
    got = u64_of(acc)
    with np.errstate(over="ignore"):
        assert np.array_equal(got[:G * G], start[:G * G] + want[0].reshape(-1)) and np.array_equal(got[G * G:], start[G * G:] + want[1])
    # one shard against the model's own shard; ranges are clamped; empty ranges enqueue nothing
    part = room.traced(96, 11, "cosine", (n // 3, n), (31, 96)).count(groups, G, weights)
    got = room.run(groups, G, 96, 11, "cosine", weights, src=(n // 3, n + 1000), shard=(31, 1 << 20))
    assert np.array_equal(got[0], part[0]) and np.array_equal(got[1], part[1])
    for src, shard in (((n, n + 5), None), (None, (96, 200)), ((7, 7), None)):
        got = room.run(groups, G, 96, 11, "cosine", weights, src=src, shard=shard, start=start)
        assert np.array_equal(got[0].reshape(-1), start[:G * G]) and np.array_equal(got[1], start[G * G:])


# ---- 8. both scratch paths ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [3, 5, 6])
def test_copy_path_and_direct_path_give_the_models_words(room, kernel):
    """The private copies are used while they fit 256 MiB (G <= 1447 with escapes, G <= 1448 without): G = 7 and G = N count into them,
    G = 1448 with escapes and G = 1500 add straight onto the caller's words.  The same groups under both G give the same non-zero block."""
    t, n = room.t, room.n
    weights = full_range_weights(n, 7)
    spread = (np.arange(n, dtype=np.uint32) * 7) % 1400  # group numbers up to 1337: legal under every G used here
    traced = room.traced(37, 21, "cosine")
    t.set_option("kernel", kernel)
    try:
        blocks = {}
        for groups, G in ((room_groups(n, 7), 7), (room_groups(n, n), n), (spread, 1400), (spread, 1448), (spread, 1500)):
            want = traced.count(groups, G, weights)
            got = room.run(groups, G, 37, 21, "cosine", weights)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].any(), G
            only = room.run(groups, G, 37, 21, "cosine", weights, escaped=False)
            assert np.array_equal(only[0], want[0]) and not only[1].any(), G
            blocks[G] = got[0][:1400, :1400]
        assert np.array_equal(blocks[1400], blocks[1448]) and np.array_equal(blocks[1400], blocks[1500])  # copy path == direct path
    finally:
        t.set_option("kernel", -1)


# ---- 9. streams, capture, updates, instances ------------------------------------------------------------------------------------------------------
def test_two_streams_at_once(room):
    import torch
    t, n, G = room.t, room.n, 7
    groups = model.wall_groups(144, 2)
    wa, wb = full_range_weights(n, 8), full_range_weights(n, 9)
    wants = [room.traced(96, 11, "cosine").count(groups, G, wa), room.traced(96, 11, "uniform").count(groups, G, wb)]
    d_g, da, db = dev_u32(groups), dev_u32(wa), dev_u32(wb)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    v1, v2 = torch.zeros(G * G + G, dtype=torch.int64, device="cuda"), torch.zeros(G * G + G, dtype=torch.int64, device="cuda")
    for buf, st in ((d_g, s1), (d_g, s2), (da, s1), (v1, s1), (db, s2), (v2, s2)):
        buf.record_stream(st)
    torch.cuda.synchronize()
    for rep in range(3):
        v1.zero_(); v2.zero_()
        torch.cuda.synchronize()
        t.view_factor_groups_device(d_g.data_ptr(), G, v1.data_ptr(), 96, 11, "cosine", da.data_ptr(), v1.data_ptr() + 8 * G * G, stream=s1.cuda_stream)
        t.view_factor_groups_device(d_g.data_ptr(), G, v2.data_ptr(), 96, 11, "uniform", db.data_ptr(), v2.data_ptr() + 8 * G * G, stream=s2.cuda_stream)
        torch.cuda.synchronize()
        for v, want in zip((v1, v2), wants):
            g = u64_of(v)
            assert np.array_equal(g[:G * G].reshape(G, G), want[0]) and np.array_equal(g[G * G:], want[1]), rep
    t.wait_for_gpu()


def test_captured_call_follows_rewritten_groups_and_weights(rc, oracle):
    import torch
    w = World(rc, oracle, room_cfg(rc))  # a scene of its own: the captured launch is released with it
    t, n, G, rays, seed = w.t, w.n, 7, 48, 31
    traced = w.traced(rays, seed, "cosine")
    g0, w0 = model.wall_groups(144, 2), full_range_weights(n, 10)
    g1, w1 = ((np.arange(n, dtype=np.uint32) * 5) % 7).astype(np.uint32), full_range_weights(n, 11)
    g1[10:20] = U32_MAX
    d_g, d_w = dev_u32(g0), dev_u32(w0)
    out = torch.zeros(G * G + G, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    for buf in (d_g, d_w, out):
        buf.record_stream(st)
    torch.cuda.synchronize()

    def call(stream):
        out.zero_()
        t.view_factor_groups_device(d_g.data_ptr(), G, out.data_ptr(), rays, seed, "cosine", d_w.data_ptr(), out.data_ptr() + 8 * G * G, stream=stream)

    def check(groups, weights, what):
        want = traced.count(groups, G, weights)
        got = u64_of(out)
        assert np.array_equal(got[:G * G].reshape(G, G), want[0]) and np.array_equal(got[G * G:], want[1]), what

    with torch.cuda.stream(st):
        call(st.cuda_stream)  # eager first, as for every captured launch
    st.synchronize()
    check(g0, w0, "the eager call")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        call(torch.cuda.current_stream().cuda_stream)
    assert not np.array_equal(traced.count(g0, G, w0)[0], traced.count(g1, G, w1)[0])
    for groups, weights, what in ((g1, w1, "replay with new groups and weights"), (g0, w1, "replay with the first groups again")):
        with torch.cuda.stream(st):
            d_g.copy_(dev_u32(groups))  # in place: the graph reads the arrays when it runs
            d_w.copy_(dev_u32(weights))
            graph.replay()
        st.synchronize()
        check(groups, weights, what)
    del graph
    torch.cuda.synchronize()
    t.wait_for_gpu()
    t.set_option("release_captures", 1)
    assert t.get_option("release_captures") == 0
    t.free()


def test_after_a_geometry_update_on_the_same_stream(rc, oracle):
    import torch
    import dynamic_kit as dyn
    sc = rc.scenes
    verts = np.concatenate([sc.fan_sphere(12, 7, centre=(0, 0, 0), radius=0.5), sc.box_room((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5), 2)])
    n = len(verts)
    m = np.arange(1, n + 1, dtype=np.uint32)
    t = rc.TLAS()
    h = t.push_instances(t.add_geometry(verts, m), sc.IDENTITY3x4[None], np.zeros(1, np.uint32))
    t.sync()
    new_verts, new_meta = dyn.deform(verts, 1), np.ascontiguousarray(np.roll(m, 14))
    o = oracle.Scene()
    o.add_instance(o.add_blas(new_verts, new_meta), sc.IDENTITY3x4, 0)
    o.build()
    groups, weights, G, rays, seed = model.wall_groups(144, 2), full_range_weights(n, 12), 7, 64, 17
    want = model.Traced(o, rays, seed, "cosine").count(groups, G, weights)
    before = model.Traced(build_oracle(oracle, room_cfg(rc)), rays, seed, "cosine").count(groups, G, weights)
    assert not np.array_equal(want[0], before[0]) and want[0].any()
    s = torch.cuda.Stream()
    d_soup, d_meta = torch.from_numpy(new_verts).cuda(), dev_u32(new_meta)
    d_g, d_w = dev_u32(groups), dev_u32(weights)
    out = torch.zeros(G * G + G, dtype=torch.int64, device="cuda")
    for buf in (d_soup, d_meta, d_g, d_w, out):
        buf.record_stream(s)
    torch.cuda.synchronize()
    t.update_geometry_device_async(h, d_soup, d_meta=d_meta, stream=s.cuda_stream)
    t.refit_device_async(stream=s.cuda_stream)
    t.view_factor_groups_device(d_g.data_ptr(), G, out.data_ptr(), rays, seed, "cosine", d_w.data_ptr(), out.data_ptr() + 8 * G * G, stream=s.cuda_stream)
    s.synchronize()
    t.wait_for_gpu()
    got = u64_of(out)
    assert np.array_equal(got[:G * G].reshape(G, G), want[0]) and np.array_equal(got[G * G:], want[1])
    t.free()


@pytest.mark.parametrize("sampling", ["uniform", "cosine"])
def test_instanced_scene(rc, oracle, sampling):
    """Sources are the untransformed primitives of the BLAS (all_blas_prims, as in the reference); hits are counted by the metadata of the
    hit primitive whatever instance it sits in."""
    w = World(rc, oracle, rc.scenes.config_c3(lon=8, bands=5, lattice=(2, 2, 2)))
    groups = (np.arange(w.n, dtype=np.uint32) % 5).astype(np.uint32)
    weights = full_range_weights(w.n, 13)
    want = w.traced(64, 9, sampling).count(groups, 5, weights)
    got = w.run(groups, 5, 64, 9, sampling, weights)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].any()
    w.t.free()


# ---- 10. the error codes -----------------------------------------------------------------------------------------------------------------------
def test_error_codes(room):
    import torch
    from raycore_jl_amd._capi import lib, ptr
    L, t, n, G = lib(), room.t, room.n, 7
    d_g = dev_u32(model.wall_groups(144, 2))
    out = torch.zeros(G * G + G, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    g, m, e = ptr(d_g.data_ptr()), ptr(out.data_ptr()), ptr(out.data_ptr() + 8 * G * G)
    f = L.rc_view_factor_groups_device
    assert f(None, 16, 1, 0, 0, n, 0, 16, g, G, None, m, e, None) == RC_ERR_INVALID_ARGUMENT
    assert f(t._h, 16, 1, 0, 0, n, 0, 16, None, G, None, m, e, None) == RC_ERR_INVALID_ARGUMENT
    assert f(t._h, 16, 1, 0, 0, n, 0, 16, g, G, None, None, e, None) == RC_ERR_INVALID_ARGUMENT
    assert f(t._h, 16, 1, 2, 0, n, 0, 16, g, G, None, m, e, None) == RC_ERR_INVALID_ARGUMENT
    assert f(t._h, 16, 1, 0xFFFFFFFF, 0, n, 0, 16, g, G, None, m, e, None) == RC_ERR_INVALID_ARGUMENT
    for bad in (0, 65536, 0xFFFFFFFF):
        assert f(t._h, 16, 1, 0, 0, n, 0, 16, g, bad, None, m, e, None) == RC_ERR_INVALID_ARGUMENT
    s = L.rc_view_factor_sampled_rays_device
    d_rays = torch.zeros(16 * 32, dtype=torch.uint8, device="cuda")
    r = ptr(d_rays.data_ptr())
    assert s(None, 1, 0, 0, 0, 16, r, None) == RC_ERR_INVALID_ARGUMENT
    assert s(t._h, 1, 0, 0, 0, 16, None, None) == RC_ERR_INVALID_ARGUMENT
    assert s(t._h, 1, 2, 0, 0, 16, r, None) == RC_ERR_INVALID_ARGUMENT
    assert s(t._h, 1, 1, n, 0, 16, r, None) == RC_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    t.wait_for_gpu()
    assert not u64_of(out).any() and not d_rays.cpu().numpy().any()  # nothing was enqueued
    with pytest.raises(ValueError, match="sampling"):
        t.view_factor_groups_device(d_g.data_ptr(), G, out.data_ptr(), 16, 1, "lambert")
