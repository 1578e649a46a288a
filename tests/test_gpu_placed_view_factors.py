"""rc_placed_primitive_bases / rc_placed_triangles_device / rc_placed_view_factor_rays_device / rc_placed_view_factor_groups_device: the
grouped view-factor job with its sources in world space, counted per placed primitive (instance, local primitive).

The yardstick is the numpy model of tests/placed_vf_model.py (checked on the CPU in tests/test_placed_vf_model.py): its world triangles and
rays, traced by the ORACLE, then the rule of the header.  A model trace is computed once per (scene, rays, seed, sampling, shard) and
shared.  Every comparison of integers is np.array_equal; there is no tolerance but the plates' 4 sigma against the analytic form factor,
which the CPU test derives."""
import numpy as np
import pytest

import placed_vf_model as model
import vf_groups_model as sibling
from gpu_kit import dev_u32, dev_u64, f32_tensor, u64_of
from gpu_kit import rc  # noqa: F401
from helpers import assert_f32_bits_equal, assert_rays_equal, build_oracle, build_product
from worlds import VfWorld, room_world

pytestmark = pytest.mark.gpu

U32_MAX = model.U32_MAX
RC_ERR_INVALID_ARGUMENT, RC_ERR_NOT_SYNCED = 1, 6
PLATES_RAYS, PLATES_SEED = 4096, 5  # tests/test_placed_vf_model.py's
SIGMA = np.sqrt(0.2 * 0.8 / 32768)


def call(t, groups, G, rays, seed, sampling, weights=None, escaped=True, placed=None, shard=None, stream=None, start=None):
    """One device call into fresh (or `start`: G * G + G given) words; returns (matrix, escaped) after a full wait."""
    import torch
    d_g = dev_u32(groups)
    d_w = dev_u32(weights) if weights is not None else None
    out = dev_u64(start) if start is not None else torch.zeros(G * G + G, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    t.placed_view_factor_groups_device(d_g.data_ptr(), G, out.data_ptr(), rays, seed, sampling, d_w.data_ptr() if d_w is not None else None,
                                       out.data_ptr() + 8 * G * G if escaped else None, placed=placed, rays=shard, stream=stream)
    torch.cuda.synchronize()
    t.wait_for_gpu()  # (a stack overflow would be reported here)
    words = u64_of(out)
    return words[:G * G].reshape(G, G).copy(), words[G * G:].copy()


class World:
    """One scene in the product and in the oracle; the model's traces are computed once per job and only read."""

    def __init__(self, rc, oracle, cfg):
        self.rc, self.cfg = rc, cfg
        self.t, self.o = build_product(rc, cfg), build_oracle(oracle, cfg)
        self.base = model.bases(self.o)
        self.P = int(self.base[-1])
        self._traced = {}

    def traced(self, rays, seed, sampling, placed=None, shard=None):
        key = (rays, seed, sampling, placed, shard)
        if key not in self._traced:
            self._traced[key] = model.Traced(self.o, rays, seed, sampling, placed, shard)
        return self._traced[key]

    def run(self, groups, G, rays, seed, sampling, weights=None, **kw):
        return call(self.t, groups, G, rays, seed, sampling, weights, **kw)

    def instance_groups(self):
        return np.repeat(np.arange(len(self.base) - 1, dtype=np.uint32), np.diff(self.base.astype(np.int64)))


@pytest.fixture(scope="module")
def mixed(rc, oracle):
    w = World(rc, oracle, model.mixed_cfg(rc))
    assert w.P == 640 and w.t.n_primitives() == 192 and w.t.n_instances() == 8
    yield w
    w.t.free()


@pytest.fixture(scope="module")
def lattice(rc, oracle):
    w = World(rc, oracle, rc.scenes.config_c3(lon=8, bands=5, lattice=(2, 2, 2)))
    assert w.P == 8 * w.t.n_primitives()
    yield w
    w.t.free()


def full_range_weights(n, seed):
    w = np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint32)
    w[:3] = (U32_MAX, 0, 1 << 31)
    return w


def mixed_groups(w, G):
    """G = 1: everything; G = 7: the seven bodies, the room (group 7) excluded because >= G; G = P: every placed primitive."""
    return {1: np.zeros(w.P, np.uint32), 7: w.instance_groups(), w.P: np.arange(w.P, dtype=np.uint32)}[G]


# ---- 1. the exports ----------------------------------------------------------------------------------------------------------------------
def test_bases_and_world_triangles(rc, mixed):
    import torch
    t = mixed.t
    base = t.placed_primitive_bases()
    assert base.dtype == np.uint32 and np.array_equal(base, mixed.base) and rc.placed_primitive_count(t) == mixed.P
    inst = t.adapt().instances
    prims_per_blas = np.diff(np.append(t.adapt().blas_descriptors["primitives_offset"], t.n_primitives()))
    assert np.array_equal(np.diff(base.astype(np.int64)), prims_per_blas[inst["blas_index"].astype(np.int64) - 1])
    want = model.world_triangles(mixed.o).reshape(-1, 9)
    for q0, n in ((0, mixed.P), (150, 20), (mixed.P - 1, 1), (8, 0)):  # all; across the boundary between instances 1 and 2 (base 152); the last; none
        buf = torch.full((9 * n + 16,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        t.placed_triangles_device(buf.data_ptr(), q0, n)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert np.isnan(got[9 * n:]).all()
        if n:
            assert_f32_bits_equal(got[:9 * n].reshape(-1, 9), want[q0:q0 + n], f"placed triangles {q0}..{q0 + n}")
    areas = rc.placed_primitive_areas(t)
    v = want.reshape(-1, 3, 3).astype(np.float64)
    assert areas.dtype == np.float64 and np.array_equal(areas, 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1))
    assert np.array_equal(rc.placed_groups(t), mixed.instance_groups())


# ---- 2. the stage rays -------------------------------------------------------------------------------------------------------------------
def test_stage_rays_equal_the_models(rc, mixed):
    import torch
    n_ray, first, seed = 300, 5, 99
    buf = torch.empty(n_ray * 32, dtype=torch.uint8, device="cuda")
    idx = np.arange(first, first + n_ray, dtype=np.uint64)
    b = mixed.base.astype(np.int64)
    # the first and last placed primitive of: the first square, the mirrored square, the scaled and rotated sphere, the last sphere, the room
    for q in (0, 7, b[2], b[3] - 1, b[3], b[4] - 1, b[6], b[7] - 1, b[7], mixed.P - 1):
        for sampling in model.SAMPLINGS:
            buf.fill_(0x55)
            mixed.t.placed_view_factor_rays_device(buf.data_ptr(), int(q), n_ray, seed=seed, sampling=sampling, ray_begin=first)
            torch.cuda.synchronize()
            assert_rays_equal(buf.cpu().numpy().view(rc.RAY_DT), model.placed_rays(mixed.o, int(q), idx, seed, sampling), f"placed primitive {q}, {sampling}")


# ---- 3. the fused call equals the model, in every shell ------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", ["uniform", "cosine"])
@pytest.mark.parametrize("kernel", [3, 5, 6, -1])
def test_fused_call_equals_the_model(mixed, kernel, sampling):
    P = mixed.P
    top = np.full(P, U32_MAX, np.uint32)  # a wave's sum of 64 rays carries past 32 bits
    mixed.t.set_option("kernel", kernel)
    try:
        for rays, seed in ((192, 77), (37, 21), (1, 22)):  # a wave holds one source / two or three / 64 across instance boundaries
            traced = mixed.traced(rays, seed, sampling)
            for G in (1, 7, P):
                groups = mixed_groups(mixed, G)
                for weights in (None, full_range_weights(P, 1), top):
                    got = mixed.run(groups, G, rays, seed, sampling, weights)
                    want = traced.count(groups, G, weights)
                    what = (kernel, sampling, rays, G, None if weights is None else int(weights[5]))
                    assert got[0].dtype == np.uint64 and np.array_equal(got[0], want[0]), what
                    assert np.array_equal(got[1], want[1]), what
                    assert want[0].any() and want[1].any(), what
                    if weights is top and G < P:
                        assert got[0].max() > U32_MAX, what
        assert mixed.t.last_kernel_ms() > 0
    finally:
        mixed.t.set_option("kernel", -1)


@pytest.mark.parametrize("shape", [(3, 3, 2), (7, 7, 6)])
def test_the_scenes_own_choice_of_shell(rc, oracle, shape):
    """18 instances: the whole top level in LDS; 294: only the top of the TLAS is staged.  The launcher chooses, no option is set."""
    w = World(rc, oracle, rc.scenes.config_c3(lon=8, bands=5, lattice=shape))
    n_inst = shape[0] * shape[1] * shape[2]
    assert w.t.n_instances() == n_inst and w.P == n_inst * 64
    groups = (np.arange(n_inst, dtype=np.uint32) % 11).repeat(64)
    weights = full_range_weights(w.P, 14)
    want = w.traced(5, 3, "cosine").count(groups, 11, weights)
    got = w.run(groups, 11, 5, 3, "cosine", weights)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].any() and got[1].any()
    w.t.free()


# ---- 4. the composed path on the device --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", ["uniform", "cosine"])
def test_composed_path_on_the_device(rc, lattice, sampling):
    import torch
    t, P, rays, seed = lattice.t, lattice.P, 37, 21
    d_rays = torch.empty(P * rays * 32, dtype=torch.uint8, device="cuda")
    d_hits = torch.empty(P * rays * 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for q in range(P):
        t.placed_view_factor_rays_device(d_rays.data_ptr() + q * rays * 32, q, rays, seed=seed, sampling=sampling)
    t.trace_device(d_rays.data_ptr(), d_hits.data_ptr(), P * rays)
    torch.cuda.synchronize()
    t.wait_for_gpu()
    hits = d_hits.cpu().numpy().view(rc.HIT_DT)
    static = t.adapt()
    offs = static.blas_descriptors["primitives_offset"].astype(np.int64)[static.instances["blas_index"].astype(np.int64) - 1]
    a = np.repeat(np.arange(P, dtype=np.int64), rays)
    b = model.placed_hits(hits, t.placed_primitive_bases(), offs)
    groups, w = lattice.instance_groups(), full_range_weights(P, 3)
    want = model.count(a, hits["hit"] == 1, b, P, groups, 8, w)
    got = lattice.run(groups, 8, rays, seed, sampling, w)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].any() and got[1].any()
    model_want = lattice.traced(rays, seed, sampling).count(groups, 8, w)
    assert np.array_equal(got[0], model_want[0]) and np.array_equal(got[1], model_want[1])


# ---- 5. one identity instance: the sibling's words ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def room(rc, oracle):
    yield from room_world(VfWorld, rc, oracle)


@pytest.mark.parametrize("sampling", ["uniform", "cosine"])
def test_identity_instance_gives_the_siblings_words(room, sampling):
    import torch
    t, n, G, rays, seed = room.t, room.n, 7, 64, 9
    assert np.array_equal(t.placed_primitive_bases(), [0, n])
    meta = t.adapt().all_blas_prims["meta"].astype(np.int64)
    assert np.array_equal(np.sort(meta), np.arange(1, n + 1))
    groups, weights = sibling.wall_groups(144, 2), full_range_weights(n, 2)
    gq, wq = groups[meta - 1], weights[meta - 1]  # placed primitive q of the one instance is flat primitive q
    d_g, d_w = dev_u32(groups), dev_u32(weights)
    ref = torch.zeros(G * G + G, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    t.view_factor_groups_device(d_g.data_ptr(), G, ref.data_ptr(), rays, seed, sampling, d_w.data_ptr(), ref.data_ptr() + 8 * G * G)
    torch.cuda.synchronize()
    want = u64_of(ref)
    got = call(t, gq, G, rays, seed, sampling, wq)
    assert want.any() and np.array_equal(got[0].reshape(-1), want[:G * G]) and np.array_equal(got[1], want[G * G:])


# ---- 6. the two plates -------------------------------------------------------------------------------------------------------------------
def test_the_two_plates(rc, oracle):
    w = World(rc, oracle, model.plates_cfg(rc))
    assert w.P == 16 and np.array_equal(w.t.placed_primitive_bases(), [0, 8, 16])
    groups = w.instance_groups()
    want = w.traced(PLATES_RAYS, PLATES_SEED, "cosine").count(groups, 2)
    got = w.run(groups, 2, PLATES_RAYS, PLATES_SEED, "cosine")
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    total = 8 * PLATES_RAYS
    F = got[0].astype(np.float64) / total
    print("plates: F[0, 1] = %.6f, F[1, 0] = %.6f, analytic %.6f, 4 sigma = %.6f" % (F[0, 1], F[1, 0], sibling.F_OPPOSITE, 4 * SIGMA))
    for a, b in ((0, 1), (1, 0)):
        assert abs(F[a, b] - sibling.F_OPPOSITE) <= 4 * SIGMA, (a, b, F[a, b])
    assert np.array_equal(got[0].sum(axis=1, dtype=np.uint64) + got[1], np.full(2, total, np.uint64))
    assert np.allclose(rc.placed_primitive_areas(w.t), 0.125, rtol=0, atol=1e-12)
    F2, esc = rc.instance_form_factors(w.t, PLATES_RAYS, seed=PLATES_SEED)
    assert F2.dtype == np.float64 and F2.shape == (2, 2) and np.abs(F2 - F).max() < 1e-15 and np.abs(esc - got[1] / total).max() < 1e-15
    w.t.free()


# ---- 7. the call follows a device-side move ----------------------------------------------------------------------------------------------
def test_follows_a_device_side_move(rc, oracle):
    import torch
    cfg = model.plates_cfg(rc)
    t = build_product(rc, cfg)
    h = t.handles[0]
    groups, weights, G, rays, seed = np.repeat(np.arange(2, dtype=np.uint32), 8), full_range_weights(16, 6), 2, 512, 31
    wants = {z: model.Traced(build_oracle(oracle, model.plates_cfg(rc, z)), rays, seed, "cosine").count(groups, G, weights) for z in (1.0, 2.0, 3.0)}
    assert wants[1.0][0].any() and not np.array_equal(wants[1.0][0], wants[2.0][0]) and not np.array_equal(wants[2.0][0], wants[3.0][0])
    before = call(t, groups, G, rays, seed, "cosine", weights)
    assert np.array_equal(before[0], wants[1.0][0]) and np.array_equal(before[1], wants[1.0][1])

    def xf(z):
        return f32_tensor(np.stack([rc.scenes.IDENTITY3x4, model.upper_plate(z)]))

    d_xf, d_g, d_w = xf(2.0), dev_u32(groups), dev_u32(weights)
    out = torch.zeros(G * G + G, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    for buf in (d_xf, d_g, d_w, out):
        buf.record_stream(st)
    torch.cuda.synchronize()

    def frame(stream):
        t.update_transforms_device(h, d_xf, stream=stream)
        t.refit_device_async(stream=stream)
        out.zero_()
        t.placed_view_factor_groups_device(d_g.data_ptr(), G, out.data_ptr(), rays, seed, "cosine", d_w.data_ptr(), out.data_ptr() + 8 * G * G, stream=stream)

    def check(z, what):
        got = u64_of(out)
        assert np.array_equal(got[:G * G].reshape(G, G), wants[z][0]) and np.array_equal(got[G * G:], wants[z][1]), what

    with torch.cuda.stream(st):
        frame(st.cuda_stream)  # no host wait between the move, the refit and the call; eager first, as for every captured launch
    st.synchronize()
    check(2.0, "eager, behind the move to z = 2")
    assert not np.array_equal(u64_of(out)[:G * G].reshape(G, G), before[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        frame(torch.cuda.current_stream().cuda_stream)
    for z in (3.0, 1.0):
        with torch.cuda.stream(st):
            d_xf.copy_(xf(z))  # in place: the graph reads the transforms when it runs
            graph.replay()
        st.synchronize()
        check(z, f"replay at z = {z}")
    del graph
    torch.cuda.synchronize()
    t.wait_for_gpu()
    t.set_option("release_captures", 1)
    assert t.get_option("release_captures") == 0
    t.free()


# ---- 8. excluded groups, shards onto non-zero words, NULL escaped, both scratch paths ------------------------------------------------------
def test_excluded_groups_shards_and_scratch_paths(mixed):
    import torch
    t, P, G, rays, seed = mixed.t, mixed.P, 7, 96, 11
    groups = ((np.arange(P, dtype=np.uint32) // 3) % 7).astype(np.uint32)
    groups[20:30] = U32_MAX  # excluded whatever G is
    groups[200:260] = 7      # excluded because >= G
    weights = full_range_weights(P, 6)
    want = mixed.traced(rays, seed, "cosine").count(groups, G, weights)
    assert want[0].any() and want[1].any() and want[2].any()
    start = np.random.default_rng(3).integers(1, 1 << 64, G * G + G, dtype=np.uint64)  # accumulation modulo 2^64
    d_g, d_w, acc = dev_u32(groups), dev_u32(weights), dev_u64(start)
    st = torch.cuda.Stream()
    for buf in (d_g, d_w, acc):
        buf.record_stream(st)
    torch.cuda.synchronize()
    cut = int(mixed.base[3]) + 50  # inside the scaled sphere
    for placed in ((0, cut), (cut, P)):
        for shard in ((0, 31), (31, rays)):
            t.placed_view_factor_groups_device(d_g.data_ptr(), G, acc.data_ptr(), rays, seed, "cosine", d_w.data_ptr(), acc.data_ptr() + 8 * G * G, placed=placed,
                                               rays=shard, stream=st.cuda_stream)
    st.synchronize()
    t.wait_for_gpu()
    got = u64_of(acc)
    with np.errstate(over="ignore"):
        assert np.array_equal(got[:G * G], start[:G * G] + want[0].reshape(-1)) and np.array_equal(got[G * G:], start[G * G:] + want[1])
    # one shard against the model's own shard; ranges are clamped; empty ranges enqueue nothing
    part = mixed.traced(rays, seed, "cosine", (cut, P), (31, rays)).count(groups, G, weights)
    got = mixed.run(groups, G, rays, seed, "cosine", weights, placed=(cut, P + 1000), shard=(31, 1 << 20))
    assert np.array_equal(got[0], part[0]) and np.array_equal(got[1], part[1]) and part[0].any()
    for placed, shard in (((P, P + 5), None), (None, (rays, 200)), ((7, 7), None), ((9, 3), None)):
        got = mixed.run(groups, G, rays, seed, "cosine", weights, placed=placed, shard=shard, start=start)
        assert np.array_equal(got[0].reshape(-1), start[:G * G]) and np.array_equal(got[1], start[G * G:])
    # escaped = NULL leaves the matrix unchanged
    only = mixed.run(groups, G, rays, seed, "cosine", weights, escaped=False)
    assert np.array_equal(only[0], want[0]) and not only[1].any()
    # the private copies are used while they fit 256 MiB (G <= 1447 with escapes): G = 1448 adds straight onto the caller's words
    spread = ((np.arange(P, dtype=np.uint32) * 7) % 1400).astype(np.uint32)
    traced = mixed.traced(37, 21, "cosine")
    blocks = {}
    for Gs in (1400, 1448):
        wantG = traced.count(spread, Gs, weights)
        gotG = mixed.run(spread, Gs, 37, 21, "cosine", weights)
        assert np.array_equal(gotG[0], wantG[0]) and np.array_equal(gotG[1], wantG[1]) and gotG[0].any(), Gs
        onlyG = mixed.run(spread, Gs, 37, 21, "cosine", weights, escaped=False)
        assert np.array_equal(onlyG[0], wantG[0]) and not onlyG[1].any(), Gs
        blocks[Gs] = gotG[0][:1400, :1400]
    assert np.array_equal(blocks[1400], blocks[1448])  # copy path == direct path


# ---- 9. structure: a deleted handle, save / load -----------------------------------------------------------------------------------------
def test_structure_changes_rebuild_the_table(rc, oracle, tmp_path):
    cfg = model.mixed_cfg(rc)
    t = build_product(rc, cfg)
    assert t.delete(t.handles[3])  # the scaled sphere
    t.sync()
    assert t.last_sync_action == "rebuild"
    compact = dict(cfg, instances=cfg["instances"][:3] + cfg["instances"][4:])
    o = build_oracle(oracle, compact)
    base = model.bases(o)
    assert int(base[-1]) == 640 - 144 and np.array_equal(t.placed_primitive_bases(), base) and rc.placed_primitive_count(t) == 496
    P, G, rays, seed = 496, 7, 24, 5
    groups = np.repeat(np.arange(7, dtype=np.uint32), np.diff(base.astype(np.int64)))
    groups[groups == 6] = U32_MAX  # the room
    weights = full_range_weights(P, 8)
    want = model.Traced(o, rays, seed, "uniform").count(groups, G, weights)
    got = call(t, groups, G, rays, seed, "uniform", weights)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].any() and got[1].any()
    path = tmp_path / "mixed.rcscene"
    t.save(path)
    t2 = rc.TLAS.load(path)
    t2.sync()
    assert np.array_equal(t2.placed_primitive_bases(), base)
    again = call(t2, groups, G, rays, seed, "uniform", weights)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
    t2.free()
    t.free()


# ---- 10. errors and legality -------------------------------------------------------------------------------------------------------------
def test_error_codes(rc):
    import ctypes as C
    import torch
    from raycore_jl_amd._capi import lib, ptr
    L = lib()
    t = build_product(rc, model.plates_cfg(rc))
    h, P, G = t.handles[0], 16, 2
    d_g = dev_u32(np.repeat(np.arange(2, dtype=np.uint32), 8))
    out = torch.zeros(G * G + G, dtype=torch.int64, device="cuda")
    d_rays = torch.zeros(16 * 32, dtype=torch.uint8, device="cuda")
    d_tris = torch.zeros(9 * P, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    g, m, e, r, v = ptr(d_g.data_ptr()), ptr(out.data_ptr()), ptr(out.data_ptr() + 8 * G * G), ptr(d_rays.data_ptr()), ptr(d_tris.data_ptr())
    f, s, tri, bases = L.rc_placed_view_factor_groups_device, L.rc_placed_view_factor_rays_device, L.rc_placed_triangles_device, L.rc_placed_primitive_bases
    assert f(None, 16, 1, 0, 0, P, 0, 16, g, G, None, m, e, None) == RC_ERR_INVALID_ARGUMENT
    assert f(t._h, 16, 1, 0, 0, P, 0, 16, None, G, None, m, e, None) == RC_ERR_INVALID_ARGUMENT
    assert f(t._h, 16, 1, 0, 0, P, 0, 16, g, G, None, None, e, None) == RC_ERR_INVALID_ARGUMENT
    assert f(t._h, 16, 1, 2, 0, P, 0, 16, g, G, None, m, e, None) == RC_ERR_INVALID_ARGUMENT
    for bad in (0, 65536, 0xFFFFFFFF):
        assert f(t._h, 16, 1, 0, 0, P, 0, 16, g, bad, None, m, e, None) == RC_ERR_INVALID_ARGUMENT
    assert s(None, 1, 0, 0, 0, 16, r, None) == RC_ERR_INVALID_ARGUMENT
    assert s(t._h, 1, 0, 0, 0, 16, None, None) == RC_ERR_INVALID_ARGUMENT
    assert s(t._h, 1, 2, 0, 0, 16, r, None) == RC_ERR_INVALID_ARGUMENT
    assert s(t._h, 1, 1, P, 0, 16, r, None) == RC_ERR_INVALID_ARGUMENT
    assert tri(None, 0, P, v, None) == RC_ERR_INVALID_ARGUMENT and tri(t._h, 0, P, None, None) == RC_ERR_INVALID_ARGUMENT
    assert tri(t._h, 1, P, v, None) == RC_ERR_INVALID_ARGUMENT and tri(t._h, P + 1, 0, v, None) == RC_ERR_INVALID_ARGUMENT
    assert tri(t._h, 0xFFFFFFFF, 2, v, None) == RC_ERR_INVALID_ARGUMENT
    n = C.c_uint32(0)
    small = np.zeros(2, np.uint32)
    assert bases(None, None, 0, C.byref(n)) == RC_ERR_INVALID_ARGUMENT
    assert bases(t._h, ptr(small), 2, C.byref(n)) == RC_ERR_INVALID_ARGUMENT and n.value == 3 and not small.any()
    assert tri(t._h, P, 0, None, None) == 0  # nothing to write: success, nothing enqueued

    def refused(code):
        return (f(t._h, 16, 1, 0, 0, P, 0, 16, g, G, None, m, e, None) == code and s(t._h, 1, 0, 0, 0, 16, r, None) == code
                and tri(t._h, 0, P, v, None) == code and bases(t._h, None, 0, C.byref(n)) == code)

    t.update_transforms(h, np.stack([rc.scenes.IDENTITY3x4, model.upper_plate(2.0)]))
    assert refused(RC_ERR_NOT_SYNCED)  # a host-side update is pending
    t.sync()
    d_xf = f32_tensor(np.stack([rc.scenes.IDENTITY3x4, model.upper_plate(1.0)]))
    t.update_transforms_device(h, d_xf)
    assert refused(RC_ERR_NOT_SYNCED)  # a device-side update is pending before its refit
    torch.cuda.synchronize()
    assert not u64_of(out).any() and not d_rays.cpu().numpy().any() and not d_tris.cpu().numpy().any()  # nothing was enqueued
    t.refit_device_async()
    assert f(t._h, 16, 1, 0, 0, P, 0, 16, g, G, None, m, e, None) == 0
    torch.cuda.synchronize()
    t.wait_for_gpu()
    assert u64_of(out).any()
    t.push_instances(1, rc.scenes.IDENTITY3x4[None], np.full(1, 2, np.uint32))
    assert refused(RC_ERR_NOT_SYNCED)  # a host-side push is pending
    t.sync()
    assert np.array_equal(t.placed_primitive_bases(), [0, 8, 16, 24])
    with pytest.raises(ValueError, match="sampling"):
        t.placed_view_factor_groups_device(d_g.data_ptr(), G, out.data_ptr(), 16, 1, "lambert")
    with pytest.raises(ValueError, match="one value per placed primitive"):
        rc.placed_view_factor_groups(t, np.zeros(8, np.uint32), 16)
    t.free()
