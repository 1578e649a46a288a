"""rc_view_factor_products*: the view-factor matrix applied to a vector without the matrix -- mx = M x, mtx = M^T x in u64 for the
reference's M = result[src_meta, hit_meta] (src/kernels.jl:74-104) -- and the integer bounce iteration built on it.

The yardstick is always the ORACLE's matrix, computed once per (scene, rays, seed) and never written again, through the numpy model of
tests/vf_products_model.py.  Every comparison of integers is np.array_equal; there is no tolerance.  Covered: the three kernel shells;
wave sums that carry past 32 bits; waves that straddle two, three and 64 sources; source x ray shards, NULL outputs and accumulation;
metadata with gaps, duplicates, 0 and N + 50; an instanced scene; two streams at once; a captured bounce replayed; view_factor_bounces
and radiosity."""
import numpy as np
import pytest

import vf_products_model as model
from gpu_kit import dev_u32, dev_u64, finish, u64_of
from gpu_kit import rc  # noqa: F401
from scene_kit import bounce_inputs, distinct_x, full_range_x, meta, room_cfg
from worlds import VfWorld, room_world

pytestmark = pytest.mark.gpu

U32_MAX = model.U32_MAX
RC_ERR_INVALID_ARGUMENT = 1


@pytest.fixture(scope="module")
def room(rc, oracle):
    yield from room_world(VfWorld, rc, oracle)


# ---- 1. identity with the matrix, in every shell ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [3, 5, 6, -1])
def test_products_equal_the_matrix_times_x(rc, room, kernel):
    M = room.M(192, 77)
    assert (M.sum(axis=1, dtype=np.uint64) == 192).all()  # closed: every ray is counted
    room.t.set_option("kernel", kernel)
    try:
        x = full_range_x(room.n, 1)
        mx, mtx = rc.view_factor_products(room.t, x, 192, seed=77)
        w_mx, w_mtx = model.products(M, x)
        assert mx.dtype == mtx.dtype == np.uint64
        assert np.array_equal(mx, w_mx) and np.array_equal(mtx, w_mtx)
        assert room.t.last_kernel_ms() > 0
        # x = 1: the totals
        ones = np.ones(room.n, np.uint32)
        mx, mtx = rc.view_factor_products(room.t, ones, 192, seed=77)
        recv, emit = rc.view_factor_totals(room.t, 192, seed=77)
        assert np.array_equal(mx, emit) and np.array_equal(mtx, recv)
        assert np.array_equal(mx, M.sum(axis=1, dtype=np.uint64)) and np.array_equal(mtx, M.sum(axis=0, dtype=np.uint64))
        # x = 2^32 - 1: a wave's sum of one source's 64 rays carries past 32 bits
        top = np.full(room.n, U32_MAX, np.uint32)
        mx, mtx = rc.view_factor_products(room.t, top, 192, seed=77)
        assert (mx == np.uint64(192 * U32_MAX)).all()
        assert np.array_equal(mtx, M.sum(axis=0, dtype=np.uint64) * np.uint64(U32_MAX))
    finally:
        room.t.set_option("kernel", -1)


# ---- 2. waves that straddle sources -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [3, 5, 6])
@pytest.mark.parametrize("rays,seed", [(37, 21), (1, 22)])  # a wave holds two or three sources / 64 sources
def test_waves_that_straddle_sources(rc, room, kernel, rays, seed):
    M = room.M(rays, seed)
    x = distinct_x(room.n)
    room.t.set_option("kernel", kernel)
    try:
        mx, mtx = rc.view_factor_products(room.t, x, rays, seed=seed)
    finally:
        room.t.set_option("kernel", -1)
    w_mx, w_mtx = model.products(M, x)
    assert int(M.sum(dtype=np.uint64)) == rays * room.n
    assert np.array_equal(mx, w_mx) and np.array_equal(mtx, w_mtx)


# ---- 3. shards, NULLs, accumulation -------------------------------------------------------------------------------------------------------
def test_shards_nulls_and_accumulation(rc, room):
    import torch
    from raycore_jl_amd._capi import lib, ptr
    t, n = room.t, room.n
    M = room.M(96, 11)
    x = full_range_x(n, 2)
    w_mx, w_mtx = model.products(M, x)
    d_x = dev_u32(x)
    start = np.random.default_rng(3).integers(0, 1 << 64, 2 * n, dtype=np.uint64)  # accumulation onto non-zero words, modulo 2^64
    acc = dev_u64(start)
    st = torch.cuda.Stream()
    for buf in (d_x, acc):
        buf.record_stream(st)
    torch.cuda.synchronize()
    for src in ((0, n // 2), (n // 2, n)):
        for rays in ((0, 31), (31, 96)):
            t.view_factor_products_device(d_x.data_ptr(), acc.data_ptr(), acc.data_ptr() + 8 * n, 96, 11, src=src, rays=rays, stream=st.cuda_stream)
    st.synchronize()
    got = u64_of(acc)
    assert np.array_equal(got[:n], start[:n] + w_mx) and np.array_equal(got[n:], start[n:] + w_mtx)
    # one output only
    only = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    t.view_factor_products_device(d_x.data_ptr(), only.data_ptr(), None, 96, 11)
    t.view_factor_products_device(d_x.data_ptr(), None, only.data_ptr() + 8 * n, 96, 11)
    finish(room.t)
    got = u64_of(only)
    assert np.array_equal(got[:n], w_mx) and np.array_equal(got[n:], w_mtx)
    # ranges are clamped, empty ranges enqueue nothing
    before = u64_of(only).copy()
    t.view_factor_products_device(d_x.data_ptr(), only.data_ptr(), only.data_ptr() + 8 * n, 96, 11, src=(n, n + 5))
    t.view_factor_products_device(d_x.data_ptr(), only.data_ptr(), only.data_ptr() + 8 * n, 96, 11, rays=(96, 200))
    t.view_factor_products_device(d_x.data_ptr(), only.data_ptr(), only.data_ptr() + 8 * n, 96, 11, src=(7, 7))
    finish(room.t)
    assert np.array_equal(u64_of(only), before)
    t.view_factor_products_device(d_x.data_ptr(), only.data_ptr(), only.data_ptr() + 8 * n, 96, 11, src=(0, n + 1000), rays=(0, 1 << 20))
    finish(room.t)
    assert np.array_equal(u64_of(only)[:n], 2 * w_mx) and np.array_equal(u64_of(only)[n:], 2 * w_mtx)
    # the error contract
    L = lib()
    assert L.rc_view_factor_products_device(t._h, 96, 11, 0, n, 0, 96, ptr(d_x.data_ptr()), None, None, None) == RC_ERR_INVALID_ARGUMENT
    assert L.rc_view_factor_products_device(t._h, 96, 11, 0, n, 0, 96, None, ptr(only.data_ptr()), None, None) == RC_ERR_INVALID_ARGUMENT
    assert L.rc_view_factor_products_device(None, 96, 11, 0, n, 0, 96, ptr(d_x.data_ptr()), ptr(only.data_ptr()), None, None) == RC_ERR_INVALID_ARGUMENT
    assert L.rc_view_factor_products(t._h, 96, 11, None, ptr(only.data_ptr()), None) == RC_ERR_INVALID_ARGUMENT
    finish(room.t)
    assert np.array_equal(u64_of(only)[:n], 2 * w_mx)


# ---- 4. metadata with gaps, duplicates, 0 and N + 50 -----------------------------------------------------------------------------------
def test_metadata_gaps_duplicates_and_out_of_range(rc, oracle):
    w = VfWorld(rc, oracle, room_cfg(rc, meta))
    M = w.M(128, 5)
    assert M[6].sum() > 0 and not M[8:39].any() and int(M.sum(dtype=np.uint64)) < 128 * w.n  # rays from and onto metadata 0 / N + 50 are dropped
    x = full_range_x(w.n, 4)
    for k in (3, 5, 6):
        w.t.set_option("kernel", k)
        mx, mtx = rc.view_factor_products(w.t, x, 128, seed=5)
        w_mx, w_mtx = model.products(M, x)
        assert np.array_equal(mx, w_mx) and np.array_equal(mtx, w_mtx), k
    assert mx[6] > 0 and not mx[8:39].any()
    w.t.free()


# ---- 5. an instanced scene -------------------------------------------------------------------------------------------------------------------
def test_instanced_scene(rc, oracle):
    """Hits are counted by the metadata of the hit primitive whatever instance it sits in (src/kernels.jl:93-97)."""
    w = VfWorld(rc, oracle, rc.scenes.config_c3(lon=8, bands=5, lattice=(2, 2, 2)))
    M = w.M(64, 9)
    x = full_range_x(w.n, 5)
    mx, mtx = rc.view_factor_products(w.t, x, 64, seed=9)
    w_mx, w_mtx = model.products(M, x)
    assert np.array_equal(mx, w_mx) and np.array_equal(mtx, w_mtx) and M.sum() > 0
    w.t.free()


# ---- 6. two streams at once, each into its own vectors ----------------------------------------------------------------------------------
def test_two_streams_at_once(rc, room):
    import torch
    t, n = room.t, room.n
    M = room.M(96, 11)
    xa, xb = full_range_x(n, 6), distinct_x(n)
    wants = [model.products(M, xa), model.products(M, xb)]
    da, db = dev_u32(xa), dev_u32(xb)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    v1, v2 = torch.zeros(2 * n, dtype=torch.int64, device="cuda"), torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    for buf, st in ((da, s1), (v1, s1), (db, s2), (v2, s2)):
        buf.record_stream(st)
    torch.cuda.synchronize()
    for rep in range(3):
        v1.zero_(); v2.zero_()
        torch.cuda.synchronize()
        t.view_factor_products_device(da.data_ptr(), v1.data_ptr(), v1.data_ptr() + 8 * n, 96, 11, stream=s1.cuda_stream)
        t.view_factor_products_device(db.data_ptr(), v2.data_ptr(), v2.data_ptr() + 8 * n, 96, 11, stream=s2.cuda_stream)
        torch.cuda.synchronize()
        for v, (w_mx, w_mtx) in zip((v1, v2), wants):
            g = u64_of(v)
            assert np.array_equal(g[:n], w_mx) and np.array_equal(g[n:], w_mtx), rep
    finish(room.t)


# ---- 7. a captured bounce, replayed ---------------------------------------------------------------------------------------------------------


def test_captured_bounce_replayed(rc, oracle):
    """zero -> products -> the torch update (raycore_jl_amd.api.bounce_step, the step view_factor_bounces runs), captured on one stream after
    one eager step; five replays are five bounces."""
    import torch
    from raycore_jl_amd.api import bounce_step
    w = VfWorld(rc, oracle, room_cfg(rc))  # a scene of its own: the captured launches are released with it
    t, n = w.t, w.n
    R, seed = 48, 31
    M = w.M(R, seed)
    e_np, rho_np = bounce_inputs(n, 8)
    e, rho = torch.from_numpy(e_np.astype(np.int64)).cuda(), torch.from_numpy(rho_np.astype(np.int64)).cuda()
    x = e.clone()
    x32, mx = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    for buf in (e, rho, x, x32, mx):
        buf.record_stream(st)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        bounce_step(t, e, rho, x, x32, mx, R, seed, st.cuda_stream)  # eager first, as for every captured launch
    st.synchronize()
    assert np.array_equal(x.cpu().numpy().astype(np.uint32), model.bounces(M, R, e_np, rho_np, 1)), "the eager step"
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        bounce_step(t, e, rho, x, x32, mx, R, seed, torch.cuda.current_stream().cuda_stream)
    with torch.cuda.stream(st):
        x.copy_(e)
        for _ in range(5):
            g.replay()
    st.synchronize()
    want = model.bounces(M, R, e_np, rho_np, 5)
    assert np.array_equal(x.cpu().numpy().astype(np.uint32), want) and (want != e_np).any()
    del g
    torch.cuda.synchronize()
    t.wait_for_gpu()
    t.set_option("release_captures", 1)
    assert t.get_option("release_captures") == 0
    t.free()


# ---- 8. view_factor_bounces and radiosity -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 5])
def test_view_factor_bounces_equal_the_model(rc, room, k):
    import torch
    R, seed = 48, 31
    M = room.M(R, seed)
    e, rho = bounce_inputs(room.n, 9)
    e[7] = U32_MAX - 3   # saturates at the first bounce wherever anything arrives
    rho[7] = 65536
    want = model.bounces(M, R, e, rho, k)
    got = rc.view_factor_bounces(room.t, e, rho, k, rays_per_triangle=R, seed=seed)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint32 and np.array_equal(got, want)
    if k:
        assert want[7] == U32_MAX and (want < U32_MAX).any()
    # device tensors in, a device tensor out, on a side stream
    st = torch.cuda.Stream()
    d_e, d_rho = torch.from_numpy(e.astype(np.int64)).cuda(), dev_u32(rho)  # int64 values and int32 bit patterns
    for buf in (d_e, d_rho):
        buf.record_stream(st)
    torch.cuda.synchronize()
    out = rc.view_factor_bounces(room.t, d_e, d_rho, k, rays_per_triangle=R, seed=seed, stream=st)
    st.synchronize()
    assert out.dtype == torch.int64 and out.is_cuda and np.array_equal(out.cpu().numpy().astype(np.uint32), want)
    finish(room.t)


def test_radiosity(rc, room):
    R, seed, K = 48, 31, 5
    M = room.M(R, seed).astype(np.float64)
    rng = np.random.default_rng(10)
    e = rng.random(room.n) * 3.0
    e[::13] = 0.0
    # rho = 0: the emission comes back to one quantisation step of the scale (e * scale is floored to an integer; the float rounding of
    # e * scale <= 2^32 and of the division back is below 2^-20 of a step)
    got, scale = rc.radiosity(room.t, e, np.zeros(room.n), K, rays_per_triangle=R, seed=seed, return_scale=True)
    assert got.dtype == np.float64 and scale == U32_MAX / e.max()
    assert (np.abs(e - got) <= (1 + 2.0 ** -20) / scale).all()
    # rho = 0.7: K float64 steps of B <- e + rho (M B) / R on the oracle's matrix.  In units of 1 / scale the integer iterate x_k and
    # scale * B_k differ by d_k with d_0 <= 1 (the floor of e * scale) and
    #     d_{k+1} <= 1 (e) + 2 (the two floors, the inner one weighted by rho <= 1) + U * drho (rho in 16.16: (M x / R) <= U = 2^32 - 1)
    #                + rho * d_k (rows of M sum to at most R),
    # so d_k <= (3 + U * drho) / (1 - rho) for every k; the float64 reference itself is good to a few ulp of its largest value.
    rho = np.full(room.n, 0.7)
    got, scale = rc.radiosity(room.t, e, rho, K, rays_per_triangle=R, seed=seed, return_scale=True)
    B = e.copy()
    for _ in range(K):
        B = e + rho * (M @ B) / R
    drho = abs(np.rint(0.7 * 65536) / 65536 - 0.7)
    bound = (3 + U32_MAX * drho) / (1 - 0.7) / scale + 64 * np.finfo(np.float64).eps * B.max()
    err = np.abs(got - B).max()
    print(f"radiosity rho 0.7: max error {err:.3e}, bound {bound:.3e}, scale {scale:.6e}, max B {B.max():.6f}")
    assert err <= bound and bound < 1e-4 * B.max()
    assert (B > e + 0.1).any()  # the bounces matter: the bound is far below what they add
    assert np.array_equal(rc.radiosity(room.t, e, rho, K, rays_per_triangle=R, seed=seed), got)
