"""rc_placed_view_factors_sparse_device and the Python layer on top of it: the matrix of counts between PLACED primitives itself, as
canonical CSR built on the device; its products through rc_view_factor_sparse_products_device; the bounce iteration and the radiosity of an
instanced scene on the matrix.

The yardstick is the ORACLE through CPU-checked models: tests/placed_vf_model.py's Traced -> tests/placed_products_model.py's matrix ->
tests/vf_sparse_model.py's canonical CSR (the composition is pinned on the CPU in tests/test_placed_sparse_api.py).  A model trace is
computed once per (scene, rays, seed, sampling) and only read.  Every comparison is np.array_equal on integers; there is no tolerance."""
import numpy as np
import pytest

import placed_products_model as pm
import placed_vf_model as model
import vf_sparse_model as sparse
from gpu_kit import dev_u32, f32_tensor, finish, u32_of, u64_of
from gpu_kit import rc  # noqa: F401
from helpers import build_oracle, build_product
from scene_kit import bounce_inputs, full_range_x
from worlds import VfWorld, room_world

pytestmark = pytest.mark.gpu

U32_MAX = model.U32_MAX
RC_ERR_INVALID_ARGUMENT, RC_ERR_NOT_SYNCED = 1, 6
GUARD = 0x5A5A5A5A
HEAD_FILL = 0x7B7B7B7B7B7B7B7B
SAMPLINGS = ("uniform", "cosine")


class World:
    """One scene in the product and in the oracle; the model's traces and matrices are computed once per job and only read."""

    def __init__(self, rc, oracle, cfg):
        self.rc, self.cfg = rc, cfg
        self.t, self.o = build_product(rc, cfg), build_oracle(oracle, cfg)
        self.base = model.bases(self.o)
        self.P = int(self.base[-1])
        self._traced, self._m = {}, {}

    def traced(self, rays, seed, sampling):
        key = (rays, seed, sampling)
        if key not in self._traced:
            self._traced[key] = model.Traced(self.o, rays, seed, sampling)
        return self._traced[key]

    def Mp(self, rays, seed, sampling):
        """The model's P x P matrix, read-only."""
        key = (rays, seed, sampling)
        if key not in self._m:
            m, _ = pm.matrix(self.traced(rays, seed, sampling))
            assert m.shape == (self.P, self.P)
            m.setflags(write=False)
            self._m[key] = m
        return self._m[key]

    def device_matrix(self, rays, seed, sampling):
        """Mp (P, P) from rc_placed_view_factor_groups_device with every placed primitive its own group."""
        import torch
        P = self.P
        d_g = dev_u32(np.arange(P, dtype=np.uint32))
        out = torch.zeros(P * P, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        self.t.placed_view_factor_groups_device(d_g.data_ptr(), P, out.data_ptr(), rays, seed, sampling)
        finish(self.t)
        return u64_of(out).reshape(P, P).copy()


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


@pytest.fixture(scope="module")
def plates(rc, oracle):
    w = World(rc, oracle, model.plates_cfg(rc))
    assert w.P == 16
    yield w
    w.t.free()


@pytest.fixture(scope="module")
def room(rc, oracle):
    yield from room_world(VfWorld, rc, oracle)


class DeviceCsr:
    """Device arrays for one rc_placed_view_factors_sparse_device call: row_ptr[rows + 1], nnz, and cols / vals of `capacity` words
    followed by `guard` words -- everything pre-filled with a pattern the call has to overwrite (or, behind the capacity, leave alone)."""

    def __init__(self, rows, capacity, guard=8):
        import torch
        self.rows, self.capacity, self.guard = rows, capacity, guard
        self.head = torch.full((rows + 2,), HEAD_FILL, dtype=torch.int64, device="cuda")
        self.cols = torch.full((capacity + guard,), GUARD, dtype=torch.int32, device="cuda")
        self.vals = torch.full((capacity + guard,), GUARD, dtype=torch.int32, device="cuda")

    def buffers(self):
        return self.head, self.cols, self.vals

    def pointers(self, null_arrays=False):
        """(row_ptr, cols, vals, capacity, nnz) as the raw call takes them."""
        return (self.head.data_ptr(), None if null_arrays else self.cols.data_ptr(), None if null_arrays else self.vals.data_ptr(), self.capacity,
                self.head.data_ptr() + 8 * (self.rows + 1))

    def build(self, t, rays, seed, sampling, rows=None, stream=None, null_arrays=False):
        t.placed_view_factors_sparse_device(*self.pointers(null_arrays), rays, seed, sampling, rows, stream)

    def read(self):
        head = u64_of(self.head)
        return head[:self.rows + 1].copy(), int(head[self.rows + 1]), u32_of(self.cols), u32_of(self.vals)

    def untouched(self):
        return (u64_of(self.head) == np.uint64(HEAD_FILL)).all() and (u32_of(self.cols) == GUARD).all() and (u32_of(self.vals) == GUARD).all()


def assert_is_the_matrix(csr, M, what=""):
    row_ptr, cols, vals = csr
    n = M.shape[1]
    assert row_ptr.dtype == np.uint64 and cols.dtype == np.uint32 and vals.dtype == np.uint32, what
    assert sparse.is_canonical(csr, n), what
    nnz = np.count_nonzero(M)
    assert int(row_ptr[-1]) == nnz == len(cols) == len(vals), what
    assert np.array_equal(sparse.densify(csr, n), M), what
    for got, w in zip(csr, sparse.csr_from_dense(M)):  # canonical: the arrays themselves are determined
        assert np.array_equal(got, w), what


def no_diagonal(csr, row_offset=0):
    row_ptr, cols, _ = csr
    r = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr.astype(np.int64))) + row_offset
    return not (cols.astype(np.int64) == r).any()


# ---- 1. the three arrays equal the canonical CSR of the model's matrix, in every shell ---------------------------------------------------
@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("kernel", [3, 5, 6, -1])
def test_matches_the_model_in_every_shell(rc, mixed, kernel, sampling):
    P = mixed.P
    mixed.t.set_option("kernel", kernel)
    try:
        for rays, seed in ((192, 77), (37, 21), (1, 22)):  # a wave holds one source / two or three / 64 across instance boundaries
            Mp = mixed.Mp(rays, seed, sampling)
            assert Mp.any() and int(Mp.sum(dtype=np.uint64)) < rays * P  # the room is open: some rays escape
            csr = rc.placed_view_factors_sparse(mixed.t, rays, seed=seed, sampling=sampling)
            what = (kernel, sampling, rays)
            assert isinstance(csr, rc.SparseViewFactors) and csr.placed is True and csr.n == P and csr.n_rows == P and csr.row_offset == 0, what
            assert csr.nnz == np.count_nonzero(Mp) and csr.sampling == SAMPLINGS.index(sampling) and (csr.rays_per_triangle, csr.seed) == (rays, seed), what
            assert_is_the_matrix(tuple(csr), Mp, what)
            assert no_diagonal(tuple(csr)), what
            if rays == 1:
                assert (csr[2] == 1).all() and (np.diff(csr[0].astype(np.int64)) <= 1).all()
        assert mixed.t.last_kernel_ms() > 0
    finally:
        mixed.t.set_option("kernel", -1)


# ---- 2. device against device -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["mixed", "lattice"])
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_device_against_device(rc, request, scene, sampling):
    w = request.getfixturevalue(scene)
    P, rays, seed = w.P, 37, 21
    csr = rc.placed_view_factors_sparse(w.t, rays, seed=seed, sampling=sampling)
    Mp = w.device_matrix(rays, seed, sampling)
    assert Mp.any() and not np.diag(Mp).any() and int(Mp.max()) <= rays
    assert np.array_equal(sparse.densify(tuple(csr), P).astype(np.uint64), Mp) and sparse.is_canonical(tuple(csr), P)
    for x in (full_range_x(P, 3), np.full(P, U32_MAX, np.uint32)):
        mx, mtx = rc.view_factor_sparse_products(csr, x)
        r_mx, r_mtx = rc.placed_view_factor_products(w.t, x, rays, seed=seed, sampling=sampling)  # the retraced products: the same words
        assert mx.dtype == mtx.dtype == np.uint64 and len(mx) == len(mtx) == P
        assert np.array_equal(mx, r_mx) and np.array_equal(mtx, r_mtx), (scene, sampling, int(x[5]))
        assert mx.any() and mtx.any()
    assert (rc.view_factor_sparse_products(csr, np.full(P, U32_MAX, np.uint32))[0] > U32_MAX).any()  # the sums carry past 32 bits
    received, emitted, _ = rc.placed_view_factor_totals(w.t, rays, seed=seed, sampling=sampling)
    mx, mtx = rc.view_factor_sparse_products(csr, np.ones(P, np.uint32))
    assert np.array_equal(mx, emitted) and np.array_equal(mtx, received)


# ---- 3. long runs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_long_runs(rc, oracle, plates, sampling):
    """Sixteen triangles, 4096 rays each.  On the plates one unit apart single entries count more rays than a wave holds (the model's
    largest entry is 89 uniform, 169 cosine); with the upper plate lowered to z = 0.1 thirty-two entries count more than 1024 -- runs
    longer than a block of the sort or of the encoding, the bound of the per-triangle family's test.  Both are asserted on the model first."""
    R, seed = 4096, 13
    Mp = plates.Mp(R, seed, sampling)
    assert int(Mp.max()) > 64 and np.count_nonzero(Mp) <= 16 * 8
    csr = rc.placed_view_factors_sparse(plates.t, R, seed=seed, sampling=sampling)
    assert_is_the_matrix(tuple(csr), Mp, (sampling, 1.0))
    near = World(rc, oracle, model.plates_cfg(rc, 0.1))
    try:
        Mp = near.Mp(R, seed, sampling)
        assert int((Mp > 1024).sum()) >= 16 and np.count_nonzero(Mp) <= 16 * 8
        csr = rc.placed_view_factors_sparse(near.t, R, seed=seed, sampling=sampling)
        assert_is_the_matrix(tuple(csr), Mp, (sampling, 0.1))
        assert int(csr[2].max()) > 1024
    finally:
        near.t.free()


# ---- 4. chunking changes nothing ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_chunking_changes_nothing(rc, mixed, sampling):
    t, P, R, seed = mixed.t, mixed.P, 128, 5
    default = t.get_option("vf_sparse_scratch_bytes")
    assert default == 256 << 20
    whole = rc.placed_view_factors_sparse(t, R, seed=seed, sampling=sampling)  # one chunk
    assert_is_the_matrix(tuple(whole), mixed.Mp(R, seed, sampling), sampling)
    try:
        # one row per chunk (a row's R rays exceed the option: a chunk of its own); 50 rows; 61 rows and a remainder; two chunks, one short of all rows
        for cap in (8, 8 * R * 50, 8 * R * 61 + 3, 8 * R * P - 1):
            t.set_option("vf_sparse_scratch_bytes", cap)
            assert t.get_option("vf_sparse_scratch_bytes") == cap
            got = rc.placed_view_factors_sparse(t, R, seed=seed, sampling=sampling)
            assert got.nnz == whole.nnz
            for a, b in zip(got, whole):
                assert np.array_equal(a, b), cap
    finally:
        t.set_option("vf_sparse_scratch_bytes", default)


# ---- 5. row blocks ---------------------------------------------------------------------------------------------------------------------------
def test_row_blocks_concatenate(rc, mixed):
    t, P, R, seed, sampling = mixed.t, mixed.P, 128, 5, "cosine"
    Mp = mixed.Mp(R, seed, sampling)
    whole = rc.placed_view_factors_sparse(t, R, seed=seed, sampling=sampling)
    c1, c2 = int(mixed.base[2]) + 3, int(mixed.base[3]) + 50  # inside the mirrored square, inside the scaled sphere
    x = full_range_x(P, 2)
    want = pm.products(mixed.traced(R, seed, sampling), x)
    d_x = dev_u32(x)
    import torch
    both = torch.zeros(2 * P, dtype=torch.int64, device="cuda")
    parts = []
    for r0, r1 in ((0, c1), (c1, c1), (c1, c2), (c2, P + 1000)):  # three ragged blocks and an empty one; the end is clamped past P
        b = rc.placed_view_factors_sparse(t, R, seed=seed, sampling=sampling, rows=(r0, r1))
        r1 = min(r1, P)
        assert b.placed and b.row_offset == r0 and b.n_rows == r1 - r0 and int(b[0][0]) == 0 and b.n == P
        assert_is_the_matrix(tuple(b), Mp[r0:r1], (r0, r1))
        assert no_diagonal(tuple(b), r0)
        parts.append(b)
        bp, bc, bv = b.device_arrays()
        t.view_factor_sparse_products_device(r1 - r0, bp.data_ptr(), bc.data_ptr() if b.nnz else None, bv.data_ptr() if b.nnz else None, d_x.data_ptr(),
                                             both.data_ptr(), both.data_ptr() + 8 * P, row_offset=r0)
        finish(t)
        if r1 > r0:
            one = rc.view_factor_sparse_products(b, x)
            s_mx, s_mtx = sparse.spmv(tuple(b), x, row_offset=r0)
            assert np.array_equal(one[0], s_mx) and np.array_equal(one[1], s_mtx) and not one[0][:r0].any() and not one[0][r1:].any()
    assert np.array_equal(np.concatenate([p[1] for p in parts]), whole[1]) and np.array_equal(np.concatenate([p[2] for p in parts]), whole[2])
    ptr, base = [np.zeros(1, np.uint64)], 0
    for p in parts:
        ptr.append(p[0][1:] + np.uint64(base))
        base += int(p[0][-1])
    assert np.array_equal(np.concatenate(ptr), whole[0])
    got = u64_of(both)  # the blocks' products with their offsets accumulate to the whole products
    assert np.array_equal(got[:P], want[0]) and np.array_equal(got[P:], want[1])
    # a block wholly past P is empty
    b = rc.placed_view_factors_sparse(t, R, seed=seed, sampling=sampling, rows=(P + 5, P + 9))
    assert b.n_rows == 0 and b.nnz == 0 and np.array_equal(b[0], np.zeros(1, np.uint64)) and b.row_offset == P
    with pytest.raises(ValueError, match="all rows"):
        rc.placed_view_factor_bounces(parts[0], np.zeros(P, np.uint32), np.zeros(P, np.uint32), 1)


# ---- 6. capacity ------------------------------------------------------------------------------------------------------------------------------
def test_capacity_contract(rc, mixed):
    t, P, R, seed, sampling = mixed.t, mixed.P, 128, 5, "uniform"
    want_ptr, want_cols, want_vals = sparse.csr_from_dense(mixed.Mp(R, seed, sampling))
    nnz = len(want_cols)
    assert nnz > 100
    # the counting call: NULL arrays
    d = DeviceCsr(P, 0)
    d.build(t, R, seed, sampling, null_arrays=True)
    finish(t)
    row_ptr, got_nnz, cols, vals = d.read()
    assert got_nnz == nnz and np.array_equal(row_ptr, want_ptr)
    assert (cols == GUARD).all() and (vals == GUARD).all()
    # too small by five, exact, larger than needed, one
    for capacity in (nnz - 5, nnz, nnz + 3, 1):
        d = DeviceCsr(P, capacity)
        d.build(t, R, seed, sampling)
        finish(t)
        row_ptr, got_nnz, cols, vals = d.read()
        k = min(capacity, nnz)
        assert got_nnz == nnz and np.array_equal(row_ptr, want_ptr), capacity
        assert np.array_equal(cols[:k], want_cols[:k]) and np.array_equal(vals[:k], want_vals[:k]), capacity
        assert (cols[k:] == GUARD).all() and (vals[k:] == GUARD).all(), capacity  # nothing at or beyond the capacity, nothing beyond nnz
    # the python wrapper with a capacity reports the true count; the products refuse a truncated matrix
    short = rc.placed_view_factors_sparse(t, R, seed=seed, sampling=sampling, capacity=nnz - 5)
    assert short.nnz == nnz and len(short[1]) == nnz - 5 and np.array_equal(short[1], want_cols[:nnz - 5]) and np.array_equal(short[0], want_ptr)
    with pytest.raises(ValueError, match="truncated"):
        rc.view_factor_sparse_products(short, np.ones(P, np.uint32))
    with pytest.raises(ValueError, match="truncated"):
        rc.placed_view_factor_bounces(short, np.zeros(P, np.uint32), np.zeros(P, np.uint32), 1)
    roomy = rc.placed_view_factors_sparse(t, R, seed=seed, sampling=sampling, capacity=nnz + 3)
    assert roomy.nnz == nnz and np.array_equal(roomy[1], want_cols) and np.array_equal(roomy[2], want_vals)


# ---- 7. one identity instance: the per-triangle family's matrix ----------------------------------------------------------------------------
def test_identity_instance_gives_the_siblings_matrix(rc, room):
    t, n, rays, seed = room.t, room.n, 64, 9
    assert np.array_equal(t.placed_primitive_bases(), [0, n])
    meta = t.adapt().all_blas_prims["meta"].astype(np.int64)
    assert np.array_equal(np.sort(meta), np.arange(1, n + 1))  # no two primitives share metadata
    sibling = rc.view_factors_sparse(t, rays, seed=seed)
    M = sparse.densify(tuple(sibling), n)  # [source metadata - 1, hit metadata - 1]
    placed = rc.placed_view_factors_sparse(t, rays, seed=seed, sampling="uniform")
    Mp = sparse.densify(tuple(placed), n)  # placed primitive q of the one instance is flat primitive q
    assert M.any() and np.array_equal(Mp, M[np.ix_(meta - 1, meta - 1)])
    assert np.array_equal(M, room.M(rays, seed))
    finish(t)


# ---- 8. the build follows a device-side move, and a built matrix is a snapshot ---------------------------------------------------------------
def test_follows_a_device_side_move(rc, oracle):
    import torch
    t = build_product(rc, model.plates_cfg(rc))
    h, P, rays, seed = t.handles[0], 16, 512, 31
    wants = {z: sparse.csr_from_dense(pm.matrix(model.Traced(build_oracle(oracle, model.plates_cfg(rc, z)), rays, seed, "cosine"))[0]) for z in (1.0, 2.0, 3.0)}
    assert not np.array_equal(wants[2.0][2], wants[3.0][2]) and not np.array_equal(wants[1.0][2], wants[2.0][2])
    before = rc.placed_view_factors_sparse(t, rays, seed=seed, sampling="cosine")
    for got, want in zip(before, wants[1.0]):
        assert np.array_equal(got, want), "before the move"

    def xf(z):
        return f32_tensor(np.stack([rc.scenes.IDENTITY3x4, model.upper_plate(z)]))

    d_xf = {z: xf(z) for z in (2.0, 3.0)}
    built = {z: DeviceCsr(P, P * (P - 1)) for z in (2.0, 3.0)}
    st = torch.cuda.Stream()
    for buf in list(d_xf.values()) + [b for d in built.values() for b in d.buffers()]:
        buf.record_stream(st)
    torch.cuda.synchronize()
    for z in (2.0, 3.0):  # no host wait between the move, the refit and the build, nor between the two frames
        t.update_transforms_device(h, d_xf[z], stream=st.cuda_stream)
        t.refit_device_async(stream=st.cuda_stream)
        built[z].build(t, rays, seed, "cosine", stream=st.cuda_stream)
    st.synchronize()
    t.wait_for_gpu()
    for z in (2.0, 3.0):
        row_ptr, nnz, cols, vals = built[z].read()
        want = wants[z]
        assert nnz == len(want[1]) and np.array_equal(row_ptr, want[0]) and np.array_equal(cols[:nnz], want[1]) and np.array_equal(vals[:nnz], want[2]), z
        assert (cols[nnz:] == GUARD).all() and (vals[nnz:] == GUARD).all(), z
    # a snapshot: the matrix built before the move still holds the old placement, on the host and on the device
    for got, want in zip(before, wants[1.0]):
        assert np.array_equal(got, want)
    for got, want, view in zip(before.device_arrays(), wants[1.0], (np.uint64, np.uint32, np.uint32)):
        assert np.array_equal(got.cpu().numpy().view(view), want)
    # and a fresh build sees the scene where the last move left it
    after = rc.placed_view_factors_sparse(t, rays, seed=seed, sampling="cosine")
    for got, want in zip(after, wants[3.0]):
        assert np.array_equal(got, want), "after the moves"
    t.free()


# ---- 9. two streams at once, each into its own arrays -------------------------------------------------------------------------------------
def test_two_streams_at_once(rc, mixed):
    import torch
    t, P = mixed.t, mixed.P
    jobs = [(128, 5, "cosine"), (192, 77, "uniform")]
    wants = [sparse.csr_from_dense(mixed.Mp(*job)) for job in jobs]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for rep in range(3):
        ds = [DeviceCsr(P, len(w[1])) for w in wants]
        for d, st in zip(ds, (s1, s2)):
            for buf in d.buffers():
                buf.record_stream(st)
        torch.cuda.synchronize()
        for d, st, (R, seed, sampling) in zip(ds, (s1, s2), jobs):
            d.build(t, R, seed, sampling, stream=st.cuda_stream)
        torch.cuda.synchronize()
        for d, w in zip(ds, wants):
            row_ptr, nnz, cols, vals = d.read()
            assert nnz == len(w[1]) and np.array_equal(row_ptr, w[0]), rep
            assert np.array_equal(cols[:nnz], w[1]) and np.array_equal(vals[:nnz], w[2]), rep
    finish(t)


# ---- 10. errors and legality ---------------------------------------------------------------------------------------------------------------
def test_error_codes(rc):
    import torch
    from raycore_jl_amd._capi import lib, ptr
    f = lib().rc_placed_view_factors_sparse_device
    t = build_product(rc, model.plates_cfg(rc))
    h, P = t.handles[0], 16
    d = DeviceCsr(P, 240)
    torch.cuda.synchronize()
    row_ptr, cols, vals, nnz = ptr(d.head.data_ptr()), ptr(d.cols.data_ptr()), ptr(d.vals.data_ptr()), ptr(d.head.data_ptr() + 8 * (P + 1))
    assert f(None, 16, 1, 0, 0, P, row_ptr, cols, vals, 240, nnz, None) == RC_ERR_INVALID_ARGUMENT
    assert f(t._h, 16, 1, 0, 0, P, None, cols, vals, 240, nnz, None) == RC_ERR_INVALID_ARGUMENT
    assert f(t._h, 16, 1, 0, 0, P, row_ptr, cols, vals, 64, None, None) == RC_ERR_INVALID_ARGUMENT
    assert f(t._h, 16, 1, 0, 0, P, row_ptr, None, vals, 240, nnz, None) == RC_ERR_INVALID_ARGUMENT
    assert f(t._h, 16, 1, 0, 0, P, row_ptr, cols, None, 240, nnz, None) == RC_ERR_INVALID_ARGUMENT
    assert f(t._h, 16, 1, 0, 0, P, row_ptr, None, None, 1, nnz, None) == RC_ERR_INVALID_ARGUMENT
    for bad in (2, 3, 0xFFFFFFFF):
        assert f(t._h, 16, 1, bad, 0, P, row_ptr, cols, vals, 240, nnz, None) == RC_ERR_INVALID_ARGUMENT
    t.update_transforms(h, np.stack([rc.scenes.IDENTITY3x4, model.upper_plate(2.0)]))
    assert f(t._h, 16, 1, 1, 0, P, row_ptr, cols, vals, 240, nnz, None) == RC_ERR_NOT_SYNCED  # a host-side update is pending
    t.sync()
    d_xf = f32_tensor(np.stack([rc.scenes.IDENTITY3x4, model.upper_plate(1.0)]))
    t.update_transforms_device(h, d_xf)
    assert f(t._h, 16, 1, 1, 0, P, row_ptr, cols, vals, 240, nnz, None) == RC_ERR_NOT_SYNCED  # a device-side update is pending before its refit
    torch.cuda.synchronize()
    assert d.untouched()  # nothing was enqueued by any refused call
    t.refit_device_async()
    assert f(t._h, 16, 1, 1, 0, P, row_ptr, cols, vals, 240, nnz, None) == 0
    finish(t)
    got_ptr, got_nnz, got_cols, _ = d.read()
    assert 0 < got_nnz <= 240 and int(got_ptr[0]) == 0 and int(got_ptr[-1]) == got_nnz and (got_cols[:got_nnz] < P).all() and (got_cols[got_nnz:] == GUARD).all()
    # an empty range and rays_per_triangle = 0 are empty matrices, not errors
    for args in ((16, 1, 1, P, P), (16, 1, 1, 9, 3), (0, 1, 1, 0, P)):
        e = DeviceCsr(P, 8)
        assert f(t._h, *args, ptr(e.head.data_ptr()), ptr(e.cols.data_ptr()), ptr(e.vals.data_ptr()), 8, ptr(e.head.data_ptr() + 8 * (P + 1)), None) == 0
        finish(t)
        rows = max(min(args[4], P) - args[3], 0)
        head = u64_of(e.head)
        assert not head[:rows + 1].any() and int(head[P + 1]) == 0 and (u32_of(e.cols) == GUARD).all(), args
    d = DeviceCsr(P, 240)
    row_ptr, cols, vals, nnz = ptr(d.head.data_ptr()), ptr(d.cols.data_ptr()), ptr(d.vals.data_ptr()), ptr(d.head.data_ptr() + 8 * (P + 1))
    t.push_instances(1, rc.scenes.IDENTITY3x4[None], np.full(1, 2, np.uint32))
    assert f(t._h, 16, 1, 1, 0, P, row_ptr, cols, vals, 240, nnz, None) == RC_ERR_NOT_SYNCED  # a host-side push is pending
    t.sync()
    # a capturing stream: the build sorts and sizes its scratch on the host
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        status = f(t._h, 16, 1, 1, 0, P, row_ptr, cols, vals, 240, nnz, ptr(torch.cuda.current_stream().cuda_stream))
        d.head.add_(0)  # (a graph must hold something)
    assert status == RC_ERR_NOT_SYNCED
    del g
    torch.cuda.synchronize()
    assert d.untouched()
    with pytest.raises(ValueError, match="sampling"):
        t.placed_view_factors_sparse_device(*d.pointers(), 16, 1, "lambert")
    assert rc.placed_view_factors_sparse(t, 16, seed=1, sampling="cosine").n == 24  # P is 24 now
    t.free()


# ---- 11. bounces and radiosity on the matrix -----------------------------------------------------------------------------------------------
def bounce_case(w, R, seed, sampling, salt):
    e, rho = bounce_inputs(w.P, salt)
    e[7] = U32_MAX - 3  # saturates at the first bounce wherever anything arrives
    rho[7] = 65536
    return e, rho, w.Mp(R, seed, sampling)


@pytest.mark.parametrize("k", [0, 1, 5])
@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("scene,R", [("plates", 96), ("mixed", 37)])
def test_bounces_on_the_matrix_equal_the_model_and_the_retraced_ones(rc, request, scene, R, sampling, k):
    import torch
    w = request.getfixturevalue(scene)
    seed = 31
    e, rho, Mp = bounce_case(w, R, seed, sampling, 9)
    want = pm.bounces(Mp, R, e, rho, k)
    assert Mp[7].any() and (k == 0 or (want[7] == U32_MAX and (want != e).any()))
    csr = rc.placed_view_factors_sparse(w.t, R, seed=seed, sampling=sampling)
    got = rc.placed_view_factor_bounces(csr, e, rho, k)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint32 and np.array_equal(got, want)
    assert np.array_equal(got, rc.placed_view_factor_bounces(w.t, e, rho, k, rays_per_triangle=R, seed=seed, sampling=sampling))
    # device tensors in, a device tensor out, on a side stream
    st = torch.cuda.Stream()
    d_e, d_rho = torch.from_numpy(e.astype(np.int64)).cuda(), dev_u32(rho)
    for buf in (d_e, d_rho):
        buf.record_stream(st)
    torch.cuda.synchronize()
    out = rc.placed_view_factor_bounces(csr, d_e, d_rho, k, stream=st)
    st.synchronize()
    assert out.dtype == torch.int64 and out.is_cuda and np.array_equal(out.cpu().numpy().astype(np.uint32), want)
    with pytest.raises(ValueError, match="one value per placed primitive"):
        rc.placed_view_factor_bounces(csr, e[:-1], rho[:-1], k)
    finish(w.t)


def test_captured_sparse_bounce_replayed(rc, mixed):
    """zero -> sparse products -> the torch update (raycore_jl_amd.api.bounce_step_sparse) on the PLACED matrix, captured with no eager
    step before it: the product reads nothing on the host.  Five replays are five bounces."""
    import torch
    from raycore_jl_amd.api import bounce_step_sparse
    R, seed, P = 37, 31, mixed.P
    e_np, rho_np, Mp = bounce_case(mixed, R, seed, "cosine", 8)
    csr = rc.placed_view_factors_sparse(mixed.t, R, seed=seed, sampling="cosine")
    csr.device_arrays()
    e, rho = torch.from_numpy(e_np.astype(np.int64)).cuda(), torch.from_numpy(rho_np.astype(np.int64)).cuda()
    x = e.clone()
    x32, mx = torch.empty(P, dtype=torch.int32, device="cuda"), torch.empty(P, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    for buf in (e, rho, x, x32, mx):
        buf.record_stream(st)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        bounce_step_sparse(csr, e, rho, x, x32, mx, torch.cuda.current_stream().cuda_stream)
    with torch.cuda.stream(st):
        x.copy_(e)
        for _ in range(5):
            g.replay()
    st.synchronize()
    want = pm.bounces(Mp, R, e_np, rho_np, 5)
    assert np.array_equal(x.cpu().numpy().astype(np.uint32), want) and (want != e_np).any()
    del g
    finish(mixed.t)


@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_placed_radiosity_on_the_matrix(rc, mixed, sampling):
    R, seed, K, P = 37, 31, 5, mixed.P
    csr = rc.placed_view_factors_sparse(mixed.t, R, seed=seed, sampling=sampling)
    rng = np.random.default_rng(10)
    e = rng.random(P) * 3.0
    e[::13] = 0.0
    rho = np.full(P, 0.7)
    want, w_scale = rc.placed_radiosity(mixed.t, e, rho, K, rays_per_triangle=R, seed=seed, sampling=sampling, return_scale=True)
    got, scale = rc.placed_radiosity(mixed.t, e, rho, K, return_scale=True, matrix=csr)
    assert scale == w_scale and got.dtype == np.float64 and np.array_equal(got, want)
    assert (got > e + 0.1).any()  # the bounces matter
    scale_q, e_q, rho_q = rc.radiosity_scale(e, rho)
    assert scale_q == scale and np.array_equal(got, pm.bounces(mixed.Mp(R, seed, sampling), R, e_q, rho_q, K).astype(np.float64) / scale)
    finish(mixed.t)
