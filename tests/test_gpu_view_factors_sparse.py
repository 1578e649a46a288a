"""rc_view_factors_sparse*: the view-factor matrix of the reference (src/kernels.jl:74-104) itself, as canonical CSR built on the device,
and rc_view_factor_sparse_products_device, its products with a vector.

The yardstick is always the ORACLE's dense matrix, computed once per (scene, rays, seed) and never written again, through the numpy
models of tests/vf_sparse_model.py and tests/vf_products_model.py.  Every comparison is np.array_equal on integers; there is no tolerance.
Covered: the three kernel shells; waves that straddle sources; runs far longer than a wave or a sort block; chunking (one row per chunk,
ragged chunks, a shared row larger than the scratch, empty rows); row blocks; the capacity contract with guard words; an instanced scene;
two streams at once; the products on traced and on handmade matrices (empty, one entry, rows of 0 .. 4100 entries, a hot column, words
that wrap past 2^64); the bounce iteration and radiosity on the matrix, eager and captured."""
import numpy as np
import pytest

import vf_products_model as dense
import vf_sparse_model as model
from gpu_kit import dev_u32, dev_u64, finish, u32_of, u64_of
from gpu_kit import rc  # noqa: F401
from scene_kit import bounce_inputs, full_range_x, meta, room_cfg
from worlds import VfWorld, room_world

pytestmark = pytest.mark.gpu

U32_MAX = model.U32_MAX
RC_ERR_INVALID_ARGUMENT, RC_ERR_NOT_SYNCED = 1, 6
GUARD = 0x5A5A5A5A


class World(VfWorld):
    """One scene in the product and in the oracle.  The oracle's matrices and the product's default build of each are computed once per
    (rays, seed) and are read-only."""

    def __init__(self, rc, oracle, cfg):
        super().__init__(rc, oracle, cfg)
        self._csr = {}

    def csr(self, rays, seed):
        if (rays, seed) not in self._csr:
            c = self.rc.view_factors_sparse(self.t, rays, seed=seed)
            for a in c:
                a.setflags(write=False)
            self._csr[rays, seed] = c
        return self._csr[rays, seed]


@pytest.fixture(scope="module")
def room(rc, oracle):
    yield from room_world(World, rc, oracle)


@pytest.fixture(scope="module")
def gaps(rc, oracle):
    w = World(rc, oracle, room_cfg(rc, meta))
    yield w
    w.t.free()


@pytest.fixture(scope="module")
def lattice(rc, oracle):
    w = World(rc, oracle, rc.scenes.config_c3(lon=8, bands=5, lattice=(2, 2, 2)))
    yield w
    w.t.free()


class DeviceCsr:
    """Device arrays for one rc_view_factors_sparse_device call: row_ptr[rows + 1], nnz, and cols / vals of `capacity` words followed
    by `guard` words -- everything pre-filled with a pattern the call has to overwrite (or, behind the capacity, leave alone)."""

    def __init__(self, rows, capacity, guard=8):
        import torch
        self.rows, self.capacity, self.guard = rows, capacity, guard
        self.head = torch.full((rows + 2,), 0x7B7B7B7B7B7B7B7B, dtype=torch.int64, device="cuda")
        self.cols = torch.full((capacity + guard,), GUARD, dtype=torch.int32, device="cuda")
        self.vals = torch.full((capacity + guard,), GUARD, dtype=torch.int32, device="cuda")

    def build(self, t, rays, seed, rows=None, stream=None, null_arrays=False):
        t.view_factors_sparse_device(self.head.data_ptr(), None if null_arrays else self.cols.data_ptr(), None if null_arrays else self.vals.data_ptr(),
                                     self.capacity, self.head.data_ptr() + 8 * (self.rows + 1), rays, seed, rows, stream)

    def read(self):
        head = u64_of(self.head)
        return head[:self.rows + 1].copy(), int(head[self.rows + 1]), u32_of(self.cols), u32_of(self.vals)


def assert_is_the_matrix(csr, M, what=""):
    row_ptr, cols, vals = csr
    n = M.shape[1]
    assert row_ptr.dtype == np.uint64 and cols.dtype == np.uint32 and vals.dtype == np.uint32, what
    assert model.is_canonical(csr, n), what
    nnz = np.count_nonzero(M)
    assert int(row_ptr[-1]) == nnz == len(cols) == len(vals), what
    assert np.array_equal(model.densify(csr, n), M), what
    want = model.csr_from_dense(M)
    for got, w in zip(csr, want):  # canonical: the arrays themselves are determined
        assert np.array_equal(got, w), what


# ---- 1. identity with the dense matrix, in every shell ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [3, 5, 6, -1])
def test_sparse_equals_the_dense_matrix(rc, room, kernel):
    M = room.M(192, 77)
    assert (M.sum(axis=1, dtype=np.uint64) == 192).all()  # closed: every ray is counted
    room.t.set_option("kernel", kernel)
    try:
        csr = rc.view_factors_sparse(room.t, 192, seed=77)
    finally:
        room.t.set_option("kernel", -1)
    assert isinstance(csr, rc.SparseViewFactors) and csr.nnz == np.count_nonzero(M) and csr.n == room.n and csr.row_offset == 0
    assert_is_the_matrix(tuple(csr), M, kernel)
    assert np.array_equal(rc.view_factors(room.t, 192, seed=77), M)
    row_ptr, cols, vals = csr  # unpacks as the triple
    assert int(row_ptr[-1]) == len(cols)


# ---- 2. waves that straddle sources -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [3, 5, 6])
@pytest.mark.parametrize("rays,seed", [(37, 21), (1, 22)])  # a wave holds two or three sources / 64 sources
def test_waves_that_straddle_sources(rc, room, kernel, rays, seed):
    M = room.M(rays, seed)
    assert int(M.sum(dtype=np.uint64)) == rays * room.n
    room.t.set_option("kernel", kernel)
    try:
        csr = rc.view_factors_sparse(room.t, rays, seed=seed)
    finally:
        room.t.set_option("kernel", -1)
    assert_is_the_matrix(tuple(csr), M)
    if rays == 1:
        assert (csr[2] == 1).all() and len(csr[2]) == room.n and np.array_equal(csr[0], np.arange(room.n + 1, dtype=np.uint64))


# ---- 3. long runs ---------------------------------------------------------------------------------------------------------------------------
def test_long_runs(rc, oracle):
    """Twelve triangles, 4096 rays each: single entries count hundreds and thousands of rays -- runs longer than a wave and longer than a
    block of the sort or of the encoding."""
    sc = rc.scenes
    verts = sc.box_room((-1, -1, -1), (1, 1, 1), 1)
    assert len(verts) == 12
    cfg = {"blas": [(verts, np.arange(1, 13, dtype=np.uint32))], "instances": [(1, sc.IDENTITY3x4[None], np.zeros(1, np.uint32))]}
    w = World(rc, oracle, cfg)
    M = w.M(4096, 13)
    assert (M.sum(axis=1, dtype=np.uint64) == 4096).all() and int(M.max()) > 1024 and int(M[M > 0].min()) >= 64
    csr = rc.view_factors_sparse(w.t, 4096, seed=13)
    assert_is_the_matrix(tuple(csr), M)
    assert len(csr[1]) <= 12 * 11
    w.t.free()


# ---- 4. chunking changes nothing ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["room", "gaps"])
def test_chunking_changes_nothing(rc, room, gaps, which):
    w = room if which == "room" else gaps
    R, seed = 128, 5
    M = w.M(R, seed)
    if which == "gaps":
        assert M[6].sum() > 0 and not M[8:39].any() and int(M.sum(dtype=np.uint64)) < R * w.n  # rays from and onto metadata 0 / N + 50 are dropped
    t = w.t
    default = t.get_option("vf_sparse_scratch_bytes")
    assert default == 256 << 20
    whole = w.csr(R, seed)  # one chunk
    assert_is_the_matrix(tuple(whole), M)
    if which == "gaps":
        p = whole[0].astype(np.int64)
        assert (np.diff(p)[8:39] == 0).all() and p[7] > p[6]  # the empty rows; the shared row 6 holds the 35 sources' hits
        assert int(whole[2][p[6]:p[7]].sum()) > R  # more rays than ONE source shoots: the sources were merged into the row
    try:
        # one row per chunk (the shared row's 35 sources x R rays exceed it: a chunk of its own); a handful of ragged chunks
        for cap in (8, 1, 8 * R * 50, 8 * R * 61 + 3, 8 * R * w.n - 1):
            t.set_option("vf_sparse_scratch_bytes", cap)
            assert t.get_option("vf_sparse_scratch_bytes") == max(cap, 8)
            got = rc.view_factors_sparse(t, R, seed=seed)
            for a, b in zip(got, whole):
                assert np.array_equal(a, b), cap
    finally:
        t.set_option("vf_sparse_scratch_bytes", default)


# ---- 5. row blocks ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["room", "gaps"])
def test_row_blocks_concatenate(rc, room, gaps, which):
    w = room if which == "room" else gaps
    R, seed = 128, 5
    whole = w.csr(R, seed)
    M = w.M(R, seed)
    parts = []
    for r0, r1 in ((0, 50), (50, 50), (50, 131), (131, w.n + 1000)):  # three ragged blocks and an empty one; the end is clamped
        b = rc.view_factors_sparse(w.t, R, seed=seed, rows=(r0, r1))
        r1 = min(r1, w.n)
        assert b.row_offset == r0 and b.n_rows == r1 - r0 and int(b[0][0]) == 0 and b.n == w.n
        assert_is_the_matrix(tuple(b), M[r0:r1], (r0, r1))
        parts.append(b)
    assert np.array_equal(np.concatenate([p[1] for p in parts]), whole[1]) and np.array_equal(np.concatenate([p[2] for p in parts]), whole[2])
    ptr, base = [np.zeros(1, np.uint64)], 0
    for p in parts:
        ptr.append(p[0][1:] + np.uint64(base))
        base += int(p[0][-1])
    assert np.array_equal(np.concatenate(ptr), whole[0])
    # blocks past the end are empty
    b = rc.view_factors_sparse(w.t, R, seed=seed, rows=(w.n + 5, w.n + 9))
    assert b.n_rows == 0 and b.nnz == 0 and np.array_equal(b[0], np.zeros(1, np.uint64))


# ---- 6. capacity ------------------------------------------------------------------------------------------------------------------------------
def test_capacity_contract(rc, room):
    from raycore_jl_amd._capi import lib, ptr
    t, n = room.t, room.n
    R, seed = 128, 5
    want_ptr, want_cols, want_vals = room.csr(R, seed)
    nnz = len(want_cols)
    assert nnz > 100
    # the counting call: NULL arrays
    d = DeviceCsr(n, 0)
    d.build(t, R, seed, null_arrays=True)
    finish(room.t)
    row_ptr, got_nnz, cols, vals = d.read()
    assert got_nnz == nnz and np.array_equal(row_ptr, want_ptr)
    assert (cols == GUARD).all() and (vals == GUARD).all()
    # too small by five, exact, larger than needed
    for capacity in (nnz - 5, nnz, nnz + 3, 1):
        d = DeviceCsr(n, capacity)
        d.build(t, R, seed)
        finish(room.t)
        row_ptr, got_nnz, cols, vals = d.read()
        k = min(capacity, nnz)
        assert got_nnz == nnz and np.array_equal(row_ptr, want_ptr), capacity
        assert np.array_equal(cols[:k], want_cols[:k]) and np.array_equal(vals[:k], want_vals[:k]), capacity
        assert (cols[k:] == GUARD).all() and (vals[k:] == GUARD).all(), capacity  # nothing at or beyond the capacity, nothing beyond nnz
    # the python wrapper with a capacity reports the true count
    short = rc.view_factors_sparse(t, R, seed=seed, capacity=nnz - 5)
    assert short.nnz == nnz and len(short[1]) == nnz - 5 and np.array_equal(short[1], want_cols[:nnz - 5]) and np.array_equal(short[0], want_ptr)
    with pytest.raises(ValueError, match="truncated"):
        rc.view_factor_sparse_products(short, np.ones(n, np.uint32))
    # the host form of the C ABI
    L = lib()
    row_ptr, cols, vals = np.zeros(n + 1, np.uint64), np.full(nnz + 2, GUARD, np.uint32), np.full(nnz + 2, GUARD, np.uint32)
    out_nnz = np.zeros(1, np.uint64)
    assert L.rc_view_factors_sparse(t._h, R, seed, ptr(row_ptr), None, None, 0, ptr(out_nnz)) == 0
    assert int(out_nnz[0]) == nnz and np.array_equal(row_ptr, want_ptr)
    assert L.rc_view_factors_sparse(t._h, R, seed, ptr(row_ptr), ptr(cols), ptr(vals), nnz - 5, ptr(out_nnz)) == 0
    assert int(out_nnz[0]) == nnz and np.array_equal(cols[:nnz - 5], want_cols[:nnz - 5]) and (cols[nnz - 5:] == GUARD).all()
    assert L.rc_view_factors_sparse(t._h, R, seed, ptr(row_ptr), ptr(cols), ptr(vals), nnz, ptr(out_nnz)) == 0
    assert np.array_equal(cols[:nnz], want_cols) and np.array_equal(vals[:nnz], want_vals) and (vals[nnz:] == GUARD).all()
    # the error contract
    d = DeviceCsr(n, 16)
    h = d.head.data_ptr()
    assert L.rc_view_factors_sparse_device(None, R, seed, 0, n, ptr(h), ptr(d.cols.data_ptr()), ptr(d.vals.data_ptr()), 16, ptr(h), None) == RC_ERR_INVALID_ARGUMENT
    assert L.rc_view_factors_sparse_device(t._h, R, seed, 0, n, None, ptr(d.cols.data_ptr()), ptr(d.vals.data_ptr()), 16, ptr(h), None) == RC_ERR_INVALID_ARGUMENT
    assert L.rc_view_factors_sparse_device(t._h, R, seed, 0, n, ptr(h), None, ptr(d.vals.data_ptr()), 16, ptr(h), None) == RC_ERR_INVALID_ARGUMENT
    assert L.rc_view_factors_sparse_device(t._h, R, seed, 0, n, ptr(h), ptr(d.cols.data_ptr()), ptr(d.vals.data_ptr()), 16, None, None) == RC_ERR_INVALID_ARGUMENT
    finish(room.t)


# ---- 7. an instanced scene -------------------------------------------------------------------------------------------------------------------
def test_instanced_scene(rc, lattice):
    """Hits are counted by the metadata of the hit primitive whatever instance it sits in (src/kernels.jl:93-97)."""
    M = lattice.M(64, 9)
    assert M.sum() > 0
    assert_is_the_matrix(tuple(lattice.csr(64, 9)), M)


# ---- 8. two streams at once, each into its own arrays -------------------------------------------------------------------------------------
def test_two_streams_at_once(rc, room):
    import torch
    t, n = room.t, room.n
    wants = [room.csr(128, 5), room.csr(192, 77)]
    jobs = [(128, 5), (192, 77)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for rep in range(3):
        ds = [DeviceCsr(n, len(w[1])) for w in wants]
        for d, st in zip(ds, (s1, s2)):
            for buf in (d.head, d.cols, d.vals):
                buf.record_stream(st)
        torch.cuda.synchronize()
        for d, st, (R, seed) in zip(ds, (s1, s2), jobs):
            d.build(t, R, seed, stream=st.cuda_stream)
        torch.cuda.synchronize()
        for d, w in zip(ds, wants):
            row_ptr, nnz, cols, vals = d.read()
            assert nnz == len(w[1]) and np.array_equal(row_ptr, w[0]), rep
            assert np.array_equal(cols[:nnz], w[1]) and np.array_equal(vals[:nnz], w[2]), rep
    finish(room.t)


def test_build_refuses_a_capturing_stream(rc, room):
    import torch
    from raycore_jl_amd._capi import lib, ptr
    t, n = room.t, room.n
    room.csr(128, 5)  # the source order exists: the refusal is the build's own
    d = DeviceCsr(n, 64)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        h = d.head.data_ptr()
        status = lib().rc_view_factors_sparse_device(t._h, 128, 5, 0, n, ptr(h), ptr(d.cols.data_ptr()), ptr(d.vals.data_ptr()), 64, ptr(h + 8 * (n + 1)),
                                                     ptr(torch.cuda.current_stream().cuda_stream))
        d.head.add_(0)  # (a graph must hold something)
    assert status == RC_ERR_NOT_SYNCED
    del g
    torch.cuda.synchronize()
    assert (u32_of(d.cols) == GUARD).all()
    finish(room.t)


# ---- 9. the products on traced matrices ----------------------------------------------------------------------------------------------------
def traced(room, gaps, lattice, which):
    return {"room": (room, 192, 77), "gaps": (gaps, 128, 5), "lattice": (lattice, 64, 9)}[which]


@pytest.mark.parametrize("which", ["room", "gaps", "lattice"])
def test_products_on_traced_matrices(rc, room, gaps, lattice, which):
    import torch
    w, R, seed = traced(room, gaps, lattice, which)
    t, n = w.t, w.n
    M, csr = w.M(R, seed), w.csr(R, seed)
    for x in (full_range_x(n, 1), np.ones(n, np.uint32), np.full(n, U32_MAX, np.uint32)):
        mx, mtx = rc.view_factor_sparse_products(csr, x)
        w_mx, w_mtx = dense.products(M, x)
        assert mx.dtype == mtx.dtype == np.uint64 and len(mx) == len(mtx) == n
        assert np.array_equal(mx, w_mx) and np.array_equal(mtx, w_mtx)
        r_mx, r_mtx = rc.view_factor_products(t, x, R, seed=seed)  # the retraced products: the same words
        assert np.array_equal(mx, r_mx) and np.array_equal(mtx, r_mtx)
    # x = 1: the totals
    recv, emit = rc.view_factor_totals(t, R, seed=seed)
    mx, mtx = rc.view_factor_sparse_products(csr, np.ones(n, np.uint32))
    assert np.array_equal(mx, emit) and np.array_equal(mtx, recv)
    # the device call: NULL outputs, accumulation onto non-zero words modulo 2^64, a row block with its offset
    x = full_range_x(n, 2)
    w_mx, w_mtx = dense.products(M, x)
    row_ptr, cols, vals = csr.device_arrays()
    d_x = dev_u32(x)
    start = np.random.default_rng(3).integers(0, 1 << 64, 2 * n, dtype=np.uint64)
    acc = dev_u64(start)
    torch.cuda.synchronize()
    t.view_factor_sparse_products_device(n, row_ptr.data_ptr(), cols.data_ptr(), vals.data_ptr(), d_x.data_ptr(), acc.data_ptr(), None)
    t.view_factor_sparse_products_device(n, row_ptr.data_ptr(), cols.data_ptr(), vals.data_ptr(), d_x.data_ptr(), None, acc.data_ptr() + 8 * n)
    finish(w.t)
    got = u64_of(acc)
    assert np.array_equal(got[:n], start[:n] + w_mx) and np.array_equal(got[n:], start[n:] + w_mtx)
    both = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    a, c = n // 4 + 2, (2 * n) // 3 + 1
    for r0, r1 in ((0, a), (a, a), (a, c), (c, n)):  # three ragged blocks and an empty one
        b = rc.view_factors_sparse(t, R, seed=seed, rows=(r0, r1))
        bp, bc, bv = b.device_arrays()
        t.view_factor_sparse_products_device(r1 - r0, bp.data_ptr(), bc.data_ptr() if b.nnz else None, bv.data_ptr() if b.nnz else None, d_x.data_ptr(),
                                             both.data_ptr(), both.data_ptr() + 8 * n, row_offset=r0)
        finish(w.t)
        if r1 > r0:
            one = rc.view_factor_sparse_products(b, x)
            s_mx, s_mtx = model.spmv(tuple(b), x, row_offset=r0)
            assert np.array_equal(one[0], s_mx) and np.array_equal(one[1], s_mtx)
    got = u64_of(both)
    assert np.array_equal(got[:n], w_mx) and np.array_equal(got[n:], w_mtx)
    # the error contract
    from raycore_jl_amd._capi import lib, ptr
    L = lib()
    args = (ptr(row_ptr.data_ptr()), ptr(cols.data_ptr()), ptr(vals.data_ptr()))
    assert L.rc_view_factor_sparse_products_device(t._h, n, 0, *args, ptr(d_x.data_ptr()), None, None, None) == RC_ERR_INVALID_ARGUMENT
    assert L.rc_view_factor_sparse_products_device(t._h, n, 0, *args, None, ptr(both.data_ptr()), None, None) == RC_ERR_INVALID_ARGUMENT
    assert L.rc_view_factor_sparse_products_device(t._h, n, 0, None, *args[1:], ptr(d_x.data_ptr()), ptr(both.data_ptr()), None, None) == RC_ERR_INVALID_ARGUMENT
    finish(w.t)
    assert np.array_equal(u64_of(both)[:n], w_mx)


# ---- 10. the products on handmade matrices -------------------------------------------------------------------------------------------------
def handmade(n, lengths, rng, top=1 << 32, hot=None):
    """A canonical CSR with the given row lengths (rows beyond the list get 0..8 entries), random columns and values in 1..top - 1;
    hot: a column every row contains."""
    lengths = list(lengths) + [int(v) for v in rng.integers(0, 9, n - len(lengths))]
    cols = []
    for L in lengths:
        c = np.sort(rng.choice(n, L, replace=False)) if L < n else np.arange(n)
        if hot is not None and hot not in c:
            c = np.sort(np.append(c, hot)) if L else np.array([hot])
        cols.append(c)
    row_ptr = np.zeros(n + 1, np.uint64)
    row_ptr[1:] = np.cumsum([len(c) for c in cols])
    cols = np.concatenate(cols).astype(np.uint32) if n else np.zeros(0, np.uint32)
    vals = rng.integers(1, top, len(cols), dtype=np.uint64).astype(np.uint32)
    csr = (row_ptr, cols, vals)
    assert model.is_canonical(csr, max(n, 1))
    return csr


def test_products_on_handmade_matrices(rc, room):
    rng = np.random.default_rng(17)
    t = room.t  # any scene: the products read the arrays alone
    cases = {"empty": (handmade(7, [0] * 7, rng), 7),
             "one": ((np.array([0, 1], np.uint64), np.array([0], np.uint32), np.array([U32_MAX], np.uint32)), 1),
             "one_empty": ((np.array([0, 0], np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32)), 1),
             "lengths": (handmade(4100, [0, 1, 63, 64, 65, 1025, 4100, 0, 0, 127, 128, 129], rng), 4100),
             "hot": (handmade(4100, [3] * 4100, rng, hot=1234), 4100),
             "wrap": (handmade(300, [300] * 300, rng, top=1 << 32), 300)}
    cases["wrap"][0][2][:] = U32_MAX  # 300 x (2^32 - 1)^2 wraps past 2^64
    assert len(cases["empty"][0][1]) == 0 and len(cases["lengths"][0][1]) > 4100 + 1025
    assert (np.bincount(cases["hot"][0][1], minlength=4100)[1234]) == 4100
    for name, (csr, n) in cases.items():
        m = rc.SparseViewFactors.from_arrays(t, *csr, n=n)
        for x in (full_range_x(max(n, 3), 5)[:n], np.full(n, U32_MAX, np.uint32)):
            mx, mtx = rc.view_factor_sparse_products(m, x)
            w_mx, w_mtx = model.spmv(csr, x)
            assert np.array_equal(mx, w_mx) and np.array_equal(mtx, w_mtx), name
    x = np.full(300, U32_MAX, np.uint32)
    mx, _ = rc.view_factor_sparse_products(rc.SparseViewFactors.from_arrays(t, *cases["wrap"][0]), x)
    assert [int(v) for v in mx[:2]] == [(300 * U32_MAX * U32_MAX) % (1 << 64)] * 2 and 300 * U32_MAX * U32_MAX >= 1 << 64
    # a block of the `lengths` matrix with its offset
    row_ptr, cols, vals = cases["lengths"][0]
    r0, r1 = 2, 9
    block = ((row_ptr[r0:r1 + 1] - row_ptr[r0]), cols[int(row_ptr[r0]):int(row_ptr[r1])], vals[int(row_ptr[r0]):int(row_ptr[r1])])
    x = full_range_x(4100, 6)
    got = rc.view_factor_sparse_products(rc.SparseViewFactors.from_arrays(t, *block, n=4100, row_offset=r0), x)
    want = model.spmv(block, x, row_offset=r0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and not got[0][:r0].any() and not got[0][r1:].any()
    finish(room.t)


# ---- 11. bounces and radiosity on the matrix -----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("k", [0, 1, 5])
def test_bounces_on_the_matrix_equal_the_retraced_ones(rc, room, k):
    import torch
    R, seed = 48, 31
    M, csr = room.M(R, seed), room.csr(R, seed)
    e, rho = bounce_inputs(room.n, 9)
    e[7] = U32_MAX - 3  # saturates at the first bounce wherever anything arrives
    rho[7] = 65536
    want = dense.bounces(M, R, e, rho, k)
    got = rc.view_factor_bounces(csr, e, rho, k)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint32 and np.array_equal(got, want)
    assert np.array_equal(got, rc.view_factor_bounces(room.t, e, rho, k, rays_per_triangle=R, seed=seed))
    # device tensors in, a device tensor out, on a side stream
    st = torch.cuda.Stream()
    d_e, d_rho = torch.from_numpy(e.astype(np.int64)).cuda(), dev_u32(rho)
    for buf in (d_e, d_rho):
        buf.record_stream(st)
    torch.cuda.synchronize()
    out = rc.view_factor_bounces(csr, d_e, d_rho, k, stream=st)
    st.synchronize()
    assert out.dtype == torch.int64 and out.is_cuda and np.array_equal(out.cpu().numpy().astype(np.uint32), want)
    # a block of rows is no matrix to bounce on
    with pytest.raises(ValueError, match="all rows"):
        rc.view_factor_bounces(rc.view_factors_sparse(room.t, R, seed=seed, rows=(0, 10)), e, rho, k)
    finish(room.t)


def test_captured_sparse_bounce_replayed(rc, room):
    """zero -> sparse products -> the torch update (raycore_jl_amd.api.bounce_step_sparse), captured with no eager step before it: the
    product reads nothing on the host.  Five replays are five bounces."""
    import torch
    from raycore_jl_amd.api import bounce_step_sparse
    R, seed = 48, 31
    M, csr = room.M(R, seed), room.csr(R, seed)
    n = room.n
    csr.device_arrays()
    e_np, rho_np = bounce_inputs(n, 8)
    e, rho = torch.from_numpy(e_np.astype(np.int64)).cuda(), torch.from_numpy(rho_np.astype(np.int64)).cuda()
    x = e.clone()
    x32, mx = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda")
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
    want = dense.bounces(M, R, e_np, rho_np, 5)
    assert np.array_equal(x.cpu().numpy().astype(np.uint32), want) and (want != e_np).any()
    del g
    finish(room.t)


def test_radiosity_on_the_matrix(rc, room):
    R, seed, K = 48, 31, 5
    csr = room.csr(R, seed)
    rng = np.random.default_rng(10)
    e = rng.random(room.n) * 3.0
    e[::13] = 0.0
    rho = np.full(room.n, 0.7)
    want, w_scale = rc.radiosity(room.t, e, rho, K, rays_per_triangle=R, seed=seed, return_scale=True)
    got, scale = rc.radiosity(room.t, e, rho, K, return_scale=True, matrix=csr)
    assert scale == w_scale and got.dtype == np.float64 and np.array_equal(got, want)
    assert (got > e + 0.1).any()  # the bounces matter
    finish(room.t)
