"""CPU-side checks of the sparse matrix between placed primitives (rc_placed_view_factors_sparse_device) and of the Python layer on top
of it: the binding matches the header's prototype, the library exports it, the Julia layer and the documents carry it, every ValueError of
placed_view_factors_sparse and of the bounce calls with a placed matrix is raised before a device is touched -- and the composed
yardstick of tests/test_gpu_placed_view_factors_sparse.py is pinned on the oracle: the canonical CSR of the placed model's matrix, applied
with the sparse model's product, gives the placed model's own products."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import placed_products_model as pm
import placed_vf_model as placed
import vf_sparse_model as sparse
from api_kit import ROOT, header, julia_text, prototype
from api_kit import rc  # noqa: F401
from helpers import build_oracle
from scene_kit import full_range_x, scenes_module

NAME = "rc_placed_view_factors_sparse_device"
PROTOTYPE = ["rc_scene*", "uint32_t", "uint64_t", "uint32_t", "uint32_t", "uint32_t", "uint64_t*", "uint32_t*", "uint32_t*", "uint64_t", "uint64_t*", "void*"]
JL_ARGS = ["Ptr{Cvoid}", "UInt32", "UInt64", "UInt32", "UInt32", "UInt32", "Ptr{UInt64}", "Ptr{UInt32}", "Ptr{UInt32}", "UInt64", "Ptr{UInt64}", "Ptr{Cvoid}"]
CTYPES = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
RC_ERR_INVALID_ARGUMENT = 1


class Untouchable:
    """Stands in for an accel: any use of it is a failure of the test -- the argument checks come first."""

    def __getattr__(self, name):
        raise AssertionError(f"the accel was touched ({name}) before the arguments were checked")


# ---- the symbol in the header, the binding, the library, Julia and the documents ---------------------------------------------------------
def test_header_capi_and_julia_agree_on_the_symbol(rc):
    assert prototype(NAME) == PROTOTYPE
    res, args = {n: (r, a) for n, r, a in rc.SYMBOLS}[NAME]
    assert res is C.c_int and args == [CTYPES.get(a, C.c_void_p) for a in PROTOTYPE]
    assert hasattr(rc.lib(), NAME)
    text = julia_text()
    m = re.search(r"ccall\(\(:" + NAME + r", LIB\), Cint,\s*\(([^)]*)\)", text)
    assert m, f"no ccall of {NAME}"
    assert [t.strip() for t in m.group(1).split(",")] == JL_ARGS
    assert re.search(r"^placed_view_factors_sparse_device!\(a::MI355XStaticTLAS, rays_per_triangle::Integer, seed::UInt64, sampling::Integer, placed_begin::Integer,", text,
                     flags=re.M)


def test_header_documents_the_call():
    text = header()
    at = text.index("int " + NAME)
    comment = " ".join(text[text.rindex("/* ----", 0, at):at].replace("\n *", " ").split())
    for needle in ("Sparse matrix between placed primitives", "min(R, P - 1)", "bit for bit those of rc_placed_view_factor_rays_device",
                   "b = base[hit instance] + prim - 1 with b != a", "the diagonal is empty", "OVERWRITES", "placed_end is clamped to P",
                   "is always the true one", "*d_nnz is the true count", "nothing is written at or beyond `capacity`", "counting call", "strictly ascending within a row",
                   "every d_vals >= 1", '"vf_sparse_scratch_bytes"', "THE MATRIX IS A SNAPSHOT", "still describe the OLD placement", "rebuilding the matrix is the caller's job",
                   "THE PRODUCTS are rc_view_factor_sparse_products_device", "row_offset = placed_begin", "There is no host-array form", "two streams may build at once",
                   "rc_update_transforms_device -> rc_refit_device_async", "rc_update_geometry_device_async", "NOT capturable",
                   "all before anything is enqueued and with the outputs untouched", "NULL d_cols / d_vals with capacity > 0", "sampling above RC_VF_SAMPLING_COSINE",
                   "P >= 2^32", "RC_ERR_NOT_SYNCED in the states in which rc_placed_view_factor_products_device returns it",
                   'docs/EXPERIMENTS.md, "Sparse matrix between placed primitives"'):
        assert needle in comment, needle
    assert "of the sparse matrix do not exist yet" not in text
    assert "A placed form of the dense matrix does not exist yet" in " ".join(text.replace("\n *", " ").split())


def test_the_documents_carry_the_call():
    for f in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert NAME in open(os.path.join(ROOT, f)).read(), f
    assert "placed_view_factors_sparse_device!" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "## Sparse matrix between placed primitives" in open(os.path.join(ROOT, "docs", "EXPERIMENTS.md")).read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "placed_view_factors_sparse_isa.txt"))


def test_python_surface(rc):
    sig = inspect.signature(rc.TLAS.placed_view_factors_sparse_device)
    assert list(sig.parameters) == ["self", "row_ptr_ptr", "cols_ptr", "vals_ptr", "capacity", "nnz_ptr", "rays_per_triangle", "seed", "sampling", "rows", "stream"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["sampling"], d["rows"], d["stream"]) == ("uniform", None, None)
    sig = inspect.signature(rc.placed_view_factors_sparse)
    assert list(sig.parameters) == ["accel", "rays_per_triangle", "seed", "sampling", "rows", "capacity"]
    assert [p.default for p in sig.parameters.values()][1:] == [10000, 0, "uniform", None, None]
    sig = inspect.signature(rc.placed_radiosity)
    assert list(sig.parameters)[-1] == "matrix" and sig.parameters["matrix"].default is None
    sig = inspect.signature(rc.SparseViewFactors.__new__)
    assert (sig.parameters["sampling"].default, sig.parameters["placed"].default) == (None, False)
    assert "snapshot" in rc.placed_view_factors_sparse.__doc__.lower() and "SparseViewFactors" in rc.placed_view_factor_bounces.__doc__


def test_existing_uses_of_the_matrix_class_are_unchanged(rc):
    row_ptr, cols, vals = good_csr()
    m = rc.SparseViewFactors.from_arrays(Untouchable(), row_ptr, cols, vals)
    assert m.placed is False and m.sampling is None and m.n == 3 and m.nnz == 3
    m = rc.SparseViewFactors(row_ptr, cols, vals, Untouchable(), 3, 0, 16, 5, 3, None)  # every positional argument it had
    assert m.placed is False and m.sampling is None and (m.rays_per_triangle, m.seed) == (16, 5)


def test_null_and_sampling_arguments_are_refused_without_a_device(rc):
    f = rc.lib().rc_placed_view_factors_sparse_device
    assert f(None, 16, 1, 0, 0, 4, 64, 64, 64, 8, 64, None) == RC_ERR_INVALID_ARGUMENT
    assert f(None, 0, 0, 0, 0, 0, None, None, None, 0, None, None) == RC_ERR_INVALID_ARGUMENT
    no_scene = type("NoScene", (), {"_h": None})()  # the sampling name is refused while the arguments are put together
    with pytest.raises(ValueError, match="sampling"):
        rc.TLAS.placed_view_factors_sparse_device(no_scene, 64, 64, 64, 8, 64, 16, 0, "lambert")


# ---- the argument checks, without a device -------------------------------------------------------------------------------------------------
def test_sparse_arguments_are_checked_before_the_library(rc):
    accel = Untouchable()
    cases = [({"rays_per_triangle": 0}, "rays_per_triangle"), ({"rays_per_triangle": 1 << 32}, "rays_per_triangle"), ({"rays_per_triangle": 2.5}, "rays_per_triangle"),
             ({"rays_per_triangle": True}, "rays_per_triangle"), ({"seed": -1}, "seed"), ({"seed": 1 << 64}, "seed"), ({"rows": (5, 3)}, "rows"),
             ({"rows": (-1, 3)}, "rows"), ({"rows": 7}, "rows"), ({"rows": (0, 1, 2)}, "rows"), ({"rows": (0, 1.5)}, "rows"), ({"capacity": -1}, "capacity"),
             ({"capacity": 1.5}, "capacity"), ({"sampling": "lambert"}, "sampling"), ({"sampling": 2}, "sampling"), ({"sampling": None}, "sampling"),
             ({"sampling": True}, "sampling")]
    for kw, what in cases:
        with pytest.raises(ValueError, match=what):
            rc.placed_view_factors_sparse(accel, **kw)
    assert rc.check_placed_sparse_arguments((1 << 32) - 1, (1 << 64) - 1, "cosine", (0, 0), 0) == 1  # the largest and smallest legal values pass
    assert rc.check_placed_sparse_arguments(1, 0, "uniform", None, None) == 0
    assert rc.check_placed_sparse_arguments(1, 0, 1, None, None) == 1
    with pytest.raises(ValueError, match="sampling"):
        rc.check_placed_sparse_arguments(16, 0, "lambert", None, None)


def good_csr():
    return np.array([0, 2, 2, 3], np.uint64), np.array([1, 2, 1], np.uint32), np.array([5, 1, 7], np.uint32)


def test_bounce_matrix_checks_raise_before_the_library(rc):
    accel = Untouchable()
    row_ptr, cols, vals = good_csr()
    e, rho = np.arange(3, dtype=np.uint32), np.full(3, 65536, np.uint32)

    def matrix(n=3, **kw):
        kw = {"rays_per_triangle": 16, "seed": 0, "sampling": 1, "placed": True, **kw}
        return rc.SparseViewFactors(row_ptr, cols, vals, accel, n, **kw)

    # a matrix that is not placed: the per-triangle family's, traced or handmade
    for m in (matrix(placed=False), rc.SparseViewFactors.from_arrays(accel, row_ptr, cols, vals)):
        with pytest.raises(ValueError, match="placed"):
            rc.check_placed_bounce_matrix(m)
        with pytest.raises(ValueError, match="placed"):
            rc.placed_view_factor_bounces(m, e, rho, 1)
    with pytest.raises(ValueError, match="placed"):
        rc.check_placed_bounce_matrix((row_ptr, cols, vals))
    # a row block
    for block in (matrix(5, row_offset=1), matrix(5)):
        with pytest.raises(ValueError, match="all rows"):
            rc.check_placed_bounce_matrix(block)
        with pytest.raises(ValueError, match="all rows"):
            rc.placed_view_factor_bounces(block, np.arange(5, dtype=np.uint32), np.full(5, 65536, np.uint32), 1)
    # a truncated matrix
    with pytest.raises(ValueError, match="truncated"):
        rc.check_placed_bounce_matrix(matrix(nnz=9))
    with pytest.raises(ValueError, match="truncated"):
        rc.placed_view_factor_bounces(matrix(nnz=9), e, rho, 1)
    # a wrong length: counted in placed primitives, the matrix's n
    rc.check_placed_bounce_matrix(matrix())
    for n in (2, 4):
        with pytest.raises(ValueError, match="one value per placed primitive: %d values for 3 placed primitives" % n):
            rc.placed_view_factor_bounces(matrix(), np.zeros(n, np.uint32), np.zeros(n, np.uint32), 1)
        with pytest.raises(ValueError, match="one value per placed primitive: %d values for 3 placed primitives" % n):
            rc.placed_radiosity(accel, np.ones(n), np.full(n, 0.5), 2, matrix=matrix())
    # an unknown sampling, in the matrix and in the call
    for bad in ("lambert", 2, None):
        with pytest.raises(ValueError, match="sampling"):
            rc.placed_view_factor_bounces(matrix(sampling=bad), e, rho, 1)
    with pytest.raises(ValueError, match="sampling"):
        rc.placed_radiosity(accel, np.ones(3), np.full(3, 0.5), 2, sampling="lambert", matrix=matrix())
    # the other arguments keep their checks; the matrix's own rays_per_triangle is the one that is read
    for args, what in (((e, np.array([0, 65537, 2], np.uint32), 1), "reflectance"), ((e, rho, -1), "bounces"), ((e.astype(np.float32), rho, 1), "emission")):
        with pytest.raises(ValueError, match=what):
            rc.placed_view_factor_bounces(matrix(), *args)
    with pytest.raises(ValueError, match="rays_per_triangle"):
        rc.placed_view_factor_bounces(matrix(rays_per_triangle=1 << 31), e, rho, 1, rays_per_triangle=16)
    with pytest.raises(ValueError, match="SparseViewFactors"):
        rc.placed_radiosity(accel, np.ones(3), np.full(3, 0.5), 2, matrix=(row_ptr, cols, vals))
    with pytest.raises(ValueError, match=r"reflectance must lie in \[0, 1\)"):
        rc.placed_radiosity(accel, np.ones(3), np.ones(3), 2, matrix=matrix())
    # the per-triangle bounce still takes its own matrices only by their rows and counts
    with pytest.raises(ValueError, match="view_factors_sparse"):
        rc.view_factor_bounces(rc.SparseViewFactors.from_arrays(accel, row_ptr, cols, vals), e, rho, 1)


# ---- the composed yardstick, on the oracle alone ---------------------------------------------------------------------------------------------
class Rc:
    """What the scene makers of the model read of the product module: its scene generators (pure numpy)."""
    scenes = scenes_module()


@pytest.fixture(scope="module")
def plates(oracle):
    return build_oracle(oracle, placed.plates_cfg(Rc))


@pytest.mark.parametrize("sampling", placed.SAMPLINGS)
def test_the_csr_of_the_models_matrix_gives_the_models_products(plates, sampling):
    R = 96
    traced = placed.Traced(plates, R, 7, sampling)
    P = traced.n
    assert P == 16
    Mp, escaped = pm.matrix(traced)
    csr = sparse.csr_from_dense(Mp)
    assert sparse.is_canonical(csr, P) and int(csr[0][-1]) == np.count_nonzero(Mp) > 0
    dense = sparse.densify(csr, P)
    assert np.array_equal(dense, Mp) and not np.diag(dense).any()
    for x in (full_range_x(P, 1), np.full(P, pm.U32_MAX, np.uint32), np.ones(P, np.uint32)):
        mx, mtx = sparse.spmv(csr, x)
        want = pm.products(traced, x)
        assert mx.dtype == mtx.dtype == np.uint64 and np.array_equal(mx, want[0]) and np.array_equal(mtx, want[1])
    # every ray of a source is in its row, escaped, or a hit on the source itself
    _, _, esc, self_hits = pm.products(traced, None)
    assert np.array_equal(esc, escaped)
    assert np.array_equal(dense.sum(axis=1, dtype=np.uint64) + esc + self_hits, np.full(P, R, np.uint64))
    # a row block with its offset accumulates to the whole
    mx, mtx = np.zeros(P, np.uint64), np.zeros(P, np.uint64)
    x = full_range_x(P, 2)
    for r0, r1 in ((0, 5), (5, 5), (5, P)):
        block = sparse.csr_from_dense(Mp[r0:r1])
        a, b = sparse.spmv(block, x, row_offset=r0)
        with np.errstate(over="ignore"):
            mx += a
            mtx += b
    want = pm.products(traced, x)
    assert np.array_equal(mx, want[0]) and np.array_equal(mtx, want[1])
