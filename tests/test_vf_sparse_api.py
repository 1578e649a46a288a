"""CPU-side checks of the sparse view-factor matrix (rc_view_factors_sparse_device, rc_view_factors_sparse,
rc_view_factor_sparse_products_device): the bindings match the header's prototypes, the library exports them, the Python and Julia layers
carry them, and every ValueError of view_factors_sparse, view_factor_sparse_products, SparseViewFactors.from_arrays and of the bounce
calls with a matrix is raised before the library is touched, with or without a GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from api_kit import ROOT, header, julia_text, prototype
from api_kit import rc  # noqa: F401

C_TO_CTYPES = {"rc_scene*": C.c_void_p, "void*": C.c_void_p, "const uint32_t*": C.c_void_p, "const uint64_t*": C.c_void_p, "uint64_t*": C.c_void_p,
               "uint32_t*": C.c_void_p, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
ARGS = {"rc_view_factors_sparse_device": ["rc_scene*", "uint32_t", "uint64_t", "uint32_t", "uint32_t", "uint64_t*", "uint32_t*", "uint32_t*", "uint64_t",
                                          "uint64_t*", "void*"],
        "rc_view_factors_sparse": ["rc_scene*", "uint32_t", "uint64_t", "uint64_t*", "uint32_t*", "uint32_t*", "uint64_t", "uint64_t*"],
        "rc_view_factor_sparse_products_device": ["rc_scene*", "uint32_t", "uint32_t", "const uint64_t*", "const uint32_t*", "const uint32_t*",
                                                  "const uint32_t*", "uint64_t*", "uint64_t*", "void*"]}
JL_ARGS = {"rc_view_factors_sparse_device": ["Ptr{Cvoid}", "UInt32", "UInt64", "UInt32", "UInt32", "Ptr{UInt64}", "Ptr{UInt32}", "Ptr{UInt32}", "UInt64",
                                             "Ptr{UInt64}", "Ptr{Cvoid}"],
           "rc_view_factors_sparse": ["Ptr{Cvoid}", "UInt32", "UInt64", "Ptr{UInt64}", "Ptr{UInt32}", "Ptr{UInt32}", "UInt64", "Ptr{UInt64}"],
           "rc_view_factor_sparse_products_device": ["Ptr{Cvoid}", "UInt32", "UInt32", "Ptr{UInt64}", "Ptr{UInt32}", "Ptr{UInt32}", "Ptr{UInt32}", "Ptr{UInt64}",
                                                     "Ptr{UInt64}", "Ptr{Cvoid}"]}
NAMES = sorted(ARGS)


class Untouchable:
    """Stands in for an accel: any use of it is a failure of the test -- the argument checks come first."""

    def __getattr__(self, name):
        raise AssertionError(f"the accel was touched ({name}) before the arguments were checked")


@pytest.mark.parametrize("name", NAMES)
def test_symbol_matches_the_header(rc, name):
    assert prototype(name) == ARGS[name]
    bound = {n: (res, args) for n, res, args in rc.SYMBOLS}
    assert name in bound, f"{name} is missing from SYMBOLS"
    res, args = bound[name]
    assert res is C.c_int
    assert args == [C_TO_CTYPES[a] for a in ARGS[name]]


@pytest.mark.parametrize("name", NAMES)
def test_library_exports_the_symbol(rc, name):
    assert hasattr(rc.lib(), name)


def test_header_documents_both_families():
    text = header()
    at = text.index("int rc_view_factors_sparse_device")
    comment = text[text.rindex("/*", 0, at):at]
    build, products = comment.split("rc_view_factor_sparse_products_device:", 1)
    for needle in ("src/kernels.jl:74-104", "OVERWRITES", "canonical CSR", "strictly ascending", "no explicit zeros", "vf_sparse_scratch_bytes", "WHOLE rows",
                   "capacity", "always the true values", "nothing is written at or beyond capacity", "counting call", "RC_ERR_NOT_SYNCED",
                   "RC_ERR_INVALID_ARGUMENT", "2^32", "two streams may build at once", "row_end is clamped"):
        assert needle in build, needle
    for needle in ("src/kernels.jl:74-104", "ACCUMULATES", "modulo 2^64", "either output may be NULL", "d_mx [row_offset + r] += d_vals[k] * d_x[d_cols[k]]",
                   "d_mtx[d_cols[k]]      += d_vals[k] * d_x[row_offset + r]", "bit", "capturable", "NOT validated", "RC_ERR_INVALID_ARGUMENT",
                   'docs/EXPERIMENTS.md, "Sparse view-factor matrix"'):
        assert needle in products, needle


def test_python_surface(rc):
    sig = inspect.signature(rc.TLAS.view_factors_sparse_device)
    assert list(sig.parameters) == ["self", "row_ptr_ptr", "cols_ptr", "vals_ptr", "capacity", "nnz_ptr", "rays_per_triangle", "seed", "rows", "stream"]
    assert (sig.parameters["rows"].default, sig.parameters["stream"].default) == (None, None)
    sig = inspect.signature(rc.TLAS.view_factor_sparse_products_device)
    assert list(sig.parameters) == ["self", "n_rows", "row_ptr_ptr", "cols_ptr", "vals_ptr", "x_ptr", "mx_ptr", "mtx_ptr", "row_offset", "stream"]
    assert (sig.parameters["row_offset"].default, sig.parameters["stream"].default) == (0, None)
    sig = inspect.signature(rc.view_factors_sparse)
    assert list(sig.parameters) == ["accel", "rays_per_triangle", "seed", "rows", "capacity"]
    assert [p.default for p in sig.parameters.values()][1:] == [10000, 0, None, None]
    assert list(inspect.signature(rc.view_factor_sparse_products).parameters) == ["csr", "x"]
    sig = inspect.signature(rc.radiosity)
    assert "matrix" in sig.parameters and sig.parameters["matrix"].default is None
    assert "scipy.sparse.csr_matrix((vals, cols, row_ptr)" in " ".join(rc.view_factors_sparse.__doc__.split())
    assert "SparseViewFactors" in rc.view_factor_bounces.__doc__ and "matrix" in rc.radiosity.__doc__


def test_the_package_does_not_import_scipy():
    text = open(os.path.join(ROOT, "raycore.jl_amd", "api.py")).read()
    assert not re.search(r"^\s*(import|from)\s+scipy", text, flags=re.M)


@pytest.mark.parametrize("name", NAMES)
def test_julia_binding_has_the_method(name):
    text = julia_text()
    m = re.search(r"ccall\(\(:" + name + r", LIB\), Cint,\s*\(([^)]*)\)", text)
    assert m, f"no ccall of {name}"
    assert [t.strip() for t in m.group(1).split(",")] == JL_ARGS[name]
    method = name[3:] + ("!" if name.endswith("_device") else "")
    assert re.search(r"^(function )?" + re.escape(method) + r"\(a::MI355XStaticTLAS[,;] ", text, flags=re.M), method
    assert method in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert name in open(os.path.join(ROOT, "README.md")).read()


def test_null_arguments_are_refused_before_anything_else(rc):
    """NULL scene -> RC_ERR_INVALID_ARGUMENT whether or not a GPU is visible: the check comes first."""
    L = rc.lib()
    assert L.rc_view_factors_sparse_device(None, 16, 1, 0, 4, 64, 64, 64, 8, 64, None) == 1
    assert L.rc_view_factors_sparse_device(None, 0, 0, 0, 0, None, None, None, 0, None, None) == 1
    assert L.rc_view_factors_sparse(None, 16, 1, 64, 64, 64, 8, 64) == 1
    assert L.rc_view_factor_sparse_products_device(None, 4, 0, 64, 64, 64, 64, 64, 64, None) == 1
    assert L.rc_view_factor_sparse_products_device(None, 0, 0, None, None, None, None, None, None, None) == 1


def test_sparse_arguments_are_checked_before_the_library(rc):
    accel = Untouchable()
    cases = [({"rays_per_triangle": 0}, "rays_per_triangle"), ({"rays_per_triangle": 1 << 32}, "rays_per_triangle"), ({"rays_per_triangle": 2.5}, "rays_per_triangle"),
             ({"rays_per_triangle": True}, "rays_per_triangle"), ({"seed": -1}, "seed"), ({"seed": 1 << 64}, "seed"), ({"rows": (5, 3)}, "rows"),
             ({"rows": (-1, 3)}, "rows"), ({"rows": 7}, "rows"), ({"rows": (0, 1, 2)}, "rows"), ({"rows": (0, 1.5)}, "rows"), ({"capacity": -1}, "capacity"),
             ({"capacity": 1.5}, "capacity")]
    for kw, what in cases:
        with pytest.raises(ValueError, match=what):
            rc.view_factors_sparse(accel, **kw)
    from raycore_jl_amd.api import check_sparse_arguments
    check_sparse_arguments((1 << 32) - 1, (1 << 64) - 1, (0, 0), 0)  # the largest and smallest legal values pass
    check_sparse_arguments(1, 0, None, None)


def good_csr():
    return np.array([0, 2, 2, 3], np.uint64), np.array([0, 2, 1], np.uint32), np.array([5, 1, 7], np.uint32)


def test_csr_arrays_are_checked_before_the_library(rc):
    accel = Untouchable()
    row_ptr, cols, vals = good_csr()
    m = rc.SparseViewFactors.from_arrays(accel, row_ptr, cols, vals)
    assert m.n == 3 and m.n_rows == 3 and m.row_offset == 0 and m.nnz == 3 and m.rays_per_triangle is None
    a, b, c = m
    assert a is not None and np.array_equal(b, cols) and np.array_equal(c, vals)
    bad = [((row_ptr.astype(np.int64), cols, vals), "row_ptr"), ((row_ptr, cols.astype(np.int32), vals), "cols"), ((row_ptr, cols, vals.astype(np.float32)), "vals"),
           ((row_ptr + np.uint64(1), cols, vals), "start at 0"), ((row_ptr[:-1], cols, vals), "end at the number of entries"),
           ((row_ptr, cols[:-1], vals), "end at the number of entries"), ((np.array([0, 2, 1, 3], np.uint64), cols, vals), "not decrease"),
           ((row_ptr, np.array([0, 3, 1], np.uint32), vals), "cols must lie below 3"), ((list(row_ptr), cols, vals), "row_ptr"),
           ((np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32)), "start at 0")]
    for arrays, what in bad:
        with pytest.raises(ValueError, match=what):
            rc.SparseViewFactors.from_arrays(accel, *arrays)
    for kw, what in (({"n": 2}, "n must"), ({"n": 1 << 32}, "n must"), ({"row_offset": -1}, "row_offset"), ({"row_offset": 1, "n": 3}, "n must")):
        with pytest.raises(ValueError, match=what):
            rc.SparseViewFactors.from_arrays(accel, row_ptr, cols, vals, **kw)
    wide = rc.SparseViewFactors.from_arrays(accel, row_ptr, np.array([0, 9, 1], np.uint32), vals, n=10, row_offset=4)
    assert wide.n == 10 and wide.row_offset == 4
    # the products: the matrix and x are checked first
    for x in (np.zeros(3, np.float32), np.zeros(3, np.int32), np.zeros((3, 1), np.uint32), [1, 2, 3], None):
        with pytest.raises(ValueError, match="uint32"):
            rc.view_factor_sparse_products(m, x)
    with pytest.raises(ValueError, match="one value per primitive"):
        rc.view_factor_sparse_products(m, np.zeros(4, np.uint32))
    with pytest.raises(ValueError, match="SparseViewFactors"):
        rc.view_factor_sparse_products((row_ptr, cols, vals), np.zeros(3, np.uint32))
    truncated = rc.SparseViewFactors(row_ptr, cols, vals, accel, 3, nnz=8)
    with pytest.raises(ValueError, match="truncated"):
        rc.view_factor_sparse_products(truncated, np.zeros(3, np.uint32))
    cols[1] = 3  # edited after the check: checked again at the call
    with pytest.raises(ValueError, match="cols must lie below 3"):
        rc.view_factor_sparse_products(m, np.zeros(3, np.uint32))


def test_bounce_arguments_with_a_matrix_are_checked_before_the_library(rc):
    accel = Untouchable()
    row_ptr, cols, vals = good_csr()
    e, rho = np.arange(3, dtype=np.uint32), np.full(3, 65536, np.uint32)
    handmade = rc.SparseViewFactors.from_arrays(accel, row_ptr, cols, vals)
    with pytest.raises(ValueError, match="view_factors_sparse"):
        rc.view_factor_bounces(handmade, e, rho, 1)
    block = rc.SparseViewFactors(row_ptr, cols, vals, accel, 5, row_offset=1, rays_per_triangle=16, seed=0)
    with pytest.raises(ValueError, match="all rows"):
        rc.view_factor_bounces(block, e, rho, 1)
    short = rc.SparseViewFactors(row_ptr, cols, vals, accel, 3, rays_per_triangle=16, seed=0, nnz=9)
    with pytest.raises(ValueError, match="truncated"):
        rc.view_factor_bounces(short, e, rho, 1)
    whole = rc.SparseViewFactors(row_ptr, cols, vals, accel, 3, rays_per_triangle=16, seed=0)
    for args, what in (((e, np.array([0, 65537, 2], np.uint32), 1), "reflectance"), ((e, rho, -1), "bounces"), ((e[:2], rho[:2], 1), "one value per primitive"),
                       ((e.astype(np.float32), rho, 1), "emission")):
        with pytest.raises(ValueError, match=what):
            rc.view_factor_bounces(whole, *args)
    with pytest.raises(ValueError, match="SparseViewFactors"):
        rc.radiosity(accel, np.ones(3), np.full(3, 0.5), 2, matrix=(row_ptr, cols, vals))
    with pytest.raises(ValueError, match=r"reflectance must lie in \[0, 1\)"):
        rc.radiosity(accel, np.ones(3), np.ones(3), 2, matrix=whole)
