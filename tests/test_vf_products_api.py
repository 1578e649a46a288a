"""CPU-side checks of the view-factor products (rc_view_factor_products_device, rc_view_factor_products): the bindings match the header's
prototypes, the library exports them, the Python and Julia layers carry them, and every ValueError of view_factor_products,
view_factor_bounces and radiosity is raised before the library is touched, with or without a GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from api_kit import ROOT, header, julia_text, prototype
from api_kit import rc  # noqa: F401

C_TO_CTYPES = {"rc_scene*": C.c_void_p, "void*": C.c_void_p, "const uint32_t*": C.c_void_p, "uint64_t*": C.c_void_p, "uint32_t": C.c_uint32,
               "uint64_t": C.c_uint64}
ARGS = {"rc_view_factor_products_device": ["rc_scene*", "uint32_t", "uint64_t", "uint32_t", "uint32_t", "uint32_t", "uint32_t", "const uint32_t*",
                                           "uint64_t*", "uint64_t*", "void*"],
        "rc_view_factor_products": ["rc_scene*", "uint32_t", "uint64_t", "const uint32_t*", "uint64_t*", "uint64_t*"]}
JL_ARGS = {"rc_view_factor_products_device": ["Ptr{Cvoid}", "UInt32", "UInt64", "UInt32", "UInt32", "UInt32", "UInt32", "Ptr{UInt32}", "Ptr{UInt64}",
                                              "Ptr{UInt64}", "Ptr{Cvoid}"],
           "rc_view_factor_products": ["Ptr{Cvoid}", "UInt32", "UInt64", "Ptr{UInt32}", "Ptr{UInt64}", "Ptr{UInt64}"]}
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


def test_device_call_mirrors_the_totals_call():
    """Argument for argument rc_view_factor_totals_device's, with d_x in front of the two outputs."""
    totals = prototype("rc_view_factor_totals_device")
    assert ARGS["rc_view_factor_products_device"] == totals[:7] + ["const uint32_t*"] + totals[7:]


def test_header_documents_the_call():
    text = header()
    at = text.index("int rc_view_factor_products_device")
    comment = text[text.rindex("/*", 0, at):at]
    for needle in ("src/kernels.jl:74-104", "mx [a-1] += x[b-1]", "mtx[b-1] += x[a-1]", "modulo 2^64", "either output may be NULL", "ACCUMULATED",
                   "OVERWRITTEN", "rc_view_factor_totals", "RC_ERR_INVALID_ARGUMENT", "captured", 'docs/EXPERIMENTS.md, "View-factor products"'):
        assert needle in comment, needle


def test_python_surface(rc):
    sig = inspect.signature(rc.TLAS.view_factor_products_device)
    assert list(sig.parameters) == ["self", "x_ptr", "mx_ptr", "mtx_ptr", "rays_per_triangle", "seed", "src", "rays", "stream"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["src"], d["rays"], d["stream"]) == (None, None, None)
    sig = inspect.signature(rc.view_factor_products)
    assert list(sig.parameters) == ["accel", "x", "rays_per_triangle", "seed"]
    assert (sig.parameters["rays_per_triangle"].default, sig.parameters["seed"].default) == (10000, 0)
    sig = inspect.signature(rc.view_factor_bounces)
    assert list(sig.parameters) == ["accel", "emission", "reflectance", "bounces", "rays_per_triangle", "seed", "stream"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["rays_per_triangle"], d["seed"], d["stream"]) == (10000, 0, None)
    sig = inspect.signature(rc.radiosity)
    assert list(sig.parameters)[:6] == ["accel", "emission", "reflectance", "bounces", "rays_per_triangle", "seed"]
    for f in (rc.view_factor_bounces, rc.radiosity):  # the docstrings say what M is
        doc = " ".join(f.__doc__.split())
        assert "uniform" in doc and "hemisphere" in doc and "not cosine-corrected" in doc.lower(), f.__name__


@pytest.mark.parametrize("name", NAMES)
def test_julia_binding_has_the_method(name):
    text = julia_text()
    m = re.search(r"ccall\(\(:" + name + r", LIB\), Cint,\s*\(([^)]*)\)", text)
    assert m, f"no ccall of {name}"
    assert [t.strip() for t in m.group(1).split(",")] == JL_ARGS[name]
    method = name[3:] + ("!" if name.endswith("_device") else "")
    assert re.search(r"^(function )?" + re.escape(method) + r"\(a::MI355XStaticTLAS, ", text, flags=re.M), method
    assert method in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_null_arguments_are_refused_before_anything_else(rc):
    """NULL scene -> RC_ERR_INVALID_ARGUMENT whether or not a GPU is visible: the check comes first."""
    L = rc.lib()
    assert L.rc_view_factor_products_device(None, 16, 1, 0, 4, 0, 16, 64, 64, 64, None) == 1
    assert L.rc_view_factor_products_device(None, 0, 0, 0, 0, 0, 0, None, None, None, None) == 1
    assert L.rc_view_factor_products(None, 16, 1, 64, 64, 64) == 1


def test_products_x_is_checked_before_the_library(rc):
    accel = Untouchable()
    for bad in (np.zeros(4, np.float32), np.zeros(4, np.int32), np.zeros(4, np.uint64), np.zeros((2, 2), np.uint32), [1, 2, 3], None):
        with pytest.raises(ValueError, match="uint32"):
            rc.view_factor_products(accel, bad)
    from raycore_jl_amd.api import check_products_x
    with pytest.raises(ValueError, match="one value per primitive"):
        check_products_x(np.zeros(5, np.uint32), 4)
    x = np.arange(8, dtype=np.uint32)[::2]
    got = check_products_x(x, 4)
    assert got.flags["C_CONTIGUOUS"] and np.array_equal(got, x)


def test_bounce_arguments_are_checked_before_the_library(rc):
    accel = Untouchable()
    e, rho = np.arange(4, dtype=np.uint32), np.full(4, 65536, np.uint32)
    cases = [((e, np.array([0, 1, 65537, 2], np.uint32), 1), {}, "reflectance"),
             ((e, np.array([0, -1, 5, 2], np.int64), 1), {}, "reflectance"),
             ((e, rho, 1), {"rays_per_triangle": 1 << 31}, "rays_per_triangle"),
             ((e, rho, 1), {"rays_per_triangle": 0}, "rays_per_triangle"),
             ((e, rho, -1), {}, "bounces"),
             ((e, rho, 1.5), {}, "bounces"),
             ((np.array([0, 1 << 32, 0, 0], np.int64), rho, 1), {}, "emission"),
             ((e.astype(np.float32), rho, 1), {}, "emission"),
             ((e, rho[:3], 1), {}, "one value per primitive")]
    for args, kw, what in cases:
        with pytest.raises(ValueError, match=what):
            rc.view_factor_bounces(accel, *args, **kw)
    from raycore_jl_amd.api import check_bounce_arguments
    e64, r64 = check_bounce_arguments(e, rho, 0, (1 << 31) - 1)  # the largest legal values pass
    assert e64.dtype == r64.dtype == np.int64 and np.array_equal(e64, e) and np.array_equal(r64, rho)
    check_bounce_arguments(np.array([(1 << 32) - 1], np.uint32), np.array([0], np.uint32), 3, 1)


def test_radiosity_arguments_and_scale(rc):
    accel = Untouchable()
    e = np.array([0.0, 2.5, 1.0, 0.25])
    for bad in (np.array([0.1, 1.0, 0.2, 0.3]), np.array([0.1, -0.01, 0.2, 0.3]), np.array([0.1, np.nan, 0.2, 0.3]), np.array([0.1, 1.5, 0.2, 0.3])):
        with pytest.raises(ValueError, match=r"reflectance must lie in \[0, 1\)"):
            rc.radiosity(accel, e, bad, 3)
    for bad in (np.array([0.0, -1.0, 1.0, 1.0]), np.array([0.0, np.inf, 1.0, 1.0])):
        with pytest.raises(ValueError, match="emission"):
            rc.radiosity(accel, bad, np.full(4, 0.5), 3)
    with pytest.raises(ValueError, match="one value per primitive"):
        rc.radiosity(accel, e, np.full(3, 0.5), 3)
    # the scale leaves the headroom 1 / (1 - max rho) below 2^32
    rho = np.array([0.0, 0.5, 0.75, 0.25])
    scale, e_q, rho_q = rc.radiosity_scale(e, rho)
    assert np.array_equal(rho_q, [0, 32768, 49152, 16384])
    assert scale == ((1 << 32) - 1) * 0.25 / 2.5
    assert np.array_equal(e_q, np.floor(e * scale).astype(np.int64)) and int(e_q.max()) * 4 <= (1 << 32) - 1
    assert rc.radiosity_scale(np.zeros(4), rho)[0] == 1.0
