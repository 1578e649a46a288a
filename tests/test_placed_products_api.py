"""CPU-side checks of the placed products (rc_placed_view_factor_products_device) and of the Python layer on top of it: the binding
matches the header's prototype, the library exports it, the option is bound, the Julia layer and the documents carry it, and every
argument error of placed_view_factor_products / _totals / _bounces / placed_radiosity is raised before a device is touched -- with lengths
counted in PLACED primitives."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from api_kit import ROOT, header, julia_text, prototype
from api_kit import rc  # noqa: F401

NAME = "rc_placed_view_factor_products_device"
PROTOTYPE = ["rc_scene*", "uint32_t", "uint64_t", "uint32_t", "uint32_t", "uint32_t", "uint32_t", "uint32_t", "const uint32_t*", "uint64_t*", "uint64_t*",
             "uint64_t*", "void*"]
JL_ARGS = ["Ptr{Cvoid}", "UInt32", "UInt64", "UInt32", "UInt32", "UInt32", "UInt32", "UInt32", "Ptr{UInt32}", "Ptr{UInt64}", "Ptr{UInt64}", "Ptr{UInt64}",
           "Ptr{Cvoid}"]
CTYPES = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
RC_ERR_INVALID_ARGUMENT = 1


def test_symbol_matches_the_header(rc):
    assert prototype(NAME) == PROTOTYPE
    res, args = {n: (r, a) for n, r, a in rc.SYMBOLS}[NAME]
    assert res is C.c_int and args == [CTYPES.get(a, C.c_void_p) for a in PROTOTYPE]
    assert hasattr(rc.lib(), NAME)


def test_header_documents_the_call():
    text = header()
    at = text.index("int " + NAME)
    comment = " ".join(text[text.rindex("/* ----", 0, at):at].replace("\n *", " ").split())
    for needle in ("Radiosity between instances", "q = base[i] + l", "bit for bit those of rc_placed_view_factor_rays_device", "estimates the Lambertian form factor F_ab",
                   "with no metadata in it", "Item w = placed primitive placed_begin + w / n_ray", "a = the source's q",
                   "b = base[hit instance] + prim - 1", "mx [a] += x[b]", "mtx[b] += x[a]", "A miss: escaped[a] += 1", "A hit on the source itself adds nothing",
                   "u64 modulo 2^64", "any partition of placed primitives x rays gives the same words", "d_x == NULL means x = 1", "read WHEN THE KERNEL RUNS",
                   "every one may be NULL", "ACCUMULATE", "placed_end is clamped to P and ray_end to rays_per_triangle",
                   "an empty range, or all three outputs NULL, enqueues nothing", '"placed_copy_bytes"', "default 256 MiB", "the same words either way",
                   "Scratch is per stream", "has run the call eagerly once", "rc_update_transforms_device -> rc_refit_device_async",
                   "rc_update_geometry_device_async", "P >= 2^32", "RC_ERR_NOT_SYNCED in the states in which rc_placed_view_factor_groups_device returns it",
                   "A stack overflow is reported by rc_wait", 'docs/EXPERIMENTS.md, "Radiosity between instances"'):
        assert needle in comment, needle
    assert "the products, the sparse matrix and the bounce solve do not exist yet" not in text
    assert '"placed_copy_bytes" (rc_placed_view_factor_products_device' in text


def test_python_surface(rc):
    sig = inspect.signature(rc.TLAS.placed_view_factor_products_device)
    assert list(sig.parameters) == ["self", "x_ptr", "mx_ptr", "mtx_ptr", "rays_per_triangle", "seed", "sampling", "escaped_ptr", "placed", "rays", "stream"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["sampling"], d["escaped_ptr"], d["placed"], d["rays"], d["stream"]) == ("uniform", None, None, None, None)
    sig = inspect.signature(rc.placed_view_factor_products)
    assert list(sig.parameters) == ["accel", "x", "rays_per_triangle", "seed", "sampling", "return_escaped"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["rays_per_triangle"], d["seed"], d["sampling"], d["return_escaped"]) == (10000, 0, "uniform", False)
    sig = inspect.signature(rc.placed_view_factor_totals)
    assert list(sig.parameters) == ["accel", "rays_per_triangle", "seed", "sampling"] and sig.parameters["sampling"].default == "uniform"
    sig = inspect.signature(rc.placed_view_factor_bounces)
    assert list(sig.parameters) == ["accel", "emission", "reflectance", "bounces", "rays_per_triangle", "seed", "sampling", "stream"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["rays_per_triangle"], d["seed"], d["sampling"], d["stream"]) == (10000, 0, "cosine", None)
    sig = inspect.signature(rc.placed_radiosity)
    d = {k: v.default for k, v in sig.parameters.items()}
    assert list(sig.parameters)[:4] == ["accel", "emission", "reflectance", "bounces"] and (d["sampling"], d["return_scale"]) == ("cosine", False)
    from raycore_jl_amd import api
    assert list(inspect.signature(api.placed_bounce_step).parameters) == ["t", "e", "rho", "x", "x32", "mx", "rays_per_triangle", "seed", "sampling", "stream"]


def test_julia_binding_and_the_documents():
    text = julia_text()
    m = re.search(r"ccall\(\(:" + NAME + r", LIB\), Cint,\s*\(([^)]*)\)", text)
    assert m, f"no ccall of {NAME}"
    assert [t.strip() for t in m.group(1).split(",")] == JL_ARGS
    assert re.search(r"^placed_view_factor_products_device!\(a::MI355XStaticTLAS, rays_per_triangle::Integer, seed::UInt64, sampling::Integer, placed_begin::Integer,", text, flags=re.M)
    for f in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert NAME in open(os.path.join(ROOT, f)).read(), f
    assert '## Radiosity between instances' in open(os.path.join(ROOT, "docs", "EXPERIMENTS.md")).read()


def test_invalid_arguments_are_refused_without_a_device(rc):
    f = rc.lib().rc_placed_view_factor_products_device
    assert f(None, 16, 0, 0, 0, 8, 0, 16, None, 64, 64, 64, None) == RC_ERR_INVALID_ARGUMENT
    assert f(None, 16, 0, 1, 0, 8, 0, 16, 64, None, None, None, None) == RC_ERR_INVALID_ARGUMENT


class NoDevice:
    """Stands where an accel is expected: any use of it is a failure -- the argument checks come first."""

    def __getattr__(self, name):
        raise AssertionError(f"the accel was touched ({name}) before the arguments were checked")


class Bases:
    """Stands where a synced TLAS is expected and answers placed_primitive_bases() only: P = 8 from three instances."""
    device = 0

    def placed_primitive_bases(self):
        return np.array([0, 2, 7, 8], np.uint32)

    def __getattr__(self, name):
        raise AssertionError(f"the accel was touched ({name}) after a length error")


@pytest.fixture()
def fake_owner(rc, monkeypatch):
    from raycore_jl_amd import api
    monkeypatch.setattr(api, "_owner", lambda accel: accel)
    return Bases()


def test_products_and_totals_check_their_arguments_without_a_device(rc):
    acc = NoDevice()
    x = np.arange(8, dtype=np.uint32)
    for bad in (x.astype(np.int64), x.astype(np.float32), x.reshape(2, 4), list(range(8)), None):
        with pytest.raises(ValueError, match="x must be"):
            rc.placed_view_factor_products(acc, bad, 16)
    for bad in ("lambert", "", 2, -1, None, True, 0.0):
        with pytest.raises(ValueError, match="sampling"):
            rc.placed_view_factor_products(acc, x, 16, sampling=bad)
        with pytest.raises(ValueError, match="sampling"):
            rc.placed_view_factor_totals(acc, 16, sampling=bad)
    for bad in (-1, 1 << 32, 1.5, True):
        with pytest.raises(ValueError, match="rays_per_triangle"):
            rc.placed_view_factor_products(acc, x, bad)
        with pytest.raises(ValueError, match="rays_per_triangle"):
            rc.placed_view_factor_totals(acc, bad)
    for bad in (-1, 1 << 64, 0.5):
        with pytest.raises(ValueError, match="seed"):
            rc.placed_view_factor_products(acc, x, 16, seed=bad)
        with pytest.raises(ValueError, match="seed"):
            rc.placed_view_factor_totals(acc, 16, seed=bad)
    no_scene = type("NoScene", (), {"_h": None})()  # the sampling name is refused while the arguments are put together
    with pytest.raises(ValueError, match="sampling"):
        rc.TLAS.placed_view_factor_products_device(no_scene, 64, 64, 64, 16, 0, "lambert")


def test_bounces_and_radiosity_check_their_arguments_without_a_device(rc):
    acc = NoDevice()
    e, rho = np.arange(8, dtype=np.uint32), np.full(8, 32768, np.uint32)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="bounces"):
            rc.placed_view_factor_bounces(acc, e, rho, bad, 16)
    for bad in (0, 1 << 31, 2.5, True):
        with pytest.raises(ValueError, match="rays_per_triangle"):
            rc.placed_view_factor_bounces(acc, e, rho, 2, bad)
    for bad in (np.array([0, -1]), np.array([0, 1 << 32]), e.astype(np.float64), e.reshape(2, 4)):
        with pytest.raises(ValueError, match="emission"):
            rc.placed_view_factor_bounces(acc, bad, rho, 2, 16)
    for bad in (np.full(8, 65537), np.full(8, -1), rho.astype(np.float32)):
        with pytest.raises(ValueError, match="reflectance"):
            rc.placed_view_factor_bounces(acc, e, bad, 2, 16)
    with pytest.raises(ValueError, match="one value per primitive each"):
        rc.placed_view_factor_bounces(acc, e, rho[:5], 2, 16)
    for bad in (-1, 1 << 64, 0.5):
        with pytest.raises(ValueError, match="seed"):
            rc.placed_view_factor_bounces(acc, e, rho, 2, 16, seed=bad)
    for bad in ("lambert", 2, None, True):
        with pytest.raises(ValueError, match="sampling"):
            rc.placed_view_factor_bounces(acc, e, rho, 2, 16, sampling=bad)
        with pytest.raises(ValueError, match="sampling"):
            rc.placed_radiosity(acc, np.ones(8), np.full(8, 0.5), 2, 16, sampling=bad)
    for bad_e, bad_rho, what in ((np.full(8, -1.0), np.full(8, 0.5), "emission"), (np.full(8, np.inf), np.full(8, 0.5), "emission"),
                                 (np.ones(8), np.ones(8), "reflectance"), (np.ones(8), np.full(5, 0.5), "one value per primitive each")):
        with pytest.raises(ValueError, match=what):
            rc.placed_radiosity(acc, bad_e, bad_rho, 2, 16)


def test_lengths_are_counted_in_placed_primitives(rc, fake_owner):
    for n in (3, 7, 9):  # 3 instances, not P = 8
        with pytest.raises(ValueError, match="one value per placed primitive: %d values for 8 placed primitives" % n):
            rc.placed_view_factor_products(fake_owner, np.zeros(n, np.uint32), 16)
        with pytest.raises(ValueError, match="one value per placed primitive: %d values for 8 placed primitives" % n):
            rc.placed_view_factor_bounces(fake_owner, np.zeros(n, np.uint32), np.zeros(n, np.uint32), 2, 16)
        with pytest.raises(ValueError, match="one value per placed primitive: %d values for 8 placed primitives" % n):
            rc.placed_radiosity(fake_owner, np.ones(n), np.full(n, 0.5), 2, 16)
