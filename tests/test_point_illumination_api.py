"""CPU-side checks of the point-source illumination calls (rc_point_source_rays_device, rc_get_illumination_points_device): the bindings
match the header's prototypes, the library exports them, the header states their contract, the Python and Julia layers carry them, and
get_illumination_points validates its arguments before it touches a device."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

from api_kit import ROOT, header, julia_text
from api_kit import rc  # noqa: F401

C_TO_CTYPES = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
PROTOTYPES = {"rc_point_source_rays_device": ["rc_scene*", "const rc_ray*", "uint32_t", "uint32_t", "uint64_t", "uint32_t", "rc_ray*", "void*"],
              "rc_get_illumination_points_device": ["rc_scene*", "const rc_ray*", "uint32_t", "uint32_t", "uint64_t", "uint32_t", "uint32_t*", "uint64_t",
                                                    "uint32_t*", "void*"]}
JULIA_TYPES = {"rc_point_source_rays_device": ["Ptr{Cvoid}", "Ptr{RTRay}", "UInt32", "UInt32", "UInt64", "UInt32", "Ptr{RTRay}", "Ptr{Cvoid}"],
               "rc_get_illumination_points_device": ["Ptr{Cvoid}", "Ptr{RTRay}", "UInt32", "UInt32", "UInt64", "UInt32", "Ptr{UInt32}", "UInt64", "Ptr{UInt32}",
                                                     "Ptr{Cvoid}"]}


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_symbol_matches_the_header(rc, name):
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in the header"
    assert [" ".join(a.split()[:-1]) for a in m.group(1).split(",")] == PROTOTYPES[name]
    bound = {n: (res, args) for n, res, args in rc.SYMBOLS}
    assert name in bound, f"{name} is missing from SYMBOLS"
    res, args = bound[name]
    assert res is C.c_int and args == [C_TO_CTYPES.get(a, C.c_void_p) for a in PROTOTYPES[name]]
    assert hasattr(rc.lib(), name)


def test_header_documents_the_calls():
    """The comment in front of the declarations cites the reference call it extends, says what a count means physically, and states the
    definition bit for bit, the outputs, the grouping, the capture rules and the error contract."""
    text = header()
    at = text.index("int rc_point_source_rays_device(")
    comment = text[text.rindex("/*", 0, at):at]
    for needle in ("src/kernels.jl:112-124", "solid angle over 4 pi", "form factor", "1 / r^2", "no float in the kernel", "ISOTROPIC", "LAMBERTIAN",
                   "either sign of zero", "(cell, first_source + k, 0, 0x50530000)", "Philox4x32-10", "(word >> 8) * 2^-24", "cell = a * grid + b",
                   "u1 = ((float)a + xi1) / (float)grid", "z = 1 - 2 * u1", "sqrtf(fmaxf(0, 1 - z * z))", "(2 * 3.1415927f) * u2", "not renormalised",
                   "rc_bounce_rays_device", "no contraction", "k * grid^2 + cell", "WHEN THE KERNEL RUNS", "ACCUMULATE", "the caller zeroes",
                   "row_stride >= n_prims", "src/kernels.jl:123", "may be NULL", "row sum + escaped + dropped = grid^2", "illum_scratch_bytes",
                   "changes no result", "capturing stream", "rc_update_geometry_device_async", "CURRENT d_sources", "nothing enqueued",
                   "RC_ERR_INVALID_ARGUMENT", "grid >= 65536", "first_source + n_sources > 2^32", "RC_ERR_NOT_SYNCED", "rc_wait",
                   'docs/EXPERIMENTS.md, "Illumination from point sources"'):
        assert needle in comment, needle
    assert "int rc_get_illumination_points_device(" in text[at:]
    # the header still ends with the ambient-occlusion pair (tests/test_ao_api.py): the new block sits in front of it
    assert text.index("int rc_get_illumination_points_device(") < text.index("int rc_ambient_occlusion_rays_device(")


def test_python_surface(rc):
    sig = inspect.signature(rc.TLAS.point_source_rays_device)
    assert list(sig.parameters) == ["self", "d_sources", "n_sources", "grid", "d_rays", "seed", "first_source", "stream"]
    sig = inspect.signature(rc.TLAS.illumination_points_device)
    assert list(sig.parameters) == ["self", "d_sources", "n_sources", "grid", "d_counts", "row_stride", "d_escaped", "seed", "first_source", "stream"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["row_stride"], d["d_escaped"], d["seed"], d["first_source"], d["stream"]) == (None, None, 0, 0, None)
    sig = inspect.signature(rc.get_illumination_points)
    assert list(sig.parameters) == ["accel", "points", "grid_size", "axes", "max_dist", "weights", "seed", "return_escaped"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["grid_size"], d["axes"], d["max_dist"], d["weights"], d["seed"], d["return_escaped"]) == (256, None, math.inf, None, 0, False)
    assert "solid angle over 4 pi" in rc.get_illumination_points.__doc__ and "form factor" in rc.get_illumination_points.__doc__


def test_julia_binding_and_documents():
    text = julia_text()
    for name, types in JULIA_TYPES.items():
        m = re.search(r"ccall\(\(:" + name + r", LIB\), Cint,\s*\(([^)]*)\)", text)
        assert m, name
        assert [t.strip() for t in m.group(1).split(",")] == types, name
    assert re.search(r"^point_source_rays_device!\(a::MI355XStaticTLAS, d_sources::Ptr\{RTRay\}, n_sources::Integer, grid_size::Integer, d_rays::Ptr\{RTRay\}", text, flags=re.M)
    assert re.search(r"^illumination_points_device!\(a::MI355XStaticTLAS, d_sources::Ptr\{RTRay\}, n_sources::Integer, grid_size::Integer, d_counts::Ptr\{UInt32\}", text, flags=re.M)
    assert re.search(r"^function get_illumination_points\(a::MI355XStaticTLAS, points", text, flags=re.M)
    for doc in ("INTEGRATION.md", "README.md"):
        body = open(os.path.join(ROOT, doc)).read()
        assert "rc_get_illumination_points_device" in body and "rc_point_source_rays_device" in body, doc
    assert "rc_get_illumination_points_device" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## Illumination from point sources" in open(os.path.join(ROOT, "docs", "EXPERIMENTS.md")).read()


def test_null_scene_is_refused_before_anything_else(rc):
    """NULL scene -> RC_ERR_INVALID_ARGUMENT whether or not a GPU is visible (the check comes first), with or without work."""
    f, g = rc.lib().rc_get_illumination_points_device, rc.lib().rc_point_source_rays_device
    assert f(None, None, 0, 0, 0, 0, None, 0, None, None) == 1 and f(None, 64, 3, 8, 1, 0, 64, 16, 64, None) == 1
    assert g(None, None, 0, 0, 0, 0, None, None) == 1 and g(None, 64, 3, 8, 1, 0, 64, None) == 1


class NoDevice:
    """Stands where an accel is expected: any use of it is a failure -- the argument checks come first."""

    def __getattr__(self, name):
        raise AssertionError(f"the accel was touched ({name}) before the arguments were checked")


def test_point_sources_builds_the_records(rc):
    src = rc.point_sources([[1, 2, 3], [4, 5, 6]], axes=[[0, 0, 0], [0, 0, 2]], max_dist=[0.75, np.inf], t_min=0.125)
    assert src.dtype == rc.RAY_DT and src.shape == (2,)
    assert np.array_equal(src["o"], np.array([[1, 2, 3], [4, 5, 6]], np.float32)) and np.array_equal(src["d"], np.array([[0, 0, 0], [0, 0, 2]], np.float32))
    assert np.array_equal(src["tmax"], np.array([0.75, np.inf], np.float32)) and (src["tmin"] == np.float32(0.125)).all()
    src = rc.point_sources(np.zeros((3, 3)))
    assert (src["d"] == 0).all() and (src["tmax"] == np.inf).all() and (src["tmin"] == 0).all()
    assert len(rc.point_sources(np.zeros((0, 3)))) == 0


def test_arguments_are_checked_before_the_device_is_touched(rc):
    acc = NoDevice()
    pts = np.array([[0, 0, 1], [1, 0, 0]], np.float32)
    for bad in (np.zeros(3, np.float32), np.zeros((2, 4), np.float32), np.zeros((2, 3, 1), np.float32)):
        with pytest.raises(ValueError, match=r"\(S, 3\)"):
            rc.get_illumination_points(acc, bad, 8)
    for bad in (np.array([[0, 0, np.nan]]), np.array([[np.inf, 0, 0]])):
        with pytest.raises(ValueError, match="points must be finite"):
            rc.get_illumination_points(acc, bad, 8)
    for bad in (np.zeros((3, 3)), np.zeros(3), np.zeros((2, 2))):
        with pytest.raises(ValueError, match="axes"):
            rc.get_illumination_points(acc, pts, 8, axes=bad)
    with pytest.raises(ValueError, match="axes must be finite"):
        rc.get_illumination_points(acc, pts, 8, axes=np.array([[0, 0, 1], [np.nan, 0, 0]]))
    for bad in (0.0, -1.0, -math.inf, math.nan, [1.0, 0.0], [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError, match="max_dist"):
            rc.get_illumination_points(acc, pts, 8, max_dist=bad)
    for bad in (-1, 65536, 1 << 40, 2.5, True, None):
        with pytest.raises(ValueError, match="grid_size"):
            rc.get_illumination_points(acc, pts, bad)
    for bad in (-1, 1 << 64, 0.5, True):
        with pytest.raises(ValueError, match="seed"):
            rc.get_illumination_points(acc, pts, 8, seed=bad)
    for bad in (np.ones(3), np.ones(1), np.ones((2, 1)), 1.0):
        with pytest.raises(ValueError, match="weights"):
            rc.get_illumination_points(acc, pts, 8, weights=bad)
    with pytest.raises(ValueError, match="weights"):
        rc.get_illumination_points(acc, pts, 0, weights=np.ones(2))
