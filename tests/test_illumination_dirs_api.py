"""CPU-side checks of the many-direction illumination calls (rc_get_illumination_dirs_device, rc_generate_ray_grid_dirs_device): the
bindings match the header's prototypes, the library exports them, the header states their contract behind rc_recent_kernel_ms, the Python
and Julia layers carry them, and get_illumination_dirs validates its arguments before it touches a device."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from api_kit import header, julia_text, prototype
from api_kit import rc  # noqa: F401

C_TO_CTYPES = {"rc_scene*": C.c_void_p, "void*": C.c_void_p, "const float*": C.c_void_p, "uint32_t*": C.c_void_p, "rc_ray*": C.c_void_p,
               "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
PROTOTYPES = {"rc_get_illumination_dirs_device": ["rc_scene*", "const float*", "uint32_t", "uint32_t", "uint32_t*", "uint64_t", "void*"],
              "rc_generate_ray_grid_dirs_device": ["rc_scene*", "const float*", "uint32_t", "uint32_t", "rc_ray*", "void*"]}
JULIA_TYPES = {"rc_get_illumination_dirs_device": ["Ptr{Cvoid}", "Ptr{Float32}", "UInt32", "UInt32", "Ptr{UInt32}", "UInt64", "Ptr{Cvoid}"],
               "rc_generate_ray_grid_dirs_device": ["Ptr{Cvoid}", "Ptr{Float32}", "UInt32", "UInt32", "Ptr{RTRay}", "Ptr{Cvoid}"]}


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_symbol_matches_the_header(rc, name):
    assert prototype(name) == PROTOTYPES[name]
    bound = {n: (res, args) for n, res, args in rc.SYMBOLS}
    assert name in bound, f"{name} is missing from SYMBOLS"
    res, args = bound[name]
    assert res is C.c_int
    assert args == [C_TO_CTYPES[a] for a in PROTOTYPES[name]]


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_library_exports_the_symbol(rc, name):
    assert hasattr(rc.lib(), name)


def test_declarations_sit_behind_rc_recent_kernel_ms():
    """Appended at the end: the header lines other tests cite by number do not move."""
    text = header()
    last = text.index("int rc_recent_kernel_ms(")
    for name in PROTOTYPES:
        assert text.index("int " + name + "(") > last, name
    before = text[:last].count("\n")
    assert before >= 725


def test_header_documents_the_calls():
    """The comment in front of the declarations cites the reference, states the work-item layout, when the inputs are read, the accumulate
    rule, the integer counts, the error contract, and that the calls are the exception to the stale-world-bound rule."""
    text = header()
    at = text.index("int rc_get_illumination_dirs_device(")
    comment = text[text.rindex("/*", 0, at):at]
    for needle in ("src/kernels.jl:10-72,112-124", "d * grid^2 + cell", "KERNEL RUNS", "ACCUMULATES", "u32", "f32", "2^24", "row_stride",
                   "stale world bound", "rc_refit_device_async", "EXCEPTION", "capturing stream", "illum_scratch_bytes", "RC_ERR_INVALID_ARGUMENT",
                   "RC_ERR_NOT_SYNCED", "nothing enqueued", "rc_generate_ray_grid_device", "rc_wait"):
        assert needle in comment, needle
    assert "int rc_generate_ray_grid_dirs_device(" in text[at:]


def test_python_surface(rc):
    sig = inspect.signature(rc.TLAS.illumination_dirs_device)
    assert list(sig.parameters) == ["self", "d_dirs", "n_dirs", "grid", "d_counts", "row_stride", "stream"]
    assert sig.parameters["row_stride"].default is None and sig.parameters["stream"].default is None
    sig = inspect.signature(rc.TLAS.ray_grid_dirs_device)
    assert list(sig.parameters) == ["self", "d_dirs", "n_dirs", "grid", "d_rays", "stream"]
    assert sig.parameters["stream"].default is None
    sig = inspect.signature(rc.get_illumination_dirs)
    assert list(sig.parameters) == ["accel", "viewdirs", "grid_size", "weights"]
    assert sig.parameters["grid_size"].default == 1000 and sig.parameters["weights"].default is None


def test_julia_binding_has_the_methods():
    text = julia_text()
    for name, types in JULIA_TYPES.items():
        m = re.search(r"ccall\(\(:" + name + r", LIB\), Cint,\s*\(([^)]*)\)", text)
        assert m, name
        assert [t.strip() for t in m.group(1).split(",")] == types, name
    assert re.search(r"illumination_dirs_device!\(a::MI355XStaticTLAS, d_dirs::Ptr\{Float32\}, n_dirs::Integer, grid_size::Integer, d_counts::Ptr\{UInt32\}", text)
    assert re.search(r"ray_grid_dirs_device!\(a::MI355XStaticTLAS, d_dirs::Ptr\{Float32\}, n_dirs::Integer, grid_size::Integer, d_rays::Ptr\{RTRay\}", text)
    assert re.search(r"function get_illumination_dirs\(a::MI355XStaticTLAS, viewdirs", text)


def test_null_scene_is_refused_before_anything_else(rc):
    """NULL scene -> RC_ERR_INVALID_ARGUMENT whether or not a GPU is visible (the check comes first), with or without work."""
    f, g = rc.lib().rc_get_illumination_dirs_device, rc.lib().rc_generate_ray_grid_dirs_device
    assert f(None, None, 0, 0, None, 0, None) == 1 and f(None, 64, 3, 8, 64, 16, None) == 1  # RC_ERR_INVALID_ARGUMENT
    assert g(None, None, 0, 0, None, None) == 1 and g(None, 64, 3, 8, 64, None) == 1


def test_arguments_are_checked_before_the_device_is_touched(rc):
    """Every refusal below comes before the accel is looked at: it is None."""
    for bad in (np.zeros(3, np.float32), np.zeros((2, 4), np.float32), np.zeros((2, 3, 1), np.float32)):
        with pytest.raises(ValueError, match=r"\(D, 3\)"):
            rc.get_illumination_dirs(None, bad, 8)
    dirs = np.array([[0, 0, 1], [1, 0, 0]], np.float32)
    for bad in (np.ones(3), np.ones(1), np.ones((2, 1)), 1.0):
        with pytest.raises(ValueError, match="weights"):
            rc.get_illumination_dirs(None, dirs, 8, weights=bad)
