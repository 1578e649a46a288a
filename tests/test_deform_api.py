"""CPU-side checks of the device-side geometry update (rc_update_geometry_device_async, rc_update_mesh_vertices_device_async): the
bindings match the header's prototypes, the library exports them, the Python and Julia layers carry them, and without a GPU they sit behind
the same argument checks as everything else."""
import ctypes as C
import inspect
import re

import pytest

from api_kit import header, julia_text, prototype
from api_kit import rc  # noqa: F401

C_TO_CTYPES = {"rc_scene*": C.c_void_p, "void*": C.c_void_p, "const float*": C.c_void_p, "const uint32_t*": C.c_void_p, "uint32_t": C.c_uint32}
CALLS = {
    "rc_update_geometry_device_async": ["rc_scene*", "uint32_t", "const float*", "const uint32_t*", "uint32_t", "void*"],
    "rc_update_mesh_vertices_device_async": ["rc_scene*", "uint32_t", "const float*", "const float*", "uint32_t", "void*"],
}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_symbol_matches_the_header(rc, name):
    assert prototype(name) == CALLS[name]
    bound = {n: (res, args) for n, res, args in rc.SYMBOLS}
    assert name in bound, f"{name} is missing from SYMBOLS"
    res, args = bound[name]
    assert res is C.c_int
    assert args == [C_TO_CTYPES[a] for a in CALLS[name]]


@pytest.mark.parametrize("name", sorted(CALLS))
def test_library_exports_the_symbol(rc, name):
    assert hasattr(rc.lib(), name)


def test_status_code(rc):
    assert re.search(r"#define\s+RC_ERR_GEOMETRY_CHANGED\s+8\b", header())
    assert rc.RaycoreError.RC_ERR_GEOMETRY_CHANGED == 8


def test_header_documents_the_calls():
    """The comment in front of the declarations cites the reference's update! and build_blas and states the in-place contract."""
    text = header()
    at = text.index("int rc_update_geometry_device_async")
    comment = text[text.rindex("/*", 0, at):at]
    for needle in ("update!", ":808-857", "build_blas", ":1376-1443", "RC_ERR_GEOMETRY_CHANGED", "capturing stream", "n_prims",
                   "rc_update_mesh_vertices_device_async"):
        assert needle in comment, needle


def test_python_surface(rc):
    from raycore_jl_amd.wavefront import WavefrontPaths
    sig = inspect.signature(rc.TLAS.update_geometry_device_async)
    assert list(sig.parameters) == ["self", "handle", "d_verts", "n", "d_meta", "stream"]
    assert all(sig.parameters[k].default is None for k in ("n", "d_meta", "stream"))
    sig = inspect.signature(rc.TLAS.update_mesh_vertices_device_async)
    assert list(sig.parameters) == ["self", "handle", "d_verts", "d_normals", "stream"]
    assert all(sig.parameters[k].default is None for k in ("d_normals", "stream"))
    p = inspect.signature(WavefrontPaths.__init__).parameters
    assert "deform" in p and p["deform"].default is None
    assert p["dynamic"].default is None and p["rebuild"].default is False  # (unchanged)


def test_julia_binding_has_the_methods(rc):
    text = julia_text()
    for name in CALLS:
        assert ":" + name in text
    assert re.search(r"Raycore\.update!\(t::MI355XTLAS, h(andle)?(::TLASHandle)?, d_verts::Ptr\{Cfloat\}, n(::Integer)?, stream::Ptr\{Cvoid\}", text)


def test_null_scene_is_refused_before_anything_else(rc):
    """NULL scene -> RC_ERR_INVALID_ARGUMENT whether or not a GPU is visible (the check comes first); with none visible a scene cannot
    exist, so the methods are unreachable otherwise."""
    assert rc.lib().rc_update_geometry_device_async(None, 1, None, None, 0, None) == 1  # RC_ERR_INVALID_ARGUMENT
    assert rc.lib().rc_update_mesh_vertices_device_async(None, 1, None, None, 0, None) == 1
    if rc.device_count() == 0:
        with pytest.raises(rc.RaycoreError) as e:
            rc.TLAS(0)
        assert e.value.code == 3  # RC_ERR_NO_DEVICE
