"""CPU-side checks of the device-side TLAS rebuild (rc_rebuild_tlas_device_async): the binding matches the header's prototype, the library
exports it, the Python and Julia layers carry it, and without a GPU it sits behind the same argument checks as everything else."""
import ctypes as C
import inspect
import re

import pytest

from api_kit import header, julia_text, prototype
from api_kit import rc  # noqa: F401

NAME = "rc_rebuild_tlas_device_async"
C_ARGS = ["rc_scene*", "void*"]
C_TO_CTYPES = {"rc_scene*": C.c_void_p, "void*": C.c_void_p}


def test_symbol_matches_the_header(rc):
    assert prototype(NAME) == C_ARGS
    bound = {n: (res, args) for n, res, args in rc.SYMBOLS}
    assert NAME in bound, f"{NAME} is missing from SYMBOLS"
    res, args = bound[NAME]
    assert res is C.c_int
    assert args == [C_TO_CTYPES[a] for a in C_ARGS]


def test_library_exports_the_symbol(rc):
    assert hasattr(rc.lib(), NAME)


def test_header_documents_the_call():
    """The comment in front of the declaration cites the reference's rebuild and states the bound of the single-workgroup path."""
    text = header()
    at = text.index("int " + NAME)
    comment = text[text.rindex("/*", 0, at):at]
    for needle in ("rebuild_bvh!", "build_tlas_topology", "256 instances", "tlas_rebuild_fused", "RC_ERR_NOT_SYNCED", "capturing stream"):
        assert needle in comment, needle


def test_python_surface(rc):
    from raycore_jl_amd.wavefront import WavefrontPaths
    sig = inspect.signature(rc.TLAS.rebuild_device_async)
    assert list(sig.parameters) == ["self", "stream"]
    assert sig.parameters["stream"].default is None
    p = inspect.signature(WavefrontPaths.__init__).parameters
    assert "rebuild" in p and p["rebuild"].default is False
    assert "dynamic" in p and p["dynamic"].default is None  # (unchanged)


def test_julia_binding_has_the_method(rc):
    text = julia_text()
    assert ":" + NAME in text
    assert re.search(r"Raycore\.rebuild_bvh!\(t::MI355XTLAS, stream::Ptr\{Cvoid\}\)", text)


def test_null_scene_is_refused_before_anything_else(rc):
    """NULL scene -> RC_ERR_INVALID_ARGUMENT whether or not a GPU is visible (the check comes first); with none visible a scene cannot
    exist, so the method is unreachable otherwise."""
    assert rc.lib().rc_rebuild_tlas_device_async(None, None) == 1  # RC_ERR_INVALID_ARGUMENT
    if rc.device_count() == 0:
        with pytest.raises(rc.RaycoreError) as e:
            rc.TLAS(0).rebuild_device_async()
        assert e.value.code == 3  # RC_ERR_NO_DEVICE
