"""CPU-side checks of the gated TLAS rebuild (rc_tlas_cost_device, rc_refit_or_rebuild_tlas_device_async, rc_tlas_quality): the bindings
match the header's prototypes, the library exports them, the Python and Julia layers carry them, and the argument checks that need no
device come first."""
import ctypes as C
import inspect
import os
import re

import pytest

from api_kit import ROOT, header, julia_text, prototype
from api_kit import rc  # noqa: F401

PROTOS = {
    "rc_tlas_cost_device": (["rc_scene*", "double*", "void*"], [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rc_refit_or_rebuild_tlas_device_async": (["rc_scene*", "double", "void*"], [C.c_void_p, C.c_double, C.c_void_p]),
    "rc_tlas_quality": (["rc_scene*", "rc_tlas_quality_info*"], [C.c_void_p, C.c_void_p]),
}
RC_ERR_INVALID_ARGUMENT, RC_ERR_NO_DEVICE = 1, 3


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_symbol_matches_the_header(rc, name):
    c_args, ctypes_args = PROTOS[name]
    assert prototype(name) == c_args
    bound = {n: (res, args) for n, res, args in rc.SYMBOLS}
    assert name in bound, f"{name} is missing from SYMBOLS"
    res, args = bound[name]
    assert res is C.c_int and args == ctypes_args
    assert hasattr(rc.lib(), name)


def test_quality_struct_matches_the_header(rc):
    from raycore_jl_amd import _capi
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"typedef struct rc_tlas_quality_info \{(.*?)\} rc_tlas_quality_info;", text, flags=re.S)
    assert m
    fields = []
    for decl in m.group(1).split(";"):
        parts = decl.replace(",", " ").split()
        fields += [(name, parts[0]) for name in parts[1:]]
    assert fields == [("cost", "double"), ("cost_built", "double"), ("evaluations", "uint32_t"), ("rebuilds", "uint32_t"),
                      ("last_rebuilt", "uint32_t"), ("armed", "uint32_t")]
    ctype_of = {"double": C.c_double, "uint32_t": C.c_uint32}
    assert [(n, ctype_of[t]) for n, t in fields] == list(_capi.TlasQualityInfo._fields_)
    assert C.sizeof(_capi.TlasQualityInfo) == 32


def test_header_documents_the_calls():
    text = header()
    at = text.index("int rc_tlas_cost_device")
    comment = text[text.rindex("/*", 0, at):at]
    for needle in ("rebuild_bvh!", "cost > ratio * cost_built", "NaN", "same 8 bytes", "floating-point atomics", "ARMS", "capturing stream",
                   "RC_ERR_NOT_SYNCED", "RC_ERR_INVALID_ARGUMENT", "256 instances", "tlas_rebuild_fused", "BEFORE arming does not record"):
        assert needle in comment, needle


def test_python_surface(rc):
    from raycore_jl_amd.wavefront import WavefrontPaths
    assert list(inspect.signature(rc.TLAS.tlas_cost_device).parameters) == ["self", "out", "stream"]
    sig = inspect.signature(rc.TLAS.refit_or_rebuild_device_async)
    assert list(sig.parameters) == ["self", "ratio", "stream"] and sig.parameters["stream"].default is None
    assert list(inspect.signature(rc.TLAS.tlas_quality).parameters) == ["self"]
    p = inspect.signature(WavefrontPaths.__init__).parameters
    assert p["rebuild"].default is False
    assert "no measurement" in WavefrontPaths.__doc__ and 'rebuild="auto"' in WavefrontPaths.__doc__


def test_julia_binding_has_the_methods():
    text = julia_text()
    for name in PROTOS:
        assert ":" + name in text
    assert re.search(r"ccall\(\(:rc_refit_or_rebuild_tlas_device_async, LIB\), Cint, \(Ptr\{Cvoid\}, Cdouble, Ptr\{Cvoid\}\)", text)
    for doc in ("INTEGRATION.md",):
        body = open(os.path.join(ROOT, doc)).read()
        for name in PROTOS:
            assert name in body, (doc, name)


def test_arguments_are_refused_before_the_library_needs_a_device(rc):
    """NULL scene -> RC_ERR_INVALID_ARGUMENT with or without a GPU; a bad ratio is refused by the C entry point before it looks at the scene's
    state and by the Python method before it calls the library at all."""
    L = rc.lib()
    assert L.rc_tlas_cost_device(None, None, None) == RC_ERR_INVALID_ARGUMENT
    assert L.rc_refit_or_rebuild_tlas_device_async(None, 1.5, None) == RC_ERR_INVALID_ARGUMENT
    assert L.rc_tlas_quality(None, None) == RC_ERR_INVALID_ARGUMENT

    class NoLibrary:  # a TLAS whose handle must never reach the library
        device = 0

        @property
        def _h(self):
            raise AssertionError("the library was called")

    for bad in (float("nan"), 0.0, -1.0, float("inf")):
        with pytest.raises(rc.RaycoreError) as e:
            rc.TLAS.refit_or_rebuild_device_async(NoLibrary(), bad)
        assert e.value.code == RC_ERR_INVALID_ARGUMENT
    from raycore_jl_amd.wavefront import WavefrontPaths
    for kw in ({"rebuild": "auto"}, {"rebuild": "sometimes", "dynamic": [(None, None)]}, {"rebuild": ("auto", 2.0), "dynamic": [(None, None)]}):
        with pytest.raises(ValueError):
            WavefrontPaths(None, 8, 8, 1, 1, {}, light=[0, 0, 0], **kw)
    if rc.device_count() == 0:
        with pytest.raises(rc.RaycoreError) as e:
            rc.TLAS(0).refit_or_rebuild_device_async(1.5)
        assert e.value.code == RC_ERR_NO_DEVICE
