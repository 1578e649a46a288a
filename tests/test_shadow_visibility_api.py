"""CPU-side checks of the fused shadow-visibility query (rc_shadow_visibility_device): the binding matches the header's prototype, the
library exports it, the Python and Julia layers carry it, WavefrontPaths validates its new arguments before it touches a device, and
without a GPU the call sits behind the same argument checks as everything else."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from api_kit import header, julia_text, prototype
from api_kit import rc  # noqa: F401

NAME = "rc_shadow_visibility_device"
C_TO_CTYPES = {"rc_scene*": C.c_void_p, "void*": C.c_void_p, "const rc_ray*": C.c_void_p, "const rc_hit*": C.c_void_p, "const float*": C.c_void_p,
               "uint8_t*": C.c_void_p, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}
ARGS = ["rc_scene*", "const rc_ray*", "const rc_hit*", "uint64_t", "const float*", "uint32_t", "float", "uint8_t*", "void*"]


def test_symbol_matches_the_header(rc):
    assert prototype(NAME) == ARGS
    bound = {n: (res, args) for n, res, args in rc.SYMBOLS}
    assert NAME in bound, f"{NAME} is missing from SYMBOLS"
    res, args = bound[NAME]
    assert res is C.c_int
    assert args == [C_TO_CTYPES[a] for a in ARGS]


def test_library_exports_the_symbol(rc):
    assert hasattr(rc.lib(), NAME)


def test_header_documents_the_call():
    """The comment in front of the declaration cites the reference's three kernels, names the layout and states the identity with the
    composed path and the error contract."""
    text = header()
    at = text.index("int " + NAME)
    comment = text[text.rindex("/*", 0, at):at]
    for needle in ("generate_shadow_rays!", ":279-333", "test_shadow_rays!", ":340-362", ":395-416", "i * n_lights + l", "rc_shadow_rays_device",
                   "rc_trace_any_device", "KERNEL RUNS", "entry_cull", "2^32", "RC_ERR_INVALID_ARGUMENT", "RC_ERR_NOT_SYNCED", "rc_wait"):
        assert needle in comment, needle


def test_python_surface(rc):
    from raycore_jl_amd.wavefront import WavefrontPaths
    sig = inspect.signature(rc.TLAS.shadow_visibility_device)
    assert list(sig.parameters) == ["self", "d_rays", "d_hits", "n", "d_lights", "n_lights", "d_visible", "bias", "stream"]
    assert sig.parameters["stream"].default is None
    p = inspect.signature(WavefrontPaths.__init__).parameters
    assert p["lights"].default is None and p["fused_shadows"].default is False
    assert list(p)[:7] == ["self", "accel", "width", "height", "samples", "depth", "camera"] and list(p)[7] == "light"  # (positions unchanged)
    assert p["dynamic"].default is None and p["rebuild"].default is False and p["deform"].default is None and p["compact"].default is True


def test_julia_binding_has_the_method(rc):
    text = julia_text()
    assert ":" + NAME in text
    m = re.search(r"ccall\(\(:" + NAME + r", LIB\), Cint,\s*\(([^)]*)\)", text)
    assert m
    assert [t.strip() for t in m.group(1).split(",")] == ["Ptr{Cvoid}", "Ptr{RTRay}", "Ptr{RTHitResult}", "UInt64", "Ptr{Float32}", "UInt32", "Cfloat",
                                                          "Ptr{UInt8}", "Ptr{Cvoid}"]
    assert re.search(r"shadow_visibility_device!\(a::MI355XStaticTLAS, d_rays::Ptr\{RTRay\}, d_hits::Ptr\{RTHitResult\}, n::Integer, d_lights::Ptr\{Float32\}", text)


def test_null_scene_is_refused_before_anything_else(rc):
    """NULL scene -> RC_ERR_INVALID_ARGUMENT whether or not a GPU is visible (the check comes first), with or without work."""
    f = rc.lib().rc_shadow_visibility_device
    assert f(None, None, None, 0, None, 0, 1e-3, None, None) == 1  # RC_ERR_INVALID_ARGUMENT
    assert f(None, 64, 64, 16, 64, 4, 1e-3, 64, None) == 1
    if rc.device_count() == 0:
        with pytest.raises(rc.RaycoreError) as e:
            rc.TLAS(0)
        assert e.value.code == 3  # RC_ERR_NO_DEVICE


CAMERA = {"pos": (0, 0, 5), "right": (1, 0, 0), "up": (0, 1, 0), "forward": (0, 0, -1), "half_width": 0.5, "half_height": 0.5}
LIGHTS = np.array([[10, 10, 10], [-4, 6, 3]], np.float32)


def test_wavefront_arguments_are_checked_before_the_device_is_touched():
    """Every refusal below comes before the first tensor is made: accel is None."""
    from raycore_jl_amd.wavefront import WavefrontPaths
    with pytest.raises(ValueError, match="fused_shadows"):  # no silent loop over the lights
        WavefrontPaths(None, 8, 8, 1, 1, CAMERA, (1, 2, 3), lights=LIGHTS)
    with pytest.raises(ValueError, match="fused_shadows"):
        WavefrontPaths(None, 8, 8, 1, 1, CAMERA, lights=LIGHTS)
    with pytest.raises(ValueError, match="lights"):
        WavefrontPaths(None, 8, 8, 1, 1, CAMERA, (1, 2, 3), fused_shadows=True)
    with pytest.raises(ValueError, match="light"):
        WavefrontPaths(None, 8, 8, 1, 1, CAMERA)
    for bad in (np.zeros(3, np.float32), np.zeros((2, 4), np.float32), np.zeros((0, 3), np.float32)):
        with pytest.raises(ValueError, match=r"\(L, 3\)"):
            WavefrontPaths(None, 8, 8, 1, 1, CAMERA, lights=bad, fused_shadows=True)
    with pytest.raises(ValueError, match="2\\^32"):  # n * L must fit the launch's 32-bit item index
        WavefrontPaths(None, 1 << 15, 1 << 15, 1, 1, CAMERA, lights=np.zeros((4, 3), np.float32), fused_shadows=True)
    with pytest.raises(ValueError, match="depth"):  # (unchanged)
        WavefrontPaths(None, 8, 8, 1, 0, CAMERA, (1, 2, 3))
