"""CPU-side checks of the device-side animation interface (rc_update_transforms_device, rc_refit_device_async): the binding matches the
header's prototypes, the wavefront frame takes `dynamic`, and without a GPU the new methods sit behind RC_ERR_NO_DEVICE like everything else."""
import ctypes as C
import inspect
import re

import pytest

from api_kit import julia_text, prototype
from api_kit import rc  # noqa: F401

C_TO_CTYPES = {"rc_scene*": C.c_void_p, "uint32_t": C.c_uint32, "const float*": C.c_void_p, "void*": C.c_void_p}


@pytest.mark.parametrize("name, c_args", [
    ("rc_update_transforms_device", ["rc_scene*", "uint32_t", "const float*", "uint32_t", "void*"]),
    ("rc_refit_device_async", ["rc_scene*", "void*"]),
])
def test_symbols_match_the_header(rc, name, c_args):
    assert prototype(name) == c_args
    bound = {n: (res, args) for n, res, args in rc.SYMBOLS}
    assert name in bound, f"{name} is missing from SYMBOLS"
    res, args = bound[name]
    assert res is C.c_int
    assert args == [C_TO_CTYPES[a] for a in c_args]
    assert hasattr(rc.lib(), name)


def test_python_surface(rc):
    from raycore_jl_amd.wavefront import WavefrontPaths
    p = inspect.signature(WavefrontPaths.__init__).parameters
    assert "dynamic" in p and p["dynamic"].default is None
    for method, params in (("update_transforms_device", ["self", "handle", "d_xforms", "stream"]), ("refit_device_async", ["self", "stream"])):
        sig = inspect.signature(getattr(rc.TLAS, method))
        assert list(sig.parameters) == params
        assert sig.parameters["stream"].default is None


def test_julia_binding_has_the_device_method(rc):
    text = julia_text()
    assert re.search(r"function Raycore\.update_transforms!\(t::MI355XTLAS, h::TLASHandle, d_transforms::Ptr\{Float32\}", text)
    assert ":rc_update_transforms_device" in text and ":rc_refit_device_async" in text


def test_no_device_no_fallback(rc):
    if rc.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(rc.RaycoreError) as e:  # a scene cannot exist without a GPU, so the new methods are unreachable
        rc.TLAS(0).refit_device_async()
    assert e.value.code == 3  # RC_ERR_NO_DEVICE
    L = rc.lib()
    assert L.rc_update_transforms_device(None, 1, None, 0, None) == 1  # RC_ERR_INVALID_ARGUMENT: NULL scene, checked before anything else
    assert L.rc_refit_device_async(None, None) == 1
