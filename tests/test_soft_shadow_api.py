"""CPU-side checks of the soft-shadow pair (rc_soft_shadow_rays_device, rc_soft_shadow_visibility_device): the bindings match the header's
prototypes, the library exports them, the header states the identity, the Python and Julia layers carry them, WavefrontPaths validates
its new arguments before it touches a device, and without a GPU the calls sit behind the same argument checks as everything else."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from api_kit import ROOT, header, julia_text, prototype
from api_kit import rc  # noqa: F401

C_TO_CTYPES = {"rc_scene*": C.c_void_p, "void*": C.c_void_p, "const rc_ray*": C.c_void_p, "const rc_hit*": C.c_void_p, "const float*": C.c_void_p,
               "const uint32_t*": C.c_void_p, "rc_ray*": C.c_void_p, "uint32_t*": C.c_void_p, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
               "float": C.c_float}
HEAD = ["rc_scene*", "const rc_ray*", "const rc_hit*", "uint64_t", "const float*", "const float*", "uint32_t", "uint32_t", "uint64_t", "uint32_t",
        "const uint32_t*", "uint64_t", "float"]
ARGS = {"rc_soft_shadow_rays_device": HEAD + ["rc_ray*", "void*"], "rc_soft_shadow_visibility_device": HEAD + ["uint32_t*", "void*"]}
JL_HEAD = ["Ptr{Cvoid}", "Ptr{RTRay}", "Ptr{RTHitResult}", "UInt64", "Ptr{Float32}", "Ptr{Float32}", "UInt32", "UInt32", "UInt64", "UInt32", "Ptr{UInt32}",
           "UInt64", "Cfloat"]
JL_ARGS = {"rc_soft_shadow_rays_device": JL_HEAD + ["Ptr{RTRay}", "Ptr{Cvoid}"], "rc_soft_shadow_visibility_device": JL_HEAD + ["Ptr{UInt32}", "Ptr{Cvoid}"]}
NAMES = sorted(ARGS)


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


@pytest.mark.parametrize("name", NAMES)
def test_header_documents_the_call(name):
    """The comment in front of the declarations cites the reference's lines, states the identity with the composed path, the one-sample
    special case, the Philox counter layout, the t_max convention and the error contract."""
    text = header()
    at = text.index("int " + name)
    comment = text[text.rindex("/*", 0, at):at]
    for needle in ("docs/src/raytracing-core.jl:58-99", ":119-129", ":61-81", ":74-81", ":94", "shadow_factor", "compute_light", "compute_multi_light",
                   "d_count[i * n_lights + l] += sum over s of (d_hits[i].hit && ray(i, l, s).t_max > 0 && !any_hit(ray(i, l, s)).hit)",
                   "bit for bit what rc_soft_shadow_rays_device writes", "no tolerance", "(i * n_lights + l) * samples + s",
                   "samples == 1: target == light", "rc_shadow_visibility_device's byte", "rc_trace_any_device",
                   "(lo32 path, hi32 path, s | depth << 16, 0x53460000 | l)", "Philox4x32-10", "rc_bounce_rays_device", "t_max = Inf",
                   "hit_dist >= shadow_dist", "ACCUMULATES", "KERNEL RUNS", "entry_cull", "2^32", "samples >= 65536", "depth >= 65536",
                   "n_lights >= 65536", "RC_ERR_INVALID_ARGUMENT", "RC_ERR_NOT_SYNCED", "rc_wait", "divides a count by `samples`"):
        assert needle in comment, needle


def test_python_surface(rc):
    from raycore_jl_amd.wavefront import WavefrontPaths
    sig = inspect.signature(rc.TLAS.soft_shadow_visibility_device)
    assert list(sig.parameters) == ["self", "d_rays", "d_hits", "n", "d_lights", "d_radii", "n_lights", "samples", "d_count", "seed", "depth", "bias",
                                    "d_path_in", "path_base", "stream"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["seed"], d["depth"], d["bias"], d["d_path_in"], d["path_base"], d["stream"]) == (0, 0, 0.01, None, 0, None)
    sig = inspect.signature(rc.TLAS.soft_shadow_rays_device)
    assert list(sig.parameters) == ["self", "d_rays", "d_hits", "n", "d_lights", "d_radii", "n_lights", "samples", "d_shadow_rays", "seed", "depth",
                                    "bias", "d_path_in", "path_base", "stream"]
    p = inspect.signature(WavefrontPaths.__init__).parameters
    assert list(p)[-2:] == ["shadow_samples", "light_radii"]  # appended after the existing keyword arguments
    assert list(p)[:-2] == ["self", "accel", "width", "height", "samples", "depth", "camera", "light", "seed", "bias", "compact", "dynamic", "rebuild",
                            "deform", "lights", "fused_shadows"]
    assert p["shadow_samples"].default == 1 and p["light_radii"].default is None


@pytest.mark.parametrize("name", NAMES)
def test_julia_binding_has_the_method(name):
    text = julia_text()
    m = re.search(r"ccall\(\(:" + name + r", LIB\), Cint,\s*\(([^)]*)\)", text)
    assert m, f"no ccall of {name}"
    assert [t.strip() for t in m.group(1).split(",")] == JL_ARGS[name]
    method = name[3:] + "!"
    assert re.search(r"^" + method + r"\(a::MI355XStaticTLAS, d_rays::Ptr\{RTRay\}, d_hits::Ptr\{RTHitResult\}, n::Integer, d_lights::Ptr\{Float32\},\s*"
                     r"d_radii::Ptr\{Float32\}, n_lights::Integer, samples::Integer", text, flags=re.M), method
    assert method in open(os.path.join(ROOT, "INTEGRATION.md")).read()


@pytest.mark.parametrize("name", NAMES)
def test_null_scene_is_refused_before_anything_else(rc, name):
    """NULL scene -> RC_ERR_INVALID_ARGUMENT whether or not a GPU is visible (the check comes first), with or without work."""
    f = getattr(rc.lib(), name)
    assert f(None, None, None, 0, None, None, 0, 0, 0, 0, None, 0, 1e-3, None, None) == 1  # RC_ERR_INVALID_ARGUMENT
    assert f(None, 64, 64, 16, 64, 64, 4, 4, 0, 0, None, 0, 1e-3, 64, None) == 1
    if rc.device_count() == 0:
        with pytest.raises(rc.RaycoreError) as e:
            rc.TLAS(0)
        assert e.value.code == 3  # RC_ERR_NO_DEVICE


CAMERA = {"pos": (0, 0, 5), "right": (1, 0, 0), "up": (0, 1, 0), "forward": (0, 0, -1), "half_width": 0.5, "half_height": 0.5}
LIGHTS = np.array([[10, 10, 10], [-4, 6, 3]], np.float32)
RADII = np.array([1.0, 0.5], np.float32)


def test_wavefront_arguments_are_checked_before_the_device_is_touched():
    """Every refusal below comes before the first tensor is made: accel is None."""
    from raycore_jl_amd.wavefront import WavefrontPaths
    with pytest.raises(ValueError, match="fused_shadows"):  # soft shadows are the fused launch only
        WavefrontPaths(None, 8, 8, 1, 1, CAMERA, (1, 2, 3), shadow_samples=4, light_radii=RADII)
    with pytest.raises(ValueError, match="light_radii"):
        WavefrontPaths(None, 8, 8, 1, 1, CAMERA, lights=LIGHTS, fused_shadows=True, shadow_samples=4)
    for bad in (np.zeros(3, np.float32), np.zeros((2, 1), np.float32), np.float32(1.0), np.zeros(0, np.float32)):
        with pytest.raises(ValueError, match=r"\(L,\)"):
            WavefrontPaths(None, 8, 8, 1, 1, CAMERA, lights=LIGHTS, fused_shadows=True, shadow_samples=4, light_radii=bad)
    for bad in (0, 65536):
        with pytest.raises(ValueError, match="shadow_samples"):
            WavefrontPaths(None, 8, 8, 1, 1, CAMERA, lights=LIGHTS, fused_shadows=True, shadow_samples=bad, light_radii=RADII)
    with pytest.raises(ValueError, match="shadow_samples > 1"):  # radii without samples: refused, not ignored
        WavefrontPaths(None, 8, 8, 1, 1, CAMERA, lights=LIGHTS, fused_shadows=True, light_radii=RADII)
    with pytest.raises(ValueError, match="2\\^32"):  # n * L * S must fit the launch's 32-bit item index: 2^26 * 2 * 32 = 2^32
        WavefrontPaths(None, 1 << 13, 1 << 13, 1, 1, CAMERA, lights=LIGHTS, fused_shadows=True, shadow_samples=32, light_radii=RADII)
