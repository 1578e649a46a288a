"""CPU-side checks of the ambient-occlusion pair (rc_ambient_occlusion_rays_device, rc_ambient_occlusion_device): the bindings match the
header's prototypes, the library exports them, the header states the identity and the contract, the Python and Julia layers carry them,
the frame's arguments are validated before a device is touched, and a NULL scene is refused first, with or without a GPU."""
import ctypes as C
import inspect
import math
import os
import re

import pytest

from api_kit import ROOT, header, julia_text, prototype
from api_kit import rc  # noqa: F401

C_TO_CTYPES = {"rc_scene*": C.c_void_p, "void*": C.c_void_p, "const rc_ray*": C.c_void_p, "const rc_hit*": C.c_void_p, "const uint32_t*": C.c_void_p,
               "rc_ray*": C.c_void_p, "uint32_t*": C.c_void_p, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}
HEAD = ["rc_scene*", "const rc_ray*", "const rc_hit*", "uint64_t", "uint32_t", "float", "uint64_t", "uint32_t", "const uint32_t*", "uint64_t", "float"]
ARGS = {"rc_ambient_occlusion_rays_device": HEAD + ["rc_ray*", "void*"], "rc_ambient_occlusion_device": HEAD + ["uint32_t*", "void*"]}
JL_HEAD = ["Ptr{Cvoid}", "Ptr{RTRay}", "Ptr{RTHitResult}", "UInt64", "UInt32", "Cfloat", "UInt64", "UInt32", "Ptr{UInt32}", "UInt64", "Cfloat"]
JL_ARGS = {"rc_ambient_occlusion_rays_device": JL_HEAD + ["Ptr{RTRay}", "Ptr{Cvoid}"], "rc_ambient_occlusion_device": JL_HEAD + ["Ptr{UInt32}", "Ptr{Cvoid}"]}
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


def test_declarations_close_the_header():
    """Appended after rc_generate_ray_grid_dirs_device, inside the extern "C" block: no earlier line of the header moved."""
    text = header()
    at = [text.index("int " + n + "(") for n in ("rc_generate_ray_grid_dirs_device", "rc_ambient_occlusion_rays_device", "rc_ambient_occlusion_device")]
    assert at == sorted(at)
    tail = re.sub(r"/\*.*?\*/", "", text[at[2]:], flags=re.S)
    assert re.fullmatch(r'int rc_ambient_occlusion_device\([^)]*\);\s*#ifdef __cplusplus\s*}\s*#endif\s*#endif\s*', tail), tail[-200:]


@pytest.mark.parametrize("name", NAMES)
def test_header_documents_the_call(name):
    """The comment in front of the declarations states the sample, the slot layout, the identity with the composed path, what a NaN frame
    does, the conventions and the error contract."""
    text = header()
    at = text.index("int " + name)
    comment = text[text.rindex("/*", 0, at):at]
    for needle in ("(lo32 path, hi32 path, s, 0x414F0000 | depth)", "Philox4x32-10", "(word >> 8) * 2^-24", "rc_bounce_rays_device", "not renormalised",
                   "p + nn * bias", "t_max max_dist", "no contraction", "i * samples + s", "d = (0,0,1), t_max = 0",
                   "d_count[i] += sum over s of (d_hits[i].hit && ray(i, s).t_max > 0 && !any_hit(ray(i, s)).hit)",
                   "bit for bit what rc_ambient_occlusion_rays_device writes", "no tolerance", "rc_trace_any_device", "NaN", "NO extra gate",
                   "the same in both paths", "ACCUMULATES", "the caller zeroes", "No allocation, copy, event, memset, host synchronisation or scene-owned scratch",
                   "re-entrant across streams", "captured", "rc_wait", "n == 0 or samples == 0", "entry_cull", "RC_ERR_INVALID_ARGUMENT", "NULL scene",
                   "n * samples >= 2^32", "wrap in 64 bits", "samples >= 65536", "depth >= 65536", "max_dist not > 0", "+Inf is legal",
                   "RC_ERR_NOT_SYNCED", "rc_shadow_visibility_device", 'docs/EXPERIMENTS.md, "Ambient occlusion"'):
        assert needle in comment, needle


def test_python_surface(rc):
    sig = inspect.signature(rc.TLAS.ambient_occlusion_device)
    assert list(sig.parameters) == ["self", "d_rays", "d_hits", "n", "samples", "d_count", "max_dist", "seed", "depth", "bias", "d_path_in", "path_base",
                                    "stream"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["max_dist"], d["seed"], d["depth"], d["bias"], d["d_path_in"], d["path_base"], d["stream"]) == (math.inf, 0, 0, 1e-3, None, 0, None)
    sig = inspect.signature(rc.TLAS.ambient_occlusion_rays_device)
    assert list(sig.parameters) == ["self", "d_rays", "d_hits", "n", "samples", "d_ao_rays", "max_dist", "seed", "depth", "bias", "d_path_in",
                                    "path_base", "stream"]
    sig = inspect.signature(rc.ambient_occlusion)
    assert list(sig.parameters) == ["accel", "rays", "hits", "samples", "max_dist", "seed", "bias"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["max_dist"], d["seed"], d["bias"]) == (math.inf, 0, 1e-3)
    sig = inspect.signature(rc.wavefront.WavefrontPaths.with_ambient_occlusion)
    assert list(sig.parameters) == ["self", "ao_samples", "ao_distance"] and sig.parameters["ao_distance"].default == math.inf


@pytest.mark.parametrize("name", NAMES)
def test_julia_binding_has_the_method(name):
    text = julia_text()
    m = re.search(r"ccall\(\(:" + name + r", LIB\), Cint,\s*\(([^)]*)\)", text)
    assert m, f"no ccall of {name}"
    assert [t.strip() for t in m.group(1).split(",")] == JL_ARGS[name]
    method = name[3:] + "!"
    assert re.search(r"^" + method + r"\(a::MI355XStaticTLAS, d_rays::Ptr\{RTRay\}, d_hits::Ptr\{RTHitResult\}, n::Integer, samples::Integer,", text,
                     flags=re.M), method
    assert method in open(os.path.join(ROOT, "INTEGRATION.md")).read()


@pytest.mark.parametrize("name", NAMES)
def test_null_scene_is_refused_before_anything_else(rc, name):
    """NULL scene -> RC_ERR_INVALID_ARGUMENT whether or not a GPU is visible (the check comes first), with or without work."""
    f = getattr(rc.lib(), name)
    assert f(None, None, None, 0, 0, math.inf, 0, 0, None, 0, 1e-3, None, None) == 1  # RC_ERR_INVALID_ARGUMENT
    assert f(None, 64, 64, 16, 4, 1.0, 0, 0, None, 0, 1e-3, 64, None) == 1
    if rc.device_count() == 0:
        with pytest.raises(rc.RaycoreError) as e:
            rc.TLAS(0)
        assert e.value.code == 3  # RC_ERR_NO_DEVICE


def test_frame_arguments_are_checked_without_a_device():
    """WavefrontPaths cannot be built without a device, so the checks of with_ambient_occlusion are exercised through the helper it calls
    first: ao_samples in [0, 65536), ao_distance > 0, width * height * samples * ao_samples < 2^32."""
    from raycore_jl_amd.wavefront import WavefrontPaths, check_ao_arguments
    assert check_ao_arguments(64 * 48 * 2, 4, 2.0) == (4, 2.0)
    assert check_ao_arguments(1, 0, math.inf) == (0, math.inf)
    assert check_ao_arguments(1, 65535, 1e-30) == (65535, 1e-30)
    for bad in (-1, 65536, 1 << 40, 2.5, True):
        with pytest.raises(ValueError, match="ao_samples"):
            check_ao_arguments(16, bad, 1.0)
    for bad in (0.0, -1.0, -math.inf, math.nan):
        with pytest.raises(ValueError, match="ao_distance"):
            check_ao_arguments(16, 4, bad)
    with pytest.raises(ValueError, match="2\\^32"):  # 2^26 paths x 64 samples
        check_ao_arguments(1 << 26, 64, 1.0)
    assert check_ao_arguments((1 << 26) - 1, 64, 1.0) == (64, 1.0)
    # the method validates before it allocates: a frame object that never saw a device still refuses
    frame = object.__new__(WavefrontPaths)
    frame.n = 1 << 26
    for args, what in (((65536,), "ao_samples"), ((4, 0.0), "ao_distance"), ((64, 1.0), "2\\^32")):
        with pytest.raises(ValueError, match=what):
            frame.with_ambient_occlusion(*args)
