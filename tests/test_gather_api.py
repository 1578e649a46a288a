"""CPU-side checks of the final gather (rc_final_gather_device): the binding matches the header's prototype, the library exports it, the
header states the identity and the contract, the Python and Julia layers carry it, every argument error of final_gather(), irradiance()
and WavefrontPaths.with_final_gather() is raised before a device is touched, irradiance()'s quantisation round-trips within one step, and
traced_rays() counts the stage."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

from api_kit import ROOT, header, julia_text
from api_kit import rc  # noqa: F401

NAME = "rc_final_gather_device"
ARGS = ["rc_scene*", "const rc_ray*", "const rc_hit*", "uint64_t", "uint32_t", "float", "uint64_t", "uint32_t", "const uint32_t*", "uint64_t", "float",
        "const uint32_t*", "uint32_t", "uint64_t*", "uint32_t*", "void*"]
CTYPES = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}
JL_ARGS = ["Ptr{Cvoid}", "Ptr{RTRay}", "Ptr{RTHitResult}", "UInt64", "UInt32", "Cfloat", "UInt64", "UInt32", "Ptr{UInt32}", "UInt64", "Cfloat", "Ptr{UInt32}",
           "UInt32", "Ptr{UInt64}", "Ptr{UInt32}", "Ptr{Cvoid}"]


def test_symbol_matches_the_header(rc):
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{NAME} is not declared in the header"
    assert [" ".join(a.split()[:-1]) for a in m.group(1).split(",")] == ARGS
    bound = {n: (res, args) for n, res, args in rc.SYMBOLS}
    res, args = bound[NAME]
    assert res is C.c_int and args == [CTYPES.get(a, C.c_void_p) for a in ARGS]
    assert hasattr(rc.lib(), NAME)


def test_header_documents_the_call():
    text = header()
    at = text.index("int " + NAME)
    comment = text[text.rindex("/*", 0, at):at]
    for needle in ("d_sum[i]  += sum over s of  live(i,s) && H.hit && 1 <= m <= N ? x[m-1]  :  live(i,s) && !H.hit ? miss_value : 0",
                   "d_open[i] += sum over s of  live(i,s) && !H.hit", "live(i,s) = d_hits[i].hit && ray(i,s).t_max > 0", "rc_trace_closest_device",
                   "rc_ambient_occlusion_rays_device", "bit for", "no tolerance", "src/kernels.jl:123", "src/instanced-bvh.jl:1902-2024",
                   "src/math.jl:1-21", "d_open equals what rc_ambient_occlusion_device adds to d_count", "t_min = 0", "NaN", "NO extra gate",
                   "ACCUMULATES", "the caller zeroes", "WHEN THE KERNEL RUNS", "may be NULL", "modulo 2^64",
                   "No allocation, copy, event, memset, host synchronisation or scene-owned scratch", "re-entrant across streams", "captured", "rc_wait",
                   "n == 0 or samples == 0", "RC_ERR_INVALID_ARGUMENT", "NULL scene", "n * samples >= 2^32", "samples >= 65536", "depth >= 65536",
                   "max_dist not > 0", "+Inf is legal", "RC_ERR_NOT_SYNCED", 'docs/EXPERIMENTS.md, "Final gather"'):
        assert needle in comment, needle


def test_python_surface(rc):
    sig = inspect.signature(rc.TLAS.final_gather_device)
    assert list(sig.parameters) == ["self", "d_rays", "d_hits", "n", "samples", "d_x", "d_sum", "d_open", "miss_value", "max_dist", "seed", "depth", "bias",
                                    "d_path_in", "path_base", "stream"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["d_open"], d["miss_value"], d["max_dist"], d["seed"], d["depth"], d["bias"], d["d_path_in"], d["path_base"], d["stream"]) == (
        None, 0, math.inf, 0, 0, 1e-3, None, 0, None)
    sig = inspect.signature(rc.final_gather)
    assert list(sig.parameters) == ["accel", "rays", "hits", "x", "samples", "max_dist", "miss_value", "seed", "bias"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["max_dist"], d["miss_value"], d["seed"], d["bias"]) == (math.inf, 0, 0, 1e-3)
    sig = inspect.signature(rc.irradiance)
    assert list(sig.parameters) == ["accel", "rays", "hits", "b", "samples", "sky", "max_dist", "seed", "bias", "return_open"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["sky"], d["max_dist"], d["seed"], d["bias"], d["return_open"]) == (0.0, math.inf, 0, 1e-3, False)
    sig = inspect.signature(rc.wavefront.WavefrontPaths.with_final_gather)
    assert list(sig.parameters) == ["self", "x", "samples", "distance", "miss_value"]
    assert (sig.parameters["distance"].default, sig.parameters["miss_value"].default) == (math.inf, 0)
    for doc in (rc.irradiance.__doc__,):
        assert "cosine-weighted mean" in doc and "IRRADIANCE" in doc and "reflectance" in doc and "1 / scale" in doc


def test_julia_binding_and_integration_line():
    text = julia_text()
    m = re.search(r"ccall\(\(:" + NAME + r", LIB\), Cint,\s*\(([^)]*)\)", text)
    assert m, f"no ccall of {NAME}"
    assert [t.strip() for t in m.group(1).split(",")] == JL_ARGS
    assert re.search(r"^final_gather_device!\(a::MI355XStaticTLAS, d_rays::Ptr\{RTRay\}, d_hits::Ptr\{RTHitResult\}, n::Integer, samples::Integer,", text, flags=re.M)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "final_gather_device!" in integration and NAME in integration


def test_null_scene_is_refused_before_anything_else(rc):
    f = getattr(rc.lib(), NAME)
    assert f(None, None, None, 0, 0, math.inf, 0, 0, None, 0, 1e-3, None, 0, None, None, None) == 1  # RC_ERR_INVALID_ARGUMENT
    assert f(None, 64, 64, 16, 4, 1.0, 0, 0, None, 0, 1e-3, 64, 7, 64, 64, None) == 1


def frame_of(rc, n):
    from oracle.pyoracle import HIT_DT, RAY_DT
    return np.zeros(n, RAY_DT), np.zeros(n, HIT_DT)


class NoDevice:
    """Stands where an accel is expected: any use of it is a failure -- the argument checks come first."""

    def __getattr__(self, name):
        raise AssertionError(f"the accel was touched ({name}) before the arguments were checked")


def test_final_gather_checks_its_arguments_without_a_device(rc):
    rays, hits = frame_of(rc, 16)
    x = np.ones(8, np.uint32)
    acc = NoDevice()
    with pytest.raises(ValueError, match="hits"):
        rc.final_gather(acc, rays, hits[:5], x, 4)
    with pytest.raises(ValueError, match="hits"):
        rc.final_gather(acc, rays, hits.view(np.uint8), x, 4)
    for bad in (-1, 65536, 1 << 40, 2.5, True):
        with pytest.raises(ValueError, match="samples"):
            rc.final_gather(acc, rays, hits, x, bad)
    for bad in (0.0, -1.0, -math.inf, math.nan):
        with pytest.raises(ValueError, match="distance"):
            rc.final_gather(acc, rays, hits, x, 4, max_dist=bad)
    for bad in (-1, 1 << 32, 0.5, True):
        with pytest.raises(ValueError, match="miss_value"):
            rc.final_gather(acc, rays, hits, x, 4, miss_value=bad)
    for bad in (x.astype(np.int32), x.astype(np.float64), x.reshape(2, 4), list(x), None):
        with pytest.raises(ValueError, match="x must be"):
            rc.final_gather(acc, rays, hits, bad, 4)


def test_irradiance_checks_its_arguments_without_a_device(rc):
    rays, hits = frame_of(rc, 16)
    b = np.linspace(0.0, 2.0, 8)
    acc = NoDevice()
    for bad in (-b, np.array([1.0, np.nan]), np.array([np.inf, 1.0]), b.reshape(2, 4)):
        with pytest.raises(ValueError, match="b must"):
            rc.irradiance(acc, rays, hits, bad, 4)
    for bad in (-1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="sky"):
            rc.irradiance(acc, rays, hits, b, 4, sky=bad)
    for bad in (0, -1, 65536, 1.5, True):
        with pytest.raises(ValueError, match="samples"):
            rc.irradiance(acc, rays, hits, b, bad)
    with pytest.raises(ValueError, match="distance"):
        rc.irradiance(acc, rays, hits, b, 4, max_dist=0.0)
    with pytest.raises(ValueError, match="hits"):
        rc.irradiance(acc, rays, hits[:3], b, 4)


def test_irradiance_quantisation_round_trips(rc):
    """One scale for the field and the sky, floor: a value comes back at most one step, 1 / scale, below itself -- so a constant b and a
    sky, averaged over any mix of hit and escaped samples, come back within one step of the float mean.  The step is the bound; `eps` is
    only the float64 rounding of the check's own arithmetic: b * scale is below 2^32 and rounded to 53 bits, so it is off by at most
    2^-21 steps, and the division back by as much again -- 2^-20 of a step covers both."""
    for b0, sky in ((0.731, 0.0), (0.731, 3.9), (12.5, 0.02), (1e-9, 1e-9), (5.0, 5.0)):
        scale, b_q, sky_q = rc.irradiance_scale(np.full(7, b0), sky)
        assert scale == ((1 << 32) - 1) / max(b0, sky)
        assert b_q.dtype == np.uint32 and b_q.shape == (7,) and isinstance(sky_q, int) and 0 <= sky_q < 1 << 32
        step = 1.0 / scale
        eps = step * 2.0 ** -20
        assert -eps <= b0 - int(b_q[0]) / scale <= step + eps and -eps <= sky - sky_q / scale <= step + eps
        assert max(int(b_q.max()), sky_q) >= (1 << 32) - 2  # the larger of the two uses the whole range
        for S, n_hit in ((1, 1), (5, 2), (64, 0), (64, 64)):
            sums = n_hit * int(b_q[0]) + (S - n_hit) * sky_q  # what final_gather returns for n_hit hits and S - n_hit escapes
            want = (n_hit * b0 + (S - n_hit) * sky) / S
            assert -eps <= want - sums / (S * scale) <= step + eps
    scale, b_q, sky_q = rc.irradiance_scale(np.zeros(3), 0.0)
    assert scale == 1.0 and not b_q.any() and sky_q == 0
    scale, b_q, _ = rc.irradiance_scale(np.array([0.0, 1.0, 0.5]))
    assert b_q.tolist() == [0, (1 << 32) - 1, ((1 << 32) - 1) // 2]


def test_frame_arguments_and_traced_rays_without_a_device(rc):
    """WavefrontPaths cannot be built without a device: the checks of with_final_gather through the helper it calls first and on a frame
    object that never saw one; traced_rays() is arithmetic on the frame's fields."""
    from raycore_jl_amd.wavefront import WavefrontPaths, check_gather_arguments
    assert check_gather_arguments(64 * 48 * 2, 4, 2.0, 7) == (4, 2.0, 7)
    assert check_gather_arguments(1, 0, math.inf, 0) == (0, math.inf, 0)
    assert check_gather_arguments(1, 65535, 1e-30, (1 << 32) - 1) == (65535, 1e-30, (1 << 32) - 1)
    with pytest.raises(ValueError, match="2\\^32"):
        check_gather_arguments(1 << 26, 64, 1.0, 0)
    assert check_gather_arguments((1 << 26) - 1, 64, 1.0, 0) == (64, 1.0, 0)
    frame = object.__new__(WavefrontPaths)
    frame.n = 1 << 26
    for args, what in (((None, 65536), "samples"), ((None, -1), "samples"), ((None, 4, 0.0), "distance"), ((None, 4, math.nan), "distance"),
                       ((None, 4, 1.0, -1), "miss_value"), ((None, 4, 1.0, 1 << 32), "miss_value"), ((None, 64, 1.0), "2\\^32")):
        with pytest.raises(ValueError, match=what):
            frame.with_final_gather(*args)
    frame.n, frame.depth, frame.n_lights, frame.shadow_samples, frame.fused_shadows, frame.ao_samples = 6144, 2, 0, 1, False, 0
    frame.gather_samples = 0
    assert frame.traced_rays() == 6144 * 2 * 2
    frame.gather_samples = 4
    assert frame.traced_rays() == 6144 * 2 * 2 + 6144 * 4 * 2
    frame.ao_samples = 3
    assert frame.traced_rays() == 6144 * 2 * 2 + 6144 * 3 * 2 + 6144 * 4 * 2
