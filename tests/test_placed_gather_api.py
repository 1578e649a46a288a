"""CPU-side checks of the placed final gather (rc_placed_hit_indices_device, rc_placed_final_gather_device): the bindings match the header's
prototypes, the library exports them, the header states the rule and the contract, the Python and Julia layers carry them, the documents
name them, every argument error of placed_hit_indices(), placed_final_gather(), placed_irradiance() and
WavefrontPaths.with_placed_final_gather() is raised before a device is touched, and the metadata switch keeps its signature."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

from api_kit import ROOT, header, julia_text, prototype
from api_kit import rc  # noqa: F401

GATHER, INDICES = "rc_placed_final_gather_device", "rc_placed_hit_indices_device"
ARGS = {GATHER: ["rc_scene*", "const rc_ray*", "const rc_hit*", "uint64_t", "uint32_t", "float", "uint64_t", "uint32_t", "const uint32_t*", "uint64_t",
                 "float", "const uint32_t*", "uint32_t", "uint64_t*", "uint32_t*", "void*"],
        INDICES: ["rc_scene*", "const rc_hit*", "uint64_t", "uint32_t*", "void*"]}
CTYPES = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}
JL_ARGS = {GATHER: ["Ptr{Cvoid}", "Ptr{RTRay}", "Ptr{RTHitResult}", "UInt64", "UInt32", "Cfloat", "UInt64", "UInt32", "Ptr{UInt32}", "UInt64", "Cfloat",
                    "Ptr{UInt32}", "UInt32", "Ptr{UInt64}", "Ptr{UInt32}", "Ptr{Cvoid}"],
           INDICES: ["Ptr{Cvoid}", "Ptr{RTHitResult}", "UInt64", "Ptr{UInt32}", "Ptr{Cvoid}"]}


@pytest.mark.parametrize("name", [GATHER, INDICES])
def test_symbols_match_the_header(rc, name):
    assert prototype(name) == ARGS[name]
    bound = {n: (res, args) for n, res, args in rc.SYMBOLS}
    res, args = bound[name]
    assert res is C.c_int and args == [CTYPES.get(a, C.c_void_p) for a in ARGS[name]]
    assert hasattr(rc.lib(), name)


def test_the_gather_takes_the_metadata_gathers_arguments():
    assert prototype(GATHER) == prototype("rc_final_gather_device")


def test_header_documents_the_calls():
    text = header()
    at = text.index("int " + INDICES)
    # the block stands behind the placed CSR and in front of the final gather: the seven declarations from there to the end of the header
    # are pinned by tests/test_placed_vf_api.py and tests/test_ao_api.py, and no earlier line of the header moved
    assert text.index("int rc_placed_view_factors_sparse_device") < at < text.index("int " + GATHER) < text.index("/* ---- Final gather:")
    assert at > sum(len(line) + 1 for line in text.split("\n")[:725])  # (tests/test_lifecycle_model.py cites lines up to 725)
    comment = text[text.rindex("/*", 0, at):at]
    for needle in ("d_sum[i]  += sum over s of  live(i,s) && H.hit ? x[base[H.instance_id] + l(H)]  :  live(i,s) && !H.hit ? miss_value : 0",
                   "d_open[i] += sum over s of  live(i,s) && !H.hit", "no metadata", "exact, no tolerance", "prim = l + 1", "base[instance] + prim - 1",
                   "EVERY hit is counted", "d_open equals what rc_final_gather_device and rc_ambient_occlusion_device add for the same arguments",
                   "rc_ambient_occlusion_rays_device", "bit for bit", "WHEN THE KERNEL RUNS", "may be NULL", "modulo 2^64", "ACCUMULATES", "the caller zeroes",
                   "x IS WHATEVER THE CALLER HANDS IN", "RC_INVALID_ID", "hit == 0", "rc_hit_points_device", "One kernel, no scratch",
                   "No allocation, copy, event, memset, host synchronisation or scene-owned scratch", "re-entrant across streams", "captured", "rc_wait",
                   "rc_update_transforms_device -> rc_refit_device_async", "rc_update_geometry_device_async", "base does not change there",
                   "n == 0 or samples == 0", "rc_final_gather_device's in its order", "RC_ERR_INVALID_ARGUMENT", "NULL scene", "samples >= 65536",
                   "depth >= 65536", "max_dist not > 0", "+Inf is legal", "n * samples >= 2^32", "NULL d_rays, d_hits, d_sum or d_x while there is work",
                   "RC_ERR_NOT_SYNCED", "P >= 2^32", "where rc_placed_view_factor_products_device checks", "no test can reach it",
                   'docs/EXPERIMENTS.md, "Placed final gather"'):
        assert needle in comment, needle


def test_python_surface(rc):
    sig = inspect.signature(rc.TLAS.placed_final_gather_device)
    twin = inspect.signature(rc.TLAS.final_gather_device)
    assert list(sig.parameters) == list(twin.parameters) == ["self", "d_rays", "d_hits", "n", "samples", "d_x", "d_sum", "d_open", "miss_value", "max_dist",
                                                             "seed", "depth", "bias", "d_path_in", "path_base", "stream"]
    assert [p.default for p in sig.parameters.values()] == [p.default for p in twin.parameters.values()]
    sig = inspect.signature(rc.TLAS.placed_hit_indices_device)
    assert list(sig.parameters) == ["self", "d_hits", "n", "d_q", "stream"] and sig.parameters["stream"].default is None
    sig = inspect.signature(rc.placed_hit_indices)
    assert list(sig.parameters) == ["accel", "hits"]
    sig = inspect.signature(rc.placed_final_gather)
    assert list(sig.parameters) == ["accel", "rays", "hits", "x", "samples", "max_dist", "miss_value", "seed", "bias"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["max_dist"], d["miss_value"], d["seed"], d["bias"]) == (math.inf, 0, 0, 1e-3)
    sig = inspect.signature(rc.placed_irradiance)
    assert list(sig.parameters) == ["accel", "rays", "hits", "b", "samples", "sky", "max_dist", "seed", "bias", "return_open"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["sky"], d["max_dist"], d["seed"], d["bias"], d["return_open"]) == (0.0, math.inf, 0, 1e-3, False)
    assert "IRRADIANCE" in rc.placed_irradiance.__doc__ and "placed primitive" in rc.placed_irradiance.__doc__
    W = rc.wavefront.WavefrontPaths
    sig = inspect.signature(W.with_placed_final_gather)
    assert list(sig.parameters) == ["self", "x", "samples", "distance", "miss_value"]
    assert (sig.parameters["distance"].default, sig.parameters["miss_value"].default) == (math.inf, 0)
    sig = inspect.signature(W.with_final_gather)  # the metadata switch is what it was
    assert list(sig.parameters) == ["self", "x", "samples", "distance", "miss_value"]
    assert (sig.parameters["distance"].default, sig.parameters["miss_value"].default) == (math.inf, 0)


def test_julia_bindings_and_documents():
    text = julia_text()
    for name in (GATHER, INDICES):
        m = re.search(r"ccall\(\(:" + name + r", LIB\), Cint,\s*\(([^)]*)\)", text)
        assert m, f"no ccall of {name}"
        assert [t.strip() for t in m.group(1).split(",")] == JL_ARGS[name]
    assert re.search(r"^placed_final_gather_device!\(a::MI355XStaticTLAS, d_rays::Ptr\{RTRay\}, d_hits::Ptr\{RTHitResult\}, n::Integer, samples::Integer,", text, flags=re.M)
    assert re.search(r"^placed_hit_indices_device!\(a::MI355XStaticTLAS, d_hits::Ptr\{RTHitResult\}, n::Integer, d_q::Ptr\{UInt32\};", text, flags=re.M)
    read = lambda name: open(os.path.join(ROOT, name)).read()  # noqa: E731
    integration, readme, design = read("INTEGRATION.md"), read("README.md"), read("DESIGN.md")
    for name, bang in ((GATHER, "placed_final_gather_device!"), (INDICES, "placed_hit_indices_device!")):
        assert name in integration and bang in integration
        assert name in readme and name in design
    assert "placed_irradiance" in readme and "with_placed_final_gather" in design
    open_list = design[design.index("Still open:"):]
    assert "a placed final gather" not in open_list and "placed illumination" in open_list[:1200]
    assert "## Placed final gather" in read(os.path.join("docs", "EXPERIMENTS.md"))


def test_null_scene_is_refused_before_anything_else(rc):
    f = getattr(rc.lib(), GATHER)
    assert f(None, None, None, 0, 0, math.inf, 0, 0, None, 0, 1e-3, None, 0, None, None, None) == 1  # RC_ERR_INVALID_ARGUMENT
    assert f(None, 64, 64, 16, 4, 1.0, 0, 0, None, 0, 1e-3, 64, 7, 64, 64, None) == 1
    g = getattr(rc.lib(), INDICES)
    assert g(None, None, 0, None, None) == 1
    assert g(None, 64, 16, 64, None) == 1


def frame_of(n):
    from oracle.pyoracle import HIT_DT, RAY_DT
    return np.zeros(n, RAY_DT), np.zeros(n, HIT_DT)


class NoDevice:
    """Stands where an accel is expected: any use of it is a failure -- the argument checks come first."""

    def __getattr__(self, name):
        raise AssertionError(f"the accel was touched ({name}) before the arguments were checked")


def test_placed_final_gather_checks_its_arguments_without_a_device(rc):
    rays, hits = frame_of(16)
    x = np.ones(16, np.uint32)
    acc = NoDevice()
    with pytest.raises(ValueError, match="hits"):
        rc.placed_final_gather(acc, rays, hits[:5], x, 4)
    with pytest.raises(ValueError, match="hits"):
        rc.placed_final_gather(acc, rays, hits.view(np.uint8), x, 4)
    for bad in (-1, 65536, 1 << 40, 2.5, True):
        with pytest.raises(ValueError, match="samples"):
            rc.placed_final_gather(acc, rays, hits, x, bad)
    for bad in (0.0, -1.0, -math.inf, math.nan):
        with pytest.raises(ValueError, match="distance"):
            rc.placed_final_gather(acc, rays, hits, x, 4, max_dist=bad)
    for bad in (-1, 1 << 32, 0.5, True):
        with pytest.raises(ValueError, match="miss_value"):
            rc.placed_final_gather(acc, rays, hits, x, 4, miss_value=bad)
    for bad in (x.astype(np.int32), x.astype(np.float64), x.reshape(4, 4), list(x), None):
        with pytest.raises(ValueError, match="x must be .* per placed primitive"):
            rc.placed_final_gather(acc, rays, hits, bad, 4)


def test_placed_irradiance_checks_its_arguments_without_a_device(rc):
    rays, hits = frame_of(16)
    b = np.linspace(0.0, 2.0, 16)
    acc = NoDevice()
    for bad in (-b, np.array([1.0, np.nan]), np.array([np.inf, 1.0]), b.reshape(4, 4)):
        with pytest.raises(ValueError, match="b must"):
            rc.placed_irradiance(acc, rays, hits, bad, 4)
    for bad in (-1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="sky"):
            rc.placed_irradiance(acc, rays, hits, b, 4, sky=bad)
    for bad in (0, -1, 65536, 1.5, True):
        with pytest.raises(ValueError, match="samples"):
            rc.placed_irradiance(acc, rays, hits, b, bad)
    with pytest.raises(ValueError, match="distance"):
        rc.placed_irradiance(acc, rays, hits, b, 4, max_dist=0.0)
    with pytest.raises(ValueError, match="hits"):
        rc.placed_irradiance(acc, rays, hits[:3], b, 4)


def test_placed_hit_indices_checks_its_argument_without_a_device(rc):
    _, hits = frame_of(16)
    acc = NoDevice()
    for bad in (hits.view(np.uint8), hits.reshape(4, 4), np.zeros(16, np.uint32), None):
        with pytest.raises(ValueError, match="hits"):
            rc.placed_hit_indices(acc, bad)


def test_frame_arguments_and_traced_rays_without_a_device(rc):
    """WavefrontPaths cannot be built without a device: the checks of with_placed_final_gather on a frame object that never saw one --
    they are check_gather_arguments', before the accel is read --, and traced_rays() on a frame that has no gather_placed field."""
    from raycore_jl_amd.wavefront import WavefrontPaths
    frame = object.__new__(WavefrontPaths)
    frame.n = 1 << 26
    frame.accel = NoDevice()
    for args, what in (((None, 65536), "samples"), ((None, -1), "samples"), ((None, 4, 0.0), "distance"), ((None, 4, math.nan), "distance"),
                       ((None, 4, 1.0, -1), "miss_value"), ((None, 4, 1.0, 1 << 32), "miss_value"), ((None, 64, 1.0), "2\\^32")):
        with pytest.raises(ValueError, match=what):
            frame.with_placed_final_gather(*args)
        with pytest.raises(ValueError, match=what):
            frame.with_final_gather(*args)
    bare = object.__new__(WavefrontPaths)
    bare.n, bare.depth, bare.n_lights, bare.shadow_samples, bare.fused_shadows, bare.ao_samples = 6144, 2, 0, 1, False, 0
    bare.gather_samples = 4
    assert not hasattr(bare, "gather_placed")
    assert bare.traced_rays() == 6144 * 2 * 2 + 6144 * 4 * 2  # the placed stage traces the same rays: the count does not read the flag
