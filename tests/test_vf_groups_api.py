"""CPU-side checks of the grouped view-factor calls (rc_view_factor_sampled_rays_device, rc_view_factor_groups_device): the bindings match
the header's prototypes, the library exports them, the header states the rule and the identity, the Python and Julia layers carry them,
and every argument error of view_factor_groups() and form_factors() is raised before a device is touched."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from api_kit import ROOT, header, julia_text
from api_kit import rc  # noqa: F401

PROTOTYPES = {
    "rc_view_factor_sampled_rays_device": ["rc_scene*", "uint64_t", "uint32_t", "uint32_t", "uint32_t", "uint32_t", "rc_ray*", "void*"],
    "rc_view_factor_groups_device": ["rc_scene*", "uint32_t", "uint64_t", "uint32_t", "uint32_t", "uint32_t", "uint32_t", "uint32_t", "const uint32_t*", "uint32_t",
                                     "const uint32_t*", "uint64_t*", "uint64_t*", "void*"],
}
JL_ARGS = {
    "rc_view_factor_sampled_rays_device": ["Ptr{Cvoid}", "UInt64", "UInt32", "UInt32", "UInt32", "UInt32", "Ptr{RTRay}", "Ptr{Cvoid}"],
    "rc_view_factor_groups_device": ["Ptr{Cvoid}", "UInt32", "UInt64", "UInt32", "UInt32", "UInt32", "UInt32", "UInt32", "Ptr{UInt32}", "UInt32", "Ptr{UInt32}",
                                     "Ptr{UInt64}", "Ptr{UInt64}", "Ptr{Cvoid}"],
}
CTYPES = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
RC_ERR_INVALID_ARGUMENT = 1


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_symbols_match_the_header(rc, name):
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in the header"
    assert [" ".join(a.split()[:-1]) for a in m.group(1).split(",")] == PROTOTYPES[name]
    res, args = {n: (r, a) for n, r, a in rc.SYMBOLS}[name]
    assert res is C.c_int and args == [CTYPES.get(a, C.c_void_p) for a in PROTOTYPES[name]]
    assert hasattr(rc.lib(), name)


def test_header_documents_the_calls():
    text = header()
    assert re.search(r"#define RC_VF_SAMPLING_UNIFORM 0u\b", text) and re.search(r"#define RC_VF_SAMPLING_COSINE\s+1u\b", text)
    at = text.index("int rc_view_factor_sampled_rays_device")
    comment = text[text.rindex("/* ----", 0, at):at]
    for needle in ("N = number of flat primitives", "a = the source's metadata, b = the hit's", "ga = groups[a-1], gb = groups[b-1]", "wa = weights ? weights[a-1] : 1",
                   "A source whose a is outside 1..N, or whose ga >= G, contributes nothing", "Miss: escaped[ga] += wa, if escaped is given",
                   "Hit with b in 1..N, b != a and gb < G: matrix[ga * G + gb] += wa", "hit_idx != tri_idx, src/kernels.jl:96", "Any other hit adds nothing",
                   "u64 modulo 2^64", "any partition of sources x rays gives the same words", "counter (ray_idx, src_prim, 0,", "pt + normal * 0.01f",
                   "bit for bit", "rc_bounce_rays_device", "not renormalised", "t_min = 0, t_max = inf", "src/kernels.jl:92", "P diag(w) M P^T",
                   "rc_view_factor_totals", "rc_view_factor_sampled_rays_device -> rc_trace_closest_device", "ACCUMULATE", "the caller zeroes",
                   "WHEN THE KERNEL RUNS", "or NULL", "fit 256 MiB (G <= 1447 with escapes)", "Both paths give the same words", "captured",
                   "rc_update_geometry_device_async",
                   "RC_ERR_INVALID_ARGUMENT for a NULL scene, d_groups or d_matrix, for sampling > 1, and for n_groups outside 1..65535", "RC_ERR_NOT_SYNCED",
                   'docs/EXPERIMENTS.md, "Form factors between surface groups"'):
        assert needle in comment, needle


def test_python_surface(rc):
    sig = inspect.signature(rc.TLAS.view_factor_sampled_rays_device)
    assert list(sig.parameters) == ["self", "d_rays", "src_prim", "n_rays", "seed", "sampling", "ray_begin", "stream"]
    sig = inspect.signature(rc.TLAS.view_factor_groups_device)
    assert list(sig.parameters) == ["self", "groups_ptr", "n_groups", "matrix_ptr", "rays_per_triangle", "seed", "sampling", "weights_ptr", "escaped_ptr", "src",
                                    "rays", "stream"]
    sig = inspect.signature(rc.view_factor_groups)
    assert list(sig.parameters) == ["accel", "groups", "rays_per_triangle", "seed", "weights", "sampling", "n_groups", "return_escaped"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["rays_per_triangle"], d["seed"], d["weights"], d["sampling"], d["n_groups"], d["return_escaped"]) == (10000, 0, None, "uniform", None, False)
    sig = inspect.signature(rc.form_factors)
    assert list(sig.parameters) == ["accel", "groups", "rays_per_triangle", "seed", "n_groups"]
    assert list(inspect.signature(rc.form_factor_weights).parameters) == ["areas", "rays_per_triangle"]
    assert list(inspect.signature(rc.primitive_areas).parameters) == ["accel"]
    from raycore_jl_amd import api
    assert api.vf_sampling("uniform") == 0 and api.vf_sampling("cosine") == 1 and api.vf_sampling(1) == 1
    for doc in (rc.view_factor_bounces.__doc__, rc.radiosity.__doc__):
        assert "form_factors()" in doc


def test_julia_binding_and_integration_line():
    text = julia_text()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, jl in JL_ARGS.items():
        m = re.search(r"ccall\(\(:" + name + r", LIB\), Cint,\s*\(([^)]*)\)", text)
        assert m, f"no ccall of {name}"
        assert [t.strip() for t in m.group(1).split(",")] == jl
        assert name in integration
    assert re.search(r"^view_factor_groups_device!\(a::MI355XStaticTLAS, rays_per_triangle::Integer, seed::UInt64, sampling::Integer,", text, flags=re.M)
    assert re.search(r"^view_factor_sampled_rays_device!\(a::MI355XStaticTLAS, seed::UInt64, sampling::Integer, src_prim::Integer,", text, flags=re.M)
    assert "view_factor_groups_device!" in integration


def test_invalid_arguments_are_refused_without_a_device(rc):
    L = rc.lib()
    f, g = L.rc_view_factor_groups_device, L.rc_view_factor_sampled_rays_device
    assert f(None, 16, 0, 0, 0, 8, 0, 16, None, 1, None, None, None, None) == RC_ERR_INVALID_ARGUMENT
    assert f(None, 16, 0, 1, 0, 8, 0, 16, 64, 7, None, 64, None, None) == RC_ERR_INVALID_ARGUMENT
    assert g(None, 0, 0, 0, 0, 0, None, None) == RC_ERR_INVALID_ARGUMENT
    assert g(None, 0, 1, 0, 0, 4, 64, None) == RC_ERR_INVALID_ARGUMENT


class NoDevice:
    """Stands where an accel is expected: any use of it is a failure -- the argument checks come first."""

    def __getattr__(self, name):
        raise AssertionError(f"the accel was touched ({name}) before the arguments were checked")


def test_view_factor_groups_checks_its_arguments_without_a_device(rc):
    acc = NoDevice()
    g = np.arange(8, dtype=np.uint32) % 3
    for bad in (g.astype(np.float64), g.reshape(2, 4), np.array([0, -1]), np.array([0, 1 << 32]), np.array([True, False]), None):
        with pytest.raises(ValueError, match="groups"):
            rc.view_factor_groups(acc, bad, 16)
    for bad in (g[:5], g.astype(np.float32), np.full(8, -1), np.full(8, 1 << 32, np.uint64)):
        with pytest.raises(ValueError, match="weights"):
            rc.view_factor_groups(acc, g, 16, weights=bad)
    for bad in ("lambert", "", 2, -1, None, True, 0.0):
        with pytest.raises(ValueError, match="sampling"):
            rc.view_factor_groups(acc, g, 16, sampling=bad)
    for bad in (0, 65536, -1, 2.0, True):
        with pytest.raises(ValueError, match="n_groups"):
            rc.view_factor_groups(acc, g, 16, n_groups=bad)
    with pytest.raises(ValueError, match="n_groups"):  # the default: the largest group below 2^32 - 1, plus one
        rc.view_factor_groups(acc, np.array([0, 65535], np.uint32), 16)
    with pytest.raises(ValueError, match="n_groups"):  # nothing but excluded primitives
        rc.view_factor_groups(acc, np.full(4, 0xFFFFFFFF, np.uint32), 16)
    for bad in (-1, 1 << 32, 1.5, True):
        with pytest.raises(ValueError, match="rays_per_triangle"):
            rc.view_factor_groups(acc, g, bad)
    for bad in (-1, 1 << 64, 0.5):
        with pytest.raises(ValueError, match="seed"):
            rc.view_factor_groups(acc, g, 16, seed=bad)
    from raycore_jl_amd.api import check_groups_arguments
    gg, ww, word, G = check_groups_arguments(np.array([0, 2, 0xFFFFFFFF, 1], np.int64), None, 16, 0, "cosine", None)
    assert gg.dtype == np.uint32 and ww is None and word == 1 and G == 3
    assert check_groups_arguments(g, np.ones(8, np.int64), 0, (1 << 64) - 1, "uniform", 65535)[2:] == (0, 65535)


def test_form_factors_checks_its_arguments_without_a_device(rc):
    acc = NoDevice()
    g = np.zeros(8, np.uint32)
    with pytest.raises(ValueError, match="groups"):
        rc.form_factors(acc, g.astype(np.float64))
    with pytest.raises(ValueError, match="n_groups"):
        rc.form_factors(acc, g, n_groups=0)
    with pytest.raises(ValueError, match="seed"):
        rc.form_factors(acc, g, seed=-1)
    with pytest.raises(ValueError, match="rays_per_triangle"):
        rc.form_factors(acc, g, rays_per_triangle=1 << 32)
