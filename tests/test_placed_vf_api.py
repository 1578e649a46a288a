"""CPU-side checks of the placed view-factor calls (rc_placed_primitive_bases, rc_placed_triangles_device,
rc_placed_view_factor_rays_device, rc_placed_view_factor_groups_device): the bindings match the header's prototypes at the END of the
header, the library exports them, the header states the index space, the ray and the rule, the Python and Julia layers carry them, and
every argument error of the Python layer is raised before a device is touched -- with lengths counted in PLACED primitives."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from api_kit import ROOT, header, julia_text, prototype
from api_kit import rc  # noqa: F401

PROTOTYPES = {
    "rc_placed_primitive_bases": ["rc_scene*", "uint32_t*", "uint32_t", "uint32_t*"],
    "rc_placed_triangles_device": ["rc_scene*", "uint32_t", "uint32_t", "float*", "void*"],
    "rc_placed_view_factor_rays_device": ["rc_scene*", "uint64_t", "uint32_t", "uint32_t", "uint32_t", "uint32_t", "rc_ray*", "void*"],
    "rc_placed_view_factor_groups_device": ["rc_scene*", "uint32_t", "uint64_t", "uint32_t", "uint32_t", "uint32_t", "uint32_t", "uint32_t", "const uint32_t*",
                                            "uint32_t", "const uint32_t*", "uint64_t*", "uint64_t*", "void*"],
}
JL_ARGS = {
    "rc_placed_primitive_bases": ["Ptr{Cvoid}", "Ptr{UInt32}", "UInt32", "Ref{UInt32}"],
    "rc_placed_triangles_device": ["Ptr{Cvoid}", "UInt32", "UInt32", "Ptr{Float32}", "Ptr{Cvoid}"],
    "rc_placed_view_factor_rays_device": ["Ptr{Cvoid}", "UInt64", "UInt32", "UInt32", "UInt32", "UInt32", "Ptr{RTRay}", "Ptr{Cvoid}"],
    "rc_placed_view_factor_groups_device": ["Ptr{Cvoid}", "UInt32", "UInt64", "UInt32", "UInt32", "UInt32", "UInt32", "UInt32", "Ptr{UInt32}", "UInt32", "Ptr{UInt32}",
                                            "Ptr{UInt64}", "Ptr{UInt64}", "Ptr{Cvoid}"],
}
CTYPES = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
RC_ERR_INVALID_ARGUMENT = 1


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_symbols_match_the_header(rc, name):
    assert prototype(name) == PROTOTYPES[name]
    res, args = {n: (r, a) for n, r, a in rc.SYMBOLS}[name]
    want = [CTYPES.get(a, C.c_void_p) for a in PROTOTYPES[name]]
    if name == "rc_placed_primitive_bases":
        want[3] = C.POINTER(C.c_uint32)  # the count comes back through byref, like the exports'
    assert res is C.c_int and args == want
    assert hasattr(rc.lib(), name)


def test_the_declarations_move_no_cited_line():
    """tests/test_lifecycle_model.py cites header lines by number up to 725, and tests/test_ao_api.py wants the ambient-occlusion
    declarations to close the header: the four declarations sit between the two, behind the final gather."""
    lines = header().split("\n")
    first = next(i for i, l in enumerate(lines, 1) if "Form factors between instances" in l)
    assert first > 725
    names = re.findall(r"\bint\s+(rc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header(), flags=re.S))
    assert names[-7:] == ["rc_final_gather_device", "rc_placed_primitive_bases", "rc_placed_triangles_device", "rc_placed_view_factor_rays_device",
                          "rc_placed_view_factor_groups_device", "rc_ambient_occlusion_rays_device", "rc_ambient_occlusion_device"]


def test_header_documents_the_calls():
    text = header()
    at = text.index("int rc_placed_primitive_bases")
    comment = " ".join(text[text.rindex("/* ----", 0, at):at].replace("\n *", " ").split())
    for needle in ("A placed primitive is a pair (instance i, local primitive l)", "rc_export_instances' order and rc_hit::instance_id",
                   "the flat index is prims_offset(i) + l", "the traversal core reports prim = l + 1", "q = base[i] + l", "exclusive prefix sum",
                   "P = base[n_inst]", "built by the rebuilding rc_sync", "rc_update_geometry_device_async commits only on an equal face count",
                   "kept on the host and on the device", "re-derived by rc_scene_load", "A scene whose P reaches 2^32 keeps working for everything else",
                   "p_k = transform_point(T_i, v_k) in f32", "((m0 * x + m1 * y) + m2 * z) + m3", "no contraction", "FORWARD `transform`", "WHEN THE KERNEL RUNS",
                   "a mirroring instance flips it", "a non-uniform scale bends it correctly", "pt + normal * 0.01f in WORLD units",
                   "(ray_idx, flat primitive index, i, 0)", "word 2 is the only difference from the per-triangle family",
                   "instance 0 with an identity transform draws the sibling's numbers", "hits are found through `inv_transform`", "rc_add_instances_with_inverse",
                   "Singular transforms are outside the contract", "a = the source's q", "b = base[hit instance] + prim - 1", "ga = groups[a], gb = groups[b]",
                   "wa = weights ? weights[a] : 1", "A source with ga >= G contributes nothing", "A miss: escaped[ga] += wa, if escaped is given",
                   "A hit with b != a and gb < G: matrix[ga * G + gb] += wa", "Any other hit adds nothing", "u64 modulo 2^64",
                   "any partition of placed primitives x rays gives the same words", "P u32 each, indexed by q", "ACCUMULATE",
                   "item w = placed primitive placed_begin + w / n_ray, ray ray_begin + w % n_ray", "an empty range enqueues nothing", "1 <= n_groups <= 65535",
                   "fit 256 MiB", "Scratch is per stream", "has run the call eagerly once", "rc_update_transforms_device -> rc_refit_device_async",
                   "RC_ERR_NOT_SYNCED in the states in which rc_view_factor_groups_device returns it", 'docs/EXPERIMENTS.md, "Form factors between instances"'):
        assert needle in comment, needle


def test_python_surface(rc):
    assert list(inspect.signature(rc.TLAS.placed_primitive_bases).parameters) == ["self"]
    assert list(inspect.signature(rc.TLAS.placed_triangles_device).parameters) == ["self", "d_verts", "placed_begin", "n", "stream"]
    sig = inspect.signature(rc.TLAS.placed_view_factor_rays_device)
    assert list(sig.parameters) == ["self", "d_rays", "placed_prim", "n_rays", "seed", "sampling", "ray_begin", "stream"]
    sig = inspect.signature(rc.TLAS.placed_view_factor_groups_device)
    assert list(sig.parameters) == ["self", "groups_ptr", "n_groups", "matrix_ptr", "rays_per_triangle", "seed", "sampling", "weights_ptr", "escaped_ptr", "placed",
                                    "rays", "stream"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["sampling"], d["weights_ptr"], d["escaped_ptr"], d["placed"], d["rays"], d["stream"]) == ("uniform", None, None, None, None, None)
    sig = inspect.signature(rc.placed_view_factor_groups)
    assert list(sig.parameters) == ["accel", "groups", "rays_per_triangle", "seed", "weights", "sampling", "n_groups", "return_escaped"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["rays_per_triangle"], d["seed"], d["weights"], d["sampling"], d["n_groups"], d["return_escaped"]) == (10000, 0, None, "uniform", None, False)
    assert list(inspect.signature(rc.placed_form_factors).parameters) == ["accel", "groups", "rays_per_triangle", "seed", "n_groups"]
    sig = inspect.signature(rc.instance_form_factors)
    assert list(sig.parameters) == ["accel", "rays_per_triangle", "seed"] and sig.parameters["rays_per_triangle"].default == 10000
    assert list(inspect.signature(rc.placed_groups).parameters) == ["accel", "per_instance"]
    assert list(inspect.signature(rc.placed_primitive_count).parameters) == ["accel"]
    assert list(inspect.signature(rc.placed_primitive_areas).parameters) == ["accel"]


def test_julia_binding_and_the_documents():
    text = julia_text()
    docs = {f: open(os.path.join(ROOT, f)).read() for f in ("INTEGRATION.md", "README.md", "DESIGN.md")}
    for name, jl in JL_ARGS.items():
        m = re.search(r"ccall\(\(:" + name + r", LIB\), Cint,\s*\(([^)]*)\)", text)
        assert m, f"no ccall of {name}"
        assert [t.strip() for t in m.group(1).split(",")] == jl
        for f, doc in docs.items():
            assert name in doc, (name, f)
    assert re.search(r"^placed_view_factor_groups_device!\(a::MI355XStaticTLAS, rays_per_triangle::Integer, seed::UInt64, sampling::Integer, placed_begin::Integer,", text, flags=re.M)
    assert "sources of instanced scenes, which stay untransformed" not in docs["DESIGN.md"]


def test_invalid_arguments_are_refused_without_a_device(rc):
    L = rc.lib()
    n = C.c_uint32(7)
    assert L.rc_placed_primitive_bases(None, None, 0, C.byref(n)) == RC_ERR_INVALID_ARGUMENT and n.value == 7
    assert L.rc_placed_triangles_device(None, 0, 0, None, None) == RC_ERR_INVALID_ARGUMENT
    assert L.rc_placed_view_factor_rays_device(None, 0, 0, 0, 0, 4, 64, None) == RC_ERR_INVALID_ARGUMENT
    f = L.rc_placed_view_factor_groups_device
    assert f(None, 16, 0, 0, 0, 8, 0, 16, None, 1, None, None, None, None) == RC_ERR_INVALID_ARGUMENT
    assert f(None, 16, 0, 1, 0, 8, 0, 16, 64, 7, None, 64, None, None) == RC_ERR_INVALID_ARGUMENT


class NoDevice:
    """Stands where an accel is expected: any use of it is a failure -- the argument checks come first."""

    def __getattr__(self, name):
        raise AssertionError(f"the accel was touched ({name}) before the arguments were checked")


class Bases:
    """Stands where a synced TLAS is expected and answers placed_primitive_bases() only: three instances of 2, 5 and 1 primitives, so
    P = 8 where a flat primitive count would be something else."""
    device = 0

    def placed_primitive_bases(self):
        return np.array([0, 2, 7, 8], np.uint32)

    def __getattr__(self, name):
        raise AssertionError(f"the accel was touched ({name}) after a length error")


@pytest.fixture()
def fake_owner(rc, monkeypatch):
    from raycore_jl_amd import api
    monkeypatch.setattr(api, "_owner", lambda accel: accel)
    return Bases()


def test_placed_view_factor_groups_checks_its_arguments_without_a_device(rc):
    acc = NoDevice()
    g = np.arange(8, dtype=np.uint32) % 3
    for bad in (g.astype(np.float64), g.reshape(2, 4), np.array([0, -1]), np.array([0, 1 << 32]), np.array([True, False]), None):
        with pytest.raises(ValueError, match="groups"):
            rc.placed_view_factor_groups(acc, bad, 16)
    for bad in (g[:5], g.astype(np.float32), np.full(8, -1), np.full(8, 1 << 32, np.uint64)):
        with pytest.raises(ValueError, match="weights"):
            rc.placed_view_factor_groups(acc, g, 16, weights=bad)
    for bad in ("lambert", "", 2, -1, None, True, 0.0):
        with pytest.raises(ValueError, match="sampling"):
            rc.placed_view_factor_groups(acc, g, 16, sampling=bad)
    for bad in (0, 65536, -1, 2.0, True):
        with pytest.raises(ValueError, match="n_groups"):
            rc.placed_view_factor_groups(acc, g, 16, n_groups=bad)
        with pytest.raises(ValueError, match="n_groups"):
            rc.placed_form_factors(acc, g, 16, n_groups=bad)
    with pytest.raises(ValueError, match="n_groups"):  # the default: the largest group below 2^32 - 1, plus one
        rc.placed_view_factor_groups(acc, np.array([0, 65535], np.uint32), 16)
    for bad in (-1, 1 << 32, 1.5, True):
        with pytest.raises(ValueError, match="rays_per_triangle"):
            rc.placed_view_factor_groups(acc, g, bad)
    for bad in (-1, 1 << 64, 0.5):
        with pytest.raises(ValueError, match="seed"):
            rc.placed_form_factors(acc, g, seed=bad)
    no_scene = type("NoScene", (), {"_h": None})()  # the sampling name is refused while the arguments are put together
    with pytest.raises(ValueError, match="sampling"):
        rc.TLAS.placed_view_factor_groups_device(no_scene, 64, 2, 64, 16, 0, "lambert")
    with pytest.raises(ValueError, match="sampling"):
        rc.TLAS.placed_view_factor_rays_device(no_scene, 64, 0, 16, sampling=2)


def test_lengths_are_counted_in_placed_primitives(rc, fake_owner):
    for n in (3, 7, 9):  # 3 instances, not P = 8
        with pytest.raises(ValueError, match="one value per placed primitive: %d values for 8 placed primitives" % n):
            rc.placed_view_factor_groups(fake_owner, np.zeros(n, np.uint32), 16)
    assert rc.placed_primitive_count(fake_owner) == 8


def test_placed_groups_shapes(rc, fake_owner):
    g = rc.placed_groups(fake_owner)
    assert g.dtype == np.uint32 and np.array_equal(g, [0, 0, 1, 1, 1, 1, 1, 2])
    g = rc.placed_groups(fake_owner, [5, 0xFFFFFFFF, 5])
    assert g.dtype == np.uint32 and np.array_equal(g, [5, 5] + [0xFFFFFFFF] * 5 + [5])
    for bad in ([0, 1], [0, 1, 2, 3], np.zeros((3, 1), np.uint32), [0.0, 1.0, 2.0], [0, -1, 2]):
        with pytest.raises(ValueError, match="per_instance"):
            rc.placed_groups(fake_owner, bad)
    with pytest.raises(ValueError, match="per_instance"):
        rc.placed_groups(NoDevice(), [0.5])
    empty = type("Empty", (), {"placed_primitive_bases": lambda self: np.zeros(1, np.uint32)})()  # a synced scene without instances
    assert rc.placed_groups(empty).shape == (0,) and rc.placed_groups(empty, np.zeros(0, np.uint32)).dtype == np.uint32
