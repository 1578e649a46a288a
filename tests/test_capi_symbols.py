"""CPU-side checks of the drop-in boundary: the library loads, exports every symbol the header declares,
and refuses to compute without a GPU (no CPU fallback)."""
import os
import re
import subprocess

import pytest

from api_kit import header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rc():
    import raycore_jl_amd
    if not os.path.exists(raycore_jl_amd.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "raycore.jl_amd", "csrc"), "-s", "-j4"])
    return raycore_jl_amd


def header_symbols():
    text = header()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rc_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_what_binding_binds(rc):
    declared = header_symbols()
    bound = sorted(name for name, _, _ in rc.SYMBOLS)
    assert declared == bound


def test_library_exports_every_declared_symbol(rc):
    L = rc.lib()
    for name in header_symbols():
        assert hasattr(L, name), f"libraycore_mi355x.so does not export {name}"


def test_no_cpu_fallback_without_gpu(rc):
    if rc.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(rc.RaycoreError) as e:
        rc.TLAS(0)
    assert e.value.code == 3  # RC_ERR_NO_DEVICE
    assert "no CPU fallback" in str(e.value)


def test_product_does_not_link_oracle(rc):
    out = subprocess.run(["ldd", rc.LIB_PATH], capture_output=True, text=True).stdout
    assert "rc_oracle" not in out
    src = os.path.join(ROOT, "raycore.jl_amd")
    for dirpath, _, files in os.walk(src):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".jl")):
                text = open(os.path.join(dirpath, f)).read()
                for needle in ("pyoracle", "rc_oracle", "librc_oracle", "from oracle", "import oracle", "rco_"):
                    assert needle not in text, f"{f} references the oracle ({needle})"


def test_header_is_plain_c_and_example_links(rc, tmp_path):
    """The boundary is a C ABI: the header compiles as C11 and a C client links against the library (not run here: no GPU)."""
    exe = tmp_path / "trace_quad"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "trace_quad.c"),
                           "-L", os.path.dirname(rc.LIB_PATH), "-lraycore_mi355x", "-Wl,-rpath," + os.path.dirname(rc.LIB_PATH), "-o", str(exe)])
    if rc.device_count() == 0:
        r = subprocess.run([str(exe)], capture_output=True, text=True)
        assert r.returncode == 2 and "no GPU" in r.stderr


def test_c_struct_layouts_match_the_reference_records(rc, tmp_path):
    """The wire / export structs are the reference's records byte for byte: RTRay / RTHitResult 32 B (src/rt_transport.jl), BVHNode2 60 B,
    InstanceDescriptor 108 B, BLASDescriptor 32 B, Triangle{UInt32} 136 B, BVHNode4 120 B, ContactPair 8 B -- checked from C."""
    src = tmp_path / "sizes.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "raycore_mi355x.h"
#define CHECK(T, N) _Static_assert(sizeof(T) == N, #T " must be " #N " bytes")
CHECK(rc_ray, 32); CHECK(rc_hit, 32); CHECK(rc_bvh_node, 60); CHECK(rc_instance_desc, 108); CHECK(rc_blas_desc, 32);
CHECK(rc_prim, 40); CHECK(rc_triangle, 136); CHECK(rc_bvh4_node, 120); CHECK(rc_contact_pair, 8);
_Static_assert(offsetof(rc_hit, t) == 4 && offsetof(rc_hit, primitive_id) == 8 && offsetof(rc_hit, bary_u) == 16 && offsetof(rc_hit, instance_id) == 24, "RTHitResult fields");
_Static_assert(offsetof(rc_instance_desc, transform) == 8 && offsetof(rc_instance_desc, inv_transform) == 56 && offsetof(rc_instance_desc, flags) == 104, "InstanceDescriptor fields");
_Static_assert(offsetof(rc_triangle, normals) == 36 && offsetof(rc_triangle, tangents) == 72 && offsetof(rc_triangle, uv) == 108 && offsetof(rc_triangle, metadata) == 132, "Triangle fields");
_Static_assert(offsetof(rc_bvh4_node, aabb) == 16 && offsetof(rc_bvh4_node, parent) == 112 && offsetof(rc_bvh4_node, child_count) == 116, "BVHNode4 fields");
int main(void) { puts("ok"); return 0; }
''')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.run([str(exe)], capture_output=True, text=True).stdout.strip() == "ok"
