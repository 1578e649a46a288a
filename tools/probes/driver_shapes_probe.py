"""Dev (GPU): device time of the persistent drivers for one build of the library, for A/B runs of two builds in one job (tools/ab_build.sh
builds a variant into tools/ab/):

    python tools/probes/driver_shapes_probe.py                      # the in-tree library
    python tools/probes/driver_shapes_probe.py tools/ab/parent.so

Workloads: get_illumination on full-size C3 (256 instances: top level in LDS) with a 2048 x 2048 grid, the bench's C3 ray count;
view_factor_totals and view_factors on a reduced C5 (5 420 triangles, 1024 rays per triangle = 5.5 M rays, under a second per call).
Each is warmed up, then repeated; per workload one JSON line with the median / min / max of rc_last_kernel_ms (the launches' own device
events) and of the wall time per call.  Fails without a GPU."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import raycore_jl_amd as rc  # noqa: E402


def build(cfg):
    t = rc.TLAS(0)
    for verts, meta in cfg["blas"]:
        t.add_geometry(verts, meta)
    for b, xf, ids in cfg["instances"]:
        t.push_instances(b, xf, ids)
    return t.sync()


def measure(label, name, t, call, warmup, reps):
    for _ in range(warmup):
        ref = call()
    dev_ms, wall_ms = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(t.last_kernel_ms())
        assert all(np.array_equal(a, b) for a, b in zip(out, ref)), f"{name}: the result changed between calls"
    row = {"build": label, "workload": name, "reps": reps}
    for key, xs in (("device_ms", dev_ms), ("wall_ms", wall_ms)):
        row[key] = {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4)}
    row["checksum"] = int(sum(int(np.asarray(a, np.float64).sum()) for a in out))
    print(json.dumps(row), flush=True)


def main():
    assert rc.device_count() > 0, "no GPU visible: nothing is measured on a CPU"
    label = "in-tree"
    if len(sys.argv) > 1:
        sys.modules[rc.lib.__module__].LIB_PATH = os.path.abspath(sys.argv[1])
        label = os.path.basename(sys.argv[1])
    sc = rc.scenes
    t3 = build(sc.config_c3())
    measure(label, "get_illumination C3 2048x2048", t3, lambda: (rc.get_illumination(t3, (0.2, -0.1, 1.0), 2048),), 5, 20)
    t3.free()
    t5 = build(sc.config_c5(lon=32, bands=17, wall_k=5))
    assert t5.n_primitives() == 5420
    measure(label, "view_factor_totals C5/5420 x 1024", t5, lambda: rc.view_factor_totals(t5, 1024, 7), 3, 20)
    out = np.empty((5420, 5420), np.uint32, order="F")
    measure(label, "view_factors C5/5420 x 1024", t5, lambda: (rc.view_factors(t5, 1024, 7, out=out),), 3, 20)
    t5.free()


if __name__ == "__main__":
    main()
