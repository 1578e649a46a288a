"""Dev (GPU): device time of the persistent drivers for one build of the library, for A/B runs of two builds in one job (tools/ab_build.sh
builds a variant into tools/ab/):

    python tools/probes/driver_shapes_probe.py                      # the in-tree library
    python tools/probes/driver_shapes_probe.py tools/ab/parent.so

    python tools/probes/driver_shapes_probe.py tools/ab/parent.so totals gather     # only the workloads whose name holds one of the words

Workloads: get_illumination on full-size C3 (256 instances: top level in LDS) with a 2048 x 2048 grid, the bench's C3 ray count;
view_factor_totals, view_factors, view_factor_products, view_factor_groups (11 bodies, both samplings) and view_factors_sparse on a reduced
C5 (5 420 triangles, 1024 rays per triangle = 5.5 M rays, under a second per call); soft shadows (4 lights), ambient occlusion and the
final gather over the first 1 Mi hit slots of a 2048 x 2048 view of C3 with 4 samples; 16 point sources at grid 256 in C3.  Every workload
runs in the scene's default shell and once more with option "kernel" = 3 (the plain shell).  Each is warmed up, then repeated; per
workload one JSON line with the median / min / max of rc_last_kernel_ms (the launches' own device events; of a call with several
launches, the last one's) and of the wall time per call.  Fails without a GPU."""
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


def c3_workloads(cfg, t3):
    """The device-array workloads on C3: (name, call) pairs; a call zeroes its accumulators, runs and returns them as numpy arrays."""
    import torch
    n, S, L = 1 << 20, 4, 4
    rays = rc.scenes.c3_primary_rays(cfg, 2048, 2048)
    all_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).cuda()
    all_hits = torch.zeros(len(rays) * 32, dtype=torch.uint8, device="cuda")
    t3.trace_device(all_rays.data_ptr(), all_hits.data_ptr(), len(rays))
    torch.cuda.synchronize()
    idx = torch.nonzero(all_hits.view(torch.int32).view(-1, 8)[:, 0] != 0)[:, 0][:n]
    assert idx.numel() == n, f"the view has only {idx.numel()} hits"
    d_rays, d_hits = all_rays.view(-1, 32)[idx].contiguous().view(-1), all_hits.view(-1, 32)[idx].contiguous().view(-1)
    del all_rays, all_hits
    c, e = cfg["lattice_centre"], (np.array((8, 8, 4)) - 1) * 1.5
    lights = np.array([cfg["light"], c + (-e[0], 0.6 * e[1], -e[2] - 6.0), c + (0.0, -1.5 * e[1], -e[2]), c + (0.1 * e[0], 2.5 * e[1], 0.2 * e[2])], np.float32)
    d_lights, d_radii = torch.from_numpy(lights).cuda(), torch.ones(L, dtype=torch.float32, device="cuda")
    N = t3.n_primitives()
    d_x = torch.from_numpy(np.random.default_rng(7).integers(0, 1 << 32, N, dtype=np.uint32).view(np.int32).copy()).cuda()
    counts = torch.zeros(n * L, dtype=torch.int32, device="cuda")
    sums, opened = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    g = np.random.default_rng(0x9051)
    lo, hi = np.asarray(cfg["centres"], np.float64).min(axis=0), np.asarray(cfg["centres"], np.float64).max(axis=0)
    src = rc.point_sources(g.uniform(lo, hi, (16, 3)).astype(np.float32))
    d_src = torch.from_numpy(src.view(np.uint8).reshape(-1).copy()).cuda()
    rows, escaped = torch.zeros(16 * N, dtype=torch.int32, device="cuda"), torch.zeros(16, dtype=torch.int32, device="cuda")

    def done(*bufs):
        torch.cuda.synchronize()
        return tuple(b.cpu().numpy() for b in bufs)

    def soft():
        counts.zero_()
        t3.soft_shadow_visibility_device(d_rays.data_ptr(), d_hits.data_ptr(), n, d_lights.data_ptr(), d_radii.data_ptr(), L, S, counts.data_ptr(), seed=5, bias=1e-3)
        return done(counts)

    def ao():
        counts.zero_()
        t3.ambient_occlusion_device(d_rays.data_ptr(), d_hits.data_ptr(), n, S, counts.data_ptr(), seed=5, bias=1e-3)
        return done(counts[:n])

    def gather():
        sums.zero_(), opened.zero_()
        t3.final_gather_device(d_rays.data_ptr(), d_hits.data_ptr(), n, S, d_x.data_ptr(), sums.data_ptr(), opened.data_ptr(), miss_value=12345, seed=5, bias=1e-3)
        return done(sums, opened)

    def points():
        rows.zero_(), escaped.zero_()
        t3.illumination_points_device(d_src.data_ptr(), 16, 256, rows.data_ptr(), N, escaped.data_ptr(), seed=5)
        return done(rows, escaped)

    return [("soft_shadow_visibility C3 1Mi hits x 4 lights x 4", soft), ("ambient_occlusion C3 1Mi hits x 4", ao),
            ("final_gather C3 1Mi hits x 4", gather), ("illumination_points C3 16 x 256^2", points)]


def main():
    assert rc.device_count() > 0, "no GPU visible: nothing is measured on a CPU"
    label, words = "in-tree", sys.argv[2:]
    if len(sys.argv) > 1 and sys.argv[1] != "-":  # ("-": the in-tree library, with a choice of workloads)
        sys.modules[rc.lib.__module__].LIB_PATH = os.path.abspath(sys.argv[1])
        label = os.path.basename(sys.argv[1])

    def run(name, t, call, warmup, reps=20):
        if words and not any(w in name for w in words):
            return
        for shell, kernel in (("default", -1), ("plain", 3)):
            t.set_option("kernel", kernel)
            measure(label, f"{name} [{shell}]", t, call, warmup, reps)
        t.set_option("kernel", -1)

    sc = rc.scenes
    cfg3 = sc.config_c3()
    t3 = build(cfg3)
    run("get_illumination C3 2048x2048", t3, lambda: (rc.get_illumination(t3, (0.2, -0.1, 1.0), 2048),), 5)
    if not words or any(w in name for w in words for name in ("soft_shadow_visibility", "ambient_occlusion", "final_gather", "illumination_points")):
        for name, call in c3_workloads(cfg3, t3):
            run(name, t3, call, 3)
    t3.free()
    t5 = build(sc.config_c5(lon=32, bands=17, wall_k=5))
    assert t5.n_primitives() == 5420
    run("view_factor_totals C5/5420 x 1024", t5, lambda: rc.view_factor_totals(t5, 1024, 7), 3)
    out = np.empty((5420, 5420), np.uint32, order="F")
    run("view_factors C5/5420 x 1024", t5, lambda: (rc.view_factors(t5, 1024, 7, out=out),), 3)
    x = np.random.default_rng(7).integers(0, 1 << 32, 5420, dtype=np.uint32)
    run("view_factor_products C5/5420 x 1024", t5, lambda: rc.view_factor_products(t5, x, 1024, 7), 3)
    per_sphere, per_wall = 2 * 32 * 16, 2 * 5 * 5  # config_c5's bodies in the order of its metadata: 5 spheres, then 6 walls
    bodies = np.concatenate([np.repeat(np.arange(5, dtype=np.uint32), per_sphere), 5 + np.repeat(np.arange(6, dtype=np.uint32), per_wall)])
    for sampling in ("uniform", "cosine"):
        run(f"view_factor_groups {sampling} C5/5420 x 1024, 11 bodies", t5, lambda: rc.view_factor_groups(t5, bodies, 1024, 7, sampling=sampling, return_escaped=True), 3)
    run("view_factors_sparse C5/5420 x 1024", t5, lambda: tuple(rc.view_factors_sparse(t5, 1024, 7)[:3]), 3)
    t5.free()


if __name__ == "__main__":
    main()
