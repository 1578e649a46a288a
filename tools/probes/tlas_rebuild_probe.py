"""The device-side TLAS rebuild (rebuild_device_async): what it costs next to the asynchronous refit and to the structural sync it replaces,
and what it buys an animation that carries instances far from where they were sorted.  Conventions of tools/dynamic_frame_probe.py: both
sides of every comparison run in this one process on one device; every case has `--warmup` unrecorded runs, then `--reps` recorded ones; min
and median are reported.

  cost, for n = 256 (the C3 scene), 864 (a 12 x 12 x 6 lattice of fan spheres) and 5 000 instances, per frame on the probe's stream:
    refit          : update_transforms_device + refit_device_async
    rebuild_chain  : update_transforms_device + rebuild_device_async with tlas_rebuild_fused = 0 (the build's chain of kernels)
    rebuild_fused  : the same with tlas_rebuild_fused = 1 (one workgroup; n <= 256 only)
  each eager and as a graph replay.  "device_ms": two events of the probe's own around the calls on its stream, idle gaps between the
  kernels included; "enqueue_ms": host time until the calls have returned; "wall_ms": until a stream synchronise has returned as well.
    sync_rebuild   : host wall time of the structural rc_sync over the same instances (the handle deleted and pushed again, outside the
                     timed region): upload of the mirror, flat arrays, build, root read-back.

  quality, on C3: the 256 instances exchange lattice positions under a seeded permutation.  The 4 Mi-ray primary trace (rc_last_kernel_ms)
  and the summed surface area of the TLAS's internal boxes relative to the root's (numpy, from rc_export_tlas_nodes) for three trees:
  built fresh with the permuted transforms, the original tree refitted to them, and the original tree rebuilt on the device.

  auto (refit_or_rebuild_device_async, the rebuild gated on the device; written to --auto-out), same scenes, same conventions, per frame
  update_transforms_device + one of
    auto_refits    : the conditional call on a frame that merely drifts (the gate stays clear; checked on tlas_quality's rebuild counter)
    auto_rebuilds  : the conditional call on a frame whose translations were permuted among the instances just before (the gate opens)
    refit / rebuild: refit_device_async / rebuild_device_async on the same drifting frames, measured in the same run -- the yardsticks
  on both device paths where both exist (n <= 256: tlas_rebuild_fused 1 and 0), eager and as a graph replay; and `cost_only`:
  tlas_cost_device alone.
  curve, on C3: the relative cost (numpy and tlas_cost_device) and the 4 Mi-ray trace time of the REFITTED tree after exchanging the
  positions of 0, 1/8, 1/4, 1/2 and all of the instances -- what a default ratio can be chosen from.

Usage: python tools/probes/tlas_rebuild_probe.py [--out profiles/tlas_rebuild.json] [--auto-out profiles/tlas_auto_rebuild.json]
                                                 [--only all|rebuild|auto] [--reps 30] [--warmup 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

import raycore_jl_amd as rc  # noqa: E402

sc = rc.scenes


def summary(xs):
    return {"min": round(float(np.min(xs)), 4), "median": round(float(np.median(xs)), 4)}


def measure(frame, finish, warmup, reps, stream=None, prepare=None):
    wall, enq, dev = [], [], []
    for it in range(warmup + reps):
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        if prepare is not None:
            prepare()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if stream is not None:
            ev[0].record(stream)
        frame()
        if stream is not None:
            ev[1].record(stream)
        t1 = time.perf_counter()
        finish()
        t2 = time.perf_counter()
        if it >= warmup:
            enq.append((t1 - t0) * 1e3)
            wall.append((t2 - t0) * 1e3)
            if stream is not None:
                dev.append(ev[0].elapsed_time(ev[1]))
    out = {"wall_ms": summary(wall), "enqueue_ms": summary(enq)}
    if dev:
        out["device_ms"] = summary(dev)
    return out


def scene_of(n):
    """(mesh, transforms) of the n-instance scene."""
    if n == 256:
        cfg = sc.config_c3()
        return cfg["blas"][0][0], np.ascontiguousarray(cfg["instances"][0][1], dtype=np.float32).reshape(-1, 12)
    if n == 864:
        return sc.fan_sphere(10, 6, radius=0.5), sc.lattice_transforms(12, 12, 6, 1.6, 3)[0]
    g = np.random.default_rng(5)
    xf = np.tile(sc.IDENTITY3x4, (n, 1)).astype(np.float32)
    xf[:, [3, 7, 11]] = (g.random((n, 3)) * 40).astype(np.float32)
    return sc.fan_sphere(16, 9), xf


def cost_cases(n, warmup, reps):
    mesh, xf = scene_of(n)
    t = rc.TLAS(0)
    blas = t.add_geometry(mesh)
    h = t.push_instances(blas, xf, np.arange(n, dtype=np.uint32))
    t.sync()
    out = {"instances": n, "tlas_top_k": int(t.get_option("tlas_top_k"))}
    s = torch.cuda.Stream()
    d_xf = torch.from_numpy(xf).cuda()
    d_xf.record_stream(s)
    torch.cuda.synchronize()

    def device_step():  # the stand-in physics step: not timed, the same for every route
        d_xf[:, 3] += 0.01

    def run_case(name, commit):
        def frame():
            t.update_transforms_device(h, d_xf, stream=s.cuda_stream)
            commit(stream=s.cuda_stream)

        out[name + "_eager"] = measure(frame, s.synchronize, warmup, reps, stream=s, prepare=device_step)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            frame()

        def replay():
            with torch.cuda.stream(s):
                graph.replay()

        out[name + "_graph_replay"] = measure(replay, s.synchronize, warmup, reps, stream=s, prepare=device_step)
        del graph
        torch.cuda.synchronize()
        t.set_option("release_captures", 1)

    run_case("refit", t.refit_device_async)
    t.set_option("tlas_rebuild_fused", 0)
    run_case("rebuild_chain", t.rebuild_device_async)
    if n <= 256:
        t.set_option("tlas_rebuild_fused", 1)
        run_case("rebuild_fused", t.rebuild_device_async)
    t.sync()
    state = {"h": h}
    host_xf = t.get_instances(h)["transform"].copy()

    def repush():
        t.delete(state["h"])
        state["h"] = t.push_instances(blas, host_xf, np.arange(n, dtype=np.uint32))

    def structural_sync():
        t.sync()
        assert t.last_sync_action == "rebuild"

    out["sync_rebuild"] = measure(structural_sync, t.wait_for_gpu, warmup, reps, prepare=repush)
    t.free()
    return out


def relative_area(nodes, n):
    """Summed surface area of the boxes of the n - 1 internal nodes (union of the two child boxes), relative to the root's."""
    lo = np.minimum(nodes["aabb0_min"][:n - 1], nodes["aabb1_min"][:n - 1]).astype(np.float64)
    hi = np.maximum(nodes["aabb0_max"][:n - 1], nodes["aabb1_max"][:n - 1]).astype(np.float64)
    e = hi - lo
    area = 2.0 * (e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0])
    return float(area.sum() / area[0])


def quality_case(warmup, reps):
    cfg = sc.config_c3()
    mesh, meta = cfg["blas"][0]
    xf = np.ascontiguousarray(cfg["instances"][0][1], dtype=np.float32).reshape(-1, 12)
    ids = cfg["instances"][0][2]
    n = len(xf)
    perm = sc.rng(0xC3 + 17).permutation(n)
    moved = xf.reshape(n, 3, 4).copy()
    moved[:, :, 3] = moved[perm][:, :, 3]
    moved = np.ascontiguousarray(moved.reshape(n, 12))
    rays = sc.c3_primary_rays(cfg)
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).cuda()
    d_hits = torch.zeros(len(rays) * 32, dtype=torch.uint8, device="cuda")
    d_moved = torch.from_numpy(moved).cuda()
    s = torch.cuda.Stream()
    for buf in (d_rays, d_hits, d_moved):
        buf.record_stream(s)
    torch.cuda.synchronize()

    def build(transforms):
        t = rc.TLAS(0)
        b = t.add_geometry(mesh, meta)
        return t, t.push_instances(b, transforms, ids)

    def trace_ms(t):
        ms = []
        for it in range(warmup + reps):
            t.trace_device(d_rays.data_ptr(), d_hits.data_ptr(), len(rays), stream=s.cuda_stream)
            s.synchronize()
            if it >= warmup:
                ms.append(t.last_kernel_ms())
        return summary(ms), d_hits.cpu().numpy().tobytes()

    out = {"scene": "C3 (256 fan spheres, 1 048 576 triangles), lattice positions exchanged under rng(0xC3 + 17).permutation(256)",
           "rays": int(len(rays))}
    t0, _ = build(xf)
    t0.sync()
    ms, _ = trace_ms(t0)
    out["original_scene"] = {"trace_ms": ms, "relative_area": round(relative_area(t0.adapt().nodes, n), 3)}
    t0.free()
    fresh, _ = build(moved)
    fresh.sync()
    ms, hits_fresh = trace_ms(fresh)
    nodes_fresh = fresh.adapt().nodes
    out["built_fresh"] = {"trace_ms": ms, "relative_area": round(relative_area(nodes_fresh, n), 3)}
    t, h = build(xf)
    t.sync()
    t.update_transforms_device(h, d_moved, stream=s.cuda_stream)
    t.refit_device_async(stream=s.cuda_stream)
    ms, hits_refit = trace_ms(t)
    out["refit_only"] = {"trace_ms": ms, "relative_area": round(relative_area(t.adapt().nodes, n), 3)}
    for fused in (1, 0):
        t.set_option("tlas_rebuild_fused", fused)
        t.rebuild_device_async(stream=s.cuda_stream)
        ms, hits_rebuilt = trace_ms(t)
        nodes = t.adapt().nodes
        out["rebuilt_fused" if fused else "rebuilt_chain"] = {
            "trace_ms": ms, "relative_area": round(relative_area(nodes, n), 3),
            "nodes_equal_built_fresh": nodes.tobytes() == nodes_fresh.tobytes(), "hits_equal_built_fresh": hits_rebuilt == hits_fresh}
    out["refit_only"]["hit_records_differing_from_built_fresh"] = int(np.count_nonzero(np.any(
        np.frombuffer(hits_refit, np.uint32).reshape(-1, 8) != np.frombuffer(hits_fresh, np.uint32).reshape(-1, 8), axis=1)))
    fresh.free()
    t.free()
    return out


AUTO_RATIO = 1.5


def auto_cases(n, warmup, reps):
    """The conditional call next to the plain refit and the unconditional rebuild, on both device paths."""
    mesh, xf = scene_of(n)
    out = {"instances": n, "ratio": AUTO_RATIO}
    s = torch.cuda.Stream()
    for fused in ((1, 0) if n <= 256 else (0,)):
        t = rc.TLAS(0)
        blas = t.add_geometry(mesh)
        h = t.push_instances(blas, xf, np.arange(n, dtype=np.uint32))
        t.sync()
        t.set_option("tlas_rebuild_fused", fused)
        d_xf = torch.from_numpy(xf).cuda()
        d_xf.record_stream(s)
        d_cost = torch.zeros(1, dtype=torch.float64, device="cuda")
        d_cost.record_stream(s)
        torch.cuda.synchronize()
        path = "fused" if fused else "chain"

        def drift():  # the stand-in physics step of a frame that does not rebuild: not timed
            d_xf[:, 3] += 0.01

        def scatter():  # ... and of one that does: the translation columns permuted among the instances
            m = d_xf.view(n, 3, 4)
            m[:, :, 3] = m[torch.randperm(n, device="cuda")][:, :, 3]

        def run_case(name, commit, prepare, expect_rebuilds):
            def frame():
                t.update_transforms_device(h, d_xf, stream=s.cuda_stream)
                commit()

            for mode in ("eager", "graph_replay"):
                graph = None
                run = frame
                if mode == "graph_replay":
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph, stream=s):
                        frame()

                    def run():
                        with torch.cuda.stream(s):
                            graph.replay()
                before = t.tlas_quality()["rebuilds"]
                r = measure(run, s.synchronize, warmup, reps, stream=s, prepare=prepare)
                if expect_rebuilds is not None:
                    r["rebuilds_taken"] = t.tlas_quality()["rebuilds"] - before
                    r["rebuilds_expected"] = (warmup + reps) if expect_rebuilds else 0
                out[f"{name}_{path}_{mode}"] = r
                if graph is not None:
                    del graph
                    torch.cuda.synchronize()
                    t.set_option("release_captures", 1)

        run_case("refit", lambda: t.refit_device_async(stream=s.cuda_stream), drift, None)
        run_case("rebuild", lambda: t.rebuild_device_async(stream=s.cuda_stream), drift, None)
        t.refit_or_rebuild_device_async(AUTO_RATIO, stream=s.cuda_stream)  # arms; the two yardsticks above ran unarmed, as on the parent commit
        s.synchronize()
        run_case("auto_refits", lambda: t.refit_or_rebuild_device_async(AUTO_RATIO, stream=s.cuda_stream), drift, False)
        run_case("auto_rebuilds", lambda: t.refit_or_rebuild_device_async(AUTO_RATIO, stream=s.cuda_stream), scatter, True)
        if fused == 0:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ms = []
            for it in range(warmup + reps):
                torch.cuda.synchronize()
                ev[0].record(s)
                t.tlas_cost_device(d_cost, stream=s.cuda_stream)
                ev[1].record(s)
                s.synchronize()
                if it >= warmup:
                    ms.append(ev[0].elapsed_time(ev[1]))
            out["cost_only_device_ms"] = summary(ms)
        t.free()
    return out


def curve_case(warmup, reps):
    """C3, refit only: cost and trace time against the fraction of instances whose lattice positions were exchanged."""
    cfg = sc.config_c3()
    mesh, meta = cfg["blas"][0]
    xf = np.ascontiguousarray(cfg["instances"][0][1], dtype=np.float32).reshape(-1, 12)
    ids = cfg["instances"][0][2]
    n = len(xf)
    rays = sc.c3_primary_rays(cfg)
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).cuda()
    d_hits = torch.zeros(len(rays) * 32, dtype=torch.uint8, device="cuda")
    d_cost = torch.zeros(1, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    for buf in (d_rays, d_hits, d_cost):
        buf.record_stream(s)
    out = {"scene": "C3 (256 fan spheres), a seeded subset of the instances exchanges lattice positions, refit only", "rays": int(len(rays)), "points": []}
    base = None
    for frac in (0.0, 0.125, 0.25, 0.5, 1.0):
        k = int(round(frac * n))
        g = sc.rng(0xC3 + 31)
        subset = np.sort(g.permutation(n)[:k])
        moved = xf.reshape(n, 3, 4).copy()
        if k:
            moved[subset, :, 3] = moved[subset[g.permutation(k)]][:, :, 3]
        moved = np.ascontiguousarray(moved.reshape(n, 12))
        t = rc.TLAS(0)
        h = t.push_instances(t.add_geometry(mesh, meta), xf, ids)
        t.sync()
        d_moved = torch.from_numpy(moved).cuda()
        d_moved.record_stream(s)
        torch.cuda.synchronize()
        t.update_transforms_device(h, d_moved, stream=s.cuda_stream)
        t.refit_device_async(stream=s.cuda_stream)
        t.tlas_cost_device(d_cost, stream=s.cuda_stream)
        ms = []
        for it in range(warmup + reps):
            t.trace_device(d_rays.data_ptr(), d_hits.data_ptr(), len(rays), stream=s.cuda_stream)
            s.synchronize()
            if it >= warmup:
                ms.append(t.last_kernel_ms())
        area = relative_area(t.adapt().nodes, n)
        base = area if base is None else base
        out["points"].append({"fraction_exchanged": frac, "instances_moved": int(np.count_nonzero(np.any(moved != xf, axis=1))),
                              "relative_area": round(area, 3), "device_cost": round(float(d_cost.cpu()[0]), 3),
                              "cost_over_original": round(area / base, 3), "trace_ms": summary(ms)})
        t.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "tlas_rebuild.json"))
    ap.add_argument("--auto-out", default=os.path.join("profiles", "tlas_auto_rebuild.json"))
    ap.add_argument("--only", choices=("all", "rebuild", "auto"), default="all")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    head = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup}
    if args.only in ("all", "rebuild"):
        res = dict(head, cost=[])
        for n in (256, 864, 5000):
            res["cost"].append(cost_cases(n, args.warmup, args.reps))
            print(json.dumps(res["cost"][-1]), flush=True)
        res["quality_c3"] = quality_case(args.warmup, args.reps)
        print(json.dumps(res["quality_c3"]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    if args.only in ("all", "auto"):
        res = dict(head, auto=[])
        for n in (256, 864, 5000):
            res["auto"].append(auto_cases(n, args.warmup, args.reps))
            print(json.dumps(res["auto"][-1]), flush=True)
        res["curve_c3"] = curve_case(args.warmup, args.reps)
        print(json.dumps(res["curve_c3"]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.auto_out)), exist_ok=True)
        with open(args.auto_out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
