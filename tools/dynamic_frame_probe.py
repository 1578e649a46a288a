"""Animating instances: what a frame's transform update + TLAS refit costs by each route, and what it adds to a wavefront frame.

  refit, 5 000 instances (the scene of bench.py's tlas_refit_5000_instances extra), per frame:
    (a) host        : update_transforms (host array) + sync                                   -- upload, five passes, root read-back
    (b) alias       : descriptors rewritten through the instance_buffer alias by a torch scatter, host wait, refit_device(recompute_inverse)
    (c) async eager : update_transforms_device + refit_device_async on the probe's stream      -- no host wait
    (d) async graph : (c) captured once, replayed
  (a) and (b) exist without the asynchronous entry points and are the baseline, measured in the same run.  "wall_ms" is host time from the
  first call until the work is done (for (c) / (d) that includes a stream synchronise the frame itself does not need); "enqueue_ms" is
  host time until the calls have returned.  "device_ms": (b) runs on the scene's own stream, so it is the scene's own event pair
  around rc_refit_device's kernels (rc_last_kernel_ms: without the scatter; bench.py's refit_device_kernels_ms); (a) has none (rc_sync's
  refit is not timed by the library); (c) / (d) are two events of the probe's own around the calls on its stream, idle gaps between the
  kernels included.

  frame: WavefrontPaths on C3 at 720 x 400 x 4 spp, depth 2 -- static, and with dynamic=[(handle, transforms)] (update + refit in front
  of the primary rays), eager and as a graph replay, events around each frame.

Every route gets new transforms every frame from the same stand-in physics step, outside the timed region.
Every case: `--warmup` unrecorded runs, then `--reps` recorded ones; min and median are reported.

Usage: python tools/dynamic_frame_probe.py [--out profiles/dynamic_frame.json] [--reps 30] [--warmup 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import raycore_jl_amd as rc  # noqa: E402

sc = rc.scenes


def summary(xs):
    return {"min": round(float(np.min(xs)), 4), "median": round(float(np.median(xs)), 4)}


def measure(frame, finish, device_ms, warmup, reps, stream=None, prepare=None):
    """prepare() produces the frame's transforms (the stand-in for a physics step: not timed, the same for every route), frame() enqueues
    one frame, finish() waits for it; device_ms(events) -> the frame's device time."""
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
            if device_ms is not None:
                dev.append(device_ms(ev))
    out = {"wall_ms": summary(wall), "enqueue_ms": summary(enq)}
    if dev:
        out["device_ms"] = summary(dev)
    return out


def refit_cases(warmup, reps):
    g = np.random.default_rng(5)
    n = 5000
    xf = np.tile(sc.IDENTITY3x4, (n, 1)).astype(np.float32)
    xf[:, [3, 7, 11]] = (g.random((n, 3)) * 40).astype(np.float32)
    t = rc.TLAS(0)
    h = t.push(sc.fan_sphere(16, 9), xf)
    t.sync()
    out = {"instances": n}
    state = {"xf": xf.copy()}

    def host_step():
        state["xf"][:, 3] += 0.01

    def host_frame():
        t.update_transforms(h, state["xf"])
        t.sync()

    out["a_host_update_sync"] = measure(host_frame, t.wait_for_gpu, None, warmup, reps, prepare=host_step)  # (rc_sync's refit is not timed by the library)

    ptr, cnt = t.instance_buffer(h)

    class Alias:
        __cuda_array_interface__ = {"shape": (cnt, 27), "typestr": "<f4", "data": (ptr, False), "version": 2}

    recs = torch.as_tensor(Alias(), device="cuda")
    d_xf = torch.from_numpy(state["xf"]).cuda()

    def device_step():
        d_xf[:, 3] += 0.01

    def alias_frame():
        recs[:, 2:14] = d_xf
        torch.cuda.current_stream().synchronize()  # the refit runs on the scene's own stream: the host orders it behind the scatter
        t.refit_device(recompute_inverse=True)

    out["b_alias_refit_device"] = measure(alias_frame, t.wait_for_gpu, lambda ev: t.last_kernel_ms(), warmup, reps, prepare=device_step)

    s = torch.cuda.Stream()
    d_xf.record_stream(s)
    torch.cuda.synchronize()

    def async_frame():
        t.update_transforms_device(h, d_xf, stream=s.cuda_stream)
        t.refit_device_async(stream=s.cuda_stream)

    out["c_async_eager"] = measure(async_frame, s.synchronize, lambda ev: ev[0].elapsed_time(ev[1]), warmup, reps, stream=s, prepare=device_step)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        async_frame()

    def replay():
        with torch.cuda.stream(s):
            graph.replay()

    out["d_async_graph_replay"] = measure(replay, s.synchronize, lambda ev: ev[0].elapsed_time(ev[1]), warmup, reps, stream=s, prepare=device_step)
    b = out["b_alias_refit_device"]
    for key in ("c_async_eager", "d_async_graph_replay"):
        out[key]["wall_vs_b"] = round(out[key]["wall_ms"]["median"] / b["wall_ms"]["median"], 3)
        out[key]["device_vs_b_kernels"] = round(out[key]["device_ms"]["median"] / b["device_ms"]["median"], 3)
    del graph
    torch.cuda.synchronize()
    t.set_option("release_captures", 1)
    bound = t.world_bound()  # the lazy read-back still works after all of it
    out["world_bound_after"] = [float(x) for x in np.concatenate([bound.p_min, bound.p_max])]
    t.free()
    return out


def frame_cases(warmup, reps):
    cfg = sc.config_c3()
    t = rc.TLAS(0)
    for verts, meta in cfg["blas"]:
        t.add_geometry(verts, meta)
    handles = [(t.push_instances(b, xf, ids), xf) for b, xf, ids in cfg["instances"]]
    t.sync()
    w, h, spp, depth = 720, 400, 4, 2
    cam = rc.wavefront.lookat_camera(cfg["eye"], cfg["lattice_centre"], w, h, 45.0)
    light = cfg["light"].astype(np.float32)
    rows = []
    for dynamic in (False, True):
        s = torch.cuda.Stream()
        dyn = [(hd, torch.from_numpy(np.ascontiguousarray(xf, dtype=np.float32).reshape(-1, 12)).cuda()) for hd, xf in handles] if dynamic else None
        torch.cuda.synchronize()
        wf = rc.wavefront.WavefrontPaths(t, w, h, spp, depth, cam, light, seed=0xF00D, dynamic=dyn)
        r = measure(lambda: wf.run(s), s.synchronize, lambda ev: ev[0].elapsed_time(ev[1]), warmup, reps, stream=s)
        rows.append(dict(r, dynamic=dynamic, mode="eager", instances=sum(len(x) for _, x in handles), traced_slots=wf.traced_rays()))
        wf.capture(s)

        def replay():
            with torch.cuda.stream(s):
                wf.replay()

        r = measure(replay, s.synchronize, lambda ev: ev[0].elapsed_time(ev[1]), warmup, reps, stream=s)
        rows.append(dict(r, dynamic=dynamic, mode="graph replay", instances=sum(len(x) for _, x in handles), traced_slots=wf.traced_rays()))
        torch.cuda.synchronize()
        del wf
        t.set_option("release_captures", 1)
        print(json.dumps(rows[-2]), "\n", json.dumps(rows[-1]), flush=True)
    t.free()
    return {"width": w, "height": h, "spp": spp, "depth": depth, "scene": "C3 (256 fan spheres, 1 048 576 triangles)", "cases": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "dynamic_frame.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup}
    res["refit_5000_instances"] = refit_cases(args.warmup, args.reps)
    for k, v in res["refit_5000_instances"].items():
        print(k, json.dumps(v), flush=True)
    res["wavefront_frame"] = frame_cases(args.warmup, args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
