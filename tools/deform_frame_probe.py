"""Deforming geometry: what a frame's geometry update + TLAS refit costs by each route.

  per scene, per frame:
    (a) host        : update (host soup, rc_update_geometry) + sync   -- upload, three host waits, reallocation of the flat arrays, a
                      structural rebuild; the only route before rc_update_geometry_device_async, measured in the same run
    (b) async eager : update_geometry_device_async + refit_device_async on the probe's stream  -- no host wait
    (c) async graph : (b) captured once, replayed
  scenes: one BLAS of 100 000 random triangles under 64 instances; the C3 sphere BLAS (4 096 triangles) under 256 instances.
  "wall_ms" is host time from the first call until the work is done (for (b) / (c) that includes a stream synchronise the frame itself
  does not need); "enqueue_ms" is host time until the calls have returned; "device_ms" ((b) / (c)): two events of the probe's own around
  the calls on its stream, idle gaps between the kernels included.  (a) has none: rc_sync's rebuild is not timed by the library as a whole.

Every route gets a new soup every frame from the same stand-in deformation (a uniform scale about the origin, alternating up and down: no
face becomes degenerate), outside the timed region.  Every case: `--warmup` unrecorded runs, then `--reps` recorded ones; min and median.

`--trace-frames K` instead runs K eager frames of (b) on the first scene and exits: the run to put under
`rocprofv3 --kernel-trace --stats` for the dispatch count and the per-kernel times of one update.

Usage: python tools/deform_frame_probe.py [--out profiles/deform_frame.json] [--reps 30] [--warmup 5]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import raycore_jl_amd as rc  # noqa: E402
from dynamic_frame_probe import measure  # noqa: E402

sc = rc.scenes
SCALES = (np.float32(1.01), np.float32(1.0) / np.float32(1.01))


def scenes():
    g = np.random.default_rng(11)
    xf = np.tile(sc.IDENTITY3x4, (64, 1)).astype(np.float32)
    xf[:, [3, 7, 11]] = (g.random((64, 3)) * 8).astype(np.float32)
    yield "blas_100k_triangles_64_instances", sc.random_triangles(100_000, 7), xf
    cfg = sc.config_c3()
    (verts, _), = cfg["blas"]
    (_, xf3, _), = cfg["instances"]
    yield "c3_sphere_blas_256_instances", verts, np.ascontiguousarray(xf3, dtype=np.float32).reshape(-1, 12)


def build(soup, xf):
    t = rc.TLAS(0)
    h = t.push(soup, xf)
    t.sync()
    return t, h


def cases(soup, xf, warmup, reps):
    out = {"triangles": int(len(soup)), "instances": int(len(xf))}
    t, h = build(soup, xf)
    state = {"soup": soup.copy(), "k": 0}

    def host_step():
        state["soup"] *= SCALES[state["k"] % 2]
        state["k"] += 1

    def host_frame():
        t.update(h, state["soup"])
        t.sync()

    out["a_host_update_sync"] = measure(host_frame, t.wait_for_gpu, None, warmup, reps, prepare=host_step)
    t.free()

    t, h = build(soup, xf)
    s = torch.cuda.Stream()
    d_soup = torch.from_numpy(soup).cuda()
    d_soup.record_stream(s)
    torch.cuda.synchronize()
    state["k"] = 0

    def device_step():
        d_soup.mul_(float(SCALES[state["k"] % 2]))
        state["k"] += 1

    def async_frame():
        t.update_geometry_device_async(h, d_soup, stream=s.cuda_stream)
        t.refit_device_async(stream=s.cuda_stream)

    dev = lambda ev: ev[0].elapsed_time(ev[1])  # noqa: E731
    out["b_async_eager"] = measure(async_frame, s.synchronize, dev, warmup, reps, stream=s, prepare=device_step)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        async_frame()

    def replay():
        with torch.cuda.stream(s):
            graph.replay()

    out["c_async_graph_replay"] = measure(replay, s.synchronize, dev, warmup, reps, stream=s, prepare=device_step)
    a = out["a_host_update_sync"]
    for key in ("b_async_eager", "c_async_graph_replay"):
        out[key]["wall_vs_a"] = round(out[key]["wall_ms"]["median"] / a["wall_ms"]["median"], 3)
    t.wait_for_gpu()  # (raises if an update was refused: the face count is kept by construction)
    del graph
    torch.cuda.synchronize()
    t.set_option("release_captures", 1)
    d = t.adapt().blas_descriptors[0]  # the lazy read-back of the root box still works after all of it
    out["root_box_after"] = [float(x) for x in np.concatenate([d["root_min"], d["root_max"]])]
    t.free()
    return out


def trace_frames(k):
    name, soup, xf = next(scenes())
    t, h = build(soup, xf)
    s = torch.cuda.Stream()
    d_soup = torch.from_numpy(soup).cuda()
    d_soup.record_stream(s)
    torch.cuda.synchronize()
    for _ in range(k):
        t.update_geometry_device_async(h, d_soup, stream=s.cuda_stream)
        t.refit_device_async(stream=s.cuda_stream)
        s.synchronize()
    t.wait_for_gpu()
    print(f"{k} eager frames of update_geometry_device_async + refit_device_async on {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "deform_frame.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace-frames", type=int, default=0)
    args = ap.parse_args()
    if args.trace_frames:
        trace_frames(args.trace_frames)
        return
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup}
    for name, soup, xf in scenes():
        res[name] = cases(soup, xf, args.warmup, args.reps)
        for k, v in res[name].items():
            print(name, k, json.dumps(v), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
