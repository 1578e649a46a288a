"""The diffuse bounce stage (rc_bounce_rays_device) and the chained wavefront frame (raycore.jl_amd/wavefront.py) on C3, timed with HIP
events on one stream.  The first launch of every case is reported on its own; the rest are the mean / min of the repeats.

  bounce stage : 4 Mi slots slot-aligned from C3's 2048^2 primary hits; 16 Mi slots round robin (C4 made on the device: compaction +
                 bounce, each timed).  "requested_bytes" counts what the kernel loads and stores: per slot the hit record (32 B) and the
                 output ray (32 B); per LIVE slot also the source ray (32 B), the hit primitive (36 B of its 40), the instance's inverse
                 3x4 (48 B) and the source index (4 B) when gathered.  Under wrap every source is requested n_out / count times and served
                 from L2 / Infinity Cache after the first, so the rate there is above what HBM could deliver; "unique_bytes" counts each
                 source once.
  C4 trace     : closest_hit over the 16 Mi device-made bounce rays next to the host-made rays of the bench (scenes.c4_bounce_rays).
                 NOT the same workload: the device rays start on the faceted geometric normal, the bench's on the analytic sphere normal.
  frame        : WavefrontPaths at 720 x 400 x 4 spp depth 3 and 2048^2 x 1 spp depth 2, eager and as a graph replay, with and without
                 compaction; "traced" counts every traced slot (primary + shadow per depth + bounce), dead slots included.

Usage: python tools/wavefront_probe.py [--out profiles/wavefront_frame.json] [--reps 10]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import raycore_jl_amd as rc  # noqa: E402

sc = rc.scenes


def timed(fn, reps):
    """(first launch ms, [repeat ms]) of fn() on the current stream, HIP events around each call."""
    out = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out[0], out[1:]


def stats(first, rest, **extra):
    d = {"first_ms": round(first, 4), "mean_ms": round(float(np.mean(rest)), 4), "min_ms": round(float(np.min(rest)), 4)}
    d.update(extra)
    return d


def bounce_bytes(n_out, n_live, gathered):
    return n_out * (32 + 32) + n_live * (32 + 36 + 48 + (4 if gathered else 0))


def byte_stats(by, unique, ms):
    return {"requested_bytes": by, "requested_GBps_at_mean": round(by / ms / 1e6, 1), "unique_bytes": unique,
            "unique_GBps_at_mean": round(unique / ms / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "wavefront_frame.json"))
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    reps = args.reps
    cfg = sc.config_c3()
    t = rc.TLAS(0)
    for verts, meta in cfg["blas"]:
        t.add_geometry(verts, meta)
    for b, xf, ids in cfg["instances"]:
        t.push_instances(b, xf, ids)
    t.sync()
    res = {"scene": "C3 (256 fan spheres, 1 048 576 triangles)", "device": torch.cuda.get_device_name(0), "reps": reps}

    rays = sc.c3_primary_rays(cfg, 2048, 2048)
    n = len(rays)
    d_r = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()
    d_h = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    t.trace_device(d_r.data_ptr(), d_h.data_ptr(), n)
    torch.cuda.synchronize()
    hits = d_h.cpu().numpy().view(rc.HIT_DT)
    live = int(hits["hit"].sum())
    res["primary"] = {"rays": n, "hits": live}

    # ---- the bounce stage ----
    d_b4 = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    first, rest = timed(lambda: t.bounce_rays_device(d_r.data_ptr(), d_h.data_ptr(), n, d_b4.data_ptr(), seed=0xC3, bounce=0), reps)
    by = bounce_bytes(n, live, False)
    res["bounce_4Mi_slot_aligned"] = stats(first, rest, slots=n, live=live, **byte_stats(by, by, np.mean(rest)))
    n4 = 16 * 2 ** 20
    d_b16 = torch.empty(n4 * 32, dtype=torch.uint8, device="cuda")
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    cnt = torch.empty(1, dtype=torch.int32, device="cuda")
    first_c, rest_c = timed(lambda: t.compact_hits_device(d_h.data_ptr(), n, idx.data_ptr(), cnt.data_ptr()), reps)
    first, rest = timed(lambda: t.bounce_rays_device(d_r.data_ptr(), d_h.data_ptr(), n4, d_b16.data_ptr(), seed=0xC4, d_src=idx.data_ptr(),
                                                     d_src_count=cnt.data_ptr(), wrap=True), reps)
    by = bounce_bytes(n4, n4, True)
    unique = n4 * 32 + n * 32 + live * (32 + 36 + 48 + 4)  # outputs, every hit record once, each live source once
    res["compact_4Mi"] = stats(first_c, rest_c)
    res["bounce_16Mi_wrap_c4"] = stats(first, rest, slots=n4, live=n4, sources=live, **byte_stats(by, unique, np.mean(rest)))

    # ---- C4 trace: device-made vs host-made rays ----
    d_hb = torch.empty(n4 * 32, dtype=torch.uint8, device="cuda")
    first, rest = timed(lambda: t.trace_device(d_b16.data_ptr(), d_hb.data_ptr(), n4), reps)
    res["c4_trace_device_made_rays"] = stats(first, rest, rays=n4, Grays_per_s_at_mean=round(n4 / np.mean(rest) / 1e6, 3),
                                             Grays_per_s_first=round(n4 / first / 1e6, 3), normals="faceted geometric (hit_frame)")
    del d_b16
    host_c4 = sc.c4_bounce_rays(cfg, rays, hits, n4)
    d_c4 = torch.from_numpy(host_c4.view(np.uint8).reshape(-1)).cuda()
    del host_c4
    first, rest = timed(lambda: t.trace_device(d_c4.data_ptr(), d_hb.data_ptr(), n4), reps)
    res["c4_trace_host_made_rays"] = stats(first, rest, rays=n4, Grays_per_s_at_mean=round(n4 / np.mean(rest) / 1e6, 3),
                                           Grays_per_s_first=round(n4 / first / 1e6, 3), normals="analytic sphere (scenes.c4_bounce_rays)",
                                           bench_headline_Grays_per_s=5.71)
    del d_c4, d_hb, d_b4
    torch.cuda.synchronize()
    torch.cuda.empty_cache()

    # ---- chained frames ----
    frames = []
    light = cfg["light"].astype(np.float32)
    for (w, h, spp, depth) in ((720, 400, 4, 3), (2048, 2048, 1, 2)):
        cam = rc.wavefront.lookat_camera(cfg["eye"], cfg["lattice_centre"], w, h, 45.0)
        for compact in (False, True):
            s = torch.cuda.Stream()
            wf = rc.wavefront.WavefrontPaths(t, w, h, spp, depth, cam, light, seed=0xF00D, compact=compact)
            with torch.cuda.stream(s):
                first, rest = timed(lambda: wf.run(s), reps)
            traced = wf.traced_rays()
            alive = [int((wf.path_ids[b] != -1).sum().item()) for b in range(depth)]
            frames.append(dict(stats(first, rest), width=w, height=h, spp=spp, depth=depth, compact=compact, mode="eager", traced_slots=traced,
                               live_paths_per_depth=alive, Grays_per_s_at_mean=round(traced / np.mean(rest) / 1e6, 3)))
            torch.cuda.synchronize()
            wf.capture(s)
            with torch.cuda.stream(s):
                first, rest = timed(wf.replay, reps)
            frames.append(dict(stats(first, rest), width=w, height=h, spp=spp, depth=depth, compact=compact, mode="graph replay",
                               traced_slots=traced, Grays_per_s_at_mean=round(traced / np.mean(rest) / 1e6, 3)))
            torch.cuda.synchronize()
            del wf
            torch.cuda.synchronize()
            t.set_option("release_captures", 1)  # the graph is gone: its captured launches can be handed out again
            torch.cuda.empty_cache()
            print(json.dumps(frames[-2]), "\n", json.dumps(frames[-1]), flush=True)
    res["frames"] = frames
    for k in ("bounce_4Mi_slot_aligned", "compact_4Mi", "bounce_16Mi_wrap_c4", "c4_trace_device_made_rays", "c4_trace_host_made_rays"):
        print(k, json.dumps(res[k]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    t.free()


if __name__ == "__main__":
    main()
