"""Shadow visibility of all hits x all lights: the fused launch against the composed stages, on full-size C3 (256 fan spheres, 1 048 576
triangles), 2048 x 2048 pinhole primary rays, the bench's shadow workload (point light (10, 10, 10), bias 1e-3), with L = 1 and L = 4 lights
(the bench's light first, then three more around the lattice).

  A  composed : L x (rc_shadow_rays_device + rc_trace_any_device), each light into its own ray and hit buffers (L x n x 64 B), as a
                caller who shades with all lights has to keep them
  B  fused    : one rc_shadow_visibility_device into n x L bytes

Both run in this one process on one stream.  The outputs are compared first (B's bytes against hits.hit & ~shadow_hits.hit of A); then
`--warmup` unrecorded rounds of A and B, then `--reps` recorded rounds, A and B alternating, each timed with two device events around its
whole sequence.  Reported per side: median, min, max and the 10th / 90th percentile (ms); "b_over_a" is the ratio of the medians, and
"a_spread" = (p90 - p10) / median of A is the yardstick a difference has to beat.  Fails without a GPU.

Usage: python tools/probes/shadow_visibility_probe.py [--out profiles/shadow_visibility.json] [--reps 30] [--warmup 5]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

import raycore_jl_amd as rc  # noqa: E402

BIAS = 1e-3


def summary(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 4), "min": round(float(xs.min()), 4), "max": round(float(xs.max()), 4),
            "p10": round(float(np.percentile(xs, 10)), 4), "p90": round(float(np.percentile(xs, 90)), 4)}


def timed(fn, s):
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record(s)
    fn()
    ev[1].record(s)
    s.synchronize()
    return ev[0].elapsed_time(ev[1])


def case(t, d_rays, d_hits, n, lights, s, warmup, reps):
    L = len(lights)
    st = s.cuda_stream
    d_lights = torch.from_numpy(np.ascontiguousarray(lights, dtype=np.float32)).cuda()
    shadow_rays = [torch.zeros(n * 32, dtype=torch.uint8, device="cuda") for _ in range(L)]
    shadow_hits = [torch.zeros(n * 32, dtype=torch.uint8, device="cuda") for _ in range(L)]
    visible = torch.full((n * L,), 0xAB, dtype=torch.uint8, device="cuda")
    for buf in shadow_rays + shadow_hits + [visible, d_lights]:
        buf.record_stream(s)
    torch.cuda.synchronize()

    def composed():
        for l in range(L):
            t.shadow_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), n, lights[l], shadow_rays[l].data_ptr(), bias=BIAS, stream=st)
            t.trace_device(shadow_rays[l].data_ptr(), shadow_hits[l].data_ptr(), n, mode="any", stream=st)

    def fused():
        t.shadow_visibility_device(d_rays.data_ptr(), d_hits.data_ptr(), n, d_lights.data_ptr(), L, visible.data_ptr(), bias=BIAS, stream=st)

    composed()
    fused()
    s.synchronize()
    t.wait_for_gpu()
    lit = d_hits.view(torch.int32).view(n, 8)[:, 0] != 0
    want = torch.stack([lit & (h.view(torch.int32).view(n, 8)[:, 0] == 0) for h in shadow_hits], dim=1).to(torch.uint8).reshape(-1)
    differing = int((want != visible).sum().item())
    assert differing == 0, f"L = {L}: {differing} of {n * L} bytes differ between the fused and the composed path"
    a_ms, b_ms = [], []
    for it in range(warmup + reps):
        a, b = timed(composed, s), timed(fused, s)
        if it >= warmup:
            a_ms.append(a)
            b_ms.append(b)
    a, b = summary(a_ms), summary(b_ms)
    hits = int(lit.sum().item())
    return {"lights": L, "items": n * L, "primary_hits": hits, "visible_pairs": int(visible.sum().item()), "outputs_agree": True,
            "a_composed_ms": a, "b_fused_ms": b, "b_over_a": round(b["median"] / a["median"], 4),
            "a_spread": round((a["p90"] - a["p10"]) / a["median"], 4), "b_spread": round((b["p90"] - b["p10"]) / b["median"], 4),
            "a_launches": 2 * L, "b_launches": 1, "a_intermediate_bytes": n * L * 64, "b_output_bytes": n * L}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "shadow_visibility.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert args.reps >= 20, "at least 20 repetitions per side"
    assert rc.device_count() > 0, "no GPU visible: nothing is measured on a CPU"
    cfg = rc.scenes.config_c3()
    t = rc.TLAS(0)
    for verts, meta in cfg["blas"]:
        t.add_geometry(verts, meta)
    for b, xf, ids in cfg["instances"]:
        t.push_instances(b, xf, ids)
    t.sync()
    rays = rc.scenes.c3_primary_rays(cfg)
    n = len(rays)
    s = torch.cuda.Stream()
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).cuda()
    d_hits = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    for buf in (d_rays, d_hits):
        buf.record_stream(s)
    torch.cuda.synchronize()
    t.trace_device(d_rays.data_ptr(), d_hits.data_ptr(), n, stream=s.cuda_stream)
    s.synchronize()
    c, e = cfg["lattice_centre"], (np.array((8, 8, 4)) - 1) * 1.5
    lights = np.array([cfg["light"], c + (-e[0], 0.6 * e[1], -e[2] - 6.0), c + (0.0, -1.5 * e[1], -e[2]), c + (0.1 * e[0], 2.5 * e[1], 0.2 * e[2])], np.float32)
    res = {"device": torch.cuda.get_device_name(0), "scene": "C3 (256 fan spheres, 1 048 576 triangles)", "rays": n, "bias": BIAS,
           "lights": lights.tolist(), "reps": args.reps, "warmup": args.warmup, "cases": []}
    for L in (1, 4):
        res["cases"].append(case(t, d_rays, d_hits, n, lights[:L], s, args.warmup, args.reps))
        print(json.dumps(res["cases"][-1]), flush=True)
    t.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
