"""Ambient occlusion (rc_ambient_occlusion_device): the fused launch over hits x samples against the composed path, on full-size C3 (256
fan spheres, 1 048 576 triangles).  The frame is 1 Mi primary HITS: the first 1 048 576 hit slots of a 2048 x 2048 pinhole view, gathered on
the device, so every slot carries work.  S = 4 and 16 samples per hit, bias 1e-3, max_dist = inf and a tenth of the scene's diagonal.

  A  composed : rc_ambient_occlusion_rays_device + ONE rc_trace_any_device over the n * S rays + a torch reduction (the t_max > 0 gate, the
                hit flag and a sum over S), through n * S x 64 B of intermediate records
  B  fused    : a memset of the n counts + one rc_ambient_occlusion_device

Both sides run in this one process on one stream.  The outputs are compared first (zero differing counts); then `--warmup` unrecorded
rounds, then `--reps` recorded rounds with the sides alternating, each timed with two device events around its whole sequence.  Reported
per side: median, min, max and the 10th / 90th percentile (ms).  Then the same rounds twice more, with what only side A's trace kernel has
switched off step by step: option "cost_order" 0 (the probe replays one ray buffer, which lets the any-hit trace claim its chunks in the
order learned from the round before -- something a frame that draws new samples every time does not give it -- while the fused launch
claims in natural order), then also "stack16" 0 (the trace kernel in the drivers' shape: 32-bit lane-stack entries, fewer node planes in
LDS).  Writes `--out`.  `--table` (no GPU) rewrites the table between the
ambient_occlusion markers of docs/EXPERIMENTS.md from `--out`.

Usage: python tools/probes/ambient_occlusion_probe.py [--out profiles/ambient_occlusion.json] [--reps 30] [--warmup 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

BIAS = 1e-3
SEED = 0xA0
SAMPLES = (4, 16)
N_HITS = 1 << 20
BEGIN, END = "<!-- ambient_occlusion:begin (tools/probes/ambient_occlusion_probe.py --table) -->", "<!-- ambient_occlusion:end -->"


def summary(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 4), "min": round(float(xs.min()), 4), "max": round(float(xs.max()), 4),
            "p10": round(float(np.percentile(xs, 10)), 4), "p90": round(float(np.percentile(xs, 90)), 4)}


class Setup:
    def __init__(self):
        import torch

        import raycore_jl_amd as rc
        assert rc.device_count() > 0, "no GPU visible: nothing is measured on a CPU"
        self.torch = torch
        cfg = rc.scenes.config_c3()
        self.t = t = rc.TLAS(0)
        for verts, meta in cfg["blas"]:
            t.add_geometry(verts, meta)
        for b, xf, ids in cfg["instances"]:
            t.push_instances(b, xf, ids)
        t.sync()
        wb = t.world_bound()
        self.diagonal = float(np.linalg.norm(np.asarray(wb.p_max, np.float64) - np.asarray(wb.p_min, np.float64)))
        rays = rc.scenes.c3_primary_rays(cfg, 2048, 2048)
        self.s = s = torch.cuda.Stream()
        all_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).cuda()
        all_hits = torch.zeros(len(rays) * 32, dtype=torch.uint8, device="cuda")
        t.trace_device(all_rays.data_ptr(), all_hits.data_ptr(), len(rays))
        torch.cuda.synchronize()
        idx = torch.nonzero(all_hits.view(torch.int32).view(-1, 8)[:, 0] != 0)[:, 0]
        self.primary_rays, self.primary_hits = len(rays), int(idx.numel())
        assert idx.numel() >= N_HITS, f"the view has only {idx.numel()} hits"
        idx = idx[:N_HITS]
        self.n = n = N_HITS
        self.d_rays = all_rays.view(-1, 32)[idx].contiguous().view(-1)
        self.d_hits = all_hits.view(-1, 32)[idx].contiguous().view(-1)
        self.counts = torch.zeros(n, dtype=torch.int32, device="cuda")
        del all_rays, all_hits
        for buf in (self.d_rays, self.d_hits, self.counts):
            buf.record_stream(s)
        torch.cuda.synchronize()

    def fused(self, S, dist):
        with self.torch.cuda.stream(self.s):
            self.counts.zero_()
        self.t.ambient_occlusion_device(self.d_rays.data_ptr(), self.d_hits.data_ptr(), self.n, S, self.counts.data_ptr(), max_dist=dist, seed=SEED,
                                        bias=BIAS, stream=self.s.cuda_stream)


def timed(fn, s, torch):
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record(s)
    fn()
    ev[1].record(s)
    s.synchronize()
    return ev[0].elapsed_time(ev[1])


def case(u, S, dist, warmup, reps):
    torch, t, n, s = u.torch, u.t, u.n, u.s
    total = n * S
    ao_rays = torch.zeros(total * 32, dtype=torch.uint8, device="cuda")
    ao_hits = torch.zeros(total * 32, dtype=torch.uint8, device="cuda")
    composed_counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    lit = u.d_hits.view(torch.int32).view(n, 8)[:, 0] != 0
    for buf in (ao_rays, ao_hits, composed_counts):
        buf.record_stream(s)
    torch.cuda.synchronize()

    def composed():
        t.ambient_occlusion_rays_device(u.d_rays.data_ptr(), u.d_hits.data_ptr(), n, S, ao_rays.data_ptr(), max_dist=dist, seed=SEED, bias=BIAS,
                                        stream=s.cuda_stream)
        t.trace_device(ao_rays.data_ptr(), ao_hits.data_ptr(), total, mode="any", stream=s.cuda_stream)
        with torch.cuda.stream(s):
            tmax = ao_rays.view(torch.float32).view(n, S, 8)[..., 7]
            blocked = ao_hits.view(torch.int32).view(n, S, 8)[..., 0]
            seen = (tmax > 0) & (blocked == 0) & lit[:, None]
            torch.sum(seen, dim=1, dtype=torch.int32, out=composed_counts)

    composed()
    u.fused(S, dist)
    s.synchronize()
    t.wait_for_gpu()
    differing = int((composed_counts != u.counts).sum().item())
    assert differing == 0, f"S = {S}, max_dist = {dist}: {differing} of {n} counts differ between the fused and the composed path"
    visible_samples = int(u.counts.to(torch.int64).sum().item())
    res = {"samples": S, "max_dist": "inf" if np.isinf(dist) else round(float(dist), 4), "items": total, "hits": n, "visible_samples": visible_samples,
           "visible_fraction": round(visible_samples / total, 4), "differing_counts": 0}
    a_ms, b_ms = [], []
    for it in range(warmup + reps):
        a, b = timed(composed, s, torch), timed(lambda: u.fused(S, dist), s, torch)
        if it >= warmup:
            a_ms.append(a)
            b_ms.append(b)
    a, b = summary(a_ms), summary(b_ms)
    res.update({"a_composed_ms": a, "b_fused_ms": b, "b_over_a": round(b["median"] / a["median"], 4),
                "a_spread": round((a["p90"] - a["p10"]) / a["median"], 4), "b_spread": round((b["p90"] - b["p10"]) / b["median"], 4),
                "a_items_per_ns": round(total / (a["median"] * 1e6), 3), "b_items_per_ns": round(total / (b["median"] * 1e6), 3),
                "a_launches": "2 + the reduction's", "b_launches": "1 + a memset", "a_intermediate_bytes": total * 64, "b_output_bytes": n * 4})
    # The same again with what only side A's trace kernel has switched off, step by step; the fused launch takes neither option.
    #   "cost_order" 0: the probe replays one ray buffer, so the any-hit trace claims its chunks in the order learned from the round before
    #                   -- something a frame that draws new samples does not give it; the drivers always claim in natural order
    #   "stack16" 0   : the trace kernel in the drivers' shape (32-bit lane-stack entries, fewer node planes in LDS)
    for key, options in (("natural_order", {"cost_order": 0}), ("natural_order_32bit_stack", {"cost_order": 0, "stack16": 0})):
        before = {k: t.get_option(k) for k in options}
        for k, v in options.items():
            t.set_option(k, v)
        try:
            a_ms, b_ms = [], []
            for it in range(warmup + reps):
                a, b = timed(composed, s, torch), timed(lambda: u.fused(S, dist), s, torch)
                if it >= warmup:
                    a_ms.append(a)
                    b_ms.append(b)
            s.synchronize()
            t.wait_for_gpu()
            assert int((composed_counts != u.counts).sum().item()) == 0
        finally:
            for k, v in before.items():
                t.set_option(k, v)
        a, b = summary(a_ms), summary(b_ms)
        res.update({f"a_{key}_ms": a, f"b_next_to_{key}_ms": b, f"b_over_a_{key}": round(b["median"] / a["median"], 4)})
    del ao_rays, ao_hits
    return res


def run_timing(args):
    u = Setup()
    res = {"device": u.torch.cuda.get_device_name(0), "scene": "C3 (256 fan spheres, 1 048 576 triangles)", "primary_rays": u.primary_rays,
           "primary_hits": u.primary_hits, "hits_used": u.n, "scene_diagonal": round(u.diagonal, 4), "bias": BIAS, "seed": SEED, "reps": args.reps,
           "warmup": args.warmup, "cases": []}
    for S in args.samples or SAMPLES:
        for dist in (float("inf"), u.diagonal / 10.0):
            if args.reach != "both" and (args.reach == "inf") != np.isinf(dist):
                continue
            res["cases"].append(case(u, S, dist, args.warmup, args.reps))
            print(json.dumps(res["cases"][-1]), flush=True)
    u.t.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


def table(res):
    ms = lambda d: f"{d['median']:.3f} ms (min {d['min']:.3f}, p10–p90 {d['p10']:.3f}–{d['p90']:.3f})"  # noqa: E731
    lines = ["| S | max_dist | items | visible samples | A composed | B fused | B / A | verdict | A with `cost_order` 0; B next to it | B / A | "
             "A with `cost_order` 0 and `stack16` 0; B next to it | B / A |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        verdict = "**fused is SLOWER than the composed path**" if c["b_over_a"] > 1.0 else "fused faster"
        if abs(c["b_over_a"] - 1.0) <= max(c["a_spread"], c["b_spread"]):
            verdict = "no difference shown (inside a side's own p10–p90 spread)"
        lines.append(f"| {c['samples']} | {c['max_dist']} | {c['items']:,} | {c['visible_samples']:,} ({100 * c['visible_fraction']:.1f} %) | "
                     f"{ms(c['a_composed_ms'])}, {c['a_items_per_ns']:.2f} items/ns, {c['a_intermediate_bytes'] / 2 ** 20:,.0f} MiB of intermediates | "
                     f"{ms(c['b_fused_ms'])}, {c['b_items_per_ns']:.2f} items/ns | {c['b_over_a']:.2f} | {verdict} | "
                     f"{ms(c['a_natural_order_ms'])}; {ms(c['b_next_to_natural_order_ms'])} | {c['b_over_a_natural_order']:.2f} | "
                     f"{ms(c['a_natural_order_32bit_stack_ms'])}; {ms(c['b_next_to_natural_order_32bit_stack_ms'])} | "
                     f"{c['b_over_a_natural_order_32bit_stack']:.2f} |")
    return "\n".join(lines)


def write_table(args):
    res = json.load(open(args.out))
    path = os.path.join(ROOT, "docs", "EXPERIMENTS.md")
    text = open(path).read()
    a, b = text.index(BEGIN) + len(BEGIN), text.index(END)
    with open(path, "w") as f:
        f.write(text[:a] + "\n" + table(res) + "\n" + text[b:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "ambient_occlusion.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--samples", type=int, nargs="*", default=None, help="only these S (a kernel trace of one case: rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--reach", choices=("both", "inf", "tenth"), default="both", help="only this max_dist")
    ap.add_argument("--table", action="store_true")
    args = ap.parse_args()
    if args.table:
        return write_table(args)
    assert args.reps >= 20, "at least 20 repetitions per side"
    run_timing(args)


if __name__ == "__main__":
    main()
