"""Final gather (rc_final_gather_device): the fused launch over hits x samples against the composed path, on full-size C3 (256 fan
spheres, 1 048 576 triangles).  The frame is 1 Mi primary HITS: the first 1 048 576 hit slots of a 2048 x 2048 pinhole view, gathered on
the device, so every slot carries work.  S = 4, 16 and 64 samples per hit, bias 1e-3, max_dist = inf and a tenth of the scene's diagonal;
x = one seeded full-range u32 per primitive, miss_value = 12345.

  A  composed : rc_ambient_occlusion_rays_device + ONE rc_trace_closest_device over the n * S rays + a torch reduction on the device (the
                t_max > 0 gate, hit -> flat primitive -> metadata -> x, the 1..N rule, the miss value, a sum over S in int64 and the open
                count), through n * S x 64 B of intermediate records
  B  fused    : a memset of the n sums and the n open counts + one rc_final_gather_device

Both sides run in this one process on one stream.  The outputs are compared first (zero differing sums, zero differing open counts);
then `--warmup` unrecorded rounds, then `--reps` recorded rounds with the sides alternating, each timed with two device events around
its whole sequence.  Reported per side: median, min, max and the 10th / 90th percentile (ms).

`--lib PATH --variant NAME`: load another build of the library (the sink with one plain u64 atomic per counted lane instead of wave_add,
say) and record the same rounds under "variants"[NAME] of `--out`, next to the shipped build's cases: side A is the same code in both
builds and is the yardstick of each run.  `--table` (no GPU) rewrites the tables between the final_gather markers of docs/EXPERIMENTS.md.

Usage: python tools/probes/final_gather_probe.py [--out profiles/final_gather.json] [--reps 30] [--warmup 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

BIAS = 1e-3
SEED = 0xA0
SAMPLES = (4, 16, 64)
N_HITS = 1 << 20
MISS = 12345
BEGIN, END = "<!-- final_gather:begin (tools/probes/final_gather_probe.py --table) -->", "<!-- final_gather:end -->"


def summary(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 4), "min": round(float(xs.min()), 4), "max": round(float(xs.max()), 4),
            "p10": round(float(np.percentile(xs, 10)), 4), "p90": round(float(np.percentile(xs, 90)), 4)}


class Setup:
    def __init__(self, lib_path=None):
        import torch

        import raycore_jl_amd as rc
        if lib_path:
            rc._capi.LIB_PATH = os.path.abspath(lib_path)  # (before the first call loads the library)
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
        self.n_prims = t.n_primitives()
        x = np.random.default_rng(7).integers(0, 1 << 32, self.n_prims, dtype=np.uint32)
        self.d_x = torch.from_numpy(x.view(np.int32).copy()).cuda()
        self.x64 = torch.from_numpy(x.astype(np.int64)).cuda()  # the composed side's lookup table, widened once
        self.prim_meta = torch.from_numpy(t.adapt().all_blas_prims["meta"].astype(np.int64)).cuda()
        self.sums = torch.zeros(n, dtype=torch.int64, device="cuda")
        self.open = torch.zeros(n, dtype=torch.int32, device="cuda")
        del all_rays, all_hits
        for buf in (self.d_rays, self.d_hits, self.d_x, self.x64, self.prim_meta, self.sums, self.open):
            buf.record_stream(s)
        torch.cuda.synchronize()

    def fused(self, S, dist):
        with self.torch.cuda.stream(self.s):
            self.sums.zero_()
            self.open.zero_()
        self.t.final_gather_device(self.d_rays.data_ptr(), self.d_hits.data_ptr(), self.n, S, self.d_x.data_ptr(), self.sums.data_ptr(),
                                   self.open.data_ptr(), miss_value=MISS, max_dist=dist, seed=SEED, bias=BIAS, stream=self.s.cuda_stream)


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
    g_rays = torch.zeros(total * 32, dtype=torch.uint8, device="cuda")
    g_hits = torch.zeros(total * 32, dtype=torch.uint8, device="cuda")
    composed_sums = torch.zeros(n, dtype=torch.int64, device="cuda")
    composed_open = torch.zeros(n, dtype=torch.int32, device="cuda")
    lit = u.d_hits.view(torch.int32).view(n, 8)[:, 0] != 0
    for buf in (g_rays, g_hits, composed_sums, composed_open):
        buf.record_stream(s)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()

    def composed():
        t.ambient_occlusion_rays_device(u.d_rays.data_ptr(), u.d_hits.data_ptr(), n, S, g_rays.data_ptr(), max_dist=dist, seed=SEED, bias=BIAS,
                                        stream=s.cuda_stream)
        t.trace_device(g_rays.data_ptr(), g_hits.data_ptr(), total, mode="closest", stream=s.cuda_stream)
        with torch.cuda.stream(s):
            tmax = g_rays.view(torch.float32).view(n, S, 8)[..., 7]
            rec = g_hits.view(torch.int32).view(n, S, 8)
            live = (tmax > 0) & lit[:, None]
            struck = live & (rec[..., 0] != 0)
            escaped = live & (rec[..., 0] == 0)
            prim = torch.where(struck, rec[..., 2], 0).to(torch.int64)  # (flat primitive index; 0 where there is no hit: masked below)
            m = u.prim_meta[prim]
            counted = struck & (m >= 1) & (m <= u.n_prims)
            value = torch.where(counted, u.x64[torch.where(counted, m - 1, 0)], 0) + escaped.to(torch.int64) * MISS
            torch.sum(value, dim=1, out=composed_sums)
            torch.sum(escaped, dim=1, dtype=torch.int32, out=composed_open)

    composed()
    u.fused(S, dist)
    s.synchronize()
    t.wait_for_gpu()
    reduction_peak = torch.cuda.max_memory_allocated() - base  # the torch reduction's temporaries, on top of the records
    differing = int((composed_sums != u.sums).sum().item()), int((composed_open != u.open).sum().item())
    assert differing == (0, 0), f"S = {S}, max_dist = {dist}: {differing} of {n} sums / open counts differ between the fused and the composed path"
    open_samples = int(u.open.to(torch.int64).sum().item())
    res = {"samples": S, "max_dist": "inf" if np.isinf(dist) else round(float(dist), 4), "items": total, "hits": n, "open_samples": open_samples,
           "open_fraction": round(open_samples / total, 4), "differing_sums": 0, "differing_open": 0}
    a_ms, b_ms = [], []
    for it in range(warmup + reps):
        a, b = timed(composed, s, torch), timed(lambda: u.fused(S, dist), s, torch)
        if it >= warmup:
            a_ms.append(a)
            b_ms.append(b)
    s.synchronize()
    t.wait_for_gpu()
    assert int((composed_sums != u.sums).sum().item()) == 0 and int((composed_open != u.open).sum().item()) == 0
    a, b = summary(a_ms), summary(b_ms)
    res.update({"a_composed_ms": a, "b_fused_ms": b, "b_over_a": round(b["median"] / a["median"], 4),
                "a_spread": round((a["p90"] - a["p10"]) / a["median"], 4), "b_spread": round((b["p90"] - b["p10"]) / b["median"], 4),
                "a_items_per_ns": round(total / (a["median"] * 1e6), 3), "b_items_per_ns": round(total / (b["median"] * 1e6), 3),
                "a_launches": "2 + the reduction's", "b_launches": "1 + two memsets", "a_intermediate_bytes": total * 64,
                "a_reduction_peak_bytes": int(reduction_peak), "b_output_bytes": n * 12})
    del g_rays, g_hits
    return res


def run_timing(args):
    u = Setup(args.lib)
    res = {"device": u.torch.cuda.get_device_name(0), "scene": "C3 (256 fan spheres, 1 048 576 triangles)", "primary_rays": u.primary_rays,
           "primary_hits": u.primary_hits, "hits_used": u.n, "scene_diagonal": round(u.diagonal, 4), "bias": BIAS, "seed": SEED, "miss_value": MISS,
           "reps": args.reps, "warmup": args.warmup, "cases": []}
    for S in args.samples or SAMPLES:
        for dist in (float("inf"), u.diagonal / 10.0):
            res["cases"].append(case(u, S, dist, args.warmup, args.reps))
            print(json.dumps(res["cases"][-1]), flush=True)
    u.t.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.variant:  # another build's rounds: kept next to the shipped build's, which must have been recorded first
        whole = json.load(open(args.out))
        whole.setdefault("variants", {})[args.variant] = res
        res = whole
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


def table(res):
    ms = lambda d: f"{d['median']:.3f} ms (min {d['min']:.3f}, p10–p90 {d['p10']:.3f}–{d['p90']:.3f})"  # noqa: E731
    lines = ["| S | max_dist | items | open samples | A composed | A's intermediates (+ reduction temporaries) | B fused | B / A | verdict |", "|---|---|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        verdict = "**fused is SLOWER than the composed path**" if c["b_over_a"] > 1.0 else "fused faster"
        if abs(c["b_over_a"] - 1.0) <= max(c["a_spread"], c["b_spread"]):
            verdict = "no difference shown (inside a side's own p10–p90 spread)"
        lines.append(f"| {c['samples']} | {c['max_dist']} | {c['items']:,} | {c['open_samples']:,} ({100 * c['open_fraction']:.1f} %) | "
                     f"{ms(c['a_composed_ms'])}, {c['a_items_per_ns']:.2f} items/ns | {c['a_intermediate_bytes'] / 2 ** 20:,.0f} MiB "
                     f"(+ {c['a_reduction_peak_bytes'] / 2 ** 20:,.0f} MiB) | {ms(c['b_fused_ms'])}, {c['b_items_per_ns']:.2f} items/ns | "
                     f"{c['b_over_a']:.3f} | {verdict} |")
    for name, v in res.get("variants", {}).items():
        lines += ["", f"Variant `{name}`, a run of its own with the same protocol (side A is the same code in both builds):", "",
                  f"| S | max_dist | A composed | B fused, {name} | B / A, {name} | B / A, shipped build | B {name} ÷ B shipped, each over its own run's A |",
                  "|---|---|---|---|---|---|---|"]
        for c, k in zip(v["cases"], res["cases"]):
            assert (c["samples"], c["max_dist"]) == (k["samples"], k["max_dist"])
            lines.append(f"| {c['samples']} | {c['max_dist']} | {ms(c['a_composed_ms'])} | {ms(c['b_fused_ms'])} | {c['b_over_a']:.3f} | {k['b_over_a']:.3f} | "
                         f"{c['b_over_a'] / k['b_over_a']:.3f} |")
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
    ap.add_argument("--out", default=os.path.join("profiles", "final_gather.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--samples", type=int, nargs="*", default=None, help="only these S")
    ap.add_argument("--lib", default=None, help="another build of libraycore_mi355x.so to load instead of the tree's")
    ap.add_argument("--variant", default=None, help="record this run under variants[NAME] of --out")
    ap.add_argument("--table", action="store_true")
    args = ap.parse_args()
    if args.table:
        return write_table(args)
    assert args.reps >= 20, "at least 20 repetitions per side"
    run_timing(args)


if __name__ == "__main__":
    main()
