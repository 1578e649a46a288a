"""Soft shadows (rc_soft_shadow_visibility_device): the fused launch over hits x lights x samples against the composed path, on full-size
C3 (256 fan spheres, 1 048 576 triangles), 1024 x 1024 pinhole primary rays, L = 4 lights (the bench's light first, then three more around
the lattice) of radius 1, bias 1e-3, S = 1, 4 and 16 samples per (hit, light).

  A  composed : rc_soft_shadow_rays_device + ONE rc_trace_any_device over the n * L * S rays + a torch reduction (the t_max > 0 gate, the
                hit flag and a sum over S), through n * L * S x 64 B of intermediate records
  B  fused    : a memset of the n * L counts + one rc_soft_shadow_visibility_device
  C  hard     : (S = 1 only) one rc_shadow_visibility_device into n * L bytes, the call whose record on 2048 x 2048 rays is
                profiles/shadow_visibility.json; compared per item

Timing mode (default): all sides run in this one process on one stream.  The outputs are compared first (zero differing counts); then
`--warmup` unrecorded rounds, then `--reps` recorded rounds with the sides alternating, each timed with two device events around its
whole sequence.  Reported per side: median, min, max and the 10th / 90th percentile (ms).  Writes `--out`.

Counter mode (`--counters`): only launches -- the hard call once (a driver launch without sink atomics), then per S the fused call twice
-- for a counter pass of its own (rocprofv3 --pmc TCC_ATOMIC_sum TCP_TCC_ATOMIC_WITHOUT_RET_REQ_sum -d DIR -- python tools/probes/soft_shadow_probe.py --counters
--plan DIR/plan.json), no tracing next to it.  The plan lists the driver launches in order with the number of visible samples of each, i.e.
the atomics the sink must have issued.  `--merge-counters DIR` (no GPU) then reads the pass's csv and the plan and adds "sink_atomics" to
`--out`; `--table` (no GPU) rewrites the table between the soft_shadows markers of docs/EXPERIMENTS.md from `--out`.

Usage: python tools/probes/soft_shadow_probe.py [--out profiles/soft_shadows.json] [--reps 30] [--warmup 5]"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

BIAS = 1e-3
SEED = 0x50F7
SAMPLES = (1, 4, 16)
BEGIN, END = "<!-- soft_shadows:begin (tools/probes/soft_shadow_probe.py --table) -->", "<!-- soft_shadows:end -->"


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
        rays = rc.scenes.c3_primary_rays(cfg, 1024, 1024)
        self.n = n = len(rays)
        self.s = s = torch.cuda.Stream()
        self.d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).cuda()
        self.d_hits = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        c, e = cfg["lattice_centre"], (np.array((8, 8, 4)) - 1) * 1.5
        self.lights = np.array([cfg["light"], c + (-e[0], 0.6 * e[1], -e[2] - 6.0), c + (0.0, -1.5 * e[1], -e[2]), c + (0.1 * e[0], 2.5 * e[1], 0.2 * e[2])], np.float32)
        self.radii = np.ones(len(self.lights), np.float32)
        self.L = len(self.lights)
        self.d_lights, self.d_radii = torch.from_numpy(self.lights).cuda(), torch.from_numpy(self.radii).cuda()
        self.counts = torch.zeros(n * self.L, dtype=torch.int32, device="cuda")
        self.visible = torch.zeros(n * self.L, dtype=torch.uint8, device="cuda")
        for buf in (self.d_rays, self.d_hits, self.d_lights, self.d_radii, self.counts, self.visible):
            buf.record_stream(s)
        torch.cuda.synchronize()
        t.trace_device(self.d_rays.data_ptr(), self.d_hits.data_ptr(), n, stream=s.cuda_stream)
        s.synchronize()
        self.lit = self.d_hits.view(torch.int32).view(n, 8)[:, 0] != 0

    def fused(self, S):
        with self.torch.cuda.stream(self.s):
            self.counts.zero_()
        self.t.soft_shadow_visibility_device(self.d_rays.data_ptr(), self.d_hits.data_ptr(), self.n, self.d_lights.data_ptr(), self.d_radii.data_ptr(), self.L, S,
                                             self.counts.data_ptr(), seed=SEED, bias=BIAS, stream=self.s.cuda_stream)

    def hard(self):
        self.t.shadow_visibility_device(self.d_rays.data_ptr(), self.d_hits.data_ptr(), self.n, self.d_lights.data_ptr(), self.L, self.visible.data_ptr(),
                                        bias=BIAS, stream=self.s.cuda_stream)


def timed(fn, s, torch):
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record(s)
    fn()
    ev[1].record(s)
    s.synchronize()
    return ev[0].elapsed_time(ev[1])


def case(u, S, warmup, reps):
    torch, t, n, L, s = u.torch, u.t, u.n, u.L, u.s
    total = n * L * S
    shadow_rays = torch.zeros(total * 32, dtype=torch.uint8, device="cuda")
    shadow_hits = torch.zeros(total * 32, dtype=torch.uint8, device="cuda")
    composed_counts = torch.zeros(n * L, dtype=torch.int32, device="cuda")
    for buf in (shadow_rays, shadow_hits, composed_counts):
        buf.record_stream(s)
    torch.cuda.synchronize()
    lit = u.lit

    def composed():
        t.soft_shadow_rays_device(u.d_rays.data_ptr(), u.d_hits.data_ptr(), n, u.d_lights.data_ptr(), u.d_radii.data_ptr(), L, S, shadow_rays.data_ptr(),
                                  seed=SEED, bias=BIAS, stream=s.cuda_stream)
        t.trace_device(shadow_rays.data_ptr(), shadow_hits.data_ptr(), total, mode="any", stream=s.cuda_stream)
        with torch.cuda.stream(s):
            tmax = shadow_rays.view(torch.float32).view(n, L, S, 8)[..., 7]
            blocked = shadow_hits.view(torch.int32).view(n, L, S, 8)[..., 0]
            seen = (tmax > 0) & (blocked == 0) & lit[:, None, None]
            torch.sum(seen, dim=2, dtype=torch.int32, out=composed_counts.view(n, L))

    composed()
    u.fused(S)
    s.synchronize()
    t.wait_for_gpu()
    differing = int((composed_counts != u.counts).sum().item())
    assert differing == 0, f"S = {S}: {differing} of {n * L} counts differ between the fused and the composed path"
    visible_samples = int(u.counts.to(torch.int64).sum().item())
    res = {"samples": S, "lights": L, "items": total, "primary_hits": int(lit.sum().item()), "visible_samples": visible_samples, "differing_counts": 0}
    if S == 1:
        u.hard()
        s.synchronize()
        assert int((u.visible.to(torch.int32) != u.counts).sum().item()) == 0, "S = 1 differs from rc_shadow_visibility_device"
    a_ms, b_ms, c_ms = [], [], []
    for it in range(warmup + reps):
        a, b = timed(composed, s, torch), timed(lambda: u.fused(S), s, torch)
        c = timed(u.hard, s, torch) if S == 1 else None
        if it >= warmup:
            a_ms.append(a)
            b_ms.append(b)
            if c is not None:
                c_ms.append(c)
    a, b = summary(a_ms), summary(b_ms)
    res.update({"a_composed_ms": a, "b_fused_ms": b, "b_over_a": round(b["median"] / a["median"], 4),
                "a_spread": round((a["p90"] - a["p10"]) / a["median"], 4), "b_spread": round((b["p90"] - b["p10"]) / b["median"], 4),
                "b_items_per_ns": round(total / (b["median"] * 1e6), 3), "a_launches": "2 + the reduction's", "b_launches": "1 + a memset",
                "a_intermediate_bytes": total * 64, "b_output_bytes": n * L * 4})
    if c_ms:
        c = summary(c_ms)
        res.update({"c_hard_ms": c, "b_over_c": round(b["median"] / c["median"], 4), "c_items_per_ns": round(total / (c["median"] * 1e6), 3)})
        try:  # the parent commit's record of the hard call: 2048 x 2048 rays, L = 4 -- compared per item
            rec = json.load(open(os.path.join(ROOT, "profiles", "shadow_visibility.json")))
            old = [k for k in rec["cases"] if k["lights"] == L][0]
            res["recorded_hard"] = {"file": "profiles/shadow_visibility.json", "items": old["items"], "median_ms": old["b_fused_ms"]["median"],
                                    "items_per_ns": round(old["items"] / (old["b_fused_ms"]["median"] * 1e6), 3)}
        except (OSError, KeyError, IndexError, ValueError):
            pass
    del shadow_rays, shadow_hits
    return res


def run_timing(args):
    u = Setup()
    res = {"device": u.torch.cuda.get_device_name(0), "scene": "C3 (256 fan spheres, 1 048 576 triangles)", "rays": u.n, "bias": BIAS, "seed": SEED,
           "lights": u.lights.tolist(), "radii": u.radii.tolist(), "reps": args.reps, "warmup": args.warmup, "cases": []}
    for S in SAMPLES:
        res["cases"].append(case(u, S, args.warmup, args.reps))
        print(json.dumps(res["cases"][-1]), flush=True)
    u.t.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


def run_counters(args):
    u = Setup()
    plan = []
    u.hard()
    u.s.synchronize()
    plan.append({"call": "rc_shadow_visibility_device", "samples": 1, "items": u.n * u.L, "sink_atomics_expected": 0})
    for S in SAMPLES:
        for _ in range(2):
            u.fused(S)
            u.s.synchronize()
            plan.append({"call": "rc_soft_shadow_visibility_device", "samples": S, "items": u.n * u.L * S,
                         "sink_atomics_expected": int(u.counts.to(u.torch.int64).sum().item())})
    u.t.wait_for_gpu()
    u.t.free()
    with open(args.plan, "w") as f:
        json.dump(plan, f, indent=1)
    print(json.dumps(plan), flush=True)


def merge_counters(args):
    plan = json.load(open(os.path.join(args.merge_counters, "plan.json")))
    rows = []
    for path in glob.glob(os.path.join(args.merge_counters, "**", "*counter_collection.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    per = {}
    for r in rows:
        if "k_driver" not in r["Kernel_Name"]:
            continue
        per.setdefault(int(r["Dispatch_Id"]), {"kernel": r["Kernel_Name"]})[r["Counter_Name"]] = float(r["Counter_Value"])
    launches = [per[k] for k in sorted(per)]
    assert len(launches) == len(plan), f"{len(launches)} driver dispatches in the counter pass, {len(plan)} planned"
    out = []
    for p, c in zip(plan, launches):
        assert ("SoftShadowJob" in c["kernel"]) == (p["call"] == "rc_soft_shadow_visibility_device"), (p, c)
        out.append(dict(p, **{k: v for k, v in c.items() if k != "kernel"}))
    res = json.load(open(args.out))
    res["sink_atomics"] = {"command": "rocprofv3 --pmc TCC_ATOMIC_sum TCP_TCC_ATOMIC_WITHOUT_RET_REQ_sum -- python tools/probes/soft_shadow_probe.py --counters "
                                      "(a pass of its own, no tracing; every driver launch of the process in order)", "launches": out}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


def table(res):
    ms = lambda d: f"{d['median']:.3f} ms (min {d['min']:.3f}, p10–p90 {d['p10']:.3f}–{d['p90']:.3f})"  # noqa: E731
    lines = ["| S | items | visible samples | A composed | B fused | B / A | verdict |", "|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        slower = c["b_over_a"] > 1.0
        verdict = "**fused is SLOWER than the composed path**" if slower else "fused faster"
        if abs(c["b_over_a"] - 1.0) <= c["a_spread"]:
            verdict = "no difference shown (inside the composed side's own p10–p90 spread)"
        lines.append(f"| {c['samples']} | {c['items']:,} | {c['visible_samples']:,} | {ms(c['a_composed_ms'])}, {c['a_intermediate_bytes'] / 2 ** 20:,.0f} MiB of intermediates | "
                     f"{ms(c['b_fused_ms'])}, {c['b_items_per_ns']:.2f} items/ns | {c['b_over_a']:.2f} | {verdict} |")
    first = res["cases"][0]
    if "c_hard_ms" in first:
        line = (f"S = 1 against `rc_shadow_visibility_device` in the same process: hard {ms(first['c_hard_ms'])}, {first['c_items_per_ns']:.2f} items/ns; "
                f"soft / hard = {first['b_over_c']:.2f} (the soft side includes its memset).")
        if "recorded_hard" in first:
            r = first["recorded_hard"]
            line += f"  The parent's record (`{r['file']}`, {r['items']:,} items, {r['median_ms']:.3f} ms): {r['items_per_ns']:.2f} items/ns."
        lines += ["", line]
    if "sink_atomics" in res:
        lines += ["", "Counter pass of its own (" + res["sink_atomics"]["command"].split(" (")[0] + "), per driver launch in order:", "",
                  "| call | S | items | sink adds expected (= visible samples) | TCC_ATOMIC_sum | TCP_TCC_ATOMIC_WITHOUT_RET_REQ_sum |", "|---|---|---|---|---|---|"]
        for p in res["sink_atomics"]["launches"]:
            lines.append(f"| `{p['call']}` | {p['samples']} | {p['items']:,} | {p['sink_atomics_expected']:,} | {p.get('TCC_ATOMIC_sum', float('nan')):,.0f} | "
                         f"{p.get('TCP_TCC_ATOMIC_WITHOUT_RET_REQ_sum', float('nan')):,.0f} |")
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
    ap.add_argument("--out", default=os.path.join("profiles", "soft_shadows.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--counters", action="store_true")
    ap.add_argument("--plan", default="plan.json")
    ap.add_argument("--merge-counters", default=None, metavar="DIR")
    ap.add_argument("--table", action="store_true")
    args = ap.parse_args()
    if args.table:
        return write_table(args)
    if args.merge_counters:
        return merge_counters(args)
    if args.counters:
        return run_counters(args)
    assert args.reps >= 20, "at least 20 repetitions per side"
    run_timing(args)


if __name__ == "__main__":
    main()
