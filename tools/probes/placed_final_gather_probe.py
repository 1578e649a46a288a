"""Placed final gather (rc_placed_final_gather_device): the fused placed launch against its composed path and against the metadata gather,
on full-size C3 (256 fan spheres, 1 048 576 placed primitives).  The frame is final_gather_probe.py's: 1 Mi primary HITS, the first
1 048 576 hit slots of a 2048 x 2048 pinhole view, gathered on the device.  S = 4, 16 and 64 samples per hit, bias 1e-3, max_dist = inf and
a tenth of the scene's diagonal; x_meta = one seeded full-range u32 per primitive, x = its lift to the placed index space
(x[q] = x_meta[metadata(q) - 1]), miss_value = 12345 -- so all three sides must give the same words.

  A  composed : rc_ambient_occlusion_rays_device + ONE rc_trace_closest_device over the n * S rays + rc_placed_hit_indices_device on the
                sample hits + a torch gather on the device (the t_max > 0 gate, q -> x, the miss value, a sum over S in int64 and the
                open count), through n * S x 68 B of intermediate records
  B  placed   : a memset of the n sums and the n open counts + one rc_placed_final_gather_device with x
  C  metadata : the same memsets + one rc_final_gather_device with x_meta on the same frame: the kernel this one was derived from, as the
                yardstick (two dependent loads per hit where B makes one; the same atomics)

All sides run in this one process on one stream.  The outputs are compared first (zero differing sums and open counts, B against A and
B against C); then `--warmup` unrecorded rounds, then `--reps` recorded rounds, each side timed with two device events around its whole
sequence.  The order rotates -- A B C, then A C B -- because the side behind A starts on caches that A's records have swept and the
side behind its sibling on warm ones: B and C take each place half the time, and the two places are also reported apart.  Reported per
side: median, min, max and the 10th / 90th percentile (ms); B / C with C's own p10-p90 spread beside it, over all rounds and per place.
`--table` (no GPU) rewrites the tables between the placed_final_gather markers of docs/EXPERIMENTS.md.

Usage: python tools/probes/placed_final_gather_probe.py [--out profiles/placed_final_gather.json] [--reps 40] [--warmup 5]"""
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
INVALID = 0xFFFFFFFF
BEGIN, END = "<!-- placed_final_gather:begin (tools/probes/placed_final_gather_probe.py --table) -->", "<!-- placed_final_gather:end -->"


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
        self.n_prims = t.n_primitives()
        base = t.placed_primitive_bases().astype(np.int64)
        self.P, self.n_inst = int(base[-1]), len(base) - 1
        x_meta = np.random.default_rng(7).integers(0, 1 << 32, self.n_prims, dtype=np.uint32)
        # the lift: placed primitive q = base[i] + l is flat primitive prims_offset(i) + l
        static = t.adapt()
        offs = static.blas_descriptors["primitives_offset"].astype(np.int64)[static.instances["blas_index"].astype(np.int64) - 1]
        inst = np.repeat(np.arange(self.n_inst), np.diff(base))
        flat = offs[inst] + (np.arange(self.P) - base[inst])
        meta = static.all_blas_prims["meta"].astype(np.int64)[flat]
        assert meta.min() >= 1 and meta.max() <= self.n_prims, "the lift needs metadata in 1..N"
        x = x_meta[meta - 1]
        self.d_x = torch.from_numpy(x.view(np.int32).copy()).cuda()
        self.d_x_meta = torch.from_numpy(x_meta.view(np.int32).copy()).cuda()
        self.x64 = torch.from_numpy(x.astype(np.int64)).cuda()  # the composed side's lookup table, widened once
        self.sums = torch.zeros(n, dtype=torch.int64, device="cuda")
        self.open = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.meta_sums = torch.zeros(n, dtype=torch.int64, device="cuda")
        self.meta_open = torch.zeros(n, dtype=torch.int32, device="cuda")
        del all_rays, all_hits
        for buf in (self.d_rays, self.d_hits, self.d_x, self.d_x_meta, self.x64, self.sums, self.open, self.meta_sums, self.meta_open):
            buf.record_stream(s)
        torch.cuda.synchronize()

    def placed(self, S, dist):
        with self.torch.cuda.stream(self.s):
            self.sums.zero_()
            self.open.zero_()
        self.t.placed_final_gather_device(self.d_rays.data_ptr(), self.d_hits.data_ptr(), self.n, S, self.d_x.data_ptr(), self.sums.data_ptr(),
                                          self.open.data_ptr(), miss_value=MISS, max_dist=dist, seed=SEED, bias=BIAS, stream=self.s.cuda_stream)

    def metadata(self, S, dist):
        with self.torch.cuda.stream(self.s):
            self.meta_sums.zero_()
            self.meta_open.zero_()
        self.t.final_gather_device(self.d_rays.data_ptr(), self.d_hits.data_ptr(), self.n, S, self.d_x_meta.data_ptr(), self.meta_sums.data_ptr(),
                                   self.meta_open.data_ptr(), miss_value=MISS, max_dist=dist, seed=SEED, bias=BIAS, stream=self.s.cuda_stream)


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
    g_q = torch.zeros(total, dtype=torch.int32, device="cuda")
    composed_sums = torch.zeros(n, dtype=torch.int64, device="cuda")
    composed_open = torch.zeros(n, dtype=torch.int32, device="cuda")
    lit = u.d_hits.view(torch.int32).view(n, 8)[:, 0] != 0
    for buf in (g_rays, g_hits, g_q, composed_sums, composed_open):
        buf.record_stream(s)
    torch.cuda.synchronize()

    def composed():
        t.ambient_occlusion_rays_device(u.d_rays.data_ptr(), u.d_hits.data_ptr(), n, S, g_rays.data_ptr(), max_dist=dist, seed=SEED, bias=BIAS,
                                        stream=s.cuda_stream)
        t.trace_device(g_rays.data_ptr(), g_hits.data_ptr(), total, mode="closest", stream=s.cuda_stream)
        t.placed_hit_indices_device(g_hits.data_ptr(), total, g_q.data_ptr(), stream=s.cuda_stream)
        with torch.cuda.stream(s):
            tmax = g_rays.view(torch.float32).view(n, S, 8)[..., 7]
            q = g_q.view(n, S)
            live = (tmax > 0) & lit[:, None]
            struck = live & (q != -1)  # (RC_INVALID_ID read as int32)
            escaped = live & (q == -1)
            index = torch.where(struck, q, 0).to(torch.int64) & INVALID  # (the u32 value; 0 where there is no hit: masked below)
            value = torch.where(struck, u.x64[index], 0) + escaped.to(torch.int64) * MISS
            torch.sum(value, dim=1, out=composed_sums)
            torch.sum(escaped, dim=1, dtype=torch.int32, out=composed_open)

    composed()
    u.placed(S, dist)
    u.metadata(S, dist)
    s.synchronize()
    t.wait_for_gpu()

    def differing():
        return {"b_vs_a_sums": int((composed_sums != u.sums).sum().item()), "b_vs_a_open": int((composed_open != u.open).sum().item()),
                "b_vs_c_sums": int((u.meta_sums != u.sums).sum().item()), "b_vs_c_open": int((u.meta_open != u.open).sum().item())}

    d = differing()
    assert not any(d.values()), f"S = {S}, max_dist = {dist}: of {n} slots these differ between the sides: {d}"
    open_samples = int(u.open.to(torch.int64).sum().item())
    res = {"samples": S, "max_dist": "inf" if np.isinf(dist) else round(float(dist), 4), "items": total, "hits": n, "open_samples": open_samples,
           "open_fraction": round(open_samples / total, 4), "differing": d}
    # The order rotates: A B C in even rounds, A C B in odd ones.  Whatever runs behind A starts on caches that A's n * S x 68 B of records
    # and the reduction's temporaries have swept, whatever runs behind its sibling finds the frame and the scene warm: each of B and C
    # takes each place half the time, and the two places are also kept apart ("behind_a", "behind_sibling").
    ms = {"a": [], "b": [], "c": []}
    placed_ms = {("b", "a"): [], ("b", "c"): [], ("c", "a"): [], ("c", "b"): []}
    sides = {"a": composed, "b": lambda: u.placed(S, dist), "c": lambda: u.metadata(S, dist)}
    for it in range(warmup + reps):
        order = ("a", "b", "c") if it % 2 == 0 else ("a", "c", "b")
        for pos, k in enumerate(order):
            v = timed(sides[k], s, torch)
            if it >= warmup:
                ms[k].append(v)
                if pos:
                    placed_ms[k, order[pos - 1]].append(v)
    s.synchronize()
    t.wait_for_gpu()
    assert not any(differing().values())
    a, b, c = summary(ms["a"]), summary(ms["b"]), summary(ms["c"])
    behind_a = {"b_placed_ms": summary(placed_ms["b", "a"]), "c_metadata_ms": summary(placed_ms["c", "a"])}
    behind_sibling = {"b_placed_ms": summary(placed_ms["b", "c"]), "c_metadata_ms": summary(placed_ms["c", "b"])}
    for d in (behind_a, behind_sibling):
        d["b_over_c"] = round(d["b_placed_ms"]["median"] / d["c_metadata_ms"]["median"], 4)
        d["c_spread"] = round((d["c_metadata_ms"]["p90"] - d["c_metadata_ms"]["p10"]) / d["c_metadata_ms"]["median"], 4)
    res.update({"behind_a": behind_a, "behind_sibling": behind_sibling, "x_bytes": {"b_placed": u.P * 4, "c_metadata": u.n_prims * 4}})
    res.update({"a_composed_ms": a, "b_placed_ms": b, "c_metadata_ms": c, "b_over_c": round(b["median"] / c["median"], 4),
                "b_over_a": round(b["median"] / a["median"], 4), "c_spread": round((c["p90"] - c["p10"]) / c["median"], 4),
                "b_spread": round((b["p90"] - b["p10"]) / b["median"], 4), "a_spread": round((a["p90"] - a["p10"]) / a["median"], 4),
                "b_items_per_ns": round(total / (b["median"] * 1e6), 3), "c_items_per_ns": round(total / (c["median"] * 1e6), 3),
                "a_items_per_ns": round(total / (a["median"] * 1e6), 3), "a_intermediate_bytes": total * 68, "b_output_bytes": n * 12})
    del g_rays, g_hits, g_q
    return res


def run_timing(args):
    u = Setup()
    res = {"device": u.torch.cuda.get_device_name(0), "scene": "C3 (256 fan spheres, 1 048 576 placed primitives)", "primary_rays": u.primary_rays,
           "primary_hits": u.primary_hits, "hits_used": u.n, "placed_primitives": u.P, "primitives": u.n_prims, "instances": u.n_inst,
           "scene_diagonal": round(u.diagonal, 4), "bias": BIAS, "seed": SEED, "miss_value": MISS, "reps": args.reps, "warmup": args.warmup, "cases": []}
    for S in args.samples or SAMPLES:
        for dist in (float("inf"), u.diagonal / 10.0):
            res["cases"].append(case(u, S, dist, args.warmup, args.reps))
            print(json.dumps(res["cases"][-1]), flush=True)
    u.t.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


def table(res):
    ms = lambda d: f"{d['median']:.3f} ms (min {d['min']:.3f}, p10–p90 {d['p10']:.3f}–{d['p90']:.3f})"  # noqa: E731
    lines = ["| S | max_dist | items | open samples | A composed | B placed | C metadata gather | B / C | C's p10–p90 spread | verdict B against C | B / A |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]

    def verdict(ratio, spread):
        if abs(ratio - 1.0) <= spread:
            return "inside C's own spread"
        return "**placed is SLOWER than the metadata gather by more than its spread**" if ratio > 1.0 else "placed faster by more than the spread"

    for c in res["cases"]:
        lines.append(f"| {c['samples']} | {c['max_dist']} | {c['items']:,} | {c['open_samples']:,} ({100 * c['open_fraction']:.1f} %) | "
                     f"{ms(c['a_composed_ms'])} | {ms(c['b_placed_ms'])}, {c['b_items_per_ns']:.2f} items/ns | "
                     f"{ms(c['c_metadata_ms'])}, {c['c_items_per_ns']:.2f} items/ns | {c['b_over_c']:.3f} | {100 * c['c_spread']:.1f} % | "
                     f"{verdict(c['b_over_c'], c['c_spread'])} | {c['b_over_a']:.3f} |")
    lines += ["", "The two places of a round apart (medians; behind A the caches have been swept by A's records, behind the sibling they are warm):", "",
              "| S | max_dist | behind A: B placed | behind A: C metadata | B / C (C's spread) | behind the sibling: B placed | behind the sibling: C metadata | B / C (C's spread) |",
              "|---|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        pa, ps = c["behind_a"], c["behind_sibling"]
        lines.append(f"| {c['samples']} | {c['max_dist']} | {pa['b_placed_ms']['median']:.3f} ms | {pa['c_metadata_ms']['median']:.3f} ms | "
                     f"{pa['b_over_c']:.3f} ({100 * pa['c_spread']:.1f} %) | {ps['b_placed_ms']['median']:.3f} ms | {ps['c_metadata_ms']['median']:.3f} ms | "
                     f"{ps['b_over_c']:.3f} ({100 * ps['c_spread']:.1f} %) |")
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
    ap.add_argument("--out", default=os.path.join("profiles", "placed_final_gather.json"))
    ap.add_argument("--reps", type=int, default=40, help="recorded rounds (even: each order as often as the other)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--samples", type=int, nargs="*", default=None, help="only these S")
    ap.add_argument("--table", action="store_true")
    args = ap.parse_args()
    if args.table:
        return write_table(args)
    assert args.reps >= 20, "at least 20 repetitions per side"
    run_timing(args)


if __name__ == "__main__":
    main()
