"""Illumination from point sources (rc_get_illumination_points_device): the fused call against the composed path and against a loop of
one-source calls, on full-size C3 (256 fan spheres, 1 048 576 triangles, 4096 metadata values).  S = 1, 16 and 64 isotropic sources at
seeded positions inside the lattice and outside every sphere, grid = 256 and 1024 (65 536 and 1 048 576 rays per source), unbounded range.

  A  composed : rc_point_source_rays_device + ONE rc_trace_closest_device over the S * grid^2 rays + a histogram in torch on the device
                (hit -> flat primitive -> metadata -> the 1..N rule -> bincount over source * N + metadata - 1, and the escaped count),
                through S * grid^2 x 64 B of intermediate records
  B  fused    : a memset of the S x N counts and the S escaped words + one rc_get_illumination_points_device
  C  loop     : the same memsets + S one-source calls with first_source = k into the rows of the same matrix
  D  counts   : B with d_escaped = NULL (the kernel without the escape counters)

All sides run in this one process on one stream.  The outputs are compared first (zero differing words); then `--warmup` unrecorded
rounds, then `--reps` recorded rounds with the sides alternating, each timed with two device events around its whole sequence.  Reported
per side: median, min, max and the 10th / 90th percentile (ms), and Mrays/s at the median.

`--table` (no GPU) rewrites the table between the point_illumination markers of docs/EXPERIMENTS.md from `--out`.

Usage: python tools/probes/point_illumination_probe.py [--out profiles/point_illumination.json] [--reps 25] [--warmup 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SEED = 0x50C3
SOURCES = (1, 16, 64)
GRIDS = (256, 1024)
BEGIN, END = "<!-- point_illumination:begin (tools/probes/point_illumination_probe.py --table) -->", "<!-- point_illumination:end -->"


def summary(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 4), "min": round(float(xs.min()), 4), "max": round(float(xs.max()), 4),
            "p10": round(float(np.percentile(xs, 10)), 4), "p90": round(float(np.percentile(xs, 90)), 4)}


def lamp_positions(cfg, count):
    """`count` seeded points inside the lattice's box that lie outside every sphere (radius 0.5 x the instance's scale)."""
    g = np.random.default_rng(SEED)
    centres, radii = np.asarray(cfg["centres"], np.float64), 0.5 * np.asarray(cfg["scales"], np.float64)
    lo, hi = centres.min(axis=0), centres.max(axis=0)
    out = []
    while len(out) < count:
        p = g.uniform(lo, hi)
        if (np.linalg.norm(centres - p, axis=1) > radii + 0.05).all():
            out.append(p)
    return np.asarray(out, np.float32)


class Setup:
    def __init__(self):
        import torch

        import raycore_jl_amd as rc
        assert rc.device_count() > 0, "no GPU visible: nothing is measured on a CPU"
        self.torch, self.rc = torch, rc
        cfg = rc.scenes.config_c3()
        self.t = t = rc.TLAS(0)
        for verts, meta in cfg["blas"]:
            t.add_geometry(verts, meta)
        for b, xf, ids in cfg["instances"]:
            t.push_instances(b, xf, ids)
        t.sync()
        self.n_prims = t.n_primitives()
        self.src = rc.point_sources(lamp_positions(cfg, max(SOURCES)))
        self.s = torch.cuda.Stream()
        self.d_src = torch.from_numpy(self.src.view(np.uint8).reshape(-1).copy()).cuda()
        self.prim_meta = torch.from_numpy(t.adapt().all_blas_prims["meta"].astype(np.int64)).cuda()
        for buf in (self.d_src, self.prim_meta):
            buf.record_stream(self.s)
        torch.cuda.synchronize()


def timed(fn, s, torch):
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record(s)
    fn()
    ev[1].record(s)
    s.synchronize()
    return ev[0].elapsed_time(ev[1])


def case(u, S, grid, warmup, reps):
    torch, t, s, N = u.torch, u.t, u.s, u.n_prims
    cells = grid * grid
    total = S * cells
    d_rays = torch.zeros(total * 32, dtype=torch.uint8, device="cuda")
    d_hits = torch.zeros(total * 32, dtype=torch.uint8, device="cuda")
    row_of = torch.arange(S, dtype=torch.int64, device="cuda").repeat_interleave(cells) * N
    outs = {k: (torch.zeros(S * N, dtype=torch.int32, device="cuda"), torch.zeros(S, dtype=torch.int32, device="cuda")) for k in "bcd"}
    composed_out = [None, None]
    for buf in (d_rays, d_hits, row_of, *outs["b"], *outs["c"], *outs["d"]):
        buf.record_stream(s)
    torch.cuda.synchronize()
    st = s.cuda_stream

    def composed():
        t.point_source_rays_device(u.d_src.data_ptr(), S, grid, d_rays.data_ptr(), seed=SEED, stream=st)
        t.trace_device(d_rays.data_ptr(), d_hits.data_ptr(), total, mode="closest", stream=st)
        with torch.cuda.stream(s):
            rec = d_hits.view(torch.int32).view(total, 8)
            struck = rec[:, 0] != 0
            m = u.prim_meta[torch.where(struck, rec[:, 2], 0).to(torch.int64)]
            counted = struck & (m >= 1) & (m <= N)
            composed_out[0] = torch.bincount((row_of + m - 1)[counted], minlength=S * N)
            composed_out[1] = (~struck).view(S, cells).sum(dim=1)

    def fused():
        counts, escaped = outs["b"]
        with torch.cuda.stream(s):
            counts.zero_()
            escaped.zero_()
        t.illumination_points_device(u.d_src.data_ptr(), S, grid, counts.data_ptr(), N, escaped.data_ptr(), seed=SEED, stream=st)

    def loop():
        counts, escaped = outs["c"]
        with torch.cuda.stream(s):
            counts.zero_()
            escaped.zero_()
        for k in range(S):
            t.illumination_points_device(u.d_src.data_ptr() + 32 * k, 1, grid, counts.data_ptr() + 4 * N * k, N, escaped.data_ptr() + 4 * k, seed=SEED,
                                         first_source=k, stream=st)

    def counts_only():
        counts = outs["d"][0]
        with torch.cuda.stream(s):
            counts.zero_()
        t.illumination_points_device(u.d_src.data_ptr(), S, grid, counts.data_ptr(), N, None, seed=SEED, stream=st)

    def differing():
        want, want_escaped = composed_out[0].to(torch.int32), composed_out[1].to(torch.int32)
        return [int((o[0] != want).sum().item()) + int((o[1] != want_escaped).sum().item()) for o in (outs["b"], outs["c"])] + [int((outs["d"][0] != want).sum().item())]

    composed(); fused(); loop(); counts_only()
    s.synchronize()
    t.wait_for_gpu()
    assert differing() == [0, 0, 0], f"S = {S}, grid = {grid}: {differing()} words of the fused call / the loop / the counts-only call differ from the composed path"
    hits = int(outs["b"][0].to(torch.int64).sum().item())
    res = {"sources": S, "grid": grid, "rays": total, "hit_fraction": round(hits / total, 4), "differing_words": 0}
    ms = {"a": [], "b": [], "c": [], "d": []}
    for it in range(warmup + reps):
        for key, fn in (("a", composed), ("b", fused), ("c", loop), ("d", counts_only)):
            x = timed(fn, s, torch)
            if it >= warmup:
                ms[key].append(x)
    s.synchronize()
    t.wait_for_gpu()
    assert differing() == [0, 0, 0]
    a, b, c, d = (summary(ms[k]) for k in "abcd")
    spread = lambda d: round((d["p90"] - d["p10"]) / d["median"], 4)  # noqa: E731
    res.update({"a_composed_ms": a, "b_fused_ms": b, "c_loop_ms": c, "d_counts_only_ms": d, "d_over_a": round(d["median"] / a["median"], 4), "b_over_a": round(b["median"] / a["median"], 4),
                "b_over_c": round(b["median"] / c["median"], 4), "a_spread": spread(a), "b_spread": spread(b), "c_spread": spread(c),
                "a_mrays_per_s": round(total / (a["median"] * 1e3), 1), "b_mrays_per_s": round(total / (b["median"] * 1e3), 1),
                "c_mrays_per_s": round(total / (c["median"] * 1e3), 1), "a_intermediate_bytes": total * 64, "b_output_bytes": S * (N + 1) * 4})
    del d_rays, d_hits, row_of
    composed_out[0] = composed_out[1] = None
    torch.cuda.empty_cache()
    return res


def run_timing(args):
    u = Setup()
    res = {"device": u.torch.cuda.get_device_name(0), "scene": "C3 (256 fan spheres, 1 048 576 triangles)", "n_prims": u.n_prims, "seed": SEED,
           "sources": "isotropic, seeded positions inside the lattice and outside every sphere, unbounded range", "reps": args.reps,
           "warmup": args.warmup, "cases": []}
    for grid in args.grids or GRIDS:
        for S in args.sources or SOURCES:
            res["cases"].append(case(u, S, grid, args.warmup, args.reps))
            print(json.dumps(res["cases"][-1]), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    u.t.free()


def table(res):
    ms = lambda d: f"{d['median']:.3f} ms (min {d['min']:.3f}, p10–p90 {d['p10']:.3f}–{d['p90']:.3f})"  # noqa: E731
    lines = ["| S | grid | rays | hit | A composed | A's intermediates | B fused | C loop of S calls | D counts only | B / A | B / C | D / A | verdict (B against A) |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        verdict = "**fused is SLOWER than the composed path**" if c["b_over_a"] > 1.0 else "fused faster"
        if abs(c["b_over_a"] - 1.0) <= max(c["a_spread"], c["b_spread"]):
            verdict = "no difference shown (inside a side's own p10–p90 spread)"
        lines.append(f"| {c['sources']} | {c['grid']} | {c['rays']:,} | {100 * c['hit_fraction']:.1f} % | {ms(c['a_composed_ms'])}, {c['a_mrays_per_s']:,.0f} Mrays/s | "
                     f"{c['a_intermediate_bytes'] / 2 ** 20:,.0f} MiB | {ms(c['b_fused_ms'])}, {c['b_mrays_per_s']:,.0f} Mrays/s | "
                     f"{ms(c['c_loop_ms'])}, {c['c_mrays_per_s']:,.0f} Mrays/s | {ms(c['d_counts_only_ms'])} | {c['b_over_a']:.3f} | {c['b_over_c']:.3f} | {c['d_over_a']:.3f} | {verdict} |")
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
    ap.add_argument("--out", default=os.path.join("profiles", "point_illumination.json"))
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sources", type=int, nargs="*", default=None, help="only these S")
    ap.add_argument("--grids", type=int, nargs="*", default=None, help="only these grids")
    ap.add_argument("--table", action="store_true")
    args = ap.parse_args()
    if args.table:
        return write_table(args)
    assert args.reps >= 20, "at least 20 repetitions per side"
    run_timing(args)


if __name__ == "__main__":
    main()
