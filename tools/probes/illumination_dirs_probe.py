"""Illumination over many directions (rc_get_illumination_dirs_device): ONE call for D directions against the loop of D
rc_get_illumination_device calls it replaces, on C5 (one BLAS of 50 028 triangles, identity) and full-size C3 (256 fan spheres,
1 048 576 triangles), D = 46 seeded directions on the upper hemisphere (a day's sun course or a sky dome's sectors,
docs/src/viewfactors_content.md:84-92 of the reference), grid 256 and 1000.

  A  loop  : D x rc_get_illumination_device, each into its own row of a D x N f32 matrix -- per direction a host-side grid layout, a
             memset of the private histogram copies, a persistent launch with its own tail, a fold (the parent commit's path)
  B  dirs  : one rc_get_illumination_dirs_device into a D x N u32 matrix, with option "illum_scratch_bytes" set so that a launch takes
             G = 1, 2, 4, 8 and D directions: ceil(D / G) x (memset + grid-layout kernel + persistent launch + fold)

All sides run in this one process on one stream, the scene static, every matrix zeroed on the stream inside the timed window.  The rows
are compared first (B's counts equal A's, all below 2^24); then `--warmup` unrecorded rounds, then `--reps` recorded rounds with the
sides alternating, each timed with two device events around its whole sequence.  Reported per side: median, min, max and the 10th / 90th
percentile (ms).  Writes `--out`; `--table` (no GPU) rewrites the table between the illumination_dirs markers of docs/EXPERIMENTS.md
from `--out`.

Usage: python tools/probes/illumination_dirs_probe.py [--out profiles/illumination_dirs.json] [--reps 20] [--warmup 5]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N_DIRS = 46
SEED = 0x1D125
GRIDS = (256, 1000)
GROUPS = (1, 2, 4, 8, N_DIRS)
BEGIN, END = "<!-- illumination_dirs:begin (tools/probes/illumination_dirs_probe.py --table) -->", "<!-- illumination_dirs:end -->"


def summary(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 4), "min": round(float(xs.min()), 4), "max": round(float(xs.max()), 4),
            "p10": round(float(np.percentile(xs, 10)), 4), "p90": round(float(np.percentile(xs, 90)), 4)}


def directions():
    """46 seeded directions on the upper hemisphere, at least 8 degrees above the horizon (rays travel DOWN from the sky: z < 0)."""
    g = np.random.Generator(np.random.Philox(key=SEED))
    z = g.uniform(np.sin(np.radians(8.0)), 1.0, N_DIRS)
    phi = g.uniform(0.0, 2.0 * np.pi, N_DIRS)
    r = np.sqrt(1.0 - z * z)
    return np.ascontiguousarray(np.stack([r * np.cos(phi), r * np.sin(phi), -z], axis=1), dtype=np.float32)


def timed(fn, s, torch):
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record(s)
    fn()
    ev[1].record(s)
    s.synchronize()
    return ev[0].elapsed_time(ev[1])


def workload(rc, torch, name, cfg, warmup, reps):
    from raycore_jl_amd._capi import check, lib, ptr
    t = rc.TLAS(0)
    for verts, meta in cfg["blas"]:
        t.add_geometry(verts, meta)
    for b, xf, ids in cfg["instances"]:
        t.push_instances(b, xf, ids)
    t.sync()
    n = t.n_primitives()
    per_dir = 16 * 8 * ((n + 7) // 8) * 4  # bytes of one direction's private histogram copies
    dirs = directions()
    s = torch.cuda.Stream()
    d_dirs = torch.from_numpy(dirs).cuda()
    loop_counts = torch.zeros(N_DIRS * n, dtype=torch.float32, device="cuda")
    dirs_counts = torch.zeros(N_DIRS * n, dtype=torch.int32, device="cuda")
    for buf in (d_dirs, loop_counts, dirs_counts):
        buf.record_stream(s)
    torch.cuda.synchronize()
    default_cap = t.get_option("illum_scratch_bytes")
    cases = []
    for grid in GRIDS:
        cells = grid * grid

        def loop():
            with torch.cuda.stream(s):
                loop_counts.zero_()
            for d in range(N_DIRS):
                check(lib().rc_get_illumination_device(t._h, dirs[d].ctypes.data_as(C.c_void_p), grid, 0, cells, ptr(loop_counts.data_ptr() + 4 * d * n),
                                                       ptr(s.cuda_stream)))

        def fused():
            with torch.cuda.stream(s):
                dirs_counts.zero_()
            t.illumination_dirs_device(d_dirs.data_ptr(), N_DIRS, grid, dirs_counts.data_ptr(), n, stream=s.cuda_stream)

        loop()
        s.synchronize()
        want = loop_counts.cpu().numpy().copy()
        assert want.max() < (1 << 24)
        for G in GROUPS:
            t.set_option("illum_scratch_bytes", G * per_dir)
            fused()
            s.synchronize()
            t.wait_for_gpu()
            got = dirs_counts.cpu().numpy().view(np.uint32)
            assert np.array_equal(got.astype(np.float32), want), f"{name} grid {grid} G {G}: the rows differ from the one-direction loop's"
        sides = {"loop": loop}
        for G in GROUPS:
            sides[f"G{G}"] = (lambda G=G: (t.set_option("illum_scratch_bytes", G * per_dir), fused()))
        ms = {k: [] for k in sides}
        for it in range(warmup + reps):
            for k, fn in sides.items():  # the sides alternate within a round
                x = timed(fn, s, torch)
                if it >= warmup:
                    ms[k].append(x)
        a = summary(ms["loop"])
        res = {"workload": name, "n_prims": n, "n_instances": t.n_instances(), "grid": grid, "dirs": N_DIRS, "rays": N_DIRS * cells, "hits": int(want.sum()),
               "per_dir_scratch_bytes": per_dir, "a_loop_ms": a, "a_spread": round((a["p90"] - a["p10"]) / a["median"], 4), "b_dirs_ms": {}}
        for G in GROUPS:
            b = summary(ms[f"G{G}"])
            res["b_dirs_ms"][str(G)] = dict(b, launches=-(-N_DIRS // G), scratch_bytes=G * per_dir, over_loop=round(b["median"] / a["median"], 4),
                                            spread=round((b["p90"] - b["p10"]) / b["median"], 4))
        cases.append(res)
        print(json.dumps(res), flush=True)
    t.set_option("illum_scratch_bytes", default_cap)
    t.free()
    return cases, default_cap


def run_timing(args):
    import torch

    import raycore_jl_amd as rc
    assert rc.device_count() > 0, "no GPU visible: nothing is measured on a CPU"
    res = {"device": torch.cuda.get_device_name(0), "dirs": N_DIRS, "seed": SEED, "directions": directions().tolist(), "reps": args.reps, "warmup": args.warmup,
           "cases": []}
    for name, cfg in (("C5", rc.scenes.config_c5()), ("C3", rc.scenes.config_c3())):
        cases, cap = workload(rc, torch, name, cfg, args.warmup, args.reps)
        res["cases"] += cases
        res["default_scratch_bytes"] = cap
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


def table(res):
    ms = lambda d: f"{d['median']:.3f} ms (p10–p90 {d['p10']:.3f}–{d['p90']:.3f})"  # noqa: E731
    groups = [str(g) for g in GROUPS]
    lines = ["| workload | grid | rays | A loop of 46 calls | " + " | ".join(f"B, G = {g}" for g in groups) + " | best B / A |", "|---|---|---|---|" + "---|" * (len(groups) + 1)]
    for c in res["cases"]:
        b = c["b_dirs_ms"]
        best = min(groups, key=lambda g: b[g]["median"])
        cells = [f"{b[g]['median']:.3f} ms ({b[g]['over_loop']:.2f}; {b[g]['scratch_bytes'] / 2 ** 20:,.1f} MiB)" for g in groups]
        ratio = b[best]["over_loop"]
        verdict = f"{ratio:.2f} at G = {best}"
        if abs(ratio - 1.0) <= c["a_spread"]:
            verdict += " (inside the loop's own p10–p90 spread: no difference shown)"
        elif ratio > 1.0:
            verdict += " (**the new call is SLOWER than the loop**)"
        lines.append(f"| {c['workload']} ({c['n_prims']:,} primitives, {c['n_instances']} instances) | {c['grid']} | {c['rays']:,} | {ms(c['a_loop_ms'])} | " + " | ".join(cells) + f" | {verdict} |")
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
    ap.add_argument("--out", default=os.path.join("profiles", "illumination_dirs.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--table", action="store_true")
    args = ap.parse_args()
    if args.table:
        return write_table(args)
    assert args.reps >= 20, "at least 20 repetitions per side"
    run_timing(args)


if __name__ == "__main__":
    main()
