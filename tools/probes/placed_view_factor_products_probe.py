"""Dev (GPU): what the placed products call costs beside its per-triangle sibling, on the instanced workload it exists for, and where the
private copies of its hot vector stop paying.

    python tools/probes/placed_view_factor_products_probe.py --record a|b|c [--out FILE]

One process per record; the records are merged in FILE.  Every timing is taken on one stream with device events around the call (the
zeroing of the copies and the fold inside): 3 warm-up + 9 recorded calls, median / min / max; the sides of a comparison are alternated
A B A B so that drift of the device's clocks lands on both.

  a  the cost of the placed source and sink alone.  The reduced C5 of the other driver probes (5 420 triangles x 1024 rays) as ONE identity
     instance, uniform sampling: rc_placed_view_factor_products_device (x, mx, mtx; no escapes) against rc_view_factor_products_device in
     the same process.  The rays are the same bit for bit (the words are compared through the metadata permutation), so the difference is
     the functor and the sink.  Reported against the sibling's own run-to-run spread (its two medians, its min..max).
  b  C3: 256 instances of one 4096-triangle sphere, 1 048 576 placed primitives, R = 16, cosine: the call with mx only (what a bounce
     needs), with mx and mtx, and with all three outputs; time and Grays/s.
  c  copies against straight adds for mtx, by option "placed_copy_bytes" (default against 0), mtx the only output: on (b)'s scene at
     R = 1, 4, 16, 64 -- the copies cost the same 128 MiB of zeroing and folding whatever R is --, and on (a)'s scene at R = 64 and 1024,
     where a few wall triangles take most hits.  The words of both paths are compared.

Fails without a GPU."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import raycore_jl_amd as rc  # noqa: E402

SEED = 7


def build(cfg):
    t = rc.TLAS(0)
    for verts, meta in cfg["blas"]:
        t.add_geometry(verts, meta)
    for b, xf, ids in cfg["instances"]:
        t.push_instances(b, xf, ids)
    return t.sync()


def timed(torch, call, warmup=3, reps=9):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median": round(float(np.median(ms)), 4), "min": round(float(min(ms)), 4), "max": round(float(max(ms)), 4), "reps": reps}


def u32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()


def words(out):
    return out.cpu().numpy().view(np.uint64)


def full_range(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint32)


def c5_reduced():
    t = build(rc.scenes.config_c5(lon=32, bands=17, wall_k=5))
    assert t.n_primitives() == 5420 and rc.placed_primitive_count(t) == 5420
    return t


def record_a(torch):
    rays = 1024
    t = c5_reduced()
    n = t.n_primitives()
    meta = t.adapt().all_blas_prims["meta"].astype(np.int64)
    x = full_range(n, 1)
    d_x, d_xq = u32(torch, x), u32(torch, x[meta - 1])  # the sibling indexes by metadata - 1, the placed call by placed primitive = flat primitive
    ref = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    out = torch.zeros(2 * n, dtype=torch.int64, device="cuda")

    def sibling():
        t.view_factor_products_device(d_x.data_ptr(), ref.data_ptr(), ref.data_ptr() + 8 * n, rays, SEED)

    def placed():
        t.placed_view_factor_products_device(d_xq.data_ptr(), out.data_ptr(), out.data_ptr() + 8 * n, rays, SEED, "uniform")

    r = {"sibling": timed(torch, sibling), "placed": timed(torch, placed), "sibling_again": timed(torch, sibling), "placed_again": timed(torch, placed)}
    sib = (r["sibling"]["median"], r["sibling_again"]["median"])
    r["placed_over_sibling"] = round(min(r["placed"]["median"], r["placed_again"]["median"]) / min(sib), 4)
    r["sibling_median_spread"] = round(abs(sib[0] - sib[1]) / min(sib), 4)
    r["sibling_min_max_spread"] = round((max(r["sibling"]["max"], r["sibling_again"]["max"]) - min(r["sibling"]["min"], r["sibling_again"]["min"])) / min(sib), 4)
    ref.zero_(); out.zero_()
    sibling(); placed()
    torch.cuda.synchronize()
    t.wait_for_gpu()
    w_ref, w_out = words(ref), words(out)
    assert np.array_equal(w_out[:n], w_ref[:n][meta - 1]) and np.array_equal(w_out[n:], w_ref[n:][meta - 1]) and w_out.any(), "the placed words differ from the sibling's"
    r["checksum"] = int(w_out.sum(dtype=np.uint64))
    row = {"triangles": n, "rays_per_triangle": rays, "rays": n * rays, "sampling": "uniform", **r}
    print(json.dumps({"a": row}), flush=True)
    t.free()
    return row


def c3():
    t = build(rc.scenes.config_c3())
    assert rc.placed_primitive_count(t) == 1 << 20 and t.n_instances() == 256
    return t


def record_b(torch):
    rays = 16
    t = c3()
    P = 1 << 20
    d_x = u32(torch, full_range(P, 2))
    out = torch.zeros(3 * P, dtype=torch.int64, device="cuda")
    mx, mtx, esc = out.data_ptr(), out.data_ptr() + 8 * P, out.data_ptr() + 16 * P

    def call(m, mt, e):
        return lambda: t.placed_view_factor_products_device(d_x.data_ptr(), m, mt, rays, SEED, "cosine", e)

    sides = {"mx_only": call(mx, None, None), "mx_and_mtx": call(mx, mtx, None), "mx_mtx_escaped": call(mx, mtx, esc)}
    row = {"instances": 256, "placed_primitives": P, "rays_per_triangle": rays, "rays": P * rays, "sampling": "cosine"}
    for name in list(sides) + [k + "_again" for k in sides]:
        row[name] = timed(torch, sides[name.replace("_again", "")])
    for name in sides:
        row[name + "_grays_per_s"] = round(P * rays / min(row[name]["median"], row[name + "_again"]["median"]) / 1e6, 3)
    out.zero_()
    sides["mx_mtx_escaped"]()
    torch.cuda.synchronize()
    t.wait_for_gpu()
    w = words(out)
    row["counted"], row["escaped"] = int(w[:P].astype(bool).sum()), int(w[2 * P:].sum(dtype=np.uint64))
    row["checksum"] = int(w.sum(dtype=np.uint64))
    print(json.dumps({"b": row}), flush=True)
    t.free()
    return row


def copies_against_straight(torch, t, P, rays, sampling):
    d_x = u32(torch, full_range(P, 3))
    out = torch.zeros(P, dtype=torch.int64, device="cuda")
    default = t.get_option("placed_copy_bytes")
    assert 16 * 8 * 8 * ((P + 7) // 8) <= default, "the copies of this scene do not fit the default: nothing to compare"

    def side(cap):
        def call():
            t.set_option("placed_copy_bytes", cap)
            t.placed_view_factor_products_device(d_x.data_ptr(), None, out.data_ptr(), rays, SEED, sampling)
        return call

    r = {"copies": timed(torch, side(default)), "straight": timed(torch, side(0)), "copies_again": timed(torch, side(default)), "straight_again": timed(torch, side(0))}
    r["straight_over_copies"] = round(min(r["straight"]["median"], r["straight_again"]["median"]) / min(r["copies"]["median"], r["copies_again"]["median"]), 4)
    got = []
    for cap in (default, 0):
        out.zero_()
        side(cap)()
        torch.cuda.synchronize()
        t.wait_for_gpu()
        got.append(words(out).copy())
    t.set_option("placed_copy_bytes", default)
    assert np.array_equal(got[0], got[1]) and got[0].any(), "the two paths give different words"
    r.update({"placed_primitives": P, "rays_per_triangle": rays, "rays": P * rays, "copy_bytes": 16 * 8 * 8 * ((P + 7) // 8)})
    return r


def record_c(torch):
    row = {}
    t = c3()
    for rays in (1, 4, 16, 64):
        row[f"c3_R{rays}"] = copies_against_straight(torch, t, 1 << 20, rays, "cosine")
        print(json.dumps({"c": {f"c3_R{rays}": row[f"c3_R{rays}"]}}), flush=True)
    t.free()
    t = c5_reduced()
    for rays in (64, 1024):
        row[f"c5_reduced_R{rays}"] = copies_against_straight(torch, t, 5420, rays, "uniform")
        print(json.dumps({"c": {f"c5_reduced_R{rays}": row[f"c5_reduced_R{rays}"]}}), flush=True)
    t.free()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True, choices=["a", "b", "c"])
    ap.add_argument("--out", default="profiles/placed_view_factor_products.json")
    args = ap.parse_args()
    import torch  # before the library: a process initialises ONE HIP runtime, torch's (see _capi.lib)
    assert rc.device_count() > 0, "no GPU visible: nothing is measured on a CPU"
    entry = {"a": record_a, "b": record_b, "c": record_c}[args.record](torch)
    record = json.load(open(args.out)) if os.path.exists(args.out) else {}
    record[args.record] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
