"""Dev (GPU): what the placed view-factor call costs beside its per-triangle sibling, and the workloads it exists for.

    python tools/probes/placed_view_factors_probe.py --record a|b|c [--out FILE] [--full]

One process per record; the records are merged in FILE.  Every timing is taken on one stream with device events around the call (the
zeroing of the copies and the fold inside): 3 warm-up + 9 recorded calls, median / min / max.

  a  the cost of the placed source and sink alone.  The reduced C5 of the other driver probes (5 420 triangles x 1024 rays) as ONE identity
     instance: rc_placed_view_factor_groups_device against rc_view_factor_groups_device in the same process, G = 11 bodies, area weights,
     escapes, both samplings.  The rays are the same bit for bit (the words are compared), so the difference is the functor and the sink.
  b  the workload the feature exists for.  C5 rebuilt from instances -- the room BLAS at identity plus ONE sphere BLAS pushed at the five
     centres --, G = 6 bodies, form factors with cosine sampling: time, Grays/s, and the 6 x 6 matrix beside form_factors() of the flat C5
     with the same body groups.  The two estimates must agree entry by entry within 4 * sqrt(s1^2 + s2^2) of their binomial errors,
     s^2 = F (1 - F) / N_eff with N_eff = R (sum w)^2 / sum w^2 over the source group's weights (the rays of a group are weighted).
     Reduced size; --full adds C5 at full size (50 028 triangles x 4096 rays).
  c  C3: 256 instances of one 4096-triangle sphere, 1 048 576 placed primitives, R = 16, G = 256 (every instance its own group, area
     weights, cosine): time and Grays/s, for the record.

Fails without a GPU."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import raycore_jl_amd as rc  # noqa: E402

SEED = 7
C5_CENTRES = [(-1.2, -1.2, -0.6), (1.2, -1.2, 0.5), (-1.2, 1.2, 0.4), (1.2, 1.2, -0.5), (0.0, 0.0, 0.0)]  # scenes.config_c5's


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


def c5_instanced(lon, bands, wall_k):
    """config_c5 from instances: BLAS 1 = the room at identity, BLAS 2 = one sphere of radius 0.7 about the origin, pushed at the five centres.
    Instance order: the five spheres, then the room -- the order of config_c5's metadata."""
    sc = rc.scenes
    room = np.ascontiguousarray(sc.box_room((-2.5, -2.5, -2.0), (2.5, 2.5, 2.0), wall_k), np.float32)
    sphere = np.ascontiguousarray(sc.fan_sphere(lon, bands, centre=(0, 0, 0), radius=0.7), np.float32)
    xf = np.tile(sc.IDENTITY3x4, (5, 1)).reshape(5, 3, 4)
    xf[:, :, 3] = np.asarray(C5_CENTRES, np.float32)
    return {"blas": [(room, np.arange(1, len(room) + 1, dtype=np.uint32)), (sphere, np.arange(1, len(sphere) + 1, dtype=np.uint32))],
            "instances": [(2, xf.reshape(5, 12), np.arange(5, dtype=np.uint32)), (1, sc.IDENTITY3x4[None], np.full(1, 5, np.uint32))]}


def record_a(torch):
    lon, bands, wall_k, rays, G = 32, 17, 5, 1024, 11
    t = build(rc.scenes.config_c5(lon=lon, bands=bands, wall_k=wall_k))
    n = t.n_primitives()
    assert n == 5420 and rc.placed_primitive_count(t) == n
    per_sphere, per_wall = 2 * lon * (bands - 1), 2 * wall_k * wall_k
    groups = np.concatenate([np.repeat(np.arange(5, dtype=np.uint32), per_sphere), 5 + np.repeat(np.arange(6, dtype=np.uint32), per_wall)])
    weights = rc.form_factor_weights(rc.primitive_areas(t), rays)
    meta = t.adapt().all_blas_prims["meta"].astype(np.int64)
    d_g, d_w, d_gq, d_wq = u32(torch, groups), u32(torch, weights), u32(torch, groups[meta - 1]), u32(torch, weights[meta - 1])
    ref = torch.zeros(G * G + G, dtype=torch.int64, device="cuda")
    out = torch.zeros(G * G + G, dtype=torch.int64, device="cuda")
    row = {"triangles": n, "rays_per_triangle": rays, "rays": n * rays, "n_groups": G}
    for sampling in ("uniform", "cosine"):
        def sibling():
            t.view_factor_groups_device(d_g.data_ptr(), G, ref.data_ptr(), rays, SEED, sampling, d_w.data_ptr(), ref.data_ptr() + 8 * G * G)

        def placed():
            t.placed_view_factor_groups_device(d_gq.data_ptr(), G, out.data_ptr(), rays, SEED, sampling, d_wq.data_ptr(), out.data_ptr() + 8 * G * G)

        # interleaved A B A B: drift of the device's clocks lands on both
        r = {"sibling": timed(torch, sibling), "placed": timed(torch, placed), "sibling_again": timed(torch, sibling), "placed_again": timed(torch, placed)}
        r["placed_over_sibling"] = round(min(r["placed"]["median"], r["placed_again"]["median"]) / min(r["sibling"]["median"], r["sibling_again"]["median"]), 4)
        ref.zero_(); out.zero_()
        sibling(); placed()
        torch.cuda.synchronize()
        t.wait_for_gpu()
        assert np.array_equal(words(ref), words(out)) and words(out).any(), f"{sampling}: the placed words differ from the sibling's"
        r["checksum"] = int(words(out).sum(dtype=np.uint64))
        row[sampling] = r
        print(json.dumps({"a": {sampling: r}}), flush=True)
    t.free()
    return row


def n_eff(weights, groups, G, rays):
    w = weights.astype(np.float64)
    return np.array([rays * w[groups == g].sum() ** 2 / max((w[groups == g] ** 2).sum(), 1.0) for g in range(G)])


def record_b(torch, shape, rays, name):
    lon, bands, wall_k = shape
    G = 6
    per_sphere = 2 * lon * (bands - 1)
    # the flat scene: one BLAS at identity, groups by metadata
    flat = build(rc.scenes.config_c5(lon=lon, bands=bands, wall_k=wall_k))
    n = flat.n_primitives()
    g_flat = np.minimum(np.arange(n, dtype=np.uint32) // per_sphere, 5).astype(np.uint32)
    F1, esc1 = rc.form_factors(flat, g_flat, rays, seed=SEED)
    w1 = rc.form_factor_weights(rc.primitive_areas(flat), rays)
    s1 = F1 * (1 - F1) / n_eff(w1, g_flat, G, rays)[:, None]
    flat.free()
    # the instanced scene
    t = build(c5_instanced(lon, bands, wall_k))
    P = rc.placed_primitive_count(t)
    assert P == n and t.n_instances() == 6
    gq = rc.placed_groups(t)
    wq = rc.form_factor_weights(rc.placed_primitive_areas(t), rays)
    d_g, d_w = u32(torch, gq), u32(torch, wq)
    out = torch.zeros(G * G + G, dtype=torch.int64, device="cuda")

    def call():
        t.placed_view_factor_groups_device(d_g.data_ptr(), G, out.data_ptr(), rays, SEED, "cosine", d_w.data_ptr(), out.data_ptr() + 8 * G * G)

    ms = timed(torch, call)
    out.zero_()
    call()
    torch.cuda.synchronize()
    t.wait_for_gpu()
    F2, esc2 = rc.form_factors_from_counts(words(out)[:G * G].reshape(G, G), words(out)[G * G:], gq, wq, rays)
    F3, _ = rc.instance_form_factors(t, rays, seed=SEED)
    assert np.abs(F3 - F2).max() < 1e-15
    s2 = F2 * (1 - F2) / n_eff(wq, gq, G, rays)[:, None]
    bound = 4 * np.sqrt(s1 + s2)
    dev = np.abs(F1 - F2)
    ratio = np.where(bound > 0, dev / np.where(bound > 0, bound, 1), np.where(dev > 0, np.inf, 0.0))
    row = {"triangles": n, "rays_per_triangle": rays, "rays": n * rays, "n_groups": G, "ms": ms, "grays_per_s": round(n * rays / ms["median"] / 1e6, 3),
           "instanced": np.round(F2, 6).tolist(), "flat": np.round(F1, 6).tolist(), "escaped_instanced": np.round(esc2, 6).tolist(), "escaped_flat": np.round(esc1, 6).tolist(),
           "largest_deviation": float(dev.max()), "largest_deviation_over_bound": float(ratio.max()), "row_sums_instanced": np.round(F2.sum(axis=1) + esc2, 6).tolist()}
    print(json.dumps({"b": {name: row}}), flush=True)
    assert (dev <= bound).all(), f"{name}: the instanced and the flat estimate differ by more than 4 sigma: {dev.max()} (x {ratio.max()} of the bound)"
    t.free()
    return row


def record_c(torch):
    rays, G = 16, 256
    t = build(rc.scenes.config_c3())
    P = rc.placed_primitive_count(t)
    assert P == 1 << 20 and t.n_instances() == G
    gq = rc.placed_groups(t)
    wq = rc.form_factor_weights(rc.placed_primitive_areas(t), rays)
    d_g, d_w = u32(torch, gq), u32(torch, wq)
    out = torch.zeros(G * G + G, dtype=torch.int64, device="cuda")

    def call():
        t.placed_view_factor_groups_device(d_g.data_ptr(), G, out.data_ptr(), rays, SEED, "cosine", d_w.data_ptr(), out.data_ptr() + 8 * G * G)

    ms = timed(torch, call)
    out.zero_()
    call()
    torch.cuda.synchronize()
    t.wait_for_gpu()
    F, esc = rc.form_factors_from_counts(words(out)[:G * G].reshape(G, G), words(out)[G * G:], gq, wq, rays)
    row = {"instances": G, "placed_primitives": P, "rays_per_triangle": rays, "rays": P * rays, "n_groups": G, "ms": ms,
           "grays_per_s": round(P * rays / ms["median"] / 1e6, 3), "largest_factor": float(F.max()), "mean_escaped": float(esc.mean()),
           "largest_row_sum": float((F.sum(axis=1) + esc).max()), "checksum": int(words(out).sum(dtype=np.uint64))}
    print(json.dumps({"c": row}), flush=True)
    t.free()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True, choices=["a", "b", "c"])
    ap.add_argument("--out", default="profiles/placed_view_factors.json")
    ap.add_argument("--full", action="store_true")
    args = ap.parse_args()
    import torch  # before the library: a process initialises ONE HIP runtime, torch's (see _capi.lib)
    assert rc.device_count() > 0, "no GPU visible: nothing is measured on a CPU"
    if args.record == "a":
        entry = {"c5_reduced": record_a(torch)}
    elif args.record == "b":
        entry = {"c5_reduced": record_b(torch, (32, 17, 5), 1024, "c5_reduced")}
        if args.full:
            entry["c5_full"] = record_b(torch, (96, 51, 13), 4096, "c5_full")
    else:
        entry = {"c3": record_c(torch)}
    record = json.load(open(args.out)) if os.path.exists(args.out) else {}
    record[args.record] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
