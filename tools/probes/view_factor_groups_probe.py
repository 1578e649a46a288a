"""Dev (GPU): what the grouped view-factor call costs beside the tracing alone and beside what a user had before it.

    python tools/probes/view_factor_groups_probe.py [--out FILE] [--full] [--label NAME]

Scenes: the reduced C5 of tools/probes/driver_shapes_probe.py (5 420 triangles x 1024 rays); --full adds C5 at full size (50 028 triangles x
4096 rays = 204.9 M rays).  Groups: the scene's 11 bodies (5 spheres, 6 walls), G = 512 and G = 2048 (contiguous blocks of metadata), and
the identity over the first 4 096 metadata (every other primitive excluded).  Per scene and grouping, on one stream, each call warmed up
and then repeated, timed with device events around the call (memset of the copies and fold inside) -- median / min / max:

  totals            (a) rc_view_factor_totals_device over the same sources and rays, both vectors: the cost of the tracing alone
  fused_uniform     rc_view_factor_groups_device, RC_VF_SAMPLING_UNIFORM, weights, escapes
  fused_cosine      ... RC_VF_SAMPLING_COSINE
                    (the private copies while 128 * 8 * ceil((G * G + G) / 8) bytes fit 256 MiB, else straight onto the caller's words: the row's "path")
  sparse_aggregate  (b) rc_view_factors_sparse_device (capacity from one counting call outside the timing) plus a torch aggregation of the
                    CSR by group (index_add_ of the values at groups[row] * G + groups[col])
  products_calls    (c) G calls of rc_view_factor_products_device (d_mx only) with the indicator vector of one hit group each, plus a
                    torch index_add_ of every mx by source group.  Run at G = 11; for larger G the row holds one call's time x G.

At G = 11 the uniform fused words, (b) and (c) must be equal.

The records "in-tree" and "sweep" of profiles/view_factor_groups.json come from a development build that could force either path (rows
fused_copies / fused_direct; the sweep over G): the switch was removed after the measurement, and this probe times the paths the library
takes.  The entries of several runs (--label) are merged in FILE.  Fails without a GPU."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import raycore_jl_amd as rc  # noqa: E402
from raycore_jl_amd import _capi  # noqa: E402

SEED = 7


def build(cfg):
    t = rc.TLAS(0)
    for verts, meta in cfg["blas"]:
        t.add_geometry(verts, meta)
    for b, xf, ids in cfg["instances"]:
        t.push_instances(b, xf, ids)
    return t.sync()


def timed(torch, call, warmup, reps):
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


def body_groups(n, lon, bands, wall_k):
    """config_c5's bodies in the order of its metadata: 5 spheres of 2 * lon * (bands - 1) triangles, then 6 walls of 2 * wall_k^2."""
    per_sphere, per_wall = 2 * lon * (bands - 1), 2 * wall_k * wall_k
    g = np.concatenate([np.repeat(np.arange(5, dtype=np.uint32), per_sphere), 5 + np.repeat(np.arange(6, dtype=np.uint32), per_wall)])
    assert len(g) == n
    return g


def groupings(n, bodies):
    out = [("bodies_11", bodies, 11)]
    for G in (512, 2048):
        out.append((f"blocks_{G}", (np.arange(n, dtype=np.uint64) * G // n).astype(np.uint32), G))
    ident = np.full(n, 0xFFFFFFFF, np.uint32)
    ident[:4096] = np.arange(4096, dtype=np.uint32)
    out.append(("identity_4096", ident, 4096))
    return out


def scene_rows(torch, name, cfg, shape, rays, reps):
    t = build(cfg)
    n = t.n_primitives()
    L, p = rc.lib(), _capi.ptr
    weights = rc.form_factor_weights(rc.primitive_areas(t), rays)
    d_w = torch.from_numpy(weights.view(np.int32)).cuda()
    tot = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    rows = {"triangles": n, "rays_per_triangle": rays, "rays": n * rays}

    def totals():
        _capi.check(L.rc_view_factor_totals_device(t._h, rays, SEED, 0, n, 0, rays, p(tot.data_ptr()), p(tot.data_ptr() + 8 * n), None))

    rows["totals"] = timed(torch, totals, 3, reps)
    print(json.dumps({name: {"totals": rows["totals"]}}), flush=True)
    # the CSR of (b), built once outside the timing to size its arrays
    head = torch.zeros(n + 2, dtype=torch.int64, device="cuda")
    nnz_ptr = head.data_ptr() + 8 * (n + 1)
    t.view_factors_sparse_device(head.data_ptr(), None, None, 0, nnz_ptr, rays, SEED)
    torch.cuda.synchronize()
    nnz = int(head[-1].item())
    entries = torch.zeros((2, max(nnz, 1)), dtype=torch.int32, device="cuda")
    rows["nnz"] = nnz
    for gname, groups, G in groupings(n, body_groups(n, *shape)):
        d_g = torch.from_numpy(groups.view(np.int32)).cuda()
        g64 = torch.from_numpy(groups.astype(np.int64)).cuda()
        out = torch.zeros(G * G + G, dtype=torch.int64, device="cuda")
        row = {"n_groups": G, "copy_bytes": 128 * 8 * ((G * G + G + 7) // 8)}
        row["path"] = "copies" if row["copy_bytes"] <= 256 << 20 else "direct"

        def fused(sampling, with_weights=True):
            return lambda: t.view_factor_groups_device(d_g.data_ptr(), G, out.data_ptr(), rays, SEED, sampling, d_w.data_ptr() if with_weights else None,
                                                       out.data_ptr() + 8 * G * G)

        row["fused_uniform"] = timed(torch, fused("uniform"), 3, reps)
        row["fused_cosine"] = timed(torch, fused("cosine"), 3, reps)
        keep = {}

        def sparse_aggregate():
            t.view_factors_sparse_device(head.data_ptr(), entries[0].data_ptr(), entries[1].data_ptr(), nnz, nnz_ptr, rays, SEED)
            counts = head[1:n + 1] - head[:n]
            src = torch.repeat_interleave(g64, counts, output_size=nnz)
            dst = g64[entries[0].long() & 0xFFFFFFFF]
            ok = (src < G) & (dst < G)
            m = torch.zeros(G * G, dtype=torch.int64, device="cuda")
            m.index_add_(0, (src * G + dst)[ok], (entries[1].long() & 0xFFFFFFFF)[ok])
            keep["sparse"] = m

        row["sparse_aggregate"] = timed(torch, sparse_aggregate, 1, max(reps // 2, 3))
        x = torch.zeros(n, dtype=torch.int32, device="cuda")
        mx = torch.zeros(n, dtype=torch.int64, device="cuda")

        def one_products_call(b):
            x.copy_((g64 == b).to(torch.int32))
            mx.zero_()
            _capi.check(L.rc_view_factor_products_device(t._h, rays, SEED, 0, n, 0, rays, p(x.data_ptr()), p(mx.data_ptr()), None, None))

        def products_calls():
            m = torch.zeros(G, G, dtype=torch.int64, device="cuda")
            ok = g64 < G
            for b in range(G):
                one_products_call(b)
                m[:, b].index_add_(0, g64[ok], mx[ok])
            keep["products"] = m.reshape(-1)

        if G <= 16:
            row["products_calls"] = timed(torch, products_calls, 1, 3)
        else:
            one = timed(torch, lambda: one_products_call(0), 2, max(reps // 2, 3))
            row["products_calls"] = {"median": round(one["median"] * G, 2), "one_call": one, "extrapolated": True}
        for k in ("fused_uniform", "fused_cosine"):
            if k in row:
                row[k]["over_totals"] = round(row[k]["median"] / rows["totals"]["median"], 4)
                row[k]["over_sparse_aggregate"] = round(row[k]["median"] / row["sparse_aggregate"]["median"], 4)
                row[k]["over_products_calls"] = round(row[k]["median"] / row["products_calls"]["median"], 5)
        # the words: unweighted uniform == (b) == (c)
        out.zero_()
        fused("uniform", False)()
        torch.cuda.synchronize()
        t.wait_for_gpu()
        assert torch.equal(out[:G * G], keep["sparse"]), f"{gname}: the fused call and the aggregated CSR disagree"
        if "products" in keep:
            assert torch.equal(out[:G * G], keep["products"]), f"{gname}: the fused call and the products calls disagree"
        row["checksum"] = int(out.cpu().numpy().view(np.uint64).sum(dtype=np.uint64))
        rows[gname] = row
        print(json.dumps({name: {gname: row}}), flush=True)
        del d_g, g64, out, keep
    t.free()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="in-tree")
    ap.add_argument("--out", default="profiles/view_factor_groups.json")
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    import torch  # before the library: a process initialises ONE HIP runtime, torch's (see _capi.lib)
    assert rc.device_count() > 0, "no GPU visible: nothing is measured on a CPU"
    sc = rc.scenes
    entry = {"library": os.path.basename(_capi.LIB_PATH), "scenes": {}}
    entry["scenes"]["c5_reduced"] = scene_rows(torch, "c5_reduced", sc.config_c5(lon=32, bands=17, wall_k=5), (32, 17, 5), 1024, args.reps)
    assert entry["scenes"]["c5_reduced"]["triangles"] == 5420
    if args.full:
        cfg = sc.config_c5()
        entry["scenes"]["c5_full"] = scene_rows(torch, "c5_full", cfg, (96, 51, 13), cfg["rays_per_triangle"], args.reps)
    record = {}
    if os.path.exists(args.out):
        record = json.load(open(args.out))
    record[args.label] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
