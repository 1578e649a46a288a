"""Dev (GPU): what the view-factor products cost beside the totals call and beside what a user had before them.

    python tools/probes/view_factor_products_probe.py [--lib PATH] [--label NAME] [--out FILE] [--full] [--baseline]

Scenes: the reduced C5 of tools/probes/driver_shapes_probe.py (5 420 triangles x 1024 rays); --full adds C5 at full size (50 028 triangles x
4096 rays = 204.9 M rays).  Per scene, on one stream, each call warmed up and then repeated, timed with device events around the call (so
the zeroing of the scratch copies and the fold are inside) -- median / min / max:

  totals          rc_view_factor_totals_device, both vectors: the yardstick (same rays, same number of atomics on the hot vector)
  products        rc_view_factor_products_device, both vectors, x = seeded full-range u32
  products_mx     ... d_mx only (what a bounce needs)
  products_mtx    ... d_mtx only
  matrix_product  (--baseline) what a user had: zero an N x N u32 device matrix, rc_view_factors_device into it, widen it to int64 and
                  multiply it with x in torch (torch has no u32 or int64 matrix-vector product on the device: the product is a broadcast
                  multiply and a row sum) -- with the peak of torch's allocator; its mx must equal the products' words

--lib times another build of the library (a parent build without the products symbols gives the totals row only); --label names the
record's entry; the entries of several runs are merged in FILE.  Fails without a GPU."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import raycore_jl_amd as rc  # noqa: E402
from raycore_jl_amd import _capi  # noqa: E402


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


def scene_rows(torch, name, cfg, rays, reps, has_products, baseline):
    t = build(cfg)
    n = t.n_primitives()
    L, p = rc.lib(), _capi.ptr
    x = np.random.default_rng(12).integers(0, 1 << 32, n, dtype=np.uint32)
    d_x = torch.from_numpy(x.view(np.int32)).cuda()
    v = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    a, b = v.data_ptr(), v.data_ptr() + 8 * n
    row = {"triangles": n, "rays_per_triangle": rays, "rays": n * rays}

    def totals():
        _capi.check(L.rc_view_factor_totals_device(t._h, rays, 7, 0, n, 0, rays, p(a), p(b), None))

    def products(mx, mtx):
        return lambda: _capi.check(L.rc_view_factor_products_device(t._h, rays, 7, 0, n, 0, rays, p(d_x.data_ptr()), p(mx) if mx else None, p(mtx) if mtx else None, None))

    row["totals"] = timed(torch, totals, 3, reps)
    if has_products:
        row["products"] = timed(torch, products(a, b), 3, reps)
        row["products_mx"] = timed(torch, products(a, None), 3, reps)
        row["products_mtx"] = timed(torch, products(None, b), 3, reps)
        for k in ("products", "products_mx", "products_mtx"):
            row[k]["over_totals"] = round(row[k]["median"] / row["totals"]["median"], 4)
        v.zero_()
        products(a, b)()
        torch.cuda.synchronize()
        t.wait_for_gpu()
        want = v.clone()
        row["checksum"] = int(want.cpu().numpy().view(np.uint64).sum(dtype=np.uint64))
    if baseline and has_products:
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        x64 = torch.from_numpy(x.astype(np.int64)).cuda()
        out = {}

        def matrix_product():
            m = torch.zeros(n * n, dtype=torch.int32, device="cuda")  # [src + N * dst], the reference's column-major matrix
            _capi.check(L.rc_view_factors_device(t._h, rays, 7, 0, n, 0, rays, p(m.data_ptr()), 1, n, 0, 0, None))
            mm = m.view(n, n).to(torch.int64) & 0xFFFFFFFF  # mm[dst, src]
            out["mx"] = (mm * x64[:, None]).sum(dim=0)      # (M x)[src] = sum_dst M[src, dst] x[dst], modulo 2^64
            del m, mm

        row["matrix_product"] = timed(torch, matrix_product, 1, max(reps // 3, 3))
        row["matrix_product"]["peak_bytes"] = int(torch.cuda.max_memory_allocated() - before)
        row["matrix_product"]["over_products_mx"] = round(row["matrix_product"]["median"] / row["products_mx"]["median"], 2)
        assert torch.equal(out["mx"], want[:n]), "the matrix product and the products call disagree"
    t.free()
    print(json.dumps({name: row}), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--label", default="in-tree")
    ap.add_argument("--out", default="profiles/view_factor_products.json")
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--baseline", action="store_true")
    args = ap.parse_args()
    has_products = True
    import torch  # before the library: a process initialises ONE HIP runtime, torch's (see _capi.lib)
    if args.lib:
        _capi.LIB_PATH = os.path.abspath(args.lib)
        exported = C.CDLL(_capi.LIB_PATH)
        has_products = hasattr(exported, "rc_view_factor_products_device")
        _capi.SYMBOLS[:] = [s for s in _capi.SYMBOLS if hasattr(exported, s[0])]  # (an older build: bind what it has)
    assert rc.device_count() > 0, "no GPU visible: nothing is measured on a CPU"
    sc = rc.scenes
    entry = {"library": os.path.basename(_capi.LIB_PATH), "scenes": {}}
    cfg = sc.config_c5(lon=32, bands=17, wall_k=5)
    entry["scenes"]["c5_reduced"] = scene_rows(torch, "c5_reduced", cfg, 1024, 15, has_products, args.baseline)
    assert entry["scenes"]["c5_reduced"]["triangles"] == 5420
    if args.full:
        cfg = sc.config_c5()
        entry["scenes"]["c5_full"] = scene_rows(torch, "c5_full", cfg, cfg["rays_per_triangle"], 9, has_products, args.baseline)
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
