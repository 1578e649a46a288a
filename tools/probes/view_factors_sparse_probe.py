"""Dev (GPU): what the sparse view-factor matrix costs to build, what a bounce on it costs, and from how many bounces on it pays.

    python tools/probes/view_factors_sparse_probe.py [--lib PATH] [--label NAME] [--out FILE] [--full] [--sweep] [--once SCENE]

Scenes: the reduced C5 of tools/probes/view_factor_products_probe.py (5 420 triangles x 1024 rays); --full adds C5 at full size (50 028
triangles x 4096 rays = 204.9 M rays).  The protocol is that probe's: one stream, every call warmed up and then repeated, device events
around the call, median / min / max.  Per scene:

  totals        rc_view_factor_totals_device, both vectors: traces the rays the build traces -- the floor the sort and compression sit on
  retraced_mx   rc_view_factor_products_device, d_mx only: the bounce as it was
  count         rc_view_factors_sparse_device, capacity 0, NULL arrays
  build         rc_view_factors_sparse_device into arrays of exactly nnz entries; nnz, the bytes of the result (8 nnz + 8 (N + 1))
  spmv_mx / spmv_mtx / spmv   rc_view_factor_sparse_products_device, d_mx only (the bounce) / d_mtx only / both, with the bytes per
                second of nnz x 8 B next to the HBM bandwidth
  break_even    the bounce count k from which build + k spmv_mx < k retraced_mx, and the k = 30 solve both ways
  sweep         (--sweep) the build with option "vf_sparse_scratch_bytes" at 64 MiB .. 2 GiB
The products of the CSR must equal the retraced products word for word, or the probe fails.

--lib times another build of the library (a parent build without the sparse symbols gives the totals and retraced_mx rows only);
--label names the record's entry; the entries of several runs are merged in FILE.  --once SCENE (c5_reduced | c5_full) runs two builds and
two spmv_mx of that scene and writes nothing: the run to put under a kernel-trace profiler for the split between trace, sort, encode and
append.  Fails without a GPU."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import raycore_jl_amd as rc  # noqa: E402
from raycore_jl_amd import _capi  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak


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


class Scene:
    def __init__(self, torch, cfg, rays):
        self.torch, self.t, self.rays = torch, build(cfg), rays
        self.n = n = self.t.n_primitives()
        self.L, self.p = rc.lib(), _capi.ptr
        x = np.random.default_rng(12).integers(0, 1 << 32, n, dtype=np.uint32)
        self.d_x = torch.from_numpy(x.view(np.int32)).cuda()
        self.v = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
        self.head = torch.zeros(n + 2, dtype=torch.int64, device="cuda")
        self.entries = None

    def totals(self):
        a = self.v.data_ptr()
        _capi.check(self.L.rc_view_factor_totals_device(self.t._h, self.rays, 7, 0, self.n, 0, self.rays, self.p(a), self.p(a + 8 * self.n), None))

    def retraced_mx(self):
        _capi.check(self.L.rc_view_factor_products_device(self.t._h, self.rays, 7, 0, self.n, 0, self.rays, self.p(self.d_x.data_ptr()), self.p(self.v.data_ptr()), None, None))

    def count(self):
        h = self.head.data_ptr()
        self.t.view_factors_sparse_device(h, None, None, 0, h + 8 * (self.n + 1), self.rays, 7)

    def nnz(self):
        self.count()
        self.torch.cuda.synchronize()
        return int(self.head[-1].item())

    def allocate(self, nnz):
        self.entries = self.torch.zeros((2, max(nnz, 1)), dtype=self.torch.int32, device="cuda")
        self.capacity = nnz

    def fill(self):
        h = self.head.data_ptr()
        self.t.view_factors_sparse_device(h, self.entries[0].data_ptr(), self.entries[1].data_ptr(), self.capacity, h + 8 * (self.n + 1), self.rays, 7)

    def spmv(self, mx, mtx):
        a = self.v.data_ptr()
        self.t.view_factor_sparse_products_device(self.n, self.head.data_ptr(), self.entries[0].data_ptr(), self.entries[1].data_ptr(), self.d_x.data_ptr(),
                                                  a if mx else None, a + 8 * self.n if mtx else None)


def scene_rows(torch, name, cfg, rays, reps, has_sparse, sweep, lanes):
    s = Scene(torch, cfg, rays)
    n = s.n
    row = {"triangles": n, "rays_per_triangle": rays, "rays": n * rays}
    row["totals"] = timed(torch, s.totals, 3, reps)
    row["retraced_mx"] = timed(torch, s.retraced_mx, 3, reps)
    if has_sparse:
        nnz = s.nnz()
        s.allocate(nnz)
        row["nnz"], row["csr_bytes"], row["dense_bytes"] = nnz, 8 * nnz + 8 * (n + 1), 4 * n * n
        row["fill"] = round(nnz / (n * n), 5)
        row["count"] = timed(torch, s.count, 2, reps)
        row["build"] = timed(torch, s.fill, 2, reps)
        row["build"]["over_totals"] = round(row["build"]["median"] / row["totals"]["median"], 3)
        # the words: the CSR's products against the retraced ones
        s.v.zero_()
        s.retraced_mx()
        torch.cuda.synchronize()
        want = s.v[:n].clone()
        s.v.zero_()
        s.spmv(True, False)
        torch.cuda.synchronize()
        s.t.wait_for_gpu()
        assert torch.equal(s.v[:n], want), "the sparse products and the retraced products disagree"
        row["checksum"] = int(want.cpu().numpy().view(np.uint64).sum(dtype=np.uint64))
        for key, (mx, mtx) in (("spmv_mx", (True, False)), ("spmv_mtx", (False, True)), ("spmv", (True, True))):
            row[key] = timed(torch, lambda: s.spmv(mx, mtx), 5, 3 * reps)
            row[key]["entry_bytes_per_s"] = round(8.0 * nnz / (row[key]["median"] * 1e-3), 0)
            row[key]["of_hbm_peak"] = round(row[key]["entry_bytes_per_s"] / HBM_BYTES_PER_S, 4)
        for lane_count in lanes:  # (a build that still carries the lanes-per-row switch)
            s.t.set_option("vf_sparse_lanes", lane_count)
            row[f"spmv_mx_lanes{lane_count}"] = timed(torch, lambda: s.spmv(True, False), 5, 3 * reps)
            s.t.set_option("vf_sparse_lanes", 64)
        b, sp, re = row["build"]["median"], row["spmv_mx"]["median"], row["retraced_mx"]["median"]
        row["break_even"] = {"bounces": int(np.floor(b / (re - sp))) + 1 if re > sp else None,
                             "solve_30_sparse_ms": round(b + 30 * sp, 3), "solve_30_retraced_ms": round(30 * re, 3),
                             "retraced_over_spmv": round(re / sp, 2)}
        if sweep:
            default = s.t.get_option("vf_sparse_scratch_bytes")
            row["sweep"] = {}
            for mib in (64, 128, 256, 512, 1024, 2048):
                s.t.set_option("vf_sparse_scratch_bytes", mib << 20)
                row["sweep"][f"{mib}MiB"] = timed(torch, s.fill, 2, max(reps // 2, 3))
            s.t.set_option("vf_sparse_scratch_bytes", default)
    s.t.free()
    print(json.dumps({name: row}), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--label", default="in-tree")
    ap.add_argument("--out", default="profiles/view_factors_sparse.json")
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--lanes", type=int, nargs="*", default=[])
    ap.add_argument("--once")
    args = ap.parse_args()
    has_sparse = True
    import torch  # before the library: a process initialises ONE HIP runtime, torch's (see _capi.lib)
    if args.lib:
        _capi.LIB_PATH = os.path.abspath(args.lib)
        exported = C.CDLL(_capi.LIB_PATH)
        has_sparse = hasattr(exported, "rc_view_factors_sparse_device")
        _capi.SYMBOLS[:] = [s for s in _capi.SYMBOLS if hasattr(exported, s[0])]  # (an older build: bind what it has)
    assert rc.device_count() > 0, "no GPU visible: nothing is measured on a CPU"
    sc = rc.scenes
    reduced, full = sc.config_c5(lon=32, bands=17, wall_k=5), sc.config_c5()
    if args.once:
        cfg, rays = (reduced, 1024) if args.once == "c5_reduced" else (full, full["rays_per_triangle"])
        s = Scene(torch, cfg, rays)
        s.allocate(s.nnz())
        for _ in range(2):
            s.fill()
            s.spmv(True, False)
        torch.cuda.synchronize()
        s.t.wait_for_gpu()
        s.t.free()
        return
    entry = {"library": os.path.basename(_capi.LIB_PATH), "scenes": {}}
    entry["scenes"]["c5_reduced"] = scene_rows(torch, "c5_reduced", reduced, 1024, 15, has_sparse, args.sweep, args.lanes)
    assert entry["scenes"]["c5_reduced"]["triangles"] == 5420
    if args.lanes:
        entry["scenes"]["c5_reduced_64_rays"] = scene_rows(torch, "c5_reduced_64_rays", reduced, 64, 15, has_sparse, False, args.lanes)
    if args.full:
        entry["scenes"]["c5_full"] = scene_rows(torch, "c5_full", full, full["rays_per_triangle"], 9, has_sparse, args.sweep, args.lanes)
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
