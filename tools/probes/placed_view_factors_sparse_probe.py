"""Dev (GPU): what the sparse matrix between placed primitives costs to build, how large it is, what a bounce on it costs beside a retraced
bounce, and after how many bounces the build has paid for itself.

    python tools/probes/placed_view_factors_sparse_probe.py [--out FILE] [--only NAME]

The scenes are the instanced ones of the sibling probes (tools/probes/placed_view_factor_products_probe.py): C3 -- 256 instances of one
4096-triangle sphere, P = 1 048 576 placed primitives -- at R = 4, 16 and 64, and the reduced C5 (5 420 triangles) as ONE identity instance
at R = 1024.  Both samplings.  Per (scene, R, sampling), everything at the same (R, seed):

  count       rc_placed_view_factors_sparse_device, capacity 0, NULL arrays
  fill        the same call with capacity = nnz (what a caller that knows an upper bound pays)
  build       count + fill, what placed_view_factors_sparse(capacity=None) enqueues
  nnz, bytes  entries, and 8 bytes per entry + 8 per row pointer
  spmv        rc_view_factor_sparse_products_device on the built arrays, mx only: the bounce on the matrix
  retrace     rc_placed_view_factor_products_device, mx only: the bounce without it
  break_even  build / (retrace - spmv): the number of bounces after which building the matrix has paid; "never" if a retrace is not slower

Every timing is taken on one stream with device events around the call: 1 warm-up + 5 recorded calls, median / min / max; spmv and
retrace are alternated A B A B.  The mx words of both bounces are compared.  No figure here is asserted anywhere.

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


def timed(torch, call, warmup=1, reps=5):
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


def c3():
    t = build(rc.scenes.config_c3())
    assert rc.placed_primitive_count(t) == 1 << 20 and t.n_instances() == 256
    return t


def c5_reduced():
    t = build(rc.scenes.config_c5(lon=32, bands=17, wall_k=5))
    assert t.n_primitives() == 5420 and rc.placed_primitive_count(t) == 5420
    return t


def measure(torch, t, P, rays, sampling):
    head = torch.zeros(P + 2, dtype=torch.int64, device="cuda")  # row_ptr[P + 1], then nnz
    nnz_ptr = head.data_ptr() + 8 * (P + 1)

    def count():
        t.placed_view_factors_sparse_device(head.data_ptr(), None, None, 0, nnz_ptr, rays, SEED, sampling)

    row = {"placed_primitives": P, "rays_per_triangle": rays, "rays": P * rays, "sampling": sampling,
           "scratch_bytes": int(t.get_option("vf_sparse_scratch_bytes")), "count": timed(torch, count)}
    torch.cuda.synchronize()
    t.wait_for_gpu()
    nnz = int(head[-1].item())
    entries = torch.zeros((2, max(nnz, 1)), dtype=torch.int32, device="cuda")

    def fill():
        t.placed_view_factors_sparse_device(head.data_ptr(), entries[0].data_ptr(), entries[1].data_ptr(), nnz, nnz_ptr, rays, SEED, sampling)

    row["fill"] = timed(torch, fill)
    torch.cuda.synchronize()
    t.wait_for_gpu()
    assert int(head[-1].item()) == nnz and int(head[P].item()) == nnz
    row["nnz"], row["bytes"] = nnz, 8 * nnz + 8 * (P + 1)
    row["entries_per_row"] = round(nnz / P, 3)
    row["build_ms"] = round(row["count"]["median"] + row["fill"]["median"], 4)

    x = np.random.default_rng(3).integers(0, 1 << 32, P, dtype=np.uint32)
    d_x = torch.from_numpy(x.view(np.int32)).cuda()
    mx_s = torch.zeros(P, dtype=torch.int64, device="cuda")
    mx_r = torch.zeros(P, dtype=torch.int64, device="cuda")

    def spmv():
        t.view_factor_sparse_products_device(P, head.data_ptr(), entries[0].data_ptr(), entries[1].data_ptr(), d_x.data_ptr(), mx_s.data_ptr(), None)

    def retrace():
        t.placed_view_factor_products_device(d_x.data_ptr(), mx_r.data_ptr(), None, rays, SEED, sampling)

    row["spmv"], row["retrace"] = timed(torch, spmv), timed(torch, retrace)
    row["spmv_again"], row["retrace_again"] = timed(torch, spmv), timed(torch, retrace)
    mx_s.zero_(); mx_r.zero_()
    spmv(); retrace()
    torch.cuda.synchronize()
    t.wait_for_gpu()
    a, b = mx_s.cpu().numpy().view(np.uint64), mx_r.cpu().numpy().view(np.uint64)
    assert np.array_equal(a, b) and a.any(), "the bounce on the matrix differs from the retraced one"
    row["checksum"] = int(a.sum(dtype=np.uint64))
    s = min(row["spmv"]["median"], row["spmv_again"]["median"])
    r = min(row["retrace"]["median"], row["retrace_again"]["median"])
    row["retrace_over_spmv"] = round(r / s, 2)
    row["build_over_retrace"] = round(row["build_ms"] / r, 3)
    row["break_even_bounces"] = round(row["build_ms"] / (r - s), 3) if r > s else "never"
    return row


CASES = [("c3_R4", c3, 4), ("c3_R16", c3, 16), ("c3_R64", c3, 64), ("c5_reduced_R1024", c5_reduced, 1024)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/placed_view_factors_sparse.json")
    ap.add_argument("--only", default=None, help="one case name: " + ", ".join(c[0] for c in CASES))
    args = ap.parse_args()
    import torch  # before the library: a process initialises ONE HIP runtime, torch's (see _capi.lib)
    assert rc.device_count() > 0, "no GPU visible: nothing is measured on a CPU"
    record = json.load(open(args.out)) if os.path.exists(args.out) else {}
    scene, made = None, None
    for name, make, rays in CASES:
        if args.only and name != args.only:
            continue
        if made is not make:
            if scene is not None:
                scene.free()
            scene, made = make(), make
        P = rc.placed_primitive_count(scene)
        for sampling in ("uniform", "cosine"):
            row = measure(torch, scene, P, rays, sampling)
            record[f"{name}_{sampling}"] = row
            print(json.dumps({f"{name}_{sampling}": row}), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(record, f, indent=1, sort_keys=True)
                f.write("\n")
    if scene is not None:
        scene.free()


if __name__ == "__main__":
    main()
