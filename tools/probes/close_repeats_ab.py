"""Dev (GPU): A/B of the close-repeat rule of cost-ordered claiming on the bench headline's launch sequence.

One process per side and round (a process loads one library): the C3 scene, 40 + W + K launches of 4 Mi jittered primary rays, each its own
device buffer (bench.py's fresh_batch restated: same seeds, same arithmetic), enqueued without waiting; the K timed steps by the wall clock
(what bench.py reports) and by the events each launch carries (rc_recent_kernel_ms: the trace kernel alone, next to the cadence's recording launches -- the
rebuild kernels in front of the following launch are in the wall-clock figure only).

    python tools/probes/close_repeats_ab.py LABEL [LIB] [--close 0|1] [--steps 20] [--warmup 3]

LIB: a library built by tools/ab_build.sh (the parent's, for instance); default the in-tree one.  --close is ignored by a library that does not
know the option.  Prints one line per run; the driver interleaves the sides."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("label")
    ap.add_argument("lib", nargs="?")
    ap.add_argument("--close", type=int, default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--res", type=int, default=2048)
    args = ap.parse_args()
    import raycore_jl_amd as rc
    if args.lib:
        sys.modules[rc.lib.__module__].LIB_PATH = os.path.abspath(args.lib)
    import torch
    sc = rc.scenes
    cfg = sc.config_c3()
    t = rc.TLAS(0)
    for verts, meta in cfg["blas"]:
        t.add_geometry(verts, meta)
    for b, xf, ids in cfg["instances"]:
        t.push_instances(b, xf, ids)
    t.sync()
    close = "n/a"
    if args.close is not None:
        try:
            t.set_option("order_close_repeats", args.close)
            close = str(t.get_option("order_close_repeats"))
        except rc.RaycoreError:
            pass   # the parent's library: it has no such option
    n = args.res * args.res
    stream = torch.cuda.current_stream()

    def fresh_batch(seed):
        g = torch.Generator(device="cuda")
        g.manual_seed(0xC3000 + seed)
        eye = torch.tensor(np.asarray(cfg["eye"], dtype=np.float64), device="cuda")
        f = torch.tensor(sc.normalize(np.asarray(cfg["lattice_centre"], dtype=np.float64) - np.asarray(cfg["eye"], dtype=np.float64)), device="cuda")
        r_ = torch.tensor(sc.normalize(np.cross(f.cpu().numpy(), np.array([0.0, 1.0, 0.0]))), device="cuda")
        u_ = torch.linalg.cross(r_, f)
        half = float(np.tan(np.radians(45.0) / 2))
        w = h = args.res
        px = torch.arange(w, device="cuda", dtype=torch.float64)[None, :] + torch.rand((h, w), generator=g, device="cuda", dtype=torch.float64)
        py = torch.arange(h, device="cuda", dtype=torch.float64)[:, None] + torch.rand((h, w), generator=g, device="cuda", dtype=torch.float64)
        X = (px / w * 2 - 1) * half * (w / h)
        Y = (py / h * 2 - 1) * half
        d = f[None, None, :] + X[..., None] * r_ + Y[..., None] * u_
        d = (d / d.norm(dim=-1, keepdim=True)).reshape(-1, 3)
        out = torch.empty((n, 8), dtype=torch.float32, device="cuda")
        out[:, 0:3] = eye.to(torch.float32)
        out[:, 3] = 0.0
        out[:, 4:7] = d.to(torch.float32)
        out[:, 7] = float("inf")
        return out.view(torch.uint8).reshape(-1)

    clock_warm = 40
    n_launch = clock_warm + args.warmup + args.steps
    fresh = [fresh_batch(i) for i in range(n_launch)]
    hits = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def step(i):
        t.trace_device(fresh[i].data_ptr(), hits.data_ptr(), n, mode="closest", stream=stream.cuda_stream)

    for i in range(clock_warm):
        step(i)
    torch.cuda.synchronize()
    for i in range(args.warmup):
        step(clock_warm + i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(clock_warm + args.warmup + i)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    per_step = t.recent_kernel_ms(min(args.steps, 47))
    hdr = torch.zeros(48, dtype=torch.int32, device="cuda")
    ctypes.CDLL("libamdhip64.so").hipMemcpy(ctypes.c_void_p(hdr.data_ptr()), ctypes.c_void_p(t.get_option("debug_ctl_ptr")), ctypes.c_size_t(192), 3)
    hdr = hdr.cpu().numpy()
    med = float(np.median(per_step))
    # which launches of a shape whose history continues record: its launches 2-4, then the host's cadence (8, then 7, 8, 9, 7, ... launches on)
    rec, nxt, asked = {2, 3, 4}, 8, 0
    while nxt <= n_launch:
        rec.add(nxt)
        nxt, asked = nxt + 7 + asked % 3, asked + 1
    first_timed = n_launch - len(per_step) + 1
    marks = " ".join(f"{x:.4f}{'r' if hdr[4] == 0 and first_timed + i in rec else ''}" for i, x in enumerate(per_step))
    print(f"[{args.label:12s}] close={close:3s} steps={args.steps} {n * args.steps / elapsed / 1e6:8.1f} Mrays/s  {elapsed / args.steps * 1e3:.4f} ms/step by the wall clock; "
          f"kernel mean {float(np.mean(per_step)):.4f} median {med:.4f} ms; last step: fresh {hdr[4]} order {hdr[1]} recorded {hdr[5]} close {hdr[6]} gen {hdr[12 + hdr[0]]} pause {hdr[38]}", flush=True)
    print(f"[{args.label:12s}]   kernel ms per timed step (r = a recording launch, by the cadence of a continuing history): {marks}", flush=True)
    t.free()


if __name__ == "__main__":
    main()
