"""Dev (CPU, oracle only): how good a predictor of a launch's chunk costs is the PREVIOUS frame of a still or slowly turning camera?

The close-repeat rule of cost-ordered claiming (order_select, raycore.jl_amd/csrc/rc_traverse_core.h) lets a launch whose sample origins equal a
remembered batch's and whose direction term lies below kCloseDirMax (rc_traverse.hip) claim through the order learned from that batch.  This
probe sweeps what the bound has to separate: C3 at 2048 x 2048, the cost of a 128-ray chunk = the largest node-fetch count of its rays
(oracle counters), the order built from the predecessor's costs the way k_order_scatter builds it (threshold at the median cost: half of the
chunks report; nine classes linear between the threshold and the largest cost, longest first, chunk ids ascending inside a class; the
unreported chunks behind them in natural order), applied to a frame with ANOTHER jitter seed from a camera turned in place by the given angle.

Columns: the direction term of order_select (mean over its 64 sample rays of |dd|^2 / |d|^2, float32), Spearman's rank correlation of
predecessor and true chunk costs, the overlap of their top 10 % / 30 % sets, and the share of the truly longest 5 % of the chunks that the
order claims in the last 30 % of the launch (natural order: what a launch without an order does).  The bound to keep: the largest direction
term at which that share stays within 2 x the jitter row's.

    python tools/probes/close_repeat_predictor.py [--res 2048] [--threads N] > profiles/close_repeat_predictor.txt"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

POOL, CLASSES = 128, 10


def turned(eye, look_at, degrees):
    a = np.radians(degrees)
    v = look_at - eye
    return eye + np.array([np.cos(a) * v[0] + np.sin(a) * v[2], v[1], -np.sin(a) * v[0] + np.cos(a) * v[2]])


def direction_term(rays, prev):
    n = len(rays)
    lane = np.arange(64, dtype=np.int64)
    idx = np.minimum(lane * n // 64 + n // 128, n - 1)
    d, p = rays["d"][idx].astype(np.float32), prev["d"][idx].astype(np.float32)
    dd = ((d - p) ** 2).sum(axis=1, dtype=np.float32)
    nn = np.maximum((d * d).sum(axis=1, dtype=np.float32), (p * p).sum(axis=1, dtype=np.float32))
    return float(np.mean(dd / nn, dtype=np.float32)), bool(np.array_equal(rays["o"][idx], prev["o"][idx]))


def chunk_costs(o, rays, threads):
    _, cnt = o.trace(rays, nthreads=threads, counters=True)
    c = cnt[:, 0]
    pad = (-len(c)) % POOL
    return np.concatenate([c, np.zeros(pad, dtype=c.dtype)]).reshape(-1, POOL).max(axis=1).astype(np.int64)


def learned_order(cost):
    """k_order_scatter's order from one recording whose threshold let half of the chunks report"""
    thr, top = int(np.median(cost)), int(cost.max())
    span = max(top - thr + 1, 1)
    q = np.maximum(cost - thr, 0) * (CLASSES - 1) // span
    cls = np.where(cost <= thr, CLASSES - 1, np.where(q >= CLASSES - 1, 0, CLASSES - 2 - q))
    return np.argsort(cls, kind="stable")


def ranks(x):
    r = np.empty(len(x), dtype=np.float64)
    order = np.argsort(x, kind="stable")
    r[order] = np.arange(len(x))
    for v in np.unique(x):   # ties share their mean rank
        m = x == v
        r[m] = r[m].mean()
    return r


def row(name, term, pred, true, order):
    n = len(true)
    late = np.zeros(n, dtype=bool)
    late[order[int(0.7 * n):]] = True
    longest = np.argsort(-true, kind="stable")[: n // 20]
    share = late[longest].mean()
    if pred is None:
        return f"{name:34s} {'-':>10s} {'-':>9s} {'-':>8s} {'-':>8s} {share:10.4f}", share
    rho = np.corrcoef(ranks(pred), ranks(true))[0, 1]
    def overlap(f):
        k = int(f * n)
        return len(np.intersect1d(np.argsort(-pred, kind="stable")[:k], np.argsort(-true, kind="stable")[:k])) / k
    return f"{name:34s} {term:10.2e} {rho:9.3f} {overlap(0.1):8.3f} {overlap(0.3):8.3f} {share:10.4f}", share


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=2048)
    ap.add_argument("--threads", type=int, default=min(64, os.cpu_count() or 1))
    args = ap.parse_args()
    import raycore_jl_amd as rc
    from oracle import pyoracle
    sc = rc.scenes
    cfg = sc.config_c3()
    o = pyoracle.Scene()
    for verts, meta in cfg["blas"]:
        o.add_blas(verts, meta)
    for b, xf, ids in cfg["instances"]:
        for x, i in zip(xf, ids):
            o.add_instance(b, x, int(i))
    o.build()
    eye, centre = np.asarray(cfg["eye"], dtype=np.float64), np.asarray(cfg["lattice_centre"], dtype=np.float64)
    prev = sc.pinhole_rays(args.res, args.res, eye, centre, 45.0, jitter_seed=0)
    pred = chunk_costs(o, prev, args.threads)
    order = learned_order(pred)
    print(f"C3, {args.res} x {args.res} primary rays, {len(pred)} chunks of {POOL}; the order is learned from jitter seed 0 and applied to jitter seed 1 of the camera turned in place")
    print(f"{'applied to':34s} {'dir term':>10s} {'Spearman':>9s} {'top 10%':>8s} {'top 30%':>8s} {'longest 5% claimed in the last 30%':>10s}")
    rows, base = [], None
    for deg in (0.0, 0.02, 0.1, 0.15, 0.2, 0.3, 0.5, 1.0, 2.0, 5.0):
        cur = sc.pinhole_rays(args.res, args.res, eye, turned(eye, centre, deg), 45.0, jitter_seed=1)
        true = chunk_costs(o, cur, args.threads)
        term, same_o = direction_term(cur, prev)
        assert same_o
        if deg == 0.0:
            print(row("natural order (no order learned)", 0.0, None, true, np.arange(len(true)))[0])
        line, share = row("jitter seed 0 -> seed 1" if deg == 0.0 else f"turned in place by {deg:g} degrees", term, pred, true, order)
        print(line, flush=True)
        if deg == 0.0:
            base = share
        rows.append((term, share))
    ok = [t for t, s in rows if s <= 2 * base]
    worst_ok = max(ok)
    first_bad = min([t for t, s in rows if s > 2 * base and t > worst_ok], default=float("inf"))
    print(f"jitter row: {base:.4f}; within 2 x of it up to a direction term of {worst_ok:.2e}, beyond it from {first_bad:.2e}")
    for res in ((256, 256), (1280, 800), (2048, 2048)):
        a, b = (sc.pinhole_rays(res[0], res[1], eye, centre, 45.0, jitter_seed=s) for s in (0, 1))
        print(f"jitter against jitter at {res[0]} x {res[1]}: direction term {direction_term(b, a)[0]:.2e}")


if __name__ == "__main__":
    main()
