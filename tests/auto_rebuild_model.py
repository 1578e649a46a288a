"""Numpy model of the gated TLAS rebuild (refit_or_rebuild_device_async): the cost, the refit and the animation the tests run.

Nothing here touches the library's device code.  The trees come from the oracle (oracle.pyoracle.Scene, built from scratch); the model adds

* cost(nodes, n): relative_area of tools/probes/tlas_rebuild_probe.py -- the summed surface area of the internal nodes' boxes (the union of
  the two child boxes, extents in f64 from the f32 corners) relative to the root's; exactly 1.0 for a single leaf;
* refit(topology, leaves_from): the bottom-up refit of an oracle-built topology with the leaf boxes of the oracle built from the new
  transforms -- what refit_tlas! leaves when the instances have moved and the tree has not been sorted again;
* the animation: six frames from the initial lattice -- drift, shuffle, drift, drift, shuffle, drift -- and its walk under RATIO: which
  frames rebuild, what the baseline cost is after each.

drift(seed, amp): every instance keeps its translation, plus a uniform jitter in +-amp (Philox(key = seed)); the linear part is that of
lattice_transforms(*dims, 1.6, seed).  shuffle(key): the translation columns are permuted among the instances (Philox(key)).
"""
import numpy as np

RATIO = 1.5
KINDS = ("drift", "shuffle", "drift", "drift", "shuffle", "drift")
DRIFTS = ((11, 0.1), (12, 0.1), (13, 0.3), (14, 0.1))  # (seed, amp) of the drift frames, in order
SHUFFLE_KEYS = (900, 901)
REBUILDS = tuple(k == "shuffle" for k in KINDS)        # the expected decisions
INVALID = 0xFFFFFFFF
# the conditions on the inputs (asserted on yardsticks alone)
DRIFT_RATIO_MAX, SHUFFLE_RATIO_MIN, DRIFT_LEAF_DIFF_MIN, SHUFFLE_LEAF_DIFF_MIN = 1.25, 3.0, 0.2, 0.9


def animation(sc, dims, initial):
    """The six frames' transforms, float32 (n, 12) each."""
    cur = np.asarray(initial, dtype=np.float32).reshape(-1, 3, 4).copy()
    n = len(cur)
    drifts, keys = iter(DRIFTS), iter(SHUFFLE_KEYS)
    out = []
    for kind in KINDS:
        nxt = cur.copy()
        if kind == "drift":
            seed, amp = next(drifts)
            lin = sc.lattice_transforms(*dims, 1.6, seed)[0].reshape(n, 3, 4)
            jitter = np.random.Generator(np.random.Philox(key=seed)).uniform(-amp, amp, size=(n, 3)).astype(np.float32)
            nxt[:, :, :3] = lin[:, :, :3]
            nxt[:, :, 3] = cur[:, :, 3] + jitter
        else:
            perm = np.random.Generator(np.random.Philox(key=next(keys))).permutation(n)
            nxt[:, :, 3] = cur[perm][:, :, 3]
        cur = nxt
        out.append(np.ascontiguousarray(cur.reshape(n, 12)))
    return out


def cost(nodes, n):
    if n == 1:
        return 1.0
    lo = np.minimum(nodes["aabb0_min"][:n - 1], nodes["aabb1_min"][:n - 1]).astype(np.float64)
    hi = np.maximum(nodes["aabb0_max"][:n - 1], nodes["aabb1_max"][:n - 1]).astype(np.float64)
    e = hi - lo
    area = 2.0 * (e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0])
    return float(area.sum() / area[0])


def leaf_slots_differing(a, b, n):
    """Fraction of the leaf slots (sorted positions) that hold another instance in tree `a` than in tree `b`."""
    return float(np.mean(a["child1"][n - 1:] != b["child1"][n - 1:]))


def refit(topology, leaves_from, n):
    """`topology` (exported nodes, 1-based children, leaves n .. 2n - 1 naming their instance in child1) with every leaf box taken from the
    leaf of the same instance in `leaves_from`, and every internal node's two boxes recomputed bottom-up (f32 min / max: exact)."""
    out = topology.copy()
    src = {int(inst): k for k, inst in enumerate(leaves_from["child1"][n - 1:])}
    for j in range(n - 1, 2 * n - 1):
        leaf = leaves_from[n - 1 + src[int(out["child1"][j])]]
        out["aabb0_min"][j], out["aabb0_max"][j] = leaf["aabb0_min"], leaf["aabb0_max"]
    if n == 1:
        return out
    box = {}

    def box_of(idx):  # 1-based
        if idx >= n:
            return out["aabb0_min"][idx - 1], out["aabb0_max"][idx - 1]
        return box[idx]

    stack = [(1, False)]
    while stack:
        idx, done = stack.pop()
        c0, c1 = int(out["child0"][idx - 1]), int(out["child1"][idx - 1])
        if not done:
            stack.append((idx, True))
            stack.extend((c, False) for c in (c0, c1) if c < n)
            continue
        (a_lo, a_hi), (b_lo, b_hi) = box_of(c0), box_of(c1)
        out["aabb0_min"][idx - 1], out["aabb0_max"][idx - 1] = a_lo, a_hi
        out["aabb1_min"][idx - 1], out["aabb1_max"][idx - 1] = b_lo, b_hi
        box[idx] = (np.minimum(a_lo, b_lo), np.maximum(a_hi, b_hi))
    return out


def oracle_nodes(oracle, mesh, xf):
    o = oracle.Scene()
    b = o.add_blas(mesh)
    for i, x in enumerate(xf):
        o.add_instance(b, x, i)
    o.build()
    return o.tlas_nodes.copy()


def walk(trees_initial, trees_fresh, n, refit_of, ratio=RATIO):
    """The animation under `ratio`.  trees_initial: the nodes built from the initial transforms (what the arming call leaves);
    trees_fresh[f]: the nodes built from scratch with frame f's transforms; refit_of(topology, f) -> the nodes of `topology` refitted to
    frame f.  Per frame: dict(refit_cost, cost_built_before, ratio, rebuild, leaf_diff, cost_built, nodes) -- `nodes` the tree the frame
    leaves, `cost_built` the baseline after it."""
    topology, built = trees_initial, cost(trees_initial, n)
    out = []
    for f, fresh in enumerate(trees_fresh):
        refitted = refit_of(topology, f)
        c = cost(refitted, n)
        rec = {"refit_cost": c, "cost_built_before": built, "ratio": c / built, "rebuild": bool(c > ratio * built),
               "leaf_diff": leaf_slots_differing(fresh, topology, n)}
        if rec["rebuild"]:
            topology, built = fresh, cost(fresh, n)
        else:
            topology = refitted
        rec["cost_built"], rec["nodes"] = built, topology
        out.append(rec)
    return out


def assert_conditions(steps, what):
    """The conditions on the inputs: a decision taken wrongly either way cannot pass a byte comparison of the tree."""
    for f, (kind, st) in enumerate(zip(KINDS, steps)):
        print(f"{what} frame {f} ({kind}): refit cost / cost_built {st['ratio']:.3f}, leaf slots a rebuild would change {st['leaf_diff']:.3f}")
        assert st["rebuild"] == (kind == "shuffle"), (what, f, st["ratio"])
        if kind == "drift":
            assert st["ratio"] <= DRIFT_RATIO_MAX, (what, f, st["ratio"])
            assert st["leaf_diff"] >= DRIFT_LEAF_DIFF_MIN, (what, f, st["leaf_diff"])
        else:
            assert st["ratio"] >= SHUFFLE_RATIO_MIN, (what, f, st["ratio"])
            assert st["leaf_diff"] >= SHUFFLE_LEAF_DIFF_MIN, (what, f, st["leaf_diff"])
