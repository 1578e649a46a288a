"""What makes tests/test_gpu_lifecycle_walk.py's walks trustworthy, checked without a GPU on the model and the oracle alone
(tests/lifecycle_model.py): the committed seeds cover every operation, refusal, gate outcome and update-then-commit pair; the rays of
every check point are live; the model's legality agrees with a table copied from the header; the generator is deterministic."""
import os
import re
from collections import Counter

import numpy as np
import pytest

import lifecycle_model as lm

N_OPS = 120
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "raycore_mi355x.h")


_surveys = {}
SUB_FORMS = ([("ugd", f) for f in ("same", "degen", "wrong")] + [("umd", 0), ("umd", 1)] + [("ibr", how) for how in (0, 1, "refit", "rebuild")]
             + [("utd", "shared")] + [("pending", r) for r in lm.READERS] + [("vf", "after a device geometry update")])


def walk_stats(oracle, seed, regime, n_ops=N_OPS, prime=False):
    """One walk run on the model with the oracle: operation and sub-form counts, refusals, gate decisions (those of replayed captured
    chains on scenes of two or more instances apart), (update, commit) pairs, the liveness of every check point.  prime: read the oracle's
    scene after every operation, as the GPU runner's readers and check points do."""
    ops = lm.walk(seed, regime, n_ops)
    assert len(ops) == n_ops
    s = {"ops": Counter(op[0] for op in ops), "sub": Counter(), "errors": Counter(), "gates": Counter(), "captured_gates": set(), "live": [],
         "counts": [], "outcomes": []}
    order = {"valid": False, "deformed": False}  # the view-factor source order: sorted by a vf call, invalidated by a geometry update

    def after(k, op, out, m):
        s["outcomes"].append(repr(out))
        if prime:
            lm.oracle_scene(oracle, m)
        if out.error is not None:
            s["errors"][out.error] += 1
        if out.gate is not None:
            s["gates"][out.gate] += 1
            if op[0] == "replay" and m.n_total() >= 2:
                s["captured_gates"].add(out.gate)
        if out.error is None and op[0] == "ugd":
            s["sub"]["ugd", op[2]] += 1
        if out.error is None and op[0] == "umd":
            s["sub"]["umd", op[3]] += 1
        if out.error is None and op[0] == "ibr":
            s["sub"]["ibr", op[3]] += 1
        if out.error is None and op[0] == "utd" and len(m.handles_of(m.handles[op[1]].geom)) > 1:
            s["sub"]["utd", "shared"] += 1
        if out.action == "rebuild":
            order["valid"] = order["deformed"] = False
        elif out.error is None and (op[0] in ("ugd", "umd") or (op[0] == "replay" and m.captured[1])):
            order["deformed"] = order["valid"]
        elif out.error is None and op[0] == "vf":  # a vf that finds an order sorted BEFORE the update: only the invalidation saves it
            s["sub"]["vf", "after a device geometry update"] += int(order["deformed"])
            order["valid"], order["deformed"] = True, False
        if op[0] in lm.READERS and m.dev_pending:
            s["sub"]["pending", op[0]] += 1
        if out.commit is not None and m.clean:
            rays, aimed = lm.checkpoint_rays(oracle, m, k)
            hits = lm.oracle_scene(oracle, m).trace(rays)
            assert len(rays) <= lm.N_WORLD_RAYS + lm.N_AIMED_MAX
            s["live"].append((seed, k, m.n_total(), len(aimed)) + lm.liveness(hits, aimed))
            s["counts"].append(m.n_total())
            m.touched.clear()

    m, _ = lm.run(ops, oracle, after)
    s["pairs"] = {(u, c) for kinds, c in m.updates_before_commit for u in kinds}
    s["margins"] = [abs(c / bound - 1.0) for c, bound in m.trees.decisions]
    seen = s["counts"]
    first_empty = next((i for i, n in enumerate(seen) if n == 0 and i > 0 and max(seen[:i]) > 0), None)
    s["refill"] = first_empty is not None and max(seen[first_empty:]) > 0
    return s


def survey(oracle, regime):
    """Every committed walk of `regime`, summed.  Computed once, shared, left unchanged."""
    if regime in _surveys:
        return _surveys[regime]
    s = {"ops": Counter(), "sub": Counter(), "errors": Counter(), "gates": Counter(), "pairs": set(), "live": [], "margins": [], "counts": [],
         "refill": False, "both_captured_gates": False}
    for seed in lm.SEEDS[regime]:
        w = walk_stats(oracle, seed, regime)
        for f in ("ops", "sub", "errors", "gates"):
            s[f] += w[f]
        for f in ("live", "margins", "counts"):
            s[f] += w[f]
        s["pairs"] |= w["pairs"]
        s["refill"] = s["refill"] or w["refill"]
        s["both_captured_gates"] = s["both_captured_gates"] or w["captured_gates"] == {True, False}
    _surveys[regime] = s
    return s


@pytest.mark.parametrize("regime", list(lm.SEEDS))
def test_coverage_of_the_committed_seeds(oracle, regime):
    s = survey(oracle, regime)
    print(regime, dict(s["ops"]), dict(s["errors"]), dict(s["gates"]), sorted(s["pairs"]))
    assert len(lm.SEEDS[regime]) == 3
    for kind in lm.OP_KINDS:
        assert s["ops"][kind] >= 3, f"{regime}: operation {kind} runs {s['ops'][kind]} times over the seeds"
    for code in (lm.RC_ERR_NOT_SYNCED, lm.RC_ERR_INVALID_HANDLE, lm.RC_ERR_INVALID_ARGUMENT, lm.RC_ERR_GEOMETRY_CHANGED):
        assert s["errors"][code] >= 1, f"{regime}: no call is refused with {lm.ERROR_NAMES[code]}"
    assert s["gates"][True] >= 1 and s["gates"][False] >= 1, f"{regime}: gate outcomes {dict(s['gates'])}"
    for update in lm.DEVICE_UPDATES:
        for commit in lm.COMMITS:
            assert (update, commit) in s["pairs"], f"{regime}: no {commit} commits a {update}"
    # a decision within rounding of its threshold would make the walk depend on the device's summation order: 1e-6 is five decades above
    # the 1e-11 the cost is compared at
    assert min(s["margins"]) >= 1e-6, (regime, min(s["margins"]))
    for form in SUB_FORMS:  # the forms of one operation name, and every reader between a device update and its commit
        assert s["sub"][form] >= 1, f"{regime}: {form} never runs"
    if regime != "tiny":  # (two instances cost exactly 1.0 whatever the tree: one ratio cannot take both decisions there)
        assert s["both_captured_gates"], f"{regime}: no walk replays a captured gated commit that takes both decisions on two or more instances"
    lo, hi = lm.REGIMES[regime]["lo"], lm.REGIMES[regime]["hi"]
    after_first = [n for n in s["counts"] if n > 0] if regime != "tiny" else s["counts"]
    assert all(lo <= n <= hi for n in after_first), (regime, min(after_first), max(after_first))
    if regime == "tiny":
        assert {0, 1, 2} <= set(s["counts"]) and s["refill"], "the tiny walks pass through 0, 1 and 2 instances and refill after draining"


@pytest.mark.parametrize("regime", list(lm.SEEDS))
def test_every_check_point_is_live(oracle, regime):
    """At least a fifth of the check point's rays hit, at least four fifths of the touched instances are the closest hit of one of their
    own aimed rays -- on the oracle's output.  (The empty scene has nothing to hit.)"""
    s = survey(oracle, regime)
    assert len(s["live"]) >= 3 * 15
    for seed, k, n, n_aimed, hit, own in s["live"]:
        if n == 0:
            assert hit == 0.0
            continue
        assert hit >= 0.2, f"{regime} seed {seed} op {k}: {hit:.3f} of the rays hit ({n} instances)"
        assert own >= 0.8, f"{regime} seed {seed} op {k}: {own:.3f} of the {n_aimed} touched instances are seen by their own rays"


# entry point x state -> outcome, one line per rule, with the line of include/raycore_mi355x.h that states it and a few of its words
# states: "unsynced" (never synced), "clean", "host" (a push pending), "host_xf" (a host update_transforms pending), "device" (a device
# update pending), and the handles "gone" (deleted and compacted away), "soup" (live, plain soup), "mesh" (live, indexed mesh)
N, H, A = lm.RC_ERR_NOT_SYNCED, lm.RC_ERR_INVALID_HANDLE, lm.RC_ERR_INVALID_ARGUMENT
TABLE = [
    # (header line, words on it, state, operation, outcome)
    (146, "instance count", "clean", ("update_transforms", "soup", 7, 3, 2.0), A),       # m must equal the handle's instance count
    (53, "Handle has been deleted", "clean", ("update_transforms", "gone", 7, 2, 2.0), H),
    (150, "idempotent", "clean", ("delete", "gone"), None),
    (53, "Handle has been deleted", "clean", ("get_instances", "gone"), H),
    (160, "0 = no-op, 1 = refit, 2 = rebuild", "unsynced", ("sync",), "rebuild"),
    (160, "0 = no-op, 1 = refit, 2 = rebuild", "clean", ("sync",), "noop"),
    (160, "0 = no-op, 1 = refit, 2 = rebuild", "host", ("sync",), "rebuild"),
    (146, "refit on the next rc_sync", "host_xf", ("sync",), "refit"),
    (565, "rc_sync, which then refits", "device", ("sync",), "refit"),
    (548, "inside the synced scene", "host_xf", ("ibr", "soup", 7, 1, 2.0), N),
    (548, "inside the synced scene", "device", ("ibr", "soup", 7, 1, 2.0), N),
    (548, "inside the synced scene", "clean", ("ibr", "soup", 7, 0, 2.0), None),
    (567, "m != the handle's count", "clean", ("utd", "soup", 7, 3, 2.0), A),
    (568, "unknown or deleted handle", "clean", ("utd", "gone", 7, 2, 2.0), H),
    (568, "never synced, or pending host-side mutations", "unsynced", ("utd", "soup", 7, 2, 2.0), N),
    (568, "never synced, or pending host-side mutations", "host", ("utd", "soup", 7, 2, 2.0), N),
    (568, "never synced, or pending host-side mutations", "host_xf", ("utd", "soup", 7, 2, 2.0), N),
    (568, "never synced, or pending host-side mutations", "device", ("utd", "soup", 7, 2, 2.0), None),  # device updates compose
    (565, "queries fail with RC_ERR_NOT_SYNCED", "device", ("trace",), N),
    (565, "queries fail with RC_ERR_NOT_SYNCED", "device", ("exports",), N),
    (565, "queries fail with RC_ERR_NOT_SYNCED", "device", ("collide",), N),
    (565, "queries fail with RC_ERR_NOT_SYNCED", "device", ("vf",), N),
    (565, "queries fail with RC_ERR_NOT_SYNCED", "device", ("shading",), N),
    (565, "queries fail with RC_ERR_NOT_SYNCED", "device", ("save_load",), N),
    (586, "is harmless: the update stays pending", "device", ("get_instances", "soup"), None),
    (613, "pending host-side mutations", "host", ("rebuild",), N),
    (613, "pending host-side mutations", "host_xf", ("refit",), N),
    (613, "pending host-side mutations", "unsynced", ("refit",), N),
    (613, "pending host-side mutations", "device", ("rebuild",), None),
    (613, "pending host-side mutations", "clean", ("refit",), None),  # "with none since the last refit ... derived from the descriptors"
    (659, "pending host-side mutations", "host", ("gated", 1.5), N),
    (659, "pending host-side mutations", "device", ("gated", 1.5), None),
    (667, "pending host-side mutations: the block", "host", ("quality",), N),
    (667, "pending host-side mutations: the block", "device", ("quality",), None),
    (717, "unknown or deleted handle", "clean", ("ugd", "gone", "same", 9), H),
    (718, "pending host-side mutations", "host", ("ugd", "soup", "same", 9), N),
    (718, "pending host-side mutations", "device", ("ugd", "soup", "same", 9), None),
    (725, "a geometry that is not a mesh", "clean", ("umd", "soup", 9, 0), A),
    (725, "a geometry that is not a mesh", "clean", ("umd", "mesh", 9, 1), None),
    (443, "A geometry without a BLAS4", "clean", ("blas4_trace", "soup"), N),
    (443, "A geometry without a BLAS4", "host", ("blas4_build", "soup"), None),
]
# rules that take more than one call: (header line, words, operations after "clean", the outcomes of the last ones)
SEQUENCES = [
    (693, "return RC_ERR_GEOMETRY_CHANGED, once", [("ugd", "soup", "wrong", 9), ("refit",), ("wait",), ("wait",)], [lm.RC_ERR_GEOMETRY_CHANGED, None]),
    (695, "which then refits, action 1", [("ugd", "soup", "same", 9), ("trace",), ("sync",)], [N, "refit"]),
    (700, "At call time the geometry's BLAS4 is dropped", [("blas4_build", "soup"), ("blas4_trace", "soup"), ("ugd", "soup", "wrong", 9), ("blas4_trace", "soup")], [None, None, N]),
    (700, "At call time the geometry's BLAS4 is dropped", [("blas4_build", "mesh"), ("umd", "mesh", 9, 0), ("rebuild",), ("blas4_trace", "mesh")], [None, N]),
    (651, "counted as one evaluation and one rebuild", [("gated", 1.5), ("quality",)], [None, None]),
]
ARMED = {"armed": True, "evaluations": 1, "rebuilds": 1, "last_rebuilt": True}  # the state block the last sequence leaves


HANDLES = {"soup": 0, "mesh": 1, "gone": 2}  # the handle ordinals model_in() creates


def model_in(state):
    m = lm.Model()
    for op in [("push", "fan", 1, 2, 3, 2.0), ("push_mesh", 4, 2, 5, 2.0), ("push", "tri", 6, 2, 7, 2.0)]:
        m.apply(op)
    if state == "unsynced":
        return m
    for op in [("sync",), ("delete", 2), ("sync",)]:
        m.apply(op)
    extra = {"clean": [], "host": [("push", "tri", 8, 1, 9, 2.0)], "host_xf": [("update_transforms", 0, 11, 2, 2.0)], "device": [("utd", 1, 12, 2, 2.0)]}[state]
    for op in extra:
        assert m.apply(op).error is None
    return m


def resolve(op):
    return tuple(HANDLES[a] if isinstance(a, str) and a in HANDLES else a for a in op)


def outcome_of(out):
    return out.action if out.action is not None else out.error


def test_legality_table_cites_the_header():
    lines = open(HEADER).read().split("\n")
    for row in TABLE + SEQUENCES:
        line, words = row[0], row[1]
        near = " ".join(re.sub(r"^\s*\*\s?", "", x) for x in lines[line - 1:line + 1])
        assert words in near, f"include/raycore_mi355x.h:{line} no longer says {words!r}: the rule moved or changed -- update the table AND the model"


@pytest.mark.parametrize("row", range(len(TABLE)))
def test_model_follows_the_legality_table(row):
    line, words, state, op, want = TABLE[row]
    m = model_in(state)
    before = (m.counts(), m.host_pending, sorted(m.dev_pending), m.version)
    out = m.apply(resolve(op))
    assert outcome_of(out) == want, f"header line {line} ({words}): {op} in state {state} gives {out}"
    if out.error is not None:
        assert (m.counts(), m.host_pending, sorted(m.dev_pending), m.version) == before, "a refused call moved the model"


@pytest.mark.parametrize("row", range(len(SEQUENCES)))
def test_model_follows_the_multi_call_rules(row):
    line, words, ops, want = SEQUENCES[row]
    m = model_in("clean")
    outs = [m.apply(resolve(op)) for op in ops]
    assert [outcome_of(o) for o in outs[-len(want):]] == want, f"header line {line} ({words}): {outs}"
    if ops[0][0] == "gated":
        assert m.quality() == ARMED


def test_a_rebuilding_sync_compacts_and_disarms():
    m = model_in("clean")  # (one handle deleted and compacted away: its geometry left with it)
    assert m.counts() == (4, 4, 2) and not m.valid(2) and m.tree == "fresh"
    m.apply(("gated", 1.5))
    assert m.armed
    m.apply(("delete", 1))
    assert m.counts() == (2, 4, 2)  # deleted instances and their geometry stay until the rebuilding sync
    assert m.apply(("sync",)).action == "rebuild"
    assert m.counts() == (2, 2, 1) and not m.armed and m.quality()["evaluations"] == 0
    assert m.apply(("update_transforms", 0, 3, 2, 2.0)).error is None and m.apply(("sync",)).commit == "refitted"


@pytest.mark.parametrize("regime", list(lm.SEEDS))
def test_outcomes_do_not_depend_on_who_read_the_oracle_scene(oracle, regime):
    """The GPU runner reads the model's oracle scene after almost every operation, this file's survey only at check points: the
    predictions -- the gate of a replayed captured chain among them -- must be the same either way."""
    for seed in lm.SEEDS[regime]:
        assert walk_stats(oracle, seed, regime, prime=True)["outcomes"] == walk_stats(oracle, seed, regime)["outcomes"], (regime, seed)


def test_replayed_gate_is_decided_from_the_replays_own_transforms(oracle):
    """Two handles, an arming call, a captured gated chain, replays alternating a tight and a wide cloud: every replay's refitted tree
    costs more than 1.0001 x the tree built one frame earlier, whether or not the oracle's scene was read in between."""
    ops = [("push", "fan", 1, 50, 2, 6.0), ("push", "fan", 3, 50, 4, 6.0), ("sync",), ("gated", 1.0001), ("capture", 0, False, "gated", 1.0001)]
    ops += [("replay", 10 + r, 0, 40.0 if r % 2 else 6.0) for r in range(5)]
    gates = []
    for prime in (False, True):
        _, outs = lm.run(ops, oracle, (lambda k, op, out, m: lm.oracle_scene(oracle, m)) if prime else None)
        gates.append([o.gate for o in outs[-5:]])
    assert gates[0] == gates[1] == [True] * 5, gates


def test_generator_is_deterministic_and_prefix_closed():
    for regime in lm.REGIMES:
        seed = lm.SEEDS.get(regime, (1,))[0]
        a, b = lm.walk(seed, regime, N_OPS), lm.walk(seed, regime, N_OPS)
        assert a == b and len(a) == N_OPS
        assert lm.walk(seed, regime, 37) == a[:37]  # any prefix is itself a walk
        assert repr(a) == repr(eval(repr(a)))       # plain data: a failing prefix can be pasted as it is printed
        assert a != lm.walk(seed + 1, regime, N_OPS)


def test_geometry_pool(oracle):
    for kind in lm.SOUP_KINDS:
        for seed in (1, 2, 7):
            for form, extra in (("same", 0), ("degen", 0), ("wrong", 1)):
                o = oracle.Scene()
                o.add_instance(o.add_blas(lm.soup(kind, seed, form)))
                o.build()
                assert len(o.blas_prims) == lm.N_VALID[kind] + extra, (kind, seed, form)
                assert o.blas_prims["meta"].max() <= len(o.blas_prims)  # (the view-factor matrix is N x N: rows are metadata - 1)
        assert len(lm.soup(kind, 3, "degen")) > lm.N_VALID[kind]
    assert lm.N_VALID["big"] > 1024  # the refit's cross-window protocol
    v, f, nrm, uv = lm.mesh(5)
    o = oracle.Scene()
    o.add_instance(o.add_mesh(v, f, nrm, uv))
    o.build()
    assert len(o.blas_prims) == len(f) == 2 * lm.MESH_N ** 2 and np.array_equal(lm.mesh(6)[1], f)
