"""CPU: the close-repeat rule of cost-ordered claiming -- its Python restatement (tests/close_repeat_model.py) against order_model.History where
the rule does not apply, the restatement's own promises, and the bound itself against order_select's float32 arithmetic on real camera rays."""
import numpy as np
import pytest

import close_repeat_model as cm
import order_model as om


def jittered(n, first=0):
    """n jitter seeds of one camera: every launch is near its predecessor and a close repeat of it"""
    return [(("j", first + k), ((("j", first + k - 1),) if k else ()), k > 0) for k in range(n)]


def run(script, **kw):
    h = cm.History(**kw)
    return [h.launch(*step) for step in script], h


@pytest.mark.parametrize("name", list(om.scripts()))
def test_without_close_launches_the_model_is_order_model(name):
    a, b = om.History(), cm.History()
    for k, (batch, near) in enumerate(om.scripts()[name]):
        want, got = a.launch(batch, near), b.launch(batch, near, close=False)
        assert got["close"] == 0 and {f: got[f] for f in want} == want, f"{name}: launch {k + 1}"
    assert a.rebuilds == b.rebuilds
    # ... and with the option off a `close` launch is an ordinary near match
    a, b = om.History(), cm.History(close_repeats=False)
    for batch, near, close in jittered(80):
        want, got = a.launch(batch, near), b.launch(batch, near, close)
        assert {f: got[f] for f in want} == want and got["close"] == 0


def test_a_jittered_run_never_pauses_has_an_order_from_its_third_launch_and_records_like_a_repeating_batch():
    tr, h = run(jittered(80))
    assert all(t["skip_left"] == 0 for t in tr) and tr[0]["streak"] == 1 and all(t["streak"] == 0 for t in tr[1:])
    assert tr[0]["fresh"] == 1 and tr[0]["close"] == 0 and all(t["fresh"] == 0 and t["close"] == 1 for t in tr[1:])
    assert len({t["sel"] for t in tr}) == 1 and [t["gen"][t["sel"]] for t in tr] == list(range(1, 81))
    assert [t["order_valid"] for t in tr[:4]] == [0, 0, 1, 1] and all(t["order_valid"] for t in tr[2:])
    # exactly the recording launches of a batch that repeats bit for bit (tests/test_order_model.py): 2-4, then the host's cadence
    rep = om.History()
    same = [rep.launch(0) for _ in range(80)]
    assert [i + 1 for i, t in enumerate(tr) if t["records"]] == [i + 1 for i, t in enumerate(same) if t["records"]]
    assert [i + 1 for i, t in enumerate(tr) if t["records"]][:8] == [2, 3, 4, 8, 15, 23, 32, 39]
    assert h.rebuilds == rep.rebuilds


def test_only_the_close_match_continues_a_slot():
    # a camera that translates (near, never close) between two jittered stretches: every moving frame starts over, and the jitter about where it
    # stopped goes on from the last moving frame -- that frame is the slot's launch 1
    moving = [(("m", f), ((("m", f - 1),) if f > 1 else (("j", 3),)), False) for f in range(1, 7)]
    after = [(("k", 0), (("m", 6),), True)] + [(("k", k), (("k", k - 1),), True) for k in range(1, 5)]
    tr, _ = run(jittered(4) + moving + after)
    assert all(t["fresh"] == 1 and t["close"] == 0 and t["records"] == 0 and t["order_valid"] == 0 for t in tr[4:10])
    assert [t["streak"] for t in tr[4:10]] == [1, 2, 3, 4, 5, 6] and all(t["skip_left"] == 0 for t in tr)
    assert [t["gen"][t["sel"]] for t in tr[10:]] == [2, 3, 4, 5, 6] and [t["records"] for t in tr[10:]] == [1, 1, 1, 0, 1]   # (the slot's launches 2-4; the shape's launch 15 is one the host's cadence asks to record)
    assert [t["order_valid"] for t in tr[10:]] == [0, 1, 1, 1, 1] and all(t["close"] == 1 and t["streak"] == 0 for t in tr[10:])
    # an exact repeat is never reported as close, whatever the caller says
    tr, _ = run([(0, (), True)] * 3)
    assert [t["close"] for t in tr] == [0, 0, 0] and [t["fresh"] for t in tr] == [1, 0, 0]


# ---- the bound: order_select's arithmetic on the cameras the rule is for and the ones it must leave alone ----

def rotated_in_place(eye, look_at, degrees):
    """the look-at point of the camera turned about its own position (about the y axis)"""
    a = np.radians(degrees)
    v = np.asarray(look_at, dtype=np.float64) - eye
    return eye + np.array([np.cos(a) * v[0] + np.sin(a) * v[2], v[1], -np.sin(a) * v[0] + np.cos(a) * v[2]])


@pytest.fixture(scope="module")
def camera(oracle):
    import raycore_jl_amd as rc
    from helpers import build_oracle
    sc = rc.scenes
    cfg = sc.config_c3(lattice=(4, 4, 2))
    lo_hi = np.asarray(build_oracle(oracle, cfg).world_bound, dtype=np.float64).reshape(2, 3)
    e = (lo_hi[1] - lo_hi[0]).astype(np.float32)
    inv_l2 = np.float32(1.0) / (e[0] * e[0] + e[1] * e[1] + e[2] * e[2])
    centre = cfg["lattice_centre"]
    return sc, centre + np.array([0.0, 0.0, -13.0]), centre, inv_l2


@pytest.mark.parametrize("res", [(256, 256), (1280, 800), (2048, 2048)])
def test_the_bound_admits_jitter_and_rejects_a_turned_or_translated_camera(camera, res):
    sc, eye, centre, inv_l2 = camera
    w, h = res
    a, b = (sc.pinhole_rays(w, h, eye, centre, 45.0, jitter_seed=s) for s in (1, 2))
    centred = sc.pinhole_rays(w, h, eye, centre, 45.0)
    for what, x, y in (("jitter against jitter", a, b), ("jitter against pixel centres", a, centred), ("pixel centres against jitter", centred, b)):
        dist, same_o = cm.select_terms(x, y, inv_l2)
        print(f"{w} x {h} {what}: direction term {dist:.3e}")
        assert same_o and 0 < dist < cm.CLOSE_DIR_MAX and cm.classify(x, y, inv_l2) == "close", (what, dist)
    assert cm.classify(a, a.copy(), inv_l2) == "exact"
    turned = sc.pinhole_rays(w, h, eye, rotated_in_place(eye, centre, 5.0), 45.0, jitter_seed=3)
    dist, same_o = cm.select_terms(turned, a, inv_l2)
    print(f"{w} x {h} turned in place by 5 degrees: direction term {dist:.3e}")
    assert same_o and cm.CLOSE_DIR_MAX * 100 < dist < cm.MATCH_MAX and cm.classify(turned, a, inv_l2) == "near", dist
    moved = sc.pinhole_rays(w, h, eye + np.array([0.02, 0.01, 0.0]), centre, 45.0)
    dist, same_o = cm.select_terms(moved, centred, inv_l2)
    print(f"{w} x {h} translated by (0.02, 0.01, 0): distance {dist:.3e}")
    assert not same_o and cm.classify(moved, centred, inv_l2) == "near", dist   # matched, and kept out by the ORIGIN rule however small the distance
    assert cm.classify(turned, a, inv_l2, bound=0.0) == "near" and cm.classify(a, b, inv_l2, bound=0.0) == "near"   # bound 0: the rule is off
