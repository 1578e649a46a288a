"""GPU: close repeats of cost-ordered claiming -- jittered re-renders of one view continue their batch slot's history (order_select / order_commit,
raycore.jl_amd/csrc/rc_traverse_core.h; option "order_close_repeats").  The device's header words are held against tests/close_repeat_model.py after
every launch, and every launch's hits against the oracle's: the claim order never changes a result.

The mechanism engages only when a launch has at least a claim per wave, so the shape is the one tests/test_gpu_order_model.py uses: the (4, 4, 2)
lattice at 1280 x 800 (1 024 000 rays, 8 000 chunks)."""
import ctypes

import numpy as np
import pytest

import close_repeat_model as cm
from gpu_kit import rc  # noqa: F401
from helpers import assert_hits_equal, build_oracle, build_product

pytestmark = pytest.mark.gpu

W, H = 1280, 800
STEP = np.array([0.02, 0.01, 0.0])       # the translating camera's travel per frame


def turned_in_place(eye, look_at, degrees):
    a = np.radians(degrees)
    v = look_at - eye
    return eye + np.array([np.cos(a) * v[0] + np.sin(a) * v[2], v[1], -np.sin(a) * v[0] + np.cos(a) * v[2]])


class Rig:
    """the scene, its oracle, and the batches by name -- ("j", seed): jitter seed `seed` of the home camera; ("m", f): frame f of the camera
    translating away from home (pixel centres); ("s", seed): jitter about where that camera stopped after six frames; ("t", seed): the home
    camera turned in place by 5 degrees, jittered.  Rays and oracle hits are computed once per batch and shared by the tests."""

    def __init__(self, rc, oracle_mod):
        import torch
        self.rc, self.torch, self.sc = rc, torch, rc.scenes
        self.cfg = self.sc.config_c3(lattice=(4, 4, 2))
        self.o = build_oracle(oracle_mod, self.cfg)
        self.centre = self.cfg["lattice_centre"]
        self.home = self.centre + np.array([0.0, 0.0, -13.0])
        self.cache = {}
        self.hip = ctypes.CDLL("libamdhip64.so")

    def rays(self, batch):
        if batch not in self.cache:
            kind, k = batch
            eye, at, seed = self.home, self.centre, k
            if kind == "m":
                eye, seed = self.home + k * STEP, None
            elif kind == "s":
                eye = self.home + 6 * STEP
            elif kind == "t":
                at = turned_in_place(self.home, self.centre, 5.0)
            r = self.sc.pinhole_rays(W, H, eye, at, 45.0, jitter_seed=seed)
            self.cache[batch] = (self.torch.from_numpy(r.view(np.uint8).reshape(-1)).cuda(), self.o.trace(r, nthreads=16), len(r))
        return self.cache[batch]

    def header(self, t):
        h = self.torch.empty(48, dtype=self.torch.int32, device="cuda")
        self.hip.hipMemcpy(ctypes.c_void_p(h.data_ptr()), ctypes.c_void_p(t.get_option("debug_ctl_ptr")), ctypes.c_size_t(192), 3)
        self.torch.cuda.synchronize()
        return cm.device_words(h.cpu().numpy().view(np.uint32))

    def order(self, t):
        n = t.get_option("debug_order_n")
        o = self.torch.empty(n, dtype=self.torch.int32, device="cuda")
        self.hip.hipMemcpy(ctypes.c_void_p(o.data_ptr()), ctypes.c_void_p(t.get_option("debug_order_ptr")), ctypes.c_size_t(4 * n), 3)
        self.torch.cuda.synchronize()
        return o.cpu().numpy()


@pytest.fixture(scope="module")
def rig(rc, oracle):
    return Rig(rc, oracle)


def jitter_script(kind, n, after=None):
    """n jitter seeds of one camera, each a close repeat of its predecessor; `after`: the batch the first one follows (near it, close or not)"""
    out = []
    for k in range(n):
        if k:
            out.append(((kind, k), ((kind, k - 1),), True))
        else:
            out.append(((kind, 0), (after[0],), after[1]) if after else ((kind, 0), (), False))
    return out


def follow(rig, t, model, script, name):
    """every launch of the script: hits against the oracle, header words against the model; returns the model's words per launch"""
    torch = rig.torch
    trace = []
    for k, (batch, near, close) in enumerate(script):
        d, want, n = rig.rays(batch)
        out = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        t.trace_device(d.data_ptr(), out.data_ptr(), n)
        torch.cuda.synchronize()
        assert_hits_equal(out.cpu().numpy().view(rig.rc.HIT_DT), want, f"{name}: launch {k + 1}")
        expect = model.launch(batch, near, close)
        got = rig.header(t)
        assert got == expect, f"{name}: launch {k + 1}\n device {got}\n model  {expect}"
        trace.append(expect)
    assert t.get_option("claim_drift") == 0
    return trace


def test_twelve_jitter_seeds_of_one_camera_continue_one_history(rig):
    """(a) and (f): launch 1 is fresh, every later one a close repeat in the same slot; recordings at 2-4 and 8, an order from launch 3 on, no
    pause -- and the order the device built is a permutation of the chunks that is not the identity"""
    t = build_product(rig.rc, rig.cfg)
    assert t.get_option("order_close_repeats") == 1
    tr = follow(rig, t, cm.History(), jitter_script("j", 12), "jitter x 12")
    assert [x["close"] for x in tr] == [0] + [1] * 11 and [x["fresh"] for x in tr] == [1] + [0] * 11 and all(x["skip_left"] == 0 for x in tr)
    assert [i + 1 for i, x in enumerate(tr) if x["records"]] == [2, 3, 4, 8] and [x["order_valid"] for x in tr] == [0, 0] + [1] * 10
    order = rig.order(t)
    n_chunks = -(-W * H // 128)
    assert len(order) == n_chunks and np.array_equal(np.sort(order), np.arange(n_chunks)) and not np.array_equal(order, np.arange(n_chunks))
    t.free()


def test_a_translating_camera_stays_fresh_and_jitter_where_it_stops_continues_from_there(rig):
    """(b): four jittered launches, six frames of the translating camera (each starts over, as before), then jitter about where it stopped --
    close repeats of the last moving frame, which is their slot's launch 1"""
    moving = [(("m", f), ((("m", f - 1) if f > 1 else ("j", 3)),), False) for f in range(1, 7)]
    script = jitter_script("j", 4) + moving + jitter_script("s", 4, after=(("m", 6), True))
    t = build_product(rig.rc, rig.cfg)
    tr = follow(rig, t, cm.History(), script, "jitter, translate, jitter")
    assert all(x["fresh"] == 1 and x["close"] == 0 and x["records"] == 0 for x in tr[4:10]) and [x["streak"] for x in tr[4:10]] == [1, 2, 3, 4, 5, 6]
    assert [x["gen"][x["sel"]] for x in tr[10:]] == [2, 3, 4, 5] and all(x["close"] == 1 for x in tr[10:]) and [x["order_valid"] for x in tr[10:]] == [0, 1, 1, 1]
    t.free()


def test_a_camera_turned_by_degrees_starts_over_both_ways(rig):
    """(c): jitter, the camera turned in place by 5 degrees (same origin, direction term 7e-3: matched, far above the bound -> fresh), turned back
    with jitter (fresh again), then close repeats"""
    script = jitter_script("j", 3) + [(("t", 7), (("j", 2),), False), (("j", 8), (("t", 7),), False), (("j", 9), (("j", 8),), True), (("j", 10), (("j", 9),), True)]
    t = build_product(rig.rc, rig.cfg)
    tr = follow(rig, t, cm.History(), script, "jitter, turned, back")
    assert [x["fresh"] for x in tr] == [1, 0, 0, 1, 1, 0, 0] and [x["close"] for x in tr] == [0, 1, 1, 0, 0, 1, 1] and len({x["sel"] for x in tr}) == 1
    t.free()


def test_with_the_option_off_every_jittered_launch_is_fresh_and_the_shape_pauses(rig):
    """(d): order_close_repeats = 0 -- the behaviour before the rule: all fresh, the pause starts with the eighth launch"""
    t = build_product(rig.rc, rig.cfg)
    t.set_option("order_close_repeats", 0)
    assert t.get_option("order_close_repeats") == 0
    tr = follow(rig, t, cm.History(close_repeats=False), jitter_script("j", 12), "jitter x 12, option off")
    assert all(x["fresh"] == 1 and x["close"] == 0 and x["records"] == 0 and x["order_valid"] == 0 for x in tr)
    assert [x["streak"] for x in tr[:8]] == [1, 2, 3, 4, 5, 6, 7, 0] and [x["skip_left"] for x in tr[7:]] == [64, 63, 62, 61, 60]
    t.free()


def test_jittered_launches_enqueued_without_waiting_get_their_order(rig):
    """(e): the twelve launches of (a) and not one synchronisation in between: the host decides about the rebuild kernels from words it reads
    late, and the recordings of launches 2-4 must still have become the order the last launch claims through"""
    torch = rig.torch
    t = build_product(rig.rc, rig.cfg)
    bufs = [rig.rays(("j", k)) for k in range(12)]
    n = bufs[0][2]
    out = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for d, _, _ in bufs:
        t.trace_device(d.data_ptr(), out.data_ptr(), n)
    torch.cuda.synchronize()
    h = rig.header(t)
    assert h["order_valid"] == 1 and h["close"] == 1 and h["fresh"] == 0 and h["skip_left"] == 0 and h["gen"][h["sel"]] == 12 and h["has_order"][h["sel"]] == 1, h
    assert_hits_equal(out.cpu().numpy().view(rig.rc.HIT_DT), bufs[-1][1], "the last of twelve launches enqueued without waiting")
    assert t.get_option("claim_drift") == 0
    t.free()
