"""The close-repeat rule of cost-ordered claiming on top of tests/order_model.py (test infrastructure).

order_select (raycore.jl_amd/csrc/rc_traverse_core.h) knows a third outcome besides "repeat" and "not a repeat": the CLOSE REPEAT, a launch whose
64 sample origins equal the matched slot's and whose direction term (the mean over the samples of |dd|^2 / |d|^2) lies below RcClaim::close_dir_max --
a still camera that re-renders its view through other points of the same pixels.  A close repeat continues the slot's history exactly as a repeat
does: not fresh, the slot's launch count goes on, it claims through the slot's order when there is one, records in the slot's launches 2-4 and then at
the host's cadence, and ends the run of non-repeats (so it never leads to a pause).  The slot's samples follow the launch, as they always do.

`History.launch(batch, near, close=False)`: `close` says that the slot matched through `near` holds a batch this launch is a close repeat of (it has
no meaning for an exact repeat or an unmatched launch).  With close=False everywhere this class is order_model.History, transition for transition
(tests/test_close_repeat_model.py); the device is compared with it word for word in tests/test_gpu_close_repeats.py.  The model adds one word to
order_model's: "close" (header word 6: the latest launch was a close repeat).
"""
import numpy as np

import order_model as om

CLOSE = 6                      # kHistClose
CLOSE_DIR_MAX = np.float32(6e-6)   # kCloseDirMax (rc_traverse.hip)
MATCH_MAX = np.float32(0.02)       # order_select: a slot further than this is no match at all


class History(om.History):
    def __init__(self, mut=None, close_repeats=True):
        super().__init__(mut)
        self.close_repeats = close_repeats   # option "order_close_repeats"
        self.last = dict(self.last, close=0)

    def launch(self, batch, near=(), close=False):
        # ---- host: rc_cost_order_setup, unchanged by the close rule ----
        self.host_gen += 1
        paused = self.host_skip > 1
        if self.host_streak > 0:
            self.credit = om.CREDIT_AFTER_NON_REPEAT
        if paused:
            self.credit = 0
        if self.host_gen >= 2 and not paused and (self.host_gen <= om.EARLY_LAUNCHES or self.credit > 0 or (self.m.rebuild_on_pending_word and self.host_pending)):
            self.rebuilds += 1
            for k in range(om.K_SLOTS):
                if self.pending[k]:
                    self.pending[k], self.has_order[k] = 0, 1
            self.host_pending = 0
        if self.credit > 0:
            self.credit -= 1
        want_record = 0
        if self.host_gen >= self.next_record and not paused:
            want_record = 1
            self.next_record = self.host_gen + 7 + self.records_asked % 3
            self.records_asked += 1
            self.credit = max(self.credit, 1)
        # ---- device: a launch inside a pause does not look at its rays ----
        if self.skip_left > 0:
            self.skip_left -= 1
            self.host_skip = self.skip_left
            self.last = dict(self.last, skip_left=self.skip_left, pending=list(self.pending), has_order=list(self.has_order))
            return self.last
        # ---- device: order_select ----
        best, exact = None, False
        for k in range(om.K_SLOTS):
            if self.stamp[k] == 0:
                continue
            if self.batch[k] == batch:
                best, exact = k, True
                break
            if best is None and self.batch[k] in near:
                best = k
        is_close = bool(close) and self.close_repeats and best is not None and not exact
        continues = exact or is_close              # a repeat or a close repeat goes on with the slot's history
        fresh = (not continues) if self.m.only_repeats_continue else best is None
        sel = best if best is not None else min(range(om.K_SLOTS), key=lambda k: (self.stamp[k], k))
        gen = 1 if fresh else self.gen[sel] + 1
        record = (self.m.record_first <= gen <= self.m.record_last) or (want_record and gen >= 5)
        valid = (not fresh) and self.has_order[sel] != 0
        # ---- device: order_commit ----
        self.batch[sel] = batch
        self.clock += 1
        self.stamp[sel] = self.clock
        self.gen[sel] = gen
        if fresh:
            self.pending[sel] = 0
            self.has_order[sel] = 0
        if record:
            self.pending[sel] = 1
        not_counted = continues if self.m.repeats_only else best is not None
        self.streak = 0 if not_counted else self.streak + 1
        if self.streak >= self.m.give_up_after:
            self.streak, self.skip_left = 0, om.GIVE_UP_FOR
        self.host_streak = self.streak
        self.host_pending = int(any(self.pending))
        self.host_skip = self.skip_left
        self.last = {"sel": sel, "order_valid": int(valid), "records": int(record), "clock": self.clock, "fresh": int(fresh),
                     "stamp": list(self.stamp), "gen": list(self.gen), "pending": list(self.pending), "has_order": list(self.has_order), "streak": self.streak,
                     "skip_left": self.skip_left, "close": int(is_close)}
        return self.last


def device_words(w):
    """order_model.device_words plus the close-repeat word"""
    return dict(om.device_words(w), close=int(w[CLOSE]))


def sample_indices(n):
    """the 64 rays of an n-ray batch that order_select looks at"""
    lane = np.arange(64, dtype=np.uint64)
    return np.minimum(lane * np.uint64(n) // np.uint64(64) + np.uint64(n) // np.uint64(128), np.uint64(n - 1)).astype(np.int64)


def select_terms(rays, prev, inv_l2):
    """order_select's distance between a launch (`rays`) and a slot that remembers `prev` (structured ray arrays of one length), restated in float32
    operation for operation: (distance, every sample origin equal).  The 64 per-sample terms are summed by the butterfly the 64 lanes run
    (d += shfl_xor(d, m) for m = 32, 16, ..., 1), then scaled by 1/64."""
    f = np.float32
    idx = sample_indices(len(rays))
    o, d, po, pd = (np.ascontiguousarray(a[idx], dtype=f) for a in (rays["o"], rays["d"], prev["o"], prev["d"]))
    ox, oy, oz = (o[:, k] - po[:, k] for k in range(3))
    dx, dy, dz = (d[:, k] - pd[:, k] for k in range(3))
    na = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    nb = pd[:, 0] * pd[:, 0] + pd[:, 1] * pd[:, 1] + pd[:, 2] * pd[:, 2]
    t = (dx * dx + dy * dy + dz * dz) / np.maximum(np.maximum(na, nb), f(1e-30)) + (ox * ox + oy * oy + oz * oz) * f(inv_l2)
    assert t.dtype == f
    m = 32
    while m > 0:
        t = t + t[np.arange(64) ^ m]
        m >>= 1
    dist = t[0] * f(1.0 / 64)
    same_o = not bool(np.any((ox != 0) | (oy != 0) | (oz != 0)))
    return dist, same_o


def classify(rays, prev, inv_l2, bound=CLOSE_DIR_MAX):
    """what order_select makes of `rays` against a slot holding `prev`: "exact", "close", "near" (matched, starts over in the slot) or "far" """
    dist, same_o = select_terms(rays, prev, inv_l2)
    if not dist < MATCH_MAX:
        return "far"
    if dist == 0:
        return "exact"
    return "close" if same_o and dist < np.float32(bound) else "near"
