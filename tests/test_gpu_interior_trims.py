"""The interior pass's stack position as an integer address (LaneStackP::addr_t) and its position / next-node selects written from the
children's hit predicates: the position moves by (h0 + h1 - 1) entries and the next node is child 0 when it is first or the only hit, else
child 1 when hit, else the old top.  What can go wrong is one of the four outcomes of an interior step taking another's position change or
next node, and the `top < limit` test of the biased address admitting a lane one entry early or late.  Every batch is classified on the CPU
from the oracle's step records -- all four outcomes, at the top level and inside an instance, and steps that start on the last entry below
the LDS depth -- and the phased kernels, chosen explicitly, are compared with the oracle bit for bit."""
import numpy as np
import pytest

from gpu_kit import rc  # noqa: F401
from helpers import assert_hits_equal, build_oracle, build_product
from scene_kit import BOUNDARY, LDS_STACK, MID_STACK, chain, chain_cfg, corner_rays, max_depth

pytestmark = pytest.mark.gpu

N_RAYS = 4096
SHAPES = ((3, 1), (5, 1), (6, 1), (3, 0), (5, 0), (6, 0))   # (kernel, stack16)


@pytest.fixture(scope="module")
def rays4k(rc):
    rays = corner_rays(rc)[:N_RAYS]
    rays.setflags(write=False)
    return rays


def outcomes(o, rays):
    """Rays that show each outcome of an interior step (rc_oracle.c's step records: kind in the low bits -- 0 a TLAS interior node, 1 a BLAS
    one --, 0x20 pushed the far child, 0x40 popped; the depth AFTER the step in the second array):
      two      both children hit: push the far one, descend          (position + 1)
      one      one child hit and it is the near one: descend         (position unchanged)
      far_only one child hit and it is the far one: push and pop it  (position unchanged, next node = the child just written)
      none     no child hit: pop                                     (position - 1, next node = the old top)
    each for kind 0 and kind 1, and `brink`: interior steps that START with lds - 1 entries (the last position the fast loop admits) and push."""
    names = ("two", "one", "far_only", "none")
    out = {f"{n}{k}": 0 for n in names for k in (0, 1)}
    out.update({f"brink{lds}": 0 for lds in (MID_STACK, LDS_STACK)})
    for r in rays:
        ev, dp = o.trace_events(r, cap=8192)
        assert 0 < len(ev) < 8192
        start = np.concatenate([[1], dp[:-1]]).astype(np.int64)
        for k in (0, 1):
            interior = (ev & 7) == k
            for n, bits in zip(names, (0x20, 0x00, 0x60, 0x40)):
                out[f"{n}{k}"] += bool((interior & ((ev & 0x60) == bits)).any())
        for lds in (MID_STACK, LDS_STACK):
            out[f"brink{lds}"] += bool((((ev & 7) <= 1) & ((ev & 0x60) == 0x20) & (start == lds - 1)).any())
    return out


@pytest.mark.parametrize("depth", (16, 17, 25))
def test_every_outcome_of_an_interior_step(rc, oracle, rays4k, depth):
    n_inst, n_tris = BOUNDARY[depth]
    cfg = chain_cfg(rc, chain(8)[:n_tris], n_inst)
    t, o = build_product(rc, cfg), build_oracle(oracle, cfg)
    assert max_depth(o, rays4k) == depth
    got = outcomes(o, rays4k)
    for k in (0, 1):
        for n in ("two", "one", "none"):
            assert got[f"{n}{k}"] >= 64, (n, k, got)
    assert got["far_only1"] >= 64 or depth != 17, got        # (the existing stack-peek cases find push-and-pop steps at depths 14 and 17)
    assert got[f"brink{MID_STACK}"] >= 64, got               # a push from 15 to 16 entries: the lane leaves the fast loop of kernels 5 and 6
    assert (got[f"brink{LDS_STACK}"] > 0) == (depth == 25), got   # ... and from 23 to 24: kernel 3's
    want, want_any = o.trace(rays4k, nthreads=8), o.trace(rays4k, mode="any", nthreads=8)
    assert want["hit"].mean() > 0.01
    for k, s16 in SHAPES:
        t.set_option("kernel", k); t.set_option("stack16", s16)
        assert_hits_equal(t.trace(rays4k), want, f"depth {depth} k{k} stack16 {s16}")
        assert_hits_equal(t.trace(rays4k, mode="any"), want_any, f"depth {depth} any k{k} stack16 {s16}")
