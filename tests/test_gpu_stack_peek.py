"""The interior pass's pop without its read: the phased kernels (3, 5, 6 and the driver shells) read the OLD stack top together with the
node (LaneStackP::peek_lds) and select between it and the far child they have just written, instead of reading the slot back behind the
slab test.  What can go wrong is WHICH value a pop returns: the far child pushed in the same pass, the bottom entry, the sentinel of an
instance entry, the entry a general push / pop of the deep pass left on top.  The rays of every case are classified on the CPU from the
oracle's step records, the classes are asserted there, and the kernels -- chosen explicitly, so that small batches reach them -- are
compared with the oracle bit for bit, closest and any, 16- and 32-bit stack entries."""
import numpy as np
import pytest

from gpu_kit import rc  # noqa: F401
from helpers import assert_hits_equal, build_oracle, build_product
from scene_kit import BOUNDARY, GRID, LDS_STACK, MID_STACK, VIEWDIR, chain, chain_cfg, corner_rays, max_depth

pytestmark = pytest.mark.gpu

N_RAYS = 4096
SHAPES = ((3, 1), (5, 1), (6, 1), (3, 0), (5, 0), (6, 0))   # (kernel, stack16)


@pytest.fixture(scope="module")
def rays4k(rc):
    rays = corner_rays(rc)[:N_RAYS]   # (the first rays of the boundary test's batch: its deepest rays are among them)
    rays.setflags(write=False)
    return rays


def classify(o, rays):
    """Per class the number of `rays` that show it, from the oracle's step records (rc_oracle.c: kind in the low bits, 0x20 pushed the far
    child, 0x40 popped, 0x80 that pop returned to the top level; depth AFTER the step in the second array):
      push_pop   an interior step that pushes its far child and pops it again (h0 && !h1 && !first0)
      bottom     the ray's last step is an interior step whose pop takes the bottom entry: the lane finishes on INVALID
      root_miss  both children miss at a BLAS root: the step after an instance entry pops the sentinel
      cross16/24 an interior step that starts at or beyond that LDS depth (the deep pass serves it with the general push / pop) and a later
                 interior step below it (the fast loop again: its peek reads what the general forms left)
      deepest    the deepest stack at the start of a step"""
    out = dict(push_pop=0, bottom=0, root_miss=0, cross16=0, cross24=0, deepest=1)
    for r in rays:
        ev, dp = o.trace_events(r, cap=8192)
        assert 0 < len(ev) < 8192
        interior = (ev & 7) <= 1
        start = np.concatenate([[1], dp[:-1]]).astype(np.int64)   # depth at the start of each step (the initial INVALID entry included)
        out["push_pop"] += bool((interior & ((ev & 0x60) == 0x60)).any())
        out["bottom"] += bool(interior[-1] and (ev[-1] & 0xC0) == 0x40 and dp[-1] == 0)
        out["root_miss"] += bool(((ev[1:] == 0xC1) & (ev[:-1] == 2)).any())
        for lds in (MID_STACK, LDS_STACK):
            deep = np.nonzero(interior & (start >= lds))[0]
            out[f"cross{lds}"] += bool(len(deep) and (interior[deep[0]:] & (start[deep[0]:] < lds)).any())
        out["deepest"] = max(out["deepest"], int(start.max()))
    return out


def compare_shapes(t, rays, want, want_any, what, shapes=SHAPES):
    """t.trace raises on a set status word (RC_ERR_STACK_OVERFLOW), so passing also means the status word stayed 0."""
    for k, s16 in shapes:
        t.set_option("kernel", k); t.set_option("stack16", s16)
        assert_hits_equal(t.trace(rays), want, f"{what} k{k} stack16 {s16}")
        assert_hits_equal(t.trace(rays, mode="any"), want_any, f"{what} any k{k} stack16 {s16}")
    t.set_option("kernel", -1); t.set_option("stack16", 1)


# Maximum stack depth 14 ... 18 around the 16 entries kernels 5 and 6 keep in LDS, and 25 for kernel 3's 24.
DEPTHS = (14, 15, 16, 17, 18, 25)
# what the CPU classification of the 4 096 corner rays must find in each scene (chosen with the oracle; asserted below)
PUSH_POP_DEPTHS, CROSS16_DEPTHS, CROSS24_DEPTHS = (14, 17), (17, 18, 25), (25,)


@pytest.mark.parametrize("depth", DEPTHS)
def test_pops_of_every_kind_around_the_lds_depth(rc, oracle, rays4k, depth):
    """One batch per depth: rays that finish on the bottom entry (b), rays that miss both children of a BLAS root and pop the sentinel
    (c), at depths 14 and 17 rays that pop the far child they push in the same pass (a), and -- from depth 17 on -- lanes that leave the
    fast loop for the deep pass and come back, so that a peek follows a general push / pop (d)."""
    n_inst, n_tris = BOUNDARY[depth]
    cfg = chain_cfg(rc, chain(8)[:n_tris], n_inst)
    t, o = build_product(rc, cfg), build_oracle(oracle, cfg)
    cls = classify(o, rays4k)
    assert cls["deepest"] == depth == max_depth(o, rays4k)
    assert cls["bottom"] >= 64 and cls["root_miss"] >= 64
    assert (cls["push_pop"] >= 64) == (depth in PUSH_POP_DEPTHS)
    assert (cls["cross16"] >= 64) == (depth in CROSS16_DEPTHS) and (cls["cross16"] == 0) == (depth not in CROSS16_DEPTHS)
    assert (cls["cross24"] > 0) == (depth in CROSS24_DEPTHS)
    want, want_any = o.trace(rays4k, nthreads=8), o.trace(rays4k, mode="any", nthreads=8)
    assert want["hit"].mean() > 0.01
    compare_shapes(t, rays4k, want, want_any, f"depth {depth}")


def test_deep_and_shallow_lanes_interleaved(rc, oracle, rays4k):
    """(e) Deep rays 1 : 3 with shallow ones -- rays that miss everything and rays that hit the first instance only -- so that in every
    wave some lanes sit in the deep pass while the others keep peeking in the fast loop."""
    cfg = chain_cfg(rc, chain(10))
    t, o = build_product(rc, cfg), build_oracle(oracle, cfg)
    sc = rc.scenes
    g = sc.rng(31)
    n_deep = N_RAYS           # 16 384 rays in all
    deep = rays4k
    n_sh = n_deep + n_deep // 2
    target = np.stack([g.uniform(0.8, 0.95, 4 * n_deep), g.uniform(0.25, 0.3, 4 * n_deep), g.uniform(0.25, 0.3, 4 * n_deep)], axis=1)
    org = target + np.array([0.0, 0.4, 0.4]) + g.uniform(-0.02, 0.02, size=target.shape)
    cand = sc.make_rays(org, sc.normalize(target - org))
    hc = o.trace(cand, nthreads=8)
    first = cand[(hc["hit"] == 1) & (hc["instance_id"] == 0)][:n_sh]
    assert len(first) == n_sh
    away = sc.make_rays(g.uniform(2.0, 3.0, size=(n_sh, 3)), sc.normalize(g.uniform(0.05, 1.0, size=(n_sh, 3))))
    shallow = np.empty(3 * n_deep, dtype=deep.dtype)
    shallow[0::2], shallow[1::2] = first, away
    rays = np.empty(4 * n_deep, dtype=deep.dtype)
    rays[0::4] = deep
    rays[1::4], rays[2::4], rays[3::4] = shallow[0::3], shallow[1::3], shallow[2::3]
    cd, cs = classify(o, deep), classify(o, shallow[:768])
    assert cd["deepest"] > LDS_STACK + 2 and cd["cross16"] >= 64 and cd["cross24"] >= 8
    assert cs["deepest"] <= MID_STACK - 4 and cs["bottom"] >= 256
    want, want_any = o.trace(rays, nthreads=8), o.trace(rays, mode="any", nthreads=8)
    assert not want["hit"][(np.arange(len(rays)) % 4 != 0) & (rays["o"][:, 0] >= 2.0)].any()   # the rays that start beyond the scene miss
    compare_shapes(t, rays, want, want_any, "mixed waves")


def test_default_dispatch_768x768(rc, oracle):
    """One batch large enough for the default dispatch to pick the persistent kernels by itself: 768 x 768 jittered primaries of the
    headline scene."""
    sc = rc.scenes
    cfg = sc.config_c3()
    t, o = build_product(rc, cfg), build_oracle(oracle, cfg)
    rays = sc.c3_primary_rays(cfg, 768, 768, jitter_seed=7)
    want, want_any = o.trace(rays, nthreads=8), o.trace(rays, mode="any", nthreads=8)
    assert 0.2 < want["hit"].mean() < 0.8
    compare_shapes(t, rays, want, want_any, "768 x 768", shapes=((-1, 1), (-1, 0)))


@pytest.mark.parametrize("shell", ["lds", "plain", "partial"])
def test_get_illumination_through_the_driver_shells(rc, oracle, shell):
    """The three driver shells on the deep scene, against the oracle's counts (closest-hit illumination peeks in the LDS shell and keeps
    the late pop in the plain and the partial-LDS shell, which would spill the peeked value)."""
    cfg = chain_cfg(rc, chain(10), fillers=300 if shell == "partial" else 0)
    t, o = build_product(rc, cfg), build_oracle(oracle, cfg)
    L = oracle.lib()
    L.rco_max_stack(1)
    want = o.get_illumination(VIEWDIR, GRID, nthreads=8)
    assert L.rco_max_stack(1) > LDS_STACK + 2 and want.sum() > 500
    if shell == "plain":
        t.set_option("kernel", 3)
    got = rc.get_illumination(t, VIEWDIR, GRID)
    assert np.array_equal(got, want), f"get_illumination, {shell} shell"
