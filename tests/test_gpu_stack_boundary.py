"""The lane stack at the LDS depth.  The phased kernels (3, 5, 6 and the driver shells) keep the first 16 or 24 entries of every lane's
traversal stack in LDS and spill the rest; their interior loop serves only lanes below that depth, with branch-free push / pop, and
hands the others to a pass of their own.  tests/test_gpu_parity.py::test_deep_trees_use_the_stack_spill_path runs far beyond the depth;
here the stack stops AT it (last LDS slot written, first spilled entry, a pop that crosses back), deep and shallow rays share a wave, and
one ray pushes and pops in the same pass.  Everything is compared with the oracle bit for bit."""
import numpy as np
import pytest

from gpu_kit import rc  # noqa: F401
from helpers import assert_hits_equal, build_oracle, build_product
from scene_kit import BOUNDARY, GRID, LDS_STACK, MID_STACK, VIEWDIR, chain, chain_cfg, corner_rays, max_depth

pytestmark = pytest.mark.gpu


KERNELS = ((-1, 1), (3, 1), (5, 1), (6, 1), (-1, 0), (3, 0), (5, 0), (6, 0))   # (kernel, stack16)


def product_max_depth(t, rays, want):
    t.set_option("kernel", 1); t.set_option("stats", 1)
    assert_hits_equal(t.trace(rays), want, "k1 stats")
    depth = t.get_option("stat2")
    t.set_option("stats", 0)
    return depth


def compare_all_kernels(t, rays, want, want_any, what):
    """Every phased shape, 16- and 32-bit stack entries, closest and any.  t.trace raises on a set status word (RC_ERR_STACK_OVERFLOW), so
    passing also means the status word stayed 0."""
    for k, s16 in KERNELS:
        t.set_option("kernel", k); t.set_option("stack16", s16)
        assert_hits_equal(t.trace(rays), want, f"{what} k{k} stack16 {s16}")
        assert_hits_equal(t.trace(rays, mode="any"), want_any, f"{what} any k{k} stack16 {s16}")
    t.set_option("kernel", -1); t.set_option("stack16", 1)


assert sorted(BOUNDARY) == [d + k for d in (MID_STACK, LDS_STACK) for k in (-2, -1, 0, 1, 2)]


@pytest.fixture(scope="module")
def rays20k(rc):
    rays = corner_rays(rc)
    rays.setflags(write=False)
    return rays


@pytest.mark.parametrize("depth", sorted(BOUNDARY))
def test_stack_depth_at_the_lds_boundary(rc, oracle, rays20k, depth):
    """Maximum stack depth = LDS depth - 2 ... + 2 for both LDS depths: at depth 16 (24) the fast form writes the last LDS slot, at 17
    (25) the first entry spills and the pop after it crosses back into LDS."""
    n_inst, n_tris = BOUNDARY[depth]
    cfg = chain_cfg(rc, chain(8)[:n_tris], n_inst)
    t, o = build_product(rc, cfg), build_oracle(oracle, cfg)
    want, want_any = o.trace(rays20k, nthreads=8), o.trace(rays20k, mode="any", nthreads=8)
    assert want["hit"].mean() > 0.01
    assert max_depth(o, rays20k[:4000]) == depth          # (the deepest rays are among the first 4000)
    assert product_max_depth(t, rays20k, want) == depth
    compare_all_kernels(t, rays20k, want, want_any, f"depth {depth}")


def test_deep_and_shallow_rays_share_a_wave(rc, oracle, rays20k):
    """The deep scene with its rays interleaved 1 : 3 with shallow ones -- rays that miss everything and rays that hit the first
    instance only.  Consecutive rays share a wave, so within a wave some lanes are at or beyond the LDS depth while the others are not,
    the deep pass runs beside the fast loop, and one ray's stack is handled by both forms in turn."""
    cfg = chain_cfg(rc, chain(10))
    t, o = build_product(rc, cfg), build_oracle(oracle, cfg)
    sc = rc.scenes
    g = sc.rng(31)
    n_deep = 5000
    deep = rays20k[:n_deep]
    # candidates for "first instance only": aimed at the level-1 triangles' far ends, which only the unscaled instances reach
    target = np.stack([g.uniform(0.8, 0.95, 4 * n_deep), g.uniform(0.25, 0.3, 4 * n_deep), g.uniform(0.25, 0.3, 4 * n_deep)], axis=1)
    org = target + np.array([0.0, 0.4, 0.4]) + g.uniform(-0.02, 0.02, size=target.shape)
    cand = sc.make_rays(org, sc.normalize(target - org))
    hc = o.trace(cand, nthreads=8)
    first = cand[(hc["hit"] == 1) & (hc["instance_id"] == 0)][:n_deep + n_deep // 2]
    assert len(first) == n_deep + n_deep // 2
    away = sc.make_rays(g.uniform(2.0, 3.0, size=(n_deep + n_deep // 2, 3)), sc.normalize(g.uniform(0.05, 1.0, size=(n_deep + n_deep // 2, 3))))
    shallow = np.empty(3 * n_deep, dtype=deep.dtype)
    shallow[0::2], shallow[1::2] = first, away
    rays = np.empty(4 * n_deep, dtype=deep.dtype)
    rays[0::4] = deep
    rays[1::4], rays[2::4], rays[3::4] = shallow[0::3], shallow[1::3], shallow[2::3]
    want, want_any = o.trace(rays, nthreads=8), o.trace(rays, mode="any", nthreads=8)
    assert not want["hit"][np.isin(np.arange(len(rays)) % 4, (1, 2, 3)) & (rays["o"][:, 0] >= 2.0)].any()   # the rays that start beyond the scene miss
    assert max_depth(o, shallow[:600]) <= MID_STACK - 4 and max_depth(o, deep[:4000]) > LDS_STACK + 2
    assert product_max_depth(t, rays, want) > LDS_STACK + 2
    compare_all_kernels(t, rays, want, want_any, "mixed waves")


def test_push_then_pop_in_one_pass(rc, oracle):
    """Child 0 hit but not first (t1_min < t0_min), child 1 missed: the reference pushes child 0 and pops it in the same step, the fast
    form reads back the slot it has just written.  Two triangles: A far along the ray, B next to the ray's start but off to the side
    (its box fails the slab test with a small t_min).  A's Morton code is the lower one, so A is child 0."""
    def tri(cx, cy, z, r):
        return np.array([cx - r, cy - r, z, cx + r, cy - r, z, cx, cy + r, z], dtype=np.float32)
    cfg = {"blas": [(np.stack([tri(0.25, 0.25, -5.0, 1.0), tri(2.5, 0.25, 0.0, 0.5)]), None)],
           "instances": [(1, rc.scenes.IDENTITY3x4.reshape(1, 12).astype(np.float32), np.arange(1, dtype=np.uint32))]}
    t, o = build_product(rc, cfg), build_oracle(oracle, cfg)
    g = rc.scenes.rng(3)
    n = 256
    org = np.array([0.25, 0.25, 1.0]) + g.uniform(-0.05, 0.05, size=(n, 3))
    d = rc.scenes.normalize(np.array([-0.01, 0.003, -1.0]) + g.uniform(-0.002, 0.002, size=(n, 3)))
    rays = rc.scenes.make_rays(org, d)
    both = 0
    for r in rays:
        ev = o.trace_events(r)[0]
        both += int(((ev & 0x63) == 0x61).any())   # a BLAS interior step (1) that pushed its far child (0x20) and popped (0x40)
    assert both == n, f"only {both} of {n} rays push and pop in one step"
    want, want_any = o.trace(rays), o.trace(rays, mode="any")
    assert want["hit"].all() and (want["primitive_id"] == want["primitive_id"][0]).all()
    compare_all_kernels(t, rays, want, want_any, "push-then-pop")
    t.set_option("kernel", 0)
    assert_hits_equal(t.trace(rays), want, "push-then-pop k0")


@pytest.mark.parametrize("shell", ["lds", "plain", "partial"])
def test_get_illumination_on_the_deep_scene(rc, oracle, shell):
    """phased_trace is shared, but the driver shells hold other registers around it: get_illumination on the deep scene through the
    top-level-in-LDS shell (4 instances), the plain shell (kernel 3) and the partial-LDS shell (304 instances: a top level too large
    for LDS), against the oracle's counts.  The oracle's deepest stack lies beyond both LDS depths."""
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
