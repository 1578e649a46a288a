"""rc_get_illumination_points_device / rc_point_source_rays_device on the GPU: get_illumination for lamps at a finite position, all
sources x grid^2 rays in one traversal launch per group.

The yardsticks: the numpy model (tests/point_source_model.py) for the rays, the model's rays traced by the CPU oracle and counted by the
oracle's metadata for the counts, and the product's own composed path (ray stage + rc_trace_closest_device + a bincount of the downloaded
hits).  Every comparison is np.array_equal; there is no tolerance.  Covered: the three kernel shells the launcher dispatches (top level in
LDS, plain, partial LDS) and a one-instance scene whose TLAS root is a leaf; isotropic and Lambertian sources inside, between and outside
the instances, with a range and with t_min > 0; grids whose rows a 128-item chunk and a wave straddle; the ray balance, dropped metadata
included; a furnace; accumulation, row stride, a NULL d_escaped; grouping; splitting by first_source; two streams into one matrix; a
captured frame replayed over poses with the lamps rewritten in place; a device-side geometry update; non-finite sources; the error
contract; the Python function."""
import ctypes as C

import numpy as np
import pytest

import dynamic_kit as dyn
import point_source_model as pm
from gpu_kit import POISON_U32 as POISON, f32_tensor, finish, u32_of
from gpu_kit import rc  # noqa: F401
from helpers import assert_rays_equal, build_oracle, build_product
from scene_kit import single_cfg, small_cfg

pytestmark = pytest.mark.gpu

GRIDS = (13, 24)  # 169 rays per source: a 128-item chunk and a 64-lane wave straddle two sources
SEED = 0x5EED0005
AXIS = (0.3, 0.2, 1.0)
LAMP = (0.25, -0.05, 0.2)  # inside the single sphere (tests/test_point_source_model.py: the furnace)
RC_ERR_INVALID_ARGUMENT, RC_ERR_NOT_SYNCED = 1, 6
HIT_DT = pm.bm.HIT_DT


def dev_bytes(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def zeros_u32(n):
    import torch
    return torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")


def lattice_sources(mn, mx):
    """Both kinds of source at the lattice centre, between instances and outside the scene, one with a range and one with t_min > 0."""
    mn, mx = np.asarray(mn, np.float64), np.asarray(mx, np.float64)
    centre = (mn + mx) / 2 + np.array([0.25, 0.25, 0.0])  # (a quarter pitch off the lattice's axis: on it the point lies inside a sphere)
    between, outside = np.array([0.5, 0.5, 0.5]), mn - np.array([2.0, 0.0, 0.0])
    points = [centre, between, outside, outside, centre, between]
    axes = [(0, 0, 0), AXIS, (0, 0, 0), (1.0, 0.1, 0.1), (0, 0, 0), (0, 0, 0)]  # (the fourth takes the other branch of the basis choice)
    src = pm.make_sources(points, axes)
    src["tmax"][4] = 0.75
    src["tmin"][5] = 0.7  # (the nearest spheres' near sides lie closer: those rays start inside or behind them)
    return src


def single_sources(mn, mx):
    """The same kinds around the one sphere (centre (0.2, -0.1, 0.3), radius 0.6): the lamp inside it sees nothing but the sphere."""
    mn, mx = np.asarray(mn, np.float64), np.asarray(mx, np.float64)
    centre, outside = (mn + mx) / 2, mn - np.array([2.0, 0.0, 0.0])
    above = centre + np.array([0.0, 0.0, 1.1])
    points = [LAMP, above, outside, outside, above, above]
    axes = [(0, 0, 0), (0.1, -0.2, -1.0), (0, 0, 0), (1.0, 0.1, 0.1), (0, 0, 0), (0, 0, 0)]
    src = pm.make_sources(points, axes)
    src["tmax"][4] = 0.75
    src["tmin"][5] = 0.7  # beyond the near side of the sphere (0.5 away): those rays pass through it and hit its far side from inside
    return src


class World:
    """One scene in the product and in the oracle, its sources, and the model's counts, computed once per argument set and read-only."""

    def __init__(self, rc, oracle, cfg, kernel=None, sources=lattice_sources):
        self.t, self.o = build_product(rc, cfg), build_oracle(oracle, cfg)
        if kernel is not None:
            self.t.set_option("kernel", kernel)
        self.n = self.t.n_primitives()
        bound = np.asarray(self.o.world_bound, np.float64).reshape(2, 3)
        self.src = sources(bound[0], bound[1])
        self.S = len(self.src)
        self.d_src = dev_bytes(self.src)
        self._want = {}

    def want(self, grid, seed=SEED, first_source=0, src=None):
        key = (grid, seed, first_source, None if src is None else src.tobytes())
        if key not in self._want:
            got = pm.expected_counts(self.o, self.src if src is None else src, grid, seed, first_source)
            for a in got:
                a.setflags(write=False)
            self._want[key] = got
        return self._want[key]

    def run(self, grid, n_sources=None, d_src=None, counts=None, escaped=True, row_stride=None, seed=SEED, first_source=0, stream=None):
        """One call into zeroed outputs (or into `counts` / `escaped` when they are tensors; escaped None: NULL).  Returns (counts, escaped)."""
        S = self.S if n_sources is None else n_sources
        rs = self.n if row_stride is None else row_stride
        if counts is None:
            counts = zeros_u32(S * rs)
        if escaped is True:
            escaped = zeros_u32(S)
        d_src = self.d_src if d_src is None else d_src
        if stream is not None:
            import torch
            for buf in (d_src, counts, escaped):
                if buf is not None:
                    buf.record_stream(stream)
            torch.cuda.synchronize()
        self.t.illumination_points_device(d_src.data_ptr(), S, grid, counts.data_ptr(), row_stride, escaped.data_ptr() if escaped is not None else None,
                                          seed=seed, first_source=first_source, stream=stream.cuda_stream if stream else None)
        return counts, escaped

    def stage(self, grid, n_sources=None, d_src=None, seed=SEED, first_source=0):
        """The ray stage into a poisoned buffer with a guard behind it -> (RAY_DT array, the tensor)."""
        import torch
        S = self.S if n_sources is None else n_sources
        words = S * grid * grid * 8
        out = torch.full((words + 64,), float("nan"), dtype=torch.float32, device="cuda")
        out[words:] = -77.0
        self.t.point_source_rays_device((self.d_src if d_src is None else d_src).data_ptr(), S, grid, out.data_ptr(), seed=seed, first_source=first_source)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[words:] == -77.0).all(), "rays were written behind the last source"
        return got[:words].view(pm.RAY_DT), out

    def composed(self, grid, n_sources=None, d_src=None, seed=SEED, first_source=0):
        """The product's own composed path: the stage, rc_trace_closest_device, a bincount of the downloaded hits."""
        import torch
        S = self.S if n_sources is None else n_sources
        _, d_rays = self.stage(grid, S, d_src, seed, first_source)
        total = S * grid * grid
        d_hits = torch.zeros(total * 32, dtype=torch.uint8, device="cuda")
        self.t.trace_device(d_rays.data_ptr(), d_hits.data_ptr(), total, mode="closest")
        finish(self.t)
        hits = d_hits.cpu().numpy().view(HIT_DT)
        return pm.counts_of(self.t.adapt().all_blas_prims["meta"], hits, S, grid, self.n)


def rows_of(w, counts, S=None, row_stride=None):
    S = w.S if S is None else S
    rs = w.n if row_stride is None else row_stride
    return u32_of(counts)[:S * rs].reshape(S, rs)


SHAPES = ["lds", "plain", "partial", "single"]


@pytest.fixture(scope="module")
def worlds(rc, oracle):
    w = {"lds": World(rc, oracle, small_cfg(rc, (3, 3, 2))),              # 18 instances: the whole top level in LDS
         "plain": World(rc, oracle, small_cfg(rc, (3, 3, 2)), kernel=3),  # the same scene through the 256-thread shell
         "partial": World(rc, oracle, small_cfg(rc, (7, 7, 6))),          # 294 instances: only the TLAS's top is staged
         "single": World(rc, oracle, single_cfg(rc), sources=single_sources)}  # one instance: the TLAS root is a leaf
    assert w["lds"].t.n_instances() == 18 and w["partial"].t.n_instances() == 294 and w["single"].t.n_instances() == 1
    assert w["partial"].t.get_option("tlas_top_k") > 0 and w["lds"].t.get_option("tlas_top_k") == 0
    # not vacuous, on the oracle's side alone: every row has hits, every source but the furnace's loses rays, the rows differ, and the
    # range and t_min matter
    for name, x in w.items():
        for grid in GRIDS:
            counts, escaped, dropped = x.want(grid)
            assert (counts.sum(axis=1) > 0).all() and not dropped.any(), (name, grid, counts.sum(axis=1))
            assert (escaped[1 if name == "single" else 0:] > 0).all(), (name, grid, escaped)
            assert (counts.sum(axis=1) + escaped == grid * grid).all()
            assert len({r.tobytes() for r in counts}) == x.S, (name, grid)
            free = x.src.copy()
            free["tmax"], free["tmin"] = np.inf, 0
            unbounded = x.want(grid, src=free)[0]
            assert not np.array_equal(unbounded[4], counts[4]) and not np.array_equal(unbounded[5], counts[5]), (name, grid)
    assert w["single"].want(24)[1][0] == 0
    yield w
    for x in w.values():
        x.t.free()


# ---- 1. the stage's rays are the model's --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["lds", "single"])
@pytest.mark.parametrize("grid", GRIDS)
def test_stage_rays_equal_the_models(worlds, shape, grid):
    w = worlds[shape]
    got, _ = w.stage(grid)
    assert_rays_equal(got, pm.point_source_rays(w.src, grid, SEED), f"{shape} grid {grid}")
    got, _ = w.stage(grid, n_sources=3, d_src=w.d_src[2 * 32:], seed=7, first_source=0xFFFFFFFD)  # the key word's upper end
    assert_rays_equal(got, pm.point_source_rays(w.src[2:5], grid, 7, first_source=0xFFFFFFFD), f"{shape} grid {grid}, keys up to 2^32 - 1")


# ---- 2, 4. counts and escaped against the model, in every shell; the ray balance ------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("grid", GRIDS)
def test_counts_and_escaped_equal_the_models(worlds, shape, grid):
    w = worlds[shape]
    counts, escaped = w.run(grid)
    finish(w.t)
    want, want_escaped, _ = w.want(grid)
    got, got_escaped = rows_of(w, counts), u32_of(escaped)[:w.S]
    assert np.array_equal(got, want), f"{shape} grid {grid}: rows {np.nonzero((got != want).any(axis=1))[0]} differ"
    assert np.array_equal(got_escaped, want_escaped), f"{shape} grid {grid}: escaped {got_escaped} want {want_escaped}"
    assert (got.sum(axis=1, dtype=np.uint64) + got_escaped == grid * grid).all()


# ---- 3. the product's own composed path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_counts_equal_the_composed_path(worlds, shape):
    w = worlds[shape]
    want, want_escaped, dropped = w.composed(24)
    counts, escaped = w.run(24)
    finish(w.t)
    assert np.array_equal(rows_of(w, counts), want) and np.array_equal(u32_of(escaped)[:w.S], want_escaped) and not dropped.any()


def test_dropped_rays_are_accounted_for(rc, oracle):
    """Metadata with gaps, duplicates, 0, N + 3 and 2^32 - 1: row sum + escaped + dropped = grid^2, with the model's dropped count."""
    sc = rc.scenes
    verts = sc.fan_sphere(12, 7, radius=0.6)
    n = len(verts)
    meta = np.arange(1, n + 1, dtype=np.uint32)
    meta[::5] = 0
    meta[1::5] = n + 3
    meta[2::5] = 0xFFFFFFFF
    meta[3::5] = 7
    cfg = {"blas": [(verts, meta)], "instances": [(1, sc.lattice_transforms(2, 2, 1, 1.3, 9)[0], np.arange(4, dtype=np.uint32))]}
    w = World(rc, oracle, cfg, sources=lambda mn, mx: pm.make_sources([(0.65, 0.65, 0.0), (0.65, 0.65, 1.5), (-2.0, 0.3, 0.1)], [(0, 0, 0), (0, 0.1, -1), (0, 0, 0)]))
    want, want_escaped, dropped = w.want(24)
    # not vacuous, on the oracle's side alone: every source has rays of all three kinds (the one outside sees little of the scene)
    assert (dropped > 0).all() and dropped.sum() > 100 and (want.sum(axis=1) > 0).all() and (want_escaped > 0).all(), (dropped, want.sum(axis=1), want_escaped)
    counts, escaped = w.run(24)
    finish(w.t)
    got, got_escaped = rows_of(w, counts), u32_of(escaped)[:w.S]
    assert np.array_equal(got, want) and np.array_equal(got_escaped, want_escaped)
    assert (got.sum(axis=1, dtype=np.uint64) + got_escaped + dropped == 24 * 24).all()
    composed = w.composed(24)
    assert np.array_equal(composed[0], want) and np.array_equal(composed[2], dropped)
    w.t.free()


# ---- 5. the furnace ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_furnace(worlds, grid):
    """Lamps of both kinds inside the closed sphere: no ray escapes, every row sums to grid^2."""
    w = worlds["single"]
    src = pm.make_sources([LAMP, LAMP, (0.2, -0.1, 0.3)], [(0, 0, 0), AXIS, (-1, 0, 0)])
    counts, escaped = w.run(grid, n_sources=3, d_src=dev_bytes(src))
    finish(w.t)
    got = rows_of(w, counts, 3)
    assert not u32_of(escaped)[:3].any() and (got.sum(axis=1) == grid * grid).all()
    want = w.want(grid, src=src)
    assert np.array_equal(got, want[0]) and not want[1].any()


# ---- 6. accumulation, stride, NULL d_escaped ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["lds", "partial"])
def test_a_second_call_doubles_the_counts(worlds, shape):
    w = worlds[shape]
    counts, escaped = w.run(13)
    w.run(13, counts=counts, escaped=escaped)
    finish(w.t)
    want, want_escaped, _ = w.want(13)
    assert np.array_equal(rows_of(w, counts), 2 * want) and np.array_equal(u32_of(escaped)[:w.S], 2 * want_escaped)


def test_row_stride_leaves_the_padding_alone(worlds):
    import torch
    w = worlds["lds"]
    stride = w.n + 7
    out = torch.from_numpy(np.full(w.S * stride + 16, POISON, np.uint32).view(np.int32)).cuda()
    out[:w.S * stride].view(w.S, stride)[:, :w.n] = 0
    esc = torch.from_numpy(np.full(w.S + 16, POISON, np.uint32).view(np.int32)).cuda()
    esc[:w.S] = 0
    w.run(24, counts=out, escaped=esc, row_stride=stride)
    finish(w.t)
    got, got_escaped = u32_of(out), u32_of(esc)
    rows = got[:w.S * stride].reshape(w.S, stride)
    want, want_escaped, _ = w.want(24)
    assert np.array_equal(rows[:, :w.n], want) and np.array_equal(got_escaped[:w.S], want_escaped)
    assert (rows[:, w.n:] == POISON).all() and (got[w.S * stride:] == POISON).all() and (got_escaped[w.S:] == POISON).all(), "words outside the outputs were written"


@pytest.mark.parametrize("shape", SHAPES)
def test_without_escaped_the_counts_are_the_same(worlds, shape):
    w = worlds[shape]
    counts, _ = w.run(24, escaped=None)
    finish(w.t)
    assert np.array_equal(rows_of(w, counts), w.want(24)[0])


# ---- 7. grouping: the scratch cap changes how many sources a launch takes, never a count ----------------------------------------------------
@pytest.mark.parametrize("shape", ["lds", "partial"])
def test_groups_of_one_and_two_give_the_same_rows(worlds, shape):
    w = worlds[shape]
    per_source = 16 * 8 * ((w.n + 7) // 8) * 4  # kHistCopies x 8 x n8 u32
    default = w.t.get_option("illum_scratch_bytes")
    want, want_escaped, _ = w.want(13)
    try:
        for cap in (1, 2 * per_source, 3 * per_source - 1, 4 * per_source):  # G = 1 (clamped up), 2, 2 and 4: 6 = 4 + 2, the last group short
            w.t.set_option("illum_scratch_bytes", cap)
            for with_escaped in (True, None):
                counts, escaped = w.run(13, escaped=with_escaped)
                finish(w.t)
                assert np.array_equal(rows_of(w, counts), want), f"illum_scratch_bytes = {cap}"
                assert escaped is None or np.array_equal(u32_of(escaped)[:w.S], want_escaped), f"illum_scratch_bytes = {cap}"
    finally:
        w.t.set_option("illum_scratch_bytes", default)


# ---- 8. splitting: first_source makes the parts the rows of the whole -----------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["lds", "single"])
def test_split_calls_give_the_rows_of_the_one_call(worlds, shape):
    w = worlds[shape]
    want, want_escaped, _ = w.want(24)
    head, head_escaped = w.run(24, n_sources=2)
    tail, tail_escaped = w.run(24, n_sources=3, d_src=w.d_src[2 * 32:], first_source=2)
    wrong, _ = w.run(24, n_sources=3, d_src=w.d_src[2 * 32:], first_source=0)
    finish(w.t)
    assert np.array_equal(rows_of(w, head, 2), want[:2]) and np.array_equal(u32_of(head_escaped)[:2], want_escaped[:2])
    assert np.array_equal(rows_of(w, tail, 3), want[2:5]) and np.array_equal(u32_of(tail_escaped)[:3], want_escaped[2:5])
    assert (rows_of(w, wrong, 3) != want[2:5]).any(axis=1).all(), "first_source does not reach the random numbers"
    assert np.array_equal(rows_of(w, wrong, 3), w.want(24, src=w.src[2:5])[0])


# ---- 9. two streams adding into one matrix ---------------------------------------------------------------------------------------------------
def test_two_streams_into_one_matrix(worlds):
    import torch
    w = worlds["partial"]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    counts, escaped = zeros_u32(w.S * w.n), zeros_u32(w.S)
    for _ in range(3):
        w.run(24, counts=counts, escaped=escaped, stream=s1)
        w.run(13, counts=counts, escaped=escaped, stream=s2)
    s1.synchronize(); s2.synchronize()
    finish(w.t)
    a, b = w.want(24), w.want(13)
    assert np.array_equal(rows_of(w, counts), 3 * (a[0] + b[0])) and np.array_equal(u32_of(escaped)[:w.S], 3 * (a[1] + b[1]))


# ---- 10. a captured frame: update -> refit -> zero -> illumination, replayed over poses with the lamps rewritten ------------------------------
_pose_cache = {}


def pose_sources(f):
    """Lamps inside and outside the lattice of tests/test_gpu_rebuild.py at frame f (pitch 1.5 + 0.2 f): they move with the pose."""
    p = 1.5 + 0.2 * f
    return pm.make_sources([(2.5 * p, 2.5 * p, 1.5 * p), (0.5 * p, 0.5 * p, 0.5 * p), (-2.0, 0.3 * f, 0.1), (2.0 * p, 2.5 * p, -1.5), (2.5 * p, 2.5 * p, 1.5 * p)],
                           [(0, 0, 0), AXIS, (1, 0.1 * f, 0.2), (0.1, 0, 1), (0, 0, 0)], t_max=[np.inf, np.inf, np.inf, np.inf, 1.25 + 0.25 * f])


def pose_want(oracle, rc, f, grid):
    if f not in _pose_cache:
        o = oracle.Scene()
        b = o.add_blas(dyn.sphere(rc))
        for i, x in enumerate(dyn.rebuild_frame_xf(rc, dyn.SMALL, f)):
            o.add_instance(b, x, i)
        o.build()
        _pose_cache[f] = o
    want = pm.expected_counts(_pose_cache[f], pose_sources(f), grid, SEED)
    assert (want[0].sum(axis=1) > 0).all() and (want[1] > 0).all(), (f, want[0].sum(axis=1), want[1])
    return want


def test_captured_frame_follows_the_scene_and_the_lamps(rc, oracle):
    import torch
    grid = 24
    a = dyn.Frames(rc, dyn.SMALL, 1)
    n = a.t.n_primitives()
    frames = (1, dyn.TIE_FRAME, 0)
    wants = {f: pose_want(oracle, rc, f, grid) for f in (0,) + frames}
    assert not np.array_equal(wants[0][0], wants[1][0]) and not np.array_equal(wants[1][0], wants[dyn.TIE_FRAME][0])
    d_src = dev_bytes(pose_sources(0))
    d_counts = torch.full((5 * n,), 0x55, dtype=torch.int32, device="cuda")
    d_escaped = torch.full((5,), 0x55, dtype=torch.int32, device="cuda")
    for buf in (d_src, d_counts, d_escaped):
        buf.record_stream(a.s)
    torch.cuda.synchronize()

    def frame(st):
        a.t.update_transforms_device(a.h, a.d_xf, stream=st)
        a.t.refit_device_async(stream=st)
        d_counts.zero_()
        d_escaped.zero_()
        a.t.illumination_points_device(d_src.data_ptr(), 5, grid, d_counts.data_ptr(), None, d_escaped.data_ptr(), seed=SEED, stream=st)

    def check(f, what):
        assert np.array_equal(u32_of(d_counts).reshape(5, n), wants[f][0]), what
        assert np.array_equal(u32_of(d_escaped), wants[f][1]), what

    with torch.cuda.stream(a.s):
        frame(a.s.cuda_stream)  # eager first, as for every captured launch: frame 0
    a.s.synchronize()
    check(0, "eager frame 0")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=a.s):
        frame(torch.cuda.current_stream().cuda_stream)
    for f in frames:
        with torch.cuda.stream(a.s):
            a.d_xf.copy_(a.frames[f])  # in place: the graph reads the tensors when it runs
            d_src.copy_(dev_bytes(pose_sources(f)))
            g.replay()
        a.s.synchronize()
        check(f, f"replay at frame {f}")
    del g
    torch.cuda.synchronize()
    a.t.wait_for_gpu()
    a.t.set_option("release_captures", 1)
    assert a.t.get_option("release_captures") == 0
    a.t.free()


# ---- 11. behind a device-side geometry update on the same stream, no host wait ----------------------------------------------------------------
def test_after_a_geometry_update_on_the_same_stream(rc, oracle):
    import torch
    spec = dyn.Spec(rc, "144")
    t, hs = spec.build(rc)
    f, grid = 3, 24
    o = oracle.Scene()
    b = o.add_blas(dyn.deform(spec.soups[0], f))
    for i, x in enumerate(spec.xf):
        o.add_instance(b, x, i)
    o.build()
    src = pm.make_sources([(0.8, 0.8, 0.8), (4.0, 4.0, 2.4), (-2.0, 0.5, 0.3)], [(0, 0, 0), AXIS, (1, 0.2, 0.1)])
    want, want_escaped, _ = pm.expected_counts(o, src, grid, SEED)
    before = pm.expected_counts(build_oracle(oracle, {"blas": [(spec.soups[0],)], "instances": [(1, spec.xf, np.arange(len(spec.xf)))]}), src, grid, SEED)[0]
    assert (want.sum(axis=1) > 0).all() and (want_escaped > 0).all() and not np.array_equal(want, before)
    n = t.n_primitives()
    s = torch.cuda.Stream()
    d_soup = torch.from_numpy(dyn.deform(spec.soups[0], f)).cuda()
    d_src, d_counts, d_escaped = dev_bytes(src), zeros_u32(3 * n), zeros_u32(3)
    for buf in (d_soup, d_src, d_counts, d_escaped):
        buf.record_stream(s)
    torch.cuda.synchronize()
    t.update_geometry_device_async(hs[-1], d_soup, stream=s.cuda_stream)
    t.rebuild_device_async(stream=s.cuda_stream)
    t.illumination_points_device(d_src.data_ptr(), 3, grid, d_counts.data_ptr(), None, d_escaped.data_ptr(), seed=SEED, stream=s.cuda_stream)
    s.synchronize()
    t.wait_for_gpu()
    assert np.array_equal(u32_of(d_counts).reshape(3, n), want) and np.array_equal(u32_of(d_escaped), want_escaped)
    t.free()


# ---- 12. non-finite sources: the rows of the composed path, nothing faults ------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["lds", "plain", "partial"])
def test_non_finite_sources_give_the_composed_rows(worlds, shape):
    w = worlds[shape]
    centre = w.src["o"][0]
    src = pm.make_sources([(np.nan, 0.5, 0.5), centre, centre, (np.inf, 0, 0), centre], [(0, 0, 0), (np.inf, 0, 1), (np.nan, 0, 0), AXIS, (0, 0, 0)])
    src["tmax"][4] = np.nan
    d_src = dev_bytes(src)
    want, want_escaped, _ = w.composed(13, n_sources=5, d_src=d_src)
    counts, escaped = w.run(13, n_sources=5, d_src=d_src)
    finish(w.t)
    assert np.array_equal(rows_of(w, counts, 5), want) and np.array_equal(u32_of(escaped)[:5], want_escaped)
    assert (want.sum(axis=1, dtype=np.uint64) + want_escaped == 169).all()


# ---- 13. the error contract ---------------------------------------------------------------------------------------------------------------
def test_errors_and_empty_work(rc, worlds):
    import torch
    L = rc.lib()
    w = worlds["lds"]
    n, S = w.n, w.S
    out = torch.from_numpy(np.full(S * n, POISON, np.uint32).view(np.int32)).cuda()
    esc = torch.from_numpy(np.full(S, POISON, np.uint32).view(np.int32)).cuda()
    rays = torch.from_numpy(np.full(S * 13 * 13 * 8, POISON, np.uint32).view(np.int32)).cuda()
    P = lambda t: C.c_void_p(t.data_ptr())
    src = P(w.d_src)

    def illum(scene, sources, n_sources, grid, counts, stride, first=0, escaped=None):
        return L.rc_get_illumination_points_device(scene, sources, n_sources, grid, SEED, first, counts, stride, escaped if escaped is not None else P(esc), None)

    def stage(scene, sources, n_sources, grid, d_rays, first=0):
        return L.rc_point_source_rays_device(scene, sources, n_sources, grid, SEED, first, d_rays, None)

    def untouched():
        torch.cuda.synchronize()
        return (u32_of(out) == POISON).all() and (u32_of(esc) == POISON).all() and (u32_of(rays) == POISON).all()

    assert illum(None, src, S, 13, P(out), n) == RC_ERR_INVALID_ARGUMENT
    assert illum(w.t._h, None, S, 13, P(out), n) == RC_ERR_INVALID_ARGUMENT
    assert illum(w.t._h, src, S, 13, None, n) == RC_ERR_INVALID_ARGUMENT
    assert illum(w.t._h, src, S, 13, P(out), n - 1) == RC_ERR_INVALID_ARGUMENT and "row_stride" in L.rc_last_error().decode()
    assert illum(w.t._h, src, S, 65536, P(out), n) == RC_ERR_INVALID_ARGUMENT
    assert illum(w.t._h, src, S, 13, P(out), n, first=0xFFFFFFFF - S + 2) == RC_ERR_INVALID_ARGUMENT and "first_source" in L.rc_last_error().decode()
    assert stage(None, src, S, 13, P(rays)) == RC_ERR_INVALID_ARGUMENT
    assert stage(w.t._h, None, S, 13, P(rays)) == RC_ERR_INVALID_ARGUMENT
    assert stage(w.t._h, src, S, 13, None) == RC_ERR_INVALID_ARGUMENT
    assert stage(w.t._h, src, S, 65536, P(rays)) == RC_ERR_INVALID_ARGUMENT
    assert stage(w.t._h, src, S, 13, P(rays), first=0xFFFFFFFF - S + 2) == RC_ERR_INVALID_ARGUMENT
    # zero work: success, nothing enqueued, no pointer needed
    assert illum(w.t._h, None, 0, 13, None, 0) == 0 and illum(w.t._h, src, S, 0, P(out), n) == 0
    assert stage(w.t._h, None, 0, 13, None) == 0 and stage(w.t._h, src, S, 0, P(rays)) == 0
    empty = rc.TLAS()
    empty.sync()
    assert illum(empty._h, src, S, 13, P(out), 0) == 0 and stage(empty._h, src, S, 13, P(rays)) == 0
    empty.free()
    assert untouched()
    # never synced
    t, (h,), _ = dyn.make_scene(rc, (2, 2, 1))
    fresh = rc.TLAS()
    fresh.push_instances(fresh.add_geometry(dyn.sphere(rc)), dyn.initial_xf(rc, (2, 2, 1)), np.arange(4, dtype=np.uint32))
    assert illum(fresh._h, src, S, 13, P(out), n) == RC_ERR_NOT_SYNCED and stage(fresh._h, src, S, 13, P(rays)) == RC_ERR_NOT_SYNCED
    fresh.free()
    # pending host-side mutations
    np_t = t.n_primitives()
    assert np_t <= n
    t.update_transforms(h, dyn.frame_xf(rc, (2, 2, 1), 1))
    assert illum(t._h, src, S, 13, P(out), np_t) == RC_ERR_NOT_SYNCED and stage(t._h, src, S, 13, P(rays)) == RC_ERR_NOT_SYNCED
    t.sync()
    # transforms-dirty from the device, no refit yet
    d_xf = f32_tensor(dyn.frame_xf(rc, (2, 2, 1), 2))
    t.update_transforms_device(h, d_xf)
    assert illum(t._h, src, S, 13, P(out), np_t) == RC_ERR_NOT_SYNCED and stage(t._h, src, S, 13, P(rays)) == RC_ERR_NOT_SYNCED
    assert untouched()
    t.refit_device_async()
    assert illum(t._h, src, S, 13, P(out), np_t) == 0 and stage(t._h, src, S, 13, P(rays)) == 0
    # the last legal key: first_source + n_sources = 2^32
    assert stage(t._h, src, S, 13, P(rays), first=0xFFFFFFFF - S + 1) == 0
    torch.cuda.synchronize()
    t.wait_for_gpu()
    assert not (u32_of(rays) == POISON).any()
    t.free()


# ---- 14. the Python function --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["lds", "single"])
def test_get_illumination_points(rc, worlds, shape):
    w = worlds[shape]
    src = w.src[:4]  # (the host call takes positions, axes and a range: t_min stays 0)
    want, want_escaped, _ = w.want(24, seed=3, src=src)
    rows, escaped = rc.get_illumination_points(w.t, src["o"], 24, axes=src["d"], seed=3, return_escaped=True)
    assert rows.dtype == np.uint32 and rows.shape == (4, w.n) and escaped.dtype == np.uint32
    assert np.array_equal(rows, want) and np.array_equal(escaped, want_escaped)
    assert np.array_equal(rc.get_illumination_points(w.t, src["o"], 24, axes=src["d"], seed=3), want)
    weights = np.array([0.5, 1.25, 3.0, 0.0])
    got = rc.get_illumination_points(w.t, src["o"], 24, axes=src["d"], weights=weights, seed=3)
    assert got.dtype == np.float64 and got.shape == (w.n,)
    assert np.array_equal(got, (weights @ want.astype(np.float64)) / 576.0)
    # a range, per source; and no axes: all isotropic
    reach = np.array([0.75, np.inf, 1.0, np.inf], np.float32)
    ranged = pm.make_sources(src["o"], None, t_max=reach)
    got = rc.get_illumination_points(w.t, src["o"], 13, max_dist=reach, seed=3)
    assert np.array_equal(got, w.want(13, seed=3, src=ranged)[0])
