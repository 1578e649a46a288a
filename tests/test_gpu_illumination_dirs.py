"""rc_get_illumination_dirs_device / rc_generate_ray_grid_dirs_device on the GPU: get_illumination for many view directions in one call,
the grids laid out on the device from the TLAS root.

The yardstick is always the CPU oracle, per direction, on a scene built from scratch at the pose under test: oracle.Scene.get_illumination
and .ray_grid.  Every comparison is np.array_equal; there is no tolerance.  Covered: the three kernel shells the launcher dispatches (top
level in LDS, plain, partial LDS) and a one-instance scene whose TLAS root is a leaf; grids whose rows a 128-item chunk and a wave straddle;
accumulation, row stride, dropped metadata, grouping of the directions (option "illum_scratch_bytes"); the ray grids, degenerate directions
included; a captured frame update -> refit / rebuild -> zero -> illumination replayed over poses of which one grows the world bound, with
the directions rewritten in place; no dependence on the host copy of the bound; two streams; the error contract; the Python function."""
import ctypes as C

import numpy as np
import pytest

import dynamic_kit as dyn
from gpu_kit import POISON_U32 as POISON, f32_tensor, finish, u32_of
from gpu_kit import rc  # noqa: F401
from helpers import build_oracle, build_product
from scene_kit import single_cfg, small_cfg

pytestmark = pytest.mark.gpu

DIRS = np.array([[0, 0, 1], [0.3, 0.2, 1], [1, 0.1, 0.1],  # the third takes the other branch of the basis choice (|x| >= 0.9)
                 [0, -1, 0], [0, 0, 5]], np.float32)        # the last is not normalised
GRIDS = (13, 24)  # 169 rays per direction: a 128-item chunk and a 64-lane wave straddle two directions
RC_ERR_INVALID_ARGUMENT, RC_ERR_NOT_SYNCED = 1, 6


class World:
    """One scene in the product and in the oracle; the oracle's rows are computed once per (direction, grid) and never written again."""

    def __init__(self, rc, oracle, cfg, kernel=None):
        self.t, self.o = build_product(rc, cfg), build_oracle(oracle, cfg)
        if kernel is not None:
            self.t.set_option("kernel", kernel)
        self.n = self.t.n_primitives()
        self._rows = {}

    def want(self, dirs, grid):
        rows = []
        for d in np.asarray(dirs, np.float32):
            key = (d.tobytes(), grid)
            if key not in self._rows:
                row = self.o.get_illumination(d, grid, nthreads=8)
                assert row.max() < (1 << 24) and np.array_equal(row, np.floor(row))
                row = row.astype(np.uint32)
                row.setflags(write=False)
                self._rows[key] = row
            rows.append(self._rows[key])
        return np.stack(rows)

    def run(self, dirs, grid, out=None, row_stride=None, stream=None):
        """One call for all of `dirs` into a zeroed (D, row_stride) matrix (or into `out`); returns the tensor."""
        import torch
        d_dirs = f32_tensor(dirs)
        rs = self.n if row_stride is None else row_stride
        if out is None:
            out = torch.zeros(len(dirs) * rs, dtype=torch.int32, device="cuda")
        if stream is not None:
            d_dirs.record_stream(stream)
            out.record_stream(stream)
            torch.cuda.synchronize()
        self.t.illumination_dirs_device(d_dirs.data_ptr(), len(dirs), grid, out.data_ptr(), row_stride, stream=stream.cuda_stream if stream else None)
        return out


@pytest.fixture(scope="module")
def worlds(rc, oracle):
    w = {"lds": World(rc, oracle, small_cfg(rc, (3, 3, 2))),              # 18 instances: the whole top level in LDS
         "plain": World(rc, oracle, small_cfg(rc, (3, 3, 2)), kernel=3),  # the same scene through the 256-thread shell
         "partial": World(rc, oracle, small_cfg(rc, (7, 7, 6))),          # 294 instances of a 256-triangle BLAS: only the TLAS's top is staged
         "single": World(rc, oracle, single_cfg(rc))}                     # one instance: the TLAS root is a leaf
    assert w["lds"].t.n_instances() == 18 and w["partial"].t.n_instances() == 294 and w["single"].t.n_instances() == 1
    assert w["partial"].t.get_option("tlas_top_k") > 0 and w["lds"].t.get_option("tlas_top_k") == 0
    # not vacuous, on the oracle's side alone: every direction lights the scene, and the rows are not all the same
    for name, x in w.items():
        for grid in GRIDS:
            rows = x.want(DIRS, grid)
            assert (rows.sum(axis=1) > 0.2 * grid * grid).all(), (name, grid, rows.sum(axis=1))
            assert sum(not np.array_equal(rows[0], r) for r in rows[1:]) >= 1, (name, grid)
    yield w
    for x in w.values():
        x.t.free()


# ---- 1. every row against the oracle, in every shell ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["lds", "plain", "partial", "single"])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("n_dirs", [1, 3, 5])
def test_rows_equal_the_oracles(worlds, shape, grid, n_dirs):
    w = worlds[shape]
    out = w.run(DIRS[:n_dirs], grid)
    finish(w.t)
    got = u32_of(out).reshape(n_dirs, w.n)
    assert np.array_equal(got, w.want(DIRS[:n_dirs], grid)), f"{shape} grid {grid} D {n_dirs}"


def test_direction_order_is_free(worlds):
    """Row d belongs to d_dirs[d], whatever stands next to it."""
    w = worlds["lds"]
    order = [3, 0, 4, 2, 1]
    out = w.run(DIRS[order], 13)
    finish(w.t)
    assert np.array_equal(u32_of(out).reshape(5, w.n), w.want(DIRS[order], 13))


# ---- 2. accumulation, stride, metadata -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["lds", "partial"])
def test_a_second_call_doubles_the_counts(worlds, shape):
    w = worlds[shape]
    out = w.run(DIRS, 13)
    w.run(DIRS, 13, out=out)
    finish(w.t)
    assert np.array_equal(u32_of(out).reshape(5, w.n), 2 * w.want(DIRS, 13))


def test_row_stride_leaves_the_padding_alone(worlds):
    import torch
    w = worlds["lds"]
    stride = w.n + 7
    out = torch.from_numpy(np.full(5 * stride + 16, POISON, np.uint32).view(np.int32)).cuda()
    out[:5 * stride].view(5, stride)[:, :w.n] = 0
    w.run(DIRS, 24, out=out, row_stride=stride)
    finish(w.t)
    got = u32_of(out)
    rows = got[:5 * stride].reshape(5, stride)
    assert np.array_equal(rows[:, :w.n], w.want(DIRS, 24))
    assert (rows[:, w.n:] == POISON).all() and (got[5 * stride:] == POISON).all(), "words outside the rows were written"


def test_metadata_outside_1_to_n_is_dropped(rc, oracle):
    sc = rc.scenes
    verts = sc.fan_sphere(12, 7, radius=0.6)
    n = len(verts)
    meta = np.arange(1, n + 1, dtype=np.uint32)
    meta[::5] = 0          # below the range
    meta[1::5] = n + 3     # above it
    meta[2::5] = 0xFFFFFFFF
    meta[3::5] = 7         # many faces share one counter
    cfg = {"blas": [(verts, meta)], "instances": [(1, sc.lattice_transforms(2, 2, 1, 1.3, 9)[0], np.arange(4, dtype=np.uint32))]}
    w = World(rc, oracle, cfg)
    want = w.want(DIRS, 24)
    rays_hitting = [int((w.o.trace(w.o.ray_grid(d, 24), nthreads=8)["hit"] == 1).sum()) for d in DIRS]
    assert (want.sum(axis=1) > 0.05 * 24 * 24).all() and (want.sum(axis=1) < 0.6 * np.array(rays_hitting)).all(), (want.sum(axis=1), rays_hitting)
    out = w.run(DIRS, 24)
    finish(w.t)
    assert np.array_equal(u32_of(out).reshape(5, w.n), want)
    w.t.free()


# ---- 3. grouping: the scratch cap changes how many directions a launch takes, never a count ----------------------------------------------
@pytest.mark.parametrize("shape", ["lds", "partial"])
def test_groups_of_one_and_two_give_the_same_rows(worlds, shape):
    w = worlds[shape]
    per_dir = 16 * 8 * ((w.n + 7) // 8) * 4  # kHistCopies x 8 x n8 u32
    default = w.t.get_option("illum_scratch_bytes")
    assert default == 256 << 20
    whole = u32_of(w.run(DIRS, 13)).copy()
    try:
        for cap in (1, 2 * per_dir, 3 * per_dir - 1):  # G = 1 (clamped up to one direction's worth), G = 2 twice: 5 = 2 + 2 + 1, the last group short
            w.t.set_option("illum_scratch_bytes", cap)
            assert w.t.get_option("illum_scratch_bytes") == cap
            out = w.run(DIRS, 13)
            finish(w.t)
            assert np.array_equal(u32_of(out), whole), f"illum_scratch_bytes = {cap}"
    finally:
        w.t.set_option("illum_scratch_bytes", default)
    assert np.array_equal(whole.reshape(5, w.n), w.want(DIRS, 13))


# ---- 4. the ray grids -----------------------------------------------------------------------------------------------------------------
def ray_grids(w, dirs, grid):
    import torch
    d_dirs = f32_tensor(dirs)
    out = torch.full((len(dirs) * grid * grid * 8 + 64,), float("nan"), dtype=torch.float32, device="cuda")
    out[len(dirs) * grid * grid * 8:] = -77.0
    w.t.ray_grid_dirs_device(d_dirs.data_ptr(), len(dirs), grid, out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[len(dirs) * grid * grid * 8:] == -77.0).all(), "rays were written behind the last grid"
    return got[:len(dirs) * grid * grid * 8].view(np.uint32).reshape(len(dirs), grid * grid, 8)


@pytest.mark.parametrize("shape", ["lds", "partial", "single"])
@pytest.mark.parametrize("grid", GRIDS)
def test_ray_grids_equal_the_oracles(worlds, shape, grid):
    w = worlds[shape]
    got = ray_grids(w, DIRS, grid)
    for d in range(len(DIRS)):
        want = w.o.ray_grid(DIRS[d], grid)
        assert np.array_equal(got[d], np.ascontiguousarray(want).view(np.uint32).reshape(-1, 8)), f"{shape} grid {grid} direction {d}"


def test_degenerate_directions_give_the_one_direction_grids(rc, worlds):
    """A direction whose normalisation is not finite: whatever rc_generate_ray_grid_device gives for it, byte for byte."""
    import torch
    w = worlds["lds"]
    dirs = np.array([[0, 0, 0], [np.nan, np.nan, np.nan], [0.3, 0.2, 1]], np.float32)
    got = ray_grids(w, dirs, 13)
    for d in range(len(dirs)):
        one = torch.zeros(13 * 13 * 8, dtype=torch.float32, device="cuda")
        status = rc.lib().rc_generate_ray_grid_device(w.t._h, dirs[d].ctypes.data_as(C.c_void_p), 13, C.c_void_p(one.data_ptr()), None)
        assert status == 0, rc.lib().rc_last_error().decode()
        torch.cuda.synchronize()
        assert np.array_equal(got[d], one.cpu().numpy().view(np.uint32).reshape(-1, 8)), f"direction {dirs[d]}"
    # ... and the counts: nothing for the degenerate ones (a NaN ray hits nothing on either path), the oracle's for the third
    out = w.run(dirs, 13)
    finish(w.t)
    rows = u32_of(out).reshape(3, w.n)
    for d in range(len(dirs)):
        assert np.array_equal(rows[d].astype(np.float32), rc.get_illumination(w.t, dirs[d], 13)), f"direction {dirs[d]}"


# ---- 5. a captured frame: update -> refit / rebuild -> zero -> illumination, replayed over poses ----------------------------------------
_pose_cache = {}
# Directions per frame of the animation of tests/test_gpu_rebuild.py.  Its lattice is sparse (pitch 1.5 to 2.1, spheres of radius <= 0.5):
# along an axis the columns line up and under a fifth of the rays hit, so the later frames are lit obliquely (checked in pose_rows).
POSE_DIRS = {0: DIRS,
             1: np.array([[0.3, 0.2, 1], [-0.2, 0.1, -1], [0.4, 1, 0.3], [1, 0.3, 0.2], [0.5, -2, 0.5]], np.float32),
             dyn.TIE_FRAME: np.array([[0.3, 0.2, 1], [0.75, -3, 0.3], [1, 0.3, 0.2], [0.1, 1, 0.45], [-0.2, 0.1, -1]], np.float32)}


def pose_rows(oracle, rc, f, dirs, grid):
    """The oracle built from scratch with frame f's transforms (tests/test_gpu_rebuild.py), its rows for `dirs`."""
    if f not in _pose_cache:
        o = oracle.Scene()
        b = o.add_blas(dyn.sphere(rc))
        for i, x in enumerate(dyn.rebuild_frame_xf(rc, dyn.SMALL, f)):
            o.add_instance(b, x, i)
        o.build()
        _pose_cache[f] = o
    o = _pose_cache[f]
    rows = np.stack([o.get_illumination(d, grid, nthreads=8) for d in np.asarray(dirs, np.float32)]).astype(np.uint32)
    assert (rows.sum(axis=1) > 0.2 * grid * grid).all(), (f, rows.sum(axis=1))
    return rows


def bound_of(o):
    return np.asarray(o.world_bound, np.float32).reshape(2, 3)


@pytest.mark.parametrize("commit", ["refit", "rebuild"])
def test_captured_frame_follows_the_scene_and_the_directions(rc, oracle, commit):
    import torch
    grid = 24
    a = dyn.Frames(rc, dyn.SMALL, 1)
    n = a.t.n_primitives()
    dir_sets = POSE_DIRS
    wants = {f: pose_rows(oracle, rc, f, dirs, grid) for f, dirs in dir_sets.items()}
    # the last pose has the widest pitch: its bound holds the others', so a grid laid out from an earlier bound would miss the rim
    b0, b3 = bound_of(_pose_cache[0]), bound_of(_pose_cache[dyn.TIE_FRAME])
    assert (b3[1] > b0[1] + 1.5).all(), (b0, b3)  # (the lattice grows away from the origin: the upper corner moves)
    d_dirs = f32_tensor(dir_sets[0])
    d_counts = torch.full((5 * n,), 0x55, dtype=torch.int32, device="cuda")
    for buf in (d_dirs, d_counts):
        buf.record_stream(a.s)
    torch.cuda.synchronize()

    def frame(st):
        a.t.update_transforms_device(a.h, a.d_xf, stream=st)
        (a.t.refit_device_async if commit == "refit" else a.t.rebuild_device_async)(stream=st)
        d_counts.zero_()
        a.t.illumination_dirs_device(d_dirs.data_ptr(), 5, grid, d_counts.data_ptr(), stream=st)

    with torch.cuda.stream(a.s):
        frame(a.s.cuda_stream)  # eager first, as for every captured launch: frame 0
    a.s.synchronize()
    assert np.array_equal(u32_of(d_counts).reshape(5, n), wants[0]), "eager frame 0"
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=a.s):
        frame(torch.cuda.current_stream().cuda_stream)
    for f in (1, dyn.TIE_FRAME, 0):
        with torch.cuda.stream(a.s):
            a.d_xf.copy_(a.frames[f])            # in place: the graph reads the tensors when it runs
            d_dirs.copy_(f32_tensor(dir_sets[f]))
            g.replay()
        a.s.synchronize()
        assert np.array_equal(u32_of(d_counts).reshape(5, n), wants[f]), f"{commit}: replay at frame {f}"
    del g
    torch.cuda.synchronize()
    a.t.wait_for_gpu()
    a.t.set_option("release_captures", 1)
    assert a.t.get_option("release_captures") == 0
    a.t.free()


def test_no_host_copy_of_the_bound_is_needed(rc, oracle):
    """After an eager asynchronous refit the host copy of the world bound is stale; the call neither waits for it nor reads it."""
    import torch
    grid, f = 24, dyn.TIE_FRAME
    a = dyn.Frames(rc, dyn.SMALL, 1)
    n = a.t.n_primitives()
    want = pose_rows(oracle, rc, f, POSE_DIRS[f], grid)
    d_dirs = f32_tensor(POSE_DIRS[f])
    d_counts = torch.zeros(5 * n, dtype=torch.int32, device="cuda")
    for buf in (d_dirs, d_counts):
        buf.record_stream(a.s)
    torch.cuda.synchronize()
    with torch.cuda.stream(a.s):
        a.d_xf.copy_(a.frames[f])
    a.t.update_transforms_device(a.h, a.d_xf, stream=a.s.cuda_stream)
    a.t.refit_device_async(stream=a.s.cuda_stream)
    a.t.illumination_dirs_device(d_dirs.data_ptr(), 5, grid, d_counts.data_ptr(), stream=a.s.cuda_stream)
    a.s.synchronize()
    assert np.array_equal(u32_of(d_counts).reshape(5, n), want)
    a.t.wait_for_gpu()
    a.t.free()


# ---- 6. two streams at once into two matrices ----------------------------------------------------------------------------------------
def test_two_streams_into_two_matrices(worlds):
    import torch
    w = worlds["partial"]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    da, db = DIRS, DIRS[::-1].copy()
    outs = []
    for _ in range(3):
        outs.append((w.run(da, 24, stream=s1), w.run(db, 13, stream=s2)))
    s1.synchronize(); s2.synchronize()
    finish(w.t)
    for oa, ob in outs:
        assert np.array_equal(u32_of(oa).reshape(5, w.n), w.want(da, 24))
        assert np.array_equal(u32_of(ob).reshape(5, w.n), w.want(db, 13))


# ---- 7. the error contract ----------------------------------------------------------------------------------------------------------------
def test_errors_and_empty_work(rc, worlds):
    import torch
    L = rc.lib()
    w = worlds["lds"]
    n = w.n
    d_dirs = f32_tensor(DIRS)
    out = torch.from_numpy(np.full(5 * n, POISON, np.uint32).view(np.int32)).cuda()
    rays = torch.from_numpy(np.full(5 * 13 * 13 * 8, POISON, np.uint32).view(np.int32)).cuda()
    P = lambda t: C.c_void_p(t.data_ptr())

    def illum(scene, dirs, n_dirs, grid, counts, stride):
        return L.rc_get_illumination_dirs_device(scene, dirs, n_dirs, grid, counts, stride, None)

    def grids(scene, dirs, n_dirs, grid, d_rays):
        return L.rc_generate_ray_grid_dirs_device(scene, dirs, n_dirs, grid, d_rays, None)

    def untouched():
        torch.cuda.synchronize()
        return (u32_of(out) == POISON).all() and (u32_of(rays) == POISON).all()

    assert illum(None, P(d_dirs), 5, 13, P(out), n) == RC_ERR_INVALID_ARGUMENT
    assert illum(w.t._h, None, 5, 13, P(out), n) == RC_ERR_INVALID_ARGUMENT
    assert illum(w.t._h, P(d_dirs), 5, 13, None, n) == RC_ERR_INVALID_ARGUMENT
    assert illum(w.t._h, P(d_dirs), 5, 13, P(out), n - 1) == RC_ERR_INVALID_ARGUMENT and "row_stride" in L.rc_last_error().decode()
    assert illum(w.t._h, P(d_dirs), 5, 65536, P(out), n) == RC_ERR_INVALID_ARGUMENT
    assert grids(None, P(d_dirs), 5, 13, P(rays)) == RC_ERR_INVALID_ARGUMENT
    assert grids(w.t._h, None, 5, 13, P(rays)) == RC_ERR_INVALID_ARGUMENT
    assert grids(w.t._h, P(d_dirs), 5, 13, None) == RC_ERR_INVALID_ARGUMENT
    # zero work: success, nothing enqueued, no pointer needed
    assert illum(w.t._h, None, 0, 13, None, 0) == 0 and illum(w.t._h, P(d_dirs), 5, 0, P(out), n) == 0
    assert grids(w.t._h, None, 0, 13, None) == 0 and grids(w.t._h, P(d_dirs), 5, 0, P(rays)) == 0
    empty = rc.TLAS()
    empty.sync()
    assert illum(empty._h, P(d_dirs), 5, 13, P(out), 0) == 0 and grids(empty._h, P(d_dirs), 5, 13, P(rays)) == 0
    empty.free()
    assert untouched()
    # never synced
    t, (h,), _ = dyn.make_scene(rc, (2, 2, 1))
    fresh = rc.TLAS()
    fresh.push_instances(fresh.add_geometry(dyn.sphere(rc)), dyn.initial_xf(rc, (2, 2, 1)), np.arange(4, dtype=np.uint32))
    assert illum(fresh._h, P(d_dirs), 5, 13, P(out), n) == RC_ERR_NOT_SYNCED and grids(fresh._h, P(d_dirs), 5, 13, P(rays)) == RC_ERR_NOT_SYNCED
    fresh.free()
    # pending host-side mutations
    np_t = t.n_primitives()
    assert np_t <= n
    t.update_transforms(h, dyn.frame_xf(rc, (2, 2, 1), 1))
    assert illum(t._h, P(d_dirs), 5, 13, P(out), np_t) == RC_ERR_NOT_SYNCED and grids(t._h, P(d_dirs), 5, 13, P(rays)) == RC_ERR_NOT_SYNCED
    t.sync()
    # transforms-dirty from the device, no refit yet
    d_xf = f32_tensor(dyn.frame_xf(rc, (2, 2, 1), 2))
    t.update_transforms_device(h, d_xf)
    assert illum(t._h, P(d_dirs), 5, 13, P(out), np_t) == RC_ERR_NOT_SYNCED and grids(t._h, P(d_dirs), 5, 13, P(rays)) == RC_ERR_NOT_SYNCED
    assert untouched()
    t.refit_device_async()
    assert illum(t._h, P(d_dirs), 5, 13, P(out), np_t) == 0 and grids(t._h, P(d_dirs), 5, 13, P(rays)) == 0
    torch.cuda.synchronize()
    t.wait_for_gpu()
    assert not (u32_of(rays) == POISON).any()
    t.free()


# ---- 8. the Python function ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["lds", "single"])
def test_get_illumination_dirs(rc, worlds, shape):
    w = worlds[shape]
    rows = rc.get_illumination_dirs(w.t, DIRS, 24)
    assert rows.dtype == np.float32 and rows.shape == (5, w.n)
    for d in range(5):
        assert np.array_equal(rows[d], rc.get_illumination(w.t, DIRS[d], 24)), d
    assert np.array_equal(rows, w.want(DIRS, 24).astype(np.float32))
    weights = np.array([0.5, 1.25, 3.0, 0.0, 2.0])
    got = rc.get_illumination_dirs(w.t, DIRS, 24, weights=weights)
    assert got.dtype == np.float64 and got.shape == (w.n,)
    assert np.array_equal(got, weights @ rows.astype(np.float64))
