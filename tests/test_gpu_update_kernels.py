"""Every trace kernel shape after every device-side update path.

tests/test_gpu_dynamic.py, test_gpu_rebuild.py and test_gpu_deform.py trace 65 536 rays with option `kernel` at -1, and the default
dispatch (rc_launch_trace) picks kernel 0 below 6 * 256 * n_cus * 5/4 rays: 491 520 on 256 CUs.  Kernels 0 and 1 read the traversal copy
from memory and never test an entry-cull sphere, so nothing in those files reads what the update paths derive for the kernels real
batches get -- the spheres and their copies in the TLAS leaf records, the per-BLAS cull radius, the renumbered tops and the prefixes
kernels 5 and 6 stage into LDS.  Here, with the scenes, frames, oracle caches and yardsticks of those three files:

1. THE MATRIX.  After every frame of update + refit (SMALL, LARGE), update + rebuild (the three PATHS) and geometry update + refit /
   + rebuild (Specs "144", "864", "top", "two") the camera rays are traced, closest and any, under SETTINGS: kernels 0 and 1, and
   (3, -), (5, stack16 1), (5, 0), (6, 1), (6, 0) under entry_cull 1, 0 and 2 (kernel 5 on more than 256 instances and kernel 6 with
   nothing to stage fall back to 3 by the launcher's own rules).  A frame is enqueued on one stream with no host wait inside it.  Every
   result is compared bit for bit with the yardstick the path's own file uses, and with the first setting's bytes.
   One batch large enough for the default dispatch to leave kernel 0 follows the last frame; four captured frames replay kernels 5
   and 6 under entry_cull 2.
2. THE DERIVED ARRAYS.  After every frame the entry-cull spheres (8 words per instance) and the whole traversal copy (BLAS slices and
   TLAS records) are read back and compared byte for byte with a scene that got there another way: the host twin after a refit, the fresh
   twin after a rebuild.  After a geometry update + REFIT in a frame whose from-scratch TLAS topology differs from the initial one
   (test_gpu_deform.py explains when) no twin has the refitted topology: the spheres, the BLAS slices and, instance by instance, the TLAS
   leaf records but for their parent word are compared; the interior TLAS records follow the kept topology and are covered by the node
   comparison of test_gpu_deform.py (refit_restatement).

A STALE SPHERE IS VISIBLE on these frames: test_stale_sphere_would_show (CPU only) evaluates, with tests/cull_model.py on the oracle's
data, how many of 4 096 rays that hit would be refused entry to the instance they hit had that instance kept its sphere of the previous
frame; at least 200 per frame.  The camera rays of the transform paths clear that by a wide margin (1 797 .. 4 084); the deformation
grows the sphere by less than the camera rays notice (0 .. 25 of 4 096 on the coarse sphere), so the geometry paths also trace, under
every setting, 4 096 rays aimed (grazing_rays of tests/test_gpu_entry_cull.py) at the faces that reach outside the previous frame's
sphere (338 .. 612).  Frame 1 of the coarse-sphere Specs is the exception, asserted as such (UNREACHABLE): the previous sphere still
holds the whole soup there, so a stale one changes no hit and no ray can show it.
"""
import numpy as np
import pytest

import cull_model as cm
import dynamic_kit as dyn
from gpu_kit import rc  # noqa: F401
from gpu_kit import read_device
from helpers import assert_hits_equal
from scene_kit import grazing_rays

LARGE, SMALL = dyn.LARGE, dyn.SMALL
N_FRAMES = 4
SHAPES = ((3, 1), (5, 1), (5, 0), (6, 1), (6, 0))                 # (kernel, stack16)
SETTINGS = [(0, 1, 1), (1, 1, 1)] + [(k, s16, cull) for cull in (1, 0, 2) for k, s16 in SHAPES]  # (kernel, stack16, entry_cull)
PLAN_OPTIONS = ("tlas_top_k", "blas_top_k", "debug_flat_tlas_off")  # ("stack16_in_use" follows the option `stack16`, which the matrix sets)
DEFORM_NAMES = ["144", "864", "top", "two"]
N_SAMPLE, N_AIMED, STALE_MIN = 4096, 4096, 200
INPUTS = [("refit", SMALL), ("refit", LARGE), ("rebuild", SMALL), ("rebuild", LARGE)] + [("deform", name) for name in DEFORM_NAMES]
INPUT_IDS = [f"{kind}-{key if isinstance(key, str) else int(np.prod(key))}" for kind, key in INPUTS]


@pytest.fixture(scope="module")
def rcm():
    """The package without a device: scenes, record types (the CPU-only condition)."""
    import raycore_jl_amd
    return raycore_jl_amd


# ---- the condition on the inputs, on the CPU alone ----------------------------------------------------------------------------------------
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def spec_of(rcm, name):
    return cached(("spec", name), lambda: dyn.Spec(rcm, name))


def oracle_state(oracle, rcm, kind, key, f):
    """-> (instances, BLAS descriptors, primitives) of the oracle built from scratch with frame f's inputs (f = -1: the initial ones)."""
    if kind == "deform":
        w = dyn.want_frame(oracle, rcm, spec_of(rcm, key), f)
        return w.instances, w.blas_descs, w.blas_prims

    def build():
        xf = dyn.initial_xf(rcm, key) if f < 0 else (dyn.frame_xf if kind == "refit" else dyn.rebuild_frame_xf)(rcm, key, f)
        o = oracle.Scene()
        b = o.add_blas(dyn.sphere(rcm))
        for i, x in enumerate(xf):
            o.add_instance(b, x, i)
        o.build()
        return o.instances, o.blas_descs, o.blas_prims
    return cached(("state", kind, key, f), build)


def oracle_closest(oracle, rcm, kind, key, f):
    """The cached closest hits of the path's own file on the scene's camera rays."""
    if kind == "refit":
        return dyn.oracle_frame(oracle, rcm, key, f)
    if kind == "rebuild":
        return dyn.rebuild_oracle_frame(oracle, rcm, key, f).closest
    return dyn.want_frame(oracle, rcm, spec_of(rcm, key), f).closest


def spheres_of(state):
    instances, descs, prims = state
    return cm.instance_spheres(instances, descs, cm.blas_radii(descs, prims))


def aimed_targets(oracle, rcm, name, f):
    """BLAS-local points on frame f's soup outside the sphere that held the soup of frame f - 1 (the previous root box's centre, the
    previous cull radius and 2 %): on every face with a vertex out there, a fifth of the way from its farthest vertex to its centroid.
    Empty only where NO ray can tell a stale sphere: every vertex of the frame lies within 1.01 x the previous radius, which the
    sphere's own radius exceeds (cull_model.instance_spheres: A = 1.01 r + positive terms), so a segment that misses the previous
    sphere misses the geometry too."""
    spec = spec_of(rcm, name)
    _, descs, prims = oracle_state(oracle, rcm, "deform", name, f - 1)
    centre, radius, _ = cm.blas_radii(descs, prims)[0]
    v = dyn.deform(spec.soups[0], f).astype(np.float64).reshape(-1, 3, 3)
    dist = np.linalg.norm(v - centre, axis=2)
    far = v[np.arange(len(v)), dist.argmax(axis=1)]
    points = 0.8 * far + 0.2 * v.mean(axis=1)
    points = points[np.linalg.norm(points - centre, axis=1) > 1.02 * radius]
    assert len(points) >= 8 or dist.max() <= 1.01 * radius, (name, f, len(points), dist.max(), radius)
    return points if len(points) >= 8 else points[:0]


def aimed_rays(oracle, rcm, name, f):
    """Geometry paths: N_AIMED rays of grazing_rays aimed at aimed_targets of frame f on instances spread over the scene (None: no targets)."""
    def build():
        spec = spec_of(rcm, name)
        targets = aimed_targets(oracle, rcm, name, f)
        if len(targets) == 0:
            return None
        inst = np.nonzero(spec.owner == 0)[0]
        n_points = N_AIMED // 8
        pick_i = inst[(np.arange(n_points) * 7919) % len(inst)]
        pick_f = targets[(np.arange(n_points) * 104729) % len(targets)]
        m = spec.xf[pick_i].astype(np.float64).reshape(-1, 3, 4)
        world = np.einsum("kij,kj->ki", m[:, :, :3], pick_f) + m[:, :, 3]
        rays = grazing_rays(rcm, world, np.full(n_points, 0.02), 4000 + f, per_instance=8)
        assert len(rays) == N_AIMED
        return rays
    return cached(("aimed", name, f), build)


# The coarse sphere's cull radius (the farthest corner of any triangle's own box: 0.693 for the 10 x 6 fan sphere of radius 0.5) already
# holds frame 1's soup, whose vertices reach 0.7 < 1.01 x 0.696: there a stale sphere changes no hit and no ray can show it.
UNREACHABLE = {("144", 1), ("864", 1), ("two", 1)}


def aimed_want(oracle, rcm, name, f):
    """The oracle from scratch on the aimed rays of frame f (closest and any)."""
    spec = spec_of(rcm, name)
    return cached(("aimed want", name, f), lambda: dyn.Want(oracle, spec.soups_of(f), spec.owner, spec.xf, aimed_rays(oracle, rcm, name, f)))


def stale_sphere_count(prev_spheres, rays, hits, ids):
    """How many of the rays `ids` (all hits) would be refused entry to the instance they hit, given THAT instance's sphere in prev_spheres
    (the segment test of the kernel, cull_model.skip_entry, with the ray's own t_max as the closest hit so far: the longest segment)."""
    count = 0
    for r in ids:
        assert hits["hit"][r] == 1
        i = int(hits["instance_custom_index"][r])  # the instances carry their index as custom index in all these scenes
        count += bool(cm.skip_entry(prev_spheres[i], rays["o"][r], rays["d"][r], rays["tmin"][r], rays["tmax"][r]))
    return count


def fixed_sample(rcm, hits, n, seed):
    ids = np.nonzero(hits["hit"] == 1)[0]
    return ids if len(ids) <= n else np.sort(rcm.scenes.rng(seed).choice(ids, n, replace=False))


@pytest.mark.parametrize("kind, key", INPUTS, ids=INPUT_IDS)
def test_stale_sphere_would_show(rcm, oracle, kind, key):
    """No GPU.  Frames 1 .. 3 of every path: of a fixed sample of N_SAMPLE traced rays that the oracle says hit, at least STALE_MIN hit an
    instance whose sphere of the PREVIOUS frame would have refused them entry.  Transform paths: the sample is drawn from the camera
    rays.  Geometry paths: the hits among the aimed rays first (at most half the sample), camera rays for the rest."""
    rays = dyn.camera_rays(rcm, key) if kind != "deform" else spec_of(rcm, key).rays
    for f in range(1, N_FRAMES):
        prev, now = spheres_of(oracle_state(oracle, rcm, kind, key, f - 1)), spheres_of(oracle_state(oracle, rcm, kind, key, f))
        hits = oracle_closest(oracle, rcm, kind, key, f)
        n_aimed = 0
        extra = aimed_rays(oracle, rcm, key, f) if kind == "deform" else None
        assert (extra is None) == (kind != "deform" or (key, f) in UNREACHABLE), (kind, key, f)
        stale = 0
        if extra is not None:
            want = aimed_want(oracle, rcm, key, f).closest
            ids = fixed_sample(rcm, want, N_SAMPLE // 2, 4096)
            n_aimed = len(ids)
            stale = stale_sphere_count(prev, extra, want, ids)
            assert stale_sphere_count(now, extra, want, ids) == 0  # (the frame's own spheres refuse no ray that hits)
        ids = fixed_sample(rcm, hits, N_SAMPLE - n_aimed, 4096)
        assert n_aimed + len(ids) == N_SAMPLE
        stale += stale_sphere_count(prev, rays, hits, ids)
        assert stale_sphere_count(now, rays, hits, ids[::8]) == 0
        print(f"inputs {kind} {key} frame {f}: {stale} of {N_SAMPLE} hits ({n_aimed} of them aimed) would be refused entry by the previous frame's sphere")
        assert stale >= STALE_MIN or (key, f) in UNREACHABLE, (kind, key, f, stale)


# ---- the matrix ---------------------------------------------------------------------------------------------------------------------------
class Batch:
    """One ray batch on the device with a closest and an any buffer per setting."""

    def __init__(self, torch, rays, stream, n_settings=len(SETTINGS)):
        self.torch, self.rays, self.n = torch, rays, len(rays)
        self.d_rays = dyn.dev_bytes(torch, rays)
        self.out = torch.zeros((n_settings, 2, self.n * 32), dtype=torch.uint8, device="cuda")
        for buf in (self.d_rays, self.out):
            buf.record_stream(stream)

    def load(self, rays):
        """Other rays of the same count (the host wait lies between two frames)."""
        assert len(rays) == self.n
        self.rays = rays
        self.d_rays.copy_(dyn.dev_bytes(self.torch, rays))
        self.torch.cuda.synchronize()

    def enqueue(self, t, k, st):
        t.trace_device(self.d_rays.data_ptr(), self.out[k, 0].data_ptr(), self.n, stream=st)
        t.trace_device(self.d_rays.data_ptr(), self.out[k, 1].data_ptr(), self.n, mode="any", stream=st)

    def results(self, rc):
        host = self.out.cpu().numpy()
        return [(host[k, 0].view(rc.HIT_DT), host[k, 1].view(rc.HIT_DT)) for k in range(host.shape[0])]


def set_shape(t, kernel, s16, cull):
    t.set_option("kernel", kernel)
    t.set_option("stack16", s16)
    t.set_option("entry_cull", cull)


def enqueue_matrix(t, batches, s):
    """Every setting on every batch, behind whatever the stream holds: options are host-side words, nothing waits."""
    with batches[0].torch.cuda.stream(s):
        for b in batches:
            b.out.zero_()
    for k, (kernel, s16, cull) in enumerate(SETTINGS):
        set_shape(t, kernel, s16, cull)
        for b in batches:
            b.enqueue(t, k, s.cuda_stream)
    set_shape(t, -1, 1, 1)


def check_matrix(rc, batch, want_c, want_a, what, any_records=True):
    """Every setting against the yardstick (any_records=False: the any hits on their `hit` word, the records follow a topology no yardstick
    has) and against the first setting's bytes."""
    first = None
    for (kernel, s16, cull), (got_c, got_a) in zip(SETTINGS, batch.results(rc)):
        w = f"{what}, kernel {kernel}, stack16 {s16}, entry_cull {cull}"
        assert_hits_equal(got_c, want_c, f"{w}: closest")
        if any_records:
            assert_hits_equal(got_a, want_a, f"{w}: any")
        else:
            assert np.array_equal(got_a["hit"], want_a["hit"]), f"{w}: any-hit occlusion"
        if first is None:
            first = (got_c.tobytes(), got_a.tobytes())
        assert got_c.tobytes() == first[0], f"{w}: closest hits differ from the first setting's"
        assert got_a.tobytes() == first[1], f"{w}: any hits differ from the first setting's"
    return first


# ---- the derived arrays -------------------------------------------------------------------------------------------------------------------
def derived_arrays(t, n):
    """-> (spheres (n, 8), traversal copy (tlas_off + 2n - 1, 16), tlas_off, plan options), read back from the device."""
    off = t.get_option("debug_flat_tlas_off")
    cull = read_device(t.get_option("debug_inst_cull_ptr"), np.uint32, 8 * n).reshape(n, 8)
    rec = read_device(t.get_option("debug_flat_nodes_ptr"), np.uint32, 16 * (off + 2 * n - 1)).reshape(-1, 16)
    return cull, rec, off, {name: t.get_option(name) for name in PLAN_OPTIONS}


def assert_same_derived(t, yard, n, what, same_topology=True):
    cull, rec, off, plan = derived_arrays(t, n)
    ycull, yrec, yoff, yplan = derived_arrays(yard, n)
    assert plan == yplan, f"{what}: plan {plan} != {yplan}"
    bad = np.nonzero(np.any(cull != ycull, axis=1))[0]
    assert len(bad) == 0, f"{what}: the spheres of {len(bad)} instances differ, first: instance {bad[:3]} {cull[bad[:3]]} != {ycull[bad[:3]]}"
    if same_topology:
        bad = np.nonzero(np.any(rec != yrec, axis=1))[0]
        assert len(bad) == 0, f"{what}: {len(bad)} records of the traversal copy differ (TLAS from {off}), first: {bad[:3]} {rec[bad[:3]]} != {yrec[bad[:3]]}"
        return
    # a refit keeps the topology of the last sync, the yardstick was sorted anew: the BLAS slices in full, the TLAS leaves by instance
    # without dword 14 (the parent's index: topology); the interior TLAS records are the topology's
    bad = np.nonzero(np.any(rec[:off] != yrec[:off], axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} BLAS records of the traversal copy differ, first: {bad[:3]}"
    leaves, yleaves = rec[off + n - 1:], yrec[off + n - 1:]
    for lv in (leaves, yleaves):
        assert np.array_equal(np.sort(lv[:, 13]), np.arange(n)), f"{what}: the leaves do not name every instance once"
    a, b = leaves[np.argsort(leaves[:, 13])], yleaves[np.argsort(yleaves[:, 13])]
    cols = [c for c in range(16) if c != 14]
    bad = np.nonzero(np.any(a[:, cols] != b[:, cols], axis=1))[0]
    assert len(bad) == 0, f"{what}: the leaf records of {len(bad)} instances differ, first: instance {bad[:3]} {a[bad[:3]]} != {b[bad[:3]]}"


# ---- one batch through the default dispatch -------------------------------------------------------------------------------------------------
def default_dispatch_side(t):
    """Side of a square camera whose ray count leaves kernel 0 under option kernel = -1 (rc_launch_trace: n >= 6 * 256 * n_cus * 5/4)."""
    need = 6 * 256 * t.get_option("n_cus") * 5 // 4 + 256
    side = max(768, -(-int(np.ceil(np.sqrt(need))) // 64) * 64)
    assert side * side >= need, (side, need)
    return side


def big_camera_rays(rcm, dims, side):
    """camera_rays of tests/test_gpu_dynamic.py at side x side."""
    ext = (np.array(dims, dtype=np.float64) - 1) * 1.8
    centre = ext / 2
    eye = centre + np.array([0.45, 0.3, 1.0]) * (0.95 * ext[:2].max() + 3.0)
    return rcm.scenes.pinhole_rays(side, side, eye, centre, fov_deg=45.0)


def check_default_dispatch(rc, t, s, rays, want_c, want_a, what, any_records=True):
    import torch
    assert t.get_option("kernel") == -1 and len(rays) >= 6 * 256 * t.get_option("n_cus") * 5 // 4 + 256
    b = Batch(torch, rays, s, n_settings=1)
    torch.cuda.synchronize()
    b.enqueue(t, 0, s.cuda_stream)
    s.synchronize()
    (got_c, got_a), = b.results(rc)
    assert_hits_equal(got_c, want_c, f"{what}: {len(rays)} rays through the default dispatch, closest")
    if any_records:
        assert_hits_equal(got_a, want_a, f"{what}: {len(rays)} rays through the default dispatch, any")
    else:
        assert np.array_equal(got_a["hit"], want_a["hit"]), f"{what}: {len(rays)} rays through the default dispatch, any-hit occlusion"
    assert 0.2 < want_c["hit"].mean() < 0.98
    return got_c, got_a


# ---- 1. update + refit_device_async ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dims", [SMALL, LARGE], ids=["144", "864"])
def test_matrix_after_refit(rc, oracle, dims):
    import torch
    t, (h,), cuts = dyn.make_scene(rc, dims)
    twin, th, _ = dyn.make_scene(rc, dims)
    rays = dyn.camera_rays(rc, dims)
    s = torch.cuda.Stream()
    frames = [torch.from_numpy(dyn.frame_xf(rc, dims, f)).cuda() for f in range(N_FRAMES)]
    d_xf = torch.empty_like(frames[0])
    batch = Batch(torch, rays, s)
    for buf in (d_xf, *frames):
        buf.record_stream(s)
    torch.cuda.synchronize()
    for f in range(N_FRAMES):
        want = dyn.oracle_frame(oracle, rc, dims, f)
        dyn.host_frame(twin, th, cuts, dyn.frame_xf(rc, dims, f))
        with torch.cuda.stream(s):
            d_xf.copy_(frames[f])
        t.update_transforms_device(h, d_xf, stream=s.cuda_stream)
        t.refit_device_async(stream=s.cuda_stream)
        enqueue_matrix(t, [batch], s)
        s.synchronize()
        twin_c, twin_a = twin.trace(rays), twin.trace(rays, mode="any")  # (the host twin has the refitted topology: any records and all)
        assert_hits_equal(twin_c, want, f"refit {dims} frame {f}: the host twin vs oracle")
        first = check_matrix(rc, batch, want, twin_a, f"refit {dims} frame {f}")
        assert first == (twin_c.tobytes(), twin_a.tobytes()), f"refit {dims} frame {f}: hits differ from the host twin's"
        assert_same_derived(t, twin, cuts[-1], f"refit {dims} frame {f}")
    side = default_dispatch_side(t)
    big = big_camera_rays(rc, dims, side)
    xf = dyn.frame_xf(rc, dims, N_FRAMES - 1)
    want_c = cached(("big", "refit", dims, side), lambda: dyn.oracle_scene_hits(oracle, rc, xf, big))
    got_c, got_a = check_default_dispatch(rc, t, s, big, want_c, cached(("big any", "refit", dims, side), lambda: dyn.oracle_scene_hits(oracle, rc, xf, big, mode="any")),
                                          f"refit {dims}", any_records=False)
    assert (got_c.tobytes(), got_a.tobytes()) == (twin.trace(big).tobytes(), twin.trace(big, mode="any").tobytes()), "the large batch differs from the host twin's"


# ---- 2. update + rebuild_device_async -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dims, fused", dyn.PATHS, ids=dyn.PATH_IDS)
def test_matrix_after_rebuild(rc, oracle, dims, fused):
    import torch
    a = dyn.Frames(rc, dims, fused)
    batch = Batch(torch, a.rays, a.s)
    torch.cuda.synchronize()
    n_inst = len(a.frames[0])
    for f in range(N_FRAMES):
        want = dyn.rebuild_oracle_frame(oracle, rc, dims, f)
        twin = dyn.fresh_twin(rc, dyn.rebuild_frame_xf(rc, dims, f))
        with torch.cuda.stream(a.s):
            a.d_xf.copy_(a.frames[f])
        a.t.update_transforms_device(a.h, a.d_xf, stream=a.s.cuda_stream)
        a.t.rebuild_device_async(stream=a.s.cuda_stream)
        enqueue_matrix(a.t, [batch], a.s)
        a.s.synchronize()
        what = f"rebuild {dyn.PATH_IDS[dyn.PATHS.index((dims, fused))]} frame {f}"
        first = check_matrix(rc, batch, want.closest, want.any, what)
        assert first == (twin.trace(a.rays).tobytes(), twin.trace(a.rays, mode="any").tobytes()), f"{what}: hits differ from the fresh twin's"
        assert_same_derived(a.t, twin, n_inst, what)
    side = default_dispatch_side(a.t)
    big = big_camera_rays(rc, dims, side)
    w = cached(("big", "rebuild", dims, side), lambda: dyn.OracleFrame(oracle, rc, dyn.rebuild_frame_xf(rc, dims, N_FRAMES - 1), big))
    check_default_dispatch(rc, a.t, a.s, big, w.closest, w.any, f"rebuild {dims} fused {fused}")


# ---- 3. update_geometry_device_async + refit / rebuild --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("commit", ["refit", "rebuild"])
@pytest.mark.parametrize("name", DEFORM_NAMES)
def test_matrix_after_geometry_update(rc, oracle, name, commit):
    import torch
    spec = spec_of(rc, name)
    t, hs = spec.build(rc)
    n_inst = len(spec.xf)
    first_want = dyn.want_frame(oracle, rc, spec, -1)
    s = torch.cuda.Stream()
    camera = Batch(torch, spec.rays, s)
    aimed = Batch(torch, aimed_rays(oracle, rc, name, 2), s)
    soups = [torch.from_numpy(dyn.deform(spec.soups[0], f)).cuda() for f in range(N_FRAMES)]
    d_soup = torch.empty_like(soups[0])
    for buf in (d_soup, *soups):
        buf.record_stream(s)
    torch.cuda.synchronize()
    commit_fn = t.refit_device_async if commit == "refit" else t.rebuild_device_async
    as_fresh = True
    for f in range(N_FRAMES):
        want = dyn.want_frame(oracle, rc, spec, f)
        twin, _ = spec.build(rc, f)
        batches = [camera]
        extra = aimed_rays(oracle, rc, name, f) if f >= 1 else None  # (None also where no ray can tell a stale sphere: UNREACHABLE)
        if extra is not None:
            aimed.load(extra)
            batches.append(aimed)
        with torch.cuda.stream(s):
            d_soup.copy_(soups[f])
        t.update_geometry_device_async(hs[-1], d_soup, stream=s.cuda_stream)
        commit_fn(stream=s.cuda_stream)
        enqueue_matrix(t, batches, s)
        s.synchronize()
        t.wait_for_gpu()  # (no status pending)
        as_fresh = commit == "rebuild" or want.same_topology(first_want)  # after a refit: test_gpu_deform.py, the module's docstring
        what = f"{name} {commit} frame {f}"
        first = check_matrix(rc, camera, want.closest, want.any, what, any_records=as_fresh)
        assert first[0] == twin.trace(spec.rays).tobytes(), f"{what}: closest hits differ from the fresh twin's"
        if as_fresh:
            assert first[1] == twin.trace(spec.rays, mode="any").tobytes(), f"{what}: any hits differ from the fresh twin's"
        if extra is not None:
            w = aimed_want(oracle, rc, name, f)
            assert w.closest["hit"].mean() > 0.1
            check_matrix(rc, aimed, w.closest, w.any, f"{what}, aimed rays", any_records=as_fresh)
        assert_same_derived(t, twin, n_inst, what, same_topology=as_fresh)
    side = default_dispatch_side(t)
    big = big_camera_rays(rc, spec.dims, side)
    w = cached(("big", "deform", name, side), lambda: dyn.Want(oracle, spec.soups_of(N_FRAMES - 1), spec.owner, spec.xf, big))
    check_default_dispatch(rc, t, s, big, w.closest, w.any, f"{name} {commit}", any_records=as_fresh)
    if name == "144":  # the cull does spare entries on these rays (the counters of the stats kernel): the matrix did read the spheres
        set_shape(t, 5, 1, 1)
        t.set_option("stats", 1)
        t.trace(spec.rays)
        assert t.get_option("stat19") > 0
        t.set_option("stats", 0)
        set_shape(t, -1, 1, 1)


# ---- 4. captured frames: update -> commit -> closest -> any as one graph, kernels 5 and 6 under entry_cull 2 -------------------------------
CAPTURED = [("refit", SMALL, 5, 1), ("rebuild", SMALL, 5, 0), ("rebuild", LARGE, 6, 1), ("refit", LARGE, 6, 0), ("deform", "top", 6, 1), ("deform", "top", 6, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind, key, kernel, s16", CAPTURED, ids=[f"{k}-{key if isinstance(key, str) else int(np.prod(key))}-k{kn}-s{s}" for k, key, kn, s in CAPTURED])
def test_captured_frames(rc, oracle, kind, key, kernel, s16):
    """One graph per case, options set before the capture, replayed once per frame with that frame's buffers.  ("deform": geometry update
    + rebuild.)"""
    import torch
    s = torch.cuda.Stream()
    if kind == "deform":
        spec = spec_of(rc, key)
        t, hs = spec.build(rc)
        h, rays, n_inst = hs[-1], spec.rays, len(spec.xf)
        src = [torch.from_numpy(dyn.deform(spec.soups[0], f)).cuda() for f in range(N_FRAMES)]
        assert 0 < t.get_option("blas_top_k")
    else:
        t, (h,), cuts = dyn.make_scene(rc, key)
        twin, th, _ = dyn.make_scene(rc, key)
        rays, n_inst = dyn.camera_rays(rc, key), cuts[-1]
        src = [torch.from_numpy((dyn.frame_xf if kind == "refit" else dyn.rebuild_frame_xf)(rc, key, f)).cuda() for f in range(N_FRAMES)]
    d_src = src[0].clone()
    batch = Batch(torch, rays, s, n_settings=1)
    for buf in (d_src, *src):
        buf.record_stream(s)
    torch.cuda.synchronize()
    set_shape(t, kernel, s16, 2)

    def frame(st):
        if kind == "deform":
            t.update_geometry_device_async(h, d_src, stream=st)
        else:
            t.update_transforms_device(h, d_src, stream=st)
        (t.refit_device_async if kind == "refit" else t.rebuild_device_async)(stream=st)
        batch.enqueue(t, 0, st)

    with torch.cuda.stream(s):
        frame(s.cuda_stream)  # eager first
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        frame(torch.cuda.current_stream().cuda_stream)
    assert t.get_option("release_captures") == 2  # the two traces
    for f in (1, 2, 3, 0):
        batch.out.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            d_src.copy_(src[f])  # in place: the graph reads the tensor when it runs
            g.replay()
        s.synchronize()
        (got_c, got_a), = batch.results(rc)
        what = f"{kind} {key} kernel {kernel} stack16 {s16}: replay of frame {f}"
        if kind == "refit":
            dyn.host_frame(twin, th, cuts, dyn.frame_xf(rc, key, f))
            assert_hits_equal(got_c, dyn.oracle_frame(oracle, rc, key, f), f"{what}: closest vs oracle")
            assert (got_c.tobytes(), got_a.tobytes()) == (twin.trace(rays).tobytes(), twin.trace(rays, mode="any").tobytes()), f"{what}: hits differ from the host twin's"
        else:
            want = dyn.rebuild_oracle_frame(oracle, rc, key, f) if kind == "rebuild" else dyn.want_frame(oracle, rc, spec, f)
            twin = dyn.fresh_twin(rc, dyn.rebuild_frame_xf(rc, key, f)) if kind == "rebuild" else spec.build(rc, f)[0]
            assert_hits_equal(got_c, want.closest, f"{what}: closest vs oracle")
            assert_hits_equal(got_a, want.any, f"{what}: any vs oracle")
        assert_same_derived(t, twin, n_inst, what)
    if kind == "deform":
        t.wait_for_gpu()
    del g
    t.set_option("release_captures", 1)
    assert t.get_option("release_captures") == 0
    set_shape(t, -1, 1, 1)
