"""Device-side TLAS rebuild: rebuild_device_async (rc_rebuild_tlas_device_async) on the GPU, both device paths (the single-workgroup
kernel for scenes of at most 256 instances, option tlas_rebuild_fused = 1, and the chain of build kernels, = 0 or any larger scene).

Two yardsticks, neither of them the code under test:

* the ORACLE FROM SCRATCH: oracle.pyoracle.Scene built anew with the frame's transforms.  A rebuild re-sorts, and so does the oracle, so
  everything is compared: TLAS nodes, instances and world bound byte for byte, closest and any hits bit for bit, exact ties included;
* a FRESH TWIN: a new rc.TLAS() with the same pushes and the frame's transforms, synced structurally (last_sync_action == "rebuild") -- the
  synchronous path that existed before.  Same byte-for-byte comparisons (assert_same_scene of tests/test_gpu_dynamic.py).

Scene and camera are those of tests/test_gpu_dynamic.py.  Frame f: lattice_transforms(*dims, 1.5 + 0.2 f, 100 + 7 f), a non-uniform scale
at f == 2, the translation column permuted among the instances by Philox(key = 900 + f); at f == 3 instances 1 and n - 1 are exact copies
of instance 0 (equal Morton codes, coincident triangles: the sort's stability and the tie order are pinned).  Conditions on the inputs,
asserted on the oracle's output alone (oracle_frame): >= 0.9 of the TLAS leaf slots hold another instance than in the previous frame's
tree, hit fraction >= 0.2, >= 0.1 of the hit records differ from the previous frame's -- a rebuild that silently refits, or leaves the
instance -> leaf table stale, cannot pass.

WHICH KERNEL RUNS HERE: kernel 0 (option `kernel` at -1, 65 536 rays: test_gpu_dynamic.py's docstring has the arithmetic), which reads
neither the entry-cull spheres nor the renumbered top of the TLAS.  The exported TLAS nodes pin the topology; the renumbering, the
spheres in the rebuilt leaf records and kernels 3, 5 and 6 on the rebuilt tree are checked in tests/test_gpu_update_kernels.py.
"""
import numpy as np
import pytest

from dynamic_kit import Frames, LARGE, N_FRAMES, OracleFrame, PATHS, PATH_IDS, SMALL, TIE_FRAME, assert_same_scene, camera_rays, dev_bytes, fresh_twin
from dynamic_kit import hits_of, initial_xf, make_scene, rebuild_frame_xf as frame_xf, rebuild_oracle_frame as oracle_frame, sphere
from gpu_kit import rc  # noqa: F401
from helpers import assert_hits_equal

pytestmark = pytest.mark.gpu

RC_ERR_INVALID_ARGUMENT, RC_ERR_NOT_SYNCED = 1, 6


def assert_scene_is_oracle(t, want, what):
    st = t.adapt()
    assert st.nodes.tobytes() == want.nodes.tobytes(), f"{what}: TLAS nodes differ from the oracle built from scratch"
    assert st.instances.tobytes() == want.instances.tobytes(), f"{what}: instances differ from the oracle's"
    b = t.world_bound()
    assert np.concatenate([b.p_min, b.p_max]).tobytes() == want.bound.tobytes(), f"{what}: world bound"


def check_frame(rc, t, want, twin, rays, got, got_any, what):
    """Hits, lazily refreshed bound, no-op sync, nodes and instances against both yardsticks."""
    assert_hits_equal(got, want.closest, f"{what}: closest vs oracle")
    assert_hits_equal(got_any, want.any, f"{what}: any vs oracle")
    assert got.tobytes() == twin.trace(rays).tobytes(), f"{what}: closest hits differ from the fresh twin"
    assert got_any.tobytes() == twin.trace(rays, mode="any").tobytes(), f"{what}: any hits differ from the fresh twin"
    assert t.sync().last_sync_action == "noop", what  # the asynchronous rebuild left nothing pending
    assert_scene_is_oracle(t, want, what)
    assert_same_scene(t, twin, what)


# ---- 1. copy -> update -> rebuild -> trace on one stream, no host synchronisation between them -------------------------------------------
@pytest.mark.parametrize("dims, fused", PATHS, ids=PATH_IDS)
def test_eager_update_rebuild_trace(rc, oracle, dims, fused):
    import torch
    a = Frames(rc, dims, fused)
    for f in range(N_FRAMES):
        want = oracle_frame(oracle, rc, dims, f)
        twin = fresh_twin(rc, frame_xf(rc, dims, f))
        with torch.cuda.stream(a.s):
            a.d_xf.copy_(a.frames[f])  # the transforms are produced on the stream too
            a.t.update_transforms_device(a.h, a.d_xf, stream=a.s.cuda_stream)
            a.t.rebuild_device_async(stream=a.s.cuda_stream)
            a.trace(a.s.cuda_stream)
        bound = a.t.world_bound()  # the lazy refresh: waits for the rebuild, reads the root back
        assert np.concatenate([bound.p_min, bound.p_max]).tobytes() == want.bound.tobytes(), f"frame {f}: lazy world bound"
        a.s.synchronize()
        got, got_any = a.hits()
        check_frame(rc, a.t, want, twin, a.rays, got, got_any, f"frame {f}")
        assert np.array_equal(a.t.get_instances(a.h)["transform"], frame_xf(rc, dims, f))  # lazy mirror refresh
        if f == TIE_FRAME:  # rays aimed at the three coincident instances from all sides: every hit there is an exact three-way tie
            c = frame_xf(rc, dims, f)[0, [3, 7, 11]].astype(np.float64)
            d = rc.scenes.normalize(rc.scenes.rng(5).normal(size=(512, 3)))
            aimed = rc.scenes.make_rays(c - 3.0 * d + rc.scenes.rng(6).uniform(-0.2, 0.2, size=(512, 3)), d)
            ties = OracleFrame(oracle, rc, frame_xf(rc, dims, f), aimed)
            on_tie = np.isin(ties.closest["instance_id"][ties.closest["hit"] == 1], [0, 1, len(a.frames[0]) - 1])
            assert on_tie.sum() >= 50, int(on_tie.sum())
            assert_hits_equal(a.t.trace(aimed), ties.closest, "aimed at the coincident instances: closest")
            assert_hits_equal(a.t.trace(aimed, mode="any"), ties.any, "aimed at the coincident instances: any")


# ---- 2. a refit after a rebuild walks the new topology -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dims, fused", PATHS, ids=PATH_IDS)
def test_refit_after_rebuild_uses_the_new_topology(rc, oracle, dims, fused):
    import torch
    a = Frames(rc, dims, fused)
    oracle_frame(oracle, rc, dims, 0)
    want1 = oracle_frame(oracle, rc, dims, 1)  # generic rotations, no coincident instances: no exact ties
    ths = []
    twin = fresh_twin(rc, frame_xf(rc, dims, 0), handles=ths)
    th = ths[0]
    with torch.cuda.stream(a.s):
        a.d_xf.copy_(a.frames[0])
        a.t.update_transforms_device(a.h, a.d_xf, stream=a.s.cuda_stream)
        a.t.rebuild_device_async(stream=a.s.cuda_stream)
        a.d_xf.copy_(a.frames[1])
        a.t.update_transforms_device(a.h, a.d_xf, stream=a.s.cuda_stream)  # scatters through the REBUILT instance -> leaf table
        a.t.refit_device_async(stream=a.s.cuda_stream)
        a.trace(a.s.cuda_stream)
    a.s.synchronize()
    twin.update_transforms(th, frame_xf(rc, dims, 1))
    assert twin.sync().last_sync_action == "refit"
    got, got_any = a.hits()
    assert got.tobytes() == twin.trace(a.rays).tobytes(), "closest hits differ from the twin rebuilt at frame 0 and refitted to frame 1"
    assert got_any.tobytes() == twin.trace(a.rays, mode="any").tobytes()
    assert_hits_equal(got, want1.closest, "refit on the rebuilt topology vs oracle")
    assert_same_scene(a.t, twin, "refit after rebuild")
    # the refitted tree keeps frame 0's order: it is NOT the tree a rebuild at frame 1 gives
    assert a.t.adapt().nodes.tobytes() != want1.nodes.tobytes()
    # ... and a host-side update + sync refits on the new topology as well
    a.t.update_transforms(a.h, frame_xf(rc, dims, 2))
    twin.update_transforms(th, frame_xf(rc, dims, 2))
    assert a.t.sync().last_sync_action == "refit" and twin.sync().last_sync_action == "refit"
    assert_same_scene(a.t, twin, "host refit after rebuild")
    assert_hits_equal(a.t.trace(a.rays), oracle_frame(oracle, rc, dims, 2).closest, "host refit after rebuild vs oracle")


# ---- 3. update -> rebuild -> trace closest -> trace any as one graph, replayed once per frame -------------------------------------------
@pytest.mark.parametrize("dims, fused", PATHS, ids=PATH_IDS)
def test_graph_replay_per_frame(rc, oracle, dims, fused):
    import torch
    a = Frames(rc, dims, fused)

    def frame(st):
        a.t.update_transforms_device(a.h, a.d_xf, stream=st)
        a.t.rebuild_device_async(stream=st)
        a.trace(st)

    with torch.cuda.stream(a.s):
        frame(a.s.cuda_stream)  # eager first
    a.s.synchronize()
    assert_hits_equal(a.hits()[0], oracle_frame(oracle, rc, dims, 0).closest, "eager frame")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=a.s):
        frame(torch.cuda.current_stream().cuda_stream)
    assert a.t.get_option("release_captures") == 2  # the two traces; update and rebuild hold no capture slot
    for f in list(range(1, N_FRAMES)) + [0]:
        want = oracle_frame(oracle, rc, dims, f)
        twin = fresh_twin(rc, frame_xf(rc, dims, f))
        a.d_hits.zero_(); a.d_any.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(a.s):
            a.d_xf.copy_(a.frames[f])  # in place: the graph reads the tensor when it runs
            g.replay()
        a.s.synchronize()
        got, got_any = a.hits()
        check_frame(rc, a.t, want, twin, a.rays, got, got_any, f"replay of frame {f}")
    del g
    a.t.set_option("release_captures", 1)
    assert a.t.get_option("release_captures") == 0
    assert_hits_equal(a.t.trace(a.rays), oracle_frame(oracle, rc, dims, 0).closest, "after the graph is gone")


# ---- 4. a graph captured BEFORE the rebuild keeps working after it (the structural sync would have killed it) --------------------------------
@pytest.mark.parametrize("dims, fused", PATHS, ids=PATH_IDS)
def test_earlier_captures_survive(rc, oracle, dims, fused):
    import torch
    a = Frames(rc, dims, fused)
    for f in range(3):
        oracle_frame(oracle, rc, dims, f)

    def refit_frame(st):
        a.t.update_transforms_device(a.h, a.d_xf, stream=st)
        a.t.refit_device_async(stream=st)
        a.trace(st)

    with torch.cuda.stream(a.s):
        refit_frame(a.s.cuda_stream)
    a.s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=a.s):
        refit_frame(torch.cuda.current_stream().cuda_stream)
    with torch.cuda.stream(a.s):
        a.d_xf.copy_(a.frames[1])
        g.replay()                                             # frame 1 on the topology of the initial sync
        a.t.rebuild_device_async(stream=a.s.cuda_stream)       # eager, same stream: frame 1's own topology (from the descriptors)
        a.trace(a.s.cuda_stream)
    a.s.synchronize()
    ths = []
    twin = fresh_twin(rc, frame_xf(rc, dims, 1), handles=ths)
    got, got_any = a.hits()
    check_frame(rc, a.t, oracle_frame(oracle, rc, dims, 1), twin, a.rays, got, got_any, "eager rebuild between replays")
    assert a.t.get_option("release_captures") == 2  # the old graph's launches are still held: nothing was invalidated
    a.d_hits.zero_(); a.d_any.zero_()
    torch.cuda.synchronize()
    with torch.cuda.stream(a.s):
        a.d_xf.copy_(a.frames[2])
        g.replay()                                             # the OLD graph: update + refit + traces, now on frame 1's topology
    a.s.synchronize()
    twin.update_transforms(ths[0], frame_xf(rc, dims, 2))
    assert twin.sync().last_sync_action == "refit"
    got, got_any = a.hits()
    assert int(got["hit"].sum()) > 0.2 * len(got)
    assert got.tobytes() == twin.trace(a.rays).tobytes(), "replay after the rebuild: closest hits differ from the twin that followed the same sequence"
    assert got_any.tobytes() == twin.trace(a.rays, mode="any").tobytes(), "replay after the rebuild: any hits"
    assert_hits_equal(got, oracle_frame(oracle, rc, dims, 2).closest, "replay after the rebuild vs oracle")  # (frame 2 has no exact ties)
    assert_same_scene(a.t, twin, "replay after the rebuild")
    del g
    a.t.set_option("release_captures", 1)


# ---- 5. WavefrontPaths(dynamic=..., rebuild=True) -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
def test_wavefront_rebuild_frame(rc, oracle, fused):
    import torch
    from raycore_jl_amd.wavefront import WavefrontPaths, lookat_camera
    dims = SMALL
    t, (h,), _ = make_scene(rc, dims)
    t.set_option("tlas_rebuild_fused", fused)
    for f in range(N_FRAMES):
        oracle_frame(oracle, rc, dims, f)  # (the frames' inputs are the ones checked above)
    ext = (np.array(dims, dtype=np.float64) - 1) * 1.8
    cam = lookat_camera(ext / 2 + np.array([0.45, 0.3, 1.0]) * (0.95 * ext[:2].max() + 3.0), ext / 2, 64, 48)
    light = np.array([ext[0] / 2, ext[1] + 8.0, ext[2] + 6.0], dtype=np.float32)
    frames = [torch.from_numpy(frame_xf(rc, dims, f)).cuda() for f in range(N_FRAMES)]
    d_xf = frames[0].clone()
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        WavefrontPaths(t, 64, 48, 2, 2, cam, light, seed=11, rebuild=True)
    dyn = WavefrontPaths(t, 64, 48, 2, 2, cam, light, seed=11, dynamic=[(h, d_xf)], rebuild=True)
    assert WavefrontPaths(t, 8, 8, 1, 1, cam, light, dynamic=[(h, d_xf)]).rebuild is False
    s = torch.cuda.Stream()

    def compare(f, what):
        """The same frame, static, on a scene built from scratch with the frame's transforms."""
        torch.cuda.synchronize()
        twin = fresh_twin(rc, frame_xf(rc, dims, f))
        ref = WavefrontPaths(twin, 64, 48, 2, 2, cam, light, seed=11)
        ref.run(s)
        torch.cuda.synchronize()
        alive = 0
        for b in range(2):
            for name in ("rays", "hits", "shadow_hits", "path_ids"):
                x, y = getattr(dyn, name)[b], getattr(ref, name)[b]
                assert torch.equal(x, y), f"{what}: {name}[{b}] differs from the static frame on a scene built from scratch"
            alive += int(np.count_nonzero(hits_of(rc, dyn.hits[b])["hit"]))
        assert alive > 0.1 * dyn.n, what
        assert t.adapt().nodes.tobytes() == oracle_frame(oracle, rc, dims, f).nodes.tobytes(), f"{what}: TLAS nodes vs oracle"

    for f in range(N_FRAMES):  # eager
        with torch.cuda.stream(s):
            d_xf.copy_(frames[f])
            dyn.run(s)
        compare(f, f"eager frame {f}")
    dyn.capture(s)
    for f in (1, 3, 0):  # replayed
        for buf in dyn.hits + dyn.shadow_hits:
            buf.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            d_xf.copy_(frames[f])
            dyn.replay()
        compare(f, f"replayed frame {f}")
    dyn.graph = None
    torch.cuda.synchronize()
    t.set_option("release_captures", 1)


# ---- 6. descriptors rewritten through instance_buffer, no update call --------------------------------------------------------------------
@pytest.mark.parametrize("dims, fused", PATHS, ids=PATH_IDS)
def test_descriptor_path(rc, oracle, dims, fused):
    import torch
    a = Frames(rc, dims, fused)
    n_inst = len(a.frames[0])
    ptr, cnt = a.t.instance_buffer(a.h)
    assert cnt == n_inst

    class Alias:
        __cuda_array_interface__ = {"shape": (n_inst, 27), "typestr": "<f4", "data": (ptr, False), "version": 2}

    recs = torch.as_tensor(Alias(), device="cuda")
    for f in (TIE_FRAME, 1):
        want = oracle_frame(oracle, rc, dims, f)
        twin = fresh_twin(rc, frame_xf(rc, dims, f))
        recs[:, 2:14] = a.frames[f]
        recs[:, 14:26] = torch.from_numpy(want.instances["inv_transform"].copy()).cuda()  # the inverses are the caller's on this path
        torch.cuda.synchronize()
        a.t.rebuild_device_async(stream=a.s.cuda_stream)  # no update call since the last refit / rebuild: the per-instance pass runs
        a.trace(a.s.cuda_stream)
        a.s.synchronize()
        got, got_any = a.hits()
        check_frame(rc, a.t, want, twin, a.rays, got, got_any, f"descriptor path, frame {f}")


# ---- 7. sizes ------------------------------------------------------------------------------------------------------------------------------
def test_single_instance(rc, oracle):
    import torch
    mesh = sphere(rc)
    t = rc.TLAS()
    h = t.push(mesh, rc.scenes.IDENTITY3x4.reshape(1, 12), instance_ids=np.array([0], dtype=np.uint32))
    t.sync()
    moved = np.array([[0.6, 0, 0, -3.0, 0, 1.2, 0, 2.0, 0, 0, 0.9, 1.0]], dtype=np.float32)
    rays = rc.scenes.make_rays(np.array([[-3.05, 2.07, 6.0], [-2.9, 2.2, 6.0], [0.0, 0.0, 6.0], [-3.1, 1.8, 6.0]]), [0, 0, -1])
    want = OracleFrame(oracle, rc, moved, rays)
    assert want.closest["hit"].sum() == 3
    twin = fresh_twin(rc, moved)
    s = torch.cuda.Stream()
    d_xf = torch.from_numpy(moved).cuda()
    torch.cuda.synchronize()
    t.update_transforms_device(h, d_xf, stream=s.cuda_stream)
    t.rebuild_device_async(stream=s.cuda_stream)
    s.synchronize()
    check_frame(rc, t, want, twin, rays, t.trace(rays), t.trace(rays, mode="any"), "one instance")


def test_5000_instances_against_fresh_twin(rc):
    """Many workgroups, the chain with rocPRIM's sort, eager and captured."""
    import torch
    sc = rc.scenes
    g = sc.rng(9)
    pos = g.uniform(-50, 50, size=(5000, 3))
    xf = np.tile(sc.IDENTITY3x4, (5000, 1)).astype(np.float32)
    xf[:, [3, 7, 11]] = pos
    mesh = sc.fan_sphere(8, 5, radius=0.4)
    t = rc.TLAS()
    h = t.push(mesh, xf, instance_ids=np.arange(5000, dtype=np.uint32))
    t.sync()
    rays = sc.make_rays(np.repeat(pos[:3000], 2, axis=0) + g.uniform(-0.4, 0.4, size=(6000, 3)) + [0, 0, 5], [0, 0, -1])
    R = sc.random_rotations(5000, 77)
    s = torch.cuda.Stream()
    d_xf = torch.zeros(5000, 12, dtype=torch.float32, device="cuda")
    d_xf.record_stream(s)
    torch.cuda.synchronize()
    graph = None
    for k in range(3):  # k == 0 eager, then the captured pair replayed
        perm = np.random.Generator(np.random.Philox(key=40 + k)).permutation(5000)
        p1 = pos[perm] + g.uniform(-0.5, 0.5, size=pos.shape)
        xf1 = np.concatenate([R * g.uniform(0.6, 1.4, size=(5000, 1, 1)), p1[:, :, None]], axis=2)
        xf1 = np.ascontiguousarray(xf1.reshape(5000, 12), dtype=np.float32)
        twin = rc.TLAS()
        twin.push(mesh, xf1, instance_ids=np.arange(5000, dtype=np.uint32))
        twin.sync()
        assert twin.last_sync_action == "rebuild"
        src = torch.from_numpy(xf1).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            d_xf.copy_(src)
            if k == 0:
                t.update_transforms_device(h, d_xf, stream=s.cuda_stream)
                t.rebuild_device_async(stream=s.cuda_stream)
            else:
                if graph is None:
                    s.synchronize()
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph, stream=s):
                        st = torch.cuda.current_stream().cuda_stream
                        t.update_transforms_device(h, d_xf, stream=st)
                        t.rebuild_device_async(stream=st)
                graph.replay()
        s.synchronize()
        assert_same_scene(t, twin, f"5000 instances, step {k}")
        got, want = t.trace(rays), twin.trace(rays)
        assert got.tobytes() == want.tobytes() and want["hit"].mean() > 0.2
    del graph
    t.set_option("release_captures", 1)


@pytest.mark.parametrize("fused", [1, 0])
def test_two_blases_of_different_size(rc, oracle, fused):
    import torch
    sc = rc.scenes
    blas = [sc.fan_sphere(10, 6, radius=0.5), sc.fan_sphere(16, 9, radius=0.8)]
    dims = (5, 5, 4)
    n = 100
    owner = np.array([0] * 60 + [1] * 40)
    xf0 = sc.lattice_transforms(*dims, 1.9, 5)[0]
    t = rc.TLAS()
    ids = np.arange(n, dtype=np.uint32)
    hs = []
    for k, b in enumerate(blas):
        bi = t.add_geometry(b)
        hs.append(t.push_instances(bi, xf0[owner == k], ids[owner == k]))
    t.sync()
    t.set_option("tlas_rebuild_fused", fused)
    ext = (np.array(dims, dtype=np.float64) - 1) * 2.0
    rays = sc.pinhole_rays(192, 192, ext / 2 + np.array([0.45, 0.3, 1.0]) * (0.95 * ext[:2].max() + 3.0), ext / 2, fov_deg=45.0)
    s = torch.cuda.Stream()
    d_rays = dev_bytes(torch, rays)
    d_hits, d_any = (torch.zeros(len(rays) * 32, dtype=torch.uint8, device="cuda") for _ in range(2))
    for f in range(2):
        xf = sc.lattice_transforms(*dims, 1.8 + 0.3 * f, 200 + f)[0].reshape(n, 3, 4).copy()
        perm = np.random.Generator(np.random.Philox(key=700 + f)).permutation(n)
        xf[:, :, 3] = xf[perm][:, :, 3]
        xf = np.ascontiguousarray(xf.reshape(n, 12))
        want = OracleFrame(oracle, rc, xf, rays, blas=blas, owner=owner)
        assert want.closest["hit"].mean() >= 0.2
        twin = fresh_twin(rc, xf, blas=blas, owner=owner)
        parts = [torch.from_numpy(xf[owner == k]).cuda() for k in range(2)]
        torch.cuda.synchronize()
        for k in range(2):
            t.update_transforms_device(hs[k], parts[k], stream=s.cuda_stream)
        t.rebuild_device_async(stream=s.cuda_stream)
        t.trace_device(d_rays.data_ptr(), d_hits.data_ptr(), len(rays), stream=s.cuda_stream)
        t.trace_device(d_rays.data_ptr(), d_any.data_ptr(), len(rays), mode="any", stream=s.cuda_stream)
        s.synchronize()
        check_frame(rc, t, want, twin, rays, hits_of(rc, d_hits), hits_of(rc, d_any), f"two BLASes, frame {f}")


# ---- 8. errors, the empty scene, and a BLAS build beside the rebuild ------------------------------------------------------------------------
def test_errors_leave_the_scene_usable(rc):
    import torch
    dims = SMALL
    t, (h,), cuts = make_scene(rc, dims)
    n = cuts[-1]
    rays = camera_rays(rc, dims)[::16]
    base = t.trace(rays).tobytes()
    nodes = t.adapt().nodes.tobytes()
    L = rc.lib()
    assert L.rc_rebuild_tlas_device_async(None, None) == RC_ERR_INVALID_ARGUMENT  # NULL scene
    assert t.sync().last_sync_action == "noop" and t.trace(rays).tobytes() == base
    # pending push
    one = t.push(sphere(rc), rc.scenes.IDENTITY3x4.reshape(1, 12), instance_ids=np.array([7777], dtype=np.uint32))
    assert L.rc_rebuild_tlas_device_async(t._h, None) == RC_ERR_NOT_SYNCED
    assert "rc_sync" in L.rc_last_error().decode()
    with pytest.raises(rc.RaycoreError) as e:
        t.rebuild_device_async()
    assert e.value.code == RC_ERR_NOT_SYNCED
    assert t.delete(one)
    t.sync()
    assert t.trace(rays).tobytes() == base and t.adapt().nodes.tobytes() == nodes
    # pending host-side transform update: the mirror holds edits the device lacks
    same = t.get_instances(h)["transform"].copy()
    t.update_transforms(h, same)
    assert L.rc_rebuild_tlas_device_async(t._h, None) == RC_ERR_NOT_SYNCED
    assert t.sync().last_sync_action == "refit"
    assert t.trace(rays).tobytes() == base and t.adapt().nodes.tobytes() == nodes
    # never synced
    fresh = rc.TLAS()
    fresh.push(sphere(rc), initial_xf(rc, dims), instance_ids=np.arange(n, dtype=np.uint32))
    assert L.rc_rebuild_tlas_device_async(fresh._h, None) == RC_ERR_NOT_SYNCED
    fresh.sync()
    assert fresh.trace(rays).tobytes() == base
    # accepted now, with nothing moved: the same tree, the same hits (both device paths)
    for fused in (1, 0):
        fresh.set_option("tlas_rebuild_fused", fused)
        fresh.rebuild_device_async()
        assert fresh.trace(rays).tobytes() == base  # (the host-buffer trace waits for the rebuild itself)
        assert fresh.sync().last_sync_action == "noop" and fresh.adapt().nodes.tobytes() == nodes
    # a scene with no instances: success, nothing enqueued
    empty = rc.TLAS()
    empty.add_geometry(sphere(rc))
    empty.sync()
    assert L.rc_rebuild_tlas_device_async(empty._h, None) == 0
    assert empty.sync().last_sync_action == "noop"
    torch.cuda.synchronize()


def test_blas_build_beside_the_rebuild(rc, oracle):
    """add_geometry runs on the scene's own stream while the rebuild runs on the caller's: they share no scratch."""
    import torch
    dims = LARGE
    a = Frames(rc, dims, 0)
    big = rc.scenes.fan_sphere(96, 49, radius=0.5)  # 9 216 triangles: the BLAS build sorts more keys than the scene has instances
    want = oracle_frame(oracle, rc, dims, 1)
    twin = fresh_twin(rc, frame_xf(rc, dims, 1))
    a.t.add_geometry(big)  # (grows the build scratch now, so that the build below allocates nothing)
    torch.cuda.synchronize()
    with torch.cuda.stream(a.s):
        a.d_xf.copy_(a.frames[1])
        for _ in range(8):  # eight rebuilds in flight behind each other, the BLAS build beside them
            a.t.update_transforms_device(a.h, a.d_xf, stream=a.s.cuda_stream)
            a.t.rebuild_device_async(stream=a.s.cuda_stream)
    a.t.add_geometry(big)  # host returns once the scene's own stream is done; the rebuild's stream may still be running
    with torch.cuda.stream(a.s):
        a.trace(a.s.cuda_stream)
    a.s.synchronize()
    got, got_any = a.hits()
    assert_hits_equal(got, want.closest, "rebuild beside a BLAS build: closest vs oracle")
    assert_hits_equal(got_any, want.any, "rebuild beside a BLAS build: any vs oracle")
    assert a.t.sync().last_sync_action == "noop"  # add_geometry alone changes nothing the TLAS holds
    assert a.t.adapt().nodes.tobytes() == want.nodes.tobytes() == twin.adapt().nodes.tobytes()
    assert got.tobytes() == twin.trace(a.rays).tobytes()
