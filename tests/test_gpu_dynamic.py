"""Device-side animation: update_transforms_device + refit_device_async (rc_update_transforms_device, rc_refit_device_async) on the GPU.

Two yardsticks, neither of them the code under test:

* the HOST TWIN: a second scene with the same pushes that gets each frame's transforms through update_transforms + sync (a refit).  Same
  topology as the scene under test, so everything must be byte-identical: exported TLAS nodes, exported instances (inverses included),
  world bound, and every hit record, exact ties included;
* the ORACLE FROM SCRATCH: oracle.pyoracle.Scene built anew with the frame's transforms.  A rebuild re-sorts, so only hits are compared
  (fan spheres under generic rotations: no exact ties), bit for bit.

Every frame's inputs are checked on the ORACLE's output first (oracle_frame): at least a fifth of the rays hit, and at least a tenth of
the hit records differ from the previous frame's -- so a stale leaf box or inverse cannot go unnoticed.

WHICH KERNEL RUNS HERE: option `kernel` stays at -1 and a batch is 65 536 rays, below the 6 * 256 * n_cus * 5/4 (491 520 on 256 CUs) from
which the default dispatch leaves kernel 0 (rc_launch_trace).  Kernel 0 reads the traversal copy from memory and never tests an
entry-cull sphere, so nothing in this file reads the spheres, their copies in the TLAS leaf records, the LDS planes or the renumbered
tops.  The kernel matrix (0, 1, 3, 5, 6, both stack shapes, entry_cull 1 / 0 / 2) after every frame of these paths, and the derived
arrays themselves, are in tests/test_gpu_update_kernels.py.
"""
import ctypes as C

import numpy as np
import pytest

from dynamic_kit import LARGE, RC_ERR_INVALID_ARGUMENT, RC_ERR_INVALID_HANDLE, RC_ERR_NOT_SYNCED, SMALL, assert_same_scene, camera_rays, dev_bytes
from dynamic_kit import frame_xf, hits_of, host_frame, initial_xf, make_scene, oracle_frame, oracle_scene_hits, sphere
from gpu_kit import rc  # noqa: F401
from helpers import assert_hits_equal

pytestmark = pytest.mark.gpu

N_FRAMES = 4


# ---- 1. update on the device, commit with sync() ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [SMALL, LARGE])
def test_update_device_then_sync(rc, oracle, dims):
    import torch
    t, (h,), cuts = make_scene(rc, dims)
    twin, th, _ = make_scene(rc, dims)
    rays = camera_rays(rc, dims)
    for f in range(N_FRAMES):
        want = oracle_frame(oracle, rc, dims, f)
        xf = frame_xf(rc, dims, f)
        host_frame(twin, th, cuts, xf)
        d_xf = torch.from_numpy(xf).cuda()
        t.update_transforms_device(h, d_xf if f % 2 == 0 else d_xf.reshape(-1, 3, 4))
        with pytest.raises(rc.RaycoreError) as e:  # transforms-dirty from the device: no query before the refit
            t.trace(rays[:4])
        assert e.value.code == RC_ERR_NOT_SYNCED
        t.sync()
        assert t.last_sync_action == "refit"
        got = t.trace(rays)
        assert got.tobytes() == twin.trace(rays).tobytes(), f"frame {f}: hits differ from the host twin"
        assert_hits_equal(got, want, f"frame {f} vs oracle")
        assert_same_scene(t, twin, f"frame {f}")
        assert np.array_equal(t.get_instances(h)["transform"], xf)  # lazy mirror refresh
    # a later host-side push + sync starts from the refreshed mirror (stale at the time of the push: nothing has read it since)
    last = frame_xf(rc, dims, 0)
    t.update_transforms_device(h, torch.from_numpy(last).cuda())
    assert t.sync().last_sync_action == "refit"
    extra = t.push(sphere(rc)[:4])
    t.update_transform(extra, np.eye(4, dtype=np.float32))
    t.sync()
    assert t.last_sync_action == "rebuild"
    assert np.array_equal(t.get_instances(h)["transform"], last)
    assert np.array_equal(t.adapt().instances["transform"][:len(last)], last)


# ---- 2. update -> refit -> trace on one stream, no host synchronisation between them -----------------------------------------------------
@pytest.mark.parametrize("dims", [SMALL, LARGE])
def test_async_update_refit_trace(rc, oracle, dims):
    import torch
    t, (h,), cuts = make_scene(rc, dims)
    twin, th, _ = make_scene(rc, dims)
    rays = camera_rays(rc, dims)
    n = len(rays)
    frames = [torch.from_numpy(frame_xf(rc, dims, f)).cuda() for f in range(N_FRAMES)]
    d_xf = torch.empty_like(frames[0])
    d_rays = dev_bytes(torch, rays)
    d_hits, d_any = (torch.zeros(n * 32, dtype=torch.uint8, device="cuda") for _ in range(2))
    s = torch.cuda.Stream()
    for buf in (d_xf, d_rays, d_hits, d_any, *frames):
        buf.record_stream(s)
    torch.cuda.synchronize()
    for f in range(N_FRAMES):
        want = oracle_frame(oracle, rc, dims, f)
        host_frame(twin, th, cuts, frame_xf(rc, dims, f))
        with torch.cuda.stream(s):
            d_xf.copy_(frames[f])  # the transforms are produced on the stream too
            t.update_transforms_device(h, d_xf, stream=s.cuda_stream)
            t.refit_device_async(stream=s.cuda_stream)
            t.trace_device(d_rays.data_ptr(), d_hits.data_ptr(), n, stream=s.cuda_stream)
            t.trace_device(d_rays.data_ptr(), d_any.data_ptr(), n, mode="any", stream=s.cuda_stream)
        bound = t.world_bound()  # the lazy refresh: waits for the refit, reads the root back
        tb = twin.world_bound()
        assert bound.p_min.tobytes() == tb.p_min.tobytes() and bound.p_max.tobytes() == tb.p_max.tobytes(), f"frame {f}: lazy world bound"
        s.synchronize()
        got = hits_of(rc, d_hits)
        assert got.tobytes() == twin.trace(rays).tobytes(), f"frame {f}: closest hits differ from the host twin"
        assert hits_of(rc, d_any).tobytes() == twin.trace(rays, mode="any").tobytes(), f"frame {f}: any hits differ from the host twin"
        assert_hits_equal(got, want, f"frame {f} vs oracle")
        assert t.sync().last_sync_action == "noop"  # the asynchronous refit left nothing pending
        assert_same_scene(t, twin, f"frame {f}")


# ---- 3. one handle of three -----------------------------------------------------------------------------------------------------------
def test_partial_update(rc, oracle):
    import torch
    dims = SMALL
    t, hs, cuts = make_scene(rc, dims, n_handles=3)
    twin, ths, _ = make_scene(rc, dims, n_handles=3)
    rays = camera_rays(rc, dims)
    before = [t.get_instances(h).copy() for h in hs]
    xf = frame_xf(rc, dims, 1)
    host_frame(twin, ths, cuts, xf, which={1})
    s = torch.cuda.Stream()
    d_xf = torch.from_numpy(xf[cuts[1]:cuts[2]]).cuda()
    torch.cuda.synchronize()
    t.update_transforms_device(hs[1], d_xf, stream=s.cuda_stream)
    t.refit_device_async(stream=s.cuda_stream)
    s.synchronize()
    assert t.trace(rays).tobytes() == twin.trace(rays).tobytes()
    assert_same_scene(t, twin, "partial update")
    assert t.get_instances(hs[0]).tobytes() == before[0].tobytes() and t.get_instances(hs[2]).tobytes() == before[2].tobytes()
    mid = t.get_instances(hs[1])
    assert np.array_equal(mid["transform"], xf[cuts[1]:cuts[2]]) and not np.array_equal(mid["transform"], before[1]["transform"])
    assert np.array_equal(mid[["blas_index", "instance_id", "flags"]], before[1][["blas_index", "instance_id", "flags"]])
    # and the oracle, with the mixed transforms
    mixed = initial_xf(rc, dims).copy()
    mixed[cuts[1]:cuts[2]] = xf[cuts[1]:cuts[2]]
    assert_hits_equal(t.trace(rays), oracle_scene_hits(oracle, rc, mixed, rays), "partial update vs oracle")


# ---- 4. update -> refit -> trace closest -> trace any as one graph, replayed once per frame ----------------------------------------------
@pytest.mark.parametrize("dims", [SMALL, LARGE])
def test_graph_replay_per_frame(rc, oracle, dims):
    import torch
    t, (h,), cuts = make_scene(rc, dims)
    twin, th, _ = make_scene(rc, dims)
    rays = camera_rays(rc, dims)
    n = len(rays)
    frames = [torch.from_numpy(frame_xf(rc, dims, f)).cuda() for f in range(N_FRAMES)]
    d_xf = frames[0].clone()
    d_rays = dev_bytes(torch, rays)
    d_hits, d_any = (torch.zeros(n * 32, dtype=torch.uint8, device="cuda") for _ in range(2))
    s = torch.cuda.Stream()
    for buf in (d_xf, d_rays, d_hits, d_any, *frames):
        buf.record_stream(s)

    def frame(st):
        t.update_transforms_device(h, d_xf, stream=st)
        t.refit_device_async(stream=st)
        t.trace_device(d_rays.data_ptr(), d_hits.data_ptr(), n, stream=st)
        t.trace_device(d_rays.data_ptr(), d_any.data_ptr(), n, mode="any", stream=st)

    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        frame(s.cuda_stream)  # eager first
    s.synchronize()
    host_frame(twin, th, cuts, frame_xf(rc, dims, 0))
    assert hits_of(rc, d_hits).tobytes() == twin.trace(rays).tobytes(), "eager frame"
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        frame(torch.cuda.current_stream().cuda_stream)
    assert t.get_option("release_captures") == 2  # the two traces; update and refit hold no capture slot
    for f in list(range(1, N_FRAMES)) + [0]:
        want = oracle_frame(oracle, rc, dims, f)
        host_frame(twin, th, cuts, frame_xf(rc, dims, f))
        d_hits.zero_(); d_any.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            d_xf.copy_(frames[f])  # in place: the graph reads the tensor when it runs
            g.replay()
        s.synchronize()
        got = hits_of(rc, d_hits)
        assert got.tobytes() == twin.trace(rays).tobytes(), f"replay of frame {f}: closest hits differ from the host twin"
        assert hits_of(rc, d_any).tobytes() == twin.trace(rays, mode="any").tobytes(), f"replay of frame {f}: any hits differ"
        assert_hits_equal(got, want, f"replay of frame {f} vs oracle")
        assert_same_scene(t, twin, f"replay of frame {f}")  # (the bound is re-read while a graph with a refit may live)
    del g
    t.set_option("release_captures", 1)
    assert t.get_option("release_captures") == 0
    assert t.trace(rays).tobytes() == twin.trace(rays).tobytes()


# ---- 5. WavefrontPaths(dynamic=...) ---------------------------------------------------------------------------------------------------
def test_wavefront_dynamic_frame(rc, oracle):
    import torch
    from raycore_jl_amd.wavefront import WavefrontPaths, lookat_camera
    dims = SMALL
    t, (h,), cuts = make_scene(rc, dims)
    twin, th, _ = make_scene(rc, dims)
    for f in range(N_FRAMES):
        oracle_frame(oracle, rc, dims, f)  # (the frames' inputs are the ones checked above)
    ext = (np.array(dims, dtype=np.float64) - 1) * 1.8
    cam = lookat_camera(ext / 2 + np.array([0.45, 0.3, 1.0]) * (0.95 * ext[:2].max() + 3.0), ext / 2, 64, 48)
    light = np.array([ext[0] / 2, ext[1] + 8.0, ext[2] + 6.0], dtype=np.float32)
    frames = [torch.from_numpy(frame_xf(rc, dims, f)).cuda() for f in range(N_FRAMES)]
    d_xf = frames[0].clone()
    torch.cuda.synchronize()
    dyn = WavefrontPaths(t, 64, 48, 2, 2, cam, light, seed=11, dynamic=[(h, d_xf)])
    ref = WavefrontPaths(twin, 64, 48, 2, 2, cam, light, seed=11)
    assert any(b is d_xf for b in dyn.buffers()) and len(dyn.buffers()) == len(ref.buffers()) + 1
    s = torch.cuda.Stream()

    def compare(what):
        torch.cuda.synchronize()
        alive = 0
        for b in range(2):
            for name in ("rays", "hits", "shadow_hits", "path_ids"):
                x, y = getattr(dyn, name)[b], getattr(ref, name)[b]
                assert torch.equal(x, y), f"{what}: {name}[{b}] differs from the static frame on the host twin"
            alive += int(np.count_nonzero(hits_of(rc, dyn.hits[b])["hit"]))
        assert alive > 0.1 * dyn.n, what

    for f in range(N_FRAMES):  # eager
        host_frame(twin, th, cuts, frame_xf(rc, dims, f))
        with torch.cuda.stream(s):
            d_xf.copy_(frames[f])
            dyn.run(s)
            ref.run(s)
        compare(f"eager frame {f}")
    dyn.capture(s)
    for f in (1, 3, 0):  # replayed
        host_frame(twin, th, cuts, frame_xf(rc, dims, f))
        for buf in dyn.hits + dyn.shadow_hits:
            buf.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            d_xf.copy_(frames[f])
            dyn.replay()
            ref.run(s)
        compare(f"replayed frame {f}")
    dyn.graph = None
    torch.cuda.synchronize()
    t.set_option("release_captures", 1)


# ---- 6. the drivers and the lazy world bound ---------------------------------------------------------------------------------------------
def test_drivers_after_async_refit(rc):
    import torch
    dims = SMALL
    t, (h,), cuts = make_scene(rc, dims)
    twin, th, _ = make_scene(rc, dims)
    rays = camera_rays(rc, dims)
    s = torch.cuda.Stream()
    viewdir = np.array([0.3, -0.2, -1.0], dtype=np.float32)
    xf = frame_xf(rc, dims, 3)  # the widest pitch: the bound grows, so a grid laid out from the old one misses the rim
    host_frame(twin, th, cuts, xf)
    d_xf = torch.from_numpy(xf).cuda()
    torch.cuda.synchronize()
    t.update_transforms_device(h, d_xf, stream=s.cuda_stream)
    t.refit_device_async(stream=s.cuda_stream)
    got = rc.get_illumination(t, viewdir, 300)  # no host wait of the caller's in between
    want = rc.get_illumination(twin, viewdir, 300)
    assert np.array_equal(got, want) and want.sum() > 0
    # inside an open capture with a stale bound: a clear error, never an old bound
    xf2 = frame_xf(rc, dims, 0)
    host_frame(twin, th, cuts, xf2)
    d_xf.copy_(torch.from_numpy(xf2).cuda())
    torch.cuda.synchronize()
    t.update_transforms_device(h, d_xf, stream=s.cuda_stream)
    t.refit_device_async(stream=s.cuda_stream)
    n_prims = t.n_primitives()
    d_counts = torch.zeros(n_prims, dtype=torch.float32, device="cuda")
    d_grid = torch.zeros(64 * 64 * 32, dtype=torch.uint8, device="cuda")
    s.synchronize()  # (the work is done; the HOST copy of the bound is still the old one)
    L = rc.lib()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        st = torch.cuda.current_stream().cuda_stream
        d_counts.zero_()  # (something for the graph to hold)
        status = L.rc_get_illumination_device(t._h, viewdir.ctypes.data_as(C.c_void_p), 64, 0, 64 * 64, C.c_void_p(d_counts.data_ptr()), C.c_void_p(st))
        message = L.rc_last_error().decode()
        status2 = L.rc_generate_ray_grid_device(t._h, viewdir.ctypes.data_as(C.c_void_p), 64, C.c_void_p(d_grid.data_ptr()), C.c_void_p(st))
        message2 = L.rc_last_error().decode()
    assert status == RC_ERR_NOT_SYNCED and "stale world bound" in message, (status, message)
    assert status2 == RC_ERR_NOT_SYNCED and "stale world bound" in message2, (status2, message2)
    del g
    torch.cuda.synchronize()
    # ... and the scene works as before
    assert t.trace(rays).tobytes() == twin.trace(rays).tobytes()
    assert np.array_equal(rc.get_illumination(t, viewdir, 300), rc.get_illumination(twin, viewdir, 300))
    assert_same_scene(t, twin, "after the refused driver calls")


# ---- 7. arguments ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_scene_usable(rc):
    import torch
    dims = SMALL
    t, (h,), cuts = make_scene(rc, dims)
    n = cuts[-1]
    rays = camera_rays(rc, dims)[::16]
    base = t.trace(rays).tobytes()
    d_xf = torch.from_numpy(frame_xf(rc, dims, 1)).cuda()
    torch.cuda.synchronize()
    L = rc.lib()

    def call(handle_id, p, m):
        code = L.rc_update_transforms_device(t._h, handle_id, C.c_void_p(p) if p else None, m, None)
        return code, L.rc_last_error().decode()

    assert call(h.id, d_xf.data_ptr(), n - 1)[0] == RC_ERR_INVALID_ARGUMENT   # wrong m
    assert call(h.id, d_xf.data_ptr(), n + 1)[0] == RC_ERR_INVALID_ARGUMENT
    assert call(h.id, 0, n)[0] == RC_ERR_INVALID_ARGUMENT                     # NULL transforms
    assert call(h.id + 1000, d_xf.data_ptr(), n)[0] == RC_ERR_INVALID_HANDLE  # unknown handle
    assert L.rc_update_transforms_device(None, h.id, C.c_void_p(d_xf.data_ptr()), n, None) == RC_ERR_INVALID_ARGUMENT  # NULL scene
    assert L.rc_refit_device_async(None, None) == RC_ERR_INVALID_ARGUMENT
    with pytest.raises(rc.RaycoreError):  # the wrapper's own checks: dtype, shape
        t.update_transforms_device(h, d_xf.double())
    with pytest.raises(rc.RaycoreError):
        t.update_transforms_device(h, d_xf.reshape(-1, 6))
    assert t.sync().last_sync_action == "noop" and t.trace(rays).tobytes() == base  # nothing was enqueued, nothing marked dirty
    # a one-instance handle, m = 1
    one = t.push(sphere(rc), rc.scenes.IDENTITY3x4.reshape(1, 12), instance_ids=np.array([7777], dtype=np.uint32))
    code, msg = call(h.id, d_xf.data_ptr(), n)
    assert code == RC_ERR_NOT_SYNCED, msg                                     # pending push
    assert L.rc_refit_device_async(t._h, None) == RC_ERR_NOT_SYNCED
    t.sync()
    moved = np.array([[1, 0, 0, -3.0, 0, 1, 0, -3.0, 0, 0, 1, -3.0]], dtype=np.float32)
    t.update_transforms_device(one, torch.from_numpy(moved).cuda())
    t.refit_device_async()
    ray = rc.scenes.make_rays([[-3.02, -2.97, 5.0]], [0, 0, -1])
    hit = t.trace(ray)
    assert hit["hit"][0] == 1 and hit["instance_custom_index"][0] == 7777 and abs(hit["t"][0] - 7.5) < 0.05
    assert np.array_equal(t.get_instances(one)["transform"], moved)
    # pending host-side transform update: the device update would be overwritten by the mirror
    t.update_transforms(one, moved)
    assert call(one.id, d_xf.data_ptr(), 1)[0] == RC_ERR_NOT_SYNCED
    t.sync()
    # deleted handle
    assert t.delete(one)
    assert call(one.id, d_xf.data_ptr(), 1)[0] == RC_ERR_INVALID_HANDLE
    t.sync()
    assert call(one.id, d_xf.data_ptr(), 1)[0] == RC_ERR_INVALID_HANDLE
    assert t.trace(rays).tobytes() == base
    # unsynced scene
    fresh = rc.TLAS()
    fh = fresh.push(sphere(rc), initial_xf(rc, dims), instance_ids=np.arange(n, dtype=np.uint32))
    code = L.rc_update_transforms_device(fresh._h, fh.id, C.c_void_p(d_xf.data_ptr()), n, None)
    assert code == RC_ERR_NOT_SYNCED
    assert L.rc_refit_device_async(fresh._h, None) == RC_ERR_NOT_SYNCED
    fresh.sync()
    fresh.update_transforms_device(fh, d_xf)
    fresh.refit_device_async()
    # a mere READ of the mirror between update and refit is no mutation: the update stays pending and the refit is accepted
    t.update_transforms_device(h, d_xf)
    assert np.array_equal(t.get_instances(h)["transform"], frame_xf(rc, dims, 1))
    with pytest.raises(rc.RaycoreError) as e:
        t.trace(rays)
    assert e.value.code == RC_ERR_NOT_SYNCED
    t.update_transforms_device(h, d_xf)  # a second update after the read
    assert np.array_equal(t.get_instances(h)["inv_transform"], fresh.get_instances(fh)["inv_transform"])
    t.refit_device_async()
    # host-buffer queries wait for the asynchronous refit themselves (here: both enqueued on the null stream, traced on the scenes' own)
    assert fresh.trace(rays).tobytes() == t.trace(rays).tobytes()


# ---- 8. many workgroups: 5 000 instances -------------------------------------------------------------------------------------------------
def test_5000_instances_against_host_twin(rc):
    import torch
    sc = rc.scenes
    g = sc.rng(9)
    pos = g.uniform(-50, 50, size=(5000, 3))
    xf = np.tile(sc.IDENTITY3x4, (5000, 1)).astype(np.float32)
    xf[:, [3, 7, 11]] = pos
    mesh = sc.fan_sphere(8, 5, radius=0.4)
    t, twin = rc.TLAS(), rc.TLAS()
    h, th = t.push(mesh, xf), twin.push(mesh, xf)
    t.sync(); twin.sync()
    R = sc.random_rotations(5000, 77)
    xf1 = np.concatenate([R * g.uniform(0.6, 1.4, size=(5000, 1, 1)), (pos + g.uniform(-0.5, 0.5, size=pos.shape))[:, :, None]], axis=2)
    xf1 = np.ascontiguousarray(xf1.reshape(5000, 12), dtype=np.float32)
    twin.update_transforms(th, xf1)
    assert twin.sync().last_sync_action == "refit"
    s = torch.cuda.Stream()
    d_xf = torch.from_numpy(xf1).cuda()
    torch.cuda.synchronize()
    t.update_transforms_device(h, d_xf, stream=s.cuda_stream)
    t.refit_device_async(stream=s.cuda_stream)
    assert_same_scene(t, twin, "5000 instances")
    rays = sc.make_rays(np.repeat(pos[:3000], 2, axis=0) + g.uniform(-0.4, 0.4, size=(6000, 3)) + [0, 0, 5], [0, 0, -1])
    got, want = t.trace(rays), twin.trace(rays)
    assert got.tobytes() == want.tobytes() and want["hit"].mean() > 0.2
    # the alias path commits through the same asynchronous refit (no update call since the last one: the per-instance passes run)
    ptr, cnt = t.instance_buffer(h)
    assert cnt == 5000

    class Alias:
        __cuda_array_interface__ = {"shape": (5000, 27), "typestr": "<f4", "data": (ptr, False), "version": 2}

    recs = torch.as_tensor(Alias(), device="cuda")
    twin.update_transforms(th, xf)
    twin.sync()
    recs[:, 2:14] = torch.from_numpy(xf).cuda()
    recs[:, 14:26] = torch.from_numpy(twin.get_instances(th)["inv_transform"].copy()).cuda()
    torch.cuda.synchronize()
    t.refit_device_async()
    assert_same_scene(t, twin, "alias + asynchronous refit")
    assert t.trace(rays).tobytes() == twin.trace(rays).tobytes()
