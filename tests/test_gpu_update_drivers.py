"""The drivers after device-side updates (small shapes): view factors after geometry updates, eager and replayed from a graph;
get_illumination and the collision broad phase after a device rebuild and after a geometry update, against the oracle from scratch.

The view-factor drivers address their sources in metadata order through an index the scene caches (rc_ensure_vf_order).  A geometry
update re-sorts the primitives, so the index must follow every update -- also the ones a replayed graph makes, which the library does
not see -- and must be sorted behind the stream that carried the update.
"""
import ctypes as C

import numpy as np
import pytest

import dynamic_kit as dyn
from gpu_kit import rc  # noqa: F401

pytestmark = pytest.mark.gpu

SMALL = dyn.SMALL
RPT, SEED = 64, 1234
VIEWDIR = np.array([0.3, -0.2, -1.0], dtype=np.float32)
GRID = 128


# ---- 1. view factors after geometry updates -------------------------------------------------------------------------------------------------
def vf_frame(verts, meta, f):
    """Frame f of the scene of test_view_factors_parity: deform() of tests/test_gpu_deform.py, the metadata rolled with the faces."""
    return dyn.deform(verts, f), np.ascontiguousarray(np.roll(meta, 7 * (f + 1)))


def test_view_factors_after_geometry_updates(rc, oracle):
    import torch
    from raycore_jl_amd import distributed as rd
    sc = rc.scenes
    verts = np.concatenate([sc.fan_sphere(12, 7, centre=(0, 0, 0), radius=0.5), sc.box_room((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5), 2)])
    n = len(verts)
    meta = np.arange(1, n + 1, dtype=np.uint32)
    t = rc.TLAS()
    h = t.push_instances(t.add_geometry(verts, meta), sc.IDENTITY3x4[None], np.zeros(1, np.uint32))
    t.sync()
    assert t.n_primitives() == n
    wants = {}

    def want_of(f):
        if f not in wants:
            o = oracle.Scene()
            o.add_instance(o.add_blas(*vf_frame(verts, meta, f)), sc.IDENTITY3x4, 0)
            o.build()
            assert len(o.blas_prims) == n
            wants[f] = (o.view_factors(RPT, seed=SEED, nthreads=8), o.blas_prims["meta"].copy())
        return wants[f]

    order0 = want_of(0)[1]
    for f in (1, 2):  # the frames re-sort the primitives and change the matrix: a stale source order or a stale tree cannot pass
        m, order = want_of(f)
        assert np.mean(order != want_of(f - 1)[1]) > 0.8 and np.mean(m != want_of(f - 1)[0]) > 0.02, f
    assert want_of(0)[0].sum() > 0.5 * n * RPT and len(order0) == n

    s = torch.cuda.Stream()
    frames = [tuple(torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for a in vf_frame(verts, meta, f)) for f in range(3)]
    d_soup, d_meta = frames[0][0].clone(), frames[0][1].clone()
    for buf in (d_soup, d_meta, *[x for fr in frames for x in fr]):
        buf.record_stream(s)
    torch.cuda.synchronize()

    def update(st):
        t.update_geometry_device_async(h, d_soup, d_meta=d_meta, stream=st)
        t.refit_device_async(stream=st)

    def check_drivers(f, what):
        """The caller's stream holds the update (or its replay has been waited for); no host wait of the test's before the first driver."""
        want, _ = want_of(f)
        with torch.cuda.stream(s):
            out = rd.view_factors_distributed(t, RPT, SEED, mode="rays")  # first: the device entry point on the stream of the update
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want), f"{what}: view_factors_distributed, mode rays"
        with torch.cuda.stream(s):
            out = rd.view_factors_distributed(t, RPT, SEED, mode="rows")
            block, rows = rd.view_factors_distributed(t, RPT, SEED, mode="rows_sharded")
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want), f"{what}: view_factors_distributed, mode rows"
        full = np.zeros_like(want)
        full[rows] = block.cpu().numpy().view(np.uint32)
        assert np.array_equal(full, want), f"{what}: view_factors_distributed, mode rows_sharded"
        assert np.array_equal(rc.view_factors(t, rays_per_triangle=RPT, seed=SEED), want), f"{what}: view_factors"
        received, emitted = rc.view_factor_totals(t, rays_per_triangle=RPT, seed=SEED)
        assert np.array_equal(received, want.sum(axis=0, dtype=np.uint64)), f"{what}: totals received"
        assert np.array_equal(emitted, want.sum(axis=1, dtype=np.uint64)), f"{what}: totals emitted"

    rc.view_factors(t, rays_per_triangle=RPT, seed=SEED)  # the order of the scene as synced is cached
    with torch.cuda.stream(s):
        update(s.cuda_stream)  # eager, frame 0
    check_drivers(0, "eager update + refit")
    t.wait_for_gpu()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        update(torch.cuda.current_stream().cuda_stream)
    check_drivers(0, "after the capture")  # (a capture runs nothing: still frame 0; the order is cached again)
    for f in (1, 2):
        with torch.cuda.stream(s):
            d_soup.copy_(frames[f][0])  # in place: the graph reads the tensors when it runs
            d_meta.copy_(frames[f][1])
            g.replay()
        s.synchronize()  # a replay is the caller's to wait for
        check_drivers(f, f"replay of frame {f}")
    # on a stream that is being captured the order cannot be rebuilt: a clear error, never an old order
    d_m = torch.zeros(n * n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L = rc.lib()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=s):
        st = torch.cuda.current_stream().cuda_stream
        d_m.zero_()  # (something for the graph to hold)
        status = L.rc_view_factors_device(t._h, RPT, SEED, 0, n, 0, RPT, C.c_void_p(d_m.data_ptr()), n, 1, 0, rd.VF_SOURCES_BY_METADATA, C.c_void_p(st))
        message = L.rc_last_error().decode()
    assert status == dyn.RC_ERR_NOT_SYNCED and "stale view-factor source order" in message, (status, message)
    del g2, g
    torch.cuda.synchronize()
    t.wait_for_gpu()
    t.set_option("release_captures", 1)
    check_drivers(2, "after the graphs are gone")


# ---- 2. illumination after a rebuild and after a geometry update ------------------------------------------------------------------------------
def illumination_both_ways(rc, t, s):
    """get_illumination through the host-buffer call (no host wait of the caller's before it) and rc_get_illumination_device on `s`."""
    import torch
    got = rc.get_illumination(t, VIEWDIR, GRID)
    d_counts = torch.zeros(t.n_primitives(), dtype=torch.float32, device="cuda")
    d_counts.record_stream(s)
    torch.cuda.synchronize()
    status = rc.lib().rc_get_illumination_device(t._h, VIEWDIR.ctypes.data_as(C.c_void_p), GRID, 0, GRID * GRID, C.c_void_p(d_counts.data_ptr()), C.c_void_p(s.cuda_stream))
    assert status == 0, rc.lib().rc_last_error().decode()
    s.synchronize()
    return got, d_counts.cpu().numpy()


@pytest.mark.parametrize("fused", [1, 0])
def test_illumination_after_device_rebuild(rc, oracle, fused):
    import torch
    a = dyn.Frames(rc, SMALL, fused)
    f = dyn.TIE_FRAME  # the widest pitch (the bound grows: a grid laid out from the old one misses the rim), permuted, three coincident instances
    xf = dyn.rebuild_frame_xf(rc, SMALL, f)
    o = oracle.Scene()
    b = o.add_blas(dyn.sphere(rc))
    for i, x in enumerate(xf):
        o.add_instance(b, x, i)
    o.build()
    want = o.get_illumination(VIEWDIR, GRID, nthreads=8)
    with torch.cuda.stream(a.s):
        a.d_xf.copy_(a.frames[f])
    a.t.update_transforms_device(a.h, a.d_xf, stream=a.s.cuda_stream)
    a.t.rebuild_device_async(stream=a.s.cuda_stream)
    got, got_dev = illumination_both_ways(rc, a.t, a.s)
    assert want.sum() > 0.2 * GRID * GRID
    assert np.array_equal(got, want), "get_illumination after update + rebuild"
    assert np.array_equal(got_dev, want), "rc_get_illumination_device after update + rebuild"


def test_illumination_after_geometry_update(rc, oracle):
    import torch
    spec = dyn.Spec(rc, "144")
    t, hs = spec.build(rc)
    f = 3
    o = oracle.Scene()
    b = o.add_blas(dyn.deform(spec.soups[0], f))
    for i, x in enumerate(spec.xf):
        o.add_instance(b, x, i)
    o.build()
    want = o.get_illumination(VIEWDIR, GRID, nthreads=8)
    s = torch.cuda.Stream()
    d_soup = torch.from_numpy(dyn.deform(spec.soups[0], f)).cuda()
    d_soup.record_stream(s)
    torch.cuda.synchronize()
    t.update_geometry_device_async(hs[-1], d_soup, stream=s.cuda_stream)
    t.rebuild_device_async(stream=s.cuda_stream)
    got, got_dev = illumination_both_ways(rc, t, s)
    t.wait_for_gpu()
    assert want.sum() > 0.2 * GRID * GRID and np.count_nonzero(want) > 0.5 * len(want)
    assert np.array_equal(got, want), "get_illumination after geometry update + rebuild"
    assert np.array_equal(got_dev, want), "rc_get_illumination_device after geometry update + rebuild"


# ---- 3. the collision broad phase after update + refit and update + rebuild --------------------------------------------------------------------
@pytest.mark.parametrize("commit", ["refit", "rebuild-fused", "rebuild-chain"])
def test_collision_after_device_update(rc, oracle, commit):
    """Instances moved to a lattice of pitch 0.8 (neighbouring boxes overlap), the broad phase enqueued on the stream of the update with no
    host wait before the call.  After a rebuild: content AND order are the oracle's from scratch.  After a refit the contacts come out in
    the order of the kept topology: content against the oracle, order against the host twin."""
    import torch
    from raycore_jl_amd._capi import check, lib, ptr
    t, (h,), cuts = dyn.make_scene(rc, SMALL)
    n = cuts[-1]
    if commit != "refit":
        t.set_option("tlas_rebuild_fused", 1 if commit == "rebuild-fused" else 0)
    xf = rc.scenes.lattice_transforms(*SMALL, 0.8, 311)[0]
    o = oracle.Scene()
    b = o.add_blas(dyn.sphere(rc))
    for i, x in enumerate(xf):
        o.add_instance(b, x, i)
    o.build()
    want, _ = o.collide_instances()
    assert len(want) >= n, len(want)
    assert rc.collide_instances(t).num_contacts < len(want) // 4  # (the scene as synced: pitch 1.6)
    s = torch.cuda.Stream()
    d_xf = torch.from_numpy(xf).cuda()
    d_out = torch.zeros(2 * (len(want) + 8), dtype=torch.int32, device="cuda")
    for buf in (d_xf, d_out):
        buf.record_stream(s)
    torch.cuda.synchronize()
    t.update_transforms_device(h, d_xf, stream=s.cuda_stream)
    (t.refit_device_async if commit == "refit" else t.rebuild_device_async)(stream=s.cuda_stream)
    count = C.c_uint64(0)
    check(lib().rc_collide_instances_device(t._h, ptr(d_out.data_ptr()), len(want) + 8, C.byref(count), ptr(s.cuda_stream)))
    s.synchronize()
    assert count.value == len(want)
    got = d_out.cpu().numpy().view(np.uint32)[:2 * len(want)].reshape(-1, 2)
    res = rc.collide_instances(t)  # the host-buffer call waits for the update itself
    host = np.stack([res.contacts["instance_a"], res.contacts["instance_b"]], axis=1)
    assert np.array_equal(host, got), "rc_collide_instances differs from rc_collide_instances_device"
    if commit == "refit":
        def by_pair(c):
            return c[np.lexsort((c[:, 1], c[:, 0]))]
        assert np.array_equal(by_pair(got), by_pair(np.asarray(want))), "contacts after update + refit vs oracle (content)"
        twin, th, _ = dyn.make_scene(rc, SMALL)
        dyn.host_frame(twin, th, cuts, xf)
        tw = rc.collide_instances(twin)
        assert np.array_equal(got, np.stack([tw.contacts["instance_a"], tw.contacts["instance_b"]], axis=1)), "contacts after update + refit vs host twin (order)"
    else:
        assert np.array_equal(got, want), "contacts after update + rebuild vs oracle (content and order)"
