"""Gated TLAS rebuild on the GPU: tlas_cost_device, refit_or_rebuild_device_async, tlas_quality, WavefrontPaths(rebuild="auto"), on both
device paths (the single-workgroup kernel, option tlas_rebuild_fused = 1 up to 256 instances, and the chain of build kernels).

Yardsticks, none of them the code under test:

* THE DECISION: numpy, f64 (auto_rebuild_model.cost), on the EXPORTED NODES OF TWINS -- a host-path twin that refits every frame
  (update_transforms + sync, action "refit") and a fresh twin built structurally with the frame's transforms (fresh_twin of
  tests/test_gpu_rebuild.py).  cost > 1.5 * cost_built decides; after an expected rebuild the fresh twin replaces the refitting one and
  its cost becomes the expected cost_built.
* THE TREE AND THE HITS: TLAS nodes, instances and world bound byte for byte, closest and any hits bit for bit, against whichever twin took
  the expected decision; hits also against the oracle built from scratch (assert_hits_equal) -- closest hits on every frame, any hits in
  full on the frames that rebuilt (the tree is then the oracle's) and on their `hit` word on the frames that refitted: which record
  any_hit returns follows the traversal order, and a refitted tree keeps the order of the last sort (tests/test_gpu_dynamic.py compares
  closest hits only for the same reason).

The animation (tests/auto_rebuild_model.py): drift, shuffle, drift, drift, shuffle, drift from the initial lattice of
tests/test_gpu_dynamic.py, under its 256 x 256 camera.  The conditions on the inputs are asserted on the twins' nodes (and, without a GPU,
on the oracle's in tests/test_auto_rebuild_model.py): drift frames at a ratio <= 1.25 with >= 0.2 of the leaf slots different in the fresh
tree, shuffle frames at >= 3.0 with >= 0.9 -- a rebuild taken or skipped wrongly cannot pass the byte comparison.

The yardstick of a scene is computed once (track) and shared by every test; nothing modifies it.

The cost is compared at a relative error <= 1e-11: a sum of at most 863 positive f64 terms in any order is within about n 2^-53 ~ 1e-13 of
the exact one on each side, which leaves two decades for the divide and numpy's own order.
"""
import numpy as np
import pytest

import auto_rebuild_model as model
from dynamic_kit import LARGE, OracleFrame, PATHS, PATH_IDS, SMALL, camera_rays, dev_bytes, fresh_twin, hits_of, initial_xf, make_scene, sphere
from gpu_kit import rc  # noqa: F401
from helpers import assert_hits_equal

pytestmark = pytest.mark.gpu

RATIO = model.RATIO
REL = 1e-11
RC_ERR_INVALID_ARGUMENT, RC_ERR_NOT_SYNCED = 1, 6
N_FRAMES = len(model.KINDS)


def close(a, b):
    return abs(a - b) <= REL * abs(b)


def frames_of(rc, dims):
    return model.animation(rc.scenes, dims, initial_xf(rc, dims))


class Ref:
    """What one frame must leave: the twin that took the expected decision, frozen."""

    def __init__(self, rc, twin, rays, want, rebuild, cost, cost_built):
        st = twin.adapt()
        b = twin.world_bound()
        self.nodes, self.instances = st.nodes.tobytes(), st.instances.tobytes()
        self.bound = np.concatenate([b.p_min, b.p_max]).tobytes()
        self.closest, self.any = twin.trace(rays).tobytes(), twin.trace(rays, mode="any").tobytes()
        self.want, self.rebuild, self.cost, self.cost_built = want, rebuild, cost, cost_built


_tracks = {}


def track(rc, oracle, dims):
    """(refs, armed_cost): per frame the Ref of the animation under RATIO, decided in numpy from the twins' exported nodes, and the cost
    of the tree built from the initial transforms, which the arming call records."""
    if dims in _tracks:
        return _tracks[dims]
    rays = camera_rays(rc, dims)
    frames = frames_of(rc, dims)
    n = len(frames[0])
    ths = []
    twin = fresh_twin(rc, initial_xf(rc, dims), handles=ths)
    built = model.cost(twin.adapt().nodes, n)
    armed_cost = built
    refs, steps = [], []
    for f, xf in enumerate(frames):
        twin.update_transforms(ths[0], xf)
        assert twin.sync().last_sync_action == "refit"
        refit_nodes = twin.adapt().nodes.copy()
        fhs = []
        fresh = fresh_twin(rc, xf, handles=fhs)
        fresh_nodes = fresh.adapt().nodes.copy()
        c = model.cost(refit_nodes, n)
        rebuild = bool(c > RATIO * built)
        steps.append({"ratio": c / built, "rebuild": rebuild, "leaf_diff": model.leaf_slots_differing(fresh_nodes, refit_nodes, n)})
        if rebuild:
            twin, ths, built = fresh, fhs, model.cost(fresh_nodes, n)
        want = OracleFrame(oracle, rc, xf, rays)
        assert want.closest["hit"].mean() >= 0.2
        refs.append(Ref(rc, twin, rays, want, rebuild, c, built))
    model.assert_conditions(steps, f"twins, {n} instances")
    assert [r.rebuild for r in refs] == list(model.REBUILDS)
    _tracks[dims] = (refs, armed_cost)
    return _tracks[dims]


class Anim:
    """The device buffers of one scene's animation on one stream."""

    def __init__(self, rc, dims, fused):
        import torch
        self.torch, self.rc, self.dims = torch, rc, dims
        self.t, (self.h,), _ = make_scene(rc, dims)
        self.t.set_option("tlas_rebuild_fused", fused)
        self.rays = camera_rays(rc, dims)
        self.n = len(self.rays)
        self.frames = [torch.from_numpy(xf).cuda() for xf in frames_of(rc, dims)]
        self.d_xf = torch.from_numpy(initial_xf(rc, dims)).cuda()
        self.d_rays = dev_bytes(torch, self.rays)
        self.d_hits, self.d_any = (torch.zeros(self.n * 32, dtype=torch.uint8, device="cuda") for _ in range(2))
        self.s = torch.cuda.Stream()
        for buf in (self.d_xf, self.d_rays, self.d_hits, self.d_any, *self.frames):
            buf.record_stream(self.s)
        torch.cuda.synchronize()

    def arm(self):
        self.t.refit_or_rebuild_device_async(RATIO, stream=self.s.cuda_stream)  # eager: refit, unconditional rebuild, baseline
        self.s.synchronize()

    def trace(self, st):
        self.t.trace_device(self.d_rays.data_ptr(), self.d_hits.data_ptr(), self.n, stream=st)
        self.t.trace_device(self.d_rays.data_ptr(), self.d_any.data_ptr(), self.n, mode="any", stream=st)

    def frame(self, st):
        self.t.update_transforms_device(self.h, self.d_xf, stream=st)
        self.t.refit_or_rebuild_device_async(RATIO, stream=st)
        self.trace(st)

    def hits(self):
        return hits_of(self.rc, self.d_hits), hits_of(self.rc, self.d_any)


def check_scene(t, ref, what):
    assert t.sync().last_sync_action == "noop", what  # the call left nothing pending
    st = t.adapt()
    took = "rebuilt" if ref.rebuild else "refitted"
    assert st.nodes.tobytes() == ref.nodes, f"{what}: TLAS nodes differ from the twin that {took}"
    assert st.instances.tobytes() == ref.instances, f"{what}: instances"
    b = t.world_bound()
    assert np.concatenate([b.p_min, b.p_max]).tobytes() == ref.bound, f"{what}: world bound"


def check_hits(got, got_any, ref, what):
    assert got.tobytes() == ref.closest, f"{what}: closest hits differ from the twin's"
    assert got_any.tobytes() == ref.any, f"{what}: any hits differ from the twin's"
    assert_hits_equal(got, ref.want.closest, f"{what}: closest vs oracle")
    if ref.rebuild:  # the tree IS the oracle's: the first hit any_hit meets is the same record
        assert_hits_equal(got_any, ref.want.any, f"{what}: any vs oracle")
    else:            # a refitted tree keeps another order: which hit any_hit meets first follows the topology, whether it meets one does not
        assert np.array_equal(got_any["hit"], ref.want.any["hit"]), f"{what}: any vs oracle, hit word"


def check_quality(t, ref, evaluations, rebuilds, what):
    q = t.tlas_quality()
    print(f"{what}: {q}")
    assert q["armed"] and q["evaluations"] == evaluations and q["rebuilds"] == rebuilds, (what, q)
    assert q["last_rebuilt"] == ref.rebuild, (what, q)
    assert close(q["cost"], ref.cost), (what, q["cost"], ref.cost)
    assert close(q["cost_built"], ref.cost_built), (what, q["cost_built"], ref.cost_built)


def check_frame(a, ref, f, refs, what):
    got, got_any = a.hits()
    check_hits(got, got_any, ref, what)
    check_scene(a.t, ref, what)
    check_quality(a.t, ref, 2 + f, 1 + sum(r.rebuild for r in refs[:f + 1]), what)


# ---- 1. the cost ---------------------------------------------------------------------------------------------------------------------------
def device_cost(torch, t, s, out=None):
    out = torch.zeros(1, dtype=torch.float64, device="cuda") if out is None else out
    t.tlas_cost_device(out, stream=s.cuda_stream)
    s.synchronize()
    return out.cpu().numpy().copy()


@pytest.mark.parametrize("dims, fused", PATHS, ids=PATH_IDS)
def test_cost_matches_numpy(rc, oracle, dims, fused):
    import torch
    a = Anim(rc, dims, fused)
    n = len(a.frames[0])
    s = a.s

    def expect(what):
        want = model.cost(a.t.adapt().nodes, n)
        got, again = device_cost(torch, a.t, s), device_cost(torch, a.t, s)
        print(f"{what}: device {got[0]!r}, numpy {want!r}")
        assert close(float(got[0]), want), (what, got, want)
        assert got.tobytes() == again.tobytes(), f"{what}: two evaluations of one tree differ"
        return want

    c0 = expect("after sync")
    with torch.cuda.stream(s):
        a.d_xf.copy_(a.frames[1])  # the shuffled frame, refitted: a degraded tree
        a.t.update_transforms_device(a.h, a.d_xf, stream=s.cuda_stream)
        a.t.refit_device_async(stream=s.cuda_stream)
    s.synchronize()
    c1 = expect("after an asynchronous refit of the shuffled frame")
    assert c1 >= model.SHUFFLE_RATIO_MIN * c0
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    out.record_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        a.t.tlas_cost_device(out, stream=torch.cuda.current_stream().cuda_stream)
    a.t.rebuild_device_async(stream=s.cuda_stream)
    s.synchronize()
    c2 = expect("after a rebuild")
    assert c2 < 0.5 * c1
    out.zero_()
    with torch.cuda.stream(s):
        g.replay()  # captured on the degraded tree, replayed on the rebuilt one: reads the tree as it is when it runs
    s.synchronize()
    assert close(float(out.cpu()[0]), c2), "a replayed cost call returns the current tree's cost"
    del g
    q = a.t.tlas_quality()
    assert not q["armed"] and q["evaluations"] == 0 and q["rebuilds"] == 0  # the cost call and the plain rebuild leave the state alone


def test_cost_of_two_and_of_one_instance(rc):
    import torch
    s = torch.cuda.Stream()
    xf = initial_xf(rc, SMALL)
    for n in (2, 1):
        t = rc.TLAS()
        t.push(sphere(rc), xf[:n], instance_ids=np.arange(n, dtype=np.uint32))
        t.sync()
        assert device_cost(torch, t, s)[0] == 1.0, n
        t.refit_or_rebuild_device_async(0.5, stream=s.cuda_stream)  # arms
        t.refit_or_rebuild_device_async(0.5, stream=s.cuda_stream)  # cost 1.0 > 0.5 * 1.0: two instances rebuild, one never does
        s.synchronize()
        q = t.tlas_quality()
        assert q["cost"] == 1.0 and q["cost_built"] == 1.0 and q["evaluations"] == 2, (n, q)
        assert q["rebuilds"] == (2 if n == 2 else 1) and q["last_rebuilt"] == (n == 2), (n, q)
        twin = fresh_twin(rc, xf[:n])
        assert t.sync().last_sync_action == "noop"
        assert t.adapt().nodes.tobytes() == twin.adapt().nodes.tobytes()


# ---- 2. copy -> update -> refit_or_rebuild -> trace on one stream, no host wait inside a frame ---------------------------------------------------
@pytest.mark.parametrize("dims, fused", PATHS, ids=PATH_IDS)
def test_eager_frames(rc, oracle, dims, fused):
    import torch
    refs, armed_cost = track(rc, oracle, dims)
    a = Anim(rc, dims, fused)
    assert not a.t.tlas_quality()["armed"]
    a.arm()
    q = a.t.tlas_quality()
    assert q["armed"] and q["evaluations"] == 1 and q["rebuilds"] == 1 and q["last_rebuilt"], q
    assert close(q["cost_built"], armed_cost) and close(q["cost"], armed_cost), (q, armed_cost)
    for f, ref in enumerate(refs):
        with torch.cuda.stream(a.s):
            a.d_xf.copy_(a.frames[f])  # the transforms are produced on the stream too
            a.frame(a.s.cuda_stream)
        a.s.synchronize()
        check_frame(a, ref, f, refs, f"eager frame {f} ({model.KINDS[f]})")


# ---- 3. one graph, both decisions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims, fused", PATHS, ids=PATH_IDS)
def test_one_graph_takes_both_decisions(rc, oracle, dims, fused):
    import torch
    refs, _ = track(rc, oracle, dims)
    a = Anim(rc, dims, fused)
    a.arm()
    with torch.cuda.stream(a.s):
        a.trace(a.s.cuda_stream)  # the traces run eagerly once on the stream; the arming call was the conditional call's eager run
    a.s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=a.s):
        a.frame(torch.cuda.current_stream().cuda_stream)
    assert a.t.tlas_quality()["evaluations"] == 1  # capturing runs nothing
    for f, ref in enumerate(refs):
        a.d_hits.zero_(); a.d_any.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(a.s):
            a.d_xf.copy_(a.frames[f])  # in place: the graph reads the tensor when it runs
            g.replay()
        a.s.synchronize()
        check_frame(a, ref, f, refs, f"replay {f} ({model.KINDS[f]})")
    del g
    a.t.set_option("release_captures", 1)


# ---- 4. a refit after a gated rebuild walks the new topology ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims, fused", PATHS, ids=PATH_IDS)
def test_earlier_capture_refits_the_gated_rebuilds_topology(rc, oracle, dims, fused):
    import torch
    refs, _ = track(rc, oracle, dims)
    a = Anim(rc, dims, fused)
    a.arm()

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
        for f in (0, 1):  # drift, then the shuffle: the gate opens and the rebuild runs, eagerly, between the old graph's replays
            a.d_xf.copy_(a.frames[f])
            a.frame(a.s.cuda_stream)
    a.s.synchronize()
    assert a.t.tlas_quality()["rebuilds"] == 2
    check_scene(a.t, refs[1], "the gated rebuild")
    a.d_hits.zero_(); a.d_any.zero_()
    torch.cuda.synchronize()
    with torch.cuda.stream(a.s):
        a.d_xf.copy_(a.frames[2])
        g.replay()  # the OLD graph: update + refit + traces, now on frame 1's topology
    a.s.synchronize()
    got, got_any = a.hits()
    check_hits(got, got_any, refs[2], "replay of the earlier refit capture after the gated rebuild")
    check_scene(a.t, refs[2], "replay of the earlier refit capture after the gated rebuild")
    assert a.t.tlas_quality()["evaluations"] == 3  # a plain refit evaluates nothing
    del g
    a.t.set_option("release_captures", 1)


# ---- 5. the baseline follows an explicit rebuild ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims, fused", PATHS, ids=PATH_IDS)
def test_baseline_follows_an_explicit_rebuild(rc, oracle, dims, fused):
    import torch
    refs, armed_cost = track(rc, oracle, dims)
    a = Anim(rc, dims, fused)
    a.arm()
    xf = frames_of(rc, dims)[1]  # (the shuffle applied to frame 0: a fresh twin of its own)
    twin = fresh_twin(rc, xf)
    want = model.cost(twin.adapt().nodes, len(xf))
    assert abs(want - armed_cost) > 1e-6 * armed_cost  # another tree: the baseline has to move
    with torch.cuda.stream(a.s):
        a.d_xf.copy_(a.frames[1])
        a.t.update_transforms_device(a.h, a.d_xf, stream=a.s.cuda_stream)
        a.t.rebuild_device_async(stream=a.s.cuda_stream)
    a.s.synchronize()
    q = a.t.tlas_quality()
    assert close(q["cost_built"], want), (q, want)
    assert q["evaluations"] == 1 and q["rebuilds"] == 2, q
    assert a.t.adapt().nodes.tobytes() == twin.adapt().nodes.tobytes()
    with torch.cuda.stream(a.s):  # ... so a conditional call on the same transforms finds nothing to do
        a.frame(a.s.cuda_stream)
    a.s.synchronize()
    q = a.t.tlas_quality()
    assert q["evaluations"] == 2 and q["rebuilds"] == 2 and not q["last_rebuilt"] and close(q["cost"], want), q
    assert a.hits()[0].tobytes() == twin.trace(a.rays).tobytes()


# ---- 6. the kernels that read the traversal copy from LDS and the renumbered top ------------------------------------------------------------------
@pytest.mark.parametrize("dims, fused, kernel", [(SMALL, 1, 5), (SMALL, 0, 5), (LARGE, 0, 6)], ids=["144-fused-lds_tlas", "144-chain-lds_tlas", "864-chain-renumbered_top"])
def test_lds_kernels_after_both_decisions(rc, oracle, dims, fused, kernel):
    import torch
    refs, _ = track(rc, oracle, dims)
    a = Anim(rc, dims, fused)
    assert (a.t.get_option("tlas_top_k") > 0) == (kernel == 6)
    a.arm()
    for f in (0, 1):  # one that refits, one that rebuilds
        with torch.cuda.stream(a.s):
            a.d_xf.copy_(a.frames[f])
            a.t.update_transforms_device(a.h, a.d_xf, stream=a.s.cuda_stream)
            a.t.refit_or_rebuild_device_async(RATIO, stream=a.s.cuda_stream)
            a.t.set_option("kernel", kernel)
            a.trace(a.s.cuda_stream)
            a.t.set_option("kernel", -1)
        a.s.synchronize()
        got, got_any = a.hits()
        check_hits(got, got_any, refs[f], f"kernel {kernel} after frame {f} ({model.KINDS[f]})")
        assert a.t.tlas_quality()["last_rebuilt"] == refs[f].rebuild


# ---- 7. WavefrontPaths(rebuild="auto") --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
def test_wavefront_auto_frame(rc, oracle, fused):
    import torch
    from raycore_jl_amd.wavefront import WavefrontPaths, lookat_camera
    dims = SMALL
    refs, _ = track(rc, oracle, dims)  # (the frames' inputs are the ones checked there)
    t, (h,), _ = make_scene(rc, dims)
    t.set_option("tlas_rebuild_fused", fused)
    ext = (np.array(dims, dtype=np.float64) - 1) * 1.8
    cam = lookat_camera(ext / 2 + np.array([0.45, 0.3, 1.0]) * (0.95 * ext[:2].max() + 3.0), ext / 2, 64, 48)
    light = np.array([ext[0] / 2, ext[1] + 8.0, ext[2] + 6.0], dtype=np.float32)
    xfs = frames_of(rc, dims)[:3]  # drift, shuffle, drift
    frames = [torch.from_numpy(xf).cuda() for xf in xfs]
    d_xf = torch.from_numpy(initial_xf(rc, dims)).cuda()
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        WavefrontPaths(t, 64, 48, 2, 2, cam, light, seed=11, rebuild="auto")
    dyn = WavefrontPaths(t, 64, 48, 2, 2, cam, light, seed=11, dynamic=[(h, d_xf)], rebuild="auto")
    assert dyn.rebuild == "auto" and dyn.rebuild_ratio == 1.5
    q = t.tlas_quality()
    assert q["armed"] and q["rebuilds"] == 1  # the constructor armed
    s = torch.cuda.Stream()
    dyn.run(s)  # eager once (the initial transforms: nothing to rebuild), then the capture
    torch.cuda.synchronize()
    assert t.tlas_quality()["rebuilds"] == 1
    dyn.capture(s)
    ths = []
    twin = fresh_twin(rc, initial_xf(rc, dims), handles=ths)
    rebuilds = 1
    for f in range(3):
        if refs[f].rebuild:
            ths = []
            twin = fresh_twin(rc, xfs[f], handles=ths)
        else:
            twin.update_transforms(ths[0], xfs[f])
            assert twin.sync().last_sync_action == "refit"
        for buf in dyn.hits + dyn.shadow_hits:
            buf.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            d_xf.copy_(frames[f])
            dyn.replay()
        torch.cuda.synchronize()
        ref = WavefrontPaths(twin, 64, 48, 2, 2, cam, light, seed=11)
        ref.run(s)
        torch.cuda.synchronize()
        what = f"replayed frame {f} ({model.KINDS[f]})"
        alive = 0
        for b in range(2):
            for name in ("rays", "hits", "shadow_hits", "path_ids"):
                assert torch.equal(getattr(dyn, name)[b], getattr(ref, name)[b]), f"{what}: {name}[{b}] differs from the static frame on the matching twin"
            alive += int(np.count_nonzero(hits_of(rc, dyn.hits[b])["hit"]))
        assert alive > 0.1 * dyn.n, what
        rebuilds += int(refs[f].rebuild)
        assert t.tlas_quality()["rebuilds"] == rebuilds, what
        assert t.adapt().nodes.tobytes() == refs[f].nodes, what
    assert rebuilds == 2
    dyn.graph = None
    torch.cuda.synchronize()
    t.set_option("release_captures", 1)


# ---- 8. errors leave the scene usable ---------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_scene_usable(rc, oracle):
    import torch
    dims = SMALL
    refs, _ = track(rc, oracle, dims)
    a = Anim(rc, dims, 1)
    L = rc.lib()
    n = len(a.frames[0])

    def normal_frame(f, what):
        with torch.cuda.stream(a.s):
            a.d_xf.copy_(a.frames[f])
            a.frame(a.s.cuda_stream)
        a.s.synchronize()
        got, got_any = a.hits()
        check_hits(got, got_any, refs[f], what)
        check_scene(a.t, refs[f], what)

    # the first call on a capturing stream: refused, the capture ends cleanly, the scene still traces
    base = a.t.trace(a.rays).tobytes()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=a.s):
        st = torch.cuda.current_stream().cuda_stream
        assert L.rc_refit_or_rebuild_tlas_device_async(a.t._h, RATIO, st) == RC_ERR_NOT_SYNCED
        assert "eager" in L.rc_last_error().decode()
        a.d_hits.zero_()  # (something to capture)
    with torch.cuda.stream(a.s):
        g.replay()
    a.s.synchronize()
    del g
    assert not a.t.tlas_quality()["armed"] and a.t.trace(a.rays).tobytes() == base
    a.arm()
    normal_frame(0, "after the refused capture")
    # ratio
    for bad in (float("nan"), 0.0, -1.0, float("inf")):
        assert L.rc_refit_or_rebuild_tlas_device_async(a.t._h, bad, None) == RC_ERR_INVALID_ARGUMENT
        assert "ratio" in L.rc_last_error().decode()
    assert L.rc_refit_or_rebuild_tlas_device_async(None, RATIO, None) == RC_ERR_INVALID_ARGUMENT
    q = a.t.tlas_quality()
    assert q["evaluations"] == 2  # nothing was enqueued
    normal_frame(1, "after the refused ratios")
    # pending host-side mutations
    one = a.t.push(sphere(rc), rc.scenes.IDENTITY3x4.reshape(1, 12), instance_ids=np.array([7777], dtype=np.uint32))
    assert L.rc_refit_or_rebuild_tlas_device_async(a.t._h, RATIO, None) == RC_ERR_NOT_SYNCED
    assert "rc_sync" in L.rc_last_error().decode()
    with pytest.raises(rc.RaycoreError) as e:
        a.t.refit_or_rebuild_device_async(RATIO)
    assert e.value.code == RC_ERR_NOT_SYNCED
    assert L.rc_tlas_cost_device(a.t._h, a.d_hits.data_ptr(), None) == RC_ERR_NOT_SYNCED
    assert a.t.delete(one)
    assert a.t.sync().last_sync_action == "rebuild"  # structural: the state is disarmed and zeroed
    q = a.t.tlas_quality()
    assert not q["armed"] and q["evaluations"] == 0 and q["rebuilds"] == 0 and q["cost_built"] == 0.0, q
    same = a.t.get_instances(a.h)["transform"].copy()
    a.t.update_transforms(a.h, same)
    assert L.rc_refit_or_rebuild_tlas_device_async(a.t._h, RATIO, None) == RC_ERR_NOT_SYNCED
    assert a.t.sync().last_sync_action == "refit"
    a.arm()
    normal_frame(2, "after the pending mutations")
    # never synced
    fresh = rc.TLAS()
    fresh.push(sphere(rc), initial_xf(rc, dims), instance_ids=np.arange(n, dtype=np.uint32))
    assert L.rc_refit_or_rebuild_tlas_device_async(fresh._h, RATIO, None) == RC_ERR_NOT_SYNCED
    assert L.rc_tlas_cost_device(fresh._h, a.d_hits.data_ptr(), None) == RC_ERR_NOT_SYNCED
    fresh.sync()
    fresh.refit_or_rebuild_device_async(RATIO)
    assert fresh.trace(a.rays).tobytes() == base
    # a scene with no instances: success, nothing enqueued
    empty = rc.TLAS()
    empty.add_geometry(sphere(rc))
    empty.sync()
    assert L.rc_refit_or_rebuild_tlas_device_async(empty._h, RATIO, None) == 0
    assert L.rc_tlas_cost_device(empty._h, a.d_hits.data_ptr(), None) == 0
    assert empty.sync().last_sync_action == "noop" and not empty.tlas_quality()["armed"]
    normal_frame(3, "after everything")
    torch.cuda.synchronize()
