"""Device-side geometry update: update_geometry_device_async / update_mesh_vertices_device_async (rc_update_geometry_device_async,
rc_update_mesh_vertices_device_async) on the GPU.

Two yardsticks, neither of them the code under test:

* the ORACLE FROM SCRATCH: oracle.pyoracle.Scene built anew with the frame's soup;
* a FRESH TWIN: a new rc.TLAS() with the same pushes and the frame's soup, built by the structural sync.

Frame f (0..3) deforms a fan_sphere soup of radius 0.5, in float64: every vertex is rotated about z by (0.8 + 0.5 f) z / 0.5 rad, x is
scaled by 1 + 0.4 f and z by 1 - 0.15 f, the result is cast to f32 and the face order is rolled by 7 (f + 1) -- which pins the default
face-index metadata (assigned before the degenerate filter).  Conditions on the inputs, asserted on the oracle's output alone and
printed (want_frame): the primitive count is unchanged, >= 0.9 of the BLAS's leaf slots hold other metadata than in the previous frame,
hit fraction >= 0.2, >= 0.3 of the hit records differ from the previous frame's.

Compared byte for byte with both yardsticks: BLAS nodes, primitives and descriptors, instances, world bound, closest hits; after a
rebuild_device_async also the TLAS nodes and the any hits.

After a REFIT the TLAS keeps the topology of the last sync -- that is what a refit is -- while both yardsticks sort their instances anew.
The oracle shows that frames 1..3 change the Morton order of the lattice (the root box of the BLAS moves the scene bounds: printed by
want_frame as "TLAS topology as initially").  So after a refit the TLAS nodes and the any hits (whose record depends on the visit
order) are compared with the from-scratch yardsticks whenever the ORACLE's own topology of that frame equals its initial one, and
otherwise with a restatement of the refit on the oracle's data (refit_restatement: the oracle's initial tree, the oracle's new leaf
boxes, unions bottom-up) resp. on the `hit` word alone; the same scene then gets a rebuild_device_async and must equal both yardsticks
in full.

WHICH KERNEL RUNS HERE: kernel 0 (option `kernel` at -1, 65 536 rays: test_gpu_dynamic.py's docstring has the arithmetic).  It reads the
BLAS slices of the traversal copy from memory in their renumbered order, but neither the entry-cull spheres and the per-BLAS cull radius
nor the prefixes kernels 5 and 6 stage into LDS.  Those, kernels 3, 5 and 6 after every frame, and a captured update of a BLAS of more
than 1 024 primitives ("top") are in tests/test_gpu_update_kernels.py.
"""
import ctypes as C

import numpy as np
import pytest

from dynamic_kit import Spec, Want, deform, dev_bytes, frame_xf, hits_of, want_frame
from gpu_kit import rc  # noqa: F401
from helpers import assert_hits_equal

pytestmark = pytest.mark.gpu

N_FRAMES = 4
RC_ERR_INVALID_ARGUMENT, RC_ERR_INVALID_HANDLE, RC_ERR_NOT_SYNCED, RC_ERR_GEOMETRY_CHANGED = 1, 2, 6, 8
EXPORTS = ("nodes", "instances", "all_blas_nodes", "all_blas_prims", "blas_descriptors")


def refit_restatement(topo, fresh):
    """The TLAS a refit must leave: the tree `topo` (the oracle's, of the scene as last synced) with the leaf boxes of `fresh` (the
    oracle's from scratch; a leaf names its instance in child1) and, in every internal node, the boxes of its two children."""
    n = (len(topo) + 1) // 2
    out = topo.copy()
    fresh_leaf = {int(fresh["child1"][j]): j for j in range(n - 1, 2 * n - 1)}
    box = {}
    for j in range(n - 1, 2 * n - 1):
        src = fresh_leaf[int(topo["child1"][j])]
        out["aabb0_min"][j], out["aabb0_max"][j] = fresh["aabb0_min"][src], fresh["aabb0_max"][src]
        box[j + 1] = (out["aabb0_min"][j].copy(), out["aabb0_max"][j].copy())

    def visit(k):  # 1-based node index -> its box
        if k not in box:
            (mn0, mx0), (mn1, mx1) = visit(int(topo["child0"][k - 1])), visit(int(topo["child1"][k - 1]))
            out["aabb0_min"][k - 1], out["aabb0_max"][k - 1], out["aabb1_min"][k - 1], out["aabb1_max"][k - 1] = mn0, mx0, mn1, mx1
            box[k] = (np.minimum(mn0, mn1), np.maximum(mx0, mx1))
        return box[k]

    visit(1)
    return out


def assert_geometry(t, want, twin, what):
    """Everything but the TLAS nodes: BLAS nodes, primitives, descriptors, instances, world bound."""
    st, sw = t.adapt(), twin.adapt()
    for name, w in (("all_blas_nodes", want.blas_nodes), ("all_blas_prims", want.blas_prims), ("blas_descriptors", want.blas_descs),
                    ("instances", want.instances)):
        got = getattr(st, name).tobytes()
        assert got == w.tobytes(), f"{what}: {name} differ from the oracle built from scratch"
        assert got == getattr(sw, name).tobytes(), f"{what}: {name} differ from the fresh twin"
    b, bw = t.world_bound(), twin.world_bound()
    got = np.concatenate([b.p_min, b.p_max]).tobytes()
    assert got == want.bound.tobytes(), f"{what}: world bound vs oracle"
    assert got == np.concatenate([bw.p_min, bw.p_max]).tobytes(), f"{what}: world bound vs twin"


def assert_frame(t, want, twin, rays, got, got_any, what, tlas_as_fresh=True, refit_nodes=None):
    assert_hits_equal(got, want.closest, f"{what}: closest vs oracle")
    assert got.tobytes() == twin.trace(rays).tobytes(), f"{what}: closest hits differ from the fresh twin"
    assert t.sync().last_sync_action == "noop", what  # the asynchronous update + commit left nothing pending
    assert_geometry(t, want, twin, what)
    nodes = t.adapt().nodes.tobytes()
    if tlas_as_fresh:
        assert_hits_equal(got_any, want.any, f"{what}: any vs oracle")
        assert got_any.tobytes() == twin.trace(rays, mode="any").tobytes(), f"{what}: any hits differ from the fresh twin"
        assert nodes == want.nodes.tobytes(), f"{what}: TLAS nodes differ from the oracle built from scratch"
        assert nodes == twin.adapt().nodes.tobytes(), f"{what}: TLAS nodes differ from the fresh twin"
    else:
        assert np.array_equal(got_any["hit"], want.any["hit"]), f"{what}: any-hit occlusion vs oracle"
        assert nodes == refit_nodes.tobytes(), f"{what}: TLAS nodes differ from the refit restated on the oracle's data"


class Device:
    """Rays, hit buffers and a stream for one scene."""

    def __init__(self, rc, rays):
        import torch
        self.torch, self.rc, self.rays, self.n = torch, rc, rays, len(rays)
        self.d_rays = dev_bytes(torch, rays)
        self.d_hits, self.d_any = (torch.zeros(self.n * 32, dtype=torch.uint8, device="cuda") for _ in range(2))
        self.s = torch.cuda.Stream()
        for buf in (self.d_rays, self.d_hits, self.d_any):
            buf.record_stream(self.s)
        torch.cuda.synchronize()

    @property
    def st(self):
        return self.s.cuda_stream

    def soup(self, a):
        d = self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
        d.record_stream(self.s)
        self.torch.cuda.synchronize()
        return d

    def trace(self, t):
        t.trace_device(self.d_rays.data_ptr(), self.d_hits.data_ptr(), self.n, stream=self.st)
        t.trace_device(self.d_rays.data_ptr(), self.d_any.data_ptr(), self.n, mode="any", stream=self.st)

    def hits(self):
        self.s.synchronize()
        return hits_of(self.rc, self.d_hits), hits_of(self.rc, self.d_any)


# ---- 1. byte for byte, frame by frame -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("commit", ["refit", "rebuild"])
@pytest.mark.parametrize("name", ["144", "864", "top", "two"])
def test_update_commit_trace(rc, oracle, name, commit):
    spec = Spec(rc, name)
    t, hs = spec.build(rc)
    assert (t.get_option("blas_top_k") > 0) == (len(spec.soups) == 1)  # the renumbering of the BLAS's top exists in single-BLAS scenes
    if name == "top":
        assert 0 < t.get_option("blas_top_k") < len(spec.soups[0]) - 1  # ... and here it is a proper part of the tree
    dv = Device(rc, spec.rays)
    first = want_frame(oracle, rc, spec, -1)
    other = None
    if name == "two":
        st = t.adapt()
        d1 = st.blas_descriptors[1]
        other = (st.all_blas_nodes[d1["nodes_offset"]:].tobytes(), st.all_blas_prims[d1["primitives_offset"]:].tobytes())
    branches = set()
    for f in range(N_FRAMES):
        want = want_frame(oracle, rc, spec, f)
        twin, _ = spec.build(rc, f)
        d_soup = dv.soup(deform(spec.soups[0], f))
        t.update_geometry_device_async(hs[-1], d_soup if f % 2 == 0 else d_soup.reshape(-1, 3, 3), stream=dv.st)  # (through the LAST handle of the BLAS)
        with pytest.raises(rc.RaycoreError) as e:  # transforms-dirty from the device: no query before the commit
            t.trace(spec.rays[:4])
        assert e.value.code == RC_ERR_NOT_SYNCED
        if commit == "refit":
            t.refit_device_async(stream=dv.st)
        else:
            t.rebuild_device_async(stream=dv.st)
        dv.trace(t)
        got, got_any = dv.hits()
        t.wait_for_gpu()  # (no status pending)
        as_fresh = commit == "rebuild" or want.same_topology(first)
        branches.add(as_fresh)
        assert_frame(t, want, twin, spec.rays, got, got_any, f"{name} {commit} frame {f}", as_fresh,
                     None if as_fresh else refit_restatement(first.nodes, want.nodes))
        if not as_fresh:  # the same scene, rebuilt in place: now the from-scratch yardsticks apply in full
            t.rebuild_device_async(stream=dv.st)
            dv.trace(t)
            got, got_any = dv.hits()
            assert_frame(t, want, twin, spec.rays, got, got_any, f"{name} refit + rebuild frame {f}")
            first = want  # (the topology later refits keep)
        if other is not None:
            st = t.adapt()
            assert (st.all_blas_nodes[d1["nodes_offset"]:].tobytes(), st.all_blas_prims[d1["primitives_offset"]:].tobytes()) == other, "the other BLAS's slices"
    assert branches == ({True, False} if commit == "refit" else {True}), "a refit must meet a frame that keeps the oracle's topology and one that changes it"
    # a structural sync after an unrelated push copies from the geometry's own arrays and the lazily refreshed root box
    extra = spec.soups[0][:4] + np.float32(0.25)
    for scene in (t, twin):
        scene.push(extra, np.eye(4, dtype=np.float32))
        assert scene.sync().last_sync_action == "rebuild"
    for ex in EXPORTS:
        assert getattr(t.adapt(), ex).tobytes() == getattr(twin.adapt(), ex).tobytes(), f"{name} {commit}: {ex} after a structural sync"
    assert t.trace(spec.rays).tobytes() == twin.trace(spec.rays).tobytes()
    assert t.trace(spec.rays, mode="any").tobytes() == twin.trace(spec.rays, mode="any").tobytes()


# ---- 2. degenerate faces in the soup: n exceeds the primitive count ------------------------------------------------------------------------
def test_degenerate_faces_keep_the_count(rc, oracle):
    spec = Spec(rc, "poles")
    t, (h,) = spec.build(rc)
    dv = Device(rc, spec.rays)
    first = want_frame(oracle, rc, spec, -1)
    n_faces = len(spec.soups[0])
    assert len(first.blas_prims) == n_faces - 22  # one face of every pole quad is degenerate
    for f in (1, 3):
        want = want_frame(oracle, rc, spec, f)  # (asserts the count on the oracle)
        assert len(want.blas_prims) == len(first.blas_prims) < n_faces
        twin, _ = spec.build(rc, f)
        t.update_geometry_device_async(h, dv.soup(deform(spec.soups[0], f)), stream=dv.st)
        t.rebuild_device_async(stream=dv.st)
        dv.trace(t)
        got, got_any = dv.hits()
        t.wait_for_gpu()
        assert_frame(t, want, twin, spec.rays, got, got_any, f"poles frame {f}")


# ---- 3. a soup with another face count changes nothing and is reported once ----------------------------------------------------------------
def test_count_mismatch_is_reported_and_changes_nothing(rc, oracle):
    spec = Spec(rc, "144")
    t, (h,) = spec.build(rc)
    dv = Device(rc, spec.rays)
    t.update_geometry_device_async(h, dv.soup(deform(spec.soups[0], 0)), stream=dv.st)
    t.refit_device_async(stream=dv.st)
    dv.s.synchronize()
    before = {ex: getattr(t.adapt(), ex).tobytes() for ex in EXPORTS}
    hits_before = (t.trace(spec.rays).tobytes(), t.trace(spec.rays, mode="any").tobytes())
    bound_before = t.world_bound()
    bad = deform(spec.soups[0], 1).copy()
    bad[3, 6:9] = bad[3, 3:6]  # two equal vertices: (v1 - v0) x (v1 - v0) == 0 exactly
    o = oracle.Scene()
    o.add_instance(o.add_blas(bad))
    o.build()
    assert len(o.blas_prims) == len(bad) - 1  # the oracle's filter drops exactly that face
    for soup in (bad, np.zeros((5, 9), np.float32)):  # one face short; no valid face at all
        t.update_geometry_device_async(h, dv.soup(soup), stream=dv.st)
        t.refit_device_async(stream=dv.st)
        dv.trace(t)
        got, got_any = dv.hits()
        with pytest.raises(rc.RaycoreError) as e:
            t.wait_for_gpu()
        assert e.value.code == RC_ERR_GEOMETRY_CHANGED
        t.wait_for_gpu()  # reported once
        assert t.sync().last_sync_action == "noop"
        assert (got.tobytes(), got_any.tobytes()) == hits_before
        for ex in EXPORTS:
            assert getattr(t.adapt(), ex).tobytes() == before[ex], ex
        b = t.world_bound()
        assert b.p_min.tobytes() == bound_before.p_min.tobytes() and b.p_max.tobytes() == bound_before.p_max.tobytes()
        assert (t.trace(spec.rays).tobytes(), t.trace(spec.rays, mode="any").tobytes()) == hits_before
    want = want_frame(oracle, rc, spec, 2)  # the next valid update works
    twin, _ = spec.build(rc, 2)
    t.update_geometry_device_async(h, dv.soup(deform(spec.soups[0], 2)), stream=dv.st)
    t.rebuild_device_async(stream=dv.st)
    dv.trace(t)
    got, got_any = dv.hits()
    t.wait_for_gpu()
    assert_frame(t, want, twin, spec.rays, got, got_any, "after a refused update")


# ---- 4. update -> update_transforms_device -> refit -> trace as one graph ------------------------------------------------------------------
def test_graph_replay_per_frame(rc, oracle):
    import torch
    spec = Spec(rc, "144")
    t, (h,) = spec.build(rc)
    dv = Device(rc, spec.rays)
    frames = [(dv.soup(deform(spec.soups[0], f)), dv.soup(frame_xf(rc, spec.dims, f))) for f in range(N_FRAMES)]
    d_soup, d_xf = frames[0][0].clone(), frames[0][1].clone()
    d_plain = torch.zeros(dv.n * 32, dtype=torch.uint8, device="cuda")
    for buf in (d_soup, d_xf, d_plain):
        buf.record_stream(dv.s)
    torch.cuda.synchronize()

    def want_of(f):
        for k in range(f + 1):
            want_frame(oracle, rc, spec, k)  # (the soups are the ones whose conditions are checked above)
        return Want(oracle, spec.soups_of(f), spec.owner, frame_xf(rc, spec.dims, f), spec.rays)

    def frame():
        t.update_geometry_device_async(h, d_soup, stream=dv.st)
        t.update_transforms_device(h, d_xf, stream=dv.st)
        t.refit_device_async(stream=dv.st)
        dv.trace(t)

    with torch.cuda.stream(dv.s):
        t.trace_device(dv.d_rays.data_ptr(), d_plain.data_ptr(), dv.n, stream=dv.st)  # eager first
    dv.s.synchronize()
    plain = torch.cuda.CUDAGraph()  # a plain trace, captured before the first update
    with torch.cuda.graph(plain, stream=dv.s):
        t.trace_device(dv.d_rays.data_ptr(), d_plain.data_ptr(), dv.n, stream=torch.cuda.current_stream().cuda_stream)
    with torch.cuda.stream(dv.s):
        frame()  # eager first
    got, _ = dv.hits()
    assert_hits_equal(got, want_of(0).closest, "eager frame vs oracle")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=dv.s):
        frame()
    for f in (1, 2, 3, 0):
        want = want_of(f)
        dv.d_hits.zero_(); dv.d_any.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(dv.s):
            d_soup.copy_(frames[f][0])  # in place: the graph reads the tensors when it runs
            d_xf.copy_(frames[f][1])
            g.replay()
        got, got_any = dv.hits()
        assert_hits_equal(got, want.closest, f"replay of frame {f} vs oracle")
        assert np.array_equal(got_any["hit"], want.any["hit"]), f"replay of frame {f}: occlusion"
        st = t.adapt()  # the host copies are re-read while the graph may live
        assert st.all_blas_nodes.tobytes() == want.blas_nodes.tobytes() and st.all_blas_prims.tobytes() == want.blas_prims.tobytes(), f
        assert st.blas_descriptors.tobytes() == want.blas_descs.tobytes() and st.instances.tobytes() == want.instances.tobytes(), f
        b = t.world_bound()
        assert np.concatenate([b.p_min, b.p_max]).tobytes() == want.bound.tobytes(), f
        d_plain.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(dv.s):
            plain.replay()
        dv.s.synchronize()
        assert_hits_equal(hits_of(rc, d_plain), want.closest, f"the earlier plain-trace graph after frame {f}")
    t.wait_for_gpu()
    del g, plain
    t.set_option("release_captures", 1)
    assert t.sync().last_sync_action == "noop"
    assert_hits_equal(t.trace(spec.rays), want.closest, "after the graphs are gone")


# ---- 5. WavefrontPaths(deform=...) -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["deform", "deform+dynamic+rebuild"])
def test_wavefront_deform_frame(rc, oracle, mode):
    import torch
    from raycore_jl_amd.wavefront import WavefrontPaths, lookat_camera
    spec = Spec(rc, "144")
    t, (h,) = spec.build(rc)
    for f in range(N_FRAMES):
        want_frame(oracle, rc, spec, f)  # (the frames' inputs are the ones checked above)
    ext = (np.array(spec.dims, dtype=np.float64) - 1) * 1.8
    cam = lookat_camera(ext / 2 + np.array([0.45, 0.3, 1.0]) * (0.95 * ext[:2].max() + 3.0), ext / 2, 64, 48)
    light = np.array([ext[0] / 2, ext[1] + 8.0, ext[2] + 6.0], dtype=np.float32)
    moving = mode != "deform"
    xf_of = (lambda f: frame_xf(rc, spec.dims, f)) if moving else (lambda f: spec.xf)
    soups = [torch.from_numpy(deform(spec.soups[0], f)).cuda() for f in range(N_FRAMES)]
    xfs = [torch.from_numpy(xf_of(f)).cuda() for f in range(N_FRAMES)]
    d_soup, d_xf = soups[0].clone(), xfs[0].clone()
    torch.cuda.synchronize()
    kw = {"dynamic": [(h, d_xf)], "rebuild": True} if moving else {}
    dyn = WavefrontPaths(t, 64, 48, 2, 2, cam, light, seed=11, deform=[(h, d_soup)], **kw)
    assert any(b is d_soup for b in dyn.buffers())
    s = torch.cuda.Stream()

    def compare(f, what):
        """The same frame, static, on a scene built from scratch with the frame's soup and transforms.  After a refit (mode "deform") the
        tree is not the fresh one: the shadow stage's any-hit records are then compared on their `hit` word."""
        torch.cuda.synchronize()
        twin, _ = spec.build(rc, f, xf_of(f))
        ref = WavefrontPaths(twin, 64, 48, 2, 2, cam, light, seed=11)
        ref.run(s)
        torch.cuda.synchronize()
        alive = 0
        for b in range(2):
            for name in ("rays", "hits", "path_ids"):
                assert torch.equal(getattr(dyn, name)[b], getattr(ref, name)[b]), f"{what}: {name}[{b}] differs from the static frame on a scene built from scratch"
            x, y = hits_of(rc, dyn.shadow_hits[b]), hits_of(rc, ref.shadow_hits[b])
            assert np.array_equal(x["hit"], y["hit"]), f"{what}: shadow_hits[{b}]"
            if moving:
                assert x.tobytes() == y.tobytes(), f"{what}: shadow_hits[{b}] records"
            alive += int(np.count_nonzero(hits_of(rc, dyn.hits[b])["hit"]))
        assert alive > 0.1 * dyn.n, what
        assert t.adapt().all_blas_nodes.tobytes() == twin.adapt().all_blas_nodes.tobytes(), what
        if moving:
            assert t.adapt().nodes.tobytes() == twin.adapt().nodes.tobytes(), what

    for f in range(N_FRAMES):  # eager
        with torch.cuda.stream(s):
            d_soup.copy_(soups[f]); d_xf.copy_(xfs[f])
            dyn.run(s)
        compare(f, f"eager frame {f}")
    dyn.capture(s)
    for f in (1, 3, 0):  # replayed
        for buf in dyn.hits + dyn.shadow_hits:
            buf.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            d_soup.copy_(soups[f]); d_xf.copy_(xfs[f])
            dyn.replay()
        compare(f, f"replayed frame {f}")
    dyn.graph = None
    torch.cuda.synchronize()
    t.set_option("release_captures", 1)


# ---- 6. the mesh form ------------------------------------------------------------------------------------------------------------------
def test_mesh_vertices(rc, oracle):
    import torch
    from scene_kit import grid_mesh
    v, f, nrm, uv = grid_mesh(24, seed=3)
    f[17] = [5, 5, 5]      # degenerate by index: whatever the vertices do
    f[100] = [7, 8, 7]
    fm = np.arange(1000, 1000 + len(v), dtype=np.uint32)
    soup = np.array([[0, 0, 3, 1, 0, 3, 0, 1, 3], [0, 0, 4, 2, 0, 4, 0, 2, 4]], np.float32)
    t = rc.TLAS()
    h = t.push_mesh(v, f, nrm, uvs=uv, face_meta=fm)
    t.push(soup, meta=[11, 12])
    t.sync()
    g = np.random.default_rng(5)
    n = 40000
    org = np.c_[g.random((n, 2)) * 1.2 - 0.1, np.full(n, 3.5)].astype(np.float32)
    rays = rc.scenes.make_rays(org, np.tile([0, 0, -1], (n, 1)))
    s = torch.cuda.Stream()
    d_n = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    d_uv = torch.zeros((n, 2), dtype=torch.float32, device="cuda")

    def check(v_now, nrm_now, what, extra=None):
        o = oracle.Scene()
        o.add_instance(o.add_mesh(v_now, f, nrm_now, uv, fm))
        o.add_instance(o.add_blas(soup, [11, 12]))
        if extra is not None:
            o.add_instance(o.add_blas(extra))
        o.build()
        st = t.adapt()
        assert st.all_blas_nodes.tobytes() == o.blas_nodes.tobytes(), f"{what}: BLAS nodes"
        assert st.all_blas_triangles.tobytes() == o.triangles.tobytes(), f"{what}: triangles"
        assert st.blas_descriptors.tobytes() == o.blas_descs.tobytes(), f"{what}: descriptors"
        hits = t.trace(rays)
        assert_hits_equal(hits, o.trace(rays, nthreads=4), f"{what}: closest")
        assert 0.2 * n < hits["hit"].sum() < n
        d_h = dev_bytes(torch, hits)
        d_n.fill_(7.0); d_uv.fill_(7.0)
        torch.cuda.synchronize()
        t.shading_attributes_device(d_h.data_ptr(), n, d_n.data_ptr(), d_uv.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        wn, wuv = o.shading_attributes(hits)
        assert np.array_equal(d_n.cpu().numpy().view(np.uint32), wn.view(np.uint32)), f"{what}: shading normals"
        assert np.array_equal(d_uv.cpu().numpy().view(np.uint32), wuv.view(np.uint32)), f"{what}: uvs"

    check(v, nrm, "as added")  # (also builds the shading attributes: the updates below refresh them in place)
    v1 = (v + np.c_[0.05 * np.sin(7 * v[:, 1]), 0.04 * np.cos(5 * v[:, 0]), 0.3 * np.sin(3 * v[:, 0] + 2 * v[:, 1])]).astype(np.float32)
    n1 = g.standard_normal(nrm.shape)
    n1 = (n1 / np.linalg.norm(n1, axis=1, keepdims=True)).astype(np.float32)
    d_v, d_nrm = torch.from_numpy(v1).cuda(), torch.from_numpy(n1).cuda()
    torch.cuda.synchronize()
    t.update_mesh_vertices_device_async(h, d_v, d_nrm, stream=s.cuda_stream)
    t.refit_device_async(stream=s.cuda_stream)
    s.synchronize()
    t.wait_for_gpu()
    check(v1, n1, "new vertices and normals")
    v2 = (v1 * np.float32(0.9) + np.float32(0.03)).astype(np.float32)
    d_v2 = torch.from_numpy(v2).cuda()
    torch.cuda.synchronize()
    t.update_mesh_vertices_device_async(h, d_v2, stream=s.cuda_stream)  # d_normals=None: the stored ones, i.e. n1
    t.rebuild_device_async(stream=s.cuda_stream)
    s.synchronize()
    t.wait_for_gpu()
    check(v2, n1, "new vertices, normals kept")
    extra = soup[:1] + np.float32(2.0)  # a structural sync copies from the mesh's own arrays, the kept normals and the new face map
    t.push(extra)
    assert t.sync().last_sync_action == "rebuild"
    check(v2, n1, "after a structural sync", extra)


# ---- 7. argument errors leave the scene usable ---------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_scene_usable(rc):
    import torch
    from scene_kit import grid_mesh
    v, f, nrm, uv = grid_mesh(8, seed=2)
    soup = rc.scenes.fan_sphere(10, 6, radius=0.5)
    t = rc.TLAS()
    h_soup = t.push(soup, np.eye(4, dtype=np.float32))
    h_mesh = t.push_mesh(v + np.float32(2.0), f, nrm, uvs=uv)
    h_gone = t.push(soup[:6] + np.float32(5.0))
    d_soup = torch.from_numpy(deform(soup, 1)).cuda()
    d_v = torch.from_numpy(v + np.float32(2.0)).cuda()
    torch.cuda.synchronize()

    def refused(code, fn, *a, **k):
        with pytest.raises(rc.RaycoreError) as e:
            fn(*a, **k)
        assert e.value.code == code, (e.value.code, str(e.value))

    refused(RC_ERR_NOT_SYNCED, t.update_geometry_device_async, h_soup, d_soup)  # never synced
    t.sync()
    rays = rc.scenes.pinhole_rays(128, 128, (1.0, 1.0, 6.0), (1.0, 1.0, 0.0))
    before = t.trace(rays).tobytes()
    refused(RC_ERR_INVALID_ARGUMENT, t.update_geometry_device_async, h_soup, d_soup, n=0)
    refused(RC_ERR_INVALID_ARGUMENT, t.update_geometry_device_async, h_soup, None, n=4)  # NULL d_verts
    refused(RC_ERR_INVALID_ARGUMENT, t.update_geometry_device_async, h_soup, d_soup.double())
    refused(RC_ERR_INVALID_ARGUMENT, t.update_mesh_vertices_device_async, h_mesh, d_v[:-1].contiguous())  # wrong nv
    refused(RC_ERR_INVALID_ARGUMENT, t.update_mesh_vertices_device_async, h_mesh, d_v, d_v[:-1].contiguous())
    refused(RC_ERR_INVALID_ARGUMENT, t.update_mesh_vertices_device_async, h_soup, d_v)  # not a mesh
    refused(RC_ERR_INVALID_HANDLE, t.update_geometry_device_async, rc.TLASHandle(999), d_soup)
    assert t.sync().last_sync_action == "noop" and t.trace(rays).tobytes() == before
    t.delete(h_gone)
    refused(RC_ERR_INVALID_HANDLE, t.update_geometry_device_async, h_gone, d_soup)
    refused(RC_ERR_NOT_SYNCED, t.update_geometry_device_async, h_soup, d_soup)  # the delete is a pending host-side mutation
    t.sync()
    t.update_transform(h_soup, np.eye(4, dtype=np.float32))
    refused(RC_ERR_NOT_SYNCED, t.update_geometry_device_async, h_soup, d_soup)  # so is a host-side transform
    t.sync()
    assert t.trace(rays).tobytes() == before
    t.update_geometry_device_async(h_soup, d_soup)  # and the valid call works, on the null stream too
    t.update_mesh_vertices_device_async(h_mesh, d_v)
    t.refit_device_async()
    t.wait_for_gpu()
    u = rc.TLAS()
    u.push(deform(soup, 1), np.eye(4, dtype=np.float32))
    u.push_mesh(v + np.float32(2.0), f, nrm, uvs=uv)
    u.sync()
    assert t.trace(rays).tobytes() == u.trace(rays).tobytes()
    assert t.adapt().all_blas_nodes.tobytes() == u.adapt().all_blas_nodes.tobytes()


# ---- 8. the BLAS4 of an updated geometry -----------------------------------------------------------------------------------------------
def test_blas4_is_dropped_and_rebuilt(rc, oracle):
    import torch
    soup = rc.scenes.fan_sphere(10, 6, radius=0.5)
    t = rc.TLAS()
    geo = [t.add_geometry(soup), t.add_geometry(soup[:10])]  # the second never gets a BLAS4
    h = t.push_instances(geo[0])
    t.push_instances(geo[1])
    t.sync()

    def build4(k):
        n = C.c_uint32(0)
        assert rc.lib().rc_blas4_build(t._h, geo[k] - 1, C.byref(n)) == 0
        return rc.BLAS4(t, geo[k] - 1, n.value)

    rays = rc.scenes.pinhole_rays(96, 96, (0.4, 0.3, 3.0), (0.0, 0.0, 0.0))
    o = oracle.Scene()
    b = o.add_blas(soup)
    o.add_instance(b)
    o.build()
    b4 = build4(0)
    assert_hits_equal(b4.trace(rays), o.trace4(b, rays, nthreads=4), "BLAS4 before the update")
    with pytest.raises(rc.RaycoreError) as never:
        rc.BLAS4(t, geo[1] - 1, 0).trace(rays)
    d_soup = torch.from_numpy(deform(soup, 1)).cuda()
    torch.cuda.synchronize()
    t.update_geometry_device_async(h, d_soup)
    t.refit_device_async()
    for mode in ("closest", "any"):
        with pytest.raises(rc.RaycoreError) as e:
            b4.trace(rays, mode=mode)
        assert (e.value.code, str(e.value)) == (never.value.code, str(never.value))  # as for a geometry whose BLAS4 was never built
    t.wait_for_gpu()
    o = oracle.Scene()
    b = o.add_blas(deform(soup, 1))
    o.add_instance(b)
    o.build()
    b4 = build4(0)
    assert b4.nodes.tobytes() == o.blas4_nodes(b).tobytes()
    assert_hits_equal(b4.trace(rays), o.trace4(b, rays, nthreads=4), "BLAS4 rebuilt after the update")
    assert_hits_equal(b4.trace(rays, mode="any"), o.trace4(b, rays, mode="any", nthreads=4), "BLAS4 any")
    assert o.trace4(b, rays)["hit"].mean() > 0.05
