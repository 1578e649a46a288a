"""Random walks over the scene lifecycle on the GPU: host-side mutations, device-side updates and commits, the descriptor path and the
readers that refresh lazy host state, interleaved by tests/lifecycle_model.py's generator and checked against its model after EVERY call.

After every operation: the return value or the RaycoreError code, last_sync_action, is_valid of every handle and n_instances /
n_total_instances / n_geometries follow the model; after a refused call the state fingerprint (the counts, the world bound and the bytes of
the exports that are legal in that state) is what it was.

After every commit (a check point) two yardsticks, neither of them the code under test:
* the oracle built from scratch from the model (surviving geometries in creation order, handles ascending): closest hits of the check
  point's ray batch (lifecycle_model.checkpoint_rays) through the default dispatch and through one of kernels 0, 1, 3, 5, 6 in turn (5 not
  above 256 instances), world bound, instance descriptors with their inverses, BLAS nodes, primitives, descriptors and exported triangles,
  all bit for bit; any-hit records in full where the tree is byte for byte the oracle's, on their hit word where a refit kept an older
  topology (the rule of tests/test_gpu_auto_rebuild.py);
* the TLAS nodes, byte for byte, on EVERY check point: the oracle's tree after a rebuilding commit, and after a refitting one the numpy
  refit (auto_rebuild_model.refit) of the topology the model has tracked since the last rebuild to the oracle's leaf boxes -- a refit that
  walked stale topology records after a rebuild cannot pass it.  (This takes the place of a second product scene fed the host-side
  equivalents: it compares on every check point, not only while two scenes happen to be in the same tree class.)

Readers are compared with the oracle where they succeed: a loaded scene's tree and hits, BLAS4 nodes and trace4 hits (a BLAS4 the model
says was dropped must be refused), collision pairs, view-factor totals, shading attributes, the state block of the gated rebuild.

One captured segment per walk: update_transforms_device -> [update_geometry_device_async] -> commit -> trace_device runs eagerly, is
captured into one graph (a single linear chain) and replayed six times on new transforms (and a new soup) written into the captured
tensors, with a check point and a reader after every replay -- every read of the mirror, the world bound and the BLAS bounds has to fetch
from the device again.  A host push + sync ends it (the model's captured state is clear from there), then the graph is deleted and
release_captures set.

A failing walk prints its seed, regime, the failing operation's index and the operation list up to it; run(rc, oracle, ops, regime, tmp)
takes such a list as it is (tmp: a directory for the scene files of save_load, pytest's tmp_path).
"""
import ctypes as C
import os

import numpy as np
import pytest

import lifecycle_model as lm
from gpu_kit import rc  # noqa: F401
from helpers import assert_f32_bits_equal, assert_hits_equal

pytestmark = pytest.mark.gpu

N_OPS = 120
KERNELS = (0, 1, 3, 5, 6)
REL = 1e-11  # the cost: tests/test_gpu_auto_rebuild.py's bound (sums of at most 700 positive f64 terms)
FIRST_READS = ("trace", "exports", "world_bound", "collide", "save_load", "vf", "quality", "shading")
EXPORTS = ("nodes", "instances", "all_blas_nodes", "all_blas_prims", "blas_descriptors")


class Runner:
    def __init__(self, rc, oracle, regime, tmp):
        import torch
        self.torch, self.rc, self.oracle, self.tmp = torch, rc, oracle, str(tmp)
        self.cfg = lm.REGIMES[regime]
        self.t = rc.TLAS()
        self.t.set_option("tlas_rebuild_fused", self.cfg["fused"])
        self.model = lm.Model(oracle)
        self.hs = []          # TLASHandle of every handle ordinal
        self.keep = []        # device tensors the enqueued kernels read
        self.s = torch.cuda.Stream()
        self.turn = 0         # which of KERNELS the next check point adds
        self.kernels_seen = set()
        self.cap = None       # the captured segment's graph and tensors
        self.first = 0        # which read meets a check point's pending asynchronous work first

    # -- plumbing ------------------------------------------------------------------------------------------------------------------------
    def dev(self, a):
        with self.torch.cuda.stream(self.s):
            d = self.torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.keep.append(d)
        return d

    @property
    def st(self):
        return self.s.cuda_stream

    def check(self, status):
        self.rc._capi.check(status)

    def o(self):
        return lm.oracle_scene(self.oracle, self.model)

    def fingerprint(self):
        t, m = self.t, self.model
        b = t.world_bound()
        fp = [(t.n_instances(), t.n_total_instances(), t.n_geometries()), b.p_min.tobytes(), b.p_max.tobytes()]
        if m.clean:
            fp += [getattr(t.static_tlas, ex).tobytes() for ex in EXPORTS]
        else:  # the mirror may be read in every state (rc_get_instances: "the update stays pending")
            fp += [t.get_instances(self.hs[k]).tobytes() for k in m.live()]
        return fp

    # -- one operation -------------------------------------------------------------------------------------------------------------------
    def step(self, k, op):
        m, t = self.model, self.t
        out = m.apply(op)
        refused = out.error is not None and op[0] != "wait"
        before = self.fingerprint() if refused else None
        got_error, value = None, None
        try:
            value = getattr(self, "do_" + op[0])(k, out, *op[1:])
        except self.rc.RaycoreError as e:
            got_error = e.code
            if out.error is None:
                raise AssertionError(f"{op[0]} raised {lm.ERROR_NAMES.get(e.code, e.code)} ({e}); the model expects success") from e
        assert got_error == out.error, f"{op[0]}: expected {lm.ERROR_NAMES.get(out.error, out.error)}, got {lm.ERROR_NAMES.get(got_error, got_error)}"
        if out.error is None and out.value is not None and op[0] == "delete":
            assert value == out.value, f"delete returned {value}, the model says {out.value}"
        if out.action is not None:
            assert t.last_sync_action == out.action, f"last_sync_action {t.last_sync_action}, the model says {out.action}"
        assert (t.n_instances(), t.n_total_instances(), t.n_geometries()) == m.counts(), \
            f"counts {(t.n_instances(), t.n_total_instances(), t.n_geometries())}, the model says {m.counts()}"
        for j, h in enumerate(self.hs):
            assert h.id == j + 1
            assert t.is_valid(h) == m.valid(j), f"is_valid(handle {h.id}) is {t.is_valid(h)}, the model says {m.valid(j)}"
            assert t.n_instances(h) == (m.handles[j].m if m.valid(j) else 0)
        if refused:
            assert self.fingerprint() == before, "a refused call changed the scene"
        if out.commit is not None and m.clean:
            self.checkpoint(k)

    # -- host mutations ------------------------------------------------------------------------------------------------------------------
    def do_push(self, k, out, kind, gseed, n, xseed, span):
        self.hs.append(self.t.push(lm.soup(kind, gseed), lm.xforms(xseed, n, span), instance_ids=lm.instance_ids(xseed, n)))

    def do_push_shared(self, k, out, kind, gseed, parts, span):
        b = self.t.add_geometry(lm.soup(kind, gseed))
        for n, xseed in parts:
            self.hs.append(self.t.push_instances(b, lm.xforms(xseed, n, span), lm.instance_ids(xseed, n)))

    def do_push_mesh(self, k, out, gseed, n, xseed, span):
        v, f, nrm, uv = lm.mesh(gseed)
        self.hs.append(self.t.push_mesh(v, f, nrm, transforms=lm.xforms(xseed, n, span), uvs=uv, instance_ids=lm.instance_ids(xseed, n)))

    def do_delete(self, k, out, h):
        return self.t.delete(self.hs[h])

    def do_update_transforms(self, k, out, h, xseed, n, span):
        self.t.update_transforms(self.hs[h], lm.xforms(xseed, n, span))

    def do_update(self, k, out, h, kind, gseed):
        self.t.update(self.hs[h], lm.soup(kind, gseed))

    def do_update_mesh(self, k, out, h, gseed):
        v, f, nrm, uv = lm.mesh(gseed)
        self.t.update_mesh(self.hs[h], v, f, nrm, uv)

    def do_sync(self, k, out):
        self.t.sync()
        action = self.t.last_sync_action
        assert self.t.sync().last_sync_action == "noop", "a second sync found something to do"
        self.t.last_sync_action = action

    # -- device updates and commits --------------------------------------------------------------------------------------------------------
    def do_utd(self, k, out, h, xseed, n, span):
        self.t.update_transforms_device(self.hs[h], self.dev(lm.xforms(xseed, n, span)), stream=self.st)

    def do_ugd(self, k, out, h, form, gseed):
        kind = self.model.handles[h].geom.kind
        self.t.update_geometry_device_async(self.hs[h], self.dev(lm.soup(kind if kind in lm.SOUP_KINDS else "fan", gseed, form)), stream=self.st)

    def do_umd(self, k, out, h, gseed, normals):
        v, _, nrm, _ = lm.mesh(gseed)
        self.t.update_mesh_vertices_device_async(self.hs[h], self.dev(v), self.dev(nrm) if normals else None, stream=self.st)

    def do_ibr(self, k, out, h, xseed, how, span):
        recompute = how == 1
        p, cnt = C.c_void_p(), C.c_uint32()
        self.check(self.rc.lib().rc_instance_buffer_device(self.t._h, self.hs[h].id, C.byref(p), C.byref(cnt)))  # (TLAS.instance_buffer would sync first)
        n = self.model.handles[h].m
        assert cnt.value == n
        xf = lm.xforms(xseed, n, span)

        class Alias:
            __cuda_array_interface__ = {"shape": (n, 27), "typestr": "<f4", "data": (p.value, False), "version": 2}

        recs = self.torch.as_tensor(Alias(), device="cuda")
        recs[:, 2:14] = self.torch.from_numpy(xf).cuda()
        if recompute:
            recs[:, 14:26] = 0.0  # (whatever stands there: the refit recomputes it)
        else:
            recs[:, 14:26] = self.torch.from_numpy(np.stack([self.oracle.mat3x4_inverse(x) for x in xf])).cuda()
        self.torch.cuda.synchronize()
        if how in (0, 1):
            self.t.refit_device(recompute_inverse=bool(recompute))
        else:  # no update call since the last refit: the asynchronous commits derive the per-instance data from the descriptors
            (self.t.refit_device_async if how == "refit" else self.t.rebuild_device_async)(stream=self.st)

    def do_refit(self, k, out):
        self.t.refit_device_async(stream=self.st)

    def do_rebuild(self, k, out):
        self.t.rebuild_device_async(stream=self.st)

    def do_gated(self, k, out, ratio):
        self.t.refit_or_rebuild_device_async(ratio, stream=self.st)

    def do_wait(self, k, out):
        self.t.wait_for_gpu()

    # -- the captured segment --------------------------------------------------------------------------------------------------------------
    def commit_on(self, commit, ratio, st):
        if commit == "gated":
            self.t.refit_or_rebuild_device_async(ratio, stream=st)
        else:
            (self.t.refit_device_async if commit == "refit" else self.t.rebuild_device_async)(stream=st)

    def do_capture(self, k, out, h, geo, commit, ratio):
        torch, t, hd = self.torch, self.t, self.model.handles[h]
        rays = lm.checkpoint_rays(self.oracle, self.model, k)[0][:1024]
        n = len(rays)
        d_rays = self.dev(rays.view(np.uint8).reshape(-1).copy())
        d_xf, d_soup = self.dev(hd.xf), (self.dev(hd.geom.verts) if geo else None)
        with torch.cuda.stream(self.s):
            d_hits = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        self.keep.append(d_hits)
        t.trace_device(d_rays.data_ptr(), d_hits.data_ptr(), n, stream=self.st)  # eager once on the stream: its stack spill area
        t.shading_attributes_device(d_hits.data_ptr(), n, None, None, stream=self.st)  # (a captured update refreshes the attributes only if they exist)
        self.s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=self.s):  # one linear chain, no parallel branches
            st = torch.cuda.current_stream().cuda_stream
            t.update_transforms_device(self.hs[h], d_xf, stream=st)
            if geo:
                t.update_geometry_device_async(self.hs[h], d_soup, stream=st)
            self.commit_on(commit, ratio, st)
            t.trace_device(d_rays.data_ptr(), d_hits.data_ptr(), n, stream=st)
        self.cap = {"g": g, "d_xf": d_xf, "d_soup": d_soup, "d_hits": d_hits, "rays": rays, "h": h, "geo": geo}

    def do_replay(self, k, out, xseed, gseed, span):
        torch, cap, m = self.torch, self.cap, self.model
        assert m.captured_alive and cap is not None  # (never replay a graph whose addresses a rebuilding sync has freed)
        hd = m.handles[cap["h"]]
        cap["d_hits"].zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(self.s):
            cap["d_xf"].copy_(torch.from_numpy(lm.xforms(xseed, hd.m, span)))
            if cap["geo"]:
                cap["d_soup"].copy_(torch.from_numpy(lm.soup(hd.geom.kind, gseed)))
            cap["g"].replay()
        self.s.synchronize()  # the caller waits for a replay before any host-side read
        got = cap["d_hits"].cpu().numpy().view(self.rc.HIT_DT)
        assert_hits_equal(got, self.o().trace(cap["rays"]), "the replayed chain's trace")

    def do_release(self, k, out):
        self.drop_graph()
        self.t.set_option("release_captures", 1)

    def drop_graph(self):
        if self.cap is not None:
            self.torch.cuda.synchronize()
            self.cap = None
            self.torch.cuda.synchronize()

    # -- readers -------------------------------------------------------------------------------------------------------------------------
    def do_get_instances(self, k, out, h):
        got = self.t.get_instances(self.hs[h])
        first = self.model.first_instance(h)
        want = self.o().instances[first:first + self.model.handles[h].m]
        assert got.tobytes() == want.tobytes(), "get_instances differs from the oracle's descriptors"

    def do_world_bound(self, k, out):
        b = self.t.world_bound()
        if self.model.clean:
            assert np.concatenate([b.p_min, b.p_max]).tobytes() == self.o().world_bound.tobytes(), "world bound"

    def do_counts(self, k, out):
        pass  # (every step compares them)

    def do_exports(self, k, out):
        self.compare_exports(tree=True)

    def do_trace(self, k, out):
        rays, _ = lm.checkpoint_rays(self.oracle, self.model, k)
        got = self.t.trace(rays)  # raises while anything is pending
        assert_hits_equal(got, self.o().trace(rays), "trace")

    def do_quality(self, k, out):
        q = self.t.tlas_quality()
        want = self.model.quality()
        assert {f: q[f] for f in want} == want, f"tlas_quality {q}, the model says {want}"
        built = self.model.trees.cost_built
        if want["armed"] and not self.model.dev_pending:
            assert abs(q["cost_built"] - built) <= REL * built, f"cost_built {q['cost_built']!r}, numpy on the oracle's tree {built!r}"

    def do_save_load(self, k, out):
        path = os.path.join(self.tmp, f"scene_{k}.bin")
        self.check(self.rc.lib().rc_scene_save(self.t._h, path.encode()))  # (TLAS.save would sync first)
        u = self.rc.TLAS.load(path)
        try:
            assert u.sync().last_sync_action == "rebuild"
            o = self.o()
            rays, _ = lm.checkpoint_rays(self.oracle, self.model, k)
            assert u.static_tlas.nodes.tobytes() == o.tlas_nodes.tobytes(), "the loaded scene's TLAS"
            assert u.static_tlas.instances.tobytes() == o.instances.tobytes(), "the loaded scene's instances"
            assert_hits_equal(u.trace(rays), o.trace(rays), "the loaded scene's closest hits")
            assert_hits_equal(u.trace(rays, mode="any"), o.trace(rays, mode="any"), "the loaded scene's any hits")
            for j, h in enumerate(self.hs):
                assert u.is_valid(h) == self.model.valid(j), "the loaded scene's handles"
        finally:
            u.free()
            os.remove(path)

    def blas4_want(self, geom, k):
        o = self.oracle.Scene()
        b = o.add_mesh(*geom.mesh) if geom.is_mesh else o.add_blas(geom.verts)
        o.add_instance(b)
        o.build()
        g = np.random.Generator(np.random.Philox(key=[k, 99]))
        d = g.normal(size=(512, 3))
        origins = 2.0 * d / np.linalg.norm(d, axis=1, keepdims=True)
        tri = geom.triangles().astype(np.float64)  # towards points ON the geometry (a lone triangle is a small target), in its own space
        tri = tri[np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1) > 0]  # (not on its degenerate faces)
        w = g.dirichlet((1.0, 1.0, 1.0), size=512)
        dirs = np.einsum("nk,nkc->nc", w, tri[g.integers(0, len(tri), size=512)]) - origins
        rays = self.oracle.make_rays(origins, dirs / np.linalg.norm(dirs, axis=1, keepdims=True))
        return o.blas4_nodes(b), rays, o.trace4(b, rays), o.trace4(b, rays, mode="any")

    def compare_blas4(self, h, k):
        geom = self.model.handles[h].geom
        b4 = self.rc.api.BLAS4(self.t, self.model.blas_index(geom) - 1, 0)
        if not geom.blas4:
            b4.trace(self.oracle.make_rays([[0, 0, 3]], [0, 0, -1]))  # must raise: the BLAS4 was never built, or dropped by an update
            raise AssertionError("a BLAS4 that was never built (or was dropped by a geometry update) still traces")
        nodes, rays, want, want_any = self.blas4_want(geom, k)
        cnt = C.c_uint32(0)
        self.check(self.rc.lib().rc_export_blas4_nodes(self.t._h, b4._blas_id, None, 0, C.byref(cnt)))
        b4.num_interior = cnt.value
        assert b4.nodes.tobytes() == nodes.tobytes(), "BLAS4 nodes differ from the oracle's collapse of the CURRENT geometry"
        assert_hits_equal(b4.trace(rays), want, "closest_hit4")
        assert_hits_equal(b4.trace(rays, mode="any"), want_any, "any_hit4")
        assert want["hit"].mean() > 0.5

    def do_blas4_build(self, k, out, h):
        n = C.c_uint32(0)
        self.check(self.rc.lib().rc_blas4_build(self.t._h, self.model.blas_index(self.model.handles[h].geom) - 1, C.byref(n)))
        self.compare_blas4(h, k)

    def do_blas4_trace(self, k, out, h):
        self.compare_blas4(h, k)

    def do_collide(self, k, out):
        L, n = self.rc.lib(), C.c_uint64(0)
        self.check(L.rc_collide_instances(self.t._h, None, 0, C.byref(n)))  # (api.collide_instances would sync first)
        got = np.zeros((n.value, 2), dtype=np.uint32)
        if n.value:
            self.check(L.rc_collide_instances(self.t._h, self.rc._capi.ptr(got), n.value, C.byref(n)))
        want = self.o().collide_instances()[0]
        assert len(got) == len(want), f"{len(got)} contact pairs, the oracle finds {len(want)}"
        if self.model.trees.is_fresh:  # the reference algorithm's order follows the tree
            assert got.tobytes() == want.tobytes(), "contact pairs"
        else:
            key = lambda a: a[np.lexsort((a[:, 1], a[:, 0]))].tobytes()
            assert key(got) == key(want), "contact pairs (as a set: the refitted tree keeps another order)"

    def do_vf(self, k, out):
        received, emitted = self.rc.view_factor_totals(self.t.static_tlas, rays_per_triangle=2, seed=k)
        mat = self.o().view_factors(2, seed=k)
        assert np.array_equal(received, mat.sum(axis=0, dtype=np.uint64)), "view-factor totals: received"
        assert np.array_equal(emitted, mat.sum(axis=1, dtype=np.uint64)), "view-factor totals: emitted"
        # the host matrix addresses its sources through the order by metadata, which a geometry update invalidates (the totals do not)
        n, whole = len(mat), self.t.get_option("vf_chunk_bytes")
        self.t.set_option("vf_chunk_bytes", max(4096, 4 * n * -(-n // 8)))  # about eight row chunks: one chunk takes every source whatever the order
        try:
            got = self.rc.view_factors(self.t.static_tlas, rays_per_triangle=2, seed=k)
        finally:
            self.t.set_option("vf_chunk_bytes", whole)
        assert got.shape == mat.shape and np.array_equal(got, mat), "view-factor matrix"
        if len(mat):
            assert mat.sum() > 0

    def do_shading(self, k, out):
        torch = self.torch
        rays, _ = lm.checkpoint_rays(self.oracle, self.model, k)
        rays = rays[:1024]
        n = len(rays)
        d_rays = self.dev(rays.view(np.uint8).reshape(-1).copy())
        with torch.cuda.stream(self.s):
            d_hits = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
            d_nrm, d_uv = torch.zeros(n, 3, device="cuda"), torch.zeros(n, 2, device="cuda")
        self.keep += [d_hits, d_nrm, d_uv]
        self.t.trace_device(d_rays.data_ptr(), d_hits.data_ptr(), n, stream=self.st)  # raises while anything is pending
        self.t.shading_attributes_device(d_hits.data_ptr(), n, d_nrm.data_ptr(), d_uv.data_ptr(), stream=self.st)
        self.s.synchronize()
        hits = d_hits.cpu().numpy().view(self.rc.HIT_DT)
        assert_hits_equal(hits, self.o().trace(rays), "trace_device")
        nrm, uv = self.o().shading_attributes(hits)
        assert_f32_bits_equal(d_nrm.cpu().numpy(), nrm, "shading normals")
        assert_f32_bits_equal(d_uv.cpu().numpy(), uv, "shading uvs")

    # -- the check point -----------------------------------------------------------------------------------------------------------------
    def compare_exports(self, tree):
        st, o, trees = self.t.static_tlas, self.o(), self.model.trees
        assert st.instances.tobytes() == o.instances.tobytes(), "instance descriptors differ from the oracle's"
        if tree:
            took = "built from scratch" if trees.is_fresh else f"refitted on the topology of the last rebuild (tree class {self.model.tree})"
            assert st.nodes.tobytes() == trees.nodes.tobytes(), f"TLAS nodes differ from the oracle's tree {took}"
        assert st.all_blas_nodes.tobytes() == o.blas_nodes.tobytes(), "BLAS nodes"
        assert st.all_blas_prims.tobytes() == o.blas_prims.tobytes(), "primitives"
        assert st.blas_descriptors.tobytes() == o.blas_descs.tobytes(), "BLAS descriptors"
        got, want = st.all_blas_triangles, o.triangles
        assert len(got) == len(want)
        if len(got):
            assert np.array_equal(got["metadata"], want["metadata"]), "triangle metadata"
            as_f32 = lambda a: np.ascontiguousarray(a).view(np.uint32).reshape(len(a), 34)[:, :33].copy().view(np.float32)
            assert_f32_bits_equal(as_f32(got), as_f32(want), "exported triangles")
        b = self.t.world_bound()
        assert np.concatenate([b.p_min, b.p_max]).tobytes() == o.world_bound.tobytes(), f"world bound {b}, the oracle's {o.world_bound}"

    def checkpoint(self, k):
        t, m, o = self.t, self.model, self.o()
        assert t.sync().last_sync_action == "noop", "the commit left something pending"
        rays, aimed = lm.checkpoint_rays(self.oracle, m, k)
        want, want_any = o.trace(rays), o.trace(rays, mode="any")
        if m.n_total():
            hit, own = lm.liveness(want, aimed)
            assert hit >= 0.2 and own >= 0.8, f"the check point's rays are not live: {hit:.2f} hit, {own:.2f} of the touched instances seen"
        # Whichever host-side read comes first after an eager commit is the one that has to wait for the caller's stream (the header's
        # "they wait on the host for every EAGER update / refit enqueued so far"); the reads take that place in turn.
        first = FIRST_READS[self.first % len(FIRST_READS)]
        self.first += 1
        if first == "exports":
            self.compare_exports(tree=True)
        elif first != "trace":
            getattr(self, "do_" + first)(k, None)
        got = t.trace(rays)
        assert_hits_equal(got, want, "closest hits, default dispatch")
        kernel = KERNELS[self.turn % len(KERNELS)]
        self.turn += 1
        if kernel == 5 and m.n_total() > 256:
            kernel = KERNELS[self.turn % len(KERNELS)]
            self.turn += 1
        t.set_option("kernel", kernel)
        try:
            again = t.trace(rays)
        finally:
            t.set_option("kernel", -1)
        self.kernels_seen.add(kernel)
        assert_hits_equal(again, want, f"closest hits, kernel {kernel}")
        assert again.tobytes() == got.tobytes(), f"kernel {kernel} differs from the default dispatch"
        got_any = t.trace(rays, mode="any")
        if m.trees.is_fresh:
            assert_hits_equal(got_any, want_any, "any hits")
        else:
            assert np.array_equal(got_any["hit"], want_any["hit"]), "any hits, hit word (refitted tree)"
        self.compare_exports(tree=True)
        m.touched.clear()


def run(rc, oracle, ops, regime, tmp, seed=None):
    """Drive the product and the model through `ops`; every mismatch names the operation and prints the prefix that reaches it."""
    r = Runner(rc, oracle, regime, tmp)
    try:
        for k, op in enumerate(ops):
            try:
                r.step(k, op)
            except (AssertionError, rc.RaycoreError) as e:
                raise AssertionError(f"{e}\n{lm.describe(seed, regime, ops, k)}") from e
        rc.lib()  # (keeps the library loaded until the scene is gone)
    finally:
        r.drop_graph()
        r.torch.cuda.synchronize()
        r.t.free()
    return r


WALKS = [(regime, seed) for regime, seeds in lm.SEEDS.items() for seed in seeds]


@pytest.mark.parametrize("regime, seed", WALKS, ids=[f"{r}-{s}" for r, s in WALKS])
def test_walk(rc, oracle, tmp_path, regime, seed):
    r = run(rc, oracle, lm.walk(seed, regime, N_OPS), regime, tmp_path, seed)
    assert len(r.kernels_seen) >= 4, r.kernels_seen  # every kernel shape read the scene after some commit
