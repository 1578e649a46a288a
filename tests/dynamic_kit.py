"""The animated-scene kit of the device-side update tests (tests/test_gpu_dynamic.py, test_gpu_rebuild.py, test_gpu_deform.py) and of
every test that replays their frames: the lattices, the per-frame transforms and deformations, the oracle's frames of them (computed once
per process), and the twins a frame is compared with.  The rebuild tests' frames differ from the refit tests' (a frame with coincident
instances): theirs are rebuild_frame_xf / rebuild_oracle_frame."""
import numpy as np


SMALL = (6, 6, 4)     # 144 instances: at most kTlasLdsInst = 256 (kernel 5 would stage the whole TLAS in LDS: test_gpu_update_kernels.py)
LARGE = (12, 12, 6)   # 864 instances: the TLAS's top is renumbered (tlas_top_k > 0) for kernel 6, which this file does not run either
SCALED_FRAME = 2      # the frame whose linear part carries a non-uniform scale
W = H = 256
RC_ERR_INVALID_ARGUMENT, RC_ERR_INVALID_HANDLE, RC_ERR_NOT_SYNCED = 1, 2, 6


def sphere(rc):
    return rc.scenes.fan_sphere(10, 6, radius=0.5)


def initial_xf(rc, dims):
    return rc.scenes.lattice_transforms(*dims, 1.6, 3)[0]


def frame_xf(rc, dims, f):
    """Transforms of frame f: pitch 1.5 + 0.2 f, rotation seed 100 + 7 f; frame SCALED_FRAME stretches the local axes by (1.0, 0.7, 1.3)."""
    xf = rc.scenes.lattice_transforms(*dims, 1.5 + 0.2 * f, 100 + 7 * f)[0]
    if f == SCALED_FRAME:
        m = xf.reshape(-1, 3, 4).copy()
        m[:, :, :3] *= np.array([1.0, 0.7, 1.3], dtype=np.float32)
        xf = np.ascontiguousarray(m.reshape(-1, 12))
    return xf


def camera_rays(rc, dims):
    """A 256 x 256 pinhole view of the lattice from outside one of its corners (fixed per scene: the frames move under it)."""
    ext = (np.array(dims, dtype=np.float64) - 1) * 1.8   # the lattice at the frames' mean pitch
    centre = ext / 2
    eye = centre + np.array([0.45, 0.3, 1.0]) * (0.95 * ext[:2].max() + 3.0)
    return rc.scenes.pinhole_rays(W, H, eye, centre, fov_deg=45.0)


_oracle_cache = {}


def oracle_scene_hits(oracle, rc, xf, rays, mode="closest"):
    o = oracle.Scene()
    b = o.add_blas(sphere(rc))
    for i, x in enumerate(xf):
        o.add_instance(b, x, i)
    o.build()
    return o.trace(rays, mode=mode, nthreads=8)


def records_differing(a, b):
    return int(np.count_nonzero(np.any(a.view(np.uint32).reshape(len(a), -1) != b.view(np.uint32).reshape(len(b), -1), axis=1)))


def oracle_frame(oracle, rc, dims, f):
    """Closest hits of the oracle built from scratch with frame f's transforms (f = -1: the initial ones), with the conditions on the
    inputs asserted on the oracle's output alone."""
    key = (dims, f)
    if key not in _oracle_cache:
        rays = camera_rays(rc, dims)
        want = oracle_scene_hits(oracle, rc, initial_xf(rc, dims) if f < 0 else frame_xf(rc, dims, f), rays)
        if f >= 0:
            prev = oracle_frame(oracle, rc, dims, f - 1)
            hit_fraction = float(want["hit"].mean())
            changed = records_differing(want, prev) / len(want)
            print(f"inputs {dims} frame {f}: oracle hit fraction {hit_fraction:.3f}, records changed vs previous frame {changed:.3f}")
            assert hit_fraction >= 0.2, (dims, f, hit_fraction)
            assert changed >= 0.1, (dims, f, changed)
        _oracle_cache[key] = want
    return _oracle_cache[key]


def make_scene(rc, dims, n_handles=1):
    """One fan-sphere BLAS under the initial lattice, the instances split over n_handles handles (contiguous ranges)."""
    xf = initial_xf(rc, dims)
    n = len(xf)
    ids = np.arange(n, dtype=np.uint32)
    t = rc.TLAS()
    cuts = [n * k // n_handles for k in range(n_handles + 1)]
    blas = t.add_geometry(sphere(rc))
    handles = [t.push_instances(blas, xf[cuts[k]:cuts[k + 1]], ids[cuts[k]:cuts[k + 1]]) for k in range(n_handles)]
    t.sync()
    assert (t.get_option("tlas_top_k") > 0) == (n > 256)  # which top-level layout the scene exercises
    return t, handles, cuts


def host_frame(twin, handles, cuts, xf, which=None):
    for k, h in enumerate(handles):
        if which is None or k in which:
            twin.update_transforms(h, xf[cuts[k]:cuts[k + 1]])
    twin.sync()
    assert twin.last_sync_action == "refit"


def assert_same_scene(got, want, what):
    sg, sw = got.adapt(), want.adapt()
    assert sg.nodes.tobytes() == sw.nodes.tobytes(), f"{what}: TLAS nodes differ"
    assert sg.instances.tobytes() == sw.instances.tobytes(), f"{what}: instances differ"
    bg, bw = got.world_bound(), want.world_bound()
    assert bg.p_min.tobytes() == bw.p_min.tobytes() and bg.p_max.tobytes() == bw.p_max.tobytes(), f"{what}: world bound {bg.p_min} {bg.p_max} != {bw.p_min} {bw.p_max}"


def dev_bytes(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def hits_of(rc, d_hits):
    return d_hits.cpu().numpy().view(rc.HIT_DT)


N_FRAMES = 4
TIE_FRAME = 3         # the frame with three coincident instances
PATHS = [(SMALL, 1), (SMALL, 0), (LARGE, 0)]  # (lattice, tlas_rebuild_fused): the single-workgroup kernel applies up to 256 instances
PATH_IDS = ["144-fused", "144-chain", "864-chain"]


def rebuild_frame_xf(rc, dims, f):
    xf = rc.scenes.lattice_transforms(*dims, 1.5 + 0.2 * f, 100 + 7 * f)[0]
    n = len(xf)
    m = xf.reshape(n, 3, 4).copy()
    if f == SCALED_FRAME:
        m[:, :, :3] *= np.array([1.0, 0.7, 1.3], dtype=np.float32)
    perm = np.random.Generator(np.random.Philox(key=900 + f)).permutation(n)
    m[:, :, 3] = m[perm][:, :, 3]
    if f == TIE_FRAME:
        m[1] = m[0]
        m[n - 1] = m[0]
    return np.ascontiguousarray(m.reshape(n, 12))


class OracleFrame:
    def __init__(self, oracle, rc, xf, rays, blas=None, owner=None):
        o = oracle.Scene()
        blas = blas if blas is not None else [sphere(rc)]
        ids = [o.add_blas(b) for b in blas]
        for i, x in enumerate(xf):
            o.add_instance(ids[0 if owner is None else owner[i]], x, i)
        o.build()
        self.nodes, self.instances, self.bound = o.tlas_nodes, o.instances, o.world_bound
        self.closest = o.trace(rays, nthreads=8)
        self.any = o.trace(rays, mode="any", nthreads=8)


_rebuild_oracle_cache = {}


def rebuild_oracle_frame(oracle, rc, dims, f):
    """The oracle built from scratch with frame f's transforms (f = -1: the initial ones), with the conditions on the inputs asserted on
    the oracle's output alone."""
    key = (dims, f)
    if key not in _rebuild_oracle_cache:
        want = OracleFrame(oracle, rc, initial_xf(rc, dims) if f < 0 else rebuild_frame_xf(rc, dims, f), camera_rays(rc, dims))
        if f >= 0:
            prev = rebuild_oracle_frame(oracle, rc, dims, f - 1)
            n = len(want.instances)
            moved = float(np.mean(want.nodes["child1"][n - 1:] != prev.nodes["child1"][n - 1:]))
            hit_fraction = float(want.closest["hit"].mean())
            changed = records_differing(want.closest, prev.closest) / len(want.closest)
            print(f"inputs {dims} frame {f}: leaf slots with another instance {moved:.3f}, oracle hit fraction {hit_fraction:.3f}, "
                  f"records changed vs previous frame {changed:.3f}")
            assert moved >= 0.9, (dims, f, moved)
            assert hit_fraction >= 0.2, (dims, f, hit_fraction)
            assert changed >= 0.1, (dims, f, changed)
        _rebuild_oracle_cache[key] = want
    return _rebuild_oracle_cache[key]


def fresh_twin(rc, xf, blas=None, owner=None, handles=None):
    """A new scene with the same pushes and these transforms, built by the structural sync (`handles`: a list that receives the pushes')."""
    t = rc.TLAS()
    n = len(xf)
    ids = np.arange(n, dtype=np.uint32)
    blas = blas if blas is not None else [sphere(rc)]
    owner = np.zeros(n, dtype=np.int64) if owner is None else np.asarray(owner)
    for k, b in enumerate(blas):  # contiguous ranges per BLAS, in order
        bi = t.add_geometry(b)
        sel = owner == k
        handle = t.push_instances(bi, xf[sel], ids[sel])
        if handles is not None:
            handles.append(handle)
    t.sync()
    assert t.last_sync_action == "rebuild"
    return t


class Frames:
    """The device buffers of one scene's animation on one stream."""

    def __init__(self, rc, dims, fused):
        import torch
        self.torch, self.rc, self.dims = torch, rc, dims
        self.t, (self.h,), _ = make_scene(rc, dims)
        self.t.set_option("tlas_rebuild_fused", fused)
        assert self.t.get_option("tlas_rebuild_fused") == fused
        self.rays = camera_rays(rc, dims)
        self.n = len(self.rays)
        self.frames = [torch.from_numpy(rebuild_frame_xf(rc, dims, f)).cuda() for f in range(N_FRAMES)]
        self.d_xf = self.frames[0].clone()
        self.d_rays = dev_bytes(torch, self.rays)
        self.d_hits, self.d_any = (torch.zeros(self.n * 32, dtype=torch.uint8, device="cuda") for _ in range(2))
        self.s = torch.cuda.Stream()
        for buf in (self.d_xf, self.d_rays, self.d_hits, self.d_any, *self.frames):
            buf.record_stream(self.s)
        torch.cuda.synchronize()

    def trace(self, st):
        self.t.trace_device(self.d_rays.data_ptr(), self.d_hits.data_ptr(), self.n, stream=st)
        self.t.trace_device(self.d_rays.data_ptr(), self.d_any.data_ptr(), self.n, mode="any", stream=st)

    def hits(self):
        return hits_of(self.rc, self.d_hits), hits_of(self.rc, self.d_any)


def deform(soup, f):
    """Frame f of the soup (f < 0: the soup itself)."""
    if f < 0:
        return np.ascontiguousarray(soup, dtype=np.float32)
    v = np.asarray(soup, dtype=np.float64).reshape(-1, 3)
    a = (0.8 + 0.5 * f) * v[:, 2] / 0.5
    c, s = np.cos(a), np.sin(a)
    out = np.stack([(c * v[:, 0] - s * v[:, 1]) * (1 + 0.4 * f), s * v[:, 0] + c * v[:, 1], v[:, 2] * (1 - 0.15 * f)], axis=1)
    out = out.astype(np.float32).reshape(-1, 9)
    return np.ascontiguousarray(np.roll(out, 7 * (f + 1), axis=0))


class Spec:
    """A scene: soups (soup 0 is the one that deforms), the instance ranges of its handles as (soup, first, end), lattice."""

    def __init__(self, rc, name):
        sc = rc.scenes
        self.name = name
        self.dims = LARGE if name == "864" else SMALL
        self.xf = initial_xf(rc, self.dims)
        n = len(self.xf)
        self.soups = [sc.fan_sphere(40, 20, radius=0.5) if name == "top" else sc.fan_sphere(10, 6, radius=0.5)]
        self.groups = [(0, 0, n)]
        if name == "two":  # the deforming soup is shared by the first and the last handle
            self.soups.append(sc.fan_sphere(16, 9, radius=0.45))
            self.groups = [(0, 0, 60), (1, 60, 84), (0, 84, n)]
        if name == "poles":  # 2 x 11 x 8 faces, 2 x 11 of them (one per pole quad) degenerate
            self.soups = [sc.uv_sphere_grid(12, 9, radius=0.5)]
        self.owner = np.zeros(n, dtype=np.int64)
        for k, lo, hi in self.groups:
            self.owner[lo:hi] = k
        self.rays = camera_rays(rc, self.dims)

    def soups_of(self, f):
        return [deform(self.soups[0], f)] + self.soups[1:]

    def build(self, rc, f=-1, xf=None):
        """The scene with frame f's soup, built by the structural sync -> (scene, handles)."""
        xf = self.xf if xf is None else xf
        t = rc.TLAS()
        ids = np.arange(len(xf), dtype=np.uint32)
        geo = [t.add_geometry(s) for s in self.soups_of(f)]
        hs = [t.push_instances(geo[k], xf[lo:hi], ids[lo:hi]) for k, lo, hi in self.groups]
        t.sync()
        assert t.last_sync_action == "rebuild"
        return t, hs


class Want:
    """The oracle built from scratch."""

    def __init__(self, oracle, soups, owner, xf, rays, metas=None):
        o = oracle.Scene()
        ids = [o.add_blas(s, None if metas is None else metas[k]) for k, s in enumerate(soups)]
        for i, x in enumerate(xf):
            o.add_instance(ids[owner[i]], x, i)
        o.build()
        self.nodes, self.instances, self.bound = o.tlas_nodes, o.instances, o.world_bound
        self.blas_nodes, self.blas_prims, self.blas_descs = o.blas_nodes, o.blas_prims, o.blas_descs
        self.closest = o.trace(rays, nthreads=8)
        self.any = o.trace(rays, mode="any", nthreads=8)

    def same_topology(self, other):
        return all(np.array_equal(self.nodes[k], other.nodes[k]) for k in ("child0", "child1", "parent"))


_want_cache = {}


def want_frame(oracle, rc, spec, f):
    """Frame f's oracle (f = -1: the undeformed scene) with the conditions on the inputs asserted on the oracle's output alone."""
    key = (spec.name, f)
    if key not in _want_cache:
        w = Want(oracle, spec.soups_of(f), spec.owner, spec.xf, spec.rays)
        if f >= 0:
            prev, first = want_frame(oracle, rc, spec, f - 1), want_frame(oracle, rc, spec, -1)
            n0 = int(w.blas_descs["primitives_offset"][1]) if len(w.blas_descs) > 1 else len(w.blas_prims)
            moved = float(np.mean(w.blas_prims["meta"][:n0] != prev.blas_prims["meta"][:n0]))
            hit_fraction = float(w.closest["hit"].mean())
            changed = records_differing(w.closest, prev.closest) / len(w.closest)
            print(f"inputs {spec.name} frame {f}: prims {len(w.blas_prims)} (before {len(prev.blas_prims)}), leaf slots with other metadata {moved:.3f}, "
                  f"oracle hit fraction {hit_fraction:.3f}, records changed vs previous frame {changed:.3f}, TLAS topology as initially: {w.same_topology(first)}")
            assert len(w.blas_prims) == len(prev.blas_prims), (spec.name, f)
            assert moved >= 0.9, (spec.name, f, moved)
            assert hit_fraction >= 0.2, (spec.name, f, hit_fraction)
            assert changed >= 0.3, (spec.name, f, changed)
        _want_cache[key] = w
    return _want_cache[key]
