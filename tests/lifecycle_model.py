"""Plain-Python model of one scene's lifecycle across host-side and device-side mutations, and the random walk over it.

Written from the text of include/raycore_mi355x.h (the comments from rc_instance_buffer_device to rc_update_mesh_vertices_device_async, and
those of rc_sync, rc_add_blas, rc_delete, rc_get_instances, rc_wait), not from the library's source; the flag table in DESIGN.md ("Scene
state flags") names the host-side flags each rule below stands for.  Nothing here imports the product.  The oracle (oracle.pyoracle) is an
argument wherever a tree or a hit is needed; the gate of refit_or_rebuild_device_async is predicted with tests/auto_rebuild_model.py's
cost() and refit().

Model        one scene: geometries in creation order, handles in id order, the pending state, the derived state (tree class, BLAS4s,
             the state block of the gated rebuild, the sticky geometry status).  apply(op) says what the call returns (Outcome) and
             moves the state; a refused call leaves the state as it was.
Trees        the TLAS the scene must hold, byte for byte: the oracle's tree built from scratch after a rebuilding commit, the numpy refit
             of the kept topology to the oracle's leaf boxes after a refitting one.
walk         walk(seed, regime, n_ops) -> a list of operations as plain data (tuples of names, ints and floats; arrays are named by
             seeds).  Any prefix is itself a walk.
run          run(ops, oracle=None) -> (model, outcomes): the operations applied to a fresh Model.  tests/test_gpu_lifecycle_walk.py's
             run(ops) drives the product beside the same model.

Operations (h = the ordinal of a handle in creation order, 0-based; its id is h + 1)
  host mutations   ("push", kind, gseed, m, xseed, span)             a geometry of its own
                   ("push_shared", kind, gseed, ((m, xseed), ...), span)   add_geometry + one push_instances per part
                   ("push_mesh", gseed, m, xseed, span)
                   ("delete", h)   ("update_transforms", h, xseed, m, span)   ("update", h, kind, gseed)   ("update_mesh", h, gseed)
  sync             ("sync",)   followed by a second sync, which must report noop
  device updates   ("utd", h, xseed, m, span)            update_transforms_device
                   ("ugd", h, form, gseed)               update_geometry_device_async; form "same" | "degen" | "wrong"
                   ("umd", h, gseed, normals)            update_mesh_vertices_device_async
                   ("ibr", h, xseed, how, span)          instance_buffer written from a tensor, committed by refit_device(recompute =
                                                         how) for how 0 | 1, by the asynchronous refit / rebuild for "refit" | "rebuild"
  device commits   ("refit",)   ("rebuild",)   ("gated", ratio)
  status           ("wait",)    wait_for_gpu: reports the deferred RC_ERR_GEOMETRY_CHANGED once
  captured         ("capture", h, geo, commit, ratio)    update_transforms_device -> [update_geometry_device_async] -> commit -> trace_device
                                                         captured into one graph (the same chain has just run eagerly on the stream)
                   ("replay", xseed, gseed, span)        new transforms (and a new soup) written into the captured tensors, one replay
                   ("release",)                          the graph deleted, option release_captures set
  readers          ("get_instances", h)  ("world_bound",)  ("exports",)  ("counts",)  ("quality",)  ("save_load",)  ("blas4_build", h)
                   ("blas4_trace", h)  ("collide",)  ("vf",)  ("shading",)  ("trace",)
"""
import numpy as np

import auto_rebuild_model as arm

RC_ERR_INVALID_ARGUMENT, RC_ERR_INVALID_HANDLE, RC_ERR_NOT_SYNCED, RC_ERR_GEOMETRY_CHANGED = 1, 2, 6, 8
ERROR_NAMES = {1: "RC_ERR_INVALID_ARGUMENT", 2: "RC_ERR_INVALID_HANDLE", 6: "RC_ERR_NOT_SYNCED", 8: "RC_ERR_GEOMETRY_CHANGED"}

SOUP_KINDS = ("tri", "fan", "rand60", "degen", "big")  # + the indexed mesh: the geometry pool
HOST_MUTATIONS = ("push", "push_shared", "push_mesh", "delete", "update_transforms", "update", "update_mesh")
DEVICE_UPDATES = ("utd", "ugd", "umd")
COMMITS = ("refit", "rebuild", "gated", "sync")
READERS = ("get_instances", "world_bound", "exports", "counts", "quality", "save_load", "blas4_build", "blas4_trace", "collide", "vf",
           "shading", "trace")
OP_KINDS = HOST_MUTATIONS + ("sync",) + DEVICE_UPDATES + ("ibr", "refit", "rebuild", "gated", "wait") + READERS
CAPTURE_OPS = ("capture", "replay", "release")
N_REPLAYS = 6
# what each reader needs (the header's words): "synced" = RC_ERR_NOT_SYNCED with anything pending, host-side or device-side;
# "resident" = refused only while HOST-side mutations are pending (tlas_quality reads the state of the synced scene); "any" = never refused
READER_NEEDS = {"get_instances": "any", "world_bound": "any", "counts": "any", "blas4_build": "any", "blas4_trace": "any",
                "quality": "resident", "exports": "synced", "save_load": "synced", "collide": "synced", "vf": "synced", "shading": "synced",
                "trace": "synced"}
REGIMES = {  # live instances kept in [lo, hi]; m: instances per handle; the 256-instance split lies between fused and chain
    "fused": {"lo": 40, "hi": 200, "m": (6, 40), "fused": 1},
    "fused0": {"lo": 40, "hi": 200, "m": (6, 40), "fused": 0},   # the same walk shapes through the chain of build kernels
    "chain": {"lo": 300, "hi": 700, "m": (60, 160), "fused": 1},
    "tiny": {"lo": 0, "hi": 2, "m": (1, 2), "fused": 1},
}
# the walks tests/test_gpu_lifecycle_walk.py runs, 120 operations each; tests/test_lifecycle_model.py asserts what they cover
SEEDS = {"fused": (2, 11, 18), "fused0": (1, 3, 20), "chain": (1, 12, 14), "tiny": (2, 7, 33)}
N_WORLD_RAYS, N_AIMED_MAX, AIMED_PER_INSTANCE = 2048, 2048, 4


# ---- arrays from seeds ------------------------------------------------------------------------------------------------------------------
def _rng(seed, tag):
    return np.random.Generator(np.random.Philox(key=[int(seed), int(tag)]))


def _rotations(g, n):
    """Uniform random rotations (Shoemake), (n, 3, 3) float64."""
    u = g.uniform(size=(n, 3))
    x, y, z, w = (np.sqrt(1 - u[:, 0]) * np.sin(2 * np.pi * u[:, 1]), np.sqrt(1 - u[:, 0]) * np.cos(2 * np.pi * u[:, 1]),
                  np.sqrt(u[:, 0]) * np.sin(2 * np.pi * u[:, 2]), np.sqrt(u[:, 0]) * np.cos(2 * np.pi * u[:, 2]))
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                     2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)


def _fan_sphere(lon, bands, radius):
    """Closed sphere with pole fans: 2 lon (bands - 1) triangles, none degenerate, (n, 3, 3) float64."""
    th = np.linspace(0.0, np.pi, bands + 1)[1:-1]
    ph = np.arange(lon) * (2 * np.pi / lon)
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones_like(ph))], axis=-1)
    nxt = np.roll(ring, -1, axis=1)
    north, south = np.array([0, 0, 1.0]), np.array([0, 0, -1.0])
    tris = [np.stack([np.broadcast_to(north, (lon, 3)), ring[0], nxt[0]], axis=1)]
    for k in range(bands - 2):
        a, b, c, d = ring[k], ring[k + 1], nxt[k + 1], nxt[k]
        tris += [np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)]
    tris.append(np.stack([np.broadcast_to(south, (lon, 3)), nxt[-1], ring[-1]], axis=1))
    return np.concatenate(tris, axis=0) * radius


N_VALID = {"tri": 1, "fan": 64, "rand60": 60, "degen": 40, "big": 1500}


def degenerate_faces(seed, k):
    """k faces with two equal vertices: (v3 - v1) x (v2 - v1) is exactly zero."""
    p = _rng(seed, 7).uniform(-0.4, 0.4, size=(k, 2, 3))
    return np.ascontiguousarray(np.concatenate([p[:, :1], p[:, :1], p[:, 1:]], axis=1).reshape(k, 9), dtype=np.float32)


def soup(kind, seed, form="same"):
    """(n, 9) float32 around the origin, within radius ~1, under a rotation of its own (no axis-aligned faces, no duplicated triangles).
    N_VALID[kind] faces are non-degenerate whatever the seed; "degen" carries 3 + seed % 4 degenerate faces behind them.  form "degen":
    two more degenerate faces behind; form "wrong": one more VALID face (another count)."""
    g = _rng(seed, 1)
    if kind == "tri":
        t = g.uniform(-0.5, 0.5, size=(1, 3, 3))
    elif kind == "fan":
        t = _fan_sphere(8, 5, g.uniform(0.35, 0.5))
    elif kind == "big":
        t = _fan_sphere(30, 26, g.uniform(0.4, 0.5))
    elif kind in ("rand60", "degen"):
        n = N_VALID[kind]
        t = g.uniform(-0.3, 0.3, size=(n, 1, 3)) + g.uniform(-0.35, 0.35, size=(n, 3, 3))
    else:
        raise ValueError(kind)
    t = t @ _rotations(g, 1)[0].T
    out = np.ascontiguousarray(t.reshape(-1, 9), dtype=np.float32)
    assert len(out) == N_VALID[kind]
    if form == "wrong":
        out = np.concatenate([out, _rng(seed, 8).uniform(-0.3, 0.3, size=(1, 9)).astype(np.float32)])
    if kind == "degen":
        out = np.concatenate([out, degenerate_faces(seed, 3 + seed % 4)])
    if form == "degen":
        out = np.concatenate([out, degenerate_faces(seed + 1, 2)])
    return np.ascontiguousarray(out)


MESH_N = 5  # (MESH_N + 1)^2 = 36 vertices, 2 MESH_N^2 = 50 faces


def mesh(seed):
    """An indexed grid mesh with normals and uvs: (verts (36, 3), faces (50, 3) uint32, normals (36, 3), uvs (36, 2)).  Faces and uvs are
    the same for every seed; vertices (a bumpy sheet under a rotation of its own) and normals follow the seed."""
    g = _rng(seed, 2)
    n = MESH_N
    xs, ys = np.meshgrid(np.linspace(-0.5, 0.5, n + 1), np.linspace(-0.5, 0.5, n + 1), indexing="ij")
    z = g.uniform(0.05, 0.15) * np.sin(6 * xs + g.uniform(0, 3)) * np.cos(5 * ys + g.uniform(0, 3))
    v = np.stack([xs, ys, z], -1).reshape(-1, 3) @ _rotations(g, 1)[0].T
    nrm = g.normal(size=v.shape)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    uv = np.stack([xs + 0.5, ys + 0.5], -1).reshape(-1, 2)
    idx = lambda i, j: i * (n + 1) + j
    faces = [f for i in range(n) for j in range(n) for f in ([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)])]
    return v.astype(np.float32), np.array(faces, np.uint32), nrm.astype(np.float32), uv.astype(np.float32)


def xforms(seed, m, span):
    """(m, 12) float32 Mat3x4f: generic rotation x scale in [0.6, 1] | position uniform in a cube of side `span` around the origin."""
    g = _rng(seed, 3)
    R = _rotations(g, m) * g.uniform(0.6, 1.0, size=(m, 1, 1))
    pos = g.uniform(-0.5 * span, 0.5 * span, size=(m, 3))
    return np.ascontiguousarray(np.concatenate([R, pos[:, :, None]], axis=2).reshape(m, 12), dtype=np.float32)


def instance_ids(seed, m):
    return _rng(seed, 4).integers(0, 100000, size=m).astype(np.uint32)


# ---- the model --------------------------------------------------------------------------------------------------------------------------
class Geom:
    def __init__(self, kind):
        self.kind = kind          # the pool kind of a soup, "mesh" for an indexed mesh
        self.verts = None         # soup: (n, 9), degenerate faces included
        self.mesh = None          # mesh: [verts, faces, normals, uvs]
        self.blas4 = False
        self.blas4_was = False    # a BLAS4 was built at some time (the generator looks here for ones that were dropped since)

    @property
    def is_mesh(self):
        return self.mesh is not None

    def set_soup(self, kind, verts):
        self.kind, self.verts, self.mesh, self.blas4 = kind, verts, None, False

    def set_mesh(self, parts):
        self.kind, self.verts, self.mesh, self.blas4 = "mesh", None, list(parts), False

    def triangles(self):
        """(n, 3, 3) float32 of the faces as given (for bounding spheres)."""
        if self.is_mesh:
            return self.mesh[0][self.mesh[1]]
        return self.verts.reshape(-1, 3, 3)


class Handle:
    def __init__(self, geom, xf, ids):
        self.geom, self.xf, self.ids = geom, xf, ids
        self.deleted = False     # rc_delete has run
        self.compacted = False   # ... and a rebuilding rc_sync has dropped the instances: the id is unknown from then on

    @property
    def m(self):
        return len(self.xf)


class Outcome:
    """What one call must do.  error: None or the RC_ERR_* code raised (for "wait": the deferred RC_ERR_GEOMETRY_CHANGED); value: what
    it returns where the model knows (delete's bool, the new handles' ordinals); action: last_sync_action after a sync; commit: None, or
    the tree class the call leaves ("fresh" | "refitted") -- a check point; gate: the gated rebuild's decision (None when it did not
    decide)."""

    def __init__(self, error=None, value=None, action=None, commit=None, gate=None):
        self.error, self.value, self.action, self.commit, self.gate = error, value, action, commit, gate

    def __repr__(self):
        return f"Outcome(error={ERROR_NAMES.get(self.error, self.error)}, value={self.value}, action={self.action}, commit={self.commit}, gate={self.gate})"


class Model:
    def __init__(self, oracle=None):
        self.geoms, self.handles = [], []
        self.has_static = False      # a rebuilding rc_sync has run
        self.struct_pending = False  # push / delete / update / update_mesh since the last sync                       ("dirty")
        self.xf_pending = False      # host update_transforms since the last sync                  ("transforms_dirty" + "mirror_edited")
        self.dev_pending = set()     # device-update kinds enqueued since the last commit             ("device_dirty", "transforms_dirty")
        self.pending_deletes = False
        self.geometry_error = False  # a wrong-count device geometry update: the next rc_wait reports it, once
        self.armed, self.evaluations, self.rebuilds, self.last_rebuilt = False, 0, 0, False               # ("quality_armed" + the block)
        self.tree = None             # "fresh" | "refitted"
        self.touched = set()         # (handle ordinal, instance index) changed since the previous check point
        self.version = 0             # advances with every change of what an oracle scene is built from
        self.trees = Trees(oracle) if oracle is not None else None
        self.updates_before_commit = []  # (device-update kinds, commit kind) of every commit: the coverage the CPU tests count
        self.captured = None         # (h, geo, commit, ratio) of the captured chain                ("captured_update / _refit / _deform")
        self.captured_alive = False  # ... and no rebuilding rc_sync, no host-side mutation since: only then may it be replayed

    # -- state ---------------------------------------------------------------------------------------------------------------------------
    @property
    def host_pending(self):
        return self.struct_pending or self.xf_pending

    @property
    def resident(self):
        """The device-side entry points write the arrays where the last rc_sync put them: synced once, nothing pending on the host."""
        return self.has_static and not self.host_pending

    @property
    def clean(self):
        """Queries run: synced, and neither host-side mutations nor device-side updates wait for their commit."""
        return self.resident and not self.dev_pending

    def valid(self, h):
        return 0 <= h < len(self.handles) and not self.handles[h].deleted

    def present(self):
        """Handles whose instances the instance array still holds (deleted ones stay until the compaction), ascending."""
        return [k for k, hd in enumerate(self.handles) if not hd.compacted]

    def live(self):
        return [k for k, hd in enumerate(self.handles) if not hd.deleted]

    def n_live(self):
        return sum(self.handles[k].m for k in self.live())

    def n_total(self):
        return sum(self.handles[k].m for k in self.present())

    def counts(self):
        return self.n_live(), self.n_total(), len(self.geoms)

    def blas_index(self, geom):
        """1-based, as InstanceDescriptor stores it: renumbered when a rebuilding rc_sync after rc_delete drops unreferenced geometries."""
        return 1 + next(i for i, g in enumerate(self.geoms) if g is geom)

    def first_instance(self, h):
        return sum(self.handles[k].m for k in self.present() if k < h)

    def quality(self):
        return {"armed": self.armed, "evaluations": self.evaluations, "rebuilds": self.rebuilds, "last_rebuilt": self.last_rebuilt}

    def handles_of(self, geom):
        return [k for k in self.present() if self.handles[k].geom is geom]

    def _touch(self, h):
        self.touched.update((h, i) for i in range(self.handles[h].m))

    def _touch_geom(self, geom):
        for k in self.handles_of(geom):
            if not self.handles[k].deleted:
                self._touch(k)

    # -- apply ---------------------------------------------------------------------------------------------------------------------------
    def apply(self, op):
        """The Outcome of `op` in the current state; the state moves only if the call is not refused."""
        out = getattr(self, "_op_" + op[0])(*op[1:])
        if out.error is None or op[0] == "wait":
            self.version += 1
        return out

    def _handle_error(self, h):
        return None if self.valid(h) else RC_ERR_INVALID_HANDLE

    def _host_mutation(self):
        self.captured_alive = False  # (a rebuilding rc_sync frees what the graph addresses; a host update of its geometry does so at once)

    def _add_handle(self, geom, m, xseed, span):
        self._host_mutation()
        self.handles.append(Handle(geom, xforms(xseed, m, span), instance_ids(xseed, m)))
        self.struct_pending = True
        self._touch(len(self.handles) - 1)
        return len(self.handles) - 1

    def _op_push(self, kind, gseed, m, xseed, span):
        g = Geom(kind)
        g.set_soup(kind, soup(kind, gseed))
        self.geoms.append(g)
        return Outcome(value=[self._add_handle(g, m, xseed, span)])

    def _op_push_shared(self, kind, gseed, parts, span):
        g = Geom(kind)
        g.set_soup(kind, soup(kind, gseed))
        self.geoms.append(g)
        return Outcome(value=[self._add_handle(g, m, xseed, span) for m, xseed in parts])

    def _op_push_mesh(self, gseed, m, xseed, span):
        g = Geom("mesh")
        g.set_mesh(mesh(gseed))
        self.geoms.append(g)
        return Outcome(value=[self._add_handle(g, m, xseed, span)])

    def _op_delete(self, h):
        if not self.valid(h):  # idempotent: *deleted = 0, no error
            return Outcome(value=False)
        self._host_mutation()
        self.handles[h].deleted = True
        self.struct_pending = self.pending_deletes = True
        return Outcome(value=True)

    def _op_update_transforms(self, h, xseed, m, span):
        if self._handle_error(h):
            return Outcome(error=RC_ERR_INVALID_HANDLE)
        if m != self.handles[h].m:
            return Outcome(error=RC_ERR_INVALID_ARGUMENT)
        self._host_mutation()
        self.handles[h].xf = xforms(xseed, m, span)
        self.xf_pending = True
        self._touch(h)
        return Outcome()

    def _op_update(self, h, kind, gseed):
        if self._handle_error(h):
            return Outcome(error=RC_ERR_INVALID_HANDLE)
        self._host_mutation()
        self.handles[h].geom.set_soup(kind, soup(kind, gseed))  # replaces the BLAS the handle uses: every handle of the geometry sees it
        self.struct_pending = True
        self._touch_geom(self.handles[h].geom)
        return Outcome()

    def _op_update_mesh(self, h, gseed):
        if self._handle_error(h):
            return Outcome(error=RC_ERR_INVALID_HANDLE)
        self._host_mutation()
        self.handles[h].geom.set_mesh(mesh(gseed))
        self.struct_pending = True
        self._touch_geom(self.handles[h].geom)
        return Outcome()

    def sync_action(self):
        if not self.has_static or self.struct_pending:
            return "rebuild"
        return "refit" if (self.xf_pending or self.dev_pending) else "noop"

    def _op_sync(self):
        action = self.sync_action()
        if action == "noop":
            return Outcome(action=action)
        kinds = sorted(self.dev_pending)
        if action == "rebuild":
            if self.pending_deletes:  # compact_instances!: deleted handles leave, geometries nobody references leave, the rest is renumbered
                for hd in self.handles:
                    hd.compacted = hd.compacted or hd.deleted
                used = {id(self.handles[k].geom) for k in self.present()}
                self.geoms = [g for g in self.geoms if id(g) in used]
                self.pending_deletes = False
            self.has_static = True
            self.armed, self.evaluations, self.rebuilds, self.last_rebuilt = False, 0, 0, False  # the state block is zeroed and disarmed
        self.struct_pending = self.xf_pending = False
        self.dev_pending = set()
        return self._commit("sync", kinds, "fresh" if action == "rebuild" else "refitted", action=action)

    def _commit(self, kind, kinds, cls, action=None, gate=None):
        self.tree = cls
        self.version += 1
        self.updates_before_commit.append((tuple(kinds), kind))
        if self.trees is not None:
            self.trees.commit(self, cls)
        return Outcome(action=action, commit=cls, gate=gate)

    def _device_entry_error(self, h=None):
        if h is not None and self._handle_error(h):
            return RC_ERR_INVALID_HANDLE
        return None if self.resident else RC_ERR_NOT_SYNCED

    def _op_utd(self, h, xseed, m, span):
        if self._handle_error(h):
            return Outcome(error=RC_ERR_INVALID_HANDLE)
        if m != self.handles[h].m:
            return Outcome(error=RC_ERR_INVALID_ARGUMENT)
        if not self.resident:
            return Outcome(error=RC_ERR_NOT_SYNCED)
        self.handles[h].xf = xforms(xseed, m, span)
        self.dev_pending.add("utd")
        self._touch(h)
        return Outcome()

    def _op_ugd(self, h, form, gseed):
        err = self._device_entry_error(h)
        if err:
            return Outcome(error=err)
        g = self.handles[h].geom
        assert not g.is_mesh, "the walk updates soups with soups and meshes through their vertices"
        g.blas4 = False  # dropped AT CALL TIME, whatever the device then finds
        if form == "wrong":
            self.geometry_error = True  # nothing a trace, an export or a later sync reads is modified
        else:
            g.verts = soup(g.kind, gseed, form)
            self._touch_geom(g)
        self.dev_pending.add("ugd")  # scene state: exactly as after rc_update_transforms_device
        return Outcome()

    def _op_umd(self, h, gseed, normals):
        err = self._device_entry_error(h)
        if err:
            return Outcome(error=err)
        g = self.handles[h].geom
        if not g.is_mesh:
            return Outcome(error=RC_ERR_INVALID_ARGUMENT)  # a geometry that is not a mesh
        v, _, nrm, _ = mesh(gseed)
        g.mesh[0] = v
        if normals:
            g.mesh[2] = nrm
        g.blas4 = False
        self.dev_pending.add("umd")
        self._touch_geom(g)
        return Outcome()

    def _op_ibr(self, h, xseed, how, span):
        if self._handle_error(h):
            return Outcome(error=RC_ERR_INVALID_HANDLE)
        if not self.clean:  # rc_instance_buffer_device wants the synced scene
            return Outcome(error=RC_ERR_NOT_SYNCED)
        self.handles[h].xf = xforms(xseed, self.handles[h].m, span)
        self._touch(h)
        self.version += 1
        if how in (0, 1):
            return self._commit("ibr", (), "refitted")
        return self._device_commit(how)  # "with none since the last refit ... it is derived from the descriptors first"

    def _op_capture(self, h, geo, commit, ratio):
        assert self.clean and self.valid(h) and self.captured is None, "the walk captures on a synced scene, one graph at a time"
        assert commit != "gated" or self.armed, "the arming call must be eager"
        self.captured, self.captured_alive = (h, geo, commit, ratio), True
        return Outcome()  # capturing runs nothing

    def _op_replay(self, xseed, gseed, span):
        assert self.captured is not None and self.captured_alive and self.clean, "a dead graph must never be replayed"
        h, geo, commit, ratio = self.captured
        assert self._op_utd(h, xseed, self.handles[h].m, span).error is None
        if geo:
            assert self._op_ugd(h, "same", gseed).error is None
        self.version += 1  # (the gate below is decided from the oracle's scene of the NEW transforms, whoever read the cached one before)
        return self._device_commit(commit, ratio)

    def _op_release(self):
        self.captured, self.captured_alive = None, False
        return Outcome()

    def _device_commit(self, kind, ratio=None):
        if not self.resident:
            return Outcome(error=RC_ERR_NOT_SYNCED)
        kinds, self.dev_pending = sorted(self.dev_pending), set()
        n = self.n_total()
        if n == 0:  # success, nothing enqueued; the state block stays disarmed
            return self._commit(kind, kinds, self.tree)
        gate = None
        if kind == "refit":
            cls = "refitted"
        elif kind == "rebuild":
            cls = "fresh"
            if self.armed:  # while armed the explicit rebuild appends the record step
                self.rebuilds += 1
        elif not self.armed:  # the arming call: refit -> unconditional rebuild -> baseline; one evaluation, one rebuild
            self.armed, self.last_rebuilt, cls = True, True, "fresh"
            self.evaluations += 1
            self.rebuilds += 1
        else:
            gate = bool(n >= 2 and self.trees is not None and self.trees.gate(self, ratio))  # one instance: cost 1.0, never rebuilt
            self.evaluations += 1
            self.rebuilds += int(gate)
            self.last_rebuilt, cls = gate, ("fresh" if gate else "refitted")
        return self._commit(kind, kinds, cls, gate=gate)

    def _op_refit(self):
        return self._device_commit("refit")

    def _op_rebuild(self):
        return self._device_commit("rebuild")

    def _op_gated(self, ratio):
        return self._device_commit("gated", ratio)

    def _op_wait(self):
        err, self.geometry_error = (RC_ERR_GEOMETRY_CHANGED if self.geometry_error else None), False
        return Outcome(error=err)

    def _reader(self, name, h=None):
        if h is not None and self._handle_error(h):
            return Outcome(error=RC_ERR_INVALID_HANDLE)
        need = READER_NEEDS[name]
        ok = True if need == "any" else (self.resident if need == "resident" else self.clean)
        return Outcome(error=None if ok else RC_ERR_NOT_SYNCED)

    def _op_get_instances(self, h):
        return self._reader("get_instances", h)

    def _op_blas4_build(self, h):
        out = self._reader("blas4_build", h)
        if out.error is None:
            self.handles[h].geom.blas4 = self.handles[h].geom.blas4_was = True
        return out

    def _op_blas4_trace(self, h):
        out = self._reader("blas4_trace", h)
        if out.error is None and not self.handles[h].geom.blas4:
            return Outcome(error=RC_ERR_NOT_SYNCED)  # "as for a geometry whose BLAS4 was never built, until rc_blas4_build"
        return out


for _name in ("world_bound", "exports", "counts", "quality", "save_load", "collide", "vf", "shading", "trace"):
    setattr(Model, "_op_" + _name, (lambda name: lambda self: self._reader(name))(_name))


# ---- the oracle's scene of a model, the tree it must hold, the rays of a check point ------------------------------------------------------
def oracle_scene(oracle, model):
    """oracle.Scene built from scratch: surviving geometries in creation order, handles ascending.  Cached on the model's version."""
    cached = getattr(model, "_oracle_cache", None)
    if cached is not None and cached[0] == model.version:
        return cached[1]
    o = oracle.Scene()
    for g in model.geoms:
        if g.is_mesh:
            o.add_mesh(g.mesh[0], g.mesh[1], g.mesh[2], g.mesh[3])
        else:
            o.add_blas(g.verts)
    for k in model.present():
        hd = model.handles[k]
        b = model.blas_index(hd.geom)
        for x, i in zip(hd.xf, hd.ids):
            o.add_instance(b, x, int(i))
    o.build()
    model._oracle_cache = (model.version, o)
    return o


class Trees:
    """The TLAS nodes the scene must hold after every commit, and the cost baseline of the gated rebuild, from the oracle and numpy."""

    def __init__(self, oracle):
        self.oracle = oracle
        self.nodes = None        # the tree after the latest commit (reference layout, as rc_export_tlas_nodes gives it)
        self.cost_built = None   # the cost of the tree at the latest RECORDED rebuild (armed scenes)
        self.is_fresh = True     # the tree is byte for byte the oracle's
        self.decisions = []      # (cost, ratio * cost_built) of every gate decision: the CPU tests ask for room on both sides

    def _fresh(self, model):
        o = oracle_scene(self.oracle, model)
        return o.tlas_nodes, len(o.instances)

    def _refitted(self, model):
        fresh, n = self._fresh(model)
        return (arm.refit(self.nodes, fresh, n) if n else fresh), fresh, n

    def gate(self, model, ratio):
        """cost(the refitted tree) > ratio * cost_built, in f64 as the header writes it.  Called before the commit is recorded."""
        refitted, _, n = self._refitted(model)
        c = arm.cost(refitted, n)
        self.decisions.append((c, ratio * self.cost_built))
        return c > ratio * self.cost_built

    def commit(self, model, cls):
        if cls == "fresh":
            self.nodes, n = self._fresh(model)
            if model.armed and n:
                self.cost_built = arm.cost(self.nodes, n)
            self.is_fresh = True
        elif cls == "refitted":
            self.nodes, fresh, n = self._refitted(model)
            self.is_fresh = self.nodes.tobytes() == fresh.tobytes()
        if not model.armed:
            self.cost_built = None


def bounding_sphere(geom):
    """(centre, radius, aim) in the geometry's own space.  aim: the centroid of the face nearest to the centre -- an open soup or a sheet
    has nothing at the centre itself, and a ray from outside the sphere towards a point ON the geometry meets this instance first unless
    another instance stands in front."""
    tri = geom.triangles().astype(np.float64)
    t = tri.reshape(-1, 3)
    c = t.mean(axis=0)
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    mid = tri.mean(axis=1)
    dist = np.where(area > 0, np.linalg.norm(mid - c, axis=1), np.inf)
    return c, float(np.linalg.norm(t - c, axis=1).max()), mid[int(np.argmin(dist))]


def checkpoint_rays(oracle, model, seed):
    """The ray batch of a check point and the instances the aimed part is about: (rays, [(first ray, n rays, 0-based instance index)]).
    2 048 rays over the world bound (origins on a sphere around it; the targets of one half uniform inside it, those of the other half
    uniform inside the world box of an instance drawn for each ray, so that a sparse scene is not traced through its gaps alone); then, for the instances touched since
    the previous check point (the first N_AIMED_MAX // AIMED_PER_INSTANCE of them), AIMED_PER_INSTANCE rays each from just outside the
    instance's bounding sphere towards the centroid of its face nearest to the sphere's centre (bounding_sphere says why not the centre)."""
    o = oracle_scene(oracle, model)
    g = _rng(seed, 5)
    wb = o.world_bound.astype(np.float64)
    if not np.all(np.isfinite(wb)):  # the empty scene
        wb = np.array([-1, -1, -1, 1, 1, 1], dtype=np.float64)
    lo, hi = wb[:3], wb[3:]
    centre, radius = 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo)) + 0.5
    d = g.normal(size=(N_WORLD_RAYS, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    origins = [centre + radius * d]
    targets = [g.uniform(lo, hi, size=(N_WORLD_RAYS, 3))]
    n = len(o.instances)
    if n:
        leaves = o.tlas_nodes[n - 1:]
        pick = g.integers(0, n, size=N_WORLD_RAYS // 2)
        blo, bhi = leaves["aabb0_min"][pick].astype(np.float64), leaves["aabb0_max"][pick].astype(np.float64)
        targets[0][N_WORLD_RAYS // 2:] = blo + g.uniform(size=blo.shape) * (bhi - blo)
    aimed, at = [], N_WORLD_RAYS
    touched = sorted(t for t in model.touched if not model.handles[t[0]].deleted)[:N_AIMED_MAX // AIMED_PER_INSTANCE]
    for h, i in touched:
        hd = model.handles[h]
        c, r, aim = bounding_sphere(hd.geom)
        M = hd.xf[i].astype(np.float64).reshape(3, 4)
        wc, wa = M[:, :3] @ c + M[:, 3], M[:, :3] @ aim + M[:, 3]
        wr = r * float(np.linalg.norm(M[:, :3], 2)) * 1.05 + 1e-3
        dd = g.normal(size=(AIMED_PER_INSTANCE, 3))
        dd /= np.linalg.norm(dd, axis=1, keepdims=True)
        origins.append(wc + wr * dd)
        targets.append(np.broadcast_to(wa, (AIMED_PER_INSTANCE, 3)))
        aimed.append((at, AIMED_PER_INSTANCE, model.first_instance(h) + i))
        at += AIMED_PER_INSTANCE
    origins, targets = np.concatenate(origins), np.concatenate(targets)
    dirs = targets - origins
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    return oracle.make_rays(origins, dirs), aimed


def liveness(hits, aimed):
    """(fraction of all rays that hit, fraction of the aimed instances that are the closest hit of one of their own rays)."""
    own = [bool(np.any((hits["hit"][a:a + k] == 1) & (hits["instance_id"][a:a + k] == inst))) for a, k, inst in aimed]
    return float(np.mean(hits["hit"] == 1)), (float(np.mean(own)) if own else 1.0)


# ---- the walk ---------------------------------------------------------------------------------------------------------------------------
def span_for(n):
    """The side of the cube the positions are drawn in: about three instance diameters of room per instance."""
    return round(1.5 * max(n, 1) ** (1.0 / 3.0) + 0.5, 3)


class _Walker:
    def __init__(self, seed, regime, n_ops):
        self.g = _rng(seed, 6 + 16 * list(REGIMES).index(regime))
        self.cfg, self.tiny, self.n_ops = REGIMES[regime], regime == "tiny", n_ops
        self.m = Model()
        self.ops = []
        self.span = 1.0 if self.tiny else span_for(0.5 * (self.cfg["lo"] + self.cfg["hi"]))
        self.big_used = False
        self.segment_done = False

    def emit(self, op):
        if len(self.ops) < self.n_ops:
            self.m.apply(op)
            self.ops.append(op)

    def seed(self):
        return int(self.g.integers(1, 1 << 30))

    def pick(self, seq):
        return seq[int(self.g.integers(0, len(seq)))]

    def chance(self, p):
        return bool(self.g.uniform() < p)

    def others_not_tri(self, but=None):
        """A live handle other than `but` holds something else than the single triangle."""
        return any(self.m.handles[k].geom.kind != "tri" for k in self.m.live() if k != but and self.m.handles[k].geom is not (None if but is None else self.m.handles[but].geom))

    def kind(self, but=None):
        k = self.pick(SOUP_KINDS)
        if k == "tri" and self.tiny and not self.others_not_tri(but):
            k = "fan"  # (a lone triangle in its own world bound: hardly a ray of the check point would hit)
        if k == "big":  # one geometry of about 1 500 triangles per walk keeps the flat arrays (and the view-factor matrix) small
            if self.big_used:
                return "rand60"
            self.big_used = True
        return k

    def handle_size(self, room):
        lo, hi = self.cfg["m"]
        return int(self.g.integers(min(lo, room), min(hi, room) + 1))

    # -- phrases -------------------------------------------------------------------------------------------------------------------------
    def push_some(self):
        room = self.cfg["hi"] - self.m.n_live()
        if room < 1:
            return False
        r = self.g.uniform()
        if r < 0.4:
            self.emit(("push", self.kind(), self.seed(), self.handle_size(room), self.seed(), self.span))
        elif r < 0.7 and room >= 2:
            a = self.handle_size(room // 2)
            b = self.handle_size(room - a)
            self.emit(("push_shared", self.kind(), self.seed(), ((a, self.seed()), (b, self.seed())), self.span))
        else:
            self.emit(("push_mesh", self.seed(), self.handle_size(room), self.seed(), self.span))
        return True

    def delete_some(self):
        live = [k for k in self.m.live() if self.m.n_live() - self.m.handles[k].m >= self.cfg["lo"]]
        if self.tiny:  # (never leave single triangles alone)
            rest = lambda k: [j for j in self.m.live() if j != k]
            live = [k for k in live if not rest(k) or any(self.m.handles[j].geom.kind != "tri" for j in rest(k))]
        if not live:
            return False
        self.emit(("delete", self.pick(live)))
        return True

    def host_mutation(self):
        live = self.m.live()
        n = self.m.n_live()
        if not live or n < self.cfg["lo"] + (self.cfg["hi"] - self.cfg["lo"]) // 4:
            if self.push_some():
                return
        r = self.g.uniform()
        if r < 0.22 and self.push_some():
            return
        if r < 0.42 and self.delete_some():
            return
        if not live:
            return
        h = self.pick(live)
        if r < 0.70:
            self.emit(("update_transforms", h, self.seed(), self.m.handles[h].m, self.span))
        elif r < 0.88:
            self.emit(("update", h, self.kind(but=h), self.seed()))
        else:
            self.emit(("update_mesh", h, self.seed()))

    def reader(self, among=READERS):
        name = self.pick(among)
        if name in ("get_instances", "blas4_build", "blas4_trace"):
            live = self.m.live()
            if not live:
                name = "counts"
            else:
                h = self.pick(live)
                if name == "blas4_trace" and self.chance(0.7):  # more often one that was built (or built and dropped since)
                    built = [k for k in live if self.m.handles[k].geom.blas4_was]
                    h = self.pick(built) if built else h
                return self.emit((name, h))
        self.emit((name,))

    def device_update(self):
        live = self.m.live()
        if not live:
            return
        r = self.g.uniform()
        shared = [k for k in live if len(self.m.handles_of(self.m.handles[k].geom)) > 1]
        meshes = [k for k in live if self.m.handles[k].geom.is_mesh]
        soups = [k for k in live if not self.m.handles[k].geom.is_mesh]
        which = self.pick(("utd",) + (("ugd",) if soups else ()) + (("umd", "umd") if meshes else ()))
        if which == "utd":
            h = self.pick(shared) if shared and self.chance(0.4) else self.pick(live)
            self.emit(("utd", h, self.seed(), self.m.handles[h].m, self.span))
        elif self.chance(0.5):  # lazy state made valid first, so that the update has something to invalidate
            h = self.pick(soups if which == "ugd" else meshes)
            self.emit(self.pick((("vf",), ("shading",), ("blas4_build", h))) if self.m.clean else ("blas4_build", h))
            self.emit(("ugd", h, self.pick(("same", "degen")), self.seed()) if which == "ugd" else ("umd", h, self.seed(), int(self.chance(0.5))))
        elif which == "ugd":
            self.emit(("ugd", self.pick(soups), self.pick(("same", "same", "degen", "degen", "wrong")), self.seed()))
        else:
            self.emit(("umd", self.pick(meshes), self.seed(), int(self.chance(0.5))))

    def commit(self):
        k = self.pick(COMMITS + ("gated",))
        arming = k == "gated" and not self.m.armed
        deformed = bool(self.m.dev_pending & {"ugd", "umd"})
        self.emit(("gated", self.pick((0.5, 1.0001, 1.0e6))) if k == "gated" else (k,))
        if arming and self.m.live() and self.chance(0.7):  # the arming call decides nothing: move something and ask again
            h = self.pick(self.m.live())
            self.emit(("utd", h, self.seed(), self.m.handles[h].m, self.span))
            self.emit(("gated", self.pick((0.5, 1.0001, 1.0e6))))
        if self.m.geometry_error and self.chance(0.8) or self.chance(0.15):
            self.emit(("wait",))
        if self.m.clean and deformed and self.chance(0.7):  # what a geometry update must have invalidated is read right after its commit
            self.reader(("vf", "blas4_trace", "shading"))
        elif self.m.clean and self.chance(0.5):
            self.reader(("vf", "blas4_trace", "shading", "collide", "save_load", "get_instances", "quality", "world_bound"))

    def captured_segment(self):
        """The eager chain, its capture, N_REPLAYS replays with a reader after each, then a host push + sync and the release."""
        m = self.m
        live = m.live()
        soups = [k for k in live if not m.handles[k].geom.is_mesh and m.handles[k].geom.kind != "degen"]  # (a soup of constant length)
        geo = bool(soups) and self.chance(0.6)
        h = self.pick(soups) if geo else self.pick(live)
        commit, ratio = self.pick(("refit", "rebuild", "gated", "gated")), self.pick((0.5, 1.0001, 1.0e6))
        if commit == "gated":
            ratio = 1.0001  # with the repeated frames below one graph takes both decisions
        if commit == "gated" and not m.armed:
            self.emit(("gated", ratio))  # the arming call
        self.emit(("utd", h, self.seed(), m.handles[h].m, self.span))
        if geo:
            self.emit(("ugd", h, "same", self.seed()))
        self.emit(("gated", ratio) if commit == "gated" else (commit,))
        self.emit(("capture", h, geo, commit, ratio))
        frame = None
        for r in range(N_REPLAYS):
            # a gated chain sees every other frame twice: new positions degrade the refitted tree (the gate opens), the same ones again
            # find the tree just built (cost == cost_built: it stays shut)
            frame = frame if commit == "gated" and r in (1, 3) else (self.seed(), self.seed())
            self.emit(("replay", frame[0], frame[1], self.span))
            self.reader(("get_instances", "world_bound", "exports", "counts", "quality", "save_load", "collide", "vf", "shading", "trace"))
        if not self.push_some():
            self.delete_some()
        self.emit(("sync",))
        self.emit(("release",))
        self.segment_done = True

    def refused(self):
        """One call the state refuses (or that does nothing), and nothing else: never two reasons at once."""
        live, r = self.m.live(), self.g.uniform()
        gone = [k for k, hd in enumerate(self.m.handles) if hd.compacted]
        soups = [k for k in live if not self.m.handles[k].geom.is_mesh]
        if r < 0.2 and gone:
            h = self.pick(gone)
            self.emit(self.pick((("utd", h, self.seed(), self.m.handles[h].m, self.span), ("get_instances", h), ("update_transforms", h, self.seed(), self.m.handles[h].m, self.span),
                                 ("ugd", h, "same", self.seed()), ("delete", h), ("update", h, "fan", self.seed()))))
        elif r < 0.45 and live:
            h = self.pick(live)
            self.emit((self.pick(("utd", "update_transforms")), h, self.seed(), self.m.handles[h].m + 1, self.span))
        elif r < 0.6 and soups and self.m.clean:
            self.emit(("umd", self.pick(soups), self.seed(), 0))
        elif r < 0.8 and live:
            self.emit(("blas4_trace", self.pick(live)))
        else:
            self.emit(("wait",))

    def walk(self):
        m = self.m
        if not self.tiny:  # into the regime's range before the first sync
            while m.n_live() < self.cfg["lo"] + (self.cfg["hi"] - self.cfg["lo"]) // 4 and len(self.ops) < self.n_ops:
                self.push_some()
        while len(self.ops) < self.n_ops:
            if not m.resident:  # never synced, or host-side mutations pending: the device-side entry points and the queries are refused
                if m.has_static and self.chance(0.35):
                    live = m.live()
                    if live and self.chance(0.5):
                        h = self.pick(live)
                        self.emit(("utd", h, self.seed(), m.handles[h].m, self.span))
                    elif self.chance(0.5):
                        self.emit(self.pick((("refit",), ("rebuild",), ("gated", 2.0))))
                    else:
                        self.reader()
                elif self.chance(0.3):
                    self.host_mutation()
                self.emit(("sync",))
                continue
            if m.dev_pending:
                self.commit()
                continue
            if not self.segment_done and len(self.ops) >= 30 and m.live() and m.n_live() < self.cfg["hi"]:
                self.captured_segment()
                continue
            r = self.g.uniform()
            if r < 0.25:    # host churn, committed by the next round's sync
                for _ in range(int(self.g.integers(1, 4))):
                    self.host_mutation()
                    if self.chance(0.25):
                        self.reader()
            elif r < 0.62:  # device updates, a read in between, a commit
                if not m.live():
                    self.commit()  # the empty scene: every device call succeeds and enqueues nothing
                    continue
                for _ in range(int(self.g.integers(1, 3))):
                    self.device_update()
                    for _ in range(int(self.g.integers(0, 3))):  # reads between an update and its commit: harmless ones, refused ones
                        self.reader()
                if self.chance(0.2):  # a host-side mutation on top of the device's: only rc_sync commits both
                    self.host_mutation()
            elif r < 0.70:
                live = m.live()
                if live:
                    self.emit(("ibr", self.pick(live), self.seed(), self.pick((0, 1, "refit", "rebuild")), self.span))
            elif r < 0.92:
                for _ in range(int(self.g.integers(1, 4))):
                    self.reader()
            else:
                self.refused()
        return self.ops


def walk(seed, regime, n_ops):
    """The operation list of (seed, regime), n_ops long; a shorter n_ops gives a prefix of a longer one."""
    return _Walker(seed, regime, n_ops).walk()


def run(ops, oracle=None, on_outcome=None):
    """Apply `ops` to a fresh Model (with the oracle: its trees and gate decisions too).  on_outcome(index, op, outcome, model) is called
    after every operation.  -> (model, outcomes)"""
    model, outcomes = Model(oracle), []
    for k, op in enumerate(ops):
        out = model.apply(op)
        outcomes.append(out)
        if on_outcome is not None:
            on_outcome(k, op, out, model)
    return model, outcomes


def describe(seed, regime, ops, k):
    """The text a failing walk prints: seed, regime, the failing operation's index, and the prefix up to it (pasteable into run())."""
    lines = "\n".join(f"    {op!r}," for op in ops[:k + 1])
    return f"seed {seed}, regime {regime}, operation {k} {ops[k]!r}; the prefix up to it:\n[\n{lines}\n]"
