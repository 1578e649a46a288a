"""Host-side mirror of Raycore.jl's accel API for the TLAS/BLAS path, over the C ABI.

Names, argument meaning and error behaviour follow the reference (paths relative to the reference repo):
TLAS / push! / delete! / update_transform(s)! / update! / sync! / Adapt.adapt (src/instanced-bvh.jl:334-1102),
closest_hit / any_hit (:1902-2140), trace_rays (ext/RaycoreMakieExt.jl:81-87), get_illumination /
get_centroid / view_factors (src/kernels.jl:58-124).  Python has no `!`, so `push!` is `push`, etc.
Where the Julia API is 1-based (instance index returned by closest_hit, blas_index) this layer is 1-based
too; the C ABI underneath is 0-based.

Triangles are passed as (n, 9) float32 soup (v0 v1 v2) plus optional uint32 metadata: GeometryBasics mesh
decomposition is outside this path.  Transforms are 4x4 (rows 0..2 used, translation
in column 4, like Mat4f) or 12 floats in Mat3x4f byte order.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _capi
from ._capi import HIT_DT, RAY_DT, RaycoreError, check, lib, ptr

TLASHandle = namedtuple("TLASHandle", ["id"])  # src/instanced-bvh.jl:180-182
INVALID_HANDLE = TLASHandle(0)
# Triangle{UInt32} (src/triangle_mesh.jl:1-7).  Positional order (vertices, metadata) is kept for the path's own use; the
# shading fields default to None when a caller builds one by hand.
Triangle = namedtuple("Triangle", ["vertices", "metadata", "normals", "tangents", "uv"], defaults=(None, None, None))
Bounds3 = namedtuple("Bounds3", ["p_min", "p_max"])
RayHit = namedtuple("RayHit", ["hit", "point", "metadata"])  # src/kernels.jl:1-5
Ray = namedtuple("Ray", ["o", "d", "t_min", "t_max"], defaults=(0.0, np.inf))  # src/ray.jl:1-7 (time unused on the path)

EMPTY_TRIANGLE = Triangle(np.zeros((3, 3), np.float32), np.uint32(0), np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32),
                          np.zeros((3, 2), np.float32))  # empty_triangle, src/triangle_mesh.jl:49-57


def _triangle(rec):
    return Triangle(rec["vertices"].copy(), rec["metadata"], rec["normals"].copy(), rec["tangents"].copy(), rec["uv"].copy())


def mat4_to_mat3x4(m):
    """mat4_to_mat3x4 (src/instanced-bvh.jl:1663-1669): upper three rows of the 4x4, row-major."""
    m = np.asarray(m, dtype=np.float32)
    if m.shape == (4, 4):
        return np.ascontiguousarray(m[:3, :].reshape(12))
    if m.size == 12:
        return np.ascontiguousarray(m.reshape(12))
    raise ValueError("transform must be 4x4 or 12 floats (Mat3x4f)")


def _as_xforms(transforms):
    if transforms is None:
        return None
    t = np.asarray(transforms, dtype=np.float32)
    if t.ndim == 2 and t.shape == (4, 4):
        t = t[None]
    if t.ndim == 3 and t.shape[1:] == (4, 4):
        return np.ascontiguousarray(t[:, :3, :].reshape(-1, 12))
    return np.ascontiguousarray(t.reshape(-1, 12))


def _as_rays(rays):
    if isinstance(rays, np.ndarray) and rays.dtype == RAY_DT:
        return np.ascontiguousarray(rays)
    if isinstance(rays, Ray):
        rays = [rays]
    out = np.zeros(len(rays), dtype=RAY_DT)
    for i, r in enumerate(rays):
        out[i] = (tuple(r.o), r.t_min, tuple(r.d), r.t_max)
    return out


class StaticTLAS:
    """The adapted form (StaticTLAS, src/instanced-bvh.jl:155-168): what kernels traverse.  Returned by
    TLAS.adapt(); arrays are read back lazily in the reference's layout."""

    def __init__(self, owner):
        self._owner = owner

    def _export(self, fn, dt):
        n = C.c_uint32()
        check(fn(self._owner._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=dt)
        if n.value:
            check(fn(self._owner._h, ptr(out), n.value, None))
        return out

    @property
    def nodes(self):
        return self._export(lib().rc_export_tlas_nodes, _capi.NODE_DT)

    @property
    def instances(self):
        return self._export(lib().rc_export_instances, _capi.INSTANCE_DT)

    @property
    def all_blas_nodes(self):
        return self._export(lib().rc_export_blas_nodes, _capi.NODE_DT)

    @property
    def all_blas_prims(self):
        return self._export(lib().rc_export_prims, _capi.PRIM_DT)

    @property
    def all_blas_triangles(self):
        """all_blas_prims as full 136-byte Triangle{UInt32} records (vertices, normals, tangents, uv, metadata)."""
        return self._export(lib().rc_export_triangles, _capi.TRIANGLE_DT)

    @property
    def blas_descriptors(self):
        return self._export(lib().rc_export_blas_descs, _capi.DESC_DT)

    @property
    def root_aabb(self):
        return self._owner.world_bound()


class TLAS:
    """Mutable two-level accel (TLAS{Backend}, src/instanced-bvh.jl:261-310) on one MI355X."""

    def __init__(self, device=0):  # TLAS(backend), :334-358
        h = C.c_void_p()
        check(lib().rc_scene_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        self._static = StaticTLAS(self)
        self._prims_cache = None
        # Triangle{TMeta} for any TMeta (src/triangle_mesh.jl:1-7): the library keeps one uint32 per primitive; metadata that is not a
        # 32-bit unsigned integer is interned here and the word holds its 1-based index (`intern_metadata`, `typed_metadata`).
        self._meta_table = None
        self.meta_type = np.uint32

    # -- lifetime -------------------------------------------------------------------------------------
    def save(self, path):
        """Write the synced scene to a file (geometry BVHs, attributes, instances, handles); see rc_scene_save."""
        self.sync()
        check(lib().rc_scene_save(self._h, str(path).encode()))

    @classmethod
    def load(cls, path, device=0):
        """Read a scene file written by save(); handles keep their ids."""
        t = cls.__new__(cls)
        h = C.c_void_p()
        check(lib().rc_scene_load(int(device), str(path).encode(), C.byref(h)))
        t._h, t.device, t._static, t._prims_cache = h, device, StaticTLAS(t), None
        return t

    def free(self):  # free!, :383-399
        if getattr(self, "_h", None):
            for a in list(getattr(self, "_registered", {}).values()):  # arrays still pinned through host_register
                lib().rc_host_unregister(self._h, ptr(a))
            self._registered = {}
            lib().rc_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    # -- mutation -------------------------------------------------------------------------------------
    def push(self, verts, transforms=None, instance_id=0, instance_ids=None, meta=None):
        """push!(tlas, mesh, transform; instance_id) / push!(tlas, mesh, transforms; instance_ids) (:639-676)."""
        verts = np.ascontiguousarray(np.asarray(verts, dtype=np.float32).reshape(-1, 9))
        m = None if meta is None else np.ascontiguousarray(meta, dtype=np.uint32)
        if m is not None and len(m) != len(verts):
            raise ValueError("meta length != triangle count")
        xf = _as_xforms(transforms)
        n_inst = 1 if xf is None else len(xf)
        if instance_ids is not None:
            ids = np.ascontiguousarray(instance_ids, dtype=np.uint32)
            if len(ids) != n_inst:  # ArgumentError, :664-666
                raise ValueError(f"instance_ids length {len(ids)} != transforms length {n_inst}")
        else:
            ids = np.full(n_inst, instance_id, dtype=np.uint32)
        blas_id, handle = C.c_uint32(), C.c_uint32()
        check(lib().rc_add_blas(self._h, ptr(verts), ptr(m), len(verts), C.byref(blas_id)))
        check(lib().rc_add_instances(self._h, blas_id.value, ptr(xf), ptr(ids), n_inst, C.byref(handle)))
        self._prims_cache = None
        return TLASHandle(handle.value)

    def push_instances(self, blas_index, transforms=None, instance_ids=None, inv_transforms=None):
        """More instances of an existing geometry (1-based blas_index, as InstanceDescriptor stores it, :90-96)."""
        xf, inv = _as_xforms(transforms), _as_xforms(inv_transforms)
        n_inst = 1 if xf is None else len(xf)
        ids = np.zeros(n_inst, np.uint32) if instance_ids is None else np.ascontiguousarray(instance_ids, dtype=np.uint32)
        handle = C.c_uint32()
        check(lib().rc_add_instances_with_inverse(self._h, int(blas_index) - 1, ptr(xf), ptr(inv), ptr(ids), n_inst, C.byref(handle)))
        return TLASHandle(handle.value)

    def add_geometry(self, verts, meta=None):
        """build_and_append_blas! alone (:581-608); returns the 1-based BLAS index."""
        verts = np.ascontiguousarray(np.asarray(verts, dtype=np.float32).reshape(-1, 9))
        m = None if meta is None else np.ascontiguousarray(meta, dtype=np.uint32)
        blas_id = C.c_uint32()
        check(lib().rc_add_blas(self._h, ptr(verts), ptr(m), len(verts), C.byref(blas_id)))
        self._prims_cache = None
        return blas_id.value + 1

    def add_mesh(self, verts, faces, normals, uvs=None, face_meta=None, metadata_per_face=None):
        """build_and_append_blas! on a decomposed mesh (:581-608): verts / normals (nv, 3), faces (nf, 3) 0-based, uvs (nv, 2) or
        None, face_meta per vertex (as after expand_faceviews, :595) or None.  `metadata_per_face` (nf words) is the
        TLAS(items, metadata_fn) convention instead -- metadata_fn(mesh_idx, face_idx) for every face (:2300-2306) -- which a per-vertex
        array cannot carry when faces share their first vertex (the two triangles of a quad).  Returns the 1-based BLAS index."""
        v = np.ascontiguousarray(np.asarray(verts, dtype=np.float32).reshape(-1, 3))
        nrm = np.ascontiguousarray(np.asarray(normals, dtype=np.float32).reshape(-1, 3))
        f = np.ascontiguousarray(np.asarray(faces, dtype=np.uint32).reshape(-1, 3))
        uv = None if uvs is None else np.ascontiguousarray(np.asarray(uvs, dtype=np.float32).reshape(-1, 2))
        fm = None if face_meta is None else np.ascontiguousarray(face_meta, dtype=np.uint32)
        if len(nrm) != len(v) or (uv is not None and len(uv) != len(v)) or (fm is not None and len(fm) != len(v)):
            raise ValueError("normals / uvs / face_meta must have one entry per vertex")
        blas_id = C.c_uint32()
        if metadata_per_face is not None:
            if fm is not None:
                raise ValueError("face_meta (per vertex) and metadata_per_face (per face) are alternatives")
            pf = np.ascontiguousarray(metadata_per_face, dtype=np.uint32)
            if len(pf) != len(f):
                raise ValueError("metadata_per_face must have one entry per face")
            check(lib().rc_add_mesh_face_metadata(self._h, ptr(v), ptr(nrm), ptr(uv), len(v), ptr(f), len(f), ptr(pf), C.byref(blas_id)))
        else:
            check(lib().rc_add_mesh(self._h, ptr(v), ptr(nrm), ptr(uv), len(v), ptr(f), len(f), ptr(fm), C.byref(blas_id)))
        self._prims_cache = None
        return blas_id.value + 1

    def update_mesh(self, handle, verts, faces, normals, uvs=None, face_meta=None):
        """update!(tlas, handle, new_mesh) (:808-857) for a decomposed mesh."""
        v = np.ascontiguousarray(np.asarray(verts, dtype=np.float32).reshape(-1, 3))
        nrm = np.ascontiguousarray(np.asarray(normals, dtype=np.float32).reshape(-1, 3))
        f = np.ascontiguousarray(np.asarray(faces, dtype=np.uint32).reshape(-1, 3))
        uv = None if uvs is None else np.ascontiguousarray(np.asarray(uvs, dtype=np.float32).reshape(-1, 2))
        fm = None if face_meta is None else np.ascontiguousarray(face_meta, dtype=np.uint32)
        if len(nrm) != len(v) or (uv is not None and len(uv) != len(v)) or (fm is not None and len(fm) != len(v)):
            raise ValueError("normals / uvs / face_meta must have one entry per vertex")
        check(lib().rc_update_geometry_mesh(self._h, handle.id, ptr(v), ptr(nrm), ptr(uv), len(v), ptr(f), len(f), ptr(fm)))
        self._prims_cache = None
        return handle

    def push_mesh(self, verts, faces, normals, transforms=None, uvs=None, face_meta=None, instance_id=0, instance_ids=None):
        """push!(tlas, mesh, transforms; instance_ids) (:639-676) for a decomposed mesh; returns the TLASHandle."""
        blas_index = self.add_mesh(verts, faces, normals, uvs, face_meta)
        if instance_ids is None and transforms is not None:
            n_inst = len(_as_xforms(transforms))
            instance_ids = np.full(n_inst, instance_id, np.uint32)
        elif instance_ids is None:
            instance_ids = np.array([instance_id], np.uint32)
        return self.push_instances(blas_index, transforms, instance_ids)

    def primary_rays_lookat_device(self, camera_pos, right, up, forward, half_width, half_height, width, height, d_rays, samples=1, seed=0,
                                   jitter=True, stream=None):
        """generate_primary_rays_lookat! (docs/src/wavefront-renderer.jl:219-254) into a device RTRay buffer of width*height*samples."""
        v = [np.ascontiguousarray(a, dtype=np.float32) for a in (camera_pos, right, up, forward)]
        check(lib().rc_primary_rays_lookat_device(self._h, ptr(v[0]), ptr(v[1]), ptr(v[2]), ptr(v[3]), float(half_width), float(half_height),
                                                  int(width), int(height), int(samples), int(seed), 1 if jitter else 0, ptr(d_rays), ptr(stream)))

    def reflection_rays_device(self, d_rays, d_hits, n, d_out, bias=0.01, stream=None):
        """Mirror-reflection rays from hits (generate_reflection_rays! with roughness 0; reflect, src/math.jl:80)."""
        check(lib().rc_reflection_rays_device(self._h, ptr(d_rays), ptr(d_hits), int(n), float(bias), ptr(d_out), ptr(stream)))

    def compact_hits_device(self, d_hits, n, d_indices, d_count, stream=None):
        """Ascending indices of the hit rays + their count (device u32): queue compaction between wavefront stages."""
        check(lib().rc_compact_hits_device(self._h, ptr(d_hits), int(n), ptr(d_indices), ptr(d_count), ptr(stream)))

    def bounce_rays_device(self, d_rays, d_hits, n_out, d_out, seed=0, bounce=0, bias=1e-3, d_src=None, d_src_count=None, wrap=False,
                           d_path_in=None, d_path_out=None, path_base=0, stream=None):
        """Diffuse (cosine-weighted) bounce rays into n_out device RTRay slots (rc_bounce_rays_device): slot-aligned, or gathered through
        d_src / d_src_count (a device u32 count, e.g. compact_hits_device's; wrap=True reuses the sources round robin).  Dead slots get
        t_max = -1; d_path_out receives each slot's path id (RC_INVALID_ID when dead)."""
        check(lib().rc_bounce_rays_device(self._h, ptr(d_rays), ptr(d_hits), ptr(d_src) if d_src else None,
                                          ptr(d_src_count) if d_src_count else None, 1 if wrap else 0, ptr(d_path_in) if d_path_in else None,
                                          ptr(d_path_out) if d_path_out else None, int(path_base), int(n_out), int(seed), int(bounce), float(bias),
                                          ptr(d_out), ptr(stream) if stream else None))

    def shading_attributes_device(self, d_hits, n, d_normals=None, d_uvs=None, stream=None):
        """Interpolated shading normal / uv per hit on device buffers (docs/src/wavefront-renderer.jl:382-387)."""
        check(lib().rc_shading_attributes_device(self._h, ptr(d_hits), int(n), ptr(d_normals), ptr(d_uvs), ptr(stream)))

    def add_geometry_device(self, d_verts, n, d_meta=None):
        """build_and_append_blas! from device-resident soup (d_verts: device pointer to n x 9 f32); returns the 1-based BLAS index."""
        blas_id = C.c_uint32()
        check(lib().rc_add_blas_device(self._h, ptr(d_verts), ptr(d_meta) if d_meta else None, int(n), C.byref(blas_id)))
        self._prims_cache = None
        return blas_id.value + 1

    def delete(self, handle):  # delete!, :690-699
        d = C.c_int()
        check(lib().rc_delete(self._h, handle.id, C.byref(d)))
        self._prims_cache = None
        return bool(d.value)

    def update_transform(self, handle, transform):  # update_transform!, :755-770
        n = self.n_instances(handle) if self.is_valid(handle) else None
        if n is not None and n != 1:
            raise RaycoreError(_capi.RC_ERR_INVALID_ARGUMENT, f"Handle has {n} instances, use update_transforms! for multiple")
        xf = _as_xforms(transform)
        check(lib().rc_update_transforms(self._h, handle.id, ptr(xf), 1))

    def update_transforms(self, handle, transforms):  # update_transforms!, :784-797
        xf = _as_xforms(transforms)
        check(lib().rc_update_transforms(self._h, handle.id, ptr(xf), len(xf)))

    def update(self, handle, verts, meta=None):  # update!, :808-857
        verts = np.ascontiguousarray(np.asarray(verts, dtype=np.float32).reshape(-1, 9))
        m = None if meta is None else np.ascontiguousarray(meta, dtype=np.uint32)
        check(lib().rc_update_geometry(self._h, handle.id, ptr(verts), ptr(m), len(verts)))
        self._prims_cache = None

    def instance_buffer(self, handle):
        """instance_buffer(tlas, handle) (src/Raycore.jl:117-128): (device address, count) of the handle's 108-byte InstanceDescriptor
        records in the synced scene; rewrite them with your own kernels, then call refit_device()."""
        self.sync()
        p, n = C.c_void_p(), C.c_uint32()
        check(lib().rc_instance_buffer_device(self._h, handle.id, C.byref(p), C.byref(n)))
        return p.value, n.value

    def refit_device(self, recompute_inverse=True):
        """refit_tlas!(tlas) on descriptors rewritten in device memory: no host round trip."""
        check(lib().rc_refit_device(self._h, 1 if recompute_inverse else 0))
        return self

    def update_transforms_device(self, handle, d_xforms, stream=None):
        """update_transforms!(tlas, handle, transforms) for transforms that live in device memory (rc_update_transforms_device): a
        contiguous float32 torch tensor of shape (m, 12) or (m, 3, 4) on the scene's device, or a raw device pointer to m x 12 floats
        (m = the handle's instance count).  Enqueued on `stream` (a raw stream handle; None = the null stream); the tensor is read when
        the kernel runs.  Follow with refit_device_async() on the same stream, or sync()."""
        if hasattr(d_xforms, "data_ptr"):
            t = d_xforms
            if str(t.dtype) != "torch.float32" or not t.is_contiguous() or not t.is_cuda or t.device.index != self.device:
                raise RaycoreError(_capi.RC_ERR_INVALID_ARGUMENT, "transforms tensor must be contiguous float32 on the scene's device")
            if not (t.dim() >= 2 and (tuple(t.shape[1:]) == (12,) or tuple(t.shape[1:]) == (3, 4))):
                raise RaycoreError(_capi.RC_ERR_INVALID_ARGUMENT, f"transforms tensor must have shape (m, 12) or (m, 3, 4), got {tuple(t.shape)}")
            m, p = int(t.shape[0]), t.data_ptr()
        else:
            m, p = self.n_instances(handle), d_xforms
        check(lib().rc_update_transforms_device(self._h, handle.id, ptr(p) if p else None, m, ptr(stream) if stream else None))
        return self

    def refit_device_async(self, stream=None):
        """refit_tlas!(tlas) enqueued on `stream` with no host wait (rc_refit_device_async): later work on the same stream sees the new
        scene, and so do the host-buffer queries (trace(), get_illumination(), ...), which wait for it on the host; *_device queries on
        OTHER streams are the caller's to order.  world_bound() and the drivers that need it read it back lazily."""
        check(lib().rc_refit_device_async(self._h, ptr(stream) if stream else None))
        return self

    def rebuild_device_async(self, stream=None):
        """rebuild_bvh!(tlas) from the instances' current device-side transforms, enqueued on `stream` with no host wait
        (rc_rebuild_tlas_device_async): refit_device_async() with the topology built anew, so the scene traces exactly like a fresh one
        synced with these transforms.  In place: graphs that captured updates, refits or traces of this scene stay valid.  Option
        "tlas_rebuild_fused" (default 1) picks the single-workgroup kernel for scenes of 2 .. 256 instances."""
        check(lib().rc_rebuild_tlas_device_async(self._h, ptr(stream) if stream else None))
        return self

    def tlas_cost_device(self, out, stream=None):
        """The cost of the TLAS as it is when the kernels run on `stream` (rc_tlas_cost_device): the summed surface area of the internal
        nodes' boxes relative to the root's, one float64 written to `out` -- a float64 CUDA tensor of one element on the scene's device,
        or a raw device pointer.  Deterministic (no floating-point atomics); no host wait; capturable once run eagerly."""
        p = out
        if hasattr(out, "data_ptr"):
            if str(out.dtype) != "torch.float64" or out.numel() != 1 or not out.is_cuda or out.device.index != self.device:
                raise RaycoreError(_capi.RC_ERR_INVALID_ARGUMENT, "out must be a float64 tensor of one element on the scene's device")
            p = out.data_ptr()
        check(lib().rc_tlas_cost_device(self._h, ptr(p) if p else None, ptr(stream) if stream else None))
        return self

    def refit_or_rebuild_device_async(self, ratio, stream=None):
        """refit_device_async(), then rebuild_device_async() if the refitted tree costs more than `ratio` x what it cost when it was last
        built -- measured and decided on the device (rc_refit_or_rebuild_tlas_device_async), so one captured frame refits while instances
        drift and rebuilds on the replay in which they scatter.  The first call after a structural sync() arms the state (refit,
        unconditional rebuild, baseline cost) and must run eagerly.  tlas_quality() reads the decision back."""
        ratio = float(ratio)
        if not (np.isfinite(ratio) and ratio > 0.0):
            raise RaycoreError(_capi.RC_ERR_INVALID_ARGUMENT, f"ratio must be finite and > 0, got {ratio}")
        check(lib().rc_refit_or_rebuild_tlas_device_async(self._h, ratio, ptr(stream) if stream else None))
        return self

    def tlas_quality(self):
        """rc_tlas_quality: dict(cost, cost_built, evaluations, rebuilds, last_rebuilt, armed) of refit_or_rebuild_device_async.  A
        host-side read: waits for eager asynchronous work; replays of a graph that captured the call are the caller's to wait for."""
        q = _capi.TlasQualityInfo()
        check(lib().rc_tlas_quality(self._h, C.byref(q)))
        return {"cost": q.cost, "cost_built": q.cost_built, "evaluations": int(q.evaluations), "rebuilds": int(q.rebuilds),
                "last_rebuilt": bool(q.last_rebuilt), "armed": bool(q.armed)}

    def _device_f32(self, t, what, inner):
        """(rows, address) of a contiguous float32 torch tensor on the scene's device whose trailing shape multiplies to `inner`."""
        if str(t.dtype) != "torch.float32" or not t.is_contiguous() or not t.is_cuda or t.device.index != self.device:
            raise RaycoreError(_capi.RC_ERR_INVALID_ARGUMENT, f"{what} tensor must be contiguous float32 on the scene's device")
        if t.dim() < 2 or int(np.prod(t.shape[1:])) != inner:
            raise RaycoreError(_capi.RC_ERR_INVALID_ARGUMENT, f"{what} tensor must have {inner} floats per row, got shape {tuple(t.shape)}")
        return int(t.shape[0]), t.data_ptr()

    def update_geometry_device_async(self, handle, d_verts, n=None, d_meta=None, stream=None):
        """update!(tlas, handle, new_geometry) for a soup that lives in device memory (rc_update_geometry_device_async): a contiguous
        float32 torch tensor of shape (n, 9) or (n, 3, 3) on the scene's device, or a raw device pointer with `n`; d_meta an int32 /
        uint32 tensor of n words (or a raw pointer), None = face index 1..n.  The BLAS is rebuilt on `stream` and committed in place when
        the soup has as many non-degenerate faces as the BLAS has primitives; otherwise nothing changes and the next wait_for_gpu() raises
        RaycoreError with code RC_ERR_GEOMETRY_CHANGED.  The tensors are read when the kernels run.  Follow with refit_device_async() or
        rebuild_device_async() on the same stream, or sync()."""
        if hasattr(d_verts, "data_ptr"):
            rows, p = self._device_f32(d_verts, "soup", 9)
            n = rows if n is None else int(n)
            if n > rows:
                raise RaycoreError(_capi.RC_ERR_INVALID_ARGUMENT, f"n = {n} exceeds the soup tensor's {rows} faces")
        else:
            if n is None:
                raise RaycoreError(_capi.RC_ERR_INVALID_ARGUMENT, "n is required with a raw device pointer")
            n, p = int(n), d_verts
        pm = d_meta
        if hasattr(d_meta, "data_ptr"):
            if str(d_meta.dtype) not in ("torch.int32", "torch.uint32") or not d_meta.is_contiguous() or not d_meta.is_cuda or d_meta.device.index != self.device or d_meta.numel() < n:
                raise RaycoreError(_capi.RC_ERR_INVALID_ARGUMENT, "metadata tensor must be contiguous int32 / uint32 on the scene's device, one word per face")
            pm = d_meta.data_ptr()
        check(lib().rc_update_geometry_device_async(self._h, handle.id, ptr(p) if p else None, ptr(pm) if pm else None, n, ptr(stream) if stream else None))
        self._prims_cache = None
        return self

    def update_mesh_vertices_device_async(self, handle, d_verts, d_normals=None, stream=None):
        """The same for a geometry added through add_mesh (rc_update_mesh_vertices_device_async): new vertex positions, float32 (nv, 3)
        on the scene's device, and optionally new normals of the same shape (None keeps the stored ones).  Indices, uvs and metadata stay."""
        nv, p = self._device_f32(d_verts, "vertex", 3)
        pn = None
        if d_normals is not None:
            nn, pn = self._device_f32(d_normals, "normal", 3)
            if nn != nv:
                raise RaycoreError(_capi.RC_ERR_INVALID_ARGUMENT, f"{nn} normals for {nv} vertices")
        check(lib().rc_update_mesh_vertices_device_async(self._h, handle.id, ptr(p), ptr(pn) if pn else None, nv, ptr(stream) if stream else None))
        self._prims_cache = None
        return self

    def sync(self):  # sync!, :894-921
        a = C.c_int()
        check(lib().rc_sync(self._h, C.byref(a)))
        self.last_sync_action = ("noop", "refit", "rebuild")[a.value]
        if a.value == 2:
            self._prims_cache = None
        return self

    def adapt(self):  # Adapt.adapt(backend, tlas), :1085-1102: sync, then hand out the adapted form
        self.sync()
        return self._static

    @property
    def static_tlas(self):
        return self._static

    # -- queries ----------------------------------------------------------------------------------------
    def is_valid(self, handle):  # :524-526
        v = C.c_int()
        check(lib().rc_is_valid(self._h, handle.id, C.byref(v)))
        return bool(v.value)

    def _counts(self):
        c = [C.c_uint32() for _ in range(6)]
        check(lib().rc_counts(self._h, *[C.byref(x) for x in c]))
        return [x.value for x in c]

    def n_instances(self, handle=None):  # :533-537, :2391-2398
        if handle is None:
            return self._counts()[0]
        n = C.c_uint32()
        check(lib().rc_handle_instance_count(self._h, handle.id, C.byref(n)))
        return n.value

    def n_total_instances(self):  # :544
        return self._counts()[1]

    def n_geometries(self):  # :2405
        return self._counts()[2]

    def n_primitives(self):
        return self._counts()[3]

    def get_instances(self, handle):  # :732-738
        n = C.c_uint32()
        check(lib().rc_get_instances(self._h, handle.id, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=_capi.INSTANCE_DT)
        check(lib().rc_get_instances(self._h, handle.id, ptr(out), n.value, None))
        return out

    def get_instance(self, handle, instance_idx=1):  # :714-723
        inst = self.get_instances(handle)
        if not 1 <= instance_idx <= len(inst):
            raise RaycoreError(_capi.RC_ERR_INVALID_ARGUMENT, f"Instance index {instance_idx} out of range 1:{len(inst)}")
        return inst[instance_idx - 1]

    def world_bound(self):  # :2147-2149
        out = np.zeros(6, dtype=np.float32)
        check(lib().rc_world_bound(self._h, ptr(out)))
        return Bounds3(out[:3].copy(), out[3:].copy())

    def wait_for_gpu(self):  # wait_for_gpu!, :2418-2421
        check(lib().rc_wait(self._h))
        return self

    # -- batch tracing (device kernels) -------------------------------------------------------------------
    def set_option(self, name, value):
        check(lib().rc_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name):
        v = C.c_int64()
        check(lib().rc_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    def trace(self, rays, mode="closest", out=None):
        """Batch closest_hit / any_hit: RAY_DT array in, HIT_DT array out (RTRay/RTHitResult, src/rt_transport.jl).  `out` reuses a
        HIT_DT array of the same length (a render loop saves the page faults of a fresh 32 B/ray array on every call)."""
        rays = _as_rays(rays)
        if out is None:
            hits = np.empty(len(rays), dtype=HIT_DT)  # every record is written by the library
        else:
            if out.dtype != HIT_DT or len(out) != len(rays) or not out.flags["C_CONTIGUOUS"]:
                raise ValueError("out must be a contiguous HIT_DT array with one record per ray")
            hits = out
        fn = lib().rc_trace_closest if mode == "closest" else lib().rc_trace_any
        check(fn(self._h, ptr(rays), ptr(hits), len(rays)))
        return hits

    def trace_device(self, d_rays, d_hits, n, mode="closest", stream=None):
        """Device-pointer form (e.g. torch tensors' data_ptr()); asynchronous on `stream`."""
        fn = lib().rc_trace_closest_device if mode == "closest" else lib().rc_trace_any_device
        check(fn(self._h, ptr(d_rays), ptr(d_hits), int(n), ptr(stream) if stream else None))

    def trace_device_batches(self, d_rays, d_hits, n, mode="closest", stream=None):
        """Several INDEPENDENT device batches in one call (rc_trace_*_device_batches): sequences of device pointers and ray counts.  The
        batches overlap on the scene's auxiliary streams, forked from and joined back into `stream`; asynchronous like trace_device."""
        k = len(n)
        if len(d_rays) != k or len(d_hits) != k:
            raise ValueError("d_rays, d_hits and n must have one entry per batch")
        rp = (C.c_void_p * k)(*[int(x) for x in d_rays])
        hp = (C.c_void_p * k)(*[int(x) for x in d_hits])
        nn = (C.c_uint64 * k)(*[int(x) for x in n])
        fn = lib().rc_trace_closest_device_batches if mode == "closest" else lib().rc_trace_any_device_batches
        check(fn(self._h, rp, hp, nn, k, ptr(stream) if stream else None))

    def hit_points_device(self, d_rays, d_hits, n, d_points, d_normals=None, stream=None):
        check(lib().rc_hit_points_device(self._h, ptr(d_rays), ptr(d_hits), int(n), ptr(d_points), ptr(d_normals) if d_normals else None,
                                         ptr(stream) if stream else None))

    def shadow_rays_device(self, d_rays, d_hits, n, light, d_shadow_rays, bias=0.01, stream=None):
        """generate_shadow_rays! for one point light (docs/src/wavefront-renderer.jl:288-333); output feeds trace_device(mode='any')."""
        lv = np.ascontiguousarray(light, dtype=np.float32)
        check(lib().rc_shadow_rays_device(self._h, ptr(d_rays), ptr(d_hits), int(n), ptr(lv), float(bias), ptr(d_shadow_rays),
                                          ptr(stream) if stream else None))

    def shadow_visibility_device(self, d_rays, d_hits, n, d_lights, n_lights, d_visible, bias=0.01, stream=None):
        """Shadow visibility of all hits x all lights in one traversal launch (rc_shadow_visibility_device; generate_shadow_rays! +
        test_shadow_rays!, docs/src/wavefront-renderer.jl:279-362).  d_lights: device pointer to n_lights x 3 f32 positions, read when the
        kernel runs; d_visible: device pointer to n * n_lights bytes, byte i * n_lights + l = hit i is lit by light l -- what
        shadow_rays_device + trace_device(mode='any') per light give, without their buffers, under the reference's gate: a shadow ray
        whose t_max is not > 0 (0 or NaN) is not visible."""
        check(lib().rc_shadow_visibility_device(self._h, ptr(d_rays), ptr(d_hits), int(n), ptr(d_lights), int(n_lights), float(bias),
                                                ptr(d_visible), ptr(stream) if stream else None))

    def soft_shadow_rays_device(self, d_rays, d_hits, n, d_lights, d_radii, n_lights, samples, d_shadow_rays, seed=0, depth=0, bias=0.01,
                                d_path_in=None, path_base=0, stream=None):
        """The soft-shadow rays of all hits x all lights x `samples` (rc_soft_shadow_rays_device; compute_light's sampled area light,
        docs/src/raytracing-core.jl:58-99): n * n_lights * samples RTRay slots, ray (i, l, s) at (i * n_lights + l) * samples + s, ready
        for trace_device(mode='any').  d_lights / d_radii: device pointers to n_lights x 3 and n_lights f32, read when the kernel runs."""
        check(lib().rc_soft_shadow_rays_device(self._h, ptr(d_rays), ptr(d_hits), int(n), ptr(d_lights), ptr(d_radii), int(n_lights), int(samples),
                                               int(seed), int(depth), ptr(d_path_in) if d_path_in else None, int(path_base), float(bias),
                                               ptr(d_shadow_rays), ptr(stream) if stream else None))

    def soft_shadow_visibility_device(self, d_rays, d_hits, n, d_lights, d_radii, n_lights, samples, d_count, seed=0, depth=0, bias=0.01,
                                      d_path_in=None, path_base=0, stream=None):
        """Soft shadows in one traversal launch (rc_soft_shadow_visibility_device): d_count (device pointer, n * n_lights u32) is
        ACCUMULATED -- count[i * n_lights + l] += the samples of light l that hit i sees, exactly what soft_shadow_rays_device +
        trace_device(mode='any') + the t_max > 0 gate give, without their buffers.  The caller zeroes d_count and divides by `samples`
        (the reference's shadow_factor).  samples == 1 is shadow_visibility_device's byte."""
        check(lib().rc_soft_shadow_visibility_device(self._h, ptr(d_rays), ptr(d_hits), int(n), ptr(d_lights), ptr(d_radii), int(n_lights),
                                                     int(samples), int(seed), int(depth), ptr(d_path_in) if d_path_in else None, int(path_base),
                                                     float(bias), ptr(d_count), ptr(stream) if stream else None))

    def ambient_occlusion_rays_device(self, d_rays, d_hits, n, samples, d_ao_rays, max_dist=float("inf"), seed=0, depth=0, bias=1e-3,
                                      d_path_in=None, path_base=0, stream=None):
        """The ambient-occlusion rays of all hits x `samples` (rc_ambient_occlusion_rays_device): n * samples RTRay slots, ray (i, s) at
        i * samples + s -- from hit point + normal * bias in a cosine-weighted direction about the normal, t_max = max_dist -- ready for
        trace_device(mode='any').  A sample depends on (seed, path, depth, s) only."""
        check(lib().rc_ambient_occlusion_rays_device(self._h, ptr(d_rays), ptr(d_hits), int(n), int(samples), float(max_dist), int(seed), int(depth),
                                                     ptr(d_path_in) if d_path_in else None, int(path_base), float(bias), ptr(d_ao_rays),
                                                     ptr(stream) if stream else None))

    def ambient_occlusion_device(self, d_rays, d_hits, n, samples, d_count, max_dist=float("inf"), seed=0, depth=0, bias=1e-3, d_path_in=None,
                                 path_base=0, stream=None):
        """Ambient occlusion in one traversal launch (rc_ambient_occlusion_device): d_count (device pointer, n u32) is ACCUMULATED --
        count[i] += the samples of hit i's hemisphere that reach max_dist unoccluded, exactly what ambient_occlusion_rays_device +
        trace_device(mode='any') + the t_max > 0 gate give, without their buffers.  The caller zeroes d_count and divides by `samples`:
        the cosine-weighted openness of the point, its sky-view factor with max_dist = inf."""
        check(lib().rc_ambient_occlusion_device(self._h, ptr(d_rays), ptr(d_hits), int(n), int(samples), float(max_dist), int(seed), int(depth),
                                                ptr(d_path_in) if d_path_in else None, int(path_base), float(bias), ptr(d_count),
                                                ptr(stream) if stream else None))

    def final_gather_device(self, d_rays, d_hits, n, samples, d_x, d_sum, d_open=None, miss_value=0, max_dist=float("inf"), seed=0, depth=0,
                            bias=1e-3, d_path_in=None, path_base=0, stream=None):
        """The final gather in one traversal launch (rc_final_gather_device): ambient_occlusion_device's samples traced for the CLOSEST hit.
        d_sum (device pointer, n u64) is ACCUMULATED -- sum[i] += x[meta - 1] of what each sample of hit i's hemisphere hits first
        (metadata outside 1..n_primitives: nothing), miss_value for a sample that reaches max_dist --, and d_open (n u32, may be None) with
        the samples that escape: ambient_occlusion_device's counts.  d_x: device pointer to n_primitives u32, read when the kernel runs.
        The caller zeroes the outputs; sum / samples is the cosine-weighted mean of x over the hemisphere."""
        check(lib().rc_final_gather_device(self._h, ptr(d_rays), ptr(d_hits), int(n), int(samples), float(max_dist), int(seed), int(depth),
                                           ptr(d_path_in) if d_path_in else None, int(path_base), float(bias), ptr(d_x), int(miss_value), ptr(d_sum),
                                           ptr(d_open) if d_open else None, ptr(stream) if stream else None))

    def illumination_dirs_device(self, d_dirs, n_dirs, grid, d_counts, row_stride=None, stream=None):
        """get_illumination for n_dirs directions in one call (rc_get_illumination_dirs_device).  d_dirs: device pointer to n_dirs x 3 f32
        (need not be normalised), read WHEN THE KERNELS RUN, like the TLAS root the grids are laid out from: no host copy of the world
        bound is involved, so the call follows refit_device_async / rebuild_device_async without a host wait and may be captured.
        d_counts: device pointer to n_dirs rows of `row_stride` (default: the primitive count) u32, ACCUMULATED:
        d_counts[d * row_stride + meta - 1] += the hits of direction d.  Weighting the rows is the caller's."""
        rs = self.n_primitives() if row_stride is None else int(row_stride)
        check(lib().rc_get_illumination_dirs_device(self._h, ptr(d_dirs), int(n_dirs), int(grid), ptr(d_counts), rs, ptr(stream) if stream else None))

    def point_source_rays_device(self, d_sources, n_sources, grid, d_rays, seed=0, first_source=0, stream=None):
        """The rays of n_sources device-resident point sources (rc_point_source_rays_device): n_sources x grid^2 RTRay records, source
        k's at k * grid^2 in cell order.  d_sources: device pointer to n_sources RTRay records (o = position, d = axis -- zero: isotropic,
        else Lambertian about it --, t_min / t_max copied into every ray), read when the kernel runs."""
        check(lib().rc_point_source_rays_device(self._h, ptr(d_sources), int(n_sources), int(grid), int(seed), int(first_source), ptr(d_rays),
                                                ptr(stream) if stream else None))

    def illumination_points_device(self, d_sources, n_sources, grid, d_counts, row_stride=None, d_escaped=None, seed=0, first_source=0, stream=None):
        """get_illumination for n_sources POINT sources in one call (rc_get_illumination_points_device): grid^2 stratified rays per
        source, the rays of point_source_rays_device bit for bit.  d_counts: device pointer to n_sources rows of `row_stride` (default:
        the primitive count) u32, ACCUMULATED: d_counts[k * row_stride + meta - 1] += the hits of source k; d_escaped (n_sources u32, may
        be None) += the rays of source k that hit nothing.  d_sources is read WHEN THE KERNEL RUNS: the call follows the asynchronous
        updates without a host wait, may be captured, and a replay follows lamps that moved.  first_source offsets the random-number
        counter only: sources [a, b) of a set with first_source = a give rows [a, b) of the one-call result."""
        rs = self.n_primitives() if row_stride is None else int(row_stride)
        check(lib().rc_get_illumination_points_device(self._h, ptr(d_sources), int(n_sources), int(grid), int(seed), int(first_source), ptr(d_counts), rs,
                                                      ptr(d_escaped) if d_escaped else None, ptr(stream) if stream else None))

    def view_factor_products_device(self, x_ptr, mx_ptr, mtx_ptr, rays_per_triangle, seed, src=None, rays=None, stream=None):
        """The view-factor matrix applied to a device vector without the matrix (rc_view_factor_products_device).  x_ptr: N u32 indexed
        by metadata - 1; mx_ptr / mtx_ptr: N u64 each (either may be None), ACCUMULATED: mx += M x, mtx += M^T x with M what
        view_factors(accel, rays_per_triangle, seed) returns, modulo 2^64.  src / rays: (begin, end) ranges of flat source primitives and
        of ray indices (default: all) -- the shards of one job add up to the whole, on one stream or on several."""
        s0, s1 = (0, 0xFFFFFFFF) if src is None else src
        r0, r1 = (0, int(rays_per_triangle)) if rays is None else rays
        check(lib().rc_view_factor_products_device(self._h, int(rays_per_triangle), int(seed), int(s0), int(s1), int(r0), int(r1), ptr(x_ptr),
                                                   ptr(mx_ptr) if mx_ptr else None, ptr(mtx_ptr) if mtx_ptr else None,
                                                   ptr(stream) if stream else None))

    def view_factor_sampled_rays_device(self, d_rays, src_prim, n_rays, seed=0, sampling="uniform", ray_begin=0, stream=None):
        """The sampled view-factor rays of one flat source primitive (rc_view_factor_sampled_rays_device): n_rays RTRay records for ray
        indices ray_begin.. .  sampling "uniform": the reference's rays, bit for bit view_factor_rays_device's; "cosine": the same
        origins with cosine-weighted directions about the triangle's normal -- the rays of form factors."""
        check(lib().rc_view_factor_sampled_rays_device(self._h, int(seed), vf_sampling(sampling), int(src_prim), int(ray_begin), int(n_rays), ptr(d_rays),
                                                       ptr(stream) if stream else None))

    def view_factor_groups_device(self, groups_ptr, n_groups, matrix_ptr, rays_per_triangle, seed, sampling="uniform", weights_ptr=None,
                                  escaped_ptr=None, src=None, rays=None, stream=None):
        """Weighted counts between GROUPS of primitives (rc_view_factor_groups_device).  groups_ptr / weights_ptr (may be None: weight 1):
        N u32 each, indexed by metadata - 1, read when the kernel runs; matrix_ptr: n_groups x n_groups u64, row = source group;
        escaped_ptr: n_groups u64 or None.  Both outputs are ACCUMULATED: a ray from metadata a (group ga, weight wa) that hits metadata
        b != a of group gb adds wa to matrix[ga, gb], one that hits nothing adds wa to escaped[ga]; a group >= n_groups excludes the
        primitive.  src / rays: (begin, end) ranges of flat source primitives and of ray indices (default: all) -- the shards of one
        job add up to the whole, on one stream or on several."""
        s0, s1 = (0, 0xFFFFFFFF) if src is None else src
        r0, r1 = (0, int(rays_per_triangle)) if rays is None else rays
        check(lib().rc_view_factor_groups_device(self._h, int(rays_per_triangle), int(seed), vf_sampling(sampling), int(s0), int(s1), int(r0), int(r1),
                                                 ptr(groups_ptr), int(n_groups), ptr(weights_ptr) if weights_ptr else None, ptr(matrix_ptr),
                                                 ptr(escaped_ptr) if escaped_ptr else None, ptr(stream) if stream else None))

    def placed_primitive_bases(self):
        """The placed-primitive table (rc_placed_primitive_bases): n_inst + 1 uint32, base[i] = the primitives of the instances before i in
        the instance array's order; base[-1] = P, the scene's placed-primitive count.  Placed primitive q = base[i] + l is primitive l
        (0-based, in the BLAS's sorted order) of instance i."""
        n = C.c_uint32(0)
        check(lib().rc_placed_primitive_bases(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint32)
        check(lib().rc_placed_primitive_bases(self._h, ptr(out), n.value, C.byref(n)))
        return out

    def placed_triangles_device(self, d_verts, placed_begin=0, n=None, stream=None):
        """The world triangles of placed primitives [placed_begin, placed_begin + n) (rc_placed_triangles_device; default: to the last): 9 f32
        each at d_verts, the local vertices under the instance's forward transform as it is in device memory when the kernel runs."""
        if n is None:
            n = int(self.placed_primitive_bases()[-1]) - int(placed_begin)
        check(lib().rc_placed_triangles_device(self._h, int(placed_begin), int(n), ptr(d_verts), ptr(stream) if stream else None))

    def placed_view_factor_rays_device(self, d_rays, placed_prim, n_rays, seed=0, sampling="uniform", ray_begin=0, stream=None):
        """The sampled view-factor rays of one PLACED primitive (rc_placed_view_factor_rays_device): view_factor_sampled_rays_device's ray
        of the world triangle, with the instance in the third word of the random-number counter."""
        check(lib().rc_placed_view_factor_rays_device(self._h, int(seed), vf_sampling(sampling), int(placed_prim), int(ray_begin), int(n_rays), ptr(d_rays),
                                                      ptr(stream) if stream else None))

    def placed_view_factor_groups_device(self, groups_ptr, n_groups, matrix_ptr, rays_per_triangle, seed, sampling="uniform", weights_ptr=None,
                                         escaped_ptr=None, placed=None, rays=None, stream=None):
        """Weighted counts between GROUPS of PLACED primitives (rc_placed_view_factor_groups_device): view_factor_groups_device with the
        sources in world space.  groups_ptr / weights_ptr (may be None: weight 1): P u32 each, indexed by placed primitive q, read when the
        kernel runs; matrix_ptr: n_groups x n_groups u64, row = source group; escaped_ptr: n_groups u64 or None.  Both outputs are
        ACCUMULATED: a ray from placed primitive a (group ga, weight wa) that hits placed primitive b != a of group gb adds wa to
        matrix[ga, gb], one that hits nothing adds wa to escaped[ga]; a group >= n_groups excludes the primitive.  placed / rays:
        (begin, end) ranges of placed primitives and of ray indices (default: all) -- the shards of one job add up to the whole."""
        s0, s1 = (0, 0xFFFFFFFF) if placed is None else placed
        r0, r1 = (0, int(rays_per_triangle)) if rays is None else rays
        check(lib().rc_placed_view_factor_groups_device(self._h, int(rays_per_triangle), int(seed), vf_sampling(sampling), int(s0), int(s1), int(r0), int(r1),
                                                        ptr(groups_ptr), int(n_groups), ptr(weights_ptr) if weights_ptr else None, ptr(matrix_ptr),
                                                        ptr(escaped_ptr) if escaped_ptr else None, ptr(stream) if stream else None))

    def placed_view_factor_products_device(self, x_ptr, mx_ptr, mtx_ptr, rays_per_triangle, seed, sampling="uniform", escaped_ptr=None, placed=None,
                                           rays=None, stream=None):
        """The matrix of counts between PLACED primitives applied to a device vector without the matrix
        (rc_placed_view_factor_products_device): view_factor_products_device with the sources in world space and a choice of sampling.
        x_ptr: P u32 indexed by placed primitive q, or None for x = 1 (the placed totals); mx_ptr / mtx_ptr / escaped_ptr: P u64 each (every
        one may be None), ACCUMULATED: a ray from placed primitive a that hits placed primitive b != a adds x[b] to mx[a] and x[a] to
        mtx[b], one that hits nothing adds 1 to escaped[a]; modulo 2^64.  No metadata takes part.  placed / rays: (begin, end) ranges of
        placed primitives and of ray indices (default: all) -- the shards of one job add up to the whole."""
        s0, s1 = (0, 0xFFFFFFFF) if placed is None else placed
        r0, r1 = (0, int(rays_per_triangle)) if rays is None else rays
        check(lib().rc_placed_view_factor_products_device(self._h, int(rays_per_triangle), int(seed), vf_sampling(sampling), int(s0), int(s1), int(r0), int(r1),
                                                          ptr(x_ptr) if x_ptr else None, ptr(mx_ptr) if mx_ptr else None, ptr(mtx_ptr) if mtx_ptr else None,
                                                          ptr(escaped_ptr) if escaped_ptr else None, ptr(stream) if stream else None))

    def view_factors_sparse_device(self, row_ptr_ptr, cols_ptr, vals_ptr, capacity, nnz_ptr, rays_per_triangle, seed, rows=None, stream=None):
        """Rows `rows` = (begin, end) (default: all; end is clamped to N) of the view-factor matrix in canonical CSR on the device
        (rc_view_factors_sparse_device), OVERWRITTEN: row_ptr_ptr: rows + 1 u64 starting at 0; cols_ptr / vals_ptr: `capacity` u32 each
        (None with capacity 0: the counting call); nnz_ptr: one u64.  nnz and row_ptr are always the true values, entries below
        `capacity` the correct first ones, nothing is written at or beyond it.  Everything runs on `stream`; not capturable."""
        r0, r1 = (0, 0xFFFFFFFF) if rows is None else rows
        check(lib().rc_view_factors_sparse_device(self._h, int(rays_per_triangle), int(seed), int(r0), int(r1), ptr(row_ptr_ptr),
                                                  ptr(cols_ptr) if cols_ptr else None, ptr(vals_ptr) if vals_ptr else None, int(capacity),
                                                  ptr(nnz_ptr), ptr(stream) if stream else None))

    def placed_view_factors_sparse_device(self, row_ptr_ptr, cols_ptr, vals_ptr, capacity, nnz_ptr, rays_per_triangle, seed, sampling="uniform",
                                          rows=None, stream=None):
        """Rows `rows` = (begin, end) (default: all; end is clamped to P) of the matrix of counts between PLACED primitives in canonical CSR
        on the device (rc_placed_view_factors_sparse_device), OVERWRITTEN: view_factors_sparse_device's arguments and capacity contract,
        with placed rows and columns and a choice of sampling.  The matrix is a SNAPSHOT of the placement at the time its kernels run.
        Everything runs on `stream`; not capturable.  The products are view_factor_sparse_products_device."""
        r0, r1 = (0, 0xFFFFFFFF) if rows is None else rows
        check(lib().rc_placed_view_factors_sparse_device(self._h, int(rays_per_triangle), int(seed), vf_sampling(sampling), int(r0), int(r1),
                                                         ptr(row_ptr_ptr), ptr(cols_ptr) if cols_ptr else None, ptr(vals_ptr) if vals_ptr else None,
                                                         int(capacity), ptr(nnz_ptr), ptr(stream) if stream else None))

    def placed_hit_indices_device(self, d_hits, n, d_q, stream=None):
        """The placed primitive each hit record names (rc_placed_hit_indices_device): d_q (device pointer, n u32) gets
        q = base[instance_id] + (primitive_id - the first flat primitive of the instance's BLAS) for a hit and RC_INVALID_ID (2^32 - 1)
        for a miss.  B[q] is then the placed solution's value on the surface the ray sees.  One stage kernel, capturable."""
        check(lib().rc_placed_hit_indices_device(self._h, ptr(d_hits), int(n), ptr(d_q), ptr(stream) if stream else None))

    def placed_final_gather_device(self, d_rays, d_hits, n, samples, d_x, d_sum, d_open=None, miss_value=0, max_dist=float("inf"), seed=0, depth=0,
                                   bias=1e-3, d_path_in=None, path_base=0, stream=None):
        """The final gather of a field per PLACED primitive in one traversal launch (rc_placed_final_gather_device): final_gather_device's
        items, rays and outputs, with d_x a device pointer to P u32 indexed by placed primitive q (placed_radiosity's result, say), read
        when the kernel runs.  d_sum (n u64) is ACCUMULATED -- sum[i] += x[base[instance] + l] of what each sample of hit i's hemisphere
        hits first, miss_value for a sample that reaches max_dist --, and d_open (n u32, may be None) with the samples that escape.  No
        metadata takes part: every hit is counted, and two instances of one mesh carry different values.  The caller zeroes the outputs."""
        check(lib().rc_placed_final_gather_device(self._h, ptr(d_rays), ptr(d_hits), int(n), int(samples), float(max_dist), int(seed), int(depth),
                                                  ptr(d_path_in) if d_path_in else None, int(path_base), float(bias), ptr(d_x), int(miss_value),
                                                  ptr(d_sum), ptr(d_open) if d_open else None, ptr(stream) if stream else None))

    def view_factor_sparse_products_device(self, n_rows, row_ptr_ptr, cols_ptr, vals_ptr, x_ptr, mx_ptr, mtx_ptr, row_offset=0, stream=None):
        """The products of a device CSR block with a device vector (rc_view_factor_sparse_products_device), ACCUMULATED modulo 2^64:
        mx[row_offset + r] += sum_k vals[k] x[cols[k]], mtx[cols[k]] += vals[k] x[row_offset + r]; mx_ptr / mtx_ptr: u64 vectors, either
        may be None.  Nothing is read on the host: capturable, and needs no wait behind the build.  The arrays are not validated."""
        check(lib().rc_view_factor_sparse_products_device(self._h, int(n_rows), int(row_offset), ptr(row_ptr_ptr), ptr(cols_ptr) if cols_ptr else None,
                                                          ptr(vals_ptr) if vals_ptr else None, ptr(x_ptr), ptr(mx_ptr) if mx_ptr else None,
                                                          ptr(mtx_ptr) if mtx_ptr else None, ptr(stream) if stream else None))

    def ray_grid_dirs_device(self, d_dirs, n_dirs, grid, d_rays, stream=None):
        """The ray grids of n_dirs device-resident directions (rc_generate_ray_grid_dirs_device): n_dirs x grid^2 RTRay records, direction
        d's at d * grid^2 in generate_ray_grid's layout, laid out on the device from the TLAS root as it is when the kernel runs."""
        check(lib().rc_generate_ray_grid_dirs_device(self._h, ptr(d_dirs), int(n_dirs), int(grid), ptr(d_rays), ptr(stream) if stream else None))

    def last_kernel_ms(self):
        ms = C.c_float()
        check(lib().rc_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def recent_kernel_ms(self, max_launches=47):
        """Durations (ms, oldest first) of the scene's most recent eager launches, from the events the launches carried themselves
        (rc_recent_kernel_ms): for timing a run of back-to-back launches without events between them."""
        out = (C.c_float * int(max_launches))()
        n = C.c_uint32(0)
        check(lib().rc_recent_kernel_ms(self._h, int(max_launches), out, C.byref(n)))
        return [float(out[i]) for i in range(n.value)]

    def host_register(self, array):
        """Page-lock a numpy array (rays, a reused `out=` hit array, triangle soup, a view-factor matrix) so the host-buffer calls move
        it by DMA at the full PCIe rate; undo with host_unregister.  The accel keeps a reference to the array while it is registered (an
        array collected while pinned would leave a stale pinned range behind); free() unregisters what is left."""
        check(lib().rc_host_register(self._h, ptr(array), array.nbytes))
        if not hasattr(self, "_registered"):
            self._registered = {}
        self._registered[array.ctypes.data] = array
        return array

    def host_unregister(self, array):
        check(lib().rc_host_unregister(self._h, ptr(array)))
        getattr(self, "_registered", {}).pop(array.ctypes.data, None)

    def intern_metadata(self, values):
        """Metadata words for `values`: the values themselves when they are all uint32-representable integers and the accel is still
        in uint32 mode (TMetadata = UInt32, the reference's default), otherwise 1-based indices into the accel's metadata table."""
        values = list(values)
        ints = all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and 0 <= int(v) <= 0xFFFFFFFF for v in values)
        if ints and self._meta_table is None:
            return np.array(values, dtype=np.uint32)
        if self._meta_table is None:
            if self.n_geometries() > 0:
                raise RaycoreError(_capi.RC_ERR_INVALID_ARGUMENT, "an accel's metadata type is fixed by its first geometry (Triangle{TMetadata})")
            self._meta_table = []
            self.meta_type = type(values[0]) if values else object
        base = len(self._meta_table)
        self._meta_table.extend(values)
        return np.arange(base + 1, base + 1 + len(values), dtype=np.uint32)

    def typed_metadata(self, word):
        """The metadata value a primitive's uint32 word stands for (identity in uint32 mode; 0 = the empty triangle's metadata)."""
        if self._meta_table is None:
            return word
        word = int(word)
        return self._meta_table[word - 1] if word >= 1 else None

    def eltype(self):  # Base.eltype(tlas), src/instanced-bvh.jl:2334-2345
        return ("Triangle", self.meta_type)

    def _prims(self):
        if self._prims_cache is None:
            self._prims_cache = self._static.all_blas_prims
        return self._prims_cache

    def _triangles(self):
        if self._prims_cache is None or getattr(self, "_tri_cache_for", None) is not self._prims_cache:
            self._tri_cache = self._static.all_blas_triangles
            self._tri_cache_for = self._prims()
        return self._tri_cache


def _owner(accel):
    if isinstance(accel, StaticTLAS):
        return accel._owner
    if isinstance(accel, TLAS):
        accel.sync()  # the reference requires adapt-per-dispatch; adapt == sync + read (:1085-1102)
        return accel
    raise TypeError("expected TLAS or StaticTLAS")


def sync(tlas):
    return tlas.sync()


def adapt(tlas):
    return tlas.adapt()


def world_bound(accel):
    return _owner(accel).world_bound() if isinstance(accel, StaticTLAS) else accel.world_bound()


def _tuple_from_hit(t, h, miss_prim):
    """(hit, Triangle, t, bary, instance_idx) exactly as closest_hit/any_hit return it (:2010-2023, :2106-2139)."""
    if not h["hit"]:
        return (False, miss_prim, np.float32(0), np.zeros(3, np.float32), np.uint32(0))
    u, v = h["bary_u"], h["bary_v"]
    w = (np.float32(1.0) - u) - v  # 1f0 - hit_u - hit_v (:2015)
    return (True, _typed(t, _triangle(t._triangles()[h["primitive_id"]])), h["t"], np.array([w, u, v], np.float32), np.uint32(h["instance_id"] + 1))


def _typed(t, tri):
    return tri if t._meta_table is None else tri._replace(metadata=t.typed_metadata(tri.metadata))


def closest_hit(accel, ray):
    """closest_hit(tlas, ray) -> (hit, primitive, distance, barycentric, instance_idx) (:1902-2024)."""
    t = _owner(accel)
    return _tuple_from_hit(t, t.trace(_as_rays(ray))[0], EMPTY_TRIANGLE)


def any_hit(accel, ray):
    """any_hit(tlas, ray) (:2034-2140); on a miss the dummy primitive is all_blas_prims[1] (:2137)."""
    t = _owner(accel)
    h = t.trace(_as_rays(ray), mode="any")[0]
    tris = t._triangles()
    dummy = _typed(t, _triangle(tris[0])) if len(tris) else EMPTY_TRIANGLE
    return _tuple_from_hit(t, h, dummy)


def trace_rays(accel, rays):
    """trace_rays(tlas, rays) = map(closest_hit) (ext/RaycoreMakieExt.jl:81-87), one device launch."""
    t = _owner(accel)
    return [_tuple_from_hit(t, h, EMPTY_TRIANGLE) for h in t.trace(_as_rays(rays))]


ContactPair = namedtuple("ContactPair", ["instance_a", "instance_b"])  # src/collision.jl:25-28 (1-based instance indices)
CollisionResult = namedtuple("CollisionResult", ["contacts", "num_contacts", "cache"])  # :40-44
CONTACT_DT = np.dtype([("instance_a", "<u4"), ("instance_b", "<u4")])


def collide_instances(tlas, cache=None):
    """collide_instances(tlas; cache) (src/collision.jl:189-233): all instance pairs with overlapping world AABBs, as a
    CONTACT_DT array (ContactPair bytes).  `cache` is accepted for signature parity; the library keeps its own buffer."""
    tlas.sync()
    n = C.c_uint64(0)
    check(lib().rc_collide_instances(tlas._h, None, 0, C.byref(n)))
    out = np.zeros(n.value, dtype=CONTACT_DT)
    if n.value:
        check(lib().rc_collide_instances(tlas._h, ptr(out), n.value, C.byref(n)))
    return CollisionResult(out, int(n.value), cache)


def collide_instances_any(tlas, handle_a, handle_b):
    """collide_instances_any(tlas, handle_a, handle_b) -> Bool (src/collision.jl:241-261)."""
    tlas.sync()
    ov = C.c_int(0)
    check(lib().rc_collide_instances_any(tlas._h, handle_a.id, handle_b.id, C.byref(ov)))
    return bool(ov.value)


class BLAS4:
    """BLAS4 (src/bvh4.jl:154-162): a 4-wide BVH over ONE geometry, traced in the geometry's own space (the reference has no
    instanced BVH4 path).  Built by build_blas4; owns a private scene holding the geometry's BVH2 and its collapse."""

    def __init__(self, scene, blas_id, n_nodes):
        self._scene, self._blas_id, self.num_interior = scene, blas_id, n_nodes  # num_interior = length(nodes4), :521
        self._prims_cache = None

    @property
    def nodes(self):
        out = np.zeros(self.num_interior, dtype=_capi.NODE4_DT)
        cnt = C.c_uint32(0)
        check(lib().rc_export_blas4_nodes(self._scene._h, self._blas_id, ptr(out), len(out), C.byref(cnt)))
        return out

    @property
    def primitives(self):
        if self._prims_cache is None:
            self._prims_cache = self._scene.adapt().all_blas_prims  # one geometry => its Morton-sorted primitives
        return self._prims_cache

    @property
    def root_aabb(self):
        d = self._scene.adapt().blas_descriptors[0]
        return Bounds3(d["root_min"].copy(), d["root_max"].copy())

    def trace(self, rays, mode="closest"):
        rays = _as_rays(rays)
        hits = np.zeros(len(rays), dtype=HIT_DT)
        fn = lib().rc_trace_closest4 if mode == "closest" else lib().rc_trace_any4
        check(fn(self._scene._h, self._blas_id, ptr(rays), ptr(hits), len(rays)))
        return hits

    def trace_device(self, d_rays, d_hits, n, mode="closest", stream=None):
        fn = lib().rc_trace_closest4_device if mode == "closest" else lib().rc_trace_any4_device
        check(fn(self._scene._h, self._blas_id, ptr(d_rays), ptr(d_hits), int(n), ptr(stream)))

    def last_kernel_ms(self):
        return self._scene.last_kernel_ms()


def build_blas4(verts, meta=None, device=0):
    """build_blas4(primitives) (src/bvh4.jl:511-522): LBVH (BVH2) build + collapse to BVH4, both on the device."""
    scene = TLAS(device)
    blas_index = scene.add_geometry(verts, meta)
    scene.push_instances(blas_index)  # identity instance: lets the private scene sync so primitives / root_aabb can be exported
    n = C.c_uint32(0)
    check(lib().rc_blas4_build(scene._h, blas_index - 1, C.byref(n)))
    return BLAS4(scene, blas_index - 1, n.value)


def _tuple4(blas, h, miss_prim):
    if not h["hit"]:
        return (False, miss_prim, np.float32(0), np.zeros(3, np.float32))
    p = blas.primitives[h["primitive_id"]]
    u, v = h["bary_u"], h["bary_v"]
    w = np.float32(1.0) - u - v  # :681
    return (True, Triangle(p["v"].copy(), p["meta"]), h["t"], np.array([w, u, v], np.float32))


def closest_hit4(blas, ray):
    """closest_hit4(blas::BLAS4, ray) -> (hit, primitive, distance, barycentric) (src/bvh4.jl:606-689)."""
    return _tuple4(blas, blas.trace(_as_rays(ray))[0], EMPTY_TRIANGLE)


def any_hit4(blas, ray):
    """any_hit4(blas::BLAS4, ray) (src/bvh4.jl:696-766); the miss dummy is primitives[1] (:763)."""
    p = blas.primitives[0]
    return _tuple4(blas, blas.trace(_as_rays(ray), mode="any")[0], Triangle(p["v"].copy(), p["meta"]))


def generate_ray_grid(accel, viewdir, grid_size):
    """generate_ray_grid as used by hits_from_grid (src/kernels.jl:10-72), computed on the device; returns RAY_DT rays."""
    import torch
    t = _owner(accel)
    n = grid_size * grid_size
    buf = torch.empty(n * 8, dtype=torch.float32, device=f"cuda:{t.device}")
    vd = np.ascontiguousarray(viewdir, dtype=np.float32)
    check(lib().rc_generate_ray_grid_device(t._h, ptr(vd), grid_size, ptr(buf.data_ptr()), None))
    torch.cuda.synchronize(t.device)
    return buf.cpu().numpy().view(RAY_DT).reshape(n)


RAYHIT_DT = np.dtype([("hit", "?"), ("point", "<f4", 3), ("metadata", "<u4")])  # RayHit{UInt32}, src/kernels.jl:1-5


def hits_from_grid(accel, viewdir, grid_size=32):
    """hits_from_grid (src/kernels.jl:58-72): a grid_size x grid_size array of RayHit records (RAYHIT_DT, indexed [i, j] like
    the Julia Matrix); point = sum_mul(bary, prim.vertices) in the primitive's local space, metadata = prim.metadata
    (a miss carries the zero triangle: point 0, metadata 0).  Always the one structured array: on an accel whose metadata type is
    not UInt32 the `metadata` field holds the interned words, and `typed_hit_metadata(accel, hits)` maps them to the values."""
    t = _owner(accel)
    rays = generate_ray_grid(t._static, viewdir, grid_size)
    hits = t.trace(rays)
    prims = t._prims()
    out = np.zeros(len(rays), dtype=RAYHIT_DT)
    m = hits["hit"] == 1
    out["hit"] = m
    if m.any():
        p = prims[hits["primitive_id"][m]]
        u, v = hits["bary_u"][m], hits["bary_v"][m]
        w = (np.float32(1) - u) - v
        # sum_mul (src/math.jl:52): a[1]*b[1] + a[2]*b[2] + a[3]*b[3], left to right, in Float32
        out["point"][m] = (w[:, None] * p["v"][:, 0] + u[:, None] * p["v"][:, 1]) + v[:, None] * p["v"][:, 2]
        out["metadata"][m] = p["meta"]
    return out.reshape(grid_size, grid_size, order="F")


def typed_hit_metadata(accel, hits):
    """RayHit{TMetadata}.metadata for an accel with a non-UInt32 metadata type: an object array shaped like `hits` holding the values
    the interned words stand for (None where the ray missed).  In UInt32 mode it is `hits["metadata"]` itself."""
    t = _owner(accel)
    if t._meta_table is None:
        return hits["metadata"]
    typed = np.empty(hits.shape, dtype=object)
    for idx in np.ndindex(hits.shape):
        typed[idx] = t.typed_metadata(hits["metadata"][idx]) if hits["hit"][idx] else None
    return typed


def get_centroid(accel, viewdir, grid_size=32):
    """get_centroid (src/kernels.jl:106-110): the hit points and their mean."""
    hits = hits_from_grid(accel, viewdir, grid_size)
    pts = hits["point"][hits["hit"]]
    return pts, (pts.mean(axis=0) if len(pts) else np.full(3, np.nan, np.float32))


def get_illumination(accel, viewdir, grid_size=1000):
    """get_illumination (src/kernels.jl:112-124): per-primitive hit counts of a grid_size^2 orthographic ray grid."""
    t = _owner(accel)
    out = np.zeros(t.n_primitives(), dtype=np.float32)
    vd = np.ascontiguousarray(viewdir, dtype=np.float32)
    check(lib().rc_get_illumination(t._h, ptr(vd), int(grid_size), ptr(out)))
    return out


def get_illumination_dirs(accel, viewdirs, grid_size=1000, weights=None):
    """get_illumination (src/kernels.jl:112-124) for D view directions in one call: a (D, N) float32 array whose row d equals
    get_illumination(accel, viewdirs[d], grid_size) -- the integration over the sun's course or over sky sectors that the reference's users
    write as a loop.  With `weights` (length D, e.g. each direction's irradiance) the length-N float64 vector weights @ counts instead,
    formed on the host: inside the kernel a float weight would make the sum depend on the order of the atomics."""
    vd = np.ascontiguousarray(viewdirs, dtype=np.float32)
    if vd.ndim != 2 or vd.shape[1] != 3:
        raise ValueError("viewdirs must be a (D, 3) array of directions")
    w = None
    if weights is not None:
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (vd.shape[0],):
            raise ValueError("weights must hold one value per direction")
    import torch
    t = _owner(accel)
    n, d = t.n_primitives(), vd.shape[0]
    dev = f"cuda:{t.device}"
    torch.cuda.synchronize(t.device)  # (the call runs on the default stream: behind whatever the caller enqueued on streams of its own)
    dirs = torch.from_numpy(vd).to(dev)
    counts = torch.zeros(max(d * n, 1), dtype=torch.int32, device=dev)
    t.illumination_dirs_device(dirs.data_ptr(), d, grid_size, counts.data_ptr(), n)
    torch.cuda.synchronize(t.device)
    t.wait_for_gpu()  # (reports a traversal stack overflow, like the host-buffer get_illumination)
    rows = counts.cpu().numpy().view(np.uint32)[:d * n].reshape(d, n)
    rows = np.minimum(rows, np.uint32(1 << 24)).astype(np.float32)  # the reference's Float32 sums stop at 2^24
    return rows if w is None else w @ rows.astype(np.float64)


def point_sources(points, axes=None, max_dist=float("inf"), t_min=0.0):
    """The RAY_DT source records of get_illumination_points / illumination_points_device: o = points[k], d = axes[k] (zero or no axes:
    isotropic; anything else: a Lambertian emitter about it), t_min, t_max = max_dist (a scalar or one per source).  ValueError for shapes
    that do not fit, positions or axes that are not finite, a max_dist that is not > 0 (inf is legal) or a t_min that is not finite."""
    p = np.ascontiguousarray(points, dtype=np.float32)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("points must be a (S, 3) array of positions")
    if not np.isfinite(p).all():
        raise ValueError("points must be finite")
    s = p.shape[0]
    a = np.zeros((s, 3), np.float32)
    if axes is not None:
        a = np.ascontiguousarray(axes, dtype=np.float32)
        if a.shape != (s, 3):
            raise ValueError("axes must be a (S, 3) array, one axis per point (zero: isotropic)")
        if not np.isfinite(a).all():
            raise ValueError("axes must be finite")
    reach = np.asarray(max_dist, dtype=np.float32)
    if reach.shape not in ((), (s,)):
        raise ValueError("max_dist must be a scalar or hold one value per point")
    if not (reach > 0).all():
        raise ValueError("max_dist must be > 0 (inf: no limit)")
    near = np.asarray(t_min, dtype=np.float32)
    if near.shape not in ((), (s,)) or not np.isfinite(near).all():
        raise ValueError("t_min must be a finite scalar or hold one finite value per point")
    src = np.zeros(s, RAY_DT)
    src["o"], src["d"], src["tmin"], src["tmax"] = p, a, near, reach
    return src


def get_illumination_points(accel, points, grid_size=256, axes=None, max_dist=float("inf"), weights=None, seed=0, return_escaped=False):
    """get_illumination (src/kernels.jl:112-124) for S POINT sources inside the scene -- lamps, heaters, antennas -- in one call: every
    source shoots grid_size^2 jittered, stratified, equal-area rays, and the closest hits are counted per source and primitive.  Returns
    the (S, N) uint32 counts.  For an isotropic source (no axis, or a zero one) counts[k, j] / grid_size^2 is the fraction of the lamp's
    flux that arrives at the primitives with metadata j + 1, their visible solid angle over 4 pi; with axes[k] != 0 source k is a
    Lambertian emitter about that axis and the fraction is its form factor to them.  max_dist: the lamps' range, a scalar or one per
    source.  With `weights` (length S, each lamp's flux) the float64 N-vector weights @ counts / grid_size^2 instead, formed on the host
    -- the convention of get_illumination_dirs --: the received flux per primitive, the `emission` of radiosity() up to reflectance and
    area.  return_escaped: also the (S,) uint32 counts of rays that hit nothing."""
    src = point_sources(points, axes, max_dist)
    s = len(src)
    if isinstance(grid_size, bool) or not isinstance(grid_size, (int, np.integer)) or not 0 <= int(grid_size) < 65536:
        raise ValueError("grid_size must be an integer in 0..65535")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < (1 << 64):
        raise ValueError("seed must be an integer in 0..2^64 - 1")
    w = None
    if weights is not None:
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (s,):
            raise ValueError("weights must hold one value per point")
        if int(grid_size) == 0:
            raise ValueError("weights need a grid_size above 0")
    import torch
    t = _owner(accel)
    n = t.n_primitives()
    dev = f"cuda:{t.device}"
    torch.cuda.synchronize(t.device)  # (the call runs on the default stream: behind whatever the caller enqueued on streams of its own)
    d_src = torch.from_numpy(src.view(np.uint8).reshape(-1).copy()).to(dev) if s else None
    counts = torch.zeros(max(s * n, 1), dtype=torch.int32, device=dev)
    escaped = torch.zeros(max(s, 1), dtype=torch.int32, device=dev)
    t.illumination_points_device(d_src.data_ptr() if s else None, s, int(grid_size), counts.data_ptr(), n, escaped.data_ptr(), seed=int(seed))
    torch.cuda.synchronize(t.device)
    t.wait_for_gpu()  # (reports a traversal stack overflow, like the host-buffer get_illumination)
    rows = counts.cpu().numpy().view(np.uint32)[:s * n].reshape(s, n).copy()
    out = rows if w is None else (w @ rows.astype(np.float64)) / (float(int(grid_size)) ** 2)
    return (out, escaped.cpu().numpy().view(np.uint32)[:s].copy()) if return_escaped else out


def ambient_occlusion(accel, rays, hits, samples, max_dist=float("inf"), seed=0, bias=1e-3):
    """How open is the hemisphere above every hit?  rays / hits: the RAY_DT rays and the HIT_DT records a closest-hit trace of them
    returned.  Returns the (n,) uint32 counts of the `samples` cosine-weighted samples per hit that reach max_dist unoccluded (0 where
    the ray missed): count / samples is the point's openness, its sky-view factor with max_dist = inf.  Upload, one
    ambient_occlusion_device call, download."""
    r = _as_rays(rays)
    h = np.ascontiguousarray(hits)
    if h.dtype != HIT_DT or h.shape != r.shape:
        raise ValueError("hits must be a HIT_DT array with one record per ray")
    import torch
    t = _owner(accel)
    n = len(r)
    dev = f"cuda:{t.device}"
    torch.cuda.synchronize(t.device)  # (the call runs on the default stream: behind whatever the caller enqueued on streams of its own)
    d_rays = torch.from_numpy(r.view(np.uint8).reshape(-1).copy()).to(dev)
    d_hits = torch.from_numpy(h.view(np.uint8).reshape(-1).copy()).to(dev)
    counts = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    t.ambient_occlusion_device(d_rays.data_ptr(), d_hits.data_ptr(), n, samples, counts.data_ptr(), max_dist=max_dist, seed=seed, bias=bias)
    torch.cuda.synchronize(t.device)
    t.wait_for_gpu()  # (reports a traversal stack overflow)
    return counts.cpu().numpy().view(np.uint32)[:n].copy()


def _gather_inputs(rays, hits, samples, max_dist, miss_value):
    """(rays, hits, samples, max_dist, miss_value) of final_gather, checked without a device: ValueError for what
    rc_final_gather_device would refuse, and for a miss_value that is no u32."""
    from .wavefront import check_gather_arguments
    r = _as_rays(rays)
    h = np.ascontiguousarray(hits)
    if h.dtype != HIT_DT or h.shape != r.shape:
        raise ValueError("hits must be a HIT_DT array with one record per ray")
    return (r, h) + check_gather_arguments(len(r), samples, max_dist, miss_value)


def final_gather(accel, rays, hits, x, samples, max_dist=float("inf"), miss_value=0, seed=0, bias=1e-3):
    """The final gather: how much of a per-primitive field arrives at every hit?  rays / hits: the RAY_DT rays and the HIT_DT records a
    closest-hit trace of them returned; x: uint32, one value per primitive, indexed by metadata - 1 (view_factor_bounces' result, say).
    Returns (sums, open): sums (n,) uint64 -- x summed over what the `samples` cosine-weighted samples of each hit's hemisphere hit
    first (metadata outside 1..N adds nothing), miss_value for every sample that reaches max_dist --, and open (n,) uint32, the samples
    that escape: ambient_occlusion()'s counts.  sums / samples is the cosine-weighted mean of x over the hemisphere.  Upload, one
    final_gather_device call, download."""
    r, h, samples, max_dist, miss_value = _gather_inputs(rays, hits, samples, max_dist, miss_value)
    check_products_x(x)
    import torch
    t = _owner(accel)
    x = check_products_x(x, t.n_primitives())
    n = len(r)
    dev = f"cuda:{t.device}"
    torch.cuda.synchronize(t.device)  # (the call runs on the default stream: behind whatever the caller enqueued on streams of its own)
    d_rays = torch.from_numpy(r.view(np.uint8).reshape(-1).copy()).to(dev)
    d_hits = torch.from_numpy(h.view(np.uint8).reshape(-1).copy()).to(dev)
    d_x = torch.from_numpy(x.view(np.int32).copy()).to(dev)
    sums = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
    opened = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    t.final_gather_device(d_rays.data_ptr(), d_hits.data_ptr(), n, samples, d_x.data_ptr(), sums.data_ptr(), opened.data_ptr(), miss_value=miss_value,
                          max_dist=max_dist, seed=seed, bias=bias)
    torch.cuda.synchronize(t.device)
    t.wait_for_gpu()  # (reports a traversal stack overflow)
    return sums.cpu().numpy().view(np.uint64)[:n].copy(), opened.cpu().numpy().view(np.uint32)[:n].copy()


def irradiance_scale(b, sky=0.0):
    """The quantisation of irradiance(): (scale, b_q, sky_q) with ONE scale for the field and the sky, scale = (2^32 - 1) / max(max b, sky)
    (1 when both are zero), b_q = floor(b * scale) as uint32 and sky_q = floor(sky * scale) -- floor, as radiosity_scale quantises
    emission.  ValueError unless b is a vector of finite values >= 0 and sky is finite and >= 0."""
    b = np.asarray(b, dtype=np.float64)
    sky = float(sky)
    if b.ndim != 1:
        raise ValueError("b must be a vector with one value per primitive")
    if not np.isfinite(b).all() or (b < 0).any():
        raise ValueError("b must be finite and non-negative")
    if not np.isfinite(sky) or sky < 0:
        raise ValueError("sky must be finite and non-negative")
    top = max(float(b.max()) if b.size else 0.0, sky)
    scale = U32_MAX / top if top > 0 else 1.0
    b_q = np.minimum(np.floor(b * scale), U32_MAX).astype(np.uint32)
    return scale, b_q, int(min(np.floor(sky * scale), U32_MAX))


def irradiance(accel, rays, hits, b, samples, sky=0.0, max_dist=float("inf"), seed=0, bias=1e-3, return_open=False):
    """The cosine-weighted mean of the per-primitive field b over the hemisphere above every hit, float64 (n,): the mean over `samples`
    cosine-weighted directions of b at whatever each direction hits first, `sky` for a direction that reaches max_dist.  When b is a
    Lambertian radiosity (radiosity()'s result) this is the IRRADIANCE at the point in b's units, sky being the sky's radiosity; multiply
    by the local reflectance for the reflected radiosity.  0 where the ray missed.
    b (float, >= 0, one value per primitive, indexed by metadata - 1) and sky are quantised with one scale, scale = (2^32 - 1) /
    max(max b, sky), with floor (irradiance_scale); the sums are exact integers (final_gather) and the result is sums / (samples * scale).
    One quantisation step is 1 / scale = max(max b, sky) / (2^32 - 1): every sample's value is at most one step below its float value,
    and so is their mean.  return_open: also return final_gather's open counts (ambient_occlusion()'s).  samples must be >= 1."""
    scale, b_q, sky_q = irradiance_scale(b, sky)
    if isinstance(samples, bool) or samples != int(samples) or int(samples) < 1:
        raise ValueError("samples must be an integer in [1, 65536)")
    sums, opened = final_gather(accel, rays, hits, b_q, samples, max_dist=max_dist, miss_value=sky_q, seed=seed, bias=bias)
    e = sums.astype(np.float64) / (int(samples) * scale)
    return (e, opened) if return_open else e


def check_placed_x(x, n=None):
    """x of placed_final_gather: a uint32 vector (of length n, once the placed-primitive count is known)."""
    if not isinstance(x, np.ndarray) or x.dtype != np.uint32 or x.ndim != 1:
        raise ValueError("x must be a one-dimensional uint32 array with one value per placed primitive")
    if n is not None and len(x) != n:
        raise ValueError(f"x must hold one value per placed primitive: {len(x)} values for {n} placed primitives")
    return np.ascontiguousarray(x)


def placed_hit_indices(accel, hits):
    """The placed primitive each hit record names (rc_placed_hit_indices_device): (n,) uint32, q = base[instance_id] + the primitive's
    position inside its instance's BLAS for a hit, 2^32 - 1 (RC_INVALID_ID) for a miss.  hits: the HIT_DT records a closest-hit trace
    returned.  B[q] is a placed solution's value on the surface each ray sees.  Upload, one placed_hit_indices_device call, download."""
    h = np.ascontiguousarray(hits)
    if h.dtype != HIT_DT or h.ndim != 1:
        raise ValueError("hits must be a one-dimensional HIT_DT array")
    import torch
    t = _owner(accel)
    n = len(h)
    dev = f"cuda:{t.device}"
    torch.cuda.synchronize(t.device)  # (the call runs on the default stream: behind whatever the caller enqueued on streams of its own)
    d_hits = torch.from_numpy(h.view(np.uint8).reshape(-1).copy()).to(dev) if n else torch.zeros(32, dtype=torch.uint8, device=dev)
    d_q = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    t.placed_hit_indices_device(d_hits.data_ptr(), n, d_q.data_ptr())
    torch.cuda.synchronize(t.device)
    return d_q.cpu().numpy().view(np.uint32)[:n].copy()


def placed_final_gather(accel, rays, hits, x, samples, max_dist=float("inf"), miss_value=0, seed=0, bias=1e-3):
    """final_gather for a field per PLACED primitive (rc_placed_final_gather_device).  x: uint32, one value per placed primitive, indexed by
    q = base[i] + l (placed_primitive_bases(); placed_radiosity's result, say): two instances of one mesh carry different values, and no
    metadata takes part -- every hit is counted.  Returns (sums, open) as final_gather does: sums (n,) uint64 -- x summed over what the
    `samples` cosine-weighted samples of each hit's hemisphere hit first, miss_value for every sample that reaches max_dist --, and open
    (n,) uint32, the samples that escape: final_gather's and ambient_occlusion()'s counts.  Upload, one placed_final_gather_device call,
    download."""
    r, h, samples, max_dist, miss_value = _gather_inputs(rays, hits, samples, max_dist, miss_value)
    check_placed_x(x)
    import torch
    t = _owner(accel)
    x = check_placed_x(x, int(t.placed_primitive_bases()[-1]))
    n = len(r)
    dev = f"cuda:{t.device}"
    torch.cuda.synchronize(t.device)  # (the call runs on the default stream: behind whatever the caller enqueued on streams of its own)
    d_rays = torch.from_numpy(r.view(np.uint8).reshape(-1).copy()).to(dev)
    d_hits = torch.from_numpy(h.view(np.uint8).reshape(-1).copy()).to(dev)
    d_x = torch.from_numpy(x.view(np.int32).copy()).to(dev)
    sums = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
    opened = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    t.placed_final_gather_device(d_rays.data_ptr(), d_hits.data_ptr(), n, samples, d_x.data_ptr(), sums.data_ptr(), opened.data_ptr(),
                                 miss_value=miss_value, max_dist=max_dist, seed=seed, bias=bias)
    torch.cuda.synchronize(t.device)
    t.wait_for_gpu()  # (reports a traversal stack overflow)
    return sums.cpu().numpy().view(np.uint64)[:n].copy(), opened.cpu().numpy().view(np.uint32)[:n].copy()


def placed_irradiance(accel, rays, hits, b, samples, sky=0.0, max_dist=float("inf"), seed=0, bias=1e-3, return_open=False):
    """irradiance() for a field per PLACED primitive: the cosine-weighted mean of b over the hemisphere above every hit, float64 (n,), with
    b (float, >= 0) holding one value per placed primitive q = base[i] + l -- placed_radiosity's result: the IRRADIANCE at the point in
    b's units, `sky` for a direction that reaches max_dist; multiply by the local reflectance for the reflected radiosity.  0 where the
    ray missed.  The quantisation is irradiance()'s (irradiance_scale, one step 1 / scale = max(max b, sky) / (2^32 - 1), floor); the sums
    are exact integers (placed_final_gather).  return_open: also return the open counts.  samples must be >= 1."""
    scale, b_q, sky_q = irradiance_scale(b, sky)
    if isinstance(samples, bool) or samples != int(samples) or int(samples) < 1:
        raise ValueError("samples must be an integer in [1, 65536)")
    sums, opened = placed_final_gather(accel, rays, hits, b_q, samples, max_dist=max_dist, miss_value=sky_q, seed=seed, bias=bias)
    e = sums.astype(np.float64) / (int(samples) * scale)
    return (e, opened) if return_open else e


def _vf_out(n, out):
    if out is None:
        return np.empty((n, n), dtype=np.uint32, order="F")  # every element is written by the library
    if out.dtype != np.uint32 or out.shape != (n, n) or not out.flags["F_CONTIGUOUS"]:
        raise ValueError("out must be an (N, N) uint32 array in column-major (Fortran) order, like Julia's Matrix")
    return out


def view_factors(accel, rays_per_triangle=10000, seed=0, out=None):
    """view_factors (src/kernels.jl:74-104): N x N UInt32 matrix, [src_meta, hit_meta] (column-major like Julia's Matrix).  Row chunks
    are traced while the finished ones travel to the host matrix, so the call costs about the PCIe time of 4 N^2 bytes.  `out` reuses
    a matrix (a render / solve loop saves the page faults of a fresh one)."""
    t = _owner(accel)
    out = _vf_out(t.n_primitives(), out)
    check(lib().rc_view_factors(t._h, int(rays_per_triangle), int(seed), ptr(out)))
    return out


VF_MODE_ROWS, VF_MODE_RAYS = 0, 1


def view_factors_multi(accels, rays_per_triangle=10000, seed=0, mode="rows", out=None):
    """view_factors on several devices of ONE process (rc_view_factors_multi): `accels` are synced accels holding the same geometry,
    one per device.  mode="rows": accel g traces matrix rows [gN/G, (g+1)N/G) and copies them into the host matrix over its own PCIe
    link; mode="rays": every device shoots rays_per_triangle / G rays of every source, RCCL ncclReduce over xGMI into the first
    device (BASELINE's north-star partition).  Same matrix either way, bit for bit."""
    owners = [_owner(a) for a in accels]
    n = owners[0].n_primitives()
    out = _vf_out(n, out)
    handles = (C.c_void_p * len(owners))(*[o._h for o in owners])
    check(lib().rc_view_factors_multi(handles, len(owners), int(rays_per_triangle), int(seed), ptr(out), {"rows": VF_MODE_ROWS, "rays": VF_MODE_RAYS}[mode]))
    return out


def view_factor_totals(accel, rays_per_triangle=10000, seed=0):
    """Per-triangle totals of the view-factor job WITHOUT the N x N matrix (rc_view_factor_totals): (received, emitted), uint64 vectors of
    length N with received[j] = sum(view_factors(...)[:, j]) -- the rays arriving at metadata j+1, what the reference's users compute from
    the matrix (docs/src/viewfactors_content.md:62-68) -- and emitted[i] = sum(view_factors(...)[i, :]).  Costs the tracing only."""
    t = _owner(accel)
    n = t.n_primitives()
    received, emitted = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    check(lib().rc_view_factor_totals(t._h, int(rays_per_triangle), int(seed), ptr(received), ptr(emitted)))
    return received, emitted


def view_factor_totals_multi(accels, rays_per_triangle=10000, seed=0):
    """The same totals with the RAYS sharded over several devices of one process (rc_view_factor_totals_multi): accel g shoots ray indices
    [g R / G, (g+1) R / G) of every source; one RCCL ncclReduce (uint64, 2 N elements) over xGMI into the first device when the accels sit
    on distinct devices, a host sum for replicas on one device.  Identical vectors for every G."""
    owners = [_owner(a) for a in accels]
    n = owners[0].n_primitives()
    received, emitted = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    handles = (C.c_void_p * len(owners))(*[o._h for o in owners])
    check(lib().rc_view_factor_totals_multi(handles, len(owners), int(rays_per_triangle), int(seed), ptr(received), ptr(emitted)))
    return received, emitted


U32_MAX = (1 << 32) - 1
REFLECTANCE_ONE = 1 << 16  # view_factor_bounces' reflectance is 16.16 fixed point


def check_products_x(x, n=None):
    """x of view_factor_products: a uint32 vector (of length n, once the primitive count is known)."""
    if not isinstance(x, np.ndarray) or x.dtype != np.uint32 or x.ndim != 1:
        raise ValueError("x must be a one-dimensional uint32 array with one value per primitive")
    if n is not None and len(x) != n:
        raise ValueError(f"x must hold one value per primitive: {len(x)} values for {n} primitives")
    return np.ascontiguousarray(x)


def view_factor_products(accel, x, rays_per_triangle=10000, seed=0):
    """The view-factor matrix applied to a vector WITHOUT the N x N matrix (rc_view_factor_products): (mx, mtx), uint64 vectors with
    mx = M @ x and mtx = M.T @ x modulo 2^64, M = view_factors(accel, rays_per_triangle, seed) as a [src_meta - 1, hit_meta - 1] array.
    x: uint32, length N.  With x = 1 these are view_factor_totals' emitted and received.  Costs the tracing only."""
    check_products_x(x)
    t = _owner(accel)
    n = t.n_primitives()
    x = check_products_x(x, n)
    mx, mtx = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    check(lib().rc_view_factor_products(t._h, int(rays_per_triangle), int(seed), ptr(x), ptr(mx), ptr(mtx)))
    return mx, mtx


VF_SAMPLING = {"uniform": 0, "cosine": 1}  # RC_VF_SAMPLING_UNIFORM (the reference's rays) / RC_VF_SAMPLING_COSINE (Lambertian: form factors)
MAX_VF_GROUPS = 65535
VF_NO_GROUP = U32_MAX  # a group value that excludes a primitive whatever n_groups is


def vf_sampling(sampling):
    """The RC_VF_SAMPLING_* word of "uniform" / "cosine" (or of 0 / 1).  ValueError for anything else."""
    if isinstance(sampling, str) and sampling in VF_SAMPLING:
        return VF_SAMPLING[sampling]
    if not isinstance(sampling, (bool, str)) and isinstance(sampling, (int, np.integer)) and int(sampling) in (0, 1):
        return int(sampling)
    raise ValueError(f"sampling must be 'uniform' or 'cosine', not {sampling!r}")


def _u32_vector(a, what):
    """A one-dimensional array of integers in 0..2^32 - 1 as contiguous uint32.  ValueError otherwise."""
    a = np.asarray(a)
    if a.ndim != 1 or a.dtype.kind not in "iu":
        raise ValueError(f"{what} must be a one-dimensional integer array with one value per primitive")
    if a.size and (int(a.min()) < 0 or int(a.max()) > U32_MAX):
        raise ValueError(f"{what} must lie in 0..2^32 - 1")
    return np.ascontiguousarray(a.astype(np.uint32))


def check_groups_arguments(groups, weights, rays_per_triangle, seed, sampling, n_groups):
    """The arguments of view_factor_groups, checked before any device is touched: (groups u32, weights u32 or None, sampling word, G)."""
    g = _u32_vector(groups, "groups")
    w = None if weights is None else _u32_vector(weights, "weights")
    if w is not None and len(w) != len(g):
        raise ValueError(f"groups and weights must hold one value per primitive each: {len(g)} groups, {len(w)} weights")
    if isinstance(rays_per_triangle, bool) or not isinstance(rays_per_triangle, (int, np.integer)) or not 0 <= int(rays_per_triangle) <= U32_MAX:
        raise ValueError("rays_per_triangle must be an integer in 0..2^32 - 1")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < (1 << 64):
        raise ValueError("seed must be an integer in 0..2^64 - 1")
    word = vf_sampling(sampling)
    if n_groups is None:
        named = g[g < VF_NO_GROUP]
        n_groups = int(named.max()) + 1 if named.size else 0
    if isinstance(n_groups, bool) or not isinstance(n_groups, (int, np.integer)) or not 1 <= int(n_groups) <= MAX_VF_GROUPS:
        raise ValueError(f"n_groups must be an integer in 1..{MAX_VF_GROUPS} (the default is the largest group below 2^32 - 1, plus one)")
    return g, w, word, int(n_groups)


def view_factor_groups(accel, groups, rays_per_triangle=10000, seed=0, weights=None, sampling="uniform", n_groups=None, return_escaped=False):
    """Weighted view-factor counts between GROUPS of primitives -- walls, bodies, thermal zones -- without the N x N matrix
    (rc_view_factor_groups_device): the (G, G) uint64 array [source group, hit group].  groups[i] is the 0-based group of the primitives
    with metadata i + 1 (length N; a value >= n_groups, 2^32 - 1 say, leaves them out as sources and as targets); weights[i] (uint32,
    default 1) is what each of their rays adds.  Every primitive shoots rays_per_triangle rays: sampling "uniform" shoots the
    reference's (then the result is P diag(w) M P^T of M = view_factors(accel, rays_per_triangle, seed), exactly), "cosine" shoots
    them cosine-weighted about the normal, as a Lambertian surface emits: the counts of FORM factors (form_factors()).  A ray that hits
    its own source's metadata is not counted (the reference's rule); one that hits nothing is counted in `escaped` ((G,) uint64,
    returned too with return_escaped).  n_groups defaults to the largest group below 2^32 - 1, plus one.  Upload, one call, download.
    ValueError for wrong lengths, values outside u32, an unknown sampling or n_groups outside 1..65535."""
    g, w, word, G = check_groups_arguments(groups, weights, rays_per_triangle, seed, sampling, n_groups)
    import torch
    t = _owner(accel)
    n = t.n_primitives()
    if len(g) != n:
        raise ValueError(f"groups must hold one value per primitive: {len(g)} values for {n} primitives")
    dev = f"cuda:{t.device}"
    torch.cuda.synchronize(t.device)  # (the call runs on the default stream: behind whatever the caller enqueued on streams of its own)
    d_g = torch.from_numpy(g.view(np.int32)).to(dev) if n else None
    d_w = torch.from_numpy(w.view(np.int32)).to(dev) if (w is not None and n) else None
    out = torch.zeros(G * G + G, dtype=torch.int64, device=dev)
    if n:
        t.view_factor_groups_device(d_g.data_ptr(), G, out.data_ptr(), int(rays_per_triangle), int(seed), word, d_w.data_ptr() if d_w is not None else None,
                                    out.data_ptr() + 8 * G * G)
    torch.cuda.synchronize(t.device)
    t.wait_for_gpu()  # (reports a traversal stack overflow)
    words = out.cpu().numpy().view(np.uint64)
    matrix, escaped = words[:G * G].reshape(G, G).copy(), words[G * G:].copy()
    return (matrix, escaped) if return_escaped else matrix


def form_factor_weights(areas, rays_per_triangle):
    """Integer ray weights proportional to the primitives' areas, for view_factor_groups: w = floor(areas * s) as uint32, with s the
    largest scale for which every w <= 2^32 - 1 and rays_per_triangle * sum(w) < 2^63 (the u64 sums of a group then never wrap, and fit
    an int64).  Pure numpy.  ValueError unless areas is a vector of finite values >= 0 with a positive one, and rays_per_triangle an
    integer in 1..2^32 - 1."""
    a = np.asarray(areas, dtype=np.float64)
    if a.ndim != 1 or not np.isfinite(a).all() or (a < 0).any() or not (a > 0).any():
        raise ValueError("areas must be a vector of finite, non-negative values, at least one of them positive")
    if isinstance(rays_per_triangle, bool) or not isinstance(rays_per_triangle, (int, np.integer)) or not 1 <= int(rays_per_triangle) <= U32_MAX:
        raise ValueError("rays_per_triangle must be an integer in 1..2^32 - 1")
    R = int(rays_per_triangle)
    s = min(U32_MAX / float(a.max()), float(1 << 63) / (R * float(a.sum())))
    while True:
        w = np.minimum(np.floor(a * s), float(U32_MAX)).astype(np.uint64)
        if R * int(w.sum(dtype=np.uint64)) < (1 << 63):  # (sum(w) <= N * 2^32 < 2^64: the u64 sum itself does not wrap)
            return w.astype(np.uint32)
        s = np.nextafter(s, 0.0)  # the float quotient rounded up: one step down restores the bound


def primitive_areas(accel):
    """The areas of the scene's primitives as float64, indexed by metadata - 1 (the order of groups and weights), from the exported
    primitives: |cross(v1 - v0, v2 - v0)| / 2 in float64.  ValueError unless the metadata are a permutation of 1..N (the view-factor
    convention, src/kernels.jl:85)."""
    prims = _owner(accel)._prims()
    n = len(prims)
    meta = prims["meta"].astype(np.int64)
    if not np.array_equal(np.sort(meta), np.arange(1, n + 1)):
        raise ValueError("primitive_areas needs metadata that are a permutation of 1..N")
    v = prims["v"].astype(np.float64)
    out = np.empty(n, np.float64)
    out[meta - 1] = 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)
    return out


def form_factors_from_counts(matrix, escaped, groups, weights, rays_per_triangle):
    """The float arithmetic of form_factors on view_factor_groups' integers: F[A, B] = matrix[A, B] / (R * sum_{i in A} w_i) and escaped[A]
    likewise, float64; a group without weight gets zeros.  The denominators are formed in Python integers."""
    matrix, escaped = np.asarray(matrix, np.uint64), np.asarray(escaped, np.uint64)
    G = len(escaped)
    g, w = np.asarray(groups, np.int64), np.asarray(weights, np.uint64)
    denom = np.array([int(rays_per_triangle) * int(w[g == A].sum(dtype=np.uint64)) for A in range(G)], dtype=np.float64)
    safe = np.where(denom > 0, denom, 1.0)
    return matrix.astype(np.float64) / safe[:, None], escaped.astype(np.float64) / safe


def form_factors(accel, groups, rays_per_triangle=10000, seed=0, n_groups=None):
    """Form factors between groups of primitives: (F, escaped), float64, F[A, B] = the fraction of the energy a Lambertian surface A emits
    that arrives at surface B first, escaped[A] the fraction that leaves the scene.  Cosine sampling with area weights:
    F_AB = sum_{i in A} A_i F_iB / A_A is estimated by view_factor_groups(..., weights=form_factor_weights(primitive_areas(accel), R),
    sampling="cosine") over R * sum_{i in A} w_i.  Rays between two primitives of the SAME metadata are not counted; rows sum to at most 1.
    groups: as in view_factor_groups.  A G x G radiosity solve on F is one numpy line: B = solve(I - diag(rho) F, E)."""
    check_groups_arguments(groups, None, rays_per_triangle, seed, "cosine", n_groups)
    w = form_factor_weights(primitive_areas(accel), rays_per_triangle)
    matrix, escaped = view_factor_groups(accel, groups, rays_per_triangle, seed, weights=w, sampling="cosine", n_groups=n_groups, return_escaped=True)
    return form_factors_from_counts(matrix, escaped, groups, w, rays_per_triangle)


def placed_primitive_count(accel):
    """P, the number of placed primitives of the scene: the sum over the instances of their BLAS's primitive count."""
    return int(_owner(accel).placed_primitive_bases()[-1])


def placed_primitive_areas(accel):
    """The areas of the scene's PLACED primitives as float64, indexed by placed primitive q, from the world triangles
    (rc_placed_triangles_device): |cross(p2 - p1, p3 - p1)| / 2 in float64."""
    import torch
    t = _owner(accel)
    P = int(t.placed_primitive_bases()[-1])
    torch.cuda.synchronize(t.device)
    d_v = torch.empty(max(9 * P, 1), dtype=torch.float32, device=f"cuda:{t.device}")
    t.placed_triangles_device(d_v.data_ptr(), 0, P)
    torch.cuda.synchronize(t.device)
    v = d_v.cpu().numpy()[:9 * P].reshape(P, 3, 3).astype(np.float64)
    return 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)


def placed_groups(accel, per_instance=None):
    """The `groups` of placed_view_factor_groups from one group number per instance (uint32, length n_inst; a value >= n_groups leaves
    the instance out), expanded to P entries by np.repeat over the bases.  per_instance=None: every instance is its own group."""
    g = None if per_instance is None else _u32_vector(per_instance, "per_instance")
    bases = _owner(accel).placed_primitive_bases().astype(np.int64)
    n_inst = len(bases) - 1
    if g is None:
        g = np.arange(n_inst, dtype=np.uint32)
    if len(g) != n_inst:
        raise ValueError(f"per_instance must hold one group per instance: {len(g)} values for {n_inst} instances")
    return np.repeat(g, np.diff(bases))


def placed_view_factor_groups(accel, groups, rays_per_triangle=10000, seed=0, weights=None, sampling="uniform", n_groups=None, return_escaped=False):
    """view_factor_groups with the sources in WORLD space (rc_placed_view_factor_groups_device): the (G, G) uint64 array [source group,
    hit group] between groups of PLACED primitives.  groups[q] / weights[q] belong to placed primitive q = base[i] + l -- primitive l of
    instance i, placed_primitive_bases() -- so length P, not N; placed_groups() makes them from one number per instance.  Every placed
    primitive shoots rays_per_triangle rays from where its instance's transform puts it; a ray that hits its own placed primitive is
    not counted, one that hits nothing is counted in `escaped`.  No metadata takes part.  Arguments and errors as view_factor_groups."""
    g, w, word, G = check_groups_arguments(groups, weights, rays_per_triangle, seed, sampling, n_groups)
    import torch
    t = _owner(accel)
    P = int(t.placed_primitive_bases()[-1])
    if len(g) != P:
        raise ValueError(f"groups must hold one value per placed primitive: {len(g)} values for {P} placed primitives")
    dev = f"cuda:{t.device}"
    torch.cuda.synchronize(t.device)  # (the call runs on the default stream: behind whatever the caller enqueued on streams of its own)
    d_g = torch.from_numpy(g.view(np.int32)).to(dev) if P else None
    d_w = torch.from_numpy(w.view(np.int32)).to(dev) if (w is not None and P) else None
    out = torch.zeros(G * G + G, dtype=torch.int64, device=dev)
    if P:
        t.placed_view_factor_groups_device(d_g.data_ptr(), G, out.data_ptr(), int(rays_per_triangle), int(seed), word,
                                           d_w.data_ptr() if d_w is not None else None, out.data_ptr() + 8 * G * G)
    torch.cuda.synchronize(t.device)
    t.wait_for_gpu()  # (reports a traversal stack overflow)
    words = out.cpu().numpy().view(np.uint64)
    matrix, escaped = words[:G * G].reshape(G, G).copy(), words[G * G:].copy()
    return (matrix, escaped) if return_escaped else matrix


def placed_form_factors(accel, groups, rays_per_triangle=10000, seed=0, n_groups=None):
    """form_factors between groups of PLACED primitives: (F, escaped), float64.  Cosine sampling with
    form_factor_weights(placed_primitive_areas(accel), R); the quotients are form_factors_from_counts'."""
    check_groups_arguments(groups, None, rays_per_triangle, seed, "cosine", n_groups)
    w = form_factor_weights(placed_primitive_areas(accel), rays_per_triangle)
    matrix, escaped = placed_view_factor_groups(accel, groups, rays_per_triangle, seed, weights=w, sampling="cosine", n_groups=n_groups, return_escaped=True)
    return form_factors_from_counts(matrix, escaped, groups, w, rays_per_triangle)


def instance_form_factors(accel, rays_per_triangle=10000, seed=0):
    """Form factors between the scene's INSTANCES: (F, escaped), F the n_inst x n_inst float64 matrix of placed_form_factors with every
    instance its own group (at most 65535 instances)."""
    return placed_form_factors(accel, placed_groups(accel), rays_per_triangle, seed)


def _is_tensor(a):
    return type(a).__module__.split(".")[0] == "torch"


def check_csr(row_ptr, cols, vals, n_cols=None):
    """The arrays of a CSR block, checked on the host before any library call: (row_ptr uint64, cols uint32, vals uint32), contiguous.
    row_ptr starts at 0, never decreases and ends at len(cols) == len(vals); with n_cols every column index is below it.  ValueError otherwise."""
    for a, dt, what in ((row_ptr, np.uint64, "row_ptr"), (cols, np.uint32, "cols"), (vals, np.uint32, "vals")):
        if not isinstance(a, np.ndarray) or a.dtype != dt or a.ndim != 1:
            raise ValueError(f"{what} must be a one-dimensional {np.dtype(dt).name} array")
    if len(row_ptr) < 1 or int(row_ptr[0]) != 0:
        raise ValueError("row_ptr must hold rows + 1 offsets and start at 0")
    if len(cols) != len(vals) or int(row_ptr[-1]) != len(cols):
        raise ValueError(f"row_ptr must end at the number of entries: row_ptr[-1] = {int(row_ptr[-1])}, {len(cols)} cols, {len(vals)} vals")
    if len(row_ptr) > 1 and (row_ptr[1:] < row_ptr[:-1]).any():
        raise ValueError("row_ptr must not decrease")
    if n_cols is not None and len(cols) and int(cols.max()) >= n_cols:
        raise ValueError(f"cols must lie below {n_cols}: the largest is {int(cols.max())}")
    return np.ascontiguousarray(row_ptr), np.ascontiguousarray(cols), np.ascontiguousarray(vals)


class SparseViewFactors(tuple):
    """A block of rows of the view-factor matrix in CSR: unpacks as (row_ptr uint64, cols uint32, vals uint32) -- the argument order of
    scipy.sparse.csr_matrix((vals, cols, row_ptr), shape=(len(row_ptr) - 1, n)) -- and remembers what the products need: `accel` (its
    owner runs the kernels), `n` (columns = length of x), `row_offset` (the matrix row of the block's first row), `rays_per_triangle` and
    `seed` it was traced with (None for a handmade matrix), `nnz` (the true count: larger than len(cols) after a build whose capacity was
    too small).  view_factors_sparse returns one whose arrays are ALSO still on the device (device_arrays()); one made from numpy arrays
    is uploaded on first use.  `placed`: rows and columns are PLACED primitives (placed_view_factors_sparse's result, n = P), and then
    `sampling` is the RC_VF_SAMPLING_* word it was traced with; False and None for every other matrix."""

    def __new__(cls, row_ptr, cols, vals, accel, n, row_offset=0, rays_per_triangle=None, seed=None, nnz=None, device=None, sampling=None, placed=False):
        self = super().__new__(cls, (row_ptr, cols, vals))
        self.accel, self.n, self.row_offset, self.rays_per_triangle, self.seed = accel, int(n), int(row_offset), rays_per_triangle, seed
        self.nnz = int(len(cols) if nnz is None else nnz)
        self._device = device
        self.sampling, self.placed = sampling, bool(placed)
        return self

    @classmethod
    def from_arrays(cls, accel, row_ptr, cols, vals, n=None, row_offset=0, rays_per_triangle=None, seed=None):
        """A CSR block from host arrays (checked: check_csr).  n: the number of columns (default: row_offset + rows, a square matrix)."""
        if isinstance(row_offset, bool) or int(row_offset) != row_offset or row_offset < 0:
            raise ValueError("row_offset must be a non-negative integer")
        rows = len(row_ptr) - 1 if isinstance(row_ptr, np.ndarray) else 0
        n = row_offset + rows if n is None else n
        if isinstance(n, bool) or int(n) != n or n < row_offset + rows or n >= 1 << 32:
            raise ValueError("n must be an integer with row_offset + rows <= n < 2^32")
        return cls(*check_csr(row_ptr, cols, vals, n), accel, n, row_offset, rays_per_triangle, seed)

    @property
    def n_rows(self):
        return len(self[0]) - 1

    def device_arrays(self):
        """(row_ptr int64, cols int32, vals int32) torch tensors on the accel's device holding the bit patterns of the unsigned words."""
        if self._device is None:
            import torch
            dev = torch.device("cuda", _owner(self.accel).device)
            self._device = tuple(torch.from_numpy(a.view(s)).to(dev) for a, s in zip(self, (np.int64, np.int32, np.int32)))
        return self._device


def check_sparse_arguments(rays_per_triangle, seed, rows, capacity):
    """The arguments of view_factors_sparse, checked before the library is touched."""
    if isinstance(rays_per_triangle, bool) or int(rays_per_triangle) != rays_per_triangle or not 1 <= rays_per_triangle < (1 << 32):
        raise ValueError("rays_per_triangle must be an integer in 1..2^32 - 1")
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= seed < (1 << 64):
        raise ValueError("seed must be an integer in 0..2^64 - 1")
    if rows is not None:
        if not isinstance(rows, (tuple, list)) or len(rows) != 2 or any(isinstance(r, bool) or int(r) != r for r in rows) or not 0 <= rows[0] <= rows[1] < (1 << 32):
            raise ValueError("rows must be (begin, end) with 0 <= begin <= end < 2^32")
    if capacity is not None and (isinstance(capacity, bool) or int(capacity) != capacity or capacity < 0):
        raise ValueError("capacity must be None or a non-negative integer")


def view_factors_sparse(accel, rays_per_triangle=10000, seed=0, rows=None, capacity=None):
    """The view-factor matrix itself, SPARSE (rc_view_factors_sparse_device): (row_ptr uint64, cols uint32, vals uint32), the canonical CSR
    of rows `rows` = (begin, end) (default: all; end is clamped to N) of M = view_factors(accel, rays_per_triangle, seed) as a
    [src_meta - 1, hit_meta - 1] array -- columns strictly ascending within a row, every value >= 1, row_ptr starting at 0.  The triple is
    in the argument order of scipy.sparse.csr_matrix((vals, cols, row_ptr), shape=(rows, N)); scipy is not needed here.  A row has at most
    min(rays_per_triangle, N) entries, so the result has at most rows x rays_per_triangle of them where the dense matrix has N^2 words.
    capacity=None: a counting call, then a filling call of exactly that size.  With a capacity, one call: the first min(nnz, capacity)
    entries are returned and `.nnz` of the result is the true count (row_ptr is always the true one).
    The result is a SparseViewFactors: the arrays stay on the device as well, for view_factor_sparse_products and view_factor_bounces."""
    check_sparse_arguments(rays_per_triangle, seed, rows, capacity)
    import torch
    t = _owner(accel)
    n = t.n_primitives()
    r0, r1 = (0, n) if rows is None else (min(int(rows[0]), n), min(int(rows[1]), n))
    dev = torch.device("cuda", t.device)
    st = torch.cuda.current_stream(dev)
    with torch.cuda.device(dev):
        head = torch.zeros(r1 - r0 + 2, dtype=torch.int64, device=dev)  # row_ptr[rows + 1], then nnz
        nnz_ptr = head.data_ptr() + 8 * (r1 - r0 + 1)
        if capacity is None:
            t.view_factors_sparse_device(head.data_ptr(), None, None, 0, nnz_ptr, rays_per_triangle, seed, (r0, r1), st.cuda_stream)
            capacity = int(head[-1].item())
        entries = torch.zeros((2, max(int(capacity), 1)), dtype=torch.int32, device=dev)
        t.view_factors_sparse_device(head.data_ptr(), entries[0].data_ptr() if capacity else None, entries[1].data_ptr() if capacity else None,
                                     int(capacity), nnz_ptr, rays_per_triangle, seed, (r0, r1), st.cuda_stream)
        st.synchronize()
        t.wait_for_gpu()  # (reports a traversal stack overflow)
        nnz = int(head[-1].item())
        filled = min(nnz, int(capacity))
        d_row_ptr, d_cols, d_vals = head[:r1 - r0 + 1], entries[0, :filled], entries[1, :filled]
        host = (d_row_ptr.cpu().numpy().view(np.uint64), d_cols.cpu().numpy().view(np.uint32), d_vals.cpu().numpy().view(np.uint32))
    return SparseViewFactors(*host, t, n, r0, int(rays_per_triangle), int(seed), nnz, (d_row_ptr, d_cols, d_vals))


def view_factor_sparse_products(csr, x):
    """(mx, mtx) = (M x, M^T x) modulo 2^64 for a CSR block `csr` (a SparseViewFactors: view_factors_sparse's result or
    SparseViewFactors.from_arrays) and x: uint32, one value per column -- uint64 vectors of the same length, zero outside the block's rows
    (mx) .  One memory-bound pass over the entries (rc_view_factor_sparse_products_device) where view_factor_products traces every ray
    again; with the CSR of the same rays_per_triangle and seed the words are equal.  The arrays and x are checked before the library is called."""
    if not isinstance(csr, SparseViewFactors):
        raise ValueError("csr must be a SparseViewFactors (view_factors_sparse's result, or SparseViewFactors.from_arrays)")
    check_products_x(x)
    if csr.nnz != len(csr[1]):
        raise ValueError(f"the matrix is truncated: {len(csr[1])} of {csr.nnz} entries (build it with a larger capacity)")
    check_csr(*csr, csr.n)
    x = check_products_x(x, csr.n)
    import torch
    t = _owner(csr.accel)
    dev = torch.device("cuda", t.device)
    st = torch.cuda.current_stream(dev)
    with torch.cuda.device(dev):
        row_ptr, cols, vals = csr.device_arrays()
        d_x = torch.from_numpy(x.view(np.int32)).to(dev)
        out = torch.zeros((2, max(csr.n, 1)), dtype=torch.int64, device=dev)
        t.view_factor_sparse_products_device(csr.n_rows, row_ptr.data_ptr(), cols.data_ptr(), vals.data_ptr(), d_x.data_ptr(), out[0].data_ptr(),
                                             out[1].data_ptr(), csr.row_offset, st.cuda_stream)
        st.synchronize()
        got = out.cpu().numpy().view(np.uint64)
    return got[0, :csr.n].copy(), got[1, :csr.n].copy()


def check_bounce_matrix(matrix):
    """The matrix of view_factor_bounces: all rows of a traced matrix, complete."""
    if matrix.rays_per_triangle is None or matrix.seed is None:
        raise ValueError("the matrix must come from view_factors_sparse: the bounce divides by its rays_per_triangle")
    if matrix.row_offset != 0 or matrix.n_rows != matrix.n:
        raise ValueError(f"the matrix must hold all rows: it holds {matrix.n_rows} from row {matrix.row_offset} of {matrix.n}")
    if matrix.nnz != len(matrix[1]):
        raise ValueError(f"the matrix is truncated: {len(matrix[1])} of {matrix.nnz} entries (build it with a larger capacity)")


def _u32_values(a, what, limit=U32_MAX):
    """A vector of integers in 0..limit as int64: a numpy integer array, or a device int64 / int32 torch tensor (int32: read as the bit
    patterns of u32 words).  Out of range: ValueError -- for a numpy array before anything touches the device."""
    if _is_tensor(a):
        import torch
        if a.dtype not in (torch.int64, torch.int32) or a.dim() != 1:
            raise ValueError(f"{what} must be a one-dimensional int64 or int32 tensor (or a numpy integer array)")
        v = a.to(torch.int64)
        if a.dtype == torch.int32:
            v = v & U32_MAX
        if v.numel() and (int(v.min()) < 0 or int(v.max()) > limit):
            raise ValueError(f"{what} must lie in 0..{limit}")
        return v
    v = np.asarray(a)
    if v.ndim != 1 or v.dtype.kind not in "iu":
        raise ValueError(f"{what} must be a one-dimensional integer array")
    if v.size and (int(v.min()) < 0 or int(v.max()) > limit):
        raise ValueError(f"{what} must lie in 0..{limit}")
    return v.astype(np.int64)


def check_bounce_arguments(emission, reflectance, bounces, rays_per_triangle):
    """The arguments of view_factor_bounces, checked before the library is touched: (emission, reflectance) as int64 vectors of equal length."""
    if isinstance(bounces, bool) or int(bounces) != bounces or bounces < 0:
        raise ValueError("bounces must be a non-negative integer")
    if isinstance(rays_per_triangle, bool) or int(rays_per_triangle) != rays_per_triangle or not 1 <= rays_per_triangle < (1 << 31):
        raise ValueError("rays_per_triangle must be in 1..2^31 - 1: (M x)[i] <= rays_per_triangle * (2^32 - 1) has to fit int64")
    e = _u32_values(emission, "emission")
    rho = _u32_values(reflectance, "reflectance", REFLECTANCE_ONE)
    if len(e) != len(rho):
        raise ValueError("emission and reflectance must have one value per primitive each")
    return e, rho


def view_factor_bounces(accel, emission, reflectance, bounces, rays_per_triangle=10000, seed=0, stream=None):
    """`bounces` steps of the radiosity iteration with the reference's sampled view-factor matrix, in integers, on the device:

        x_0 = e,    x_{k+1}[i] = min(2^32 - 1, e[i] + (((M x_k)[i] // R) * rho[i] >> 16))

    M is what view_factors(accel, R, seed) returns, as a [src_meta - 1, hit_meta - 1] array, R = rays_per_triangle: the REFERENCE's matrix,
    whose rays leave a triangle uniformly over the hemisphere -- view factors as the reference defines them, not cosine-corrected form
    factors (form_factors() gives those, cosine-sampled and area-weighted, between groups of primitives).  The same seed is used every bounce, so this is the iteration with that one matrix, and every step is exact: no float is
    involved, and the result does not depend on how the device orders its adds.
    emission: u32 per primitive (indexed by metadata - 1); reflectance: 0..65536, 16.16 fixed point (65536 = 1.0).  Both are numpy integer
    arrays or device int64 / int32 torch tensors (int32: the bit patterns of u32 words).  Each bounce is zero -> view_factor_products_device
    -> an elementwise torch update, all on `stream` (a torch stream or a raw handle; default: the current one) with no host wait between
    bounces; the matrix never exists.  Returns x: a uint32 numpy array for numpy input, else an int64 tensor on the device, ready on `stream`.
    ValueError for reflectance > 65536, values outside u32, or rays_per_triangle >= 2^31 ((M x)[i] must fit torch's int64).
    `accel` may be the MATRIX instead: a SparseViewFactors holding all rows (view_factors_sparse(accel, R, seed)).  Then nothing is traced:
    each bounce is zero -> view_factor_sparse_products_device (mx only) -> the same update, with the matrix's own accel, rays_per_triangle and
    seed (the two keyword arguments are not read), and the result is word for word the retraced one."""
    matrix = accel if isinstance(accel, SparseViewFactors) else None
    if matrix is not None:
        check_bounce_matrix(matrix)
        accel, rays_per_triangle, seed = matrix.accel, matrix.rays_per_triangle, matrix.seed
    e, rho = check_bounce_arguments(emission, reflectance, bounces, rays_per_triangle)
    if matrix is not None and len(e) != matrix.n:
        raise ValueError(f"emission and reflectance must hold one value per primitive: {len(e)} values for {matrix.n} primitives")
    import torch
    t = _owner(accel)
    n = t.n_primitives() if matrix is None else matrix.n
    if len(e) != n:
        raise ValueError(f"emission and reflectance must hold one value per primitive: {len(e)} values for {n} primitives")
    dev = torch.device("cuda", t.device)
    on_host = not _is_tensor(e)
    ts = stream if isinstance(stream, torch.cuda.Stream) else (torch.cuda.ExternalStream(int(stream), device=dev) if stream else torch.cuda.current_stream(dev))
    with torch.cuda.stream(ts):
        e, rho = (torch.from_numpy(a).to(dev) if not _is_tensor(a) else a.to(dev) for a in (e, rho))
        for a in (e, rho):
            a.record_stream(ts)  # (a caller's tensor, or its int64 copy made on the stream the caller was on)
        x = e.clone()
        x32 = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        mx = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        for _ in range(int(bounces)):
            if matrix is None:
                bounce_step(t, e, rho, x, x32, mx, int(rays_per_triangle), int(seed), ts.cuda_stream)
            else:
                bounce_step_sparse(matrix, e, rho, x, x32, mx, ts.cuda_stream)
    if on_host:
        ts.synchronize()
        t.wait_for_gpu()  # (reports a traversal stack overflow)
        return x.cpu().numpy().astype(np.uint32)
    return x


def bounce_step(t, e, rho, x, x32, mx, rays_per_triangle, seed, stream):
    """One bounce of view_factor_bounces on the current torch stream, whose raw handle is `stream`: x (int64, values in u32) is replaced by
    the next iterate; x32 (int32) and mx (int64) are scratch of the same length.  Nothing here waits for the device, so a loop of steps may
    be captured into a graph (after one eager step)."""
    import torch
    n = x.numel()
    x32[:n].copy_(x.view(torch.int32).view(n, 2)[:, 0])  # the low words: x as u32
    mx.zero_()
    t.view_factor_products_device(x32.data_ptr(), mx.data_ptr(), None, rays_per_triangle, seed, stream=stream)
    nxt = e + ((torch.div(mx[:n], rays_per_triangle, rounding_mode="floor") * rho) >> 16)  # (M x)[i] < 2^63: non-negative in int64
    x.copy_(nxt.clamp_(max=U32_MAX))


def bounce_step_sparse(matrix, e, rho, x, x32, mx, stream):
    """bounce_step with the matrix held sparse on the device (a SparseViewFactors with all rows): the same zero -> M x -> update, the product
    being one pass over the entries.  Nothing waits for the device or reads it on the host, so the step may be captured at once."""
    import torch
    n = x.numel()
    row_ptr, cols, vals = matrix.device_arrays()
    x32[:n].copy_(x.view(torch.int32).view(n, 2)[:, 0])
    mx.zero_()
    _owner(matrix.accel).view_factor_sparse_products_device(n, row_ptr.data_ptr(), cols.data_ptr(), vals.data_ptr(), x32.data_ptr(), mx.data_ptr(), None,
                                                           0, stream)
    nxt = e + ((torch.div(mx[:n], matrix.rays_per_triangle, rounding_mode="floor") * rho) >> 16)
    x.copy_(nxt.clamp_(max=U32_MAX))


def radiosity_scale(emission, reflectance):
    """The quantisation of radiosity(): (scale, e_q, rho_q) with e_q = floor(e * scale) u32 and rho_q = rint(rho * 65536); scale leaves the
    headroom 1 / (1 - max rho) of the converged solution below 2^32.  ValueError unless e is finite and >= 0 and rho lies in [0, 1)."""
    e = np.asarray(emission, dtype=np.float64)
    rho = np.asarray(reflectance, dtype=np.float64)
    if e.ndim != 1 or rho.shape != e.shape:
        raise ValueError("emission and reflectance must be vectors with one value per primitive each")
    if not np.isfinite(e).all() or (e < 0).any():
        raise ValueError("emission must be finite and non-negative")
    if not (np.isfinite(rho).all() and (rho >= 0).all() and (rho < 1).all()):
        raise ValueError("reflectance must lie in [0, 1)")
    rho_q = np.rint(rho * REFLECTANCE_ONE).astype(np.int64)
    top = min(int(rho_q.max()), REFLECTANCE_ONE - 1) / REFLECTANCE_ONE if rho_q.size else 0.0
    e_max = float(e.max()) if e.size else 0.0
    scale = U32_MAX * (1.0 - top) / e_max if e_max > 0 else 1.0
    e_q = np.minimum(np.floor(e * scale), U32_MAX).astype(np.int64)
    return scale, e_q, rho_q


def radiosity(accel, emission, reflectance, bounces, rays_per_triangle=10000, seed=0, stream=None, return_scale=False, matrix=None):
    """Radiosity by `bounces` steps of B <- E + rho .* (M B) / R in float terms: the convenience on top of view_factor_bounces.
    M is the REFERENCE's view-factor matrix view_factors(accel, R, seed), sampled with its uniform-hemisphere rays -- view factors as the
    reference defines them, NOT cosine-corrected form factors (for those, at the level of groups of primitives, see form_factors(): a
    G x G solve on its matrix is one numpy line).  emission: float array >= 0; reflectance: float array in [0, 1) (ValueError
    otherwise).  e is quantised to u32 with a scale that leaves the headroom 1 / (1 - max rho) below 2^32, rho to 16.16 fixed point
    (radiosity_scale), the iteration runs in integers on the device, and the result is scaled back to float64.
    return_scale: also return the scale (result = integer iterate / scale; one quantisation step is 1 / scale).
    matrix: the SparseViewFactors of view_factors_sparse(accel, rays_per_triangle, seed) -- the bounces then apply it instead of tracing
    (view_factor_bounces); the result is the same."""
    scale, e_q, rho_q = radiosity_scale(emission, reflectance)
    if matrix is not None and not isinstance(matrix, SparseViewFactors):
        raise ValueError("matrix must be a SparseViewFactors (view_factors_sparse's result)")
    x = view_factor_bounces(accel if matrix is None else matrix, e_q, rho_q, bounces, rays_per_triangle, seed, stream)
    b = x.astype(np.float64) / scale
    return (b, scale) if return_scale else b


def check_placed_products_arguments(x, rays_per_triangle, seed, sampling):
    """The arguments of placed_view_factor_products / placed_view_factor_totals (x = None), checked before any device is touched:
    (x as contiguous uint32 or None, the sampling word)."""
    if x is not None:
        if not isinstance(x, np.ndarray) or x.dtype != np.uint32 or x.ndim != 1:
            raise ValueError("x must be a one-dimensional uint32 array with one value per placed primitive")
        x = np.ascontiguousarray(x)
    if isinstance(rays_per_triangle, bool) or not isinstance(rays_per_triangle, (int, np.integer)) or not 0 <= int(rays_per_triangle) <= U32_MAX:
        raise ValueError("rays_per_triangle must be an integer in 0..2^32 - 1")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < (1 << 64):
        raise ValueError("seed must be an integer in 0..2^64 - 1")
    return x, vf_sampling(sampling)


def _placed_products(accel, x, rays_per_triangle, seed, word):
    """Upload, one rc_placed_view_factor_products_device over everything, download: (mx, mtx, escaped) as uint64 of length P."""
    import torch
    t = _owner(accel)
    P = int(t.placed_primitive_bases()[-1])
    if x is not None and len(x) != P:
        raise ValueError(f"x must hold one value per placed primitive: {len(x)} values for {P} placed primitives")
    dev = f"cuda:{t.device}"
    torch.cuda.synchronize(t.device)  # (the call runs on the default stream: behind whatever the caller enqueued on streams of its own)
    d_x = torch.from_numpy(x.view(np.int32)).to(dev) if (x is not None and P) else None
    out = torch.zeros(3 * max(P, 1), dtype=torch.int64, device=dev)
    if P:
        t.placed_view_factor_products_device(d_x.data_ptr() if d_x is not None else None, out.data_ptr(), out.data_ptr() + 8 * P, int(rays_per_triangle), int(seed),
                                             word, out.data_ptr() + 16 * P)
    torch.cuda.synchronize(t.device)
    t.wait_for_gpu()  # (reports a traversal stack overflow)
    words = out.cpu().numpy().view(np.uint64)
    return words[:P].copy(), words[P:2 * P].copy(), words[2 * P:3 * P].copy()


def placed_view_factor_products(accel, x, rays_per_triangle=10000, seed=0, sampling="uniform", return_escaped=False):
    """view_factor_products with the sources in WORLD space (rc_placed_view_factor_products_device): (mx, mtx[, escaped]), uint64 vectors of
    length P with mx = M @ x and mtx = M.T @ x modulo 2^64, M[a, b] = the rays of placed primitive a that hit placed primitive b != a
    first -- placed_view_factor_groups(accel, arange(P), ...) is that matrix.  x: uint32, length P, indexed by placed primitive
    q = base[i] + l (placed_primitive_bases()).  escaped[a] = the rays of a that hit nothing.  sampling "cosine": M / R estimates the
    Lambertian form factors between the placed primitives.  No metadata takes part.  Costs the tracing only.
    ValueError for a wrong length, an x that is not uint32, or an unknown sampling."""
    x, word = check_placed_products_arguments(x, rays_per_triangle, seed, sampling)
    if x is None:
        raise ValueError("x must be a one-dimensional uint32 array with one value per placed primitive")
    mx, mtx, escaped = _placed_products(accel, x, rays_per_triangle, seed, word)
    return (mx, mtx, escaped) if return_escaped else (mx, mtx)


def placed_view_factor_totals(accel, rays_per_triangle=10000, seed=0, sampling="uniform"):
    """view_factor_totals per PLACED primitive: (received, emitted, escaped), uint64 vectors of length P -- the rays that arrive at placed
    primitive q from another one, the rays of q that hit another one, and the rays of q that hit nothing.  placed_view_factor_products with
    x = 1 (the C call takes NULL for it): emitted[q] + escaped[q] + the hits of q on itself = rays_per_triangle."""
    _, word = check_placed_products_arguments(None, rays_per_triangle, seed, sampling)
    mx, mtx, escaped = _placed_products(accel, None, rays_per_triangle, seed, word)
    return mtx, mx, escaped


def check_placed_sparse_arguments(rays_per_triangle, seed, sampling, rows, capacity):
    """The arguments of placed_view_factors_sparse, checked before the library is touched: check_sparse_arguments' rules and a known
    sampling.  Returns the sampling word."""
    check_sparse_arguments(rays_per_triangle, seed, rows, capacity)
    return vf_sampling(sampling)


def placed_view_factors_sparse(accel, rays_per_triangle=10000, seed=0, sampling="uniform", rows=None, capacity=None):
    """The matrix that placed_view_factor_products applies, KEPT, sparse (rc_placed_view_factors_sparse_device): the canonical CSR
    (row_ptr uint64, cols uint32, vals uint32) of rows `rows` = (begin, end) (default: all; end is clamped to P) of M[a, b] = the rays of
    placed primitive a that hit placed primitive b != a first -- placed_view_factor_groups(accel, arange(P), ...) is that matrix dense.
    Rows and columns are placed primitives q = base[i] + l (placed_primitive_bases()); no metadata takes part; the diagonal is empty.  A
    row has at most min(rays_per_triangle, P - 1) entries.  capacity: as view_factors_sparse (None: a counting call, then a filling call).
    The result is a SparseViewFactors with placed = True, n = P, row_offset = rows[0] and the sampling word; the arrays stay on the device
    for view_factor_sparse_products, placed_view_factor_bounces and placed_radiosity.
    THE MATRIX IS A SNAPSHOT of the placement at the time of the call: after the instances move it describes the old placement, and
    building it again is the caller's job."""
    word = check_placed_sparse_arguments(rays_per_triangle, seed, sampling, rows, capacity)
    import torch
    t = _owner(accel)
    P = int(t.placed_primitive_bases()[-1])
    r0, r1 = (0, P) if rows is None else (min(int(rows[0]), P), min(int(rows[1]), P))
    dev = torch.device("cuda", t.device)
    st = torch.cuda.current_stream(dev)
    with torch.cuda.device(dev):
        head = torch.zeros(r1 - r0 + 2, dtype=torch.int64, device=dev)  # row_ptr[rows + 1], then nnz
        nnz_ptr = head.data_ptr() + 8 * (r1 - r0 + 1)
        if capacity is None:
            t.placed_view_factors_sparse_device(head.data_ptr(), None, None, 0, nnz_ptr, rays_per_triangle, seed, word, (r0, r1), st.cuda_stream)
            capacity = int(head[-1].item())
        entries = torch.zeros((2, max(int(capacity), 1)), dtype=torch.int32, device=dev)
        t.placed_view_factors_sparse_device(head.data_ptr(), entries[0].data_ptr() if capacity else None, entries[1].data_ptr() if capacity else None,
                                            int(capacity), nnz_ptr, rays_per_triangle, seed, word, (r0, r1), st.cuda_stream)
        st.synchronize()
        t.wait_for_gpu()  # (reports a traversal stack overflow)
        nnz = int(head[-1].item())
        filled = min(nnz, int(capacity))
        d_row_ptr, d_cols, d_vals = head[:r1 - r0 + 1], entries[0, :filled], entries[1, :filled]
        host = (d_row_ptr.cpu().numpy().view(np.uint64), d_cols.cpu().numpy().view(np.uint32), d_vals.cpu().numpy().view(np.uint32))
    return SparseViewFactors(*host, t, P, r0, int(rays_per_triangle), int(seed), nnz, (d_row_ptr, d_cols, d_vals), sampling=word, placed=True)


def check_placed_bounce_matrix(matrix):
    """The matrix of placed_view_factor_bounces: placed_view_factors_sparse's result with all P rows, complete."""
    if not isinstance(matrix, SparseViewFactors) or not matrix.placed:
        raise ValueError("the matrix must be placed_view_factors_sparse's result: rows and columns must be placed primitives")
    check_bounce_matrix(matrix)


def placed_view_factor_bounces(accel, emission, reflectance, bounces, rays_per_triangle=10000, seed=0, sampling="cosine", stream=None):
    """view_factor_bounces over PLACED primitives: `bounces` steps of

        x_0 = e,    x_{k+1}[q] = min(2^32 - 1, e[q] + (((M x_k)[q] // R) * rho[q] >> 16))

    in integers on the device, with M the matrix of placed_view_factor_products (sources in world space, hits named by (instance,
    primitive)) and R = rays_per_triangle.  With sampling "cosine" (the default) M / R estimates the Lambertian form factors between the
    surface elements, so this is the radiosity equation of an instanced scene; "uniform" shoots the reference's directions.  The same
    seed is used every bounce: the iteration with that one matrix, exact, independent of the order of the device's adds.
    emission: u32 per placed primitive (length P, indexed by q = base[i] + l); reflectance: 0..65536, 16.16 fixed point.  Both are numpy
    integer arrays or device int64 / int32 torch tensors.  Each bounce is zero -> placed_view_factor_products_device (mx only) -> an
    elementwise torch update (placed_bounce_step), all on `stream` with no host wait between bounces.  Returns x: a uint32 numpy array for
    numpy input, else an int64 tensor on the device, ready on `stream`.  ValueError as view_factor_bounces, and for an unknown sampling.
    `accel` may be the MATRIX instead: a placed SparseViewFactors holding all P rows (placed_view_factors_sparse(accel, R, seed, sampling)).
    Then nothing is traced: each bounce is zero -> view_factor_sparse_products_device (mx only) -> the same update (bounce_step_sparse), with
    the matrix's own accel and rays_per_triangle (the three keyword arguments are not read), word for word the retraced result for the
    placement the matrix was built in -- the matrix is a snapshot.  ValueError for a matrix that is not placed, is truncated, does not hold
    all P rows, or whose n differs from len(emission)."""
    matrix = accel if isinstance(accel, SparseViewFactors) else None
    if matrix is not None:
        check_placed_bounce_matrix(matrix)
        accel, rays_per_triangle, seed, sampling = matrix.accel, matrix.rays_per_triangle, matrix.seed, matrix.sampling
    e, rho = check_bounce_arguments(emission, reflectance, bounces, rays_per_triangle)
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < (1 << 64):
        raise ValueError("seed must be an integer in 0..2^64 - 1")
    word = vf_sampling(sampling)
    if matrix is not None and len(e) != matrix.n:
        raise ValueError(f"emission and reflectance must hold one value per placed primitive: {len(e)} values for {matrix.n} placed primitives")
    import torch
    t = _owner(accel)
    P = int(t.placed_primitive_bases()[-1]) if matrix is None else matrix.n
    if len(e) != P:
        raise ValueError(f"emission and reflectance must hold one value per placed primitive: {len(e)} values for {P} placed primitives")
    dev = torch.device("cuda", t.device)
    on_host = not _is_tensor(e)
    ts = stream if isinstance(stream, torch.cuda.Stream) else (torch.cuda.ExternalStream(int(stream), device=dev) if stream else torch.cuda.current_stream(dev))
    with torch.cuda.stream(ts):
        e, rho = (torch.from_numpy(a).to(dev) if not _is_tensor(a) else a.to(dev) for a in (e, rho))
        for a in (e, rho):
            a.record_stream(ts)  # (a caller's tensor, or its int64 copy made on the stream the caller was on)
        x = e.clone()
        x32 = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
        mx = torch.empty(max(P, 1), dtype=torch.int64, device=dev)
        for _ in range(int(bounces)):
            if matrix is None:
                placed_bounce_step(t, e, rho, x, x32, mx, int(rays_per_triangle), int(seed), word, ts.cuda_stream)
            else:
                bounce_step_sparse(matrix, e, rho, x, x32, mx, ts.cuda_stream)
    if on_host:
        ts.synchronize()
        t.wait_for_gpu()  # (reports a traversal stack overflow)
        return x.cpu().numpy().astype(np.uint32)
    return x


def placed_bounce_step(t, e, rho, x, x32, mx, rays_per_triangle, seed, sampling, stream):
    """bounce_step over placed primitives: one bounce of placed_view_factor_bounces on the current torch stream, whose raw handle is
    `stream`.  x (int64, values in u32, length P) is replaced by the next iterate; x32 (int32) and mx (int64) are scratch of the same
    length.  Nothing here waits for the device, so a loop of steps may be captured into a graph (after one eager step)."""
    import torch
    n = x.numel()
    x32[:n].copy_(x.view(torch.int32).view(n, 2)[:, 0])  # the low words: x as u32
    mx.zero_()
    t.placed_view_factor_products_device(x32.data_ptr(), mx.data_ptr(), None, rays_per_triangle, seed, sampling, stream=stream)
    nxt = e + ((torch.div(mx[:n], rays_per_triangle, rounding_mode="floor") * rho) >> 16)  # (M x)[q] < 2^63: non-negative in int64
    x.copy_(nxt.clamp_(max=U32_MAX))


def placed_radiosity(accel, emission, reflectance, bounces, rays_per_triangle=10000, seed=0, sampling="cosine", stream=None, return_scale=False, matrix=None):
    """Radiosity per surface element of an INSTANCED scene by `bounces` steps of B <- E + rho .* (M B) / R in float terms: radiosity() on top
    of placed_view_factor_bounces.  emission: float array >= 0, reflectance: float array in [0, 1), one value per PLACED primitive
    (ValueError otherwise).  With sampling "cosine" (the default) M / R estimates the form factors F_ab, so the fixed point is the
    radiosity equation's; the per-triangle radiosity() is uniform-only.  Quantisation and scaling back: radiosity_scale.
    return_scale: also return the scale (result = integer iterate / scale).
    matrix: the placed SparseViewFactors of placed_view_factors_sparse(accel, rays_per_triangle, seed, sampling) -- the bounces then apply it
    instead of tracing (placed_view_factor_bounces); the result is the same while the instances are where they were when it was built."""
    vf_sampling(sampling)
    scale, e_q, rho_q = radiosity_scale(emission, reflectance)
    if matrix is not None and not isinstance(matrix, SparseViewFactors):
        raise ValueError("matrix must be a SparseViewFactors (placed_view_factors_sparse's result)")
    x = placed_view_factor_bounces(accel if matrix is None else matrix, e_q, rho_q, bounces, rays_per_triangle, seed, sampling, stream)
    b = x.astype(np.float64) / scale
    return (b, scale) if return_scale else b


def multi_prepare(accels):
    """Once per set of devices, before the *_multi calls that are timed (rc_multi_prepare): RCCL and its communicator, the scenes' auxiliary
    streams and staging vectors, a warm-up collective.  Returns the host milliseconds each item took and the number of RCCL ranks the
    accels form (0: replicas on one device, partial results are added on the host)."""
    owners = [_owner(a) for a in accels]
    handles = (C.c_void_p * len(owners))(*[o._h for o in owners])
    ms = np.zeros(4, np.float32)
    check(lib().rc_multi_prepare(handles, len(owners), ptr(ms)))
    ranks = C.c_int(0)
    check(lib().rc_multi_ranks(handles, len(owners), C.byref(ranks)))
    return {"comm_init_ms": float(ms[0]), "streams_and_buffers_ms": float(ms[1]), "warmup_collective_ms": float(ms[2]), "total_ms": float(ms[3]), "rccl_ranks": int(ranks.value)}


def trace_multi(accels, rays, mode="closest", out=None):
    """One host batch of rays on several devices of ONE process (rc_trace_closest_multi / rc_trace_any_multi): `accels` are synced accels
    holding the same scene, one per device; accel g uploads, traces and downloads the g-th contiguous shard of the batch over its own
    PCIe link (rays are independent -- replicas, no collective).  hits[i] is what any one accel's trace gives for rays[i]."""
    owners = [_owner(a) for a in accels]
    rays = _as_rays(rays)
    if out is None:
        hits = np.empty(len(rays), dtype=HIT_DT)
    else:
        if out.dtype != HIT_DT or len(out) != len(rays) or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a contiguous HIT_DT array with one record per ray")
        hits = out
    handles = (C.c_void_p * len(owners))(*[o._h for o in owners])
    fn = lib().rc_trace_closest_multi if mode == "closest" else lib().rc_trace_any_multi
    check(fn(handles, len(owners), ptr(rays), ptr(hits), len(rays)))
    return hits


def get_illumination_multi(accels, viewdir, grid_size=1000):
    """get_illumination with the ray grid cut into one share per device (rc_get_illumination_multi); the partial histograms are added
    on the host.  Same counts as get_illumination."""
    owners = [_owner(a) for a in accels]
    out = np.zeros(owners[0].n_primitives(), dtype=np.float32)
    vd = np.ascontiguousarray(viewdir, dtype=np.float32)
    handles = (C.c_void_p * len(owners))(*[o._h for o in owners])
    check(lib().rc_get_illumination_multi(handles, len(owners), ptr(vd), int(grid_size), ptr(out)))
    return out


def expand_faceviews(positions, position_faces, **attributes):
    """GeometryBasics.expand_faceviews as build_and_append_blas! uses it (src/instanced-bvh.jl:581-590): a mesh whose attributes are
    indexed by their own face arrays (a cube: 8 positions, 6 normals, one metadata value per face) becomes a mesh with ONE index set,
    which is what `add_mesh` / `rc_add_mesh` take.  Every face corner is the tuple of its indices into all attributes; each distinct
    tuple becomes one vertex, numbered in order of first appearance.

    attributes: name=(values, faces) with faces (nf, 3) indices into values, or name=(values, None) for one value per FACE (the
    `face_meta` convention, :595: after expansion it is per vertex).  Returns (positions, faces, {name: per-vertex values})."""
    pf = np.asarray(position_faces, dtype=np.int64).reshape(-1, 3)
    nf = len(pf)
    cols = [pf.reshape(-1)]
    names, values = [], []
    for name, (vals, faces) in attributes.items():
        vals = np.asarray(vals)
        if faces is None:
            if len(vals) != nf:
                raise ValueError(f"{name}: one value per face expected")
            idx = np.repeat(np.arange(nf, dtype=np.int64), 3)
        else:
            idx = np.asarray(faces, dtype=np.int64).reshape(-1)
            if len(idx) != 3 * nf:
                raise ValueError(f"{name}: faces must have one index triple per position face")
        cols.append(idx); names.append(name); values.append(vals)
    corners = np.stack(cols, axis=1)                                  # (3 nf, 1 + n_attributes) index tuples
    uniq, first, inverse = np.unique(corners, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                          # first-appearance order, as GeometryBasics numbers the merged vertices
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    new_faces = rank[np.asarray(inverse).reshape(-1)].reshape(nf, 3).astype(np.uint32)
    tuples = uniq[order]
    out_pos = np.asarray(positions, dtype=np.float32).reshape(-1, 3)[tuples[:, 0]]
    out_attr = {name: vals[tuples[:, k + 1]] for k, (name, vals) in enumerate(zip(names, values))}
    return out_pos, new_faces, out_attr


def TLAS_from_items(items, metadata_fn, device=0):
    """TLAS(items, metadata_fn; backend) (src/instanced-bvh.jl:2276-2324): one BLAS + one identity instance per
    item, instance_id = item index, metadata = metadata_fn(item_idx, face_idx) (1-based); returns the adapted accel."""
    t = TLAS(device)
    for mi, verts in enumerate(items, start=1):
        verts = np.asarray(verts, dtype=np.float32).reshape(-1, 9)
        meta = t.intern_metadata([metadata_fn(mi, fi) for fi in range(1, len(verts) + 1)])  # TMetadata = typeof(metadata_fn(1, 1)), :2281-2282
        b = t.add_geometry(verts, meta)
        ident = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]], dtype=np.float32)
        t.push_instances(b, ident, [mi], inv_transforms=ident)  # identity for both, :2314-2320
    return t.adapt()


def TLAS_from_meshes(meshes, device=0):
    """TLAS(meshes; backend) -> (tlas, handles) (src/instanced-bvh.jl:2361-2378)."""
    if len(meshes) == 0:
        raise RaycoreError(_capi.RC_ERR_INVALID_ARGUMENT, "Cannot create TLAS from empty mesh list")
    t = TLAS(device)
    handles = [t.push(m) for m in meshes]
    t.sync()
    return t, handles
