/*
 * raycore_mi355x.h -- C ABI of the MI355X-native TLAS/BLAS traversal library (libraycore_mi355x.so).
 *
 * This is the drop-in boundary for ONE path of JuliaGeometry/Raycore.jl: the two-level BVH build,
 * closest_hit / any_hit traversal, and the get_illumination / view_factors drivers that sit on it.
 * The reference has no FFI of its own; its plug-in point is the Julia-level AbstractAccel contract
 * (src/Raycore.jl:14-49), already implemented by Raycore.TLAS and the external Lava.HWTLAS.  Each entry
 * point below names the reference function it replaces (paths relative to the reference repo); the
 * Julia `ccall` binding a maintainer would add is shown in INTEGRATION.md and
 * raycore.jl_amd/julia/RaycoreMI355X.jl.
 *
 * Conventions
 *  - Every function returns 0 on success, non-zero on error; rc_last_error() returns the message of the
 *    calling thread's last failure.  No C++ exception crosses this boundary.  The Julia wrapper turns a
 *    non-zero status into ErrorException (test/test_tlas_stress.jl:585-617 expects that type).
 *  - The caller owns every host buffer it passes.  The library owns all device memory behind the opaque
 *    rc_scene handle and frees it in rc_scene_destroy (replaces free!, src/instanced-bvh.jl:383-399).
 *  - Threading.  Mutations (rc_add_*, rc_update_*, rc_delete, rc_sync, rc_set_option, rc_blas4_build, rc_refit_device*) on one scene
 *    must be externally serialised and must not overlap queries.  QUERIES ON A SYNCED SCENE ARE RE-ENTRANT: any number of host threads
 *    may call rc_trace_closest / rc_trace_any (each call stages through its own stream and buffers; a fifth concurrent call waits for a
 *    staging context) and the *_device entry points (rc_trace_*_device, rc_get_illumination_device, rc_view_factors_device,
 *    rc_trace_*4_device and the wavefront stage kernels) at once -- the reference's own drivers call closest_hit on one adapted accel
 *    from Threads.@threads (src/kernels.jl:64,82).  Only the enqueue of a launch is serialised inside the library (microseconds); the
 *    launches overlap on their streams, each with its own work counters and -- per stream -- its own stack spill area.  The other
 *    host-buffer queries (rc_get_illumination, rc_view_factors*, rc_collide_instances, rc_trace_*4) are safe to call concurrently and run
 *    one at a time per scene.  rc_compact_hits_device and rc_collide_instances_device use scene-owned scratch: keep their calls on one
 *    scene on one stream.  rc_last_kernel_ms reports the calling thread's latest launch.  No global mutable state.
 *    rc_update_transforms_device and rc_refit_device_async are mutations too, enqueued on the caller's stream: work enqueued LATER ON THE
 *    SAME STREAM sees the new scene; *_device queries on other streams or threads must be ordered behind them by the caller (events), as
 *    for any mutation; the host-buffer queries wait for them on the host (see rc_refit_device_async).  A captured update / refit holds device addresses that a REBUILDING rc_sync invalidates, like the address
 *    rc_instance_buffer_device returns.
 *  - hipGraph capture: trace / driver launches on a capturing stream are captured (no events, a counter slot of their own that eager
 *    launches never use); the stream must have run one eager launch on the scene before (stack spill area), see INTEGRATION.md.
 *    Entry points that allocate, copy or free (scene create / destroy / sync, the host-buffer queries) may run on any thread while a
 *    capture is open elsewhere in the process, also one in hipStreamCaptureModeGlobal: they set the calling thread's capture interaction
 *    mode to relaxed for their duration and touch only the scene's own streams.  rc_scene_destroy waits for the scene's own streams and
 *    for the launches it recorded on the callers' streams, not for the whole device.
 *  - There is NO CPU fallback: every compute entry point runs hand-written gfx950 HIP kernels and fails
 *    with RC_ERR_NO_DEVICE when no GPU is present.
 *  - Index bases at this boundary are 0-based (C); the host wrappers add 1 where the Julia API is 1-based.
 */
#ifndef RAYCORE_MI355X_H
#define RAYCORE_MI355X_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RC_OK 0
#define RC_ERR_INVALID_ARGUMENT 1
#define RC_ERR_INVALID_HANDLE 2   /* "Invalid handle" / "Handle has been deleted" (src/instanced-bvh.jl:715-716,756-757) */
#define RC_ERR_NO_DEVICE 3
#define RC_ERR_HIP 4
#define RC_ERR_EMPTY_GEOMETRY 5   /* "Geometry has no valid triangles" (src/instanced-bvh.jl:601) */
#define RC_ERR_NOT_SYNCED 6
#define RC_ERR_STACK_OVERFLOW 7
#define RC_ERR_GEOMETRY_CHANGED 8 /* an in-place geometry update met another face count (rc_update_geometry_device_async); reported by rc_wait */

#define RC_INVALID_ID 0xFFFFFFFFu

/* Wire structs: byte-identical to RTRay / RTHitResult (src/rt_transport.jl:10-19, 33-42). */
typedef struct rc_ray {
    float origin_x, origin_y, origin_z, tmin;
    float dir_x, dir_y, dir_z, tmax;
} rc_ray;

/* hit: 1/0.  t: world-ray parameter (direction is NOT renormalised, src/instanced-bvh.jl:1974-1975).
 * primitive_id: 0-based index into the flat Morton-sorted primitive array (all_blas_prims).
 * instance_id: 0-based position in the instance array (Julia closest_hit returns this + 1).
 * instance_custom_index: InstanceDescriptor.instance_id of the hit instance.
 * bary_u/bary_v: Moeller-Trumbore u, v; Julia's bary = ((1-u)-v, u, v) (src/instanced-bvh.jl:2015-2016).
 * Miss: hit=0, t=0, bary 0, primitive_id=instance_id=RC_INVALID_ID (Julia: empty triangle, index 0). */
typedef struct rc_hit {
    uint32_t hit;
    float t;
    uint32_t primitive_id;
    uint32_t instance_custom_index;
    float bary_u, bary_v;
    uint32_t instance_id;
    uint32_t _pad;
} rc_hit;

/* Reference-layout records for introspection / parity checks (rc_export_*). */
typedef struct rc_bvh_node { /* BVHNode2, 60 bytes (src/instanced-bvh.jl:50-63) */
    float aabb0_min[3], aabb0_max[3], aabb1_min[3], aabb1_max[3];
    uint32_t child0, child1, parent;
} rc_bvh_node;
typedef struct rc_instance_desc { /* InstanceDescriptor, 108 bytes (src/instanced-bvh.jl:90-96) */
    uint32_t blas_index; /* 1-based, as stored by the reference */
    uint32_t instance_id;
    float transform[12];     /* Mat3x4f = Vulkan row-major 3x4 (src/instanced-bvh.jl:28-31) */
    float inv_transform[12];
    uint32_t flags;
} rc_instance_desc;
typedef struct rc_blas_desc { /* BLASDescriptor, 32 bytes (src/instanced-bvh.jl:132-136) */
    uint32_t nodes_offset, primitives_offset;
    float root_min[3], root_max[3];
} rc_blas_desc;
typedef struct rc_prim { /* the part of Triangle{UInt32} the path reads (src/triangle_mesh.jl:1-7) */
    float v[9];
    uint32_t meta;
} rc_prim;

typedef struct rc_scene rc_scene; /* opaque; plays the role of the mutable TLAS (src/instanced-bvh.jl:261-310) */

const char* rc_last_error(void);
/* Tracing (the reference's method: docs/src/hw_acceleration.md:198-218 times phases by hand; SURVEY.md section 5 asks for roctx ranges).  Every
 * entry point below is one roctx range named after itself while a marker library (rocprofiler-sdk's roctx, else libroctx64) can be loaded
 * and RC_ROCTX is not "0"; a caller brackets its own phases with these two, so that `rocprofv3 --marker-trace --kernel-trace` attributes
 * dispatches to phases.  Both always succeed (no-ops without a marker library); rc_ranges_enabled: 1 when ranges are being emitted. */
int rc_range_push(const char* name);
int rc_range_pop(void);
int rc_ranges_enabled(void);
/* Number of visible HIP devices (0 when none); never fails. */
int rc_device_count(void);

/* TLAS(backend) (src/instanced-bvh.jl:334-358).  device = HIP device ordinal. */
int rc_scene_create(int device, rc_scene** out);
/* free!(tlas) (src/instanced-bvh.jl:383-399) */
int rc_scene_destroy(rc_scene* scene);

/* build_and_append_blas! minus the GeometryBasics mesh decomposition (src/instanced-bvh.jl:581-608):
 * verts = n x 9 f32 triangle soup, meta = n u32 or NULL (=> face index 1..n, assigned BEFORE the
 * degenerate filter, :595).  Degenerate faces (is_degenerate, src/triangle_mesh.jl:14-17) are dropped,
 * the LBVH is built on the device (build_blas, :1376-1443).  *blas_id receives the 0-based geometry id; like the reference's
 * blas_index it is renumbered when an rc_sync after rc_delete drops unreferenced geometries (compact_instances!, :996-1065), so
 * use it right away (rc_add_instances, rc_blas4_build) or re-derive it from rc_get_instances(...).blas_index - 1. */
int rc_add_blas(rc_scene* scene, const float* verts, const uint32_t* meta, uint32_t n, uint32_t* blas_id);
/* Same with the triangle soup already in device memory (the reference builds BLASes "directly on the backend",
 * src/instanced-bvh.jl:16-21): no host staging; filter, sort and tree construction all run on the GPU. */
int rc_add_blas_device(rc_scene* scene, const float* d_verts, const uint32_t* d_meta, uint32_t n, uint32_t* blas_id);

/* push!(tlas, mesh, transforms; instance_ids) once the geometry exists (src/instanced-bvh.jl:639-676,
 * append_instances_with_handle! :612-623): m instances of blas_id.  xforms = m x 12 f32 (Mat3x4f bytes)
 * or NULL for identity; instance_ids = m u32 or NULL for 0.  *handle receives the TLASHandle id (>= 1). */
int rc_add_instances(rc_scene* scene, uint32_t blas_id, const float* xforms, const uint32_t* instance_ids,
                     uint32_t m, uint32_t* handle);
/* Same, but the caller supplies the inverse transforms too (the InstanceDescriptor(..., transform,
 * inv_transform, ...) constructor used with build_tlas, src/instanced-bvh.jl:90-102, 1605). */
int rc_add_instances_with_inverse(rc_scene* scene, uint32_t blas_id, const float* xforms, const float* inv_xforms,
                                  const uint32_t* instance_ids, uint32_t m, uint32_t* handle);

/* update_transform! / update_transforms! (src/instanced-bvh.jl:755-797): m must equal the handle's
 * instance count; marks the scene transforms-dirty (refit on the next rc_sync). */
int rc_update_transforms(rc_scene* scene, uint32_t handle, const float* xforms, uint32_t m);
/* update!(tlas, handle, new_geometry) (src/instanced-bvh.jl:808-857): replace the BLAS the handle uses. */
int rc_update_geometry(rc_scene* scene, uint32_t handle, const float* verts, const uint32_t* meta, uint32_t n);
/* delete!(tlas, handle) (src/instanced-bvh.jl:690-699): *deleted = 1 if it was live, 0 otherwise (idempotent). */
int rc_delete(rc_scene* scene, uint32_t handle, int* deleted);
/* is_valid (src/instanced-bvh.jl:524-526); n_instances(tlas, handle) (:533-537) */
int rc_is_valid(rc_scene* scene, uint32_t handle, int* valid);
int rc_handle_instance_count(rc_scene* scene, uint32_t handle, uint32_t* count);
/* get_instances(tlas, handle) (src/instanced-bvh.jl:732-738): copies the handle's descriptors. */
int rc_get_instances(rc_scene* scene, uint32_t handle, rc_instance_desc* out, uint32_t capacity, uint32_t* count);

/* sync!(tlas) (src/instanced-bvh.jl:894-921): dirty => compact + rebuild TLAS + flat BLAS arrays;
 * only transforms dirty => refit in place (refit_tlas!, :2197-2222); clean => no-op without a device
 * synchronise.  *action (optional) receives 0 = no-op, 1 = refit, 2 = rebuild. */
int rc_sync(rc_scene* scene, int* action);

/* n_instances(tlas) (live, :2391-2398), length(tlas.instances) (n_total_instances, :544), n_geometries (:2405),
 * number of flat primitives / TLAS nodes / BLAS nodes after the last sync. */
int rc_counts(rc_scene* scene, uint32_t* n_live_instances, uint32_t* n_total_instances, uint32_t* n_geometries,
              uint32_t* n_prims, uint32_t* n_tlas_nodes, uint32_t* n_blas_nodes);
/* world_bound(tlas) (src/instanced-bvh.jl:2147-2149): out = {min xyz, max xyz}.  After rc_refit_device_async the call first waits for
 * the refit and reads the root box back (see there). */
int rc_world_bound(rc_scene* scene, float out[6]);
/* wait_for_gpu! (src/instanced-bvh.jl:2418-2421).  Also the place where asynchronous launches (the *_device entry points) report a
 * traversal-stack overflow (RC_ERR_STACK_OVERFLOW): the host-buffer entry points check after every call, the device ones cannot. */
int rc_wait(rc_scene* scene);

/* Reference-layout copies of the synced StaticTLAS arrays (src/instanced-bvh.jl:155-168).  Pass NULL
 * buffers to query counts only. */
int rc_export_tlas_nodes(rc_scene* scene, rc_bvh_node* out, uint32_t capacity, uint32_t* count);
int rc_export_blas_nodes(rc_scene* scene, rc_bvh_node* out, uint32_t capacity, uint32_t* count);
int rc_export_instances(rc_scene* scene, rc_instance_desc* out, uint32_t capacity, uint32_t* count);
int rc_export_blas_descs(rc_scene* scene, rc_blas_desc* out, uint32_t capacity, uint32_t* count);
int rc_export_prims(rc_scene* scene, rc_prim* out, uint32_t capacity, uint32_t* count);

/* closest_hit / any_hit over a batch (src/instanced-bvh.jl:1902-2024, 2034-2140; batch shape =
 * trace_rays, ext/RaycoreMakieExt.jl:81-87, and Lava.trace_closest_hits!, docs/src/hw_acceleration.md:141-146).
 * Host-buffer form: copies rays in, hits out. */
int rc_trace_closest(rc_scene* scene, const rc_ray* rays, rc_hit* hits, uint64_t n);
int rc_trace_any(rc_scene* scene, const rc_ray* rays, rc_hit* hits, uint64_t n);
/* Device-buffer form: d_rays / d_hits are device pointers on the scene's device; the launch is enqueued
 * on `stream` (a hipStream_t, NULL = the null stream) and is asynchronous.  Launches on different streams
 * may be in flight together (each has its own work counters); for batches of about a million rays that is
 * worth 1.4x: the end of a launch -- waves waiting for their longest rays -- leaves most of the machine to
 * the next one (mid-size batches). */
int rc_trace_closest_device(rc_scene* scene, const rc_ray* d_rays, rc_hit* d_hits, uint64_t n, void* stream);
int rc_trace_any_device(rc_scene* scene, const rc_ray* d_rays, rc_hit* d_hits, uint64_t n, void* stream);
/* Several INDEPENDENT device batches in one call: d_rays / d_hits / n are HOST arrays of n_batches device pointers / counts.  The
 * reference's batch API takes one ray array per call (trace_rays(tlas, rays), ext/RaycoreMakieExt.jl:81-87; Lava.trace_closest_hits!,
 * docs/src/hw_acceleration.md:141-146), which gives a caller holding several mid-size batches -- tiles of a frame, the queues of a
 * wavefront tracer (docs/src/wavefront-renderer.jl:260-512) -- no way to say that they do not depend on each other.  Here the batches
 * go round-robin onto four auxiliary streams of the scene, forked from `stream` and joined back into it with events: to the caller the
 * call is one asynchronous operation on `stream`, and each batch's hits are exactly what rc_trace_*_device gives for it.  Worth ~1.3x
 * for batches of about a million rays (the tail of one launch overlaps the bulk of the next); nothing for batches that fill the machine
 * for long.  Capture-safe: on a capturing `stream` the auxiliary streams join the capture through the fork event and are all joined back
 * before the call returns (also when a launch fails); each captured launch holds a capture slot like a single captured launch does. */
int rc_trace_closest_device_batches(rc_scene* scene, const rc_ray* const* d_rays, rc_hit* const* d_hits, const uint64_t* n, int n_batches, void* stream);
int rc_trace_any_device_batches(rc_scene* scene, const rc_ray* const* d_rays, rc_hit* const* d_hits, const uint64_t* n, int n_batches, void* stream);

/* Kernel selection for the trace entry points (tuning / A-B measurement).  The default is the tuned
 * kernel; every variant returns identical results.  Names: "kernel" (clamped to -1..6: -1 auto, 0 one ray per lane,
 * 1 persistent waves, 3 phased, 5 phased with the top level in LDS -- scenes of at most 256 instances, else 3 runs --, 6 phased with the
 * tops of the TLAS and of a single BLAS in LDS; 2 and 4 are retired ids kept as aliases: setting 2 stores 3, setting 4 stores 5, and
 * rc_get_option returns what was stored),
 * "blocks_per_cu", "refill", "sched_thr", "pool", "claim_shards" (scheduling knobs of the
 * persistent kernels), "lds_stack" (retired: still accepted, without effect; reads back 24, the LDS depth of every 256-thread kernel),
 * "taper" (guided claim sizes: towards the end of the claim order a 128-ray chunk is dealt in halves, quarters,
 * eighths; in eighths of (part size x waves) still to hand out per piece, default 12, 0 = whole chunks only), "cost_order" (1 = the
 * chunks that held long-lived rays in earlier launches of the same BATCH are claimed first: the batch is recognised on the device by sample
 * rays among up to four remembered per launch shape -- chunk count, mode, stream --, records its chunk costs in its launches 2-4 (never the first: a batch that does not come back pays nothing) and
 * then in one launch of eight; default 1), "order_close_repeats" (1 = a launch with a remembered batch's ray origins and nearly its directions -- jittered re-renders of a still view -- continues that batch's history like an exact repeat; 0 = exact repeats only; default 1),
 * "cost_thr" (its initial reporting threshold), "entry_cull" (1 = an instance whose conservative sphere the ray's segment misses is
 * not entered: the reference's traversal of it would test no triangle; 0 = off, 1 = closest_hit and the drivers (default),
 * 2 = any_hit batches too), "vf_chunk_bytes" (device block per row chunk of the host-matrix view factors), "illum_scratch_bytes" (rc_get_illumination_dirs_device: histogram scratch per launch, which bounds its group of directions; default 256 MiB), "placed_copy_bytes" (rc_placed_view_factor_products_device: d_mtx is counted into private copies while 16 copies of P u64 fit, added straight onto the caller's words above; 0 = always straight; default 256 MiB; changes no result), "vf_first_touch" (ROWS on several devices: each device's
 * host thread joins the device's NUMA node and faults in its own row block; default 1), "release_captures" (set to 1 when the hipGraphs that
 * captured launches of this scene have been destroyed: frees their stack spill regions and counter slots, 16 per scene; get: how many are held),
 * "blas_top" (1 = a scene with a single BLAS keeps that BLAS's top internal
 * nodes in LDS; takes effect at the next structural rc_sync), "tlas_rebuild_fused" (1 = rc_rebuild_tlas_device_async rebuilds scenes of
 * 2 .. 256 instances with its single-workgroup kernel, 0 = always with the chain of build kernels), "onesweep_min" (key count from which
 * the builds sort with Onesweep radix passes instead of a merge sort), "stats" (dev counters),
 * "timeline_ptr" (dev: device address of 8 x u64 per wave that kernel 5 fills with its waves' event
 * times, tools/archive/timeline_probe.py; 0 = off).
 * None of them changes a result: every variant and every claim order returns identical hits.
 * Read-only: "n_cus", "blas_top_k", "tlas_top_k", "claim_drift", "stat0".."statf", "stat16".."stat23". */
int rc_set_option(rc_scene* scene, const char* name, int64_t value);
int rc_get_option(rc_scene* scene, const char* name, int64_t* value);

/* generate_ray_grid as used by hits_from_grid (src/kernels.jl:10-72): grid*grid rays written to the
 * device buffer d_rays (column-major (i-1) + grid*(j-1)), direction = normalize(viewdir). */
int rc_generate_ray_grid_device(rc_scene* scene, const float viewdir[3], uint32_t grid, rc_ray* d_rays, void* stream);
/* get_illumination(tlas, viewdir; grid_size) (src/kernels.jl:112-124): out_counts = n_prims f32 (host). */
int rc_get_illumination(rc_scene* scene, const float viewdir[3], uint32_t grid, float* out_counts);
/* Rays [ray_begin, ray_end) of the grid only, accumulated into a device histogram (n_prims f32) --
 * the shard unit for multi-GPU runs.  The kernel counts into private copies of the histogram (a few large, well-lit
 * triangles take most of the hits) and adds them to d_counts ATOMICALLY at the end of the launch: shards add up whether they are enqueued
 * on one stream or run concurrently on several.  A count saturates at 2^24 like the reference's f32 `+= 1`. */
int rc_get_illumination_device(rc_scene* scene, const float viewdir[3], uint32_t grid, uint64_t ray_begin,
                               uint64_t ray_end, float* d_counts, void* stream);

/* view_factors(tlas; rays_per_triangle) (src/kernels.jl:74-104) with the unseeded task-local RNG replaced
 * by Philox4x32-10: key = seed, counter = (ray_idx, src_prim_index, 0, 0) -> (r1, r2, xi1, xi2), so a result
 * does not depend on how the work is sharded.  Shoots rays [ray_begin, ray_end) of source primitives
 * [src_begin, src_end) and ACCUMULATES into d_matrix (device, u32): element (src_meta-1, hit_meta-1) lives
 * at (row - row_offset)*row_stride + (hit_meta-1)*col_stride with row = src_meta-1, or -- with
 * RC_VF_ROW_BY_PRIMITIVE in flags -- row = the source's index in the flat (Morton-sorted) primitive array,
 * which is what makes a contiguous source range own a contiguous row block.  Julia's column-major N x N
 * Matrix is row_stride=1, col_stride=N, row_offset=0, flags=0; a row-sharded block is row_stride=N,
 * col_stride=1, row_offset=src_begin, flags=RC_VF_ROW_BY_PRIMITIVE (the gatherer then permutes rows by
 * metadata once).  With RC_VF_SOURCES_BY_METADATA, [src_begin, src_end) are positions in the primitives' order
 * by ascending metadata (ties by flat index) and row = that position: when the metadata are a permutation of
 * 1..N -- the view-factor convention, src/kernels.jl:85 -- position p IS matrix row src_meta-1, so a contiguous
 * source range owns a contiguous block of FINAL rows and a multi-GPU gather / reduce needs no row permutation
 * and no second N x N buffer.
 * RC_VF_ROW_BY_METADATA_VALUE (with RC_VF_SOURCES_BY_METADATA): sources are addressed by position in the metadata order, but
 * row = src_meta-1 as without flags -- for metadata that are not a permutation of 1..N (duplicates share a row, gaps leave rows
 * empty) a range of matrix rows is still a contiguous range of positions, which is how the host-matrix entry points cut the job
 * into row chunks and row blocks. */
#define RC_VF_ROW_BY_PRIMITIVE 1u
#define RC_VF_SOURCES_BY_METADATA 2u
#define RC_VF_ROW_BY_METADATA_VALUE 4u
int rc_view_factors_device(rc_scene* scene, uint32_t rays_per_triangle, uint64_t seed, uint32_t src_begin,
                           uint32_t src_end, uint32_t ray_begin, uint32_t ray_end, uint32_t* d_matrix,
                           uint64_t row_stride, uint64_t col_stride, uint32_t row_offset, uint32_t flags, void* stream);
/* Whole job into a host N x N column-major matrix (the Julia return value, src/kernels.jl:74-78).  The matrix never exists on the
 * device: row chunks (192 MB blocks) are traced on alternating streams while the finished ones travel to out_matrix as 2-D copies,
 * so the call lasts about as long as N*N*4 bytes need over the PCIe link (C5: 10 GB, ~0.18 s; the tracing, 41 ms, hides inside).
 * out_matrix may be pageable or registered (rc_host_register); every element is written. */
int rc_view_factors(rc_scene* scene, uint32_t rays_per_triangle, uint64_t seed, uint32_t* out_matrix);
/* Matrix rows [row_begin, row_end) only, into a host column-major matrix with leading dimension ld >= N (element (r, c) at
 * out_matrix[r + ld*c]): the unit of a multi-PROCESS run -- every rank maps the same shared-memory matrix and brings its own row
 * block home over its own PCIe link (raycore.jl_amd/distributed.py, mode "rows_host"). */
int rc_view_factors_rows_host(rc_scene* scene, uint32_t rays_per_triangle, uint64_t seed, uint32_t row_begin, uint32_t row_end,
                              uint32_t* out_matrix, uint64_t ld);
/* The same job on several devices of one process: scenes[g] is a synced scene on device g's ordinal, all built from the same
 * geometry (view_factors shards across the GPUs of a node).
 *   RC_VF_MODE_ROWS: scene g traces matrix rows [g N / G, (g+1) N / G) and copies its chunks straight into out_matrix -- G PCIe links
 *     in parallel, nothing crosses xGMI, no collective.  Several scenes may share a device.
 *   RC_VF_MODE_RAYS: scene g shoots ray indices [g R / G, (g+1) R / G) of every source into a full device accumulator; row chunks are
 *     summed into scenes[0]'s device with RCCL (ncclReduce, ncclUint32, over xGMI; librccl.so is loaded on first use) while the next
 *     chunk is traced, and leave from there.  Needs distinct devices.
 * Both give the matrix rc_view_factors gives, bit for bit (Philox is keyed by ray index and source primitive). */
#define RC_VF_MODE_ROWS 0
#define RC_VF_MODE_RAYS 1
int rc_view_factors_multi(rc_scene* const* scenes, int n_scenes, uint32_t rays_per_triangle, uint64_t seed, uint32_t* out_matrix, int mode);
/* The per-triangle TOTALS of the view-factor job, without the matrix: out_received[j] = sum_i result[i, j] (the column sums -- how many
 * rays ARRIVE at the triangles with metadata j+1; the quantity the reference's users read off the matrix,
 * docs/src/viewfactors_content.md:62-68: sum(view(viewf_matrix, :, i))) and out_emitted[i] = sum_j result[i, j] (the row sums: counted
 * rays that LEFT triangles with metadata i+1).  Same rays (Philox keyed by seed, ray index, source primitive) and the same counting
 * rule as view_factors! (src/kernels.jl:93-97), so the vectors equal the sums of rc_view_factors' matrix exactly; u64, n_prims each;
 * either pointer may be NULL.  No N x N array exists anywhere: the call costs the tracing (C5: ~40 ms), not 10 GB over PCIe.
 * _device: rays [ray_begin, ray_end) of the sources with flat primitive indices [src_begin, src_end), ACCUMULATED into device vectors
 *   (the shard unit of a multi-process run: torch.distributed reduce of 2 N int64).  The kernel counts into private copies of the received
 *   vector (a few large triangles receive most rays of a closed scene, and per-ray atomics onto a few hundred cache lines run at half the
 *   rate of scattered ones) and adds them to d_received atomically at the end of the launch; d_emitted takes one atomic per wave and source:
 *   shards accumulate correctly on one stream or concurrently on several.
 * _multi: scenes[g] = synced copies of one scene on DISTINCT devices; device g shoots ray indices [g R / G, (g+1) R / G) of every
 *   source and ONE ncclReduce (ncclUint64, sum, 2 N elements, over xGMI; librccl.so loaded on first use) brings the vectors to
 *   scenes[0]'s device -- "rays sharded across the GPUs with an RCCL reduce of the per-triangle accumulators" (SURVEY.md 8e).  Scenes
 *   that share a device are replicas without a communicator: their partial vectors are added on the host. */
int rc_view_factor_totals(rc_scene* scene, uint32_t rays_per_triangle, uint64_t seed, uint64_t* out_received, uint64_t* out_emitted);
int rc_view_factor_totals_device(rc_scene* scene, uint32_t rays_per_triangle, uint64_t seed, uint32_t src_begin, uint32_t src_end,
                                 uint32_t ray_begin, uint32_t ray_end, uint64_t* d_received, uint64_t* d_emitted, void* stream);
int rc_view_factor_totals_multi(rc_scene* const* scenes, int n_scenes, uint32_t rays_per_triangle, uint64_t seed, uint64_t* out_received,
                                uint64_t* out_emitted);
/* Everything the *_multi entry points need ONCE per set of devices, taken out of the calls that are timed: librccl.so and
 * the communicator over the scenes' devices (ncclCommInitAll, when they are distinct), each scene's auxiliary streams, its staging vectors
 * for the totals, and a first tiny collective that makes RCCL set up its xGMI connections.  Optional -- the *_multi calls do the same
 * lazily -- and idempotent.  out_ms (may be NULL) = 4 floats of host wall time: [0] load RCCL + create the communicator, [1] streams and
 * staging buffers, [2] the warm-up collective (0 without a communicator), [3] total.  rc_multi_ranks: how many RCCL ranks the scenes form
 * (0 when they share a device: replicas, partial results added on the host). */
int rc_multi_prepare(rc_scene* const* scenes, int n_scenes, float* out_ms);
int rc_multi_ranks(rc_scene* const* scenes, int n_scenes, int* out_ranks);
/* closest_hit / any_hit over one HOST batch on several devices of one process (rays are independent -- replicas of the
 * scene, contiguous ray shards, no collective): scenes[g] is a synced copy of the same scene on device g; shard g is uploaded, traced
 * and downloaded by device g over its own PCIe link, which is what bounds a host-to-host batch (64 bytes per ray).  hits[i] is what
 * rc_trace_closest / rc_trace_any on any one of the scenes gives for rays[i]. */
int rc_trace_closest_multi(rc_scene* const* scenes, int n_scenes, const rc_ray* rays, rc_hit* hits, uint64_t n);
int rc_trace_any_multi(rc_scene* const* scenes, int n_scenes, const rc_ray* rays, rc_hit* hits, uint64_t n);
/* get_illumination on several devices: device g traces its share of the grid's rays into its own histogram; the n_prims-long partial
 * histograms are added on the host (a count stops at 2^24 like the reference's f32 `+= 1`).  Same result as rc_get_illumination. */
int rc_get_illumination_multi(rc_scene* const* scenes, int n_scenes, const float viewdir[3], uint32_t grid, float* out_counts);
/* The rays view_factors shoots for one source primitive (ray indices [ray_begin, ray_begin + n_rays)),
 * written to a device buffer: the body of the reference's inner loop up to the Ray constructor
 * (src/kernels.jl:89-92), exposed so ray generation can be checked on its own. */
int rc_view_factor_rays_device(rc_scene* scene, uint64_t seed, uint32_t src_prim, uint32_t ray_begin, uint32_t n_rays,
                               rc_ray* d_rays, void* stream);

/* Wavefront stages next to the trace (the reference's fastest renderer is a wavefront pipeline around closest_hit /
 * any_hit, docs/src/wavefront-renderer.jl:260-362).  All buffers are device pointers; slot i belongs to ray i.
 * rc_hit_points_device: hit_point = ray.o + ray.d * t (:302) and the geometric world-space normal of the hit primitive
 * (normalize(cross(v1-v0, v2-v0)) through the instance's inverse-transpose, flipped to face the ray origin); zeros on a
 * miss.  d_points / d_normals: n x 3 f32, d_normals may be NULL.
 * rc_shadow_rays_device: generate_shadow_rays! for one point light (:288-333): origin = hit_point + normal * bias,
 * direction = normalize(light - origin), t_max = distance; misses get the reference's dummy ray (d = (0,0,1), t_max = 0).
 * The output feeds rc_trace_any_device unchanged. */
int rc_hit_points_device(rc_scene* scene, const rc_ray* d_rays, const rc_hit* d_hits, uint64_t n, float* d_points,
                         float* d_normals, void* stream);
int rc_shadow_rays_device(rc_scene* scene, const rc_ray* d_rays, const rc_hit* d_hits, uint64_t n, const float light[3],
                          float bias, rc_ray* d_shadow_rays, void* stream);

/* Shadow visibility of all hits x all lights in ONE traversal launch: generate_shadow_rays! (docs/src/wavefront-renderer.jl:279-333,
 * slot (idx-1)*NLights + light_idx) and test_shadow_rays! (:340-362) fused, producing the `visible` Bool that shade_primary_hits!
 * reads (:395-416).  d_rays / d_hits: the closest-hit stage's n rays and hit records, slot i belongs to ray i as for
 * rc_shadow_rays_device.  d_lights: a DEVICE array of n_lights x 3 f32 point-light positions, read when the KERNEL RUNS, not when the call
 * is made (the convention of rc_update_transforms_device): a captured call follows lights that move between replays.
 * d_visible: n x n_lights bytes; byte i * n_lights + l is the reference's shadow_result_queue[(idx-1)*NLights + light_idx].visible.
 * Identity with the composed path, exact, no tolerance:
 * d_visible[i * n_lights + l] == (d_hits[i].hit && shadow_ray(i, l).t_max > 0 && !any_hit(shadow_ray(i, l)).hit),
 * where shadow_ray(i, l) is bit for bit the ray rc_shadow_rays_device(..., light_l, bias, ...) writes for slot i (the same device
 * function makes both) and any_hit is what rc_trace_any_device reports for it.  The middle term is the reference's gate
 * (`ray.t_max > 0 ? !any_hit(...) : false`, :353-358): a shadow ray whose t_max is 0 (the light sits on the shadow origin) or NaN (a hit
 * with NaN t, or a NaN normal out of a singular instance transform) is not visible, whatever an any_hit of it would report.  The composed
 * path's caller holds the shadow rays and applies the gate there; here the ray is never stored, so the kernel does.  A slot whose primary
 * ray missed gets 0 for every light; it and a gated item cost no traversal: their work item is the bounce stage's dead ray (t_max = -1,
 * see rc_bounce_rays_device).
 * One persistent any_hit launch over the n * n_lights (hit, light) items, item i * n_lights + l, so neighbouring lanes share a hit's
 * records; the shadow rays are generated when a lane takes an item and are never stored: neither the L x n x 32 B of shadow rays nor the
 * L x n x 32 B of any_hit records of the composed path exist.  The items are claimed in natural order (no batch recognition: the rays are
 * generated); the entry cull follows rc_trace_any_device (off unless option "entry_cull" is 2).
 * No allocation, copy, event or host synchronisation and no scene-owned scratch: re-entrant across streams like the other *_device
 * queries, and captured on a capturing stream under the rules of the trace / driver launches (one capture slot; the stream must have run
 * the call eagerly before).  A stack overflow is reported by rc_wait like any device launch's.  After an asynchronous refit / rebuild /
 * geometry update on the same stream the call sees the new scene, like a trace.  n == 0 or n_lights == 0: succeeds, nothing is enqueued.
 * Errors, before anything is enqueued: RC_ERR_INVALID_ARGUMENT (NULL scene; NULL d_rays, d_hits, d_lights or d_visible while there is
 * work; n * n_lights >= 2^32), RC_ERR_NOT_SYNCED (never synced, or pending mutations / transform updates without their refit).
 * Measured against the composed path (L x (rc_shadow_rays_device + rc_trace_any_device)) in docs/EXPERIMENTS.md, "Shadow visibility". */
int rc_shadow_visibility_device(rc_scene* scene, const rc_ray* d_rays, const rc_hit* d_hits, uint64_t n, const float* d_lights,
                                uint32_t n_lights, float bias, uint8_t* d_visible, void* stream);

/* Soft shadows: every light a small AREA light, `samples` shadow rays per (hit, light), the visible ones counted.  This is
 * compute_light(...; shadow_samples) of the reference's tutorial (docs/src/raytracing-core.jl:58-99; raytracing_tutorial_content.md,
 * "Part 6: Soft Shadows"), run for every light as compute_multi_light does (:119-129): the caller divides a count by `samples` to get the
 * reference's shadow_factor (:94).
 * d_rays / d_hits: the closest-hit stage's n rays and hit records.  d_lights: n_lights x 3 f32 positions, d_radii: n_lights f32 radii
 * (the tutorial's light_radius, :69); both DEVICE arrays read when the KERNEL RUNS, so a captured call follows lights that move or
 * resize between replays.  d_path_in (may be NULL) / path_base: the path of slot i is path_base + (d_path_in ? d_path_in[i] : i), exactly
 * as in rc_bounce_rays_device: a compacted, chunked or sharded queue draws the same samples for the same path.
 * The sampled target of (i, l, s) restates :61-81, every expression evaluated left to right in f32 with no contraction:
 *   p = the hit point of slot i (rc_hit_points_device's);  lv = light_l - p;  light_dir = lv / sqrt(dot(lv, lv))
 *   samples == 1: target = light_l; no random number is drawn (:74-81)
 *   samples  > 1: off_k = (r_k * 2 - 1) * radius_l (k = 0, 1, 2);  off = off - light_dir * dot(off, light_dir);  target = light_l + off
 * with dot(a, b) = (a1 b1 + a2 b2) + a3 b3.  The unseeded rand(Vec3f) (:76) is replaced by Philox4x32-10, counter layout
 *   (lo32 path, hi32 path, s | depth << 16, 0x53460000 | l), key = (lo32 seed, hi32 seed);
 * r0, r1, r2 = its first three words as 24-bit floats in [0, 1): (word >> 8) * 2^-24, the conversion of rc_bounce_rays_device.
 * ray(i, l, s) is then rc_shadow_rays_device's ray toward the target: origin = hit point + normal * bias, direction = normalize(target -
 * origin), t_max = the distance to the target.  That is the wavefront renderer's convention (docs/src/wavefront-renderer.jl:288-333), which
 * this library already ships -- NOT the tutorial's t_max = Inf followed by `hit_dist >= shadow_dist` (:87-90): any_hit returns the first hit
 * FOUND, not the nearest, so with an unbounded ray a first-found hit beyond the light would decide visibility.
 *
 * rc_soft_shadow_rays_device, the composed stage: writes n * n_lights * samples rays, ray(i, l, s) at slot (i * n_lights + l) * samples + s;
 * a slot whose primary ray missed gets rc_shadow_rays_device's dummy ray (d = (0,0,1), t_max = 0).  The output feeds rc_trace_any_device
 * unchanged.
 * rc_soft_shadow_visibility_device, the fused driver: one persistent any_hit launch over all (hit, light, sample) items, the rays generated
 * when a lane takes an item and never stored.  d_count: n x n_lights u32.  Identity with the composed path, exact, no tolerance:
 *   d_count[i * n_lights + l] += sum over s of (d_hits[i].hit && ray(i, l, s).t_max > 0 && !any_hit(ray(i, l, s)).hit),
 * where ray(i, l, s) is bit for bit what rc_soft_shadow_rays_device writes (the same device function makes both) and any_hit is what
 * rc_trace_any_device reports for it.  The middle term is the gate of rc_shadow_visibility_device: a t_max of 0 or NaN (a NaN t or
 * normal; with samples > 1 also a light that sits exactly on the hit point, whose light_dir and target are NaN) is not visible; it and a
 * missed primary ray cost no traversal.  With samples == 1 no light_dir is computed: a light on the hit point then gives the hard
 * shadow's ray of length |normal * bias| > 0, which is traced -- for that degenerate light a pair's result differs between S = 1 and S > 1.
 * samples == 1: target == light, so the increment equals rc_shadow_visibility_device's byte for the same arguments.
 * The call ACCUMULATES into d_count (the convention of rc_get_illumination_device and rc_view_factors_device): the caller zeroes it, and
 * progressive accumulation over calls with different `seed` or `depth` is legal.  Each visible sample is one relaxed device-scope u32
 * atomic add; integer adds are exact in any order, so the counts are reproducible.  Items are claimed in natural order; the entry cull
 * follows rc_trace_any_device (off unless option "entry_cull" is 2).
 * No allocation, copy, event, memset, host synchronisation or scene-owned scratch: re-entrant across streams, and captured on a capturing
 * stream under the rules of the other driver launches (one capture slot; the stream must have run the call eagerly before).  A stack
 * overflow is reported by rc_wait.  n == 0, n_lights == 0 or samples == 0: succeeds, nothing is enqueued.
 * Errors, all before anything is enqueued: RC_ERR_INVALID_ARGUMENT (NULL scene, checked first and with or without a device; NULL d_rays,
 * d_hits, d_lights, d_radii or output while there is work; n * n_lights * samples >= 2^32; samples >= 65536, depth >= 65536 or
 * n_lights >= 65536), RC_ERR_NOT_SYNCED (the rules of rc_shadow_visibility_device).
 * Measured against the composed path in docs/EXPERIMENTS.md, "Soft shadows". */
int rc_soft_shadow_rays_device(rc_scene* scene, const rc_ray* d_rays, const rc_hit* d_hits, uint64_t n, const float* d_lights,
                               const float* d_radii, uint32_t n_lights, uint32_t samples, uint64_t seed, uint32_t depth,
                               const uint32_t* d_path_in, uint64_t path_base, float bias, rc_ray* d_shadow_rays, void* stream);
int rc_soft_shadow_visibility_device(rc_scene* scene, const rc_ray* d_rays, const rc_hit* d_hits, uint64_t n, const float* d_lights,
                                     const float* d_radii, uint32_t n_lights, uint32_t samples, uint64_t seed, uint32_t depth,
                                     const uint32_t* d_path_in, uint64_t path_base, float bias, uint32_t* d_count, void* stream);

/* ---- BVH4 (src/bvh4.jl; exported by the reference as BVHNode4 / BLAS4 / build_blas4 / closest_hit4 / any_hit4).
 * BLAS-level only, as in the reference: rays are traced in the geometry's own space, no instances.
 * rc_bvh4_node = BVHNode4, 120 bytes (src/bvh4.jl:40-69): interior nodes hold 1-based BVH4 child indices, a leaf
 * (child_count == 0) holds the 1-based index of its triangle in the BLAS's Morton-sorted primitive array in child[0]. */
typedef struct rc_bvh4_node {
    uint32_t child[4];
    float aabb[4][2][3]; /* aabbK_min, aabbK_max */
    uint32_t parent;
    uint8_t child_count, primitive_count, _pad1, _pad2;
} rc_bvh4_node;
/* build_blas4 (src/bvh4.jl:511-522) for geometry blas_id (from rc_add_blas*): collapses its binary LBVH into BVHNode4s on
 * the device (collapse_bvh2_to_bvh4 :314-497, same node numbering).  *n_nodes (optional) receives the node count. */
int rc_blas4_build(rc_scene* scene, uint32_t blas_id, uint32_t* n_nodes);
/* Copies the BLAS4's nodes out in the reference layout (count query when out == NULL). */
int rc_export_blas4_nodes(rc_scene* scene, uint32_t blas_id, rc_bvh4_node* out, uint32_t capacity, uint32_t* count);
/* closest_hit4 (src/bvh4.jl:606-689) / any_hit4 (:696-766) over a host ray batch.  Both ignore rc_ray.tmin (the
 * reference starts from t_min = 0, :610/:700).  rc_hit: primitive_id = 0-based index into the BLAS's sorted primitives,
 * instance_id = RC_INVALID_ID, instance_custom_index = 0; miss as rc_trace_closest.  A geometry without a BLAS4 (never built, replaced by
 * rc_update_geometry*, or updated in place by rc_update_geometry_device_async / rc_update_mesh_vertices_device_async since): RC_ERR_NOT_SYNCED,
 * from these, their _device forms and rc_export_blas4_nodes, until rc_blas4_build.  The BLAS4 entry points look at the geometry alone:
 * pending mutations of the scene do not refuse them. */
int rc_trace_closest4(rc_scene* scene, uint32_t blas_id, const rc_ray* rays, rc_hit* hits, uint64_t n);
int rc_trace_any4(rc_scene* scene, uint32_t blas_id, const rc_ray* rays, rc_hit* hits, uint64_t n);
/* Same on device buffers, enqueued on `stream` (NULL = default stream), no host synchronisation. */
int rc_trace_closest4_device(rc_scene* scene, uint32_t blas_id, const rc_ray* d_rays, rc_hit* d_hits, uint64_t n, void* stream);
int rc_trace_any4_device(rc_scene* scene, uint32_t blas_id, const rc_ray* d_rays, rc_hit* d_hits, uint64_t n, void* stream);

/* ---- collision broad phase (src/collision.jl) ------------------------------------------------------------------------
 * rc_contact_pair = ContactPair (:25-28): 1-based instance indices, instance_a < instance_b. */
typedef struct rc_contact_pair {
    uint32_t instance_a, instance_b;
} rc_contact_pair;
/* collide_instances(tlas) (:189-233) on a synced scene: all pairs of instances whose world AABBs overlap, found by one
 * TLAS walk per instance on the device (count pass, prefix sum, write pass).  *count receives the number of pairs; they
 * are written (in the reference algorithm's order) when out != NULL and capacity >= *count, else only counted.
 * rc_collide_instances copies to a host buffer, _device writes a device buffer on `stream` (the total is read back on
 * the host either way, as in the reference, :218). */
int rc_collide_instances(rc_scene* scene, rc_contact_pair* out, uint64_t capacity, uint64_t* count);
int rc_collide_instances_device(rc_scene* scene, rc_contact_pair* d_out, uint64_t capacity, uint64_t* count, void* stream);
/* collide_instances_any(tlas, handle_a, handle_b) (:241-261): do any two instances of the two handles overlap (AABB)?
 * Restated as written: the reference reads instance i's box from TLAS leaf position n-1+i (Morton-sorted order). */
int rc_collide_instances_any(rc_scene* scene, uint32_t handle_a, uint32_t handle_b, int* overlap);

/* ---- mesh ingestion and the full Triangle record -----------------------------------------------------------------------
 * rc_triangle = Triangle{UInt32}, 136 bytes (src/triangle_mesh.jl:1-7): what closest_hit returns by value. */
typedef struct rc_triangle {
    float vertices[3][3], normals[3][3], tangents[3][3], uv[3][2];
    uint32_t metadata;
} rc_triangle;
/* build_and_append_blas! after the GeometryBasics decomposition (src/instanced-bvh.jl:581-608): the caller passes what
 * expand_faceviews / decompose / decompose_normals / decompose_uv produced -- nv vertices (verts, normals: nv x 3 f32; uvs:
 * nv x 2 f32 or NULL), nf faces as 0-based index triples, and optionally the per-vertex face_meta array (the reference
 * reads face_meta[first vertex of the face], :595; NULL => face index 1..nf, assigned before the degenerate filter).
 * Expansion, is_degenerate_face filtering (:573-577), build_triangle (:555-566) and the LBVH build run on the device. */
int rc_add_mesh(rc_scene* scene, const float* verts, const float* normals, const float* uvs, uint32_t nv,
                const uint32_t* indices, uint32_t nf, const uint32_t* face_meta, uint32_t* blas_id);
/* The same with ONE METADATA WORD PER FACE (nf words): the TLAS(items, metadata_fn) constructor evaluates metadata_fn(mesh_idx, face_idx)
 * for every face (src/instanced-bvh.jl:2300-2306), which a per-vertex array cannot carry when faces share their first vertex (the two
 * triangles of a quad, the fans of a sphere).  Assigned before the degenerate filter, like the face index. */
int rc_add_mesh_face_metadata(rc_scene* scene, const float* verts, const float* normals, const float* uvs, uint32_t nv,
                              const uint32_t* indices, uint32_t nf, const uint32_t* metadata_per_face, uint32_t* blas_id);
/* update!(tlas, handle, new_mesh) (src/instanced-bvh.jl:808-857) for a decomposed mesh: replaces the BLAS the handle uses. */
int rc_update_geometry_mesh(rc_scene* scene, uint32_t handle, const float* verts, const float* normals, const float* uvs, uint32_t nv,
                            const uint32_t* indices, uint32_t nf, const uint32_t* face_meta);
/* all_blas_prims as full Triangles (synced scene; count query when out == NULL).  Geometry that came in as plain soup
 * (rc_add_blas*) has no mesh attributes: normals = geometric normal normalize((v1-v0) x (v2-v0)), uv = the reference's
 * default (0,0),(1,0),(1,1) (:561-565); tangents are NaN as in build_triangle. */
int rc_export_triangles(rc_scene* scene, rc_triangle* out, uint32_t capacity, uint32_t* count);
/* Shading epilogue next to the trace (docs/src/wavefront-renderer.jl:382-387), device buffers: per hit the interpolated
 * normal normalize(n0*b1 + n1*b2 + n2*b3) (d_normals, n x 3 f32) and uv0*b1 + uv1*b2 + uv2*b3 (d_uvs, n x 2 f32) with
 * (b1, b2, b3) = ((1-u)-v, u, v); zeros on a miss.  Either output may be NULL.  Saves returning 136-byte Triangles. */
int rc_shading_attributes_device(rc_scene* scene, const rc_hit* d_hits, uint64_t n, float* d_normals, float* d_uvs, void* stream);

/* More wavefront stages (device buffers, enqueued on `stream`):
 * rc_primary_rays_lookat_device: generate_primary_rays_lookat! (docs/src/wavefront-renderer.jl:219-254): width*height*samples
 * rays, ray (pixel-1)*samples + s for the row-major pixel (x, y); u = 2(x - 0.5 + j1)/width - 1, v = 1 - 2(y - 0.5 + j2)/height,
 * d = normalize(forward + right*(u*half_width) + up*(v*half_height)), t_min 0, t_max Inf.  The reference draws the jitter
 * from rand(Vec2f); here it is Philox4x32-10 keyed by `seed` with the ray index as counter (jitter != 0) or the pixel
 * centre (jitter == 0).
 * rc_compact_hits_device: ascending indices of the rays whose hit flag is set (d_indices, capacity n) and their number
 * (*d_count, a device u32) -- the queue compaction between stages; the reference's demo keeps dummy rays instead (:445). */
int rc_primary_rays_lookat_device(rc_scene* scene, const float camera_pos[3], const float camera_right[3], const float camera_up[3],
                                  const float camera_forward[3], float half_width, float half_height, uint32_t width, uint32_t height,
                                  uint32_t samples, uint64_t seed, int jitter, rc_ray* d_rays, void* stream);
int rc_compact_hits_device(rc_scene* scene, const rc_hit* d_hits, uint64_t n, uint32_t* d_indices, uint32_t* d_count, void* stream);
/* generate_reflection_rays! for perfect mirrors (docs/src/wavefront-renderer.jl:431-476, roughness 0) on reflect (src/math.jl:80):
 * per hit, origin = hit_point + shading_normal * bias, direction = reflect(-ray.d, shading_normal), t_max = Inf; misses get the
 * reference's dummy ray (d = (0,0,1), t_max = 0).  Material tests (metallic / roughness) stay with the caller. */
int rc_reflection_rays_device(rc_scene* scene, const rc_ray* d_rays, const rc_hit* d_hits, uint64_t n, float bias, rc_ray* d_out, void* stream);
/* rc_bounce_rays_device: diffuse (cosine-weighted) bounce rays, n_out output slots.  Output slot i continues source slot s:
 *  - d_src == NULL (slot-aligned): s = i, k = 0; d_src_count must be NULL and wrap 0.
 *  - d_src != NULL: c = *d_src_count is read ON THE DEVICE when the kernel runs (e.g. the count rc_compact_hits_device wrote earlier on
 *    the same stream), so the call needs no host read-back and can be captured.  c == 0: every slot is dead.  wrap == 0: s = d_src[i]
 *    for i < c, slots i >= c are dead (a live-first queue).  wrap == 1: s = d_src[i % c], k = i / c (round robin).
 *  - A slot whose source missed (d_hits[s].hit == 0) is dead too.
 * Path identity: path = path_base + (d_path_in ? d_path_in[s] : s); d_path_out (optional) receives lo32(path) per slot and
 * RC_INVALID_ID for dead slots, ready to be the next bounce's d_path_in (with path_base 0).  The random numbers depend only on
 * (path, k, bounce, seed), so they do not change when the queue is compacted or the batch is split into chunks or shards.
 * A live slot: (p, n) = the hit point and geometric world normal facing the ray origin (as rc_hit_points_device); origin p + n * bias,
 * t_min 0, t_max Inf; u1, u2 = the first two words of Philox4x32-10(counter = (lo32 path, hi32 path, k, 0x424E0000 | bounce),
 * key = (lo32 seed, hi32 seed)) as 24-bit floats in [0, 1); direction = cosine_sample_hemisphere(u1, u2) (src/math.jl:1-21,
 * concentric disk, Float32(pi), cos / sin evaluated in f64 and rounded once) in the basis get_orthogonal_basis(n) (src/math.jl:143-156):
 * d = (u*dx + v*dy) + n*z, not renormalised, every expression left to right without contraction.
 * A dead slot gets o = (0,0,0), d = (0,0,1), t_min = 0, t_max = -1.  Unlike the shadow stage's t_max = 0 dummy -- a [0, 0] interval can
 * still hit a triangle through the origin at t = 0 -- an interval with t_max < 0 misses under both rc_trace_closest_device and
 * rc_trace_any_device (any_hit starts from t_min = 0).
 * RC_ERR_INVALID_ARGUMENT: a NULL scene, d_rays, d_hits or d_out (the last three while n_out > 0); only one of d_src / d_src_count;
 * wrap without d_src; bounce >= 65536; n_out >= 2^32.  RC_ERR_NOT_SYNCED on an unsynced scene.  n_out == 0 writes nothing.
 * No allocation, copy or synchronisation: capture-safe and re-entrant like the other stages. */
int rc_bounce_rays_device(rc_scene* scene, const rc_ray* d_rays, const rc_hit* d_hits, const uint32_t* d_src, const uint32_t* d_src_count,
                          int wrap, const uint32_t* d_path_in, uint32_t* d_path_out, uint64_t path_base, uint64_t n_out, uint64_t seed,
                          uint32_t bounce, float bias, rc_ray* d_out, void* stream);

/* Scene files.  The reference has no on-disk format; this one keeps what a rebuild would recompute (per geometry: sorted
 * primitives, BVH2 nodes, mesh attributes; plus instance descriptors and the handle table).  rc_scene_save needs a synced
 * scene; rc_scene_load returns an unsynced scene whose handles are the saved ones -- rc_sync rebuilds the TLAS, after
 * which it traces bit-identically to the saved scene. */
int rc_scene_save(rc_scene* scene, const char* path);
int rc_scene_load(int device, const char* path, rc_scene** out);

/* instance_buffer(tlas, handle) (a stub for GPU back ends in the reference, src/Raycore.jl:117-128) + refit_tlas!
 * (src/instanced-bvh.jl:2197-2222): *d_descs receives the device address of the handle's InstanceDescriptor records (108 bytes
 * each, rc_instance_desc layout) inside the synced scene.  The caller's own kernels may rewrite `transform` (and
 * `inv_transform`) there; rc_refit_device then commits: recompute_inverse != 0 => inv_transform = mat3x4_inverse(transform) is
 * recomputed on the device for every instance first; then instance boxes, TLAS refit and traversal records are refreshed
 * in place -- no host round trip.  The host mirror is refreshed lazily (rc_get_instances / rc_export_instances / the next
 * mutation).  The address is valid until the next rebuilding rc_sync. */
int rc_instance_buffer_device(rc_scene* scene, uint32_t handle, rc_instance_desc** d_descs, uint32_t* count);
int rc_refit_device(rc_scene* scene, int recompute_inverse);

/* update_transforms!(tlas, handle, transforms) with a backend-resident array (src/instanced-bvh.jl:784-794,
 * update_instance_transforms_offset_kernel!, src/instanced-bvh-kernels.jl:455-476), and refit_tlas! (:2197-2222), both enqueued on the
 * caller's `stream` with no host wait: update -> refit -> trace can run back to back on one stream and be captured into one graph.
 *
 * rc_update_transforms_device: d_xforms = m x 12 f32 in device memory on the scene's device (Mat3x4f bytes as in rc_update_transforms,
 * 4-byte aligned), m = the handle's instance count.  One kernel writes, for every instance of the handle, transform = d_xforms[i],
 * inv_transform = mat3x4_inverse(transform) (the bytes rc_update_transforms computes on the host) -- blas_index, instance_id and flags
 * stay -- and everything the refit derives per instance (traversal record, entry-cull sphere, TLAS leaf box).  d_xforms is read WHEN THE
 * KERNEL RUNS, not when the call is made: a captured call picks up the array's current contents on every replay.  The scene becomes
 * transforms-dirty from the device: queries fail with RC_ERR_NOT_SYNCED until rc_refit_device_async (or rc_sync, which then refits from
 * the device descriptors, action 1) has been called; the host mirror of the descriptors is refreshed lazily (rc_get_instances, ...).
 * Errors, all before anything is enqueued: RC_ERR_INVALID_ARGUMENT (NULL scene or d_xforms, m != the handle's count),
 * RC_ERR_INVALID_HANDLE (unknown or deleted handle), RC_ERR_NOT_SYNCED (never synced, or pending host-side mutations: the descriptors'
 * device positions are those of the last sync).
 *
 * rc_refit_device_async: bottom-up refit of the TLAS and its traversal copy on `stream`.  After rc_update_transforms_device calls the
 * per-instance data is already in place; with none since the last refit (descriptors rewritten through rc_instance_buffer_device, with
 * their inverses) it is derived from the descriptors first, as rc_refit_device(scene, 0) does.  Do not mix the two ways between two refits.
 * No allocation, copy, event or synchronisation: legal on a capturing stream, once the stream has run it eagerly (like the trace).
 * THE WORLD BOUND stays in device memory: the host copy is refreshed lazily.  rc_world_bound, the ray grid / illumination drivers,
 * rc_scene_save and the multi-device replica check wait for the refit and read the root box back first; on a stream that is being
 * captured they fail with RC_ERR_NOT_SYNCED ("stale world bound") instead of using an old one -- call rc_world_bound before the capture.
 * The HOST-BUFFER queries (rc_trace_closest / rc_trace_any, rc_get_illumination, rc_view_factors*, rc_collide_instances*, the *_multi
 * calls, the rc_export_* calls) run on streams of the library's own, which a caller cannot order behind its stream: they wait on the
 * host for every EAGER update / refit enqueued so far (a flag test when none is pending), as do rc_sync and rc_refit_device.  Only the
 * *_device queries on OTHER streams are the caller's to order (events).
 * While a graph that captured an update or a refit may live (until a rebuilding rc_sync or "release_captures"), its replays change the
 * scene at times the library does not see: the caller waits for a replay before any host-side read or host-buffer query, and every read
 * of the world bound or of the host mirror of the descriptors then fetches it from the device again.
 * The batch-recognition scale of the trace launches (claim ordering) may use the last known bound: it cannot change a hit.
 * Reading the mirror (rc_get_instances, ...) between an update and its refit is harmless: the update stays pending.
 * rc_scene_destroy waits for eager updates / refits still in flight (their stream must still exist), not for graph replays. */
int rc_update_transforms_device(rc_scene* scene, uint32_t handle, const float* d_xforms, uint32_t m, void* stream);
int rc_refit_device_async(rc_scene* scene, void* stream);

/* rebuild_bvh!(tlas) (src/instanced-bvh.jl:968-992; build_tlas_topology, :1485-1594) from the instances' CURRENT DEVICE-SIDE transforms, enqueued on
 * the caller's `stream` with no host wait: rc_refit_device_async, except that the topology is built anew -- Morton codes from the new
 * instance boxes, stable sort, Karras tree, refit -- instead of kept from the last rc_sync.  For animations that carry instances far from
 * where they were sorted: a refitted tree's boxes grow and overlap, and the structural rc_sync that would repair it uploads the host
 * mirror, waits on the host and kills every captured update / refit.
 * RESULT: everything the trace reads is byte-identical to what a fresh scene holds after rc_sync, given the same BLASes and the same
 * instances pushed in the same order with these transforms: TLAS nodes (rc_export_tlas_nodes), world bound, and therefore every hit
 * record, exact ties and any_hit included.
 * IN PLACE: no buffer address changes and the node count, kernel choice and LDS plan depend on the instance count alone, so graphs that
 * captured updates, refits (also of this scene's WavefrontPaths frames) or traces stay valid and see the new tree on their next replay.
 * It rewrites the TLAS nodes and their traversal copy, the topology records later refits walk, the instance -> leaf table
 * rc_update_transforms_device scatters through, and the renumbering of the TLAS's top (scenes of more than 256 instances).
 * Scene state: as rc_refit_device_async.  After rc_update_transforms_device calls the per-instance data is in place; with none since the
 * last refit / rebuild it is derived from the descriptors first.  Clears transforms-dirty; leaves the world bound and the host mirror to
 * the same lazy refresh; host-buffer queries, rc_sync (then a no-op), rc_world_bound, the exports, rc_scene_save and the collision calls
 * behave as after an asynchronous refit.  A later rc_update_transforms + rc_sync refits on the new topology.
 * No allocation, host copy, event or synchronisation (its scratch, the sort's temporary storage included, is reserved by rc_sync and is
 * not shared with BLAS builds, which may run beside it on the scene's own stream): legal on a capturing stream, once the stream has run
 * it eagerly.
 * TWO DEVICE PATHS, same bytes: scenes of 2 .. 256 instances (the bound of the LDS-resident top level, where no renumbering exists) are
 * rebuilt by ONE workgroup in one dispatch, everything staged in LDS; larger ones, a single instance, and any scene with option
 * "tlas_rebuild_fused" = 0 run the build's chain of kernels (about a dozen dispatches and the sort's).
 * n == 0: success, nothing enqueued.  Errors, all before anything is enqueued: RC_ERR_INVALID_ARGUMENT (NULL scene), RC_ERR_NOT_SYNCED
 * (never synced, or pending host-side mutations).  Structural changes (instances or geometry added / deleted) stay with rc_sync. */
int rc_rebuild_tlas_device_async(rc_scene* scene, void* stream);

/* WHEN to rebuild, decided on the device: refit_tlas! every frame, rebuild_bvh! (src/instanced-bvh.jl:968-992) only on the frames whose
 * refitted tree has degraded.  A captured frame can then refit while instances drift and rebuild on the replay in which they scatter; the
 * host never reads the tree.
 *
 * rc_tlas_cost_device: the cost of the TLAS as it is WHEN THE KERNELS RUN, one f64 written to caller-owned device memory on `stream`.  For
 * n >= 2 instances, internal node i (1 <= i <= n - 1 of rc_export_tlas_nodes) has the box of the union of its two child boxes and
 * A_i = 2 (ex ey + ey ez + ez ex), the extents formed in f64 from the f32 corners; cost = sum A_i / A_1, the summed surface area of the
 * internal boxes relative to the root's (about what a ray pays per unit of root area it crosses).  n == 1: exactly 1.0.  n == 0: success,
 * nothing enqueued.  DETERMINISTIC: no floating-point atomics; per-block partial sums and their fold run in an order fixed by n alone, so
 * two evaluations of one tree give the same 8 bytes.  No allocation, host copy, event or synchronisation: legal on a capturing stream,
 * once the stream has run it eagerly.  Calls on different streams at the same time share its partial sums: one stream at a time.
 * LIFETIME: the call records no event, so rc_scene_destroy waits for it only as the scene's latest eager asynchronous work -- when an
 * update, refit or rebuild is still pending on ANOTHER stream, that stream is the one waited for, and the caller synchronises the cost
 * call's stream itself before destroying the scene.
 * Errors: RC_ERR_INVALID_ARGUMENT (NULL scene or d_cost), RC_ERR_NOT_SYNCED (never synced, or pending host-side mutations).
 *
 * rc_refit_or_rebuild_tlas_device_async: on `stream`,
 *   1. exactly what rc_refit_device_async does (the per-instance pass under the same rule);
 *   2. the cost pass, which stores `cost` and a gate word = (cost > ratio * cost_built), compared in f64 as written -- a NaN cost never
 *      rebuilds.  The gate is written on every run, 0 as well as 1: a replay never sees the previous frame's decision;
 *   3. the rebuild of rc_rebuild_tlas_device_async, taken only if the gate is set;
 *   4. if it was taken: cost_built = the new tree's cost, the rebuild counter advances, the gate is cleared.
 * All of that state is a small block in device memory; nothing is read back.
 * RESULT: after a run whose gate was clear, everything a trace, an export or a later refit reads is byte-identical to what
 * rc_refit_device_async leaves; after a run whose gate was set, to what rc_rebuild_tlas_device_async leaves, and therefore to a fresh
 * scene after rc_sync.  In place in both cases: earlier captures of updates, refits, rebuilds and traces stay valid.
 * BOTH DEVICE PATHS take the gate.  2 .. 256 instances with "tlas_rebuild_fused" = 1: one workgroup reads the refitted tree's cost,
 * decides, and either returns or rebuilds in LDS and records -- a drifting frame is a refit plus one small dispatch.  Otherwise the cost
 * pass is two small kernels and every kernel of the build's chain that writes outside the rebuild scratch (TLAS nodes, topology records,
 * instance -> leaf table, top renumbering, traversal copy) returns when it reads a clear gate; the ones that touch only the scratch,
 * the sort included, run regardless: a skipped rebuild costs their time and nothing else.  The gate crosses a kernel boundary on one
 * stream, never a launch in flight.
 * THE STATE BLOCK (cost, cost_built, gate, evaluations, rebuilds, last decision) is reserved, zeroed and DISARMED by every rebuilding
 * rc_sync.  The host cannot know what an earlier sequence of refits left, so the first call after such a sync ARMS it: refit ->
 * unconditional rebuild -> record cost_built, counted as one evaluation and one rebuild.  That call must be eager: on a capturing stream
 * it returns RC_ERR_NOT_SYNCED and says so.  While armed, rc_rebuild_tlas_device_async appends the same record step, so the baseline
 * follows explicit rebuilds; while not armed it enqueues exactly what it always did.  A graph that captured an unconditional rebuild
 * BEFORE arming does not record: replayed after arming it leaves cost_built at the previous tree's cost.
 * n == 1: refit only (the arming call aside), cost 1.0, never rebuilt.  n == 0: success, nothing enqueued.
 * Scene state (world bound, host mirror, captured-refit rule, the host wait of the host-buffer queries, no-op rc_sync): as after
 * rc_refit_device_async.  No allocation, host copy, event or synchronisation: legal on a capturing stream once armed and run eagerly.
 * Errors, all before anything is enqueued: RC_ERR_INVALID_ARGUMENT (NULL scene; ratio not finite or <= 0), RC_ERR_NOT_SYNCED (never
 * synced, pending host-side mutations, or the arming call on a capturing stream), RC_ERR_HIP (the rebuild scratch does not match the
 * instance count).  Structural changes stay with rc_sync.
 *
 * rc_tlas_quality: the block, read on the host under the rules of the other lazy reads: it waits for the EAGER asynchronous work
 * enqueued so far; while a graph that captured the call may live, the caller waits for its replay first.  cost: what the latest evaluation
 * measured (the refitted tree's, also when a rebuild followed; the arming call: the built tree's); cost_built: the tree's cost at the latest
 * recorded rebuild; evaluations, rebuilds: counts since the last rebuilding rc_sync (the arming call is
 * one of each); last_rebuilt: the latest evaluation's decision; armed: 0 until the arming call.  n == 0: all zero.
 * Errors: RC_ERR_INVALID_ARGUMENT (NULL scene or out), RC_ERR_NOT_SYNCED (never synced, or pending host-side mutations: the block belongs
 * to the synced scene).  A device-side update that still waits for its commit does not refuse the read. */
typedef struct rc_tlas_quality_info {
    double cost, cost_built;
    uint32_t evaluations, rebuilds, last_rebuilt, armed;
} rc_tlas_quality_info;
int rc_tlas_cost_device(rc_scene* scene, double* d_cost, void* stream);
int rc_refit_or_rebuild_tlas_device_async(rc_scene* scene, double ratio, void* stream);
int rc_tlas_quality(rc_scene* scene, rc_tlas_quality_info* out);

/* update!(tlas, handle, new_geometry) (src/instanced-bvh.jl:808-857) with backend-resident vertices: build_blas (:1376-1443) -- degenerate
 * filter, Morton codes, stable sort, gather, Karras tree, leaves, refit -- enqueued on the caller's `stream` with no host wait, for meshes
 * whose vertices move every frame (skinning, cloth, simulation output).  update -> [rc_update_transforms_device] -> refit -> trace can run
 * back to back on one stream and be captured into one graph.
 *
 * rc_update_geometry_device_async: d_verts = n x 9 f32 soup in device memory on the scene's device, d_meta = n u32 or NULL (NULL: face
 * index 1..n, assigned BEFORE the degenerate filter, as in rc_add_blas).  Both are read WHEN THE KERNELS RUN, not when the call is made: a
 * captured call picks up the arrays' current contents on every replay.
 * IN PLACE: the number of non-degenerate faces must equal the BLAS's current n_prims (n itself may differ, degenerate faces included).
 * Then no address, offset, node count, kernel choice or LDS plan changes, and graphs that captured traces, updates, refits or rebuilds of
 * this scene stay valid.  RESULT: everything is byte-identical to what a fresh scene holds after rc_sync given the new soup: the BLAS's
 * nodes and primitives (rc_export_blas_nodes, rc_export_prims; a later structural rc_sync copies from them), their slices of the traversal
 * copy, the root box (rc_export_blas_descs), the entry-cull radius, in a single-BLAS scene the renumbering of the BLAS's top, the shading
 * attributes of the slice if they had been built, the face map of a mesh, and, for every instance of this geometry (through whichever
 * handle), traversal record, entry-cull sphere and TLAS leaf box.
 * The face count is compared ON THE DEVICE.  On a mismatch, or zero valid faces, nothing that a trace, an export or a later sync reads is
 * modified and a sticky status makes the next rc_wait return RC_ERR_GEOMETRY_CHANGED, once; the scene then still traces the old geometry.
 * Scene state afterwards: exactly as after rc_update_transforms_device -- transforms-dirty from the device, queries fail with
 * RC_ERR_NOT_SYNCED until rc_refit_device_async, rc_rebuild_tlas_device_async or rc_sync (which then refits, action 1); it composes in
 * either order with rc_update_transforms_device on the same stream before that refit.  The HOST copies of the root box are refreshed
 * lazily under the rules of the asynchronous refit: rc_export_blas_descs, rc_scene_save and a structural rc_sync wait for the update and
 * read the box back first, and fail while the update's stream is being captured; while a graph that captured an update may live (until a
 * rebuilding rc_sync or "release_captures") they read it back on every use.
 * At call time the geometry's BLAS4 is dropped (rc_trace_*4 behave as for a geometry whose BLAS4 was never built, until rc_blas4_build;
 * a BLAS4 built while a graph that captured an update of the geometry may live describes the tree of that moment: the next replay leaves
 * it stale without dropping it, so build it again after the replay it should follow)
 * and the view-factor source order (RC_VF_SOURCES_BY_METADATA) is invalidated: the next call that needs it waits on the host for the
 * eager updates enqueued so far and sorts again.  While a graph that captured an update may live, every replay re-sorts the primitives at
 * a time the library does not see, so the order is rebuilt ON EVERY USE (one small sort and a host wait per rc_view_factors* call): such a
 * call is a host-side read -- the caller waits for the replay first -- and on a stream that is being captured it fails with
 * RC_ERR_NOT_SYNCED ("stale view-factor source order") instead of using an old order.  A captured update refreshes the shading attributes only if they existed at capture
 * time: while such a graph may live, a call that would have to build them fails with RC_ERR_NOT_SYNCED -- use
 * rc_shading_attributes_device once before capturing.  A captured update also holds the addresses of the geometry's OWN arrays: a host-side
 * rc_update_geometry / rc_update_geometry_mesh of that geometry frees them at once -- the graph is dead from that call on, not only
 * from the next rebuilding rc_sync (which is where a deleted geometry goes).
 * SCRATCH: the call's own (not the BLAS-build scratch of the scene's stream), the sort's temporary storage included, sized for the
 * largest n seen and shared by the scene's geometries -- enqueue these calls on one stream at a time.  An eager call may grow it; a call
 * on a capturing stream that would have to grow it fails before enqueuing anything.  Otherwise no allocation, host copy, event or
 * synchronisation: legal on a capturing stream once that stream has run it eagerly (with the same n).
 * Errors, all before anything is enqueued: RC_ERR_INVALID_ARGUMENT (NULL scene or d_verts, n == 0, a scratch growth needed on a
 * capturing stream), RC_ERR_INVALID_HANDLE (unknown or deleted handle, a handle without instances), RC_ERR_NOT_SYNCED (never synced, or
 * pending host-side mutations).
 *
 * rc_update_mesh_vertices_device_async: the same for a geometry added through rc_add_mesh*: d_verts = nv x 3 f32 new vertex positions,
 * d_normals = nv x 3 f32 new normals or NULL (keep the stored ones).  Indices, uvs and metadata are kept; the faces are expanded through
 * the stored indices and the face map is rebuilt, so rc_shading_attributes_device and rc_reflection_rays_device see the new normals.  In a
 * scene read by rc_scene_load the first call on a geometry recovers the per-face metadata from the surviving primitives (an allocation:
 * eager only; a face that was degenerate when the file was written gets its index as metadata should it become valid).  nv != the mesh's vertex
 * count, or a geometry that is not a mesh: RC_ERR_INVALID_ARGUMENT.
 * Out of scope: a BLAS refit without the re-sort, a changed triangle count, geometry added or deleted -- those stay with rc_sync. */
int rc_update_geometry_device_async(rc_scene* scene, uint32_t handle, const float* d_verts, const uint32_t* d_meta, uint32_t n, void* stream);
int rc_update_mesh_vertices_device_async(rc_scene* scene, uint32_t handle, const float* d_verts, const float* d_normals, uint32_t nv, void* stream);

/* Page-lock (pin) a caller-owned host array so that the host-buffer entry points (rc_trace_closest / rc_trace_any, rc_add_blas,
 * rc_view_factors ...) move it by DMA at the full PCIe rate instead of through the driver's staging copies: the option a Julia
 * `Vector{RTRay}` / `Vector{RTHitResult}` pair that is traced every frame wants (there is no counterpart in the reference, whose
 * arrays live in the backend's memory).  Thin wrappers over hipHostRegister / hipHostUnregister so that a caller without HIP
 * bindings can use them; the memory stays the caller's.  Registering an array twice, or unregistering one that is not
 * registered, is an error (non-zero status). */
int rc_host_register(rc_scene* scene, void* ptr, uint64_t bytes);
int rc_host_unregister(rc_scene* scene, void* ptr);

/* Timing of the most recent trace / driver launch or BLAS build (device pipeline, without staging copies) on this scene, measured with HIP events on the launch
 * stream (kernel only, no copies), in milliseconds.  For a trace launch the two events ride on the trace kernel's own dispatch: the figure is that
 * kernel's duration and does NOT include the pair of small claim-order rebuild kernels (5 + 8 us) the library enqueues in front of about one
 * launch in eight of a REPEATED batch (first launches enqueue nothing else).  Time a run of launches between two events of your own on the stream
 * to include them -- bench.py does so for every repeated-batch figure. */
int rc_last_kernel_ms(rc_scene* scene, float* ms);
/* The same for the scene's most recent eager launches on any stream, oldest first: up to max_launches (at most 47: a launch's events live until
 * the scene's 48th launch after it) durations into ms[], their number into *n.  Waits for the launches asked about.  For a caller that
 * enqueues a run of launches back to back and wants every one's duration afterwards without putting events of its own between them (the
 * reference times its kernels the same way, one by one: docs/src/hw_acceleration.md:198-218).  Captured launches have no events: 0. */
int rc_recent_kernel_ms(rc_scene* scene, uint32_t max_launches, float* ms, uint32_t* n);

/* ---- illumination over MANY DIRECTIONS in one call, the grids laid out on the device -------------------------------------------------
 * get_illumination (src/kernels.jl:10-72,112-124: generate_ray_grid, hits_from_grid and the histogram) for n_dirs view directions at once.
 * The reference's users integrate over directions -- the sun's course over a day, a few dozen sky sectors, each weighted by its irradiance
 * (docs/src/viewfactors_content.md:84-92) -- which with rc_get_illumination_device is n_dirs host-driven calls, each laying its grid out on
 * the host from the host copy of the world bound.
 *
 * d_dirs: n_dirs x 3 f32 in DEVICE memory; the directions need not be normalised.  Both d_dirs and the TLAS root box the grids are laid
 * out from are read WHEN THE KERNEL RUNS, not when the call is made, by the same code that lays the one-direction grid out on the host
 * (one host/device function, no contraction, IEEE divide and square root: the same bits).  The host copy of the world bound is neither read
 * nor refreshed.  This is THE EXCEPTION to the "stale world bound" rule spelled out at rc_refit_device_async: after rc_refit_device_async,
 * rc_rebuild_tlas_device_async or rc_refit_or_rebuild_tlas_device_async on the same stream these two calls need no host wait, and they are
 * legal on a capturing stream -- a captured call replays with its capture-time n_dirs and grid, with the CURRENT contents of d_dirs and the
 * CURRENT TLAS root, so an animated scene's illumination can be computed inside its frame graph.
 *
 * rc_get_illumination_dirs_device.  WORK-ITEM LAYOUT: item i = d * grid^2 + cell, cell = the ray index of rc_generate_ray_grid_device;
 * ray (d, cell) is bit for bit the ray that call writes for d_dirs[d].  Items are claimed in natural order.
 * d_counts[d * row_stride + (meta - 1)] += the number of rays of direction d whose closest hit is a primitive with metadata `meta`;
 * metadata outside 1..n_prims is dropped, as in get_illumination (src/kernels.jl:123).  row_stride >= n_prims, in u32 words; words of a
 * row beyond n_prims are not touched.  The call ACCUMULATES (the convention of rc_get_illumination_device and rc_view_factors_device): the
 * caller zeroes the matrix; the adds are u32 atomics, exact in any order, so calls on several streams may share a matrix.
 * Counts are u32, NOT the reference's saturating f32: row d equals what rc_get_illumination_device adds for d_dirs[d] whenever that count
 * is below 2^24, where the reference's Float32 sum stops.  Weighting the rows is the caller's: a float weight inside the kernel would make
 * the sum depend on the order of the atomics.
 * The directions are traced in groups of G consecutive ones, one persistent launch per group behind one memset and one small grid-layout
 * kernel, in front of one fold; G is the largest count with G * grid^2 < 2^32 whose private histogram copies (G * 512 * ceil(n_prims / 8)
 * bytes) fit option "illum_scratch_bytes" (default 256 MiB; at least one direction's worth is always used).  The option changes no result.
 * The plan (G, the scratch size) is fixed at call time.  Scratch is the per-stream area of rc_get_illumination_device; a captured call owns
 * its own, one capture slot per group, under the rules of the other driver launches (the stream must have run the call eagerly before).
 *
 * rc_generate_ray_grid_dirs_device writes n_dirs x grid^2 rays: direction d starts at d * grid^2, in the layout of
 * rc_generate_ray_grid_device.  One kernel, no scratch.
 * A direction whose normalisation is not finite (zero, NaN) gives whatever the one-direction entry points give for it.
 *
 * Scene state: as the *_device queries.  n_dirs == 0, grid == 0 or an empty scene: success, nothing enqueued.
 * Errors, all before anything is enqueued and with the output untouched: RC_ERR_INVALID_ARGUMENT (NULL scene; NULL d_dirs or output while
 * n_dirs and grid are non-zero; grid >= 65536; row_stride < n_prims), RC_ERR_NOT_SYNCED (never synced, pending host-side mutations, or
 * transforms-dirty from the device with no refit / rebuild yet).  A stack overflow is reported by rc_wait.
 * Register and scratch figures of the three new kernel shells and the comparison with a loop of one-direction calls: docs/EXPERIMENTS.md,
 * "Illumination over many directions". */
int rc_get_illumination_dirs_device(rc_scene* scene, const float* d_dirs, uint32_t n_dirs, uint32_t grid, uint32_t* d_counts,
                                    uint64_t row_stride, void* stream);
int rc_generate_ray_grid_dirs_device(rc_scene* scene, const float* d_dirs, uint32_t n_dirs, uint32_t grid, rc_ray* d_rays, void* stream);

/* ---- View-factor products: the view-factor matrix APPLIED TO A VECTOR, without the matrix: what a radiosity iteration
 * B <- E + rho .* (M * B) ./ R needs of view_factors (src/kernels.jl:74-104).  With M = the reference's result[src_meta, hit_meta], every counted ray (the rule of :93-97) from
 * a source with metadata a that hits metadata b adds
 *     mx [a-1] += x[b-1]        (M  x)[a-1]
 *     mtx[b-1] += x[a-1]        (M^T x)[b-1]
 * x: n_prims u32, indexed by metadata - 1 like the totals vectors; mx, mtx: n_prims u64, sums modulo 2^64 -- integer adds, exact in any
 * order, so every partition of sources x rays gives the same words; either output may be NULL.  Same rays (Philox keyed by seed, ray
 * index, source primitive) and the same counting rule as rc_view_factors, so the vectors equal that matrix times x exactly, and with
 * x = 1 they are `emitted` and `received` of rc_view_factor_totals.  x is read only for counted rays, whose metadata are both in 1..N:
 * metadata 0 or above N never index it.  No N x N array exists anywhere; the call costs the tracing.
 * _device: rays [ray_begin, ray_end) of the sources with flat primitive indices [src_begin, src_end), clamped to the scene, ACCUMULATED
 *   into device vectors on the caller's stream; an empty range enqueues nothing.  The argument list is rc_view_factor_totals_device's with
 *   d_x in front of the outputs, and so are the rules: the hot vector (d_mtx) is counted into private copies and added atomically at the
 *   end of the launch, scratch is per stream, shards accumulate on one stream or concurrently on several, and the call may be captured
 *   on a stream that has run it eagerly once, like rc_get_illumination_dirs_device.  It is the shard unit of a multi-process run
 *   (torch.distributed reduce of 2 N int64).  RC_ERR_INVALID_ARGUMENT for a NULL scene, a NULL d_x or both outputs NULL;
 *   RC_ERR_NOT_SYNCED as the other *_device queries.
 * rc_view_factor_products: host arrays, all sources and rays, the outputs OVERWRITTEN.
 * Register and scratch figures of the three kernel shells and the cost beside the totals call: docs/EXPERIMENTS.md, "View-factor products". */
int rc_view_factor_products_device(rc_scene* scene, uint32_t rays_per_triangle, uint64_t seed, uint32_t src_begin, uint32_t src_end,
                                   uint32_t ray_begin, uint32_t ray_end, const uint32_t* d_x, uint64_t* d_mx, uint64_t* d_mtx, void* stream);
int rc_view_factor_products(rc_scene* scene, uint32_t rays_per_triangle, uint64_t seed, const uint32_t* x, uint64_t* out_mx, uint64_t* out_mtx);

/* ---- Form factors between surface groups: the view-factor job (src/kernels.jl:74-104) with a choice of SAMPLING, counted per GROUP of
 * primitives -- a wall, a sphere, a thermal zone -- with a WEIGHT per source primitive.  The reference shoots its rays uniformly over the
 * hemisphere (random_hemisphere_uniform, src/kernels.jl:92); a Lambertian surface exchanges energy with a cosine weighting, so the
 * reference's matrix is not a form-factor matrix: between opposite walls of the unit cube it gives 0.11 where the form factor is 0.1998.
 * THE SAMPLED RAY of (source primitive, ray index): the Philox4x32-10 draw of rc_view_factor_rays_device -- counter (ray_idx, src_prim, 0,
 * 0), key = seed -> r1, r2, xi1, xi2 -- and, in BOTH samplings, its point on the triangle and its origin pt + normal * 0.01f.
 *   RC_VF_SAMPLING_UNIFORM: the direction of rc_view_factor_rays_device, bit for bit (the same device function).
 *   RC_VF_SAMPLING_COSINE:  d = the cosine-weighted direction about the triangle's unit normal that rc_bounce_rays_device makes from
 *     (normal, xi1, xi2) -- the same function, applied to the third and fourth Philox words, not renormalised.  t_min = 0, t_max = inf.
 * rc_view_factor_sampled_rays_device, the composed stage: writes rays [ray_begin, ray_begin + n_rays) of one source primitive, the sibling
 * of rc_view_factor_rays_device.  RC_ERR_INVALID_ARGUMENT for a NULL scene or d_rays, sampling > 1, or src_prim out of range.
 * rc_view_factor_groups_device, the fused driver.  Work item w -> flat source primitive src_begin + w / n_ray, ray ray_begin + w % n_ray,
 * traced for the closest hit.  THE RULE, word for word:
 *   N = number of flat primitives. a = the source's metadata, b = the hit's. ga = groups[a-1], gb = groups[b-1]. wa = weights ? weights[a-1] : 1.
 *   A source whose a is outside 1..N, or whose ga >= G, contributes nothing.
 *   Miss: escaped[ga] += wa, if escaped is given.
 *   Hit with b in 1..N, b != a and gb < G: matrix[ga * G + gb] += wa.  (The reference's rule hit_idx != tri_idx, src/kernels.jl:96, is kept.)
 *   Any other hit adds nothing.
 *   All sums are u64 modulo 2^64: exact in any order, so any partition of sources x rays gives the same words.
 * d_groups, d_weights: N u32 each, indexed by metadata - 1, read WHEN THE KERNEL RUNS and for metadata in 1..N only; d_weights may be NULL.
 * d_matrix: G * G u64, row = source group; d_escaped: G u64, or NULL.  A group value >= G (0xFFFFFFFF, say) excludes a primitive as a
 * source and as a target.
 * THE IDENTITY.  With RC_VF_SAMPLING_UNIFORM the result is an exact function of the reference's matrix M = result[src_meta, hit_meta] of
 * rc_view_factors for the same (rays_per_triangle, seed):  matrix = P diag(w) M P^T  with P[g, i] = (groups[i] == g), in integers; with
 * identity groups and no weights it IS that matrix (u32 widened), and its row and column sums are rc_view_factor_totals' vectors.  In both
 * samplings the words equal what rc_view_factor_sampled_rays_device -> rc_trace_closest_device -> the rule above give.  With
 * RC_VF_SAMPLING_COSINE and weights proportional to the primitives' areas, matrix[A, B] / (R * sum of the weights of A) estimates the form
 * factor F_AB = sum_{i in A} A_i F_iB / A_A.
 * Both outputs ACCUMULATE: the caller zeroes them.  Rays [ray_begin, ray_end) of the sources with flat primitive indices [src_begin,
 * src_end), clamped to the scene like rc_view_factor_totals_device's; an empty range enqueues nothing; shards accumulate on one stream
 * or concurrently on several.  With a handful of groups every wave adds onto a few dozen words, so the kernel counts into private copies
 * of the G * G (+ G) words and adds them to the outputs atomically at the end of the launch when the copies (128 * 8 * ceil((G * G + G) / 8)
 * bytes) fit 256 MiB (G <= 1447 with escapes), and straight onto the outputs otherwise.  Both paths give the same words.
 * Scratch is per stream; nothing is read on the host, and the call may be captured on a stream that has run it eagerly once, like
 * rc_view_factor_products_device; a replay reads the CURRENT d_groups and d_weights.  Legal behind rc_update_geometry_device_async on the
 * same stream with no host wait.
 * RC_ERR_INVALID_ARGUMENT for a NULL scene, d_groups or d_matrix, for sampling > 1, and for n_groups outside 1..65535 (the kernel indexes
 * G * G + G words in 32 bits); RC_ERR_NOT_SYNCED as the other *_device queries.
 * Register and scratch figures of the kernel shells and the measurements: docs/EXPERIMENTS.md, "Form factors between surface groups". */
#define RC_VF_SAMPLING_UNIFORM 0u   /* the reference's rays, src/kernels.jl:92 */
#define RC_VF_SAMPLING_COSINE  1u   /* Lambertian: form factors */
int rc_view_factor_sampled_rays_device(rc_scene* scene, uint64_t seed, uint32_t sampling, uint32_t src_prim, uint32_t ray_begin,
                                       uint32_t n_rays, rc_ray* d_rays, void* stream);
int rc_view_factor_groups_device(rc_scene* scene, uint32_t rays_per_triangle, uint64_t seed, uint32_t sampling, uint32_t src_begin,
                                 uint32_t src_end, uint32_t ray_begin, uint32_t ray_end, const uint32_t* d_groups, uint32_t n_groups,
                                 const uint32_t* d_weights, uint64_t* d_matrix, uint64_t* d_escaped, void* stream);

/* ---- Sparse view-factor matrix: the matrix of view_factors (src/kernels.jl:74-104) ITSELF, as CSR, built once on the device.  A source
 * shoots rays_per_triangle rays, so a row of M = the reference's result[src_meta, hit_meta] has at most min(R, N) non-zeros: the dense N x N
 * form is the wrong container (4 TB at 1 Mi triangles; the CSR at R = 256 holds at most 256 Mi entries).  Same rays (Philox keyed by seed,
 * ray index, source primitive) and the same counting rule (:93-97) as rc_view_factors, so the integers are that matrix's.
 * The call OVERWRITES its outputs with rows [row_begin, row_end) of M (row r <=> metadata r + 1; row_end is clamped to N) in canonical CSR:
 *   d_row_ptr: rows + 1 u64, d_row_ptr[0] = 0, d_row_ptr[rows] = *d_nnz; entries k in [d_row_ptr[r], d_row_ptr[r + 1]) belong to row
 *   row_begin + r; d_cols[k] (0-based column = hit metadata - 1) strictly ascending within a row; d_vals[k] >= 1 -- no explicit zeros.
 * The arrays are therefore a function of (scene, rays_per_triangle, seed, row range) alone: neither the scratch size (option
 * "vf_sparse_scratch_bytes", default 256 MiB: the job is cut into chunks of WHOLE rows whose rays x 8 bytes fit it; a single larger row gets
 * a chunk of its own) nor the shape of any kernel changes a word.  Sources with metadata 0 or above N have no row; sources that share a
 * metadata share a row.  Rows are independent: the blocks of a partition of [0, N) concatenate (each block's d_row_ptr starts at 0) -- row
 * blocks are the shard unit of a multi-device build.
 * Capacity (the idiom of rc_collide_instances, without a host read): *d_nnz and ALL of d_row_ptr are always the true values; entries at
 * positions < capacity are the correct first entries; nothing is written at or beyond capacity; d_cols / d_vals may be NULL when capacity
 * is 0 -- the counting call.
 * _device: everything on the caller's stream, no host wait between the steps (trace of one u64 key per ray, radix sort, run-length
 *   encoding, append; an exclusive scan of the row counts at the end); scratch is per stream, two streams may build at once.  NOT
 *   capturable: RC_ERR_NOT_SYNCED on a stream that is being captured.  RC_ERR_INVALID_ARGUMENT for a NULL scene, d_row_ptr or d_nnz, NULL
 *   d_cols / d_vals with capacity > 0, or a row whose sources x rays_per_triangle reaches 2^32.
 * rc_view_factors_sparse: host arrays, all rows; returns RC_OK and reports *out_nnz, which the caller compares with capacity.
 *
 * rc_view_factor_sparse_products_device: the products of a CSR block with a vector, the step of a radiosity iteration once the matrix of
 * view_factors (src/kernels.jl:74-104) is held sparse.  For block rows r in [0, n_rows) and entries k of row r it ACCUMULATES, modulo 2^64,
 *     d_mx [row_offset + r] += d_vals[k] * d_x[d_cols[k]]
 *     d_mtx[d_cols[k]]      += d_vals[k] * d_x[row_offset + r]
 * either output may be NULL.  With the CSR of the same (rays_per_triangle, seed) the sums equal rc_view_factor_products_device's words bit
 * for bit -- at the cost of reading nnz x 8 bytes instead of tracing N x R rays again.  Row-parallel, the row bounds are read from
 * d_row_ptr on the device: capturable, and no host wait is needed behind the build.  The arrays are NOT validated: d_cols[k] < the length
 * of d_x / d_mtx is the caller's contract.  RC_ERR_INVALID_ARGUMENT for a NULL scene, d_row_ptr or d_x, or both outputs NULL.
 * Measured build, product and break-even figures: docs/EXPERIMENTS.md, "Sparse view-factor matrix". */
int rc_view_factors_sparse_device(rc_scene* scene, uint32_t rays_per_triangle, uint64_t seed, uint32_t row_begin, uint32_t row_end,
                                  uint64_t* d_row_ptr, uint32_t* d_cols, uint32_t* d_vals, uint64_t capacity, uint64_t* d_nnz, void* stream);
int rc_view_factors_sparse(rc_scene* scene, uint32_t rays_per_triangle, uint64_t seed, uint64_t* out_row_ptr, uint32_t* out_cols,
                           uint32_t* out_vals, uint64_t capacity, uint64_t* out_nnz);
int rc_view_factor_sparse_products_device(rc_scene* scene, uint32_t n_rows, uint32_t row_offset, const uint64_t* d_row_ptr, const uint32_t* d_cols,
                                          const uint32_t* d_vals, const uint32_t* d_x, uint64_t* d_mx, uint64_t* d_mtx, void* stream);

/* ---- Illumination from point sources: get_illumination (src/kernels.jl:112-124) for lamps at a FINITE position.  The reference's
 * get_illumination and rc_get_illumination_dirs_device shoot an orthographic grid -- a source at infinity, the sun or a sky sector.  These
 * two calls extend that driver to sources inside the scene: a jittered, stratified, equal-area set of grid^2 rays from each source, the
 * closest hit, and one count per source and primitive.
 * WHAT A COUNT MEANS.  For an ISOTROPIC source, d_counts[k][j] / grid^2 is the fraction of the lamp's flux that arrives at the primitives
 * with metadata j + 1: their visible solid angle over 4 pi.  The 1 / r^2 and cosine factors come out of the shooting, in integers; there is
 * no float in the kernel.  For a LAMBERTIAN emitter (a ceiling panel, a window patch) the same count under cosine-weighted shooting is the
 * form factor from the emitter to those primitives; weights @ counts / grid^2 with each lamp's flux as its weight is the received flux per
 * primitive -- the `emission` of a radiosity solve, up to the caller's reflectance and area.
 * A SOURCE is one rc_ray record in DEVICE memory, read WHEN THE KERNEL RUNS: o = the lamp's position, d = its axis, t_min and t_max copied
 * unchanged into every ray it emits (t_max: the lamp's range).  d.x == 0 && d.y == 0 && d.z == 0 (either sign of zero): isotropic;
 * anything else: Lambertian about d / sqrt(dot(d, d)).
 * Source k (0-based in the call) shoots grid^2 rays, cell = a * grid + b with a, b in [0, grid); every expression f32, one operation at a
 * time, left to right, IEEE divide and square root, no contraction:
 *   rnd = Philox4x32-10, counter (cell, first_source + k, 0, 0x50530000), key = (lo32 seed, hi32 seed)
 *   xi1, xi2 = its first two words as 24-bit floats in [0, 1): (word >> 8) * 2^-24, the conversion of rc_bounce_rays_device
 *   u1 = ((float)a + xi1) / (float)grid, u2 = ((float)b + xi2) / (float)grid     (u may round to exactly 1; both mappings are defined there)
 *   isotropic:  z = 1 - 2 * u1;  s = sqrtf(fmaxf(0, 1 - z * z));  phi = (2 * 3.1415927f) * u2;  (sin, cos) of (double)phi by the f64
 *               kernels of the view-factor sampler, each rounded once to f32;  dir = (s * cos, s * sin, z), not renormalised
 *   Lambertian: dir = the cosine-weighted direction about the normalised axis that rc_bounce_rays_device makes from (axis, u1, u2): the
 *               same function, not renormalised
 *   ray(k, cell) = origin o, t_min, direction dir, t_max.
 * first_source only offsets the Philox counter: a set of sources split over several calls, groups, streams or devices gives the rows of
 * the one-call result.  A source with non-finite fields gives whatever the composed path below gives for it.
 *
 * rc_point_source_rays_device, the composed stage: writes n_sources x grid^2 rays, ray(k, cell) at k * grid^2 + cell.  One kernel, no
 * scratch.  The output feeds rc_trace_closest_device unchanged.
 * rc_get_illumination_points_device, the fused driver.  WORK-ITEM LAYOUT: item i = k * grid^2 + cell; the ray is generated when a lane takes
 * the item -- bit for bit the stage's, the same device function makes both -- and never stored.  Items are claimed in natural order.
 *   d_counts[k * row_stride + (meta - 1)] += the number of rays of source k whose closest hit has metadata `meta`; metadata outside
 *   1..n_prims is dropped (src/kernels.jl:123).  row_stride >= n_prims, in u32 words; words of a row beyond n_prims are not touched.
 *   d_escaped[k] += the number of rays of source k that hit nothing.  n_sources u32; may be NULL, and then the kernel has no code for it.
 * Both outputs ACCUMULATE with u32 atomics, exact in any order: the caller zeroes them, and calls on several streams may share them.  Per
 * source: row sum + escaped + dropped = grid^2.
 * The sources are traced in groups of G consecutive ones, one persistent launch per group behind one memset and in front of one fold; G is
 * the largest count with G * grid^2 < 2^32 whose private histogram copies (G * 512 * ceil(n_prims / 8) bytes; with d_escaped n_prims + 64
 * in place of n_prims: a source's escapes are counted in 64 more entries of each copy, not on the one word d_escaped[k]) fit option
 * "illum_scratch_bytes" (at least one source's worth is always used); the group's first index is added to first_source.
 * The option changes no result.  There is no parameter kernel in front and nothing is read on the host.
 * Scene state, capture rules and scratch ownership are those of rc_get_illumination_dirs_device: legal on a capturing stream that has run
 * the call eagerly once (one capture slot per group), and behind rc_refit_device_async, rc_rebuild_tlas_device_async or
 * rc_update_geometry_device_async on the same stream with no host wait.  A replay reads the CURRENT d_sources: lamps that move between
 * replays just work.  n_sources == 0, grid == 0 or an empty scene: success, nothing enqueued.
 * Errors, all before anything is enqueued and with the outputs untouched: RC_ERR_INVALID_ARGUMENT (NULL scene; NULL d_sources, d_counts or
 * d_rays while n_sources and grid are non-zero; grid >= 65536; row_stride < n_prims; first_source + n_sources > 2^32), RC_ERR_NOT_SYNCED
 * (as for rc_get_illumination_dirs_device).  A stack overflow is reported by rc_wait.
 * Register and scratch figures of the new kernel shells and the comparison with the composed path:
 * docs/EXPERIMENTS.md, "Illumination from point sources". */
int rc_point_source_rays_device(rc_scene* scene, const rc_ray* d_sources, uint32_t n_sources, uint32_t grid, uint64_t seed,
                                uint32_t first_source, rc_ray* d_rays, void* stream);
int rc_get_illumination_points_device(rc_scene* scene, const rc_ray* d_sources, uint32_t n_sources, uint32_t grid, uint64_t seed,
                                      uint32_t first_source, uint32_t* d_counts, uint64_t row_stride, uint32_t* d_escaped, void* stream);

/* ---- Radiosity between instances: the matrix of counts between PLACED primitives APPLIED TO A VECTOR, without the matrix -- the step of
 * B <- E + rho .* (M * B) ./ R per surface element of an INSTANCED scene.  rc_view_factor_products_device answers in metadata space: instances
 * of one mesh share metadata and its sources are shot from BLAS-local coordinates, so on an instanced scene it describes another scene.  This
 * call is its form in the index space of "Form factors between instances" (below): 1. the placed-primitive index space, q = base[i] + l,
 * P = base[n_inst]; 2. the placed ray -- the source is that family's, unchanged: the rays are bit for bit those of
 * rc_placed_view_factor_rays_device, with the same two samplings.  With sampling = RC_VF_SAMPLING_COSINE, M[a, b] / R estimates the Lambertian
 * form factor F_ab, so the iteration over placed primitives is the radiosity equation; RC_VF_SAMPLING_UNIFORM shoots the reference's
 * directions.
 * THE RULE, with no metadata in it.  Item w = placed primitive placed_begin + w / n_ray, ray ray_begin + w % n_ray, n_ray = the clamped ray
 * range's length.  a = the source's q.  For a hit, b = base[hit instance] + prim - 1.  A hit with b != a:
 *     mx [a] += x[b]        (M  x)[a]
 *     mtx[b] += x[a]        (M^T x)[b]
 * A miss: escaped[a] += 1.  A hit on the source itself adds nothing.  All adds are u64 modulo 2^64, exact in any order: any partition of
 * placed primitives x rays gives the same words.  d_x: P u32, indexed by q, read WHEN THE KERNEL RUNS and only for counted rays; d_x == NULL
 * means x = 1: mx is then the count of a source's rays that hit another placed primitive (the placed `emitted`) and mtx the placed
 * `received`, so the totals need no call of their own, and mx[a] + escaped[a] + the self hits of a = the rays of a.  d_mx, d_mtx, d_escaped:
 * P u64 each, every one may be NULL.  All outputs ACCUMULATE.
 * placed_end is clamped to P and ray_end to rays_per_triangle; an empty range, or all three outputs NULL, enqueues nothing.  d_mtx is the
 * hot vector: the kernel counts it into 16 private copies of P u64 while they fit option "placed_copy_bytes" (default 256 MiB: P <= 2 M) and a
 * fold adds them, and adds straight onto the caller's words above that -- P is 2 x 10^7 on a 4800-instance scene, where the copies would be
 * 2.5 GB: the same words either way.  d_mx and d_escaped are per source and are added onto the caller's words.  Scratch is per stream;
 * shards accumulate on one stream or concurrently on several.  Legal on a capturing stream that has run the call eagerly once, and behind
 * rc_update_transforms_device -> rc_refit_device_async (or the rebuilds) and behind rc_update_geometry_device_async on the same stream with
 * no host wait: a replay reads the CURRENT transforms and x.
 * Errors, all before anything is enqueued and with the outputs untouched: RC_ERR_INVALID_ARGUMENT (NULL scene; sampling above
 * RC_VF_SAMPLING_COSINE; P >= 2^32), RC_ERR_NOT_SYNCED in the states in which rc_placed_view_factor_groups_device returns it.  A stack
 * overflow is reported by rc_wait.
 * Register and scratch figures of the six new kernel shells: docs/EXPERIMENTS.md, "Radiosity between instances". */
int rc_placed_view_factor_products_device(rc_scene* scene, uint32_t rays_per_triangle, uint64_t seed, uint32_t sampling, uint32_t placed_begin,
                                          uint32_t placed_end, uint32_t ray_begin, uint32_t ray_end, const uint32_t* d_x, uint64_t* d_mx,
                                          uint64_t* d_mtx, uint64_t* d_escaped, void* stream);

/* ---- Sparse matrix between placed primitives: the matrix that rc_placed_view_factor_products_device applies, KEPT, as CSR -- the placed
 * form of rc_view_factors_sparse_device.  The products above retrace all P x R rays for every bounce; a solve of tens of bounces builds the
 * matrix once and then pays one pass over nnz x 8 bytes per bounce.  A placed row has at most min(R, P - 1) non-zeros, so the CSR exists
 * where P x P words cannot (P is 2 x 10^7 on a 4800-instance scene).
 * Mp[a, b] = the number of the R = rays_per_triangle placed rays of placed primitive a (bit for bit those of
 * rc_placed_view_factor_rays_device, either sampling) whose closest hit is placed primitive b = base[hit instance] + prim - 1 with b != a:
 * the rule of rc_placed_view_factor_products_device, no metadata in it.  Misses and hits on the source itself are in no entry; the diagonal
 * is empty.  It is what rc_placed_view_factor_groups_device counts with every placed primitive its own group.
 * The call OVERWRITES its outputs with rows [placed_begin, placed_end) of Mp (placed_end is clamped to P) under rc_view_factors_sparse_device's
 * contract: d_row_ptr holds rows + 1 u64 offsets starting at 0 and is always the true one, *d_nnz is the true count, entries below
 * `capacity` are the correct first entries, nothing is written at or beyond `capacity`, NULL d_cols / d_vals with capacity == 0 is the
 * counting call; d_cols (0-based placed primitive) strictly ascending within a row, every d_vals >= 1.  The arrays are a function of (scene,
 * rays_per_triangle, seed, sampling, row range) alone: the job is cut into chunks of whole consecutive rows whose rays x 8 bytes fit
 * option "vf_sparse_scratch_bytes" (a single larger row gets a chunk of its own), and neither the option nor the shape of any kernel
 * changes a word.  Row blocks of a partition of [0, P) concatenate.
 * THE MATRIX IS A SNAPSHOT.  The build reads the instances' transforms as they are WHEN ITS KERNELS RUN.  After the instances move (or the
 * geometry deforms) the arrays still describe the OLD placement; nothing tracks that, and rebuilding the matrix is the caller's job.
 * THE PRODUCTS are rc_view_factor_sparse_products_device, which reads only the arrays: n_rows = the block's rows, row_offset = placed_begin,
 * x and the outputs of length P.  With the CSR of the same (rays_per_triangle, seed, sampling) its sums equal
 * rc_placed_view_factor_products_device's d_mx and d_mtx bit for bit.  There is no host-array form.
 * Everything runs on the caller's stream with no host wait between the steps; scratch is per stream, two streams may build at once.  Legal
 * behind rc_update_transforms_device -> rc_refit_device_async (or the rebuilds) and behind rc_update_geometry_device_async on the same
 * stream with no host wait.  NOT capturable: RC_ERR_NOT_SYNCED on a stream that is being captured.
 * Errors, all before anything is enqueued and with the outputs untouched: RC_ERR_INVALID_ARGUMENT (NULL scene, d_row_ptr or d_nnz; NULL
 * d_cols / d_vals with capacity > 0; sampling above RC_VF_SAMPLING_COSINE; P >= 2^32; a chunk whose rays reach 2^32 or whose keys need
 * more than 64 bits), RC_ERR_NOT_SYNCED in the states in which rc_placed_view_factor_products_device returns it.  A stack overflow is
 * reported by rc_wait.
 * Register and scratch figures of the six new kernel shells and the measured build, product and break-even figures:
 * docs/EXPERIMENTS.md, "Sparse matrix between placed primitives". */
int rc_placed_view_factors_sparse_device(rc_scene* scene, uint32_t rays_per_triangle, uint64_t seed, uint32_t sampling, uint32_t placed_begin,
                                         uint32_t placed_end, uint64_t* d_row_ptr, uint32_t* d_cols, uint32_t* d_vals, uint64_t capacity,
                                         uint64_t* d_nnz, void* stream);

/* ---- Placed final gather: carry a solution per PLACED primitive to the hit points.  The placed family (rc_placed_view_factor_groups_device,
 * rc_placed_view_factor_products_device, rc_placed_view_factors_sparse_device and the bounce solves on them) returns one value per placed
 * primitive q = base[i] + l (section 1 of "Form factors between instances" below).  rc_final_gather_device (the next block) cannot read
 * such a vector: it indexes x by metadata - 1, and every instance of a mesh shares its metadata.  These two calls index by q instead: two
 * instances of one mesh carry different values.
 *
 * rc_placed_hit_indices_device, a stage: d_q[i] = base[d_hits[i].instance_id] + (d_hits[i].primitive_id - the first flat primitive of
 * that instance's BLAS) for a record with hit != 0, RC_INVALID_ID for a record with hit == 0.  d_hits: n records, d_q: n u32.  The radiosity
 * of the surface a camera ray sees is B[d_q[i]], one gather on the caller's side; applied to the hit records of
 * rc_ambient_occlusion_rays_device's rays (declared last in this header) it is the lookup step of the composed path.
 * One kernel, no scratch; legal wherever
 * rc_hit_points_device is, a capturing stream and the same stream behind the device-side updates included.  Records that were not written
 * by this library's closest-hit calls are outside the contract, as for rc_hit_points_device.  Errors: rc_hit_points_device's
 * (RC_ERR_INVALID_ARGUMENT for a NULL scene, d_hits or d_q, also with n == 0; RC_ERR_NOT_SYNCED in the same states), and
 * RC_ERR_INVALID_ARGUMENT on a scene whose P >= 2^32.
 *
 * rc_placed_final_gather_device, the fused driver: rc_final_gather_device's contract everywhere except the lookup rule.  The same items
 * (j = i * samples + s), the same rays -- ray(i, s) is bit for bit the ray rc_ambient_occlusion_rays_device writes at slot i * samples + s --,
 * the same d_rays, d_hits, n, samples, max_dist, seed, depth, d_path_in, path_base, bias and miss_value.  d_x: P u32 indexed by q, P the
 * scene's placed-primitive count, read WHEN THE KERNEL RUNS and for counted samples only: a captured call follows a solution that changes
 * between replays.  d_sum: n u64.  d_open: n u32, may be NULL.
 * Identity with the composed path (the rays, rc_trace_closest_device, rc_placed_hit_indices_device on the sample hits, a lookup and a
 * sum), exact, no tolerance, and with no metadata in it:
 *   d_sum[i]  += sum over s of  live(i,s) && H.hit ? x[base[H.instance_id] + l(H)]  :  live(i,s) && !H.hit ? miss_value : 0
 *   d_open[i] += sum over s of  live(i,s) && !H.hit
 * where live(i,s) and H are rc_final_gather_device's, and l(H) is the hit's 0-based position inside its instance's BLAS: the traversal core
 * reports prim = l + 1, so the index is base[instance] + prim - 1, one load where the metadata rule reads two.  EVERY hit is counted: the
 * index is below P always, there is no "outside 1..N" case.  Sums are modulo 2^64: integer adds, exact in any order, so the words do not
 * depend on scheduling, kernel shape or sharding.
 * Consequences: d_open equals what rc_final_gather_device and rc_ambient_occlusion_device add for the same arguments; and on a scene whose
 * metadata lies in 1..N the call with x_placed[q] = x[metadata(q) - 1] gives rc_final_gather_device's words for x.
 * x IS WHATEVER THE CALLER HANDS IN.  Nothing tracks whether the instances moved since a placed solution was made; a solution per placed
 * primitive keeps its meaning while base does, and base changes only in the rebuilding rc_sync.  Until the illumination drivers count per
 * placed primitive the caller supplies the emission of a placed solve itself (one value per instance expanded over the bases, say).
 * The call ACCUMULATES into d_sum and d_open: the caller zeroes them, and accumulation over calls with different `seed` or `depth` is
 * legal.  Items are claimed in natural order; the entry cull follows rc_trace_closest_device.
 * No allocation, copy, event, memset, host synchronisation or scene-owned scratch: re-entrant across streams, and captured on a capturing
 * stream under the rules of the other driver launches (one capture slot; the stream must have run the call eagerly before).  Legal behind
 * rc_update_transforms_device -> rc_refit_device_async (or the rebuilds) and behind rc_update_geometry_device_async on the same stream
 * with no host wait: base does not change there, and a replay reads the CURRENT scene and the current x.  A stack overflow is reported by
 * rc_wait.  n == 0 or samples == 0: succeeds, nothing is enqueued.
 * Errors, all before anything is enqueued, rc_final_gather_device's in its order: RC_ERR_INVALID_ARGUMENT (NULL scene, checked first and
 * with or without a device; samples >= 65536; depth >= 65536; max_dist not > 0 -- NaN included, +Inf is legal; n * samples >= 2^32,
 * products that wrap in 64 bits included; NULL d_rays, d_hits, d_sum or d_x while there is work), RC_ERR_NOT_SYNCED (the rules of
 * rc_shadow_visibility_device).  Then RC_ERR_INVALID_ARGUMENT for P >= 2^32: it sits where rc_placed_view_factor_products_device checks
 * it, behind the device and the sync state, and no test can reach it (such a scene does not fit a device).
 * Register and scratch figures of the new kernel shells and the cost against rc_final_gather_device:
 * docs/EXPERIMENTS.md, "Placed final gather". */
int rc_placed_hit_indices_device(rc_scene* scene, const rc_hit* d_hits, uint64_t n, uint32_t* d_q, void* stream);
int rc_placed_final_gather_device(rc_scene* scene, const rc_ray* d_rays, const rc_hit* d_hits, uint64_t n, uint32_t samples, float max_dist,
                                  uint64_t seed, uint32_t depth, const uint32_t* d_path_in, uint64_t path_base, float bias,
                                  const uint32_t* d_x, uint32_t miss_value, uint64_t* d_sum, uint32_t* d_open, void* stream);

/* ---- Final gather: how much of a per-triangle solution arrives at every hit point?  The step between the analysis half (a u32 per
 * primitive indexed by metadata - 1: rc_view_factor_products_device's x, a radiosity iterate) and the per-hit half: the hemisphere samples of
 * rc_ambient_occlusion_device (declared below), traced for the CLOSEST hit -- closest_hit, src/instanced-bvh.jl:1902-2024 -- and the field
 * summed over what they hit.  The samples are cosine-weighted (cosine_sample_hemisphere, src/math.jl:1-21), so sum / samples is the
 * cosine-weighted mean of x over the hemisphere: the irradiance in x's units when x is a Lambertian radiosity.
 * d_rays, d_hits, n, samples, max_dist, seed, depth, d_path_in, path_base, bias: rc_ambient_occlusion_device's, and ray(i, s) is bit for
 * bit the ray rc_ambient_occlusion_rays_device writes at slot i * samples + s (the same device function makes both); there is no ray stage
 * of its own.  d_x: n_primitives u32, indexed by metadata - 1, read WHEN THE KERNEL RUNS and for counted samples only: a captured call
 * follows a solution that changes between replays.  d_sum: n u64.  d_open: n u32, may be NULL.  miss_value: what a sample that escapes
 * adds (the sky's radiance in x's units; 0: no sky).
 * Identity with the composed path, exact, no tolerance, N = the scene's primitive count:
 *   d_sum[i]  += sum over s of  live(i,s) && H.hit && 1 <= m <= N ? x[m-1]  :  live(i,s) && !H.hit ? miss_value : 0
 *   d_open[i] += sum over s of  live(i,s) && !H.hit
 * where live(i,s) = d_hits[i].hit && ray(i,s).t_max > 0, H is what rc_trace_closest_device reports for ray(i,s), and m is the metadata of
 * the primitive H names.  A hit whose metadata lies outside 1..N adds nothing (the rule of get_illumination, src/kernels.jl:123).  Sums are
 * modulo 2^64: integer adds, exact in any order, so the words do not depend on scheduling, kernel shape or sharding.
 * Two consequences: d_open equals what rc_ambient_occlusion_device adds to d_count for the same arguments -- on these rays (t_min = 0)
 * closest_hit and any_hit agree on whether there is a hit --; and a hit whose frame is NaN gets NO extra gate, as there: its NaN ray is
 * traced and counts as whatever rc_trace_closest_device reports for it, the same in both paths.
 * The call ACCUMULATES into d_sum and d_open: the caller zeroes them, and accumulation over calls with different `seed` or `depth` is
 * legal.  Items are claimed in natural order; the entry cull follows rc_trace_closest_device.
 * No allocation, copy, event, memset, host synchronisation or scene-owned scratch: re-entrant across streams, and captured on a capturing
 * stream under the rules of the other driver launches (one capture slot; the stream must have run the call eagerly before).  A stack
 * overflow is reported by rc_wait.  n == 0 or samples == 0: succeeds, nothing is enqueued.
 * Errors, all before anything is enqueued and in rc_ambient_occlusion_device's order: RC_ERR_INVALID_ARGUMENT (NULL scene, checked first
 * and with or without a device; samples >= 65536; depth >= 65536; max_dist not > 0 -- NaN included, +Inf is legal; n * samples >= 2^32,
 * products that wrap in 64 bits included; NULL d_rays, d_hits, d_sum or d_x while there is work), RC_ERR_NOT_SYNCED (the rules of
 * rc_shadow_visibility_device).
 * Measured against the composed path in docs/EXPERIMENTS.md, "Final gather". */
int rc_final_gather_device(rc_scene* scene, const rc_ray* d_rays, const rc_hit* d_hits, uint64_t n, uint32_t samples, float max_dist,
                           uint64_t seed, uint32_t depth, const uint32_t* d_path_in, uint64_t path_base, float bias,
                           const uint32_t* d_x, uint32_t miss_value, uint64_t* d_sum, uint32_t* d_open, void* stream);

/* ---- Form factors between instances: view-factor sources in WORLD space.  The view-factor family above shoots its rays from the
 * untransformed primitives of each BLAS, as the reference does (src/kernels.jl:80-104): on a scene of one identity instance that is the
 * scene, on every other scene the sources are not where the tracer sees the bodies.  These four calls place every source by its
 * instance and name every hit by (instance, primitive): "how much of body A's emission reaches body B" is one launch, the bodies may be
 * instances of one mesh, and the call may run behind a device-side move of B with no host wait.
 * 1. THE PLACED-PRIMITIVE INDEX SPACE.  A placed primitive is a pair (instance i, local primitive l).  i is the 0-based position in the
 *    instance array: rc_export_instances' order and rc_hit::instance_id.  l is the 0-based position inside the instance's BLAS in its
 *    sorted order: the flat index is prims_offset(i) + l, and the traversal core reports prim = l + 1.  Its index is q = base[i] + l, where
 *    base is the exclusive prefix sum of the instances' primitive counts over the instance array; P = base[n_inst] is the scene's
 *    placed-primitive count.  base (n_inst + 1 u32) is built by the rebuilding rc_sync -- structure changes only there; device-side
 *    transform and geometry updates keep every count: rc_update_geometry_device_async commits only on an equal face count --, kept on the
 *    host and on the device, and re-derived by rc_scene_load.  A scene whose P reaches 2^32 keeps working for everything else; these
 *    four calls return RC_ERR_INVALID_ARGUMENT on it.
 * 2. THE PLACED RAY of (q, ray index, seed, sampling).  World triangle: p_k = transform_point(T_i, v_k) in f32, per row
 *    ((m0 * x + m1 * y) + m2 * z) + m3, no contraction; T_i is the instance's FORWARD `transform` as it is in device memory WHEN THE
 *    KERNEL RUNS.  Ray: exactly the ray of rc_view_factor_sampled_rays_device applied to (p_1, p_2, p_3): the normal is that of the
 *    transformed vertices in their order -- a mirroring instance flips it, a non-uniform scale bends it correctly --, the origin is
 *    pt + normal * 0.01f in WORLD units, the samplings are the same two.  Philox counter: (ray_idx, flat primitive index, i, 0), key =
 *    seed; word 2 is the only difference from the per-triangle family, so instance 0 with an identity transform draws the sibling's
 *    numbers.  THE CALLER'S CONTRACT: sources are placed by `transform`, hits are found through `inv_transform`; a caller who supplied
 *    an inverse of its own (rc_add_instances_with_inverse) owns their agreement.  Singular transforms are outside the contract, as
 *    everywhere else.
 * 3. THE RULE, with no metadata in it.  a = the source's q.  For a hit, b = base[hit instance] + prim - 1.  ga = groups[a], gb = groups[b],
 *    wa = weights ? weights[a] : 1.  A source with ga >= G contributes nothing.  A miss: escaped[ga] += wa, if escaped is given.  A hit
 *    with b != a and gb < G: matrix[ga * G + gb] += wa.  Any other hit adds nothing.  u64 modulo 2^64, exact in any order: any partition
 *    of placed primitives x rays gives the same words.  d_groups / d_weights: P u32 each, indexed by q, read WHEN THE KERNEL RUNS.  Both
 *    outputs ACCUMULATE.
 *
 * rc_placed_primitive_bases: the host copy of base; *count = n_inst + 1, out may be NULL to ask for the count, capacity in words (the
 * idiom of the exports).
 * rc_placed_triangles_device: 9 f32 per placed primitive for [placed_begin, placed_begin + n), the world triangle of 2. -- for areas, for a
 * model on the host, for a caller's own kernels.  One kernel, no scratch.
 * rc_placed_view_factor_rays_device, the composed stage, sibling of rc_view_factor_sampled_rays_device: writes the placed rays
 * [ray_begin, ray_begin + n_rays) of placed primitive placed_prim.  The output feeds rc_trace_closest_device unchanged.
 * rc_placed_view_factor_groups_device, the fused driver, sibling of rc_view_factor_groups_device.  WORK-ITEM LAYOUT: item w = placed
 * primitive placed_begin + w / n_ray, ray ray_begin + w % n_ray, n_ray = the clamped ray range's length; the ray is generated when a lane
 * takes the item -- bit for bit the stage's, the same device function makes both -- and never stored.  placed_end is clamped to P and
 * ray_end to rays_per_triangle; an empty range enqueues nothing.  1 <= n_groups <= 65535.  d_matrix: G * G u64, row = the source's group;
 * d_escaped: G u64, may be NULL.  The kernel counts into private copies of the G * G (+ G) words while they fit 256 MiB and a fold adds
 * them, and adds straight onto the caller's words above that: the same words either way.  Scratch is per stream.  Legal on a capturing
 * stream that has run the call eagerly once, and behind rc_update_transforms_device -> rc_refit_device_async (or the rebuilds) and
 * behind rc_update_geometry_device_async on the same stream with no host wait: a replay reads the CURRENT transforms, groups and weights.
 * Errors, all before anything is enqueued and with the outputs untouched: RC_ERR_INVALID_ARGUMENT (NULL scene, d_groups, d_matrix, d_rays,
 * or d_verts with n != 0; sampling above RC_VF_SAMPLING_COSINE; n_groups outside 1..65535; placed_prim >= P; placed_begin + n > P;
 * capacity below n_inst + 1; P >= 2^32), RC_ERR_NOT_SYNCED in the states in which rc_view_factor_groups_device returns it.  A stack
 * overflow is reported by rc_wait.
 * The placed totals, products and bounce solve: rc_placed_view_factor_products_device ("Radiosity between instances", declared ahead of the
 * final gather); the matrix itself as CSR: rc_placed_view_factors_sparse_device (declared behind it).  A placed form of the dense matrix
 * does not exist yet.
 * Register and scratch figures of the new kernel shells and the cost against the sibling: docs/EXPERIMENTS.md, "Form factors between
 * instances". */
int rc_placed_primitive_bases(rc_scene* scene, uint32_t* out, uint32_t capacity, uint32_t* count);
int rc_placed_triangles_device(rc_scene* scene, uint32_t placed_begin, uint32_t n, float* d_verts, void* stream);
int rc_placed_view_factor_rays_device(rc_scene* scene, uint64_t seed, uint32_t sampling, uint32_t placed_prim, uint32_t ray_begin,
                                      uint32_t n_rays, rc_ray* d_rays, void* stream);
int rc_placed_view_factor_groups_device(rc_scene* scene, uint32_t rays_per_triangle, uint64_t seed, uint32_t sampling, uint32_t placed_begin,
                                        uint32_t placed_end, uint32_t ray_begin, uint32_t ray_end, const uint32_t* d_groups, uint32_t n_groups,
                                        const uint32_t* d_weights, uint64_t* d_matrix, uint64_t* d_escaped, void* stream);

/* ---- Ambient occlusion: how open is the hemisphere above every hit?  `samples` cosine-weighted any_hit rays of length max_dist per hit; the
 * visible fraction count / samples is the cosine-weighted openness of the point (with max_dist = +Inf its sky-view factor, the per-point form
 * of what rc_get_illumination_device and rc_view_factor_totals answer per triangle).
 * d_rays / d_hits: the closest-hit stage's n rays and hit records.  d_path_in (may be NULL) / path_base: the path of slot i is
 * path_base + (d_path_in ? d_path_in[i] : i), exactly as in rc_bounce_rays_device: a compacted, chunked or sharded queue draws the same
 * samples for the same path.
 * Sample s of slot i, every expression evaluated left to right in f32 with no contraction:
 *   (p, nn) = the hit point and flipped geometric normal of slot i (rc_hit_points_device's)
 *   rnd = Philox4x32-10, counter (lo32 path, hi32 path, s, 0x414F0000 | depth), key = (lo32 seed, hi32 seed)
 *   u1, u2 = its first two words as 24-bit floats in [0, 1): (word >> 8) * 2^-24, the conversion of rc_bounce_rays_device
 *   d = the cosine-weighted direction about nn that rc_bounce_rays_device makes from (nn, u1, u2): the same function, not renormalised
 *   ray(i, s) = origin p + nn * bias, t_min 0, direction d, t_max max_dist.
 * A sample depends on (seed, path, depth, s) only -- not on n, the slot or `samples`: raising `samples` keeps the earlier ones.
 *
 * rc_ambient_occlusion_rays_device, the composed stage: writes n * samples rays, ray(i, s) at slot i * samples + s; a slot whose primary ray
 * missed gets rc_shadow_rays_device's dummy ray (d = (0,0,1), t_max = 0).  The output feeds rc_trace_any_device unchanged.
 * rc_ambient_occlusion_device, the fused driver: one persistent any_hit launch over all (hit, sample) items, the rays generated when a lane
 * takes an item and never stored.  d_count: n u32.  Identity with the composed path, exact, no tolerance:
 *   d_count[i] += sum over s of (d_hits[i].hit && ray(i, s).t_max > 0 && !any_hit(ray(i, s)).hit),
 * where ray(i, s) is bit for bit what rc_ambient_occlusion_rays_device writes (the same device function makes both) and any_hit is what
 * rc_trace_any_device reports for it.  t_max = max_dist > 0 for every slot that hit, so the middle term only excludes the dummy ray of a
 * missed primary ray, which costs no traversal.  A hit whose frame is NaN (a singular instance transform, say) has a NaN origin or
 * direction but t_max = max_dist > 0: NO extra gate applies, it is traced and counts as whatever rc_trace_any_device reports for that ray,
 * the same in both paths.
 * The call ACCUMULATES into d_count (the convention of rc_soft_shadow_visibility_device): the caller zeroes it, and progressive
 * accumulation over calls with different `seed` or `depth` is legal.  Each visible sample is one relaxed device-scope u32 atomic add;
 * integer adds are exact in any order, so the counts are reproducible.  Items are claimed in natural order; the entry cull follows
 * rc_trace_any_device (off unless option "entry_cull" is 2).
 * No allocation, copy, event, memset, host synchronisation or scene-owned scratch: re-entrant across streams, and captured on a capturing
 * stream under the rules of the other driver launches (one capture slot; the stream must have run the call eagerly before).  A stack
 * overflow is reported by rc_wait.  n == 0 or samples == 0: succeeds, nothing is enqueued.
 * Errors, all before anything is enqueued: RC_ERR_INVALID_ARGUMENT (NULL scene, checked first and with or without a device; NULL d_rays,
 * d_hits or output while there is work; n * samples >= 2^32, products that wrap in 64 bits included; samples >= 65536; depth >= 65536;
 * max_dist not > 0 -- NaN included, +Inf is legal), RC_ERR_NOT_SYNCED (the rules of rc_shadow_visibility_device).
 * Measured against the composed path in docs/EXPERIMENTS.md, "Ambient occlusion". */
int rc_ambient_occlusion_rays_device(rc_scene* scene, const rc_ray* d_rays, const rc_hit* d_hits, uint64_t n, uint32_t samples,
                                     float max_dist, uint64_t seed, uint32_t depth, const uint32_t* d_path_in, uint64_t path_base,
                                     float bias, rc_ray* d_ao_rays, void* stream);
int rc_ambient_occlusion_device(rc_scene* scene, const rc_ray* d_rays, const rc_hit* d_hits, uint64_t n, uint32_t samples, float max_dist,
                                uint64_t seed, uint32_t depth, const uint32_t* d_path_in, uint64_t path_base, float bias,
                                uint32_t* d_count, void* stream);

#ifdef __cplusplus
}
#endif
#endif
