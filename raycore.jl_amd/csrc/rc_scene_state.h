// rc_scene_state.h -- the host-side state flags of a mutable scene (rc_scene::state, rc_internal.h): what every entry point may trust, and
// the named transitions that are the only writers.  No HIP header: a plain host compiler builds it (tests/host/scene_state_main.cpp, which
// drives it beside tests/lifecycle_model.py on a CPU).  Which lock is held where is the callers' business, as is the stream an eager
// asynchronous call ran on (rc_scene::async_stream); per-geometry state (Blas::root_on_device, Blas::n_nodes4) stays with the geometry.
// Invariant: host_instances_stale implies !mirror_edited (a mirror the device has overtaken holds no edits of its own).
#pragma once

enum class RcSyncPlan { Noop, RefitFromDevice, Rebuild, RefitUpload };  // what rc_sync does; last_sync_action reports 0, 1, 2, 1

struct RcSceneFlags {  // snapshot(): the flags as plain data, for the test
    bool dirty = true, transforms_dirty = false, has_static = false, mirror_edited = false, device_dirty = false, host_instances_stale = false;
    bool bound_stale = false, blas_bounds_stale = false, captured_update = false, captured_refit = false, captured_deform = false;
    bool async_pending = false, quality_armed = false, flat_attrs_valid = false, vf_order_valid = false;
};

class RcSceneState {
    // dirty: structural host edits wait for a rebuilding rc_sync.  transforms_dirty: transforms, host-side or device-side, wait for a commit.
    // has_static: a rebuilding rc_sync has run.
    // mirror_edited: the host mirror of the instances holds edits the device lacks.  device_dirty: the DEVICE descriptors are newer than the
    // last refit, and the update kernel has written the per-instance data.  host_instances_stale: the device descriptors are newer than
    // the mirror.
    // bound_stale / blas_bounds_stale: the world bound / the BLAS root boxes on the device are newer than the host copies.
    // captured_update / captured_refit / captured_deform: that call was captured into a graph that may still live -- its replays happen
    // unseen, so what they rewrite is re-read from the device on every use.
    // async_pending: an EAGER asynchronous call was enqueued on rc_scene::async_stream and nobody has waited for it.
    // quality_armed: the device's RcTlasQuality::cost_built describes the tree the device holds.
    // flat_attrs_valid / vf_order_valid: the derived caches (flat attribute array, view-factor source order) match the flat primitives.
    RcSceneFlags f;

public:
    RcSceneFlags snapshot() const { return f; }

    // ---- gates and plans
    // Every query and rc_instance_buffer_device / rc_refit_device: refused (RC_ERR_NOT_SYNCED) with anything pending, host-side or device-side
    bool synced() const { return f.has_static && !f.dirty && !f.transforms_dirty; }
    // The asynchronous device-side mutations write the arrays where the last rc_sync put them: nothing the host holds may be pending
    bool device_resident() const { return f.has_static && !f.dirty && !f.mirror_edited; }
    bool tlas_present() const { return f.has_static; }
    // (captured_update: the mirror is pulled on every use -- unless it holds edits of its own that the next rc_sync has yet to upload)
    bool mirror_needs_pull() const { return f.host_instances_stale || (f.captured_update && f.has_static && !f.mirror_edited); }
    bool world_bound_needs_read() const { return f.bound_stale || f.captured_refit; }  // while true, a driver that needs the bound fails on a capturing stream
    bool blas_bounds_need_read() const { return f.blas_bounds_stale || f.captured_deform; }
    bool deform_captured() const { return f.captured_deform; }
    bool flat_attrs_current() const { return f.flat_attrs_valid; }
    bool vf_order_current() const { return f.vf_order_valid && !f.captured_deform; }
    // true: the descriptors were rewritten through rc_instance_buffer_device and the per-instance data is derived from them by the commit;
    // false: every change since the last refit came through rc_update_transforms_device, whose kernel has already written it
    bool commit_needs_per_instance_pass() const { return !f.device_dirty; }
    bool async_work_pending() const { return f.async_pending; }
    bool quality_is_armed() const { return f.quality_armed; }
    RcSyncPlan sync_plan() const {
        if (!f.dirty && !f.transforms_dirty && f.has_static) return RcSyncPlan::Noop;
        // rc_update_transforms_device since the last refit: the device descriptors are the new ones and the mirror is stale -- refit from them
        if (f.has_static && !f.dirty && f.device_dirty && f.host_instances_stale) return RcSyncPlan::RefitFromDevice;
        if (f.dirty || !f.has_static) return RcSyncPlan::Rebuild;
        return RcSyncPlan::RefitUpload;  // the mirror equals the device or holds the newer edits: it is uploaded
    }

    // ---- host mutations (each after the mirror was pulled: every reader / editor of the mirror does that first)
    void structural_edit() { f.dirty = true; }  // delete, geometry and mesh update, load
    void instances_pushed() { f.mirror_edited = true; f.dirty = true; }
    void transforms_edited() { f.mirror_edited = true; f.transforms_dirty = true; }  // rc_update_transforms
    void mirror_pulled() { f.host_instances_stale = false; }  // (device_dirty stays: a read of the mirror is no mutation, the update still waits for its refit)

    // ---- rc_sync
    void synced_by(RcSyncPlan plan) {
        if (plan == RcSyncPlan::Noop) return;
        if (plan == RcSyncPlan::Rebuild) { f.dirty = false; f.has_static = true; }
        f.transforms_dirty = false;
        if (plan != RcSyncPlan::RefitFromDevice) f.mirror_edited = false;  // the device holds what the mirror holds
        f.device_dirty = false;
    }
    // rc_build_tlas, in three steps with work that can fail in between.  Begun: the flat arrays are about to be replaced, the caches derived
    // from them are void
    void tlas_build_begun() { f.flat_attrs_valid = false; f.vf_order_valid = false; }
    // ... the flat arrays are in place (rc_sync refreshed the host's root boxes before the rebuild read them).  A graph that captured an
    // update, refit or geometry update of the old arrays is dead: its addresses are gone.  The quality block is zeroed beside this.  An
    // empty scene has its (empty) world bound at once; any other gets it from the built tree (world_bound_read)
    void tlas_built(bool empty) {
        f.captured_update = f.captured_refit = f.captured_deform = false;
        f.blas_bounds_stale = false;
        f.quality_armed = false;
        if (empty) f.bound_stale = false;
    }
    // rc_refit_tlas keeps the descriptors the device holds (rc_instance_buffer_device + rc_refit_device, the refit-from-device rc_sync)
    // instead of uploading the mirror; either refit ends with world_bound_read
    void refit_from_device_begun() { f.host_instances_stale = true; }

    // ---- device side: the calls were enqueued on a caller's stream; `capturing`: into a graph
    void device_update_enqueued() { f.host_instances_stale = f.device_dirty = f.transforms_dirty = true; }  // rc_update_transforms_device, the geometry updates
    void device_commit_enqueued() { f.device_dirty = f.transforms_dirty = false; }  // a refit / rebuild commits the updates so far
    void instances_updated_async(bool capturing) { if (capturing) f.captured_update = true; }
    // refit, rebuild and gated commit alike: every replay moves the root box again, so the host copy is never trusted while the graph may live
    void tlas_committed_async(bool capturing) {
        f.host_instances_stale = true;
        f.bound_stale = true;
        if (capturing) f.captured_refit = true;
    }
    void geometry_updated_async(bool capturing) {  // the root boxes in d_descs are newer than descs / Blas::root_min,max
        f.blas_bounds_stale = true;
        if (capturing) f.captured_deform = true;
    }
    void vf_order_invalidated() { f.vf_order_valid = false; }
    void quality_armed_now() { f.quality_armed = true; }  // the first rc_refit_or_rebuild_tlas_async after a rebuilding rc_sync
    void async_noted(bool capturing) { if (!capturing) f.async_pending = true; }  // (replays are the caller's to wait for)
    // rc_wait_async_mutations synchronised the stream: the host-buffer queries, the mirror pull, the bound read-backs, rc_sync, rc_refit_device
    // and rc_scene_destroy call it first
    void async_waited() { f.async_pending = false; }

    // ---- lazy read-backs and caches
    void world_bound_read() { f.bound_stale = false; }  // rc_ensure_world_bound; rc_build_tlas and rc_refit_tlas read the root themselves
    void blas_bounds_read() { f.blas_bounds_stale = false; }  // rc_ensure_blas_bounds
    void flat_attrs_built() { f.flat_attrs_valid = true; }
    void vf_order_built() { f.vf_order_valid = true; }

    // ---- option "release_captures": the caller's graphs are gone
    void captures_released() {
        if (f.captured_refit) { f.captured_refit = false; f.bound_stale = true; }  // (no replay can move the root box any more: one more read-back settles it)
        if (f.captured_deform) { f.captured_deform = false; f.blas_bounds_stale = true; f.vf_order_valid = false; }  // (one more read-back / sort settles them)
        if (f.captured_update) { f.captured_update = false; f.host_instances_stale = f.host_instances_stale || !f.mirror_edited; }
    }
};
