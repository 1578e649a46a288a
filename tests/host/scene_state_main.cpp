// Stand-alone driver of RcSceneState (raycore.jl_amd/csrc/rc_scene_state.h), the host-side state flags of a mutable scene.  One entry point
// per line on stdin, "name [empty|capturing|gone]"; for each the state is driven the way the library's entry point of that name drives it --
// the gate first, then the transitions in the entry point's order -- and one line is printed: ok, not_synced, or for sync its action.
// tests/test_scene_state.py feeds the walks of tests/lifecycle_model.py and compares every line with the model.  No HIP, no GPU.
//   empty      the scene holds no instance: the builds, refits and asynchronous commits return before they touch a flag
//   capturing  the caller's stream is being captured into a graph
//   gone       rc_delete of a handle that is not live: nothing happens
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "rc_scene_state.h"

namespace {
RcSceneState st;

// ---- the library's helpers (rc_capi.hip, rc_build.hip, rc_drivers.hip), flags only
void wait_async() { if (st.async_work_pending()) st.async_waited(); }                       // rc_wait_async_mutations
void pull_mirror() { if (st.mirror_needs_pull()) { wait_async(); st.mirror_pulled(); } }     // sync_host_instances
void ensure_world_bound() { if (st.world_bound_needs_read()) { wait_async(); st.world_bound_read(); } }
void ensure_blas_bounds() { if (st.blas_bounds_need_read()) { wait_async(); st.blas_bounds_read(); } }
void ensure_vf_order() { if (!st.vf_order_current()) { wait_async(); st.vf_order_built(); } }
bool ensure_flat_attrs() {  // false: refused while a graph that captured a geometry update may live
    if (st.flat_attrs_current()) return true;
    if (st.deform_captured()) return false;
    wait_async();
    st.flat_attrs_built();
    return true;
}
void build_tlas(bool empty) {
    st.tlas_build_begun();
    st.tlas_built(empty);
    if (!empty) st.world_bound_read();
}
void refit_tlas(bool from_device, bool empty) {
    if (empty) return;
    if (from_device) st.refit_from_device_begun();
    st.world_bound_read();
}
void note_async(bool capturing) { st.async_noted(capturing); }

const char* sync_scene(bool empty) {
    const RcSyncPlan plan = st.sync_plan();
    if (plan == RcSyncPlan::Noop) return "noop";
    if (plan == RcSyncPlan::RefitFromDevice) {
        wait_async();
        refit_tlas(true, empty);
    } else {
        pull_mirror();
        if (plan == RcSyncPlan::Rebuild) { ensure_blas_bounds(); build_tlas(empty); }
        else refit_tlas(false, empty);
    }
    st.synced_by(plan);
    return plan == RcSyncPlan::Rebuild ? "rebuild" : "refit";
}

// "ok" / "not_synced" / the sync action; nullptr: unknown entry point
const char* run(const std::string& name, bool empty, bool capturing, bool gone) {
    const char* const ok = "ok";
    const char* const refused = "not_synced";
    // host mutations: the mirror is pulled before it is edited
    if (name == "add_blas" || name == "counts" || name == "wait" || name == "graph_launch") return ok;  // no flag is written (counts reads tlas_present(); a replay never enters the library)
    if (name == "add_instances") { pull_mirror(); st.instances_pushed(); return ok; }
    if (name == "update_transforms") { pull_mirror(); st.transforms_edited(); return ok; }
    if (name == "update_geometry") { pull_mirror(); st.structural_edit(); return ok; }  // rc_update_geometry, rc_update_geometry_mesh
    if (name == "delete") { if (!gone) st.structural_edit(); return ok; }
    if (name == "sync") return sync_scene(empty);
    // readers without a gate
    if (name == "get_instances") { pull_mirror(); return ok; }
    if (name == "world_bound") { ensure_world_bound(); return ok; }
    // readers of the synced scene
    if (name == "export_instances") { pull_mirror(); return st.synced() ? ok : refused; }
    if (name == "scene_save") {
        pull_mirror();
        if (!st.synced()) return refused;
        ensure_world_bound();
        ensure_blas_bounds();
        return ok;
    }
    if (name == "instance_buffer_device" || name == "trace_device" || name == "export_host" || name == "trace_host" || name == "collide_instances" ||
        name == "export_blas_descs" || name == "export_triangles" || name == "shading_attributes_device" || name == "view_factor_totals" ||
        name == "view_factors" || name == "refit_device") {
        if (!st.synced()) return refused;
        if (name == "instance_buffer_device" || name == "trace_device") return ok;
        if (name == "export_blas_descs") { ensure_blas_bounds(); return ok; }
        if (name == "shading_attributes_device") return ensure_flat_attrs() ? ok : refused;
        wait_async();  // the host-buffer queries (require_synced_host), rc_refit_device, the multi-device calls' check_same_geometry
        if (name == "export_triangles") return ensure_flat_attrs() ? ok : refused;
        if (name == "view_factor_totals" || name == "view_factors") ensure_world_bound();
        if (name == "view_factors") ensure_vf_order();
        if (name == "refit_device") refit_tlas(true, empty);
        return ok;
    }
    // the asynchronous device-side entry points: nothing the host holds may be pending
    if (name == "tlas_quality") { if (!st.device_resident()) return refused; wait_async(); return ok; }
    if (name == "update_transforms_device") {
        if (!st.device_resident()) return refused;
        st.instances_updated_async(capturing);
        note_async(capturing);
        st.device_update_enqueued();
        return ok;
    }
    if (name == "update_geometry_device") {  // rc_update_geometry_device_async, rc_update_mesh_vertices_device_async
        if (!st.device_resident()) return refused;
        st.geometry_updated_async(capturing);
        note_async(capturing);
        st.vf_order_invalidated();
        st.device_update_enqueued();
        return ok;
    }
    if (name == "refit_device_async" || name == "rebuild_tlas_device_async" || name == "refit_or_rebuild_tlas_device_async") {
        if (!st.device_resident()) return refused;
        (void)st.commit_needs_per_instance_pass();
        if (!empty) {
            if (name == "refit_or_rebuild_tlas_device_async") {
                if (!st.quality_is_armed() && capturing) return refused;  // the arming call must run eagerly (the same error code)
                st.quality_armed_now();
            }
            st.tlas_committed_async(capturing);
            note_async(capturing);
        }
        st.device_commit_enqueued();
        return ok;
    }
    if (name == "release_captures") { st.captures_released(); return ok; }
    return nullptr;
}
}  // namespace

int main() {
    std::string line;
    for (long n = 1; std::getline(std::cin, line); ++n) {
        std::istringstream in(line);
        std::string name, flag;
        in >> name >> flag;
        if (name.empty()) continue;
        if (!flag.empty() && flag != "empty" && flag != "capturing" && flag != "gone") { std::fprintf(stderr, "line %ld: unknown flag %s\n", n, flag.c_str()); return 2; }
        const char* out = run(name, flag == "empty", flag == "capturing", flag == "gone");
        if (!out) { std::fprintf(stderr, "line %ld: unknown entry point %s\n", n, name.c_str()); return 2; }
        std::puts(out);
        const RcSceneFlags f = st.snapshot();
        const char* broken = nullptr;
        if (f.host_instances_stale && f.mirror_edited) broken = "host_instances_stale implies !mirror_edited";
        else if (f.device_dirty && !f.transforms_dirty) broken = "device_dirty implies transforms_dirty";
        if (broken) { std::fflush(stdout); std::fprintf(stderr, "line %ld (%s): invariant broken: %s\n", n, line.c_str(), broken); return 1; }
    }
    return 0;
}
