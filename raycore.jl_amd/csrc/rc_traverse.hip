// rc_traverse.hip -- closest_hit / any_hit over ray batches on gfx950 (wave64).
//
// Replaces the per-work-item traversal the reference runs through KernelAbstractions
// (closest_hit src/instanced-bvh.jl:1902-2024, any_hit :2034-2140, safe_invdir :1742-1748,
// fast_intersect_bbox :1841-1859, intersect_internal_node :1807-1832, fast_intersect_triangle :1756-1797).
//
// Per-ray semantics are the reference's, statement for statement: same BVH2 nodes, same near/far rule,
// same push/pop order, same Moeller-Trumbore expression order, no FMA contraction -- so hit ids and t are
// bit-identical to the reference algorithm regardless of how rays are scheduled onto lanes.  What is
// MI355X-specific is everything around that: 64-byte aligned, pair-packed node / instance records fetched with
// raw buffer loads, the per-lane traversal stack in LDS ([entry][lane] layout => conflict-free ds_read/ds_write_b32)
// with a global spill area for the rare deep path, persistent waves that refill finished lanes from a global ray
// counter (ballot + mbcnt prefix sums), and phase-structured execution so a wave only issues the block its lanes
// actually need.  Kernel variants (rc_set_option "kernel"): 0 simple, 1 persistent, 3 phased (core in rc_traverse_core.h), 5 phased with
// the top level -- TLAS interior nodes, instance records, a single BLAS's top nodes -- staged in LDS (the default when the scene has <= 256
// instances), 6 phased with the breadth-first tops staged (the default for larger scenes).  All return identical results.
#include <algorithm>
#include <cstdlib>

#include <hip/hip_ext.h>
#include <hipcub/hipcub.hpp>

#include "rc_traverse_core.h"

namespace {

using namespace rc;

// ---- kernel 0: one ray per lane, grid-stride --------------------------------------------------------
template <bool ANY>
__global__ __launch_bounds__(kBlock, 6) void k_trace_simple(TraceArgs a) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    const uint32_t gtid = blockIdx.x * kBlock + threadIdx.x;
    LaneStack st(lds_stack + threadIdx.x, a.v.overflow + gtid, a.v.total_threads, a.v.status);
    for (uint64_t i = gtid; i < a.n_rays; i += a.v.total_threads) {
        RayState s;
        init_ray(s, load_ray(a.rays, i), ANY, st, a.v.tlas_off);
        if (a.v.n_tlas_nodes != 0)
            while (step<ANY>(s, a.v, st)) {}
        write_hit(s, a.v, a.hits, i);
    }
}

// ---- kernel 1: persistent waves with lane refill ------------------------------------------------------
// Each wave owns a slice [pool_next, pool_end) of ray indices taken from the global counter a.pool at a
// time (64..128, sized so that every resident wave gets several slices even for small batches).  Lanes whose ray has finished write their hit and go idle; when at least `refill` lanes are idle
// (or every lane is) the wave hands the idle lanes consecutive new indices: the idle mask comes from
// __ballot, each idle lane's rank from mbcnt (a prefix popcount), so no lane waits for the slowest ray of
// its original 64-ray packet.

template <bool ANY, bool STATS>
__global__ __launch_bounds__(kBlock, 6) void k_trace_persistent(TraceArgs a) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    const uint32_t gtid = blockIdx.x * kBlock + threadIdx.x;
    LaneStack st(lds_stack + threadIdx.x, a.v.overflow + gtid, a.v.total_threads, a.v.status);
    const int lane = threadIdx.x & 63;
    if (a.v.n_tlas_nodes == 0) {  // empty TLAS: every ray misses (test/test_tlas_stress.jl:808-831)
        RayState miss;
        miss.closest_inst = -1;
        for (uint64_t i = gtid; i < a.n_rays; i += a.v.total_threads) write_hit(miss, a.v, a.hits, i);
        return;
    }
    unsigned long long pool_next = 0, pool_end = 0;  // wave-uniform slice of ray indices
    bool exhausted = false;                          // wave-uniform: nothing left behind the global counter
    bool active = false;
    uint64_t my_ray = 0;
    RayState s;
    s.node = RC_INVALID_NODE;
    unsigned long long st_steps = 0, st_lanes = 0, st_maxsp = 0;
    for (;;) {
        unsigned long long idle_mask = __ballot(!active);
        int n_idle = __popcll(idle_mask);
        const bool can_refill = !(exhausted && pool_next == pool_end);
        if (n_idle == 64 && !can_refill) break;
        if (can_refill && n_idle >= a.refill) {
            for (;;) {
                idle_mask = __ballot(!active);
                n_idle = __popcll(idle_mask);
                if (n_idle == 0) break;
                if (pool_next == pool_end) {
                    if (exhausted) break;
                    // one chunk of rays from this wave's shard of the interleaved chunk counters (RcClaim, rc_traverse_core.h)
                    if (!rc_claim_chunk(a.claim, nullptr, (blockIdx.x * kBlock + threadIdx.x) >> 6, lane, a.n_rays, pool_next, pool_end)) { exhausted = true; break; }
                }
                const unsigned long long left = pool_end - pool_next;
                const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(idle_mask >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((unsigned)idle_mask, 0u));
                if (!active && rank < left) {
                    my_ray = pool_next + rank;
                    init_ray(s, load_ray(a.rays, my_ray), ANY, st, a.v.tlas_off);
                    active = true;
                }
                pool_next += ((unsigned long long)n_idle < left) ? (unsigned long long)n_idle : left;
            }
        }
        if (STATS) { st_steps += 1; st_lanes += active ? 1 : 0; if ((unsigned)s.sp > st_maxsp && active) st_maxsp = s.sp; }
        if (active) {
            if (!step<ANY>(s, a.v, st)) {
                write_hit(s, a.v, a.hits, my_ray);
                active = false;
            }
        }
    }
    if (STATS) {
        if (lane == 0) atomicAdd(&a.stats[0], st_steps);
        atomicAdd(&a.stats[1], st_lanes);
        atomicMax(&a.stats[2], st_maxsp);
    }
}

// ---- kernel 5: kernel 3 with the whole top level staged in LDS (LdsShape, rc_traverse_core.h): two 768-thread workgroups per CU keep the 24
// waves per CU of kernel 3 (the shallower LDS stack costs < 2 %, measured).  Used when the scene has <= 256 instances.
template <bool ANY, unsigned FLAGS = 0u>
__global__ __launch_bounds__(kMidBlock, 6) void k_trace_phased_lds(TraceArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const LdsTop top = LdsShape<FLAGS>::prologue(smem, a.v, a.blas_k, a.lds_blas_base, 0u, a.v.n_tlas_nodes != 0);  // (the drivers never run this shape on an empty scene; a trace launch may)
    PersistArgs p{a.n_rays, a.claim, a.refill, a.sched_thr, a.stats, a.blas_k, a.lds_blas_base, 0u, a.timeline};
    phased_trace<ANY, LdsShape<FLAGS>>(a.v, p, LdsShape<FLAGS>::stacks(smem), ArraySource{a.rays}, HitWriter{a.v.inst, a.hits}, top);
}

// ---- kernel 6: kernel 5's shape for top levels that do not fit (more than 256 instances): only the breadth-first tops of the TLAS and
// of a single BLAS are staged (PartialShape, rc_traverse_core.h); TLAS leaves and instance records come from memory as in kernel 3.
template <bool ANY, unsigned FLAGS = 0u>
__global__ __launch_bounds__(kMidBlock, 6) void k_trace_phased_partial(TraceArgs a) {
    // (closest-hit with 32-bit stack entries keeps the pointer form of the interior loop's stack position: at 78 VGPRs it has no room for the
    // integer form's two stride registers -- 12 bytes of private segment otherwise; neither the LDS layout nor its size depends on the flag)
    typedef PartialShape<FLAGS | ((!ANY && (FLAGS & ShapeStack16) == 0u) ? ShapePtrStack : 0u)> Shape;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const LdsTop top = Shape::prologue(smem, a.v, a.blas_k, a.lds_blas_base, a.tlas_k);
    PersistArgs p{a.n_rays, a.claim, a.refill, a.sched_thr, a.stats, a.blas_k, a.lds_blas_base, a.tlas_k};
    phased_trace<ANY, Shape>(a.v, p, Shape::stacks(smem), ArraySource{a.rays}, HitWriter{a.v.inst, a.hits}, top);
}

// ---- kernel 3: the phase-structured persistent core (rc_traverse_core.h) on a ray array ------------------------
template <bool ANY, unsigned FLAGS = 0u>
__global__ __launch_bounds__(kBlock, 6) void k_trace_phased(TraceArgs a) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    PersistArgs p{a.n_rays, a.claim, a.refill, a.sched_thr, a.stats, 0u, 0u, 0u};
    phased_trace<ANY, PlainShape<FLAGS>>(a.v, p, lds_stack, ArraySource{a.rays}, HitWriter{a.v.inst, a.hits});
}

}  // namespace

// ---- launch bookkeeping (RcLaunchGuard, rc_internal.h) ------------------------------------------------------------------------------
namespace {
struct TlTiming { uint64_t uid = 0; TimingRef ref; };
thread_local TlTiming tl_timing;  // the calling thread's latest timed operation (rc_last_kernel_ms reports it while its slot has not been reused)

void note_timing(rc_scene* s, const TimingRef& ref) {
    s->last_timing = ref;
    tl_timing.uid = s->uid;
    tl_timing.ref = ref;
}
}  // namespace

RcLaunchGuard::RcLaunchGuard(rc_scene* scene, hipStream_t st) : s(scene), stream(st), lock(scene->launch_mu) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
    capturing = cap == hipStreamCaptureStatusActive;
    if (capturing) {
        // A captured launch bakes its addresses into the graph and may be replayed at any time, beside eager launches and beside other
        // graphs: it gets a lane-stack spill region AND a slot of claim counters that no other launch, eager or captured, will ever use
        // (graphs captured on one stream used to share that stream's region, so two of them replayed side by side on a tree
        // deeper than the LDS stack overwrote each other's entries).  Both come from a pool of kCounterSlots - kEagerSlots capture slots per
        // scene, handed back by option "release_capture" (one) / "release_captures" (all) once the caller's graphs are gone.  The region
        // is sized for the launch's own grid and allocated where that is known (rc_launch_overflow) -- inside the capture: the entry points run
        // with the thread's capture-interaction mode relaxed, in which hipMalloc is legal.
        if (s->capture_slots.empty()) s->capture_slots.resize(kCounterSlots - kEagerSlots);
        int free_slot = -1;
        for (size_t i = 0; i < s->capture_slots.size() && free_slot < 0; ++i) if (!s->capture_slots[i].in_use) free_slot = (int)i;
        if (free_slot < 0)
            throw RcError(1, "this scene already holds " + std::to_string(kCounterSlots - kEagerSlots) + " captured launches (each owns a stack spill region and a counter slot): "
                             "destroy a graph and hand its launches back (option \"release_capture\" with the token \"last_capture_token\" gave, or \"release_captures\" for all), "
                             "or capture several launches' worth of rays in one launch");
        s->capture_slots[free_slot].in_use = true;
        capture = s->last_capture = free_slot;
        slot = kEagerSlots + free_slot;
    } else {
        // the lane-stack spill area of the launch's stream (eager launches on one stream are ordered and share it), sized for the largest
        // grid any option can ask for: rc_set_option clamps blocks_per_cu to 8 blocks of 256 threads per CU
        rc_scene::OverflowRegion& region = rc_stream_slot<rc_scene::kMaxOverflowRegions>(s->overflow_regions, stream);
        region.buf.reserve((size_t)kTotalStack * (size_t)s->n_cus * 8 * kBlock);
        uses(region.last);
        overflow = region.buf.p;
        // the launch's slot of chunk counters; a launch that reuses an eager slot from another stream waits for the slot's previous user
        s->launch_seq += 1;
        slot = (int)(s->launch_seq % (uint64_t)kEagerSlots);
        rc_scene::LaunchSlot& ls = s->slots[slot];
        if (ls.recorded && ls.stream != stream) RC_HIP(hipStreamWaitEvent(stream, ls.t1, 0));
    }
    if (s->opt.stats) RC_HIP(hipMemsetAsync(rc_stats_words(s), 0, kStatsWords * sizeof(unsigned long long), stream));
}

void RcLaunchGuard::start() {
    if (capturing) return;
    rc_scene::LaunchSlot& ls = s->slots[slot];
    if (!ls.t0) {
        // t0 only marks a time in front of the kernel: nothing is published by it, so it skips the system-scope fence (0.5 % of a back-to-back
        // launch sequence, profiles/r05_launch_fixed_costs.txt); t1 keeps the default -- the host reads pinned words behind it
        RC_HIP(hipEventCreateWithFlags(&ls.t0, hipEventDisableSystemFence));
        RC_HIP(hipEventCreateWithFlags(&ls.t1, hipEventDefault));
    }
    RC_HIP(hipEventRecord(ls.t0, stream));
}

void RcLaunchGuard::bind() {  // instead of start(): the launch's kernel carries the events itself (launch_variant)
    if (capturing) return;
    rc_scene::LaunchSlot& ls = s->slots[slot];
    if (!ls.t0) {
        RC_HIP(hipEventCreateWithFlags(&ls.t0, hipEventDisableSystemFence));
        RC_HIP(hipEventCreateWithFlags(&ls.t1, hipEventDefault));
    }
    carry_t0 = ls.t0; carry_t1 = ls.t1;
}

void RcLaunchGuard::finish() {
    RC_HIP(hipGetLastError());
    if (capturing) return;  // a captured launch has no events of its own: the graph orders it, and its duration is the replay's business
    rc_scene::LaunchSlot& ls = s->slots[slot];
    if (!carried) RC_HIP(hipEventRecord(ls.t1, stream));
    // the per-stream resources this launch used are busy until here (asked by the next stream that wants to take one over): they follow the
    // launch's closing event instead of recording one of their own
    for (int i = 0; i < n_busy; ++i) busy[i]->follow(ls.t1);
    ls.stream = stream;
    ls.recorded = true;
    ls.seq = ++s->timing_seq;
    note_timing(s, TimingRef{slot, ls.seq, 0.f});
}

void rc_timing_scene_begin(rc_scene* s, hipStream_t stream) { RC_HIP(hipEventRecord(s->ev0, stream)); }
void rc_timing_scene_end(rc_scene* s, hipStream_t stream) {
    RC_HIP(hipEventRecord(s->ev1, stream));
    std::lock_guard<std::mutex> g(s->launch_mu);
    rc_scene::LaunchSlot& slot = s->slots[kSceneTimingSlot];
    slot.t0 = s->ev0; slot.t1 = s->ev1; slot.stream = stream; slot.recorded = true;
    slot.seq = ++s->timing_seq;
    note_timing(s, TimingRef{kSceneTimingSlot, slot.seq, 0.f});
}
void rc_timing_fixed(rc_scene* s, float ms) {
    std::lock_guard<std::mutex> g(s->launch_mu);
    note_timing(s, TimingRef{-1, ++s->timing_seq, ms});
}
float rc_timing_read(rc_scene* s) {
    hipEvent_t a = nullptr, b = nullptr;
    {
        std::lock_guard<std::mutex> g(s->launch_mu);
        TimingRef ref = s->last_timing;
        if (tl_timing.uid == s->uid) {
            const TimingRef& mine = tl_timing.ref;
            if (mine.slot == -1 || (mine.slot >= 0 && s->slots[mine.slot].seq == mine.seq)) ref = mine;  // else: the slot has been reused since
        }
        if (ref.slot == -2) return 0.f;
        if (ref.slot == -1) return ref.fixed_ms;
        if (s->slots[ref.slot].seq != ref.seq) return 0.f;
        a = s->slots[ref.slot].t0; b = s->slots[ref.slot].t1;
    }
    float ms = 0.f;
    RC_HIP(hipEventSynchronize(b));
    RC_HIP(hipEventElapsedTime(&ms, a, b));
    return ms;
}

void rc_claim_fill(RcLaunchGuard& g, uint64_t n_items, uint32_t total_waves, rc::RcClaim& out) {
    rc_scene* s = g.s;
    out.counters = g.counter_slot() + kShardBase;
    uint32_t shards = (uint32_t)s->opt.claim_shards, shift = 0;
    while (shards > 1 && shards > total_waves) shards >>= 1;  // every shard needs a wave: chunks dealt to a shard nobody drains would never be traced
    while ((2u << shift) <= shards) ++shift;
    out.shard_shift = shift;
    out.pool = (uint32_t)(s->opt.pool > 0 ? s->opt.pool : 128u);  // measured: 64 loses 10-16 % (a wave's lanes end up on rays of more image regions), 256+ unbalances the tail
    out.total_waves = total_waves;
    // guided claim sizes (RcClaim): the chunks of the claim order are dealt whole, then in halves, quarters, eighths; piece k ends where the
    // items left equal taper / 8 x its part size x waves
    const uint64_t P = out.pool, n_base = (n_items + P - 1) / P;
    uint64_t chunks[4] = {n_base, 0, 0, 0}, done = 0;
    if (s->opt.taper > 0 && (P & 7u) == 0) {  // parts must tile the chunk: a pool that is not a multiple of eight is dealt whole
        for (int k = 0; k < 3; ++k) {
            const uint64_t keep = (uint64_t)s->opt.taper * (P >> k) * total_waves / 8u;          // items left for the smaller parts
            const uint64_t upto = n_items > keep ? (n_items - keep) / P : 0;                          // whole chunks handed out before that point
            chunks[k] = upto > done ? upto - done : 0;
            done += chunks[k];
        }
        chunks[3] = n_base - done;
    }
    const uint64_t n_claims = chunks[0] + 2 * chunks[1] + 4 * chunks[2] + 8 * chunks[3];
    if (n_claims >= (1ull << 31)) throw RcError(1, "ray batch too large for 32-bit chunk ids");
    out.n_chunks = (uint32_t)n_claims;
    out.g1 = (uint32_t)chunks[0]; out.g2 = (uint32_t)(chunks[0] + 2 * chunks[1]); out.g3 = (uint32_t)(chunks[0] + 2 * chunks[1] + 4 * chunks[2]);
    out.c1 = (uint32_t)chunks[0]; out.c2 = (uint32_t)(chunks[0] + chunks[1]); out.c3 = (uint32_t)(chunks[0] + chunks[1] + chunks[2]);
    out.order = nullptr; out.cost = nullptr; out.hist = nullptr;
    out.sample_rays = nullptr; out.n_sample = 0; out.inv_l2 = 0.f; out.samples = nullptr; out.host_streak = nullptr; out.init_thr = 0; out.want_record = 0; out.host_gen = 0; out.close_dir_max = 0.f;
    for (int k = 0; k < 8; ++k) out.sample_host[k] = 0.f;
    out.pool_shift = 0;
    while ((2u << out.pool_shift) <= out.pool) ++out.pool_shift;
}

// The scene's arrays as the kernels see them: no launch state, no side effects.  What kernels that never spill a traversal stack get (the
// wavefront stages, which run OUTSIDE RcLaunchGuard and without launch_mu: ADVICE r5 -- they used to go through the allocating view
// below and could publish a tiny capture region into another thread's captured launch).
rc::SceneView rc_scene_view_static(rc_scene* s) {
    rc::SceneView v;
    v.tlas_nodes = s->tlas_nodes.p; v.blas_nodes = s->flat_nodes.p; v.inst = s->inst_recs.p; v.prims = s->flat_prims.p;
    v.n_tlas_nodes = s->n_tlas_nodes; v.n_prims = s->n_flat_prims; v.tlas_off = s->n_flat_nodes; v.n_nodes_total = s->n_flat_nodes + s->n_tlas_nodes; v.n_inst = s->n_static_instances;
    v.entry_cull = (s->opt.entry_cull && s->inst_cull.p && s->n_static_instances) ? 1u : 0u;
    v.overflow = nullptr; v.total_threads = 0;
    v.status = rc_status_word(s);
    return v;
}

// The launch's stack spill region.  An eager launch has its stream's region already; a captured launch gets its own here, sized for its
// own grid of `total_threads` threads (every capture used to pin the largest grid's 268 MB) -- allocated inside the capture: the
// entry points run with the thread's capture-interaction mode relaxed, in which hipMalloc is legal.  Never returns null.
uint32_t* rc_launch_overflow(RcLaunchGuard& g, uint32_t total_threads) {
    if (!g.overflow) {
        rc_scene::CaptureSlot& cs = g.s->capture_slots[g.capture];
        try {
            cs.region.reserve((size_t)kTotalStack * std::max<uint32_t>(total_threads, 64u));
        } catch (const RcError&) {
            (void)hipGetLastError();
            cs.in_use = false;
            throw RcError(1, "could not allocate the stack spill region of a captured launch inside the capture (capture mode does not allow hipMalloc here): "
                             "capture with hipStreamCaptureModeRelaxed / ThreadLocal, or run the launch eagerly");
        }
        g.overflow = cs.region.p;
    }
    return g.overflow;
}

// The view of the launch's traversal kernel with `total_threads` threads.
rc::SceneView rc_scene_view(RcLaunchGuard& g, uint32_t total_threads) {
    rc::SceneView v = rc_scene_view_static(g.s);
    v.overflow = rc_launch_overflow(g, total_threads); v.total_threads = total_threads;
    return v;
}

// Arguments of the launch's persistent kernel with `total_threads` threads.
rc::PersistArgs rc_persist_args(RcLaunchGuard& g, uint64_t n_items, uint32_t total_threads) {
    rc::PersistArgs p;
    p.n_items = n_items;
    rc_claim_fill(g, n_items, total_threads / 64u, p.claim);
    p.refill = (int)g.s->opt.refill;
    p.int_thr = (int)g.s->opt.sched_thr;
    p.stats = rc_stats_words(g.s);
    return p;
}

void rc_ensure_dynamic_lds(rc_scene* s, const void* fn, size_t bytes) {
    if (s->dynamic_lds_set.count(fn)) return;
    RC_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    s->dynamic_lds_set.insert(fn);
}

// The drivers' LDS variants (768-thread workgroups, node planes) apply under the same conditions as trace kernel 5.
bool rc_lds_driver_ok(rc_scene* s) {
    return s->opt.kernel != 3 && s->n_tlas_nodes > 0 && s->n_tlas_nodes <= (uint32_t)kTlasLdsNodes && (uint64_t)(s->n_flat_nodes + s->n_tlas_nodes) * 64u < (1ull << 32);
}
// ... and the partial-LDS variants under the conditions of trace kernel 6: a larger top level with something to stage
bool rc_partial_driver_ok(rc_scene* s) {
    return s->opt.kernel != 3 && s->n_tlas_nodes > (uint32_t)kTlasLdsNodes && s->tlas_top_k32 + s->blas_top_k32 > 0 &&
           (uint64_t)(s->n_flat_nodes + s->n_tlas_nodes) * 64u < (1ull << 32);
}
void rc_partial_driver_args(rc_scene* s, rc::PersistArgs& p) {  // (the drivers run the 32-bit shape: prefixes of the renumbered tops)
    p.tlas_k = s->tlas_top_k32; p.blas_k = s->opt.blas_top ? s->blas_top_k32 : 0; p.lds_blas_base = s->tlas_top_k32;
}
void rc_lds_driver_args(rc_scene* s, rc::PersistArgs& p) {
    if (s->opt.blas_top) { p.blas_k = s->blas_top_k32; p.lds_blas_base = (s->n_tlas_nodes + 1) / 2 - 1; }
}

// The grid of a persistent launch over n_items: a block per `block` items, at most the blocks that are resident together -- `per_cu` a
// CU (TraceShape::kBlocksPerCu), for the 256-thread shapes what option "blocks_per_cu" says, else 6 (6 x 24 KiB of LDS stacks per CU).
uint32_t rc_grid_blocks(rc_scene* s, uint64_t n_items, int block, int64_t per_cu) {
    if (per_cu == 0) per_cu = s->opt.blocks_per_cu > 0 ? s->opt.blocks_per_cu : 6;
    return (uint32_t)std::min<uint64_t>((n_items + block - 1) / block, (uint64_t)s->n_cus * per_cu);
}

// kernels 5 / 6 in their STACK16 shape: the scene's trees are all small enough, nobody asked for counters or a timeline (dev builds keep the 32-bit shape)
static bool rc_stack16(rc_scene* s) { return s->small_trees && s->opt.stack16 && !s->opt.timeline_ptr; }

// Which instantiation runs a launch of `kernel` (0, 1, 3, 5 or 6: rc_launch_trace has applied the fall-back rules).
template <bool ANY>
static void launch_variant(RcLaunchGuard& g, int64_t kernel, const TraceArgs& a, uint32_t blocks) {
    rc_scene* s = g.s;
    const bool stats = s->opt.stats != 0, s16 = rc_stack16(s);
    // The launch's timing / ordering events ride on the kernel's own dispatch (hipExtLaunchKernelGGL binds them to its start and end): no
    // event packets of their own around the kernel -- they cost ~3 us each between two back-to-back launches.  (Null outside RcLaunchGuard::bind.)
    hipEvent_t e0 = g.carry_t0, e1 = g.carry_t1;
    g.carried = e0 != nullptr;
    // a kernel with dynamic LDS: the function's limit is raised first, once per scene = per device (the attribute belongs to the function on one device)
    auto launch = [&](void (*k)(TraceArgs), auto shape) {
        if (shape.kLdsBytes) rc_ensure_dynamic_lds(s, reinterpret_cast<const void*>(k), shape.kLdsBytes);
        hipExtLaunchKernelGGL(k, dim3(blocks), dim3(shape.kBlock), (uint32_t)shape.kLdsBytes, g.stream, e0, e1, 0u, a);
    };
    if (kernel == 5) {
        // dev: the same kernel with per-phase pass / lane counters (option "stats"; tools/isa_mix.py weights the phases' static opcode histograms
        // with them), or with per-wave event times written to the caller's buffer (option "timeline_ptr")
        if (stats && s16) launch(k_trace_phased_lds<ANY, ShapeStats | ShapeStack16>, LdsShape<ShapeStats | ShapeStack16>());
        else if (stats) launch(k_trace_phased_lds<ANY, ShapeStats>, LdsShape<ShapeStats>());
        else if (a.timeline) launch(k_trace_phased_lds<ANY, ShapeTimeline>, LdsShape<ShapeTimeline>());
        else if (s16) launch(k_trace_phased_lds<ANY, ShapeStack16>, LdsShape<ShapeStack16>());
        else launch(k_trace_phased_lds<ANY>, LdsShape<>());
    } else if (kernel == 6) {
        if (s16) launch(k_trace_phased_partial<ANY, ShapeStack16>, PartialShape<ShapeStack16>());
        else launch(k_trace_phased_partial<ANY>, PartialShape<>());
    } else if (kernel == 3) {
        if (stats) launch(k_trace_phased<ANY, ShapeStats>, PlainShape<ShapeStats>());
        else launch(k_trace_phased<ANY>, PlainShape<>());
    } else if (kernel == 0) {
        launch(k_trace_simple<ANY>, PlainShape<>());
    } else {
        if (stats) launch(k_trace_persistent<ANY, true>, PlainShape<>());
        else launch(k_trace_persistent<ANY, false>, PlainShape<>());
    }
}

// ---- cost-ordered claiming (RcClaim::order / cost / hist) -------------------------------------------------------------------------------
// Which batch a launch is, whether it claims through a learned order and whether it records is decided INSIDE the launch (order_select /
// order_commit, rc_traverse_core.h): nothing runs in front of a launch for that (round 5; rounds 3-4 spent three small dispatches per launch,
// ~3 % of a 4 M-ray step and ~4 % of a 1 M-ray one, profiles/r05_bench_with_extras_by_range.csv).  What is left to separate kernels is turning
// a finished RECORDING into an order:
//   k_order_count / k_order_scatter, for every batch slot whose cost array holds a recording no order has been built from yet (kHistPending):
//     the reported chunks in nine classes, linear in the lifetime of their longest ray between the reporting threshold and the top of the scale
//     the RECORDING launch worked with, longest first; then the chunks nobody reported; chunk ids ascending inside a class (a stable
//     counting sort: k_order_count tallies the classes per 1024-chunk block, k_order_scatter places every chunk into the slot's order array,
//     clears its cost for the slot's next recording and -- block 0 -- leaves the threshold and the scale of that next recording: the
//     threshold moves so that roughly 30-70 % of the chunks report).
//   The host enqueues the pair only in front of launches that MAY follow a recording (rc_cost_order_setup): the shape's first launches, the
//   launches after a batch that was not a repeat was reported, and the launch after one the host's cadence asked to record -- one launch in
//   eight of a repeating batch.  A recording the host misses (it learns of new batches through a pinned word, late when the caller enqueues
//   far ahead) simply waits for the next pair.
//   Recording costs 25-30 us of a 0.37 ms launch, so a slot records its launches 2-4 (never the first: a batch that does not come back must
//   not pay for it) and then one in eight; the launches in between claim through the slot's order as it stands.
//   (A first-launch PREDICTOR -- claim order from the number of top-of-tree boxes each chunk's middle ray passes -- was built and measured in
//   round 4: worth 5-12 % of a 1 M-ray launch, and the small kernels it needs cost as much: profiles/r04_first_launch_predictor.txt.  Not kept.)
// hist[kHistScale + 4 slot]: [0], [1] = the threshold / the top of the scale the slot's latest recording launch worked with; [2], [3] = the pair its next one will.
// The number of cost classes of the rebuilt order and the share of the chunks (per cent) the reporting threshold aims at.  Round 5
// (tools/probes/order_quality_probe.py, docs/EXPERIMENTS.md): 10 / 16 / 26 / 31 classes order equally well; the
// share matters -- with 30-70 % of the chunks reporting (rounds 3-4: 10-40 %) the same batches run 3-8 % faster, because the chunks below
// the threshold are claimed in natural order BEHIND the reported ones and most of a batch's medium-long chunks were among them.
constexpr int kOrderClasses = 10, kOrderRaisePct = 70, kOrderLowerPct = 30;
// Close repeats (order_select): the largest direction term -- mean over the 64 samples of |dd|^2 / |d|^2 -- at which a launch with the slot's
// own origins still continues the slot's history.  Jitter inside a pixel gives 4e-8 at 2048^2, 2.4e-7 at 1280 x 800, 2.7e-6 at 256^2 (45
// degrees); a camera turned in place by 0.15 / 0.2 / 5 degrees 6.7e-6 / 1.2e-5 / 7.3e-3.  tools/probes/close_repeat_predictor.py
// (profiles/close_repeat_predictor.txt): up to 6.7e-6 the order learned from the predecessor leaves at most twice as many of the truly
// longest chunks to the end of the launch as the order learned from another jitter seed of the same view does; from 1.2e-5 on, more.
constexpr float kCloseDirMax = 6e-6f;
namespace {
constexpr int kOrderThreads = 256, kOrderPerThread = 4, kOrderTile = kOrderThreads * kOrderPerThread, kOrderMaxBlocks = 256;
constexpr int kOrderPacked = (kOrderClasses + 4) / 5;  // u64 words of 12-bit per-class counters (k_order_scatter)
static_assert(kOrderClasses + 1 <= 32, "k_order_scatter sums the blocks' counts with 32 threads per block group");
static_assert(rc_scene::ChunkHistory::kHeaderWords == (uint32_t)kHistHeaderWords, "rc_internal.h repeats the size of a header copy");
static_assert((uint32_t)(kOrderTile * kOrderMaxBlocks) == kHistSlotStride, "a slot's cost array holds the most chunks the rebuild kernels handle");
constexpr int kOrderCountWords = kOrderClasses + 1;  // per block: the classes' chunk counts, the largest cost
constexpr size_t kHistWords = kHistCounts + (size_t)kHistSlots * kOrderMaxBlocks * kOrderCountWords;

__device__ inline int order_class(uint32_t c, uint32_t thr, uint32_t top) {
    if (c == 0u) return kOrderClasses - 1;
    const uint32_t span = top > thr ? top - thr + 1u : 1u, above = c > thr ? c - thr : 0u;
    const uint32_t q = above * (uint32_t)(kOrderClasses - 1) / span;  // 0 .. kOrderClasses - 2 (and beyond when this launch's rays outlived the scale)
    return q >= (uint32_t)(kOrderClasses - 1) ? 0 : (int)(kOrderClasses - 2) - (int)q;
}
__device__ inline uint32_t* order_counts(uint32_t* hist, int slot) { return hist + kHistCounts + (size_t)slot * kOrderMaxBlocks * kOrderCountWords; }

__global__ __launch_bounds__(kOrderThreads) void k_order_count(const uint32_t* cost_base, uint32_t* ctl, uint32_t parity, uint32_t n_chunks) {
    __shared__ uint32_t cnt[kOrderCountWords];
    const uint32_t* hist = ctl + parity * kHistHeaderWords;  // the header copy the shape's next launch reads
    for (int slot = 0; slot < kHistSlots; ++slot) {
        if (hist[kHistPending + slot] == 0u) continue;  // (wave-uniform: a header word)
        if (threadIdx.x < kOrderCountWords) cnt[threadIdx.x] = 0u;
        __syncthreads();
        const uint32_t* cost = cost_base + (size_t)slot * kHistSlotStride;
        const uint32_t thr = hist[kHistScale + 4 * slot], top = hist[kHistScale + 4 * slot + 1];  // the scale the recording launch worked with
        const uint32_t first = blockIdx.x * kOrderTile + threadIdx.x * kOrderPerThread;
        uint32_t mx = 0u;
        for (int j = 0; j < kOrderPerThread; ++j)
            if (first + j < n_chunks) { const uint32_t c = cost[first + j]; atomicAdd(&cnt[order_class(c, thr, top)], 1u); mx = c > mx ? c : mx; }
        if (mx) atomicMax(&cnt[kOrderClasses], mx);
        __syncthreads();
        if (threadIdx.x < kOrderCountWords) order_counts(ctl, slot)[blockIdx.x * kOrderCountWords + threadIdx.x] = cnt[threadIdx.x];  // [classes ..., block maximum]
        __syncthreads();
    }
}
__global__ __launch_bounds__(kOrderThreads) void k_order_scatter(uint32_t* cost_base, uint32_t* order_base, uint32_t* ctl, uint32_t parity, uint32_t n_chunks, uint32_t* host_words) {
    uint32_t* hist = ctl + parity * kHistHeaderWords;
    typedef hipcub::BlockScan<unsigned long long, kOrderThreads> Scan;
    __shared__ typename Scan::TempStorage scan_tmp;
    __shared__ uint32_t total[kOrderCountWords], before[kOrderClasses];  // chunks of class k in all blocks (last: the largest cost) / in the blocks before this one
    __shared__ uint32_t unreported_of[kHistSlots], longest_of[kHistSlots];  // per rebuilt slot, for the header update at the end (a serial walk over the blocks' counts there cost 20 us)
    const uint32_t first = blockIdx.x * kOrderTile + threadIdx.x * kOrderPerThread;
    for (int slot = 0; slot < kHistSlots; ++slot) {
        if (hist[kHistPending + slot] == 0u) continue;
        uint32_t* cost = cost_base + (size_t)slot * kHistSlotStride;
        uint32_t* order = order_base + (size_t)slot * kHistSlotStride;
        if (threadIdx.x < kOrderCountWords) { total[threadIdx.x] = 0u; if (threadIdx.x < kOrderClasses) before[threadIdx.x] = 0u; }
        __syncthreads();
        const uint32_t* counts = order_counts(ctl, slot);
        {   // thread (word w, group g) sums word w of the blocks g, g + 8, ... in registers, then one LDS atomic per thread.  (One thread per
            // BLOCK with an LDS atomic per word put 32 lanes on the same LDS address twenty times over: 17 of this kernel's 22 us.)
            const uint32_t w = threadIdx.x & 31u, g = threadIdx.x >> 5;
            if (w < (uint32_t)kOrderCountWords) {
                uint32_t all = 0u, mine = 0u;
                for (uint32_t b = g; b < gridDim.x; b += kOrderThreads / 32) {
                    const uint32_t c = counts[b * kOrderCountWords + w];
                    if (w == (uint32_t)kOrderClasses) all = c > all ? c : all;
                    else { all += c; mine += b < blockIdx.x ? c : 0u; }
                }
                if (w == (uint32_t)kOrderClasses) atomicMax(&total[w], all);
                else { if (all) atomicAdd(&total[w], all); if (mine) atomicAdd(&before[w], mine); }
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) { unreported_of[slot] = total[kOrderClasses - 1]; longest_of[slot] = total[kOrderClasses]; }
        const uint32_t thr = hist[kHistScale + 4 * slot], top = hist[kHistScale + 4 * slot + 1];
        int cls[kOrderPerThread];
        unsigned long long packed[kOrderPacked];  // this thread's chunks per class, 12 bits each, five classes per word
#pragma unroll
        for (int q = 0; q < kOrderPacked; ++q) packed[q] = 0ull;
        for (int j = 0; j < kOrderPerThread; ++j) {
            cls[j] = first + j < n_chunks ? order_class(cost[first + j], thr, top) : -1;
#pragma unroll
            for (int q = 0; q < kOrderPacked; ++q) packed[q] += (cls[j] >= 0 && cls[j] / 5 == q) ? 1ull << (12 * (cls[j] % 5)) : 0ull;
        }
        unsigned long long prefix[kOrderPacked];
#pragma unroll
        for (int q = 0; q < kOrderPacked; ++q) {
            if (q) __syncthreads();
            Scan(scan_tmp).ExclusiveSum(packed[q], prefix[q]);
        }
        uint32_t pos[kOrderClasses], acc = 0;
        for (int k = 0; k < kOrderClasses; ++k) { pos[k] = acc + before[k] + (uint32_t)((prefix[k / 5] >> (12 * (k % 5))) & 0xFFFull); acc += total[k]; }
#pragma unroll
        for (int j = 0; j < kOrderPerThread; ++j) {
            if (cls[j] < 0) continue;
            uint32_t at = 0;  // pos[cls[j]]++ by selection: an array indexed by a run-time class would live in scratch memory
#pragma unroll
            for (int k = 0; k < kOrderClasses; ++k) { const bool mine = cls[j] == k; at = mine ? pos[k] : at; pos[k] += mine ? 1u : 0u; }
            order[at] = first + j;
            cost[first + j] = 0u;
        }
        __syncthreads();
    }
    // the header: every block has read what it needs of it above; the LAST block to get here turns the recordings into orders in use
    // (No fence: what the blocks wrote above -- orders, cleared costs -- is read by the NEXT kernel; the last block reads only header words
    // nobody writes in this kernel and its own LDS.  An agent-scope release here wrote back the whole L2 -- full of the previous launch's hit
    // records -- and made this kernel 25 us long.)
    __shared__ uint32_t last_block;
    if (threadIdx.x == 0) last_block = atomicAdd(ctl + kHistTicket, 1u) + 1u == gridDim.x ? 1u : 0u;
    __syncthreads();
    if (!last_block || threadIdx.x != 0) return;
    ctl[kHistTicket] = 0u;
    for (int slot = 0; slot < kHistSlots; ++slot) {
        if (hist[kHistPending + slot] == 0u) continue;
        const uint32_t unreported = unreported_of[slot], mx = longest_of[slot];
        uint32_t* scale = hist + kHistScale + 4 * slot;  // the scale of the slot's NEXT recording launch
        const uint32_t thr = scale[0], reported = n_chunks - unreported;
        uint32_t next = thr;
        if (reported * 100ull > (unsigned long long)n_chunks * kOrderRaisePct) next += (next >> 2) + 1u;        // more than this share of the chunks reported: raise the bar
        else if (reported * 100ull < (unsigned long long)n_chunks * kOrderLowerPct && next > 2u) next -= next >> 2;  // fewer than this: lower it
        scale[2] = next;
        scale[3] = mx > next ? mx : next + 8u;  // the longest lifetime just seen scales the next recording's classes
        hist[kHistPending + slot] = 0u;
        hist[kHistHasOrder + slot] = 1u;
    }
    if (host_words) __hip_atomic_store(host_words + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);  // nothing waits for a rebuild any more
}
}  // namespace

// The history entry of a launch shape (chunk count, mode, chunk geometry, stream): launches on one stream are ordered, so its buffers have
// one user at a time; another stream gets its own entry.  Returns false when cost ordering does not apply to this launch.
bool rc_cost_order_setup(RcLaunchGuard& g, uint64_t n, int any_hit, rc::RcClaim& c, const RcRay* d_rays, const float* host_sample) {
    rc_scene* s = g.s;
    const hipStream_t stream = g.stream;
    const uint64_t n_base64 = (n + c.pool - 1) / c.pool;  // chunks (the claim order permutes whole chunks; parts follow their chunk)
    // only where the order can matter: at least a claim per wave; the cost path maps rays to chunks with a shift (pool a power of two)
    if (s->n_tlas_nodes == 0) return false;  // (an empty scene's launches return before they look at the history: the header's two copies must flip with the host's parity)
    if (!s->opt.cost_order || c.n_chunks < c.total_waves || n_base64 < 64u || n_base64 > (uint64_t)(kOrderTile * kOrderMaxBlocks) || (c.pool & (c.pool - 1u)) != 0u || c.pool < 16u) return false;
    if (!d_rays && !host_sample) return false;
    const uint32_t n_base = (uint32_t)n_base64;
    // Keyed by the number of CHUNKS (a batch a few rays shorter or longer has the same chunks in the same places), mode, stream and chunk size.
    rc_scene::ChunkHistory* h = nullptr;
    for (auto& e : s->histories)
        if (e.n_chunks == n_base && e.any == any_hit && e.stream == stream && e.pool == c.pool) { h = &e; break; }
    if (!h) {
        // A shape this scene has no history for.  Nothing here may block or synchronise (the *_device entry points are
        // asynchronous, and a workload whose batch size changes with every launch -- a wavefront tracer compacting its rays bounce by
        // bounce -- misses every time): a free entry is taken at once; a full table gives up an entry only to a shape that has been seen
        // BEFORE (a one-off size learns nothing worth keeping), and only an entry whose buffers nobody can still be using -- its stream
        // is this launch's stream (stream order protects them) or whose last launch has completed (the entry's own event, queried, never waited for).  Otherwise the
        // launch simply runs in natural order.  Buffers have ONE size (the largest batch the rebuild kernels handle), so re-keying an
        // entry frees and allocates nothing.
        bool seen_before = false;
        for (const auto& r : s->recent_shapes) if (r.n_chunks == n_base && r.any == any_hit && r.stream == stream && r.pool == c.pool) { seen_before = true; break; }
        if (!seen_before) {
            if (s->recent_shapes.size() < (size_t)rc_scene::kRecentShapes) s->recent_shapes.emplace_back();
            auto& r = s->recent_shapes.size() < (size_t)rc_scene::kRecentShapes ? s->recent_shapes.back() : s->recent_shapes[s->recent_clock % (uint64_t)rc_scene::kRecentShapes];
            s->recent_clock += 1;
            r.n_chunks = n_base; r.any = any_hit; r.stream = stream; r.pool = c.pool;
        }
        if (s->histories.size() < (size_t)rc_scene::kMaxHistories) {
            s->histories.emplace_back();
            h = &s->histories.back();
            h->cost.reserve((size_t)kHistSlots * kHistSlotStride); h->order.reserve((size_t)kHistSlots * kHistSlotStride); h->ctl.reserve(kHistWords);
            h->samples.reserve(2 * kHistSampleFloats);
        } else {
            if (!seen_before) return false;
            size_t victim = s->histories.size();
            uint64_t oldest = ~0ull;
            for (size_t i = 0; i < s->histories.size(); ++i) {
                auto& e = s->histories[i];
                if (e.last_use >= oldest) continue;
                const bool reusable = e.stream == stream || e.last.idle();  // (stream order protects a same-stream entry; any other is free once its last launch is done)
                if (reusable) { victim = i; oldest = e.last_use; }
            }
            if (victim == s->histories.size()) return false;
            h = &s->histories[victim];
        }
        h->n_items = n; h->any = any_hit; h->stream = stream; h->n_chunks = n_base; h->pool = c.pool;
        h->rebuild_credit = 0; h->next_record = 8; h->records_asked = 0;
        if (h->fresh_streak.p) { reinterpret_cast<volatile uint32_t*>(h->fresh_streak.p)[0] = 0u; reinterpret_cast<volatile uint32_t*>(h->fresh_streak.p)[1] = 0u; reinterpret_cast<volatile uint32_t*>(h->fresh_streak.p)[2] = 0u; }
        RC_HIP(hipMemsetAsync(h->ctl.p, 0, sizeof(uint32_t) * kHistCounts, stream));  // every batch slot empty (the cost arrays are cleared when a slot is given out)
        h->gen = 0;
        h->parity = 0;
    }
    h->last_use = ++s->history_clock;
    g.uses(h->last);
    // (A shape whose batches never repeat leaves the mechanism for a while: counted and decided on the device, order_select / order_commit.)
    h->fresh_streak.ensure();
    h->gen += 1;
    // Turning recordings into orders: the pair of rebuild kernels goes in front of this launch only when a slot MAY hold a recording --
    // the shape's first launches (a batch records its launches 2-4), the launches after the device reported a launch that was not a
    // repeat (a new batch starts its own launches 2-4), and the launch after one this host asked to record.  Everything else about the
    // launch's claim order is decided inside the launch itself (order_select).
    volatile uint32_t* pinned = reinterpret_cast<volatile uint32_t*>(h->fresh_streak.p);  // [0] the run of non-repeats, [1] a recording waits, [2] the pause (written by order_commit at the START of a launch: as of the latest launch that has STARTED -- possibly one still in flight; benign, the rebuild kernels are stream-ordered behind it)
    // [2] = launches of the pause still to go after the launch that wrote the word | that launch's number << 8.  A caller that enqueues far ahead of the
    // device reads an OLD word: every launch of the shape enqueued since takes one launch off the pause.  (Round 6: without the age a burst of 200
    // launches enqueued behind a pause -- bench.py's repeated-batch extra -- stayed "paused" on the host for its whole length: the recordings of the
    // batch's launches 2-4 were never turned into an order.)
    const uint32_t w2 = pinned[2], skip_seen = w2 & 0xFFu, gen_seen = w2 >> 8;
    const uint32_t since = ((uint32_t)(h->gen - 1) - gen_seen) & 0xFFFFFFu;   // launches of the shape enqueued after the one that wrote the word
    const bool paused = skip_seen > 1u + since;  // (this launch and the next are still inside the pause: nothing records, nothing to rebuild)
    if (pinned[0] > 0u) h->rebuild_credit = 6;
    if (paused) h->rebuild_credit = 0;
    const uint32_t blocks = (n_base + kOrderTile - 1) / kOrderTile;
    if (h->gen >= 2 && !paused && (h->gen <= 6 || h->rebuild_credit > 0 || pinned[1] != 0u)) {
        hipLaunchKernelGGL(k_order_count, dim3(blocks), dim3(kOrderThreads), 0, stream, h->cost.p, h->ctl.p, h->parity, n_base);
        hipLaunchKernelGGL(k_order_scatter, dim3(blocks), dim3(kOrderThreads), 0, stream, h->cost.p, h->order.p, h->ctl.p, h->parity, n_base, h->fresh_streak.p);
    }
    if (h->rebuild_credit > 0) h->rebuild_credit -= 1;
    // the recording cadence of a batch past its fourth launch: one launch in 7, 8, 9, 7, ... of the shape (not a fixed period: two or three
    // batches alternating on the shape must all get their turn)
    c.want_record = 0;
    if (h->gen >= h->next_record && !paused) {
        c.want_record = 1;
        h->next_record = h->gen + 7 + (h->records_asked % 3);
        h->records_asked += 1;
        if (h->rebuild_credit < 1) h->rebuild_credit = 1;  // (the next launch gets the rebuild pair)
    }
    // (after rc_refit_device_async this is the last bound the host read back: it only scales the batch-recognition samples, never a hit)
    const float ex = s->root_max[0] - s->root_min[0], ey = s->root_max[1] - s->root_min[1], ez = s->root_max[2] - s->root_min[2];
    const float l2 = ex * ex + ey * ey + ez * ez;
    c.inv_l2 = (l2 > 0.f && l2 < 1e30f) ? 1.0f / l2 : 0.f;
    c.sample_rays = d_rays;
    c.n_sample = n;
    for (int k = 0; k < 8; ++k) c.sample_host[k] = host_sample ? host_sample[k] : 0.f;
    c.samples = h->samples.p;
    c.host_streak = h->fresh_streak.p;
    c.host_gen = (uint32_t)h->gen & 0xFFFFFFu;
    c.init_thr = (uint32_t)s->opt.cost_thr;
    c.close_dir_max = (s->opt.order_close_repeats && d_rays) ? kCloseDirMax : 0.f;  // (generated rays, described by one host sample, keep the exact rule)
    c.order = h->order.p;
    c.cost = h->cost.p;
    c.hist = h->ctl.p;
    c.parity = h->parity;  // the launch reads this copy of the header and writes the other: the shape's next launch reads that one
    h->parity ^= 1u;
    return true;
}

void rc_launch_trace(rc_scene* s, const RcRay* d_rays, RcHit* d_hits, uint64_t n, int any_hit, hipStream_t stream, bool learn_order) {
    if (n == 0) return;
    RcLaunchGuard launch(s, stream);  // serialises the enqueue: trace calls on one scene may come from several host threads
    uint32_t blocks = rc_grid_blocks(s, n, kBlock, PlainShape<>::kBlocksPerCu);
    uint32_t total_threads = blocks * kBlock;
    int64_t kernel = s->opt.kernel;  // the fall-back rules below choose for this launch only
    if (kernel < 0)  // auto: tiny batches gain nothing from refilling; a TLAS that fits the LDS planes (<= 256 instances) is read from there
        kernel = (n < (uint64_t)total_threads * 5 / 4) ? 0 : (s->n_tlas_nodes <= (uint32_t)kTlasLdsNodes ? 5 : 6);  // measured crossover (tools/archive/small_batch_probe.py): ~1.2 rays per resident lane
    if (kernel == 5 && s->n_tlas_nodes > (uint32_t)kTlasLdsNodes) kernel = 3;
    if (kernel == 6 && s->tlas_top_k + s->blas_top_k == 0) kernel = 3;  // nothing to stage
    if (kernel >= 3 && ((uint64_t)(s->n_flat_nodes + s->n_tlas_nodes) * 64u >= (1ull << 32) || n >= (1ull << 38))) kernel = 1;  // buffer offsets and chunk ids are 32-bit
    if (kernel == 5 || kernel == 6) {  // two 768-thread workgroups per CU (LdsShape and PartialShape share the grid)
        blocks = rc_grid_blocks(s, n, kMidBlock, s->opt.blocks_per_cu == 1 ? 1 : LdsShape<>::kBlocksPerCu);
        total_threads = blocks * kMidBlock;
    }
    TraceArgs a;
    a.v = rc_scene_view(launch, total_threads);
    if (any_hit && s->opt.entry_cull < 2) a.v.entry_cull = 0u;  // any_hit rays stop at their first hit and enter few instances that a cull would spare: the test costs what it saves (shadow rays -2 %); 2 = cull there too
    a.rays = d_rays; a.hits = d_hits; a.n_rays = n;
    rc_claim_fill(launch, n, total_threads / 64u, a.claim);
    a.refill = (int)s->opt.refill;
    a.sched_thr = (int)s->opt.sched_thr;
    a.stats = rc_stats_words(s);
    a.timeline = reinterpret_cast<unsigned long long*>(s->opt.timeline_ptr);
    const bool wide = rc_stack16(s);  // the STACK16 shape stages all of the renumbered tops, the 32-bit shape a prefix
    if (kernel == 5 && s->opt.blas_top) { a.blas_k = wide ? s->blas_top_k : s->blas_top_k32; a.lds_blas_base = (s->n_tlas_nodes + 1) / 2 - 1; }
    if (kernel == 6) {  // a plan made for the full-LDS kernels (<= 256 instances) has no TLAS renumbering: tlas_k = 0, its blas_k still fits
        a.tlas_k = wide ? s->tlas_top_k : s->tlas_top_k32; a.blas_k = s->opt.blas_top ? (wide ? s->blas_top_k : s->blas_top_k32) : 0; a.lds_blas_base = a.tlas_k;
    }
    launch.bind();
    if (learn_order && (kernel == 3 || kernel == 5 || kernel == 6) && !launch.capturing) rc_cost_order_setup(launch, n, any_hit, a.claim, d_rays);  // (the rebuild pair, when there is one, runs in front of the timed kernel)
    if (any_hit) launch_variant<true>(launch, kernel, a, blocks); else launch_variant<false>(launch, kernel, a, blocks);
    launch.finish();
}
