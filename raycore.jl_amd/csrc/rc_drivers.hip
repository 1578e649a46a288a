// rc_drivers.hip -- the analysis drivers that sit directly on closest_hit, run on the device.
//
// Replaces src/kernels.jl: generate_ray_grid (:10-56), hits_from_grid (:58-72), get_illumination (:112-124)
// and view_factors / view_factors! (:74-104) with their sampling helpers random_triangle_point,
// random_hemisphere_uniform, get_orthogonal_basis (src/math.jl:125-174).  The reference runs these as
// Threads.@threads CPU loops over closest_hit with a serial Dict histogram; here rays are generated in the
// kernel that traces them (no ray I/O) and results are accumulated with integer-valued device atomics,
// which are exact and order-independent.
//
// Determinism: the reference's view_factors uses the unseeded task-local RNG.  Here every (source
// primitive, ray index) pair draws its four uniforms from Philox4x32-10 keyed by the seed, so a result does
// not depend on the launch geometry or on how the job is sharded over GPUs.  sin/cos/acos are evaluated in
// f64 with fixed-order polynomial kernels (fdlibm coefficients) and rounded once to f32 -- Julia's Float32
// trig also evaluates in higher precision and rounds once -- so the CPU oracle, which uses the same formulas,
// generates bit-identical rays.
#include <hipcub/hipcub.hpp>

#include "rc_traverse_core.h"

#include <cmath>

namespace {

using namespace rc;

// norm(a) = sqrt(dot(a,a)); normalize(a) = a ./ norm(a) (GeometryBasics 0.5 fixed_arrays).
// sqrtf and / are the IEEE correctly-rounded forms here (-fhip-fp32-correctly-rounded-divide-sqrt); HIP's __fsqrt_rn is
// the NATIVE (approximate) square root unless OCML_BASIC_ROUNDED_OPERATIONS is defined, so it is not used.  On the host the builtin is sqrtf.
__host__ __device__ inline float3_ normalize3(float3_ a) {
    float n = __builtin_sqrtf(dot3(a, a));
    return mk3((a.x / n), (a.y / n), (a.z / n));
}

struct GridParams {  // everything generate_ray_grid computes before its double loop
    float gc[3], b1[3], b2[3], dir[3];
    float cell_w, cell_h;
    uint32_t grid;
};

// generate_ray_grid up to its loop (:10-46), as called from hits_from_grid (:58-61): ONE body for the host (the one-direction drivers, from
// the host copy of the world bound) and the device (k_grid_params, from the TLAS root as it is when the kernel runs).  Both sides are
// compiled with -ffp-contract=off and IEEE divide / square root, so they give the same bits; jl_min/jl_max give extrema() its Julia semantics.
__host__ __device__ inline GridParams grid_params(const float root_min[3], const float root_max[3], const float viewdir[3], uint32_t grid) {
    float3_ ray_direction = normalize3(mk3(viewdir[0], viewdir[1], viewdir[2]));
    float3_ direction = normalize3(ray_direction);
    float3_ o = mk3(root_min[0], root_min[1], root_min[2]);
    float3_ w = sub3(mk3(root_max[0], root_max[1], root_max[2]), o);
    float3_ temp = __builtin_fabsf(direction.x) < 0.9f ? mk3(1, 0, 0) : mk3(0, 1, 0);
    float3_ b1 = normalize3(cross3(direction, temp));
    float3_ b2 = normalize3(cross3(direction, b1));
    float min1 = INFINITY, max1 = -INFINITY, min2 = INFINITY, max2 = -INFINITY, mind = INFINITY;
    for (int c = 0; c < 8; ++c) {
        float3_ p = mk3(o.x + ((c & 1) ? 1.0f : 0.0f) * w.x, o.y + ((c & 2) ? 1.0f : 0.0f) * w.y, o.z + ((c & 4) ? 1.0f : 0.0f) * w.z);
        float p1 = dot3(p, b1), p2 = dot3(p, b2), pd = dot3(p, direction);
        min1 = jl_min(min1, p1); max1 = jl_max(max1, p1);
        min2 = jl_min(min2, p2); max2 = jl_max(max2, p2);
        mind = jl_min(mind, pd);
    }
    float margin = 0.05f * jl_max(max1 - min1, max2 - min2);
    float grid_width = max1 - min1 + 2.0f * margin, grid_height = max2 - min2 + 2.0f * margin;
    float min_depth = mind - margin;
    float c1 = (min1 + max1) / 2.0f, c2 = (min2 + max2) / 2.0f;
    float3_ gc = add3(add3(add3(mk3(0, 0, 0), scale3(direction, min_depth)), scale3(b1, c1)), scale3(b2, c2));
    GridParams g;
    g.gc[0] = gc.x; g.gc[1] = gc.y; g.gc[2] = gc.z;
    g.b1[0] = b1.x; g.b1[1] = b1.y; g.b1[2] = b1.z;
    g.b2[0] = b2.x; g.b2[1] = b2.y; g.b2[2] = b2.z;
    g.dir[0] = ray_direction.x; g.dir[1] = ray_direction.y; g.dir[2] = ray_direction.z;
    g.cell_w = grid_width / (float)grid; g.cell_h = grid_height / (float)grid;
    g.grid = grid;
    return g;
}
// The same for direction d of a DEVICE array, from the TLAS root as it is now (node 0; a one-instance scene's root is a leaf): what the
// many-direction drivers use, so that they follow an asynchronous refit or rebuild without the host ever reading the bound.
__device__ inline GridParams grid_params_device(const RcNode* tlas_nodes, uint32_t n_tlas_nodes, const float* dirs, uint32_t d, uint32_t grid) {
    float mn[3] = {0.f, 0.f, 0.f}, mx[3] = {0.f, 0.f, 0.f};
    if (n_tlas_nodes) host_root_aabb(tlas_nodes[0], true, mn, mx);
    const float v[3] = {dirs[3u * (size_t)d], dirs[3u * (size_t)d + 1u], dirs[3u * (size_t)d + 2u]};
    return grid_params(mn, mx, v, grid);
}
__global__ void k_grid_params(const RcNode* tlas_nodes, uint32_t n_tlas_nodes, const float* dirs, uint32_t n_dirs, uint32_t grid, GridParams* out) {
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d < n_dirs) out[d] = grid_params_device(tlas_nodes, n_tlas_nodes, dirs, d, grid);
}

// generate_ray_grid body (:47-55): u, v and the sum are Float64 ((grid_size+1)/2 is Float64) and round
// once into the Float32 point.
__device__ inline RcRay grid_ray(const GridParams& g, uint64_t idx) {
    uint32_t i = (uint32_t)(idx % g.grid) + 1, j = (uint32_t)(idx / g.grid) + 1;
    double half = ((double)g.grid + 1.0) / 2.0;
    double u = ((double)i - half) * (double)g.cell_w;
    double v = ((double)j - half) * (double)g.cell_h;
    RcRay r;
    r.ox = (float)(((double)g.gc[0] + u * (double)g.b1[0]) + v * (double)g.b2[0]);
    r.oy = (float)(((double)g.gc[1] + u * (double)g.b1[1]) + v * (double)g.b2[1]);
    r.oz = (float)(((double)g.gc[2] + u * (double)g.b1[2]) + v * (double)g.b2[2]);
    r.tmin = 0.0f; r.dx = g.dir[0]; r.dy = g.dir[1]; r.dz = g.dir[2]; r.tmax = INFINITY;
    return r;
}

__global__ __launch_bounds__(kBlock) void k_ray_grid(GridParams g, RcRay* out) {
    uint64_t n = (uint64_t)g.grid * g.grid;
    for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) store_ray(out, i, grid_ray(g, i));
}

// The grids of n_dirs directions in one launch: direction d's rays start at d * grid^2, in k_ray_grid's layout.  Every workgroup lays out
// the grid of the direction it writes (thread 0, into LDS) from the device arrays, so the call needs no scratch and no host copy of the bound.
__global__ __launch_bounds__(kBlock) void k_ray_grid_dirs(const RcNode* tlas_nodes, uint32_t n_tlas_nodes, const float* dirs, uint32_t n_dirs, uint32_t grid, RcRay* out) {
    __shared__ GridParams g;
    const uint64_t n = (uint64_t)grid * grid;
    for (uint32_t d = blockIdx.y; d < n_dirs; d += gridDim.y) {
        if (threadIdx.x == 0) g = grid_params_device(tlas_nodes, n_tlas_nodes, dirs, d, grid);
        __syncthreads();
        for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) store_ray(out + (uint64_t)d * n, i, grid_ray(g, i));
        __syncthreads();
    }
}

// hits_from_grid + the histogram of get_illumination (:58-72, :112-124) fused on the persistent phased traversal
// core: the ray is generated when a lane is refilled, and a finished ray does one f32 atomic add of 1.0 on the hit
// primitive's metadata slot (exact while counts < 2^24, as in the reference's Float32 sums).
struct GridSource {
    GridParams g;
    uint64_t first;
    __device__ inline RcRay operator()(uint64_t i) const { return grid_ray(g, first + i); }
    static constexpr bool kPrefetch = false;  // rays are generated, nothing to read ahead (ArraySource::prefetch)
};
// Counting into an accumulator array from inside a wave.  An atomic on ONE address costs ~12.7 ns on this chip whether or not it
// returns a value and however many lanes issue it (tools/archive/atomic_probe.hip), so a driver whose rays mostly land on a few large
// triangles (a ground plane under get_illumination: 10^5 hits on one counter = milliseconds) would be bound by that one word.
// The lanes that finish together first combine equal targets: up to four rounds of "the first pending lane's target, everyone
// with the same target, one atomic of the group's size", stopping at the first group of one (the common case of all-different
// targets then costs a single round); whatever is still pending adds its own 1.  Called by the active (finishing, counted) lanes only.
template <class T>
__device__ inline void wave_count(T* acc, unsigned long long index, bool counted) {
    bool pending = counted;
#pragma unroll 1
    for (int r = 0; r < 4; ++r) {
        const unsigned long long act = __ballot(pending);
        if (!act) return;
        const int leader = __ffsll((long long)act) - 1;
        const unsigned lo = __shfl((unsigned)index, leader), hi = __shfl((unsigned)(index >> 32), leader);
        const bool same = pending && index == (((unsigned long long)hi << 32) | lo);
        const unsigned long long grp = __ballot(same);
        if ((int)(threadIdx.x & 63u) == leader) atomicAdd(acc + index, (T)__popcll(grp));
        pending = pending && !same;
        if (__popcll(grp) == 1) break;  // a group of one: the targets are probably all different, stop looking for duplicates
    }
    if (pending) atomicAdd(acc + index, (T)1);
}

// get_illumination's histogram is a HOT vector (a few large, well-lit triangles take most of the hits: C5 seen from outside counts 6 852 rays on
// one wall triangle), and atomics onto a few cache lines serialise: the call took 0.59 ms where tracing the same rays takes 0.19.  The kernel
// counts into kHistCopies private u32 copies (by workgroup), each laid out transposed in rows of eight, and k_hist_fold (FoldF32Saturating) adds them into
// the caller's f32 vector with the reference's arithmetic: `counts[k] += 1f0` per ray (src/kernels.jl:119-121) is exact up to 2^24 and stays
// there, so counts = min(counts + hits, 2^24) in integers is the same number.  (Also tried: the traversal only STORES each ray's hit
// metadata and a streaming kernel counts afterwards -- two more launches and a 16 MB round trip: C3 0.62 ms instead of 0.57, C5 0.34 instead of 0.24.)
//
// The copy histogram, shared with the view-factor totals (`received` is as hot: 2 x 10^8 atomics onto a few hundred cache lines ran at HALF the
// rate of the matrix's scattered ones, C5 81 ms against 39): kHistCopies copies of 8 x n8 counters; a workgroup counts into copy blockIdx & 15;
// metadata index j sits at (j & 7) * n8 + (j >> 3), so neighbouring triangles -- a wall's two halves, a sphere's ring -- are in different cache lines.
constexpr uint32_t kHistCopies = 16;
struct CopyHist {
    uint32_t n8;  // ceil(n_prims / 8)
    __host__ __device__ __forceinline__ static CopyHist of(uint32_t n_prims) { return CopyHist{(n_prims + 7u) / 8u}; }
    __host__ __device__ __forceinline__ unsigned long long base(unsigned long long copy) const { return copy * 8u * n8; }  // first word of a copy
    __host__ __device__ __forceinline__ unsigned long long words() const { return base(kHistCopies); }                     // of one histogram
    __device__ __forceinline__ uint32_t slot(uint32_t j) const { return (j & 7u) * n8 + (j >> 3); }
    __device__ __forceinline__ static uint32_t copy() { return blockIdx.x & (kHistCopies - 1u); }
};
// The primitive metadata of a hit: the instance record's fourth 16 bytes hold its first flat primitive in .y (HitWriter reads the same words).
__device__ __forceinline__ uint32_t hit_meta(const RcInstRec* inst, const RcPrim* prims, int instance, uint32_t prim) {
    const uint4 m3 = *(reinterpret_cast<const uint4*>(inst + instance) + 3);
    return prims[m3.y + prim - 1u].meta;
}
// The sink of both illumination jobs: one count per hit on the slot of its primitive's metadata.  The one-direction job (DIRS = false) folds
// its copy's base into wave_count's pointer -- it has no register for a division by `cells`; the many-direction job folds direction and
// copy into the index: a wave straddles directions, and lanes are combined by index.
template <bool DIRS>
struct HistogramSinkT {
    const RcInstRec* inst;
    const RcPrim* prims;
    uint32_t n_prims;
    uint32_t* scratch;  // one histogram (DIRS: one per direction of the group), zeroed by the launcher
    CopyHist h;
    uint32_t cells;     // DIRS: grid^2, item i belongs to direction i / cells
    __device__ inline void operator()(uint64_t i, bool hit, float, float, float, uint32_t prim, int instance) const {
        uint32_t meta = 0;
        if (hit) meta = hit_meta(inst, prims, instance, prim);
        const bool counted = hit && meta >= 1 && meta <= n_prims;  // metadata outside 1..N is dropped (src/kernels.jl:123)
        const uint32_t j = meta - 1u;
        if (DIRS) {
            const uint32_t d = (uint32_t)i / cells;
            const unsigned long long copy = (unsigned long long)d * kHistCopies + h.copy();
            wave_count(scratch, counted ? h.base(copy) + h.slot(j) : 0ull, counted);
        } else
            wave_count(scratch + h.base(h.copy()), counted ? (unsigned long long)h.slot(j) : 0ull, counted);
    }
};
typedef HistogramSinkT<false> HistogramSink;
typedef HistogramSinkT<true> DirsHistogramSink;
// Adds the copies of `rows` histograms into the caller's array: one thread per (row, metadata index), Rule::add accumulates the sum.
// ACCUMULATES, atomically, under every rule: calls on several streams may share an array (shards traced concurrently into ONE vector
// used to be safe when the kernels themselves added with atomics).  A one-row rule indexes in 32 bits and never divides.
template <class Word, class Rule>
__global__ void k_hist_fold(const Word* scratch, CopyHist h, uint32_t n, Rule rule) {
    const typename Rule::Index t = blockIdx.x * (typename Rule::Index)blockDim.x + threadIdx.x;
    if (t >= (typename Rule::Index)rule.rows() * n) return;
    const uint32_t d = Rule::kRows ? (uint32_t)(t / n) : 0u, j = (uint32_t)(t - (typename Rule::Index)d * n);
    const Word* base = scratch + d * h.words();
    typename Rule::Sum sum = 0;
    // (h.base(c) + h.slot(j), written out and summed in 64 bits: through the helpers the address adds reassociate)
    for (uint32_t c = 0; c < kHistCopies; ++c) sum += base[(size_t)c * 8u * h.n8 + (j & 7u) * h.n8 + (j >> 3)];
    if (sum) rule.add(d, j, sum);
}
struct FoldOneRow {
    typedef uint32_t Index;
    typedef unsigned long long Sum;
    static constexpr bool kRows = false;
    __host__ __device__ static inline uint32_t rows() { return 1u; }
};
// get_illumination's f32 vector, with the reference's arithmetic: counts = min(counts + hits, 2^24) in integers (N compare-and-swaps per launch cost nothing)
struct FoldF32Saturating : FoldOneRow {
    float* counts;
    __device__ inline void add(uint32_t, uint32_t j, unsigned long long sum) const {
        uint32_t* word = reinterpret_cast<uint32_t*>(counts + j);
        uint32_t seen = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (;;) {
            const float before = __uint_as_float(seen);  // an integer below 2^24 unless the caller put something else there
            float after;
            if (before >= 0.0f && before <= 16777216.0f && before == (float)(uint32_t)before) {
                const unsigned long long total = (unsigned long long)(uint32_t)before + sum;
                after = total >= 16777216ull ? 16777216.0f : (float)(uint32_t)total;
            } else {  // not a count: add one by one like the reference would, up to where f32 stops moving
                after = before;
                for (unsigned long long k = 0; k < sum && k < 16777216ull; ++k) { const float nv = after + 1.0f; if (nv == after) break; after = nv; }
            }
            const uint32_t prev = atomicCAS(word, seen, __float_as_uint(after));
            if (prev == seen) break;
            seen = prev;
        }
    }
};
struct FoldAddU64 : FoldOneRow {  // the view-factor totals' `received`
    unsigned long long* out;
    __device__ inline void add(uint32_t, uint32_t j, unsigned long long sum) const { atomicAdd(out + j, sum); }
};
struct FoldAddU32Rows {  // the many-direction matrix: row d = direction d of the group
    typedef uint64_t Index;
    typedef uint32_t Sum;  // (a direction traces grid^2 < 2^32 rays)
    static constexpr bool kRows = true;
    uint32_t n_rows;
    uint32_t* counts;
    uint64_t row_stride;
    __host__ __device__ inline uint32_t rows() const { return n_rows; }
    __device__ inline void add(uint32_t d, uint32_t j, uint32_t sum) const { atomicAdd(counts + (uint64_t)d * row_stride + j, sum); }
};
// A driver job is the kernel argument of the three shells below: a trivially copyable struct of the job's own parameters that makes the
// Source and the Sink next to the kernel's SceneView.
// A job whose shells need another shape than the default says so in a specialisation of JobShapeFlags, next to the job (Shape* flags, rc_traverse_core.h).
template <class Job>
struct JobShapeFlags { static constexpr unsigned kPlain = 0u, kLds = 0u, kPartial = 0u; };
struct IlluminationJob {
    GridParams g;
    uint64_t ray_begin;
    uint32_t* scratch;
    CopyHist h;
    __device__ inline GridSource source(const SceneView&) const { return GridSource{g, ray_begin}; }
    __device__ inline HistogramSink sink(const SceneView& v) const { return HistogramSink{v.inst, v.prims, v.n_prims, scratch, h, 0u}; }
};
// Keeps the late pop in the plain and the partial shell: beside the sink's own arrays they have no register for the peeked stack top (80 VGPRs
// either way; with the peek their private segments grow from 92 to 124 and from 96 to 100 bytes).  The LDS shell peeks like the trace kernels,
// but keeps the pointer form of the interior loop's stack position: with the integer address (LaneStackP::addr_t) its private segment would
// grow from 92 to 108 bytes (docs/EXPERIMENTS.md, "VALU trims").  Neither the LDS layout nor its size depends on the flags.
template <>
struct JobShapeFlags<IlluminationJob> { static constexpr unsigned kPlain = ShapeLatePop, kLds = ShapePtrStack, kPartial = ShapeLatePop; };
// get_illumination for a GROUP of directions in one launch: work item i = d_local * grid^2 + cell.  The source reads direction d_local's
// GridParams (k_grid_params wrote them in front of the launch) and makes grid_ray()'s ray, bit for bit k_ray_grid's and GridSource's for that
// direction; the sink is HistogramSink with a base of d_local * kHistCopies * 8 * n8 -- folded into wave_count's index, not into its
// pointer: a wave straddles directions, and lanes are combined by index.  items = G * grid^2 < 2^32, so both divide in 32 bits.
struct DirsGridSource {
    const GridParams* params;
    uint32_t cells;  // grid^2
    __device__ inline RcRay operator()(uint64_t i) const {
        const uint32_t d = (uint32_t)i / cells, cell = (uint32_t)i - d * cells;
        return grid_ray(params[d], cell);
    }
    static constexpr bool kPrefetch = false;  // rays are generated, nothing to read ahead
};
// The many-direction job needs no shape flags: its source keeps a pointer where GridSource keeps fifteen grid words, and its shells peek in
// 76 / 77 / 80 VGPRs (plain / LDS / partial) with no private segment (docs/EXPERIMENTS.md, "Illumination over many directions").
struct IlluminationDirsJob {
    const GridParams* params;
    uint32_t cells;
    uint32_t* scratch;
    CopyHist h;
    __device__ inline DirsGridSource source(const SceneView&) const { return DirsGridSource{params, cells}; }
    __device__ inline DirsHistogramSink sink(const SceneView& v) const { return DirsHistogramSink{v.inst, v.prims, v.n_prims, scratch, h, cells}; }
};
// The three shapes every driver runs in (DriverLaunch picks one): they differ in what sits in LDS when phased_trace starts.
template <bool ANY, class Job>
__global__ __launch_bounds__(kBlock, 6) void k_driver(SceneView v, PersistArgs p, Job j) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    phased_trace<ANY, PlainShape<JobShapeFlags<Job>::kPlain>>(v, p, lds_stack, j.source(v), j.sink(v));
}
// Small top level (<= kTlasLdsNodes nodes): the shape of trace kernel 5 -- two 768-thread workgroups per CU, TLAS (and a single BLAS's
// top nodes) in LDS planes.
template <bool ANY, class Job>
__global__ __launch_bounds__(kMidBlock, 6) void k_driver_lds(SceneView v, PersistArgs p, Job j) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    typedef LdsShape<JobShapeFlags<Job>::kLds> Shape;
    const LdsTop top = Shape::prologue(smem, v, p.blas_k, p.lds_blas_base, p.tlas_k);
    phased_trace<ANY, Shape>(v, p, Shape::stacks(smem), j.source(v), j.sink(v), top);
}
// Larger top levels (the shape of trace kernel 6): only the breadth-first tops of the TLAS and of a single BLAS are staged.
template <bool ANY, class Job>
__global__ __launch_bounds__(kMidBlock, 6) void k_driver_partial(SceneView v, PersistArgs p, Job j) {
    typedef PartialShape<JobShapeFlags<Job>::kPartial> Shape;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const LdsTop top = Shape::prologue(smem, v, p.blas_k, p.lds_blas_base, p.tlas_k);
    phased_trace<ANY, Shape>(v, p, Shape::stacks(smem), j.source(v), j.sink(v), top);
}

// ---- Philox4x32-10 (Salmon et al., SC'11) ---------------------------------------------------------------
__device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ inline float u32_to_unit(uint32_t x) { return (float)(x >> 8) * 0x1.0p-24f; }

// ---- f64 trig with a fixed operation order (fdlibm kernels), valid for the ranges the sampler needs -----
// Also exact on [-pi/4, 0) (the diffuse bounce's theta): there x * two_over_pi + 0.5 lies in (-1, 0.5) (about -5e-9 at x = -pi/4 after
// rounding), the truncating cast gives k = 0, r = x exactly, and the fdlibm kernels are valid for |r| <= pi/4.
__device__ inline void sincos_f64(double x, double& s, double& c) {  // -pi/4 <= x <= 2 pi
    const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17, two_over_pi = 6.36619772367581382433e-01;
    int k = (int)(x * two_over_pi + 0.5);
    double r = (x - (double)k * pio2_hi) - (double)k * pio2_lo;
    double z = r * r;
    double sp = 8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)));
    double ks = r + (z * r) * (-1.66666666666666324348e-01 + z * sp);
    double cp = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 + z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
    double kc = 1.0 - (0.5 * z - z * cp);
    switch (k & 3) {
        case 0: s = ks; c = kc; break;
        case 1: s = kc; c = -ks; break;
        case 2: s = -ks; c = -kc; break;
        default: s = -kc; c = ks; break;
    }
}
__device__ inline double acos_f64(double x) {  // 0 <= x < 1
    const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17;
    const double pS0 = 1.66666666666666657415e-01, pS1 = -3.25565818622400915405e-01, pS2 = 2.01212532134862925881e-01,
                 pS3 = -4.00555345006794114027e-02, pS4 = 7.91534994289814532176e-04, pS5 = 3.47933107596021167570e-05,
                 qS1 = -2.40339491173441421878e+00, qS2 = 2.02094576023350569471e+00, qS3 = -6.88283971605453293030e-01,
                 qS4 = 7.70381505559019352791e-02;
    if (x < 0.5) {
        double z = x * x;
        double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        double r = p / q;
        return pio2_hi - (x - (pio2_lo - x * r));
    }
    double z = (1.0 - x) * 0.5;
    double s = __builtin_sqrt(z);  // IEEE f64 square root
    double df = __longlong_as_double(__double_as_longlong(s) & 0xFFFFFFFF00000000ll);
    double c = (z - df * df) / (s + df);
    double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    double r = p / q;
    double w = r * s + c;
    return 2.0 * (df + w);
}

// get_orthogonal_basis (src/math.jl:143-156): argmin(abs.(normal)) keeps the FIRST minimum on ties.
__device__ inline void orthogonal_basis(const float3_ normal, float3_& bu, float3_& bv) {
    float3_ n = normalize3(normal);
    float ax = fabsf(normal.x), ay = fabsf(normal.y), az = fabsf(normal.z);
    int mi = 1; float mv = ax;
    if (ay < mv) { mi = 2; mv = ay; }
    if (az < mv) { mi = 3; mv = az; }
    float3_ cand = mi == 1 ? mk3(1, 0, 0) : (mi == 2 ? mk3(0, 1, 0) : mk3(0, 0, 1));
    bv = normalize3(cross3(n, cand));
    bu = normalize3(cross3(bv, n));
}

__device__ inline float3_ cosine_hemisphere_dir(const float3_ n, float u1, float u2);  // (below, with the stages that shoot cosine-weighted rays)
// The ray of (source primitive, ray index) in the view-factor family (:83-92 + src/math.jl:125-174): the Philox draw -- counter (ray_idx, src,
// 0, 0), key = seed -> r1, r2, xi1, xi2 --, the point on the triangle and the origin pt + normal * 0.01f are the same in both samplings.
// COSINE = false: view_factors!'s own ray, the reference's uniform hemisphere (src/kernels.jl:92).  COSINE = true: d =
// cosine_hemisphere_dir(normal, xi1, xi2), the function of the bounce, AO and point-source stages applied to the triangle's unit normal
// with the third and fourth Philox words, not renormalised: the direction density of a Lambertian surface, so the counts are FORM
// factors.  t_min = 0, t_max = inf.  The sampling is a template parameter: the cosine path carries no f64 acos, the uniform path no disk mapping.
// `placed`: the third counter word, 0 in the per-triangle family; the placed family (below) passes the source's instance.
template <bool COSINE>
__device__ inline RcRay view_factor_ray(const RcPrim& tri, uint32_t src, uint32_t ray_idx, RcPhiloxKey key, uint32_t placed = 0u) {
    float3_ p1 = mk3(tri.v[0], tri.v[1], tri.v[2]), p2 = mk3(tri.v[3], tri.v[4], tri.v[5]), p3 = mk3(tri.v[6], tri.v[7], tri.v[8]);
    float3_ normal = normalize3(cross3(sub3(p2, p1), sub3(p3, p1)));  // GB.orthogonal_vector + normalize (:86-87)
    uint32_t rnd[4];
    philox4x32_10(ray_idx, src, placed, 0u, key.k0, key.k1, rnd);
    float r1 = u32_to_unit(rnd[0]), r2 = u32_to_unit(rnd[1]), xi1 = u32_to_unit(rnd[2]), xi2 = u32_to_unit(rnd[3]);
    // random_triangle_point (src/math.jl:158-174)
    float sqrt_r1 = __builtin_sqrtf(r1);
    float wu = 1.0f - sqrt_r1, wv = sqrt_r1 * (1.0f - r2), ww = sqrt_r1 * r2;
    float3_ pt = add3(add3(scale3(p1, wu), scale3(p2, wv)), scale3(p3, ww));
    float3_ o = add3(pt, scale3(normal, 0.01f));  // :91
    float3_ d;
    if (COSINE)
        d = cosine_hemisphere_dir(normal, xi1, xi2);
    else {  // random_hemisphere_uniform (src/math.jl:125-141)
        float3_ bu, bv;
        orthogonal_basis(normal, bu, bv);
        float theta = (float)acos_f64((double)xi1);
        float phi = (2.0f * 3.1415927f) * xi2;
        double st, ct, sp, cp;
        sincos_f64((double)theta, st, ct);
        sincos_f64((double)phi, sp, cp);
        float sin_t = (float)st, cos_t = (float)ct, sin_p = (float)sp, cos_p = (float)cp;
        float xl = sin_t * cos_p, yl = sin_t * sin_p, zl = cos_t;
        d = add3(add3(scale3(bu, xl), scale3(bv, yl)), scale3(normal, zl));
    }
    return RcRay{o.x, o.y, o.z, 0.0f, d.x, d.y, d.z, INFINITY};
}

// A shard of the view-factor family's work: rays [ray_begin, ray_begin + n_ray) of the sources at positions src_begin.. (vf_shard() makes
// it on the host).  Work item w is source position src_begin + w / n_ray, ray ray_begin + w % n_ray.
struct VfShard {
    RcPhiloxKey key;
    uint32_t src_begin, ray_begin, n_ray;
};
// view_factors! (:80-104): work item = (source primitive, ray); result[src_meta, hit_meta] += 1 when the hit
// primitive's metadata differs.  One u32 atomic per counted ray.  Runs on the persistent phased traversal core.
template <bool COSINE>
struct ViewFactorSource {
    const RcPrim* prims;
    const uint32_t* order;  // RC_VF_SOURCES_BY_METADATA: source position -> flat primitive index, else nullptr (position = index)
    VfShard sh;
    __device__ inline RcRay operator()(uint64_t w) const {
        const uint32_t pos = sh.src_begin + (uint32_t)(w / sh.n_ray), ray_idx = sh.ray_begin + (uint32_t)(w % sh.n_ray);
        const uint32_t src = order ? order[pos] : pos;
        return view_factor_ray<COSINE>(prims[src], src, ray_idx, sh.key);  // Philox is keyed by the PRIMITIVE index: the rays do not depend on the addressing
    }
    static constexpr bool kPrefetch = false;
};
// The (source, hit) pair of a finished item and the counting rule of view_factors! (:93-97): the hit primitive's metadata differs from the
// source's, and both are in 1..N.  The source is decoded for every item (the groups job counts a miss on its source's group), the hit
// (hit_meta) for a hit only.  `v` is the kernel's own by-value SceneView parameter: the sinks that call this keep a REFERENCE to it
// (Job::sink(v) in k_driver*), which lives as long as the kernel runs -- a sink made anywhere else must be given a view that outlives it.
struct VfPair {
    uint32_t pos, src, src_meta, to_meta;
    bool counted;
};
__device__ __forceinline__ VfPair vf_pair(const SceneView& v, const uint32_t* order, const VfShard& sh, uint64_t w, bool hit, uint32_t prim, int instance) {
    VfPair p;
    p.pos = sh.src_begin + (uint32_t)(w / sh.n_ray);
    p.src = order ? order[p.pos] : p.pos;
    p.to_meta = hit ? hit_meta(v.inst, v.prims, instance, prim) : 0u;  // (the hit's load first: in the other order the matrix job's shells change)
    p.src_meta = v.prims[p.src].meta;
    p.counted = hit && p.to_meta != p.src_meta && p.src_meta >= 1 && p.src_meta <= v.n_prims && p.to_meta >= 1 && p.to_meta <= v.n_prims;
    return p;
}
struct ViewFactorSink {
    const SceneView& v;
    const uint32_t* order;
    VfShard sh;
    uint32_t* matrix;
    uint64_t row_stride, col_stride;
    uint32_t row_offset, flags;
    __device__ inline void operator()(uint64_t w, bool hit, float, float, float, uint32_t prim, int instance) const {
        bool counted = false;
        unsigned long long index = 0;
        if (hit) {
            const VfPair p = vf_pair(v, order, sh, w, true, prim, instance);
            counted = p.counted;
            const uint32_t row = (flags & 4u) ? p.src_meta - 1 : ((flags & 2u) ? p.pos : ((flags & 1u) ? p.src : p.src_meta - 1));
            if (counted) index = (uint64_t)(row - row_offset) * row_stride + (uint64_t)(p.to_meta - 1) * col_stride;
        }
        wave_count(matrix, index, counted);
    }
};
// Per-triangle TOTALS of the same job (rc_view_factor_totals*): the column sums received[j] = sum_i result[i, j] -- what the reference's own
// use of the matrix reads off it (docs/src/viewfactors_content.md:62-68: sum(view(viewf_matrix, :, i))) -- and the row sums emitted[i] = sum_j
// result[i, j], accumulated directly: two u64 atomics per counted ray, no N x N array anywhere.  Same rays, same counting rule as
// ViewFactorSink (:93-97); 64-bit so that N x rays_per_triangle may pass 2^32.
// `received` is the hot vector -- most rays of a closed scene end on a few large triangles --, so the kernel counts it into a copy histogram
// of u64 words (CopyHist), and k_hist_fold adds the copies into the caller's vector afterwards.
struct ViewFactorTotalsSink {
    const SceneView& v;
    VfShard sh;
    unsigned long long* received;  // one histogram of scratch counters (zeroed by the launcher), or nullptr
    CopyHist h;
    unsigned long long* emitted;   // [n_prims] or nullptr: per source, nearly wave-uniform -- one atomic per group (wave_count)
    __device__ inline void operator()(uint64_t w, bool hit, float, float, float, uint32_t prim, int instance) const {
        VfPair p{0u, 0u, 1u, 1u, false};
        if (hit) p = vf_pair(v, nullptr, sh, w, true, prim, instance);
        if (received) wave_count(received + h.base(h.copy()), (unsigned long long)h.slot(p.to_meta - 1u), p.counted);
        if (emitted) wave_count(emitted, (unsigned long long)(p.src_meta - 1u), p.counted);
    }
};
struct ViewFactorTotalsJob {
    VfShard sh;
    unsigned long long* received;
    CopyHist h;
    unsigned long long* emitted;
    __device__ inline ViewFactorSource<false> source(const SceneView& v) const { return ViewFactorSource<false>{v.prims, nullptr, sh}; }
    __device__ inline ViewFactorTotalsSink sink(const SceneView& v) const { return ViewFactorTotalsSink{v, sh, received, h, emitted}; }
};
// Keeps the pointer form of the interior loop's stack position in the plain shell: 79 VGPRs, 36 bytes of private segment with the integer form.
template <>
struct JobShapeFlags<ViewFactorTotalsJob> { static constexpr unsigned kPlain = ShapePtrStack, kLds = 0u, kPartial = 0u; };
// The weighted sibling of wave_count: acc[index] += value from every active lane, one atomic per group of equal targets carrying the group's
// SUM.  Called under phased_trace's `if (fin)`, by a divergent subset of the wave, so it reads no lane it has not just balloted: the leader's
// index with a readlane, then the group's values one readlane per set bit of the group's ballot, added in scalar registers (u64: 64 values
// of up to 2^32 - 1 need 38 bits).  A butterfly over all 64 lanes would read registers of lanes that are not executing.
// (Also built: bit-plane ballots, sum = sum_b 2^b * popcount(ballot(in group && bit b of value)), 32 ballots whatever the group's size --
// docs/EXPERIMENTS.md, "View-factor products".)
__device__ inline void wave_add(unsigned long long* acc, uint32_t index, uint32_t value, bool active) {
    bool pending = active;
#pragma unroll 1
    for (int r = 0; r < 4; ++r) {
        const unsigned long long act = __ballot(pending);
        if (!act) return;
        const int leader = __ffsll((long long)act) - 1;
        const uint32_t target = (uint32_t)__builtin_amdgcn_readlane((int)index, leader);
        const bool same = pending && index == target;
        const unsigned long long grp = __ballot(same);
        unsigned long long sum = 0;
#pragma unroll 1
        for (unsigned long long m = grp; m; m &= m - 1ull) sum += (uint32_t)__builtin_amdgcn_readlane((int)value, __ffsll((long long)m) - 1);
        if ((int)(threadIdx.x & 63u) == leader) atomicAdd(acc + index, sum);
        pending = pending && !same;
        if (__popcll(grp) == 1) break;  // a group of one: the targets are probably all different, stop looking for duplicates
    }
    if (pending) atomicAdd(acc + index, (unsigned long long)value);
}
// The view-factor matrix applied to a vector without the matrix (rc_view_factor_products*): with M = the reference's
// result[src_meta, hit_meta] (:93-97), every counted ray from metadata a that hits metadata b adds x[b - 1] to mx[a - 1] = (M x)[a - 1] and
// x[a - 1] to mtx[b - 1] = (M^T x)[b - 1], in u64 modulo 2^64 -- exact in any order, so any partition of sources x rays gives the same
// words.  Same source, same rays, same counting rule as ViewFactorTotalsSink, whose vectors these are for x = 1.  x is read for counted rays
// only: both metadata are in 1..N then.  mtx is the hot vector and goes through the copy histogram like `received`; mx is per source and
// nearly wave-uniform in its target like `emitted`, but its lanes add different values (wave_add).
struct ViewFactorProductsSink {
    const RcInstRec* inst;
    const RcPrim* prims;
    uint32_t n_prims, src_begin, n_ray;
    const uint32_t* x;
    unsigned long long* mtx;  // one histogram of scratch words (zeroed by the launcher), or nullptr
    CopyHist h;
    unsigned long long* mx;   // [n_prims] or nullptr
    __device__ inline void operator()(uint64_t w, bool hit, float, float, float, uint32_t prim, int instance) const {
        bool counted = false;
        uint32_t to_meta = 1, src_meta = 1;
        // vf_pair(), written out on fields of the sink's own: through the helper (and a SceneView reference) the three shells of this job change,
        // and the default shell then timed 0.048 ms slower on the reduced C5 where the parent's own runs spread 0.041 (docs/EXPERIMENTS.md,
        // "Drivers: the view-factor, hit-sample and row-group jobs written once", and profiles/drivers_write_once_ab.txt).  This form compiles to the code it had before.
        if (hit) {
            const uint32_t src = src_begin + (uint32_t)(w / n_ray);
            const uint4 m3 = *(reinterpret_cast<const uint4*>(inst + instance) + 3);
            to_meta = prims[m3.y + prim - 1u].meta; src_meta = prims[src].meta;
            counted = to_meta != src_meta && src_meta >= 1 && src_meta <= n_prims && to_meta >= 1 && to_meta <= n_prims;
        }
        if (mtx) wave_add(mtx + h.base(h.copy()), h.slot(to_meta - 1u), counted ? x[src_meta - 1u] : 0u, counted);
        if (mx) wave_add(mx, src_meta - 1u, counted ? x[to_meta - 1u] : 0u, counted);
    }
};
struct ViewFactorProductsJob {
    VfShard sh;
    const uint32_t* x;
    unsigned long long* mtx;
    CopyHist h;
    unsigned long long* mx;
    __device__ inline ViewFactorSource<false> source(const SceneView& v) const { return ViewFactorSource<false>{v.prims, nullptr, sh}; }
    __device__ inline ViewFactorProductsSink sink(const SceneView& v) const { return ViewFactorProductsSink{v.inst, v.prims, v.n_prims, sh.src_begin, sh.n_ray, x, mtx, h, mx}; }
};
struct ViewFactorJob {
    VfShard sh;
    uint32_t* matrix;
    uint64_t row_stride, col_stride;
    uint32_t row_offset, flags;
    const uint32_t* order;
    __device__ inline ViewFactorSource<false> source(const SceneView& v) const { return ViewFactorSource<false>{v.prims, order, sh}; }
    __device__ inline ViewFactorSink sink(const SceneView& v) const { return ViewFactorSink{v, order, sh, matrix, row_stride, col_stride, row_offset, flags}; }
};

// The sparse view-factor matrix (rc_view_factors_sparse*): the same job once more, but the matrix itself is kept, as CSR.  A chunk of whole
// rows is traced with the sources in metadata order; work item w stores ONE u64 key at pairs[w] -- (row - the chunk's first row) << col_bits
// | col for a counted ray (the rule of :93-97), `sentinel` = 1 << (row_bits + col_bits), which sorts behind every key, for any other ray.
// One plain store per finished ray at an index below the launch's item count, no atomics: the keys are sorted and run-length encoded
// afterwards (rc_launch_vf_sparse), so the arrays do not depend on which wave traced what.
struct ViewFactorPairsSink {
    const SceneView& v;
    const uint32_t* order;
    VfShard sh;
    uint32_t row0, col_bits;
    unsigned long long sentinel;
    unsigned long long* pairs;
    __device__ inline void operator()(uint64_t w, bool hit, float, float, float, uint32_t prim, int instance) const {
        unsigned long long key = sentinel;
        if (hit) {
            const VfPair p = vf_pair(v, order, sh, w, true, prim, instance);
            if (p.counted) key = ((unsigned long long)(p.src_meta - 1u - row0) << col_bits) | (p.to_meta - 1u);
        }
        pairs[w] = key;
    }
};
struct ViewFactorPairsJob {
    VfShard sh;  // (whole rows: ray_begin = 0)
    uint32_t row0, col_bits;
    unsigned long long sentinel;
    unsigned long long* pairs;
    const uint32_t* order;
    __device__ inline ViewFactorSource<false> source(const SceneView& v) const { return ViewFactorSource<false>{v.prims, order, sh}; }
    __device__ inline ViewFactorPairsSink sink(const SceneView& v) const { return ViewFactorPairsSink{v, order, sh, row0, col_bits, sentinel, pairs}; }
};
// Appends one chunk's compressed keys to the CSR arrays.  unique / lengths / n_runs: the run-length encoding of the chunk's SORTED keys, on
// the device; the sentinel's run, if there is one, is the last and is dropped.  Entry i goes to position *nnz_in + i of cols / vals unless
// that is at or beyond `capacity`; the row's count (row_count, indexed from the job's first row; `row0` = the chunk's first row in it) grows
// by one per entry -- consecutive entries of a row are consecutive lanes, so a wave adds once per row it touches --; *nnz_out = *nnz_in +
// entries.  nnz_in and nnz_out are different words: every workgroup reads the one, the first writes the other.  The grid is sized by the
// chunk's rays, an upper bound of its entries that the host knows.
__global__ __launch_bounds__(256) void k_vf_sparse_append(const unsigned long long* unique, const uint32_t* lengths, const uint32_t* n_runs,
                                                          unsigned long long sentinel, uint32_t col_bits, uint32_t row0,
                                                          const unsigned long long* nnz_in, unsigned long long* nnz_out, uint32_t* cols,
                                                          uint32_t* vals, unsigned long long capacity, unsigned long long* row_count) {
    const uint32_t runs = *n_runs;
    const uint32_t entries = runs - ((runs && unique[runs - 1u] == sentinel) ? 1u : 0u);
    const unsigned long long base = *nnz_in;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i0 = (uint64_t)blockIdx.x * 256u; i0 < entries; i0 += (uint64_t)gridDim.x * 256u) {  // (uniform per workgroup: every lane reaches the ballot)
        const uint64_t i = i0 + threadIdx.x;
        const bool active = i < entries;
        const unsigned long long key = active ? unique[i] : 0ull;
        const uint32_t row = (uint32_t)(key >> col_bits);
        if (active && base + i < capacity) {
            cols[base + i] = (uint32_t)(key & ((1ull << col_bits) - 1ull));
            vals[base + i] = lengths[i];
        }
        const uint32_t before = __shfl_up(row, 1);
        const bool first = active && (lane == 0u || before != row);
        const unsigned long long ends = __ballot(first || !active);  // where a group of equal rows ends: at the next first lane, or at the first idle one
        if (first) {
            const unsigned long long behind = ends & ~((2ull << lane) - 1ull);
            const uint32_t n = (behind ? (uint32_t)__ffsll((long long)behind) - 1u : 64u) - lane;
            atomicAdd(row_count + row0 + row, (unsigned long long)n);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *nnz_out = base + entries;
}
// The products of a CSR block with a vector (rc_view_factor_sparse_products_device): one wave per row, the lanes stride the row's entries
// with coalesced loads of cols / vals and gather x.  mx[row_offset + r] += sum_k vals[k] * x[cols[k]]: a u64 butterfly over the wave and one
// atomic per row (atomic, so that row blocks on several streams may share a vector).  mtx[cols[k]] += vals[k] * x[row_offset + r]: one u64
// atomic per entry -- a row's columns are all different, so there is nothing to combine inside a wave.  All sums modulo 2^64.  The row
// bounds come from row_ptr on the device: the grid depends on n_rows alone.
// (Also built: 16 lanes per row, four rows per wave -- equal at rows of some 40 entries, 1.24 x and 1.44 x slower at the rows of the reduced
// and the full C5: docs/EXPERIMENTS.md, "Sparse view-factor matrix".)
__global__ __launch_bounds__(256) void k_vf_sparse_products(uint32_t n_rows, uint32_t row_offset, const unsigned long long* row_ptr, const uint32_t* cols,
                                                            const uint32_t* vals, const uint32_t* x, unsigned long long* mx, unsigned long long* mtx) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_waves = (uint64_t)gridDim.x * 4u;
    for (uint64_t r = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); r < n_rows; r += n_waves) {
        const unsigned long long begin = row_ptr[r], end = row_ptr[r + 1u];
        const unsigned long long xr = mtx ? x[row_offset + r] : 0u;
        unsigned long long sum = 0;
        for (unsigned long long k = begin + lane; k < end; k += 64u) {
            const uint32_t c = cols[k];
            const unsigned long long v = vals[k];
            if (mx) sum += v * x[c];
            if (xr) atomicAdd(mtx + c, v * xr);
        }
        if (mx) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
            if (lane == 0u && sum) atomicAdd(mx + row_offset + r, sum);
        }
    }
}

__global__ void k_meta_keys(const RcPrim* prims, uint32_t n, uint32_t* keys, uint32_t* vals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { keys[i] = prims[i].meta; vals[i] = i; }
}

// The composed stage: the rays [ray_begin, ray_begin + n_ray) of one source primitive.
template <bool COSINE>
__global__ void k_view_factor_rays(SceneView v, RcPhiloxKey key, uint32_t src, uint32_t ray_begin, uint32_t n_ray, RcRay* out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_ray) out[i] = view_factor_ray<COSINE>(v.prims[src], src, ray_begin + i, key);
}

// ---- wavefront stages adjacent to the trace (docs/src/wavefront-renderer.jl:296-333) ---------
// Geometric world-space normal of a hit: normalize(cross(v1-v0, v2-v0)) of the hit primitive carried through the
// instance's inverse-transpose, flipped to face the ray origin.
__device__ inline void hit_frame(const SceneView& v, const RcRay& r, const RcHit& h, float3_& point, float3_& normal) {
    point = add3(mk3(r.ox, r.oy, r.oz), scale3(mk3(r.dx, r.dy, r.dz), h.t));  // hit_point = ray.o + ray.d * dist (:302)
    const RcPrim tri = v.prims[h.primitive_id];
    const float3_ v0 = mk3(tri.v[0], tri.v[1], tri.v[2]), v1 = mk3(tri.v[3], tri.v[4], tri.v[5]), v2 = mk3(tri.v[6], tri.v[7], tri.v[8]);
    const float3_ nl = cross3(sub3(v1, v0), sub3(v2, v0));
    const float* m = v.inst[h.instance_id].inv;  // n_w = transpose(inv 3x3) * n_l
    float3_ nw = mk3(m[0] * nl.x + m[4] * nl.y + m[8] * nl.z, m[1] * nl.x + m[5] * nl.y + m[9] * nl.z, m[2] * nl.x + m[6] * nl.y + m[10] * nl.z);
    nw = normalize3(nw);
    if (dot3(nw, mk3(r.dx, r.dy, r.dz)) > 0.0f) nw = mk3(-nw.x, -nw.y, -nw.z);
    normal = nw;
}

__global__ void k_hit_points(SceneView v, const RcRay* rays, const RcHit* hits, uint64_t n, float* points, float* normals) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        float3_ p = mk3(0, 0, 0), nn = mk3(0, 0, 0);
        const RcHit h = hits[i];
        if (h.hit) hit_frame(v, rays[i], h, p, nn);
        points[3 * i] = p.x; points[3 * i + 1] = p.y; points[3 * i + 2] = p.z;
        if (normals) { normals[3 * i] = nn.x; normals[3 * i + 1] = nn.y; normals[3 * i + 2] = nn.z; }
    }
}

// The placed index of a hit record (rc_placed_hit_indices_device): q = base[instance_id] + (primitive_id - the instance's first flat
// primitive), base = rc_scene::d_placed_base (the index space of "form factors between instances" below); RC_INVALID_ID for a miss.
__global__ void k_placed_hit_indices(SceneView v, const uint32_t* base, const RcHit* hits, uint64_t n, uint32_t* out) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const RcHit h = hits[i];
        uint32_t q = 0xFFFFFFFFu;  // RC_INVALID_ID
        if (h.hit) q = base[h.instance_id] + (h.primitive_id - v.inst[h.instance_id].prims_offset);
        out[i] = q;
    }
}

// generate_shadow_rays! for one point light (:288-333): slot i of the output belongs to ray i; misses get the
// reference's dummy ray (o = 0, d = (0,0,1), t_max = 0), hits a ray from hit_point + normal*bias toward the light with
// t_max = distance, ready for rc_trace_any_device.
// The shadow ray of one hit toward one light (:296-329): shared by the stage kernel and the fused visibility driver, so the two agree bit for bit.
__device__ inline RcRay shadow_ray_from(const float3_ p, const float3_ nn, const float3_ light, float bias) {  // (p, nn): the hit's frame
    const float3_ o = add3(p, scale3(nn, bias));
    const float3_ lv = sub3(light, o);
    const float dist = __builtin_sqrtf(dot3(lv, lv));
    return RcRay{o.x, o.y, o.z, 0.f, (lv.x / dist), (lv.y / dist), (lv.z / dist), dist};
}
__device__ inline RcRay shadow_ray(const SceneView& v, const RcRay& r, const RcHit& h, const float3_ light, float bias) {
    float3_ p, nn;
    hit_frame(v, r, h, p, nn);
    return shadow_ray_from(p, nn, light, bias);
}

// ---- the hit-sample family: work items are (hit slot, sub-item), the ray of an item is made from the slot's primary ray and hit ----------
// An item description (ShadowItems, SoftShadowItems, AoItems) holds the family's parameters `q` and gives slot(j), the hit slot of item j;
// ray(v, j, i, r, h), the ray of item j of slot i whose primary ray r hit (h); and kGate, whether an item whose ray has a t_max that is
// not > 0 is dead.  One description serves the composed stage and the fused driver's source, so the two agree bit for bit.
// The composed stage: slot j of the output belongs to item j; an item whose primary ray missed gets the reference's dummy ray.  The output
// feeds rc_trace_any_device unchanged (which applies the t_max gate to the stored ray itself).  total < 2^32.
template <class Items>
__global__ void k_hit_item_rays(SceneView v, Items it, uint64_t total, RcRay* out) {
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < total; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t i = it.slot((uint32_t)j);
        RcRay r = RC_DUMMY_RAY;
        const RcHit h = it.q.hits[i];
        if (h.hit) r = it.ray(v, (uint32_t)j, i, it.q.rays[i], h);
        store_ray(out, j, r);
    }
}
// The fused driver's source: the ray is made when a lane is refilled and never stored, so only the kernel can apply the gate of
// test_shadow_rays! (:353-358), `ray.t_max > 0 ? !any_hit(...) : false`: an item whose primary ray missed, or (kGate) whose ray has a t_max
// that is not > 0 (0: the light sits on the shadow origin; NaN: a NaN t or normal out of a singular instance), gets the dead ray.
template <class Items>
struct HitItemSource {
    const SceneView& v;
    Items it;
    __device__ inline RcRay operator()(uint64_t j) const {
        const uint32_t i = it.slot((uint32_t)j);
        const RcHit h = it.q.hits[i];
        if (!h.hit) return RC_DEAD_RAY;
        const RcRay r = it.ray(v, (uint32_t)j, i, load_ray(it.q.rays, i), h);
        return (!Items::kGate || r.tmax > 0.0f) ? r : RC_DEAD_RAY;
    }
    static constexpr bool kPrefetch = false;  // rays are generated, nothing to read ahead
};

// The Philox draw of a path-keyed sample: path = path_base + (path_in ? path_in[i] : i) fills the first two counter words, the caller's
// c2 and c3 the others.  Returns the path.
__device__ inline uint64_t path_philox(uint64_t path_base, const uint32_t* path_in, uint32_t i, uint32_t c2, uint32_t c3, RcPhiloxKey key, uint32_t rnd[4]) {
    const uint64_t path = path_base + (path_in ? (uint64_t)path_in[i] : (uint64_t)i);
    philox4x32_10((uint32_t)path, (uint32_t)(path >> 32), c2, c3, key.k0, key.k1, rnd);
    return path;
}

// generate_shadow_rays! + test_shadow_rays! for all hits x all lights (:279-362) fused on the persistent phased traversal core: work item
// j = i * n_lights + l is hit i seen from light l (the reference's slot (idx-1)*NLights + light_idx), so neighbouring lanes share a hit's
// records; a finished any_hit writes the one byte the shading reads, 0 for a dead item.  STAGE: generate_shadow_rays! for ONE point light
// given by value (`light`; q.lights is null and q.n_lights 1), item j = slot j.
template <bool STAGE>
struct ShadowItems {
    ShadowParams q;
    float light[3];
    static constexpr bool kGate = true;
    __device__ inline uint32_t slot(uint32_t j) const { return STAGE ? j : j / q.n_lights; }  // (n * n_lights < 2^32)
    __device__ inline RcRay ray(const SceneView& v, uint32_t j, uint32_t i, const RcRay& r, const RcHit& h) const {
        const float* lp = STAGE ? light : q.lights + 3u * (size_t)(j - i * q.n_lights);  // q.lights is read here: a captured launch follows lights that move between replays
        return shadow_ray(v, r, h, mk3(lp[0], lp[1], lp[2]), q.bias);
    }
};
struct VisibilitySink {
    uint8_t* visible;
    // A ray that missed comes back with the t_max it went in with (the core's closest_t starts there and only an accepted hit lowers it):
    // > 0 for a live shadow ray, -1 for a dead item -- whose byte is 0, not "visible" -- and 0 from the empty-scene path.
    __device__ inline void operator()(uint64_t j, bool hit, float t, float, float, uint32_t, int) const {
        visible[j] = (!hit && t > 0.0f) ? 1u : 0u;
    }
};
// The job's kernel argument (k_driver*): its parameters, and the Source / Sink they become next to the kernel's SceneView.
struct ShadowJob {
    ShadowParams q;
    uint8_t* visible;
    __device__ inline HitItemSource<ShadowItems<false>> source(const SceneView& v) const { return {v, {q, {}}}; }  // (v: the kernel's own by-value parameter)
    __device__ inline VisibilitySink sink(const SceneView&) const { return VisibilitySink{visible}; }
};

// ---- soft shadows: every light a small area light, `samples` shadow rays per (hit, light) -------------------------------------------
// compute_light(...; shadow_samples) of the reference's tutorial (docs/src/raytracing-core.jl:58-99; compute_multi_light :119-129 runs it for
// every light): shadow_factor = visible samples / shadow_samples.  The sampled target (:61-81), with the unseeded rand(Vec3f) replaced by
// Philox4x32-10(counter = (lo32 path, hi32 path, s | depth << 16, 0x53460000 | l), key = seed) -- three 24-bit uniforms, the bounce stage's
// conversion:
//   p = hit point; lv = light - p; light_dir = lv / sqrt(dot3(lv, lv))
//   samples == 1: target = light, no random number is drawn (:74-81)
//   samples  > 1: off_k = (r_k * 2 - 1) * radius;  off = off - light_dir * dot3(off, light_dir);  target = light + off
// every expression left to right, no contraction.  The ray toward the target is shadow_ray_from()'s, the body of shadow_ray(): origin = the biased hit point, t_max = the
// distance to the target (the wavefront renderer's convention, not the tutorial's t_max = Inf followed by hit_dist >= shadow_dist: a
// first-found any_hit beyond the light would otherwise decide visibility).
// Work item j = (i * n_lights + l) * samples + s (SoftShadowParams, rc_internal.h), so the samples of a (hit, light) pair and the lights
// of a hit sit in neighbouring lanes and share the hit's records.  ShadowItems' gate.
struct SoftShadowItems {
    SoftShadowParams q;
    static constexpr bool kGate = true;
    __device__ inline uint32_t slot(uint32_t j) const { return j / q.samples / q.n_lights; }  // (n * n_lights * samples < 2^32)
    // The shadow ray of sample s of light l seen from slot i
    __device__ inline RcRay ray(const SceneView& v, uint32_t j, uint32_t i, const RcRay& r, const RcHit& h) const {
        const uint32_t il = j / q.samples, s = j - il * q.samples, l = il - i * q.n_lights;
        const float* lp = q.lights + 3u * (size_t)l;
        const float3_ light = mk3(lp[0], lp[1], lp[2]);
        float3_ target = light;
        float3_ p, nn;
        hit_frame(v, r, h, p, nn);  // once: the target's light_dir and the ray's origin come from the same frame
        if (q.samples > 1u) {
            const float3_ lv = sub3(light, p);
            const float ld = __builtin_sqrtf(dot3(lv, lv));
            const float3_ light_dir = mk3((lv.x / ld), (lv.y / ld), (lv.z / ld));
            uint32_t rnd[4];
            path_philox(q.path_base, q.path_in, i, s | (q.depth << 16), 0x53460000u | l, q.key, rnd);
            const float radius = q.radii[l];
            float3_ off = mk3((u32_to_unit(rnd[0]) * 2.0f - 1.0f) * radius, (u32_to_unit(rnd[1]) * 2.0f - 1.0f) * radius, (u32_to_unit(rnd[2]) * 2.0f - 1.0f) * radius);
            off = sub3(off, scale3(light_dir, dot3(off, light_dir)));
            target = add3(light, off);
        }
        return shadow_ray_from(p, nn, target, q.bias);
    }
};
// count[i * n_lights + l] += 1 for a visible sample (VisibilitySink's rule: a miss that comes back with a t_max > 0).  One relaxed
// agent-scope u32 add per visible sample: integer adds are exact in any order, so the counts are reproducible; shadowed, gated and
// missed items add nothing.
struct VisibilityCountSink {
    uint32_t* count;
    uint32_t samples;
    __device__ inline void operator()(uint64_t j, bool hit, float t, float, float, uint32_t, int) const {
        if (!hit && t > 0.0f) __hip_atomic_fetch_add(count + (uint32_t)j / samples, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
struct SoftShadowJob {
    SoftShadowParams q;
    uint32_t* count;
    __device__ inline HitItemSource<SoftShadowItems> source(const SceneView& v) const { return {v, {q}}; }  // (v: the kernel's own by-value parameter)
    __device__ inline VisibilityCountSink sink(const SceneView&) const { return VisibilityCountSink{count, q.samples}; }
};

// cosine_sample_hemisphere (src/math.jl:1-21, concentric disk) in the frame (bu, bv, n), combined as random_hemisphere_uniform does
// (u*x + v*y + n*z, not renormalised).  pi is Float32(pi); cos / sin of theta in [-pi/4, 3pi/4] through sincos_f64, rounded once.
__device__ inline float3_ cosine_hemisphere_dir(const float3_ n, float u1, float u2) {
    const float pi = 3.1415927f;
    const float ox = 2.0f * u1 - 1.0f, oy = 2.0f * u2 - 1.0f;
    float dx = 0.0f, dy = 0.0f;
    if (!(ox == 0.0f && oy == 0.0f)) {  // offset ≈ 0f0 with the default tolerances is exact zero
        float r, theta;
        if (fabsf(ox) > fabsf(oy)) { r = ox; theta = ((oy / ox) * pi) / 4.0f; }
        else { r = oy; theta = pi / 2.0f - ((ox / oy) * pi) / 4.0f; }
        double st, ct;
        sincos_f64((double)theta, st, ct);
        dx = r * (float)ct; dy = r * (float)st;
    }
    const float z = __builtin_sqrtf(fmaxf(0.0f, (1.0f - dx * dx) - dy * dy));
    float3_ bu, bv;
    orthogonal_basis(n, bu, bv);
    return add3(add3(scale3(bu, dx), scale3(bv, dy)), scale3(n, z));
}

// ---- ambient occlusion: `samples` cosine-weighted any_hit rays of length max_dist over the hemisphere of every hit ---------------------
// Sample s of slot i: (p, nn) = hit_frame; (u1, u2) = the first two words of Philox4x32-10(counter = (lo32 path, hi32 path, s,
// 0x414F0000 | depth), key = seed) through the bounce stage's 24-bit conversion; d = cosine_hemisphere_dir(nn, u1, u2), not renormalised;
// the ray is o = p + nn * bias, t_min = 0, d, t_max = max_dist.  Every expression left to right, no contraction.  The visible fraction
// count / samples is the cosine-weighted openness of the hemisphere (the sky-view factor of the point with max_dist = Inf).
// The cosine-weighted ray off a hit's frame (p, nn): o = p + nn * bias, d = cosine_hemisphere_dir(nn, u1, u2) from the first two Philox
// words through the 24-bit conversion, [0, t_max].  Shared by the ambient-occlusion items and the bounce stage.
__device__ inline RcRay cosine_ray(const float3_ p, const float3_ nn, float bias, const uint32_t rnd[4], float t_max) {
    const float3_ d = cosine_hemisphere_dir(nn, u32_to_unit(rnd[0]), u32_to_unit(rnd[1]));
    const float3_ o = add3(p, scale3(nn, bias));
    return RcRay{o.x, o.y, o.z, 0.f, d.x, d.y, d.z, t_max};
}
// Work item j = i * samples + s (AoParams, rc_internal.h), so the samples of a hit sit in neighbouring lanes and share its records.  A
// missed primary ray gives the dead ray; t_max = max_dist > 0 for every other item (checked by the caller), so there is no further gate: a
// hit with a NaN frame traces its NaN ray, as rc_trace_any_device does with the stored one.
struct AoItems {
    AoParams q;
    static constexpr bool kGate = false;
    __device__ inline uint32_t slot(uint32_t j) const { return j / q.samples; }  // (n * samples < 2^32)
    __device__ inline RcRay ray(const SceneView& v, uint32_t j, uint32_t i, const RcRay& r, const RcHit& h) const {
        float3_ p, nn;
        hit_frame(v, r, h, p, nn);
        uint32_t rnd[4];
        path_philox(q.path_base, q.path_in, i, j - i * q.samples, 0x414F0000u | q.depth, q.key, rnd);
        return cosine_ray(p, nn, q.bias, rnd, q.max_dist);
    }
};
// (VisibilityCountSink with count[j / samples] = slot i: one relaxed agent-scope u32 add per visible sample)
struct AoJob {
    AoParams q;
    uint32_t* count;
    __device__ inline HitItemSource<AoItems> source(const SceneView& v) const { return {v, {q}}; }  // (v: the kernel's own by-value parameter)
    __device__ inline VisibilityCountSink sink(const SceneView&) const { return VisibilityCountSink{count, q.samples}; }
};

// ---- final gather: the sum of a per-primitive field x over the closest hits of the same hemisphere samples ------------------------------
// AoItems' items and rays unchanged (item j = i * samples + s), traced for the CLOSEST hit.  Per finished item, i = j / samples:
//   a hit whose metadata m (hit_meta) lies in 1..n_prims:   sum[i] += x[m - 1]
//   a hit with metadata outside 1..n_prims:                 nothing (get_illumination's rule, src/kernels.jl:123)
//   no hit and t > 0 (VisibilityCountSink's rule: a live ray that reached max_dist):   sum[i] += miss_value, open[i] += 1 (open may be null)
//   a dead item (t = -1: the primary ray missed):           nothing
// u64 adds are exact in any order, so sum does not depend on scheduling, shell or shard.  x is read when the kernel runs, for counted
// samples only.  The samples of a slot sit in neighbouring lanes -- wave_add's good case: one atomic per slot and wave carrying the group's
// sum.  (Also built and measured: one plain u64 atomic per counted lane, within 2 % either way -- docs/EXPERIMENTS.md, "Final gather".)
struct GatherSink {
    const RcInstRec* inst;
    const RcPrim* prims;
    uint32_t n_prims;
    const uint32_t* x;
    uint32_t miss_value, samples;
    unsigned long long* sum;
    uint32_t* open;
    __device__ inline void operator()(uint64_t j, bool hit, float t, float, float, uint32_t prim, int instance) const {
        const uint32_t i = (uint32_t)j / samples;
        bool counted = false;
        uint32_t value = 0;
        if (hit) {
            const uint32_t m = hit_meta(inst, prims, instance, prim);
            counted = m >= 1 && m <= n_prims;
            if (counted) value = x[m - 1u];
        } else if (t > 0.0f) {
            counted = true;
            value = miss_value;
            if (open) __hip_atomic_fetch_add(open + i, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        wave_add(sum, i, value, counted);
    }
};
struct GatherJob {
    AoParams q;
    const uint32_t* x;
    uint32_t miss_value;
    unsigned long long* sum;
    uint32_t* open;
    __device__ inline HitItemSource<AoItems> source(const SceneView& v) const { return {v, {q}}; }  // (v: the kernel's own by-value parameter)
    __device__ inline GatherSink sink(const SceneView& v) const { return GatherSink{v.inst, v.prims, v.n_prims, x, miss_value, q.samples, sum, open}; }
};
// The placed final gather (rc_placed_final_gather_device): GatherSink with x indexed by PLACED primitive (the index space of "form factors
// between instances" below: q = base[instance] + l, base = rc_scene::d_placed_base).  No metadata in the rule: the traversal core reports
// prim = l + 1, so b = base[instance] + prim - 1 -- ONE load where GatherSink reads two -- and b < P always: every hit is counted.
//   a hit:               sum[i] += x[b]
//   no hit and t > 0:    sum[i] += miss_value, open[i] += 1 (open may be null)
//   a dead item:         nothing
struct PlacedGatherSink {
    const uint32_t* base;
    const uint32_t* x;  // P words, indexed by q
    uint32_t miss_value, samples;
    unsigned long long* sum;
    uint32_t* open;
    __device__ inline void operator()(uint64_t j, bool hit, float t, float, float, uint32_t prim, int instance) const {
        const uint32_t i = (uint32_t)j / samples;
        bool counted = false;
        uint32_t value = 0;
        if (hit) {
            counted = true;
            value = x[base[instance] + prim - 1u];
        } else if (t > 0.0f) {
            counted = true;
            value = miss_value;
            if (open) __hip_atomic_fetch_add(open + i, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        wave_add(sum, i, value, counted);
    }
};
struct PlacedGatherJob {
    AoParams q;
    const uint32_t* base;
    const uint32_t* x;
    uint32_t miss_value;
    unsigned long long* sum;
    uint32_t* open;
    __device__ inline HitItemSource<AoItems> source(const SceneView& v) const { return {v, {q}}; }  // (v: the kernel's own by-value parameter)
    __device__ inline PlacedGatherSink sink(const SceneView&) const { return PlacedGatherSink{base, x, miss_value, q.samples, sum, open}; }
};

// ---- illumination from point sources: get_illumination (src/kernels.jl:112-124) for lamps at a finite position ---------------------------
// A source is one RcRay record in device memory: o = the lamp's position, d = its axis, t_min / t_max copied unchanged into every ray it
// emits (t_max: the lamp's range).  d.x == 0 && d.y == 0 && d.z == 0 (either sign of zero): ISOTROPIC; anything else: LAMBERTIAN about
// normalize3(d).  Source k (0-based in the call) shoots grid^2 jittered, stratified, equal-area rays, cell = a * grid + b, a, b in [0, grid):
//   rnd = Philox4x32-10(counter = (cell, first_source + k, 0, 0x50530000), key = (lo32 seed, hi32 seed))
//   xi1 = u32_to_unit(rnd[0]), xi2 = u32_to_unit(rnd[1])
//   u1 = ((float)a + xi1) / (float)grid, u2 = ((float)b + xi2) / (float)grid      (f32, one operation at a time, IEEE divide; u may
//                                                                                   round to exactly 1: both mappings are defined there)
//   isotropic:  z = 1 - 2 * u1;  s = sqrtf(fmaxf(0, 1 - z * z));  phi = (2 * 3.1415927f) * u2;  (sin, cos) = sincos_f64((double)phi), each
//               rounded once to f32;  dir = (s * cos, s * sin, z), not renormalised
//   Lambertian: dir = cosine_hemisphere_dir(normalize3(d), u1, u2)
//   ray = {o, t_min, dir, t_max}
// every expression left to right, no contraction.  first_source only offsets the Philox counter: the sources of one set, split over
// calls, groups, streams or devices, give the rows of the one-call result.  A source with non-finite fields gives whatever these
// expressions give for it, in the stage and in the driver alike.  Shared by the stage kernel and the fused driver's source, so the two
// agree bit for bit.
__device__ inline RcRay point_source_ray(const RcRay* sources, uint32_t first_source, uint32_t k, uint32_t cell, uint32_t grid, RcPhiloxKey key) {
    const RcRay src = load_ray(sources, k);
    const uint32_t a = cell / grid, b = cell - a * grid;
    uint32_t rnd[4];
    philox4x32_10(cell, first_source + k, 0u, 0x50530000u, key.k0, key.k1, rnd);
    const float u1 = ((float)a + u32_to_unit(rnd[0])) / (float)grid, u2 = ((float)b + u32_to_unit(rnd[1])) / (float)grid;
    float3_ d;
    if (src.dx == 0.0f && src.dy == 0.0f && src.dz == 0.0f) {
        const float z = 1.0f - 2.0f * u1;
        const float sn = __builtin_sqrtf(fmaxf(0.0f, 1.0f - z * z));
        const float phi = (2.0f * 3.1415927f) * u2;
        double sp, cp;
        sincos_f64((double)phi, sp, cp);
        d = mk3(sn * (float)cp, sn * (float)sp, z);
    } else
        d = cosine_hemisphere_dir(normalize3(mk3(src.dx, src.dy, src.dz)), u1, u2);
    return RcRay{src.ox, src.oy, src.oz, src.tmin, d.x, d.y, d.z, src.tmax};
}
// The composed stage: n_sources * grid^2 rays, source k's from k * grid^2 on, in cell order.  One kernel, no scratch.
__global__ void k_point_source_rays(const RcRay* sources, uint32_t first_source, uint32_t grid, uint32_t k0, uint32_t k1, uint64_t total, RcRay* out) {
    const uint64_t cells = (uint64_t)grid * grid;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t k = i / cells;
        store_ray(out, i, point_source_ray(sources, first_source, (uint32_t)k, (uint32_t)(i - k * cells), grid, RcPhiloxKey{k0, k1}));
    }
}
// The fused driver for a GROUP of sources in one launch: work item i = k_local * grid^2 + cell (items = G * grid^2 < 2^32: both divide in
// 32 bits).  The source record is read HERE, when the kernel runs: a captured launch follows lamps that move between replays, and there
// is no parameter kernel in front.
struct PointSource {
    const RcRay* sources;  // the group's first source
    uint32_t first_source, cells, grid;
    RcPhiloxKey key;
    __device__ inline RcRay operator()(uint64_t i) const {
        const uint32_t k = (uint32_t)i / cells, cell = (uint32_t)i - k * cells;
        return point_source_ray(sources, first_source, k, cell, grid, key);
    }
    static constexpr bool kPrefetch = false;  // rays are generated, nothing to read ahead
};
// DirsHistogramSink (row = the source of the group) that also counts the rays that hit nothing.  A source's escapes are ONE counter, and
// about half of a lamp's rays escape: counted straight into d_escaped[k] with one wave-aggregated atomic per wave and source (the way the
// totals driver counts `emitted`, whose targets change from wave to wave) the whole call ran at the rate of that word -- 3.4 to 3.7 times
// the composed path's time at 16 and 64 sources (docs/EXPERIMENTS.md, "Illumination from point sources").  So the escapes are histogram
// entries like the hits: the copies are laid out for n_prims + kEscapeSlots indices, an escaping ray counts on index n_prims + (a slot chosen
// per WAVE, so that a wave's lanes still combine), in its workgroup's copy, and k_hist_fold (FoldAddU32RowsEscaped) adds a source's 16 x 64 words
// into d_escaped[k].  A finished ray is a counted hit, an escape or neither: one wave_count for both kinds.
constexpr uint32_t kEscapeSlots = 64;
struct PointEscapeSink {
    const RcInstRec* inst;
    const RcPrim* prims;
    uint32_t n_prims;
    uint32_t* scratch;  // one histogram of n_prims + kEscapeSlots indices per source of the group, zeroed by the launcher
    CopyHist h;
    uint32_t cells;
    __device__ inline void operator()(uint64_t i, bool hit, float, float, float, uint32_t prim, int instance) const {
        uint32_t j = n_prims + ((((blockIdx.x >> 4) * (blockDim.x >> 6)) + (threadIdx.x >> 6)) & (kEscapeSlots - 1u));
        bool counted = !hit;
        if (hit) {
            const uint32_t meta = hit_meta(inst, prims, instance, prim);
            counted = meta >= 1 && meta <= n_prims;  // metadata outside 1..N is dropped (src/kernels.jl:123)
            j = meta - 1u;
        }
        const unsigned long long copy = (unsigned long long)((uint32_t)i / cells) * kHistCopies + h.copy();
        wave_count(scratch, counted ? h.base(copy) + h.slot(j) : 0ull, counted);
    }
};
// The fold of the job that counts escapes, over n_prims + kEscapeSlots indices per source: the escape slots' sums go to escaped[k].
struct FoldAddU32RowsEscaped : FoldAddU32Rows {
    uint32_t n_prims;
    uint32_t* escaped;
    __device__ inline void add(uint32_t d, uint32_t j, uint32_t sum) const {
        if (j < n_prims) FoldAddU32Rows::add(d, j, sum);
        else atomicAdd(escaped + d, sum);
    }
};
// ESCAPED = false (d_escaped is NULL): the sink IS DirsHistogramSink, not a branch per ray.
template <bool ESCAPED>
struct PointIlluminationJobT {
    const RcRay* sources;
    uint32_t first_source, cells, grid;
    RcPhiloxKey key;
    uint32_t* scratch;
    CopyHist h;  // ESCAPED: of n_prims + kEscapeSlots indices
    __device__ inline PointSource source(const SceneView&) const { return PointSource{sources, first_source, cells, grid, key}; }
    template <bool E = ESCAPED>
    __device__ inline typename std::enable_if<E, PointEscapeSink>::type sink(const SceneView& v) const { return PointEscapeSink{v.inst, v.prims, v.n_prims, scratch, h, cells}; }
    template <bool E = ESCAPED>
    __device__ inline typename std::enable_if<!E, DirsHistogramSink>::type sink(const SceneView& v) const { return DirsHistogramSink{v.inst, v.prims, v.n_prims, scratch, h, cells}; }
};
// Keeps the late pop in the partial shell of the job that counts escapes: with the peeked stack top it has an 8-byte private segment (80
// VGPRs either way).  The five other shells of the two jobs have none with the default flags.
template <>
struct JobShapeFlags<PointIlluminationJobT<true>> { static constexpr unsigned kPlain = 0u, kLds = 0u, kPartial = ShapeLatePop; };
typedef PointIlluminationJobT<true> PointIlluminationJob;
typedef PointIlluminationJobT<false> PointIlluminationCountsJob;

// ---- form factors between surface groups: the view-factor job with a choice of sampling (view_factor_ray<COSINE>), counted per GROUP of primitives ----
// The counting rule, N = the flat primitive count, G = n_groups: a = the source's metadata, b = the hit's (hit_meta), ga = groups[a - 1],
// gb = groups[b - 1], wa = weights ? weights[a - 1] : 1.  A source whose a is outside 1..N or whose ga >= G contributes nothing.  A miss:
// escaped[ga] += wa, if escaped is given.  A hit with b in 1..N, b != a (the reference's hit_idx != tri_idx, src/kernels.jl:96) and gb < G:
// matrix[ga * G + gb] += wa.  Any other hit adds nothing.  u64 adds modulo 2^64: exact in any order, so any partition of sources x rays
// gives the same words.  groups and weights are read for metadata in 1..N only.
// With a handful of groups every wave of the launch adds onto a few dozen words -- the case CopyHist exists for: when the launcher hands
// out scratch (h.n8 != 0), a ray counts on index ga * G + gb, or G * G + ga for an escape, of its workgroup's private copy -- one wave_add
// for both kinds, a finished ray is one or the other -- and k_hist_fold (FoldAddU64Groups) adds the copies into the caller's arrays.
// Without scratch the same sums go straight onto `matrix` and `escaped`.  Indices stay below 2^32: G <= 65535, G * G + G <= 65535 * 65536.
struct ViewFactorGroupsSink {
    const SceneView& v;
    VfShard sh;
    uint32_t n_groups;
    const uint32_t* groups;
    const uint32_t* weights;      // or nullptr: every source weighs 1
    unsigned long long* matrix;   // h.n8 != 0: the launch's copy histogram (zeroed by the launcher); else the caller's G x G words
    unsigned long long* escaped;  // h.n8 != 0: non-null when escapes are counted (into the copies); else the caller's G words or nullptr
    CopyHist h;                   // of G * G (+ G) indices, or {0}: no copies
    __device__ inline void operator()(uint64_t w, bool hit, float, float, float, uint32_t prim, int instance) const {
        const VfPair p = vf_pair(v, nullptr, sh, w, hit, prim, instance);
        const uint32_t a = p.src_meta;
        bool counted = false, escape = false;
        uint32_t j = 0, wa = 0;
        if (a >= 1 && a <= v.n_prims) {
            const uint32_t ga = groups[a - 1u];
            if (ga < n_groups) {
                if (p.counted) {
                    const uint32_t gb = groups[p.to_meta - 1u];
                    if (gb < n_groups) { counted = true; j = ga * n_groups + gb; }
                } else if (!hit && escaped) { counted = true; escape = true; j = ga; }
                if (counted) wa = weights ? weights[a - 1u] : 1u;
            }
        }
        if (h.n8) {  // (uniform over the launch: every finishing lane reaches the same wave_add)
            if (escape) j += n_groups * n_groups;
            wave_add(matrix + h.base(h.copy()), counted ? h.slot(j) : 0u, wa, counted);
        } else {
            wave_add(matrix, j, wa, counted && !escape);
            if (escaped) wave_add(escaped, j, wa, escape);
        }
    }
};
// The fold of the groups job's copies: index j < n_matrix = G * G is a matrix word, the G behind them are the escapes.
struct FoldAddU64Groups : FoldOneRow {
    unsigned long long* matrix;
    unsigned long long* escaped;
    uint32_t n_matrix;
    __device__ inline void add(uint32_t, uint32_t j, unsigned long long sum) const { atomicAdd(j < n_matrix ? matrix + j : escaped + (j - n_matrix), sum); }
};
template <bool COSINE>
struct ViewFactorGroupsJob {
    VfShard sh;
    uint32_t n_groups;
    const uint32_t* groups;
    const uint32_t* weights;
    unsigned long long* matrix;
    unsigned long long* escaped;
    CopyHist h;
    __device__ inline ViewFactorSource<COSINE> source(const SceneView& v) const { return ViewFactorSource<COSINE>{v.prims, nullptr, sh}; }
    __device__ inline ViewFactorGroupsSink sink(const SceneView& v) const { return ViewFactorGroupsSink{v, sh, n_groups, groups, weights, matrix, escaped, h}; }
};

// ---- form factors between instances: the groups job with its sources placed in world space, counted per PLACED primitive ------------------
// A placed primitive is a pair (instance i, local primitive l): i = the 0-based position in the instance array (RcHit::instance_id), l = the
// 0-based position inside the instance's BLAS in its sorted order -- the flat index is inst[i].prims_offset + l, the traversal core reports
// prim = l + 1.  Its index is q = base[i] + l, base = the exclusive prefix sum of RcInstRec::n_prims over the instance array (n_inst + 1
// words, rc_scene::d_placed_base, built by rc_build_tlas: structure changes only there); P = base[n_inst].
// q -> i: the upper bound in base.  Every BLAS has a primitive, so base is strictly increasing and the i with base[i] <= q < base[i + 1] is
// unique.  The search never reads past base[n_inst - 1] and answers an instance below n_inst whatever q is (the launchers hand out q < P).
__device__ __forceinline__ uint32_t placed_instance(const uint32_t* base, uint32_t n_inst, uint32_t q) {
    uint32_t lo = 0, hi = n_inst - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (base[mid + 1u] <= q) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}
// The scene arrays a placed source reads, all as they are WHEN THE KERNEL RUNS: behind k_update_instances on the same stream `instances`
// holds the new forward transforms.
struct PlacedView {
    const RcInstanceDesc* instances;  // 108-byte records, 4-byte aligned: the 12 transform words are dword loads
    const RcInstRec* inst;
    const RcPrim* prims;
    const uint32_t* base;
    uint32_t n_inst;
};
// The world triangle of placed primitive q: p_k = transform_point(T_i, v_k) with T_i the instance's FORWARD transform, in xf_point's
// operation order ((m0 * x + m1 * y) + m2 * z) + m3 per row, no contraction.  `flat` and `i` are what the Philox counter needs.
__device__ inline RcPrim placed_triangle(const PlacedView& pv, uint32_t q, uint32_t& flat, uint32_t& i) {
    i = placed_instance(pv.base, pv.n_inst, q);
    flat = pv.inst[i].prims_offset + (q - pv.base[i]);
    const float* m = pv.instances[i].transform;
    const RcPrim local = pv.prims[flat];
    RcPrim tri;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float3_ p = xf_point(m, mk3(local.v[3 * k], local.v[3 * k + 1], local.v[3 * k + 2]));
        tri.v[3 * k] = p.x; tri.v[3 * k + 1] = p.y; tri.v[3 * k + 2] = p.z;
    }
    tri.meta = local.meta;
    return tri;
}
// The placed ray of (q, ray index): view_factor_ray<COSINE> on the world triangle -- the normal is that of the transformed vertices in
// their order, so a mirroring instance flips it and a non-uniform scale bends it correctly; the origin is pt + normal * 0.01f in WORLD
// units -- with the Philox counter (ray_idx, flat primitive index, i, 0): word 2 is the only difference from the per-triangle family, so
// instance 0 under an identity transform draws the sibling's numbers.  Shared by the stage kernel and the fused driver's source.
template <bool COSINE>
__device__ inline RcRay placed_view_factor_ray(const PlacedView& pv, uint32_t q, uint32_t ray_idx, RcPhiloxKey key) {
    uint32_t flat, i;
    const RcPrim tri = placed_triangle(pv, q, flat, i);
    return view_factor_ray<COSINE>(tri, flat, ray_idx, key, i);
}
// The two composed stages: the world triangles of placed primitives [placed_begin, placed_begin + n), 9 f32 each; and the rays
// [ray_begin, ray_begin + n_ray) of one placed primitive.
__global__ void k_placed_triangles(PlacedView pv, uint32_t placed_begin, uint32_t n, float* out) {
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < n; t += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t flat, i;
        const RcPrim tri = placed_triangle(pv, placed_begin + (uint32_t)t, flat, i);
#pragma unroll
        for (int k = 0; k < 9; ++k) out[9u * t + k] = tri.v[k];
    }
}
template <bool COSINE>
__global__ void k_placed_view_factor_rays(PlacedView pv, RcPhiloxKey key, uint32_t q, uint32_t ray_begin, uint32_t n_ray, RcRay* out) {
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < n_ray; t += (uint64_t)gridDim.x * blockDim.x)
        store_ray(out, t, placed_view_factor_ray<COSINE>(pv, q, ray_begin + (uint32_t)t, key));
}
// The fused driver's source: work item w = placed primitive sh.src_begin + w / n_ray, ray sh.ray_begin + w % n_ray.  With n_ray >= 64 a wave
// holds one or two sources: the search and the transform loads are near-uniform and cache-resident, once per ray against hundreds of node
// visits.  With n_ray = 1 a wave's 64 lanes hold 64 sources of possibly several instances; every lane searches for itself.
template <bool COSINE>
struct PlacedViewFactorSource {
    PlacedView pv;
    VfShard sh;
    __device__ inline RcRay operator()(uint64_t w) const {
        return placed_view_factor_ray<COSINE>(pv, sh.src_begin + (uint32_t)(w / sh.n_ray), sh.ray_begin + (uint32_t)(w % sh.n_ray), sh.key);
    }
    static constexpr bool kPrefetch = false;
};
// The counting rule, P = the placed-primitive count, G = n_groups, no metadata in it: a = the source's q, for a hit b = base[hit instance] +
// prim - 1, ga = groups[a], gb = groups[b], wa = weights ? weights[a] : 1.  A source with ga >= G contributes nothing.  A miss:
// escaped[ga] += wa, if escaped is given.  A hit with b != a and gb < G: matrix[ga * G + gb] += wa.  Any other hit adds nothing.  u64 adds
// modulo 2^64, exact in any order.  a comes from w alone and b needs ONE load (base[instance]) where the metadata sink reads two `meta`
// words; the counting itself is ViewFactorGroupsSink's: one wave_add into the copies, or two onto the caller's words, folded by FoldAddU64Groups.
struct PlacedGroupsSink {
    const uint32_t* base;
    VfShard sh;
    uint32_t n_groups;
    const uint32_t* groups;       // P words, indexed by q
    const uint32_t* weights;      // P words or nullptr: every source weighs 1
    unsigned long long* matrix;   // as ViewFactorGroupsSink's
    unsigned long long* escaped;
    CopyHist h;
    __device__ inline void operator()(uint64_t w, bool hit, float, float, float, uint32_t prim, int instance) const {
        const uint32_t a = sh.src_begin + (uint32_t)(w / sh.n_ray);
        const uint32_t ga = groups[a];
        bool counted = false, escape = false;
        uint32_t j = 0, wa = 0;
        if (ga < n_groups) {
            if (hit) {
                const uint32_t b = base[instance] + prim - 1u;
                if (b != a) {
                    const uint32_t gb = groups[b];
                    if (gb < n_groups) { counted = true; j = ga * n_groups + gb; }
                }
            } else if (escaped) { counted = true; escape = true; j = ga; }
            if (counted) wa = weights ? weights[a] : 1u;
        }
        if (h.n8) {  // (uniform over the launch: every finishing lane reaches the same wave_add)
            if (escape) j += n_groups * n_groups;
            wave_add(matrix + h.base(h.copy()), counted ? h.slot(j) : 0u, wa, counted);
        } else {
            wave_add(matrix, j, wa, counted && !escape);
            if (escaped) wave_add(escaped, j, wa, escape);
        }
    }
};
template <bool COSINE>
struct PlacedViewFactorGroupsJob {
    const RcInstanceDesc* instances;
    const uint32_t* base;
    VfShard sh;
    uint32_t n_groups;
    const uint32_t* groups;
    const uint32_t* weights;
    unsigned long long* matrix;
    unsigned long long* escaped;
    CopyHist h;
    __device__ inline PlacedViewFactorSource<COSINE> source(const SceneView& v) const {
        return PlacedViewFactorSource<COSINE>{PlacedView{instances, v.inst, v.prims, base, v.n_inst}, sh};
    }
    __device__ inline PlacedGroupsSink sink(const SceneView&) const { return PlacedGroupsSink{base, sh, n_groups, groups, weights, matrix, escaped, h}; }
};
// Radiosity between instances: the P x P matrix of counts between PLACED primitives applied to a vector without the matrix
// (rc_placed_view_factor_products_device).  The rule, no metadata in it: a = the source's q; for a hit b = base[hit instance] + prim - 1.  A
// hit with b != a adds x[b] to mx[a] = (M x)[a] and x[a] to mtx[b] = (M^T x)[b]; a miss adds 1 to escaped[a]; a hit on the source itself
// adds nothing.  x == nullptr is x = 1: mx and mtx are then the placed `emitted` and `received`, so the totals need no job of their own.
// u64 adds modulo 2^64, exact in any order.  x is read for counted rays only.  mtx is the hot vector: it goes through the copy histogram
// like ViewFactorProductsSink's while the copies fit (h.n8 != 0, uniform over the launch), and straight onto the caller's words above that
// (h = {0}).  mx and escaped are per source, nearly wave-uniform in their target: wave_add / wave_count onto the caller's words.  Called
// under phased_trace's `if (fin)` like its siblings: every finishing lane reaches the same three calls, and both helpers read only lanes
// they have just balloted.
struct PlacedProductsSink {
    const uint32_t* base;
    VfShard sh;
    const uint32_t* x;            // P words, indexed by q, or nullptr: every x is 1
    unsigned long long* mtx;      // one histogram of scratch words (h.n8 != 0), the caller's P words (h.n8 == 0), or nullptr
    CopyHist h;
    unsigned long long* mx;       // [P] or nullptr
    unsigned long long* escaped;  // [P] or nullptr
    __device__ inline void operator()(uint64_t w, bool hit, float, float, float, uint32_t prim, int instance) const {
        const uint32_t a = sh.src_begin + (uint32_t)(w / sh.n_ray);
        uint32_t b = a;
        if (hit) b = base[instance] + prim - 1u;
        const bool counted = b != a;
        // (h = {0}: base() is 0 and the index is b itself -- one wave_add for both layouts)
        if (mtx) wave_add(mtx + h.base(h.copy()), h.n8 ? h.slot(b) : b, counted ? (x ? x[a] : 1u) : 0u, counted);
        if (mx) wave_add(mx, a, counted ? (x ? x[b] : 1u) : 0u, counted);
        if (escaped) wave_count(escaped, (unsigned long long)a, !hit);
    }
};
template <bool COSINE>
struct PlacedViewFactorProductsJob {
    const RcInstanceDesc* instances;
    const uint32_t* base;
    VfShard sh;
    const uint32_t* x;
    unsigned long long* mtx;
    CopyHist h;
    unsigned long long* mx;
    unsigned long long* escaped;
    __device__ inline PlacedViewFactorSource<COSINE> source(const SceneView& v) const {
        return PlacedViewFactorSource<COSINE>{PlacedView{instances, v.inst, v.prims, base, v.n_inst}, sh};
    }
    __device__ inline PlacedProductsSink sink(const SceneView&) const { return PlacedProductsSink{base, sh, x, mtx, h, mx, escaped}; }
};
// As for ViewFactorTotalsJob: the uniform job's plain shell has 36 bytes of private segment with the integer form of the stack position.
template <>
struct JobShapeFlags<PlacedViewFactorProductsJob<false>> { static constexpr unsigned kPlain = ShapePtrStack, kLds = 0u, kPartial = 0u; };
// The sparse matrix between placed primitives (rc_placed_view_factors_sparse_device): ViewFactorPairsJob with the placed source and the
// counting rule of PlacedProductsSink.  A chunk is whole consecutive rows, one source per row: sh.src_begin IS the chunk's first row, so
// item w belongs to chunk row w / n_ray.  One plain u64 store per finished ray at pairs[w], w below the launch's item count, no atomics:
// (chunk row << col_bits) | b for a hit with b = base[instance] + prim - 1 != a, `sentinel` for a miss or a hit on the source itself.
struct PlacedPairsSink {
    const uint32_t* base;
    uint32_t src_begin, n_ray, col_bits;
    unsigned long long sentinel;
    unsigned long long* pairs;
    __device__ inline void operator()(uint64_t w, bool hit, float, float, float, uint32_t prim, int instance) const {
        const uint32_t row = (uint32_t)(w / n_ray), a = src_begin + row;
        unsigned long long key = sentinel;
        if (hit) {
            const uint32_t b = base[instance] + prim - 1u;
            if (b != a) key = ((unsigned long long)row << col_bits) | b;
        }
        pairs[w] = key;
    }
};
template <bool COSINE>
struct PlacedViewFactorPairsJob {
    const RcInstanceDesc* instances;
    const uint32_t* base;
    VfShard sh;  // (whole rows: ray_begin = 0)
    uint32_t col_bits;
    unsigned long long sentinel;
    unsigned long long* pairs;
    __device__ inline PlacedViewFactorSource<COSINE> source(const SceneView& v) const {
        return PlacedViewFactorSource<COSINE>{PlacedView{instances, v.inst, v.prims, base, v.n_inst}, sh};
    }
    __device__ inline PlacedPairsSink sink(const SceneView&) const { return PlacedPairsSink{base, sh.src_begin, sh.n_ray, col_bits, sentinel, pairs}; }
};

// Diffuse bounce: output slot i continues the path of source slot s (s = i, or d_src[i] for i < count, or d_src[i % count] round robin
// with k = i / count), from hit_point + normal * bias in a cosine-weighted direction about the geometric normal.  The uniforms are
// Philox4x32-10(counter = (lo32 path, hi32 path, k, 0x424E0000 | bounce), key = seed): a path's bounce does not depend on compaction,
// chunking or sharding.  Dead slots (no source, or a miss) get o = 0, d = (0,0,1), [t_min, t_max] = [0, -1], which misses everything.
__global__ void k_bounce_rays(SceneView v, const RcRay* rays, const RcHit* hits, const uint32_t* src, const uint32_t* src_count, int wrap,
                              const uint32_t* path_in, uint32_t* path_out, uint64_t path_base, uint32_t n, uint32_t k0, uint32_t k1,
                              uint32_t tag, float bias, RcRay* out) {
    const uint32_t c = src ? *src_count : 0u;
    for (uint64_t i64 = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i64 < n; i64 += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t i = (uint32_t)i64;
        bool live = true;
        uint32_t s = i, k = 0;
        if (src) {
            if (c == 0u || (!wrap && i >= c)) live = false;
            else if (wrap) { s = src[i % c]; k = i / c; }
            else s = src[i];
        }
        RcRay b = RC_DEAD_RAY;
        uint32_t path_id = 0xFFFFFFFFu;  // RC_INVALID_ID
        if (live) {
            const RcHit h = hits[s];
            if (h.hit) {
                float3_ p, nn;
                hit_frame(v, rays[s], h, p, nn);
                uint32_t rnd[4];
                path_id = (uint32_t)path_philox(path_base, path_in, s, k, tag, RcPhiloxKey{k0, k1}, rnd);
                b = cosine_ray(p, nn, bias, rnd, INFINITY);
            }
        }
        store_ray(out, i, b);
        if (path_out) path_out[i] = path_id;
    }
}

// generate_primary_rays_lookat! (docs/src/wavefront-renderer.jl:219-254): ray (pixel_idx-1)*samples + s for pixel (x, y)
// (1-based, row-major pixel_idx = (y-1)*width + x); jitter = rand(Vec2f) there, Philox4x32-10(seed; ray index) here, or the
// pixel centre when jitter is off.  u, v as written: 2*(x - 0.5 + j1)/width - 1 and 1 - 2*(y - 0.5 + j2)/height.
struct CameraParams {
    float pos[3], right[3], up[3], forward[3];
    float half_width, half_height;
    uint32_t width, height, samples, jitter;
    RcPhiloxKey key;
};
__global__ void k_primary_rays(CameraParams c, uint64_t n, RcRay* out) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t pixel = i / c.samples;
        const uint32_t x = (uint32_t)(pixel % c.width) + 1u, y = (uint32_t)(pixel / c.width) + 1u;
        float j1 = 0.5f, j2 = 0.5f;
        if (c.jitter) {
            uint32_t rnd[4];
            philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), 0u, 0x50524159u, c.key.k0, c.key.k1, rnd);
            j1 = u32_to_unit(rnd[0]); j2 = u32_to_unit(rnd[1]);
        }
        const float u = 2.0f * ((float)x - 0.5f + j1) / (float)c.width - 1.0f;
        const float v = 1.0f - 2.0f * ((float)y - 0.5f + j2) / (float)c.height;
        const float su = u * c.half_width, sv = v * c.half_height;
        const float3_ d = normalize3(add3(add3(mk3(c.forward[0], c.forward[1], c.forward[2]), scale3(mk3(c.right[0], c.right[1], c.right[2]), su)),
                                          scale3(mk3(c.up[0], c.up[1], c.up[2]), sv)));
        float4* q = reinterpret_cast<float4*>(out + i);
        q[0] = make_float4(c.pos[0], c.pos[1], c.pos[2], 0.0f);
        q[1] = make_float4(d.x, d.y, d.z, INFINITY);  // Ray(o=..., d=...): t_min 0, t_max Inf (src/ray.jl:1-7)
    }
}

__global__ void k_hit_flags(const RcHit* hits, uint64_t n, uint32_t* flags) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i < n) flags[i] = hits[i].hit ? 1u : 0u;
}
__global__ void k_scatter_hit_indices(const uint32_t* flags, const uint32_t* pos, uint64_t n, uint32_t* indices, uint32_t* count) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (flags[i]) indices[pos[i]] = (uint32_t)i;
    if (i == n - 1) *count = pos[i] + flags[i];
}

}  // namespace

// A wavefront stage: a grid-stride kernel over n items in 256-thread workgroups, at most kPerCu per CU.  kReadsScene: the kernel reads scene
// memory, so the scene remembers the stream's launch (rc_note_stage_launch, below).
template <uint32_t kPerCu = 8, bool kReadsScene = true, class Kernel, class... Args>
static void launch_stage(rc_scene* s, hipStream_t stream, uint64_t n, Kernel kernel, Args... args) {
    if (n == 0) return;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + 255) / 256, (uint64_t)s->n_cus * kPerCu);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, stream, args...);
    RC_HIP(hipGetLastError());
    if (kReadsScene) rc_note_stage_launch(s, stream);
}

void rc_launch_ray_grid(rc_scene* s, const float viewdir[3], uint32_t grid, RcRay* d_rays, hipStream_t stream) {
    rc_ensure_world_bound(s, stream);  // the grid is laid out from the world bound: after an asynchronous refit it is read back first
    launch_stage<8, false>(s, stream, (uint64_t)grid * grid, k_ray_grid, grid_params(s->root_min, s->root_max, viewdir, grid), d_rays);
}

// n_dirs x grid^2 rays from device-resident directions and the TLAS root as it is when the kernel runs: no host copy of the bound is read.
void rc_launch_ray_grid_dirs(rc_scene* s, const float* d_dirs, uint32_t n_dirs, uint32_t grid, RcRay* d_rays, hipStream_t stream) {
    const uint64_t n = (uint64_t)grid * grid;
    if (n == 0 || n_dirs == 0) return;
    const uint32_t per_dir = (uint32_t)std::min<uint64_t>((n + kBlock - 1) / kBlock, std::max<uint64_t>(((uint64_t)s->n_cus * 8 + n_dirs - 1) / n_dirs, 1));
    hipLaunchKernelGGL(k_ray_grid_dirs, dim3(per_dir, std::min<uint32_t>(n_dirs, 65535u)), dim3(kBlock), 0, stream, s->tlas_nodes.p, s->n_tlas_nodes, d_dirs, n_dirs, grid, d_rays);
    RC_HIP(hipGetLastError());
    rc_note_stage_launch(s, stream);
}

static rc_scene* range_checked(rc_scene* s) {
    if ((uint64_t)(s->n_flat_nodes + s->n_tlas_nodes) * 64u >= (1ull << 32))
        throw RcError(1, "driver kernels address nodes with 32-bit buffer offsets: scenes above 64 M nodes are not supported yet");
    return s;
}

// Scratch counters of the launch's totals kernel: launches on one stream are ordered and share an area; another stream gets its own (up to
// kMaxTotalsScratch: rc_stream_slot); a CAPTURED launch owns its area like its spill region.
static unsigned long long* rc_totals_scratch(RcLaunchGuard& g, size_t words) {
    if (words == 0) words = 1;
    if (g.capture >= 0) {
        auto& owned = g.s->capture_slots[g.capture].scratch;
        owned.emplace_back(new DevBuf<unsigned long long>());
        owned.back()->reserve(words);
        return owned.back()->p;
    }
    bool fresh = false;
    rc_scene::TotalsScratch& area = rc_stream_slot<rc_scene::kMaxTotalsScratch>(g.s->totals_scratch, g.stream, &fresh);
    if (fresh) area.buf.reset(new DevBuf<unsigned long long>());
    area.buf->reserve(words);
    g.uses(area.last);
    return area.buf->p;
}

namespace {
// The launch's scratch: `rows` copy histograms of Word counters, zeroed on the launch's stream, and room for n_params GridParams behind them.
template <class Word>
struct HistScratch {
    Word* hist;
    GridParams* params;
};
template <class Word>
HistScratch<Word> rc_hist_scratch(RcLaunchGuard& g, CopyHist h, uint32_t rows = 1, uint32_t n_params = 0) {
    const size_t hist_bytes = sizeof(Word) * (size_t)(rows * h.words());
    unsigned char* p = reinterpret_cast<unsigned char*>(rc_totals_scratch(g, (hist_bytes + sizeof(GridParams) * n_params + 7u) / 8u));
    RC_HIP(hipMemsetAsync(p, 0, hist_bytes, g.stream));
    return HistScratch<Word>{reinterpret_cast<Word*>(p), reinterpret_cast<GridParams*>(p + hist_bytes)};
}
template <class Word, class Rule>
void rc_hist_fold(hipStream_t stream, const Word* hist, CopyHist h, uint32_t n, Rule rule) {
    const uint64_t items = (uint64_t)rule.rows() * n;
    if (items) hipLaunchKernelGGL((k_hist_fold<Word, Rule>), dim3((uint32_t)((items + 255u) / 256u)), dim3(256), 0, stream, hist, h, n, rule);
}
struct Nothing { void operator()() const {} };

// What every driver launch on the persistent phased core shares.  Construction checks the node count (before the launch guard takes anything),
// takes the guard, picks the shape the scene gets (plain 256 threads, top level in LDS, partial tops in LDS) and its grid, and fills the view and
// the persistent arguments.  The caller reserves its scratch and enqueues what must run first; go<ANY>(job, between, behind) starts the guard,
// runs `between`, launches the job's shell of that shape (run() adds the shape's own arguments), runs `behind` (the fold) and finishes the guard.
struct DriverLaunch {
    RcLaunchGuard guard;
    rc_scene* s;
    hipStream_t stream;
    bool partial, lds;
    uint32_t blocks;
    SceneView v;
    PersistArgs p;
    DriverLaunch(rc_scene* scene, hipStream_t st, uint64_t n_items)
        : guard(range_checked(scene), st), s(scene), stream(st), partial(rc_partial_driver_ok(scene)), lds(partial || rc_lds_driver_ok(scene)),
          blocks(lds ? rc_grid_blocks(scene, n_items, kMidBlock, LdsShape<>::kBlocksPerCu) : rc_grid_blocks(scene, n_items, kBlock, PlainShape<>::kBlocksPerCu)) {
        const uint32_t threads = blocks * (lds ? (uint32_t)kMidBlock : (uint32_t)kBlock);
        v = rc_scene_view(guard, threads);
        p = rc_persist_args(guard, n_items, threads);
    }
    template <bool ANY, class Job>
    void run(const Job& job) {
        if (ANY && s->opt.entry_cull < 2) v.entry_cull = 0u;  // any_hit: the rule of rc_launch_trace
        if (partial) {
            rc_partial_driver_args(s, p);
            rc_ensure_dynamic_lds(s, reinterpret_cast<const void*>(&k_driver_partial<ANY, Job>), PartialShape<>::kLdsBytes);
            hipLaunchKernelGGL((k_driver_partial<ANY, Job>), dim3(blocks), dim3(kMidBlock), PartialShape<>::kLdsBytes, stream, v, p, job);
        } else if (lds) {
            rc_lds_driver_args(s, p);
            rc_ensure_dynamic_lds(s, reinterpret_cast<const void*>(&k_driver_lds<ANY, Job>), LdsShape<>::kLdsBytes);
            hipLaunchKernelGGL((k_driver_lds<ANY, Job>), dim3(blocks), dim3(kMidBlock), LdsShape<>::kLdsBytes, stream, v, p, job);
        } else
            hipLaunchKernelGGL((k_driver<ANY, Job>), dim3(blocks), dim3(kBlock), 0, stream, v, p, job);
    }
    template <bool ANY, class Job, class Between = Nothing, class Behind = Nothing>
    void go(const Job& job, Between between = Between(), Behind behind = Behind()) {
        guard.start();
        between();
        run<ANY>(job);
        behind();
        guard.finish();
    }
};
// The row-grouped illumination calls trace their n_rows rows (directions, point sources) of `cells` rays in groups of G consecutive ones,
// one persistent launch per group; G is the largest count with G * cells < 2^32 (the sources divide in 32 bits) whose private histogram
// copies (h: of one row) fit option "illum_scratch_bytes" (at least one row's worth).  each(first, count) per group.
template <class Each>
void for_row_groups(rc_scene* s, uint32_t n_rows, uint64_t cells, CopyHist h, Each each) {
    const uint64_t row_bytes = sizeof(uint32_t) * h.words();
    const uint64_t group = std::min<uint64_t>(n_rows, std::min<uint64_t>(((1ull << 32) - 1u) / cells, std::max<uint64_t>((uint64_t)s->opt.illum_scratch_bytes / row_bytes, 1)));
    for (uint32_t r0 = 0; r0 < n_rows; r0 += (uint32_t)group) each(r0, (uint32_t)std::min<uint64_t>(group, n_rows - r0));
}
// The shard of a view-factor call: the rays [ray_begin, ray_end) below rays_per_triangle of the source positions [src_begin, src_end) below
// n_sources (the flat primitive count; the placed family's P).  Returns its item count, 0 for an empty shard.
uint64_t vf_shard(uint32_t n_sources, uint32_t rays_per_triangle, uint64_t seed, uint32_t src_begin, uint32_t src_end, uint32_t ray_begin, uint32_t ray_end, VfShard& sh) {
    src_end = std::min(src_end, n_sources);
    ray_end = std::min(ray_end, rays_per_triangle);
    if (src_begin >= src_end || ray_begin >= ray_end) return 0;
    sh = VfShard{rc_philox_key(seed), src_begin, ray_begin, ray_end - ray_begin};
    return (uint64_t)(src_end - src_begin) * sh.n_ray;
}
uint64_t vf_shard(const rc_scene* s, uint32_t rays_per_triangle, uint64_t seed, uint32_t src_begin, uint32_t src_end, uint32_t ray_begin, uint32_t ray_end, VfShard& sh) {
    return vf_shard(s->n_flat_prims, rays_per_triangle, seed, src_begin, src_end, ray_begin, ray_end, sh);
}
}  // namespace

void rc_launch_illumination(rc_scene* s, const float viewdir[3], uint32_t grid, uint64_t ray_begin, uint64_t ray_end,
                            float* d_counts, hipStream_t stream) {
    if (ray_end <= ray_begin) return;
    rc_ensure_world_bound(s, stream);
    GridParams g = grid_params(s->root_min, s->root_max, viewdir, grid);
    DriverLaunch launch(s, stream, ray_end - ray_begin);
    const uint32_t np = s->n_flat_prims;
    const CopyHist h = CopyHist::of(np);
    uint32_t* scratch = rc_hist_scratch<uint32_t>(launch.guard, h).hist;
    launch.go<false>(
        IlluminationJob{g, ray_begin, scratch, h},
        [&] {  // a repeated get_illumination (same grid: item i is the same cell every time) claims the chunks that held long rays last time first
            if (launch.guard.capturing || ray_begin != 0) return;
            // (the rays are generated: the batch is described by its view direction and grid size -- another direction is another batch)
            const float diag = sqrtf((s->root_max[0] - s->root_min[0]) * (s->root_max[0] - s->root_min[0]) + (s->root_max[1] - s->root_min[1]) * (s->root_max[1] - s->root_min[1]) +
                                     (s->root_max[2] - s->root_min[2]) * (s->root_max[2] - s->root_min[2]));
            const float stand_in[8] = {(float)grid * diag, 0.f, 0.f, 0.f, g.dir[0], g.dir[1], g.dir[2], 0.f};
            rc_cost_order_setup(launch.guard, ray_end, 2, launch.p.claim, nullptr, stand_in);
        },
        [&] { rc_hist_fold(stream, scratch, h, np, FoldF32Saturating{{}, d_counts}); });
}

// get_illumination for n_dirs device-resident directions, ACCUMULATED into d_counts[d * row_stride + (meta - 1)] (u32).  The directions are
// traced in groups (for_row_groups), one persistent launch per group (IlluminationDirsJob).  Per group: the copies are zeroed,
// k_grid_params lays the group's grids out from d_dirs and the TLAS root AS THEY
// ARE WHEN IT RUNS -- nothing here reads the host copy of the world bound, so the call follows an asynchronous refit or rebuild without a
// host wait and may be captured --, the launch counts, the fold adds.  Items are claimed in natural order: the plan is fixed at call time,
// the rays are not known before the kernels run.  grid^2 < 2^32 (checked by the caller).
void rc_launch_illumination_dirs(rc_scene* s, const float* d_dirs, uint32_t n_dirs, uint32_t grid, uint32_t* d_counts, uint64_t row_stride, hipStream_t stream) {
    const uint32_t np = s->n_flat_prims;
    const CopyHist h = CopyHist::of(np);
    const uint64_t cells = (uint64_t)grid * grid;
    if (n_dirs == 0 || cells == 0 || np == 0) return;
    for_row_groups(s, n_dirs, cells, h, [&](uint32_t d0, uint32_t nd) {
        DriverLaunch launch(s, stream, nd * cells);
        const HistScratch<uint32_t> scratch = rc_hist_scratch<uint32_t>(launch.guard, h, nd, nd);  // the group's grids sit behind its histograms
        hipLaunchKernelGGL(k_grid_params, dim3((nd + 63u) / 64u), dim3(64), 0, stream, s->tlas_nodes.p, s->n_tlas_nodes, d_dirs + 3u * (size_t)d0, nd, grid, scratch.params);
        launch.go<false>(IlluminationDirsJob{scratch.params, (uint32_t)cells, scratch.hist, h}, Nothing(),
                         [&] { rc_hist_fold(stream, scratch.hist, h, np, FoldAddU32Rows{nd, d_counts + (uint64_t)d0 * row_stride, row_stride}); });
    });
}

// n_sources x grid^2 rays of device-resident point sources (k_point_source_rays): reads no scene memory.
void rc_launch_point_source_rays(rc_scene* s, const RcRay* d_sources, uint32_t n_sources, uint32_t grid, uint64_t seed, uint32_t first_source,
                                 RcRay* d_rays, hipStream_t stream) {
    const uint64_t total = (uint64_t)n_sources * grid * grid;
    const RcPhiloxKey key = rc_philox_key(seed);
    launch_stage<8, false>(s, stream, total, k_point_source_rays, d_sources, first_source, grid, key.k0, key.k1, total, d_rays);
}

// get_illumination for n_sources device-resident POINT sources, ACCUMULATED into d_counts[k * row_stride + (meta - 1)] (u32) and, unless
// it is null, the rays that hit nothing into d_escaped[k].  The sources are traced in groups of G consecutive ones like the directions of
// rc_launch_illumination_dirs (for_row_groups).  Per group: one memset, one persistent launch (PointIlluminationJob), one fold; the
// group's first index is added to
// first_source for the Philox counter, so the grouping changes no result.  Nothing is read on the host and there is no kernel in front:
// the source records are read by the traversal kernel itself.  grid^2 < 2^32 and first_source + n_sources <= 2^32 (checked by the caller).
template <bool ESCAPED>
static void launch_illumination_points(rc_scene* s, const RcRay* d_sources, uint32_t n_sources, uint32_t grid, uint64_t seed, uint32_t first_source,
                                       uint32_t* d_counts, uint64_t row_stride, uint32_t* d_escaped, hipStream_t stream) {
    const uint32_t np = s->n_flat_prims;
    const CopyHist h = CopyHist::of(ESCAPED ? np + kEscapeSlots : np);  // (the escapes are kEscapeSlots more indices of every copy: PointEscapeSink)
    const uint64_t cells = (uint64_t)grid * grid;
    for_row_groups(s, n_sources, cells, h, [&](uint32_t k0, uint32_t nk) {
        DriverLaunch launch(s, stream, nk * cells);
        uint32_t* scratch = rc_hist_scratch<uint32_t>(launch.guard, h, nk).hist;
        const FoldAddU32Rows rows{nk, d_counts + (uint64_t)k0 * row_stride, row_stride};
        launch.go<false>(PointIlluminationJobT<ESCAPED>{d_sources + k0, first_source + k0, (uint32_t)cells, grid, rc_philox_key(seed), scratch, h}, Nothing(), [&] {
            if (ESCAPED) rc_hist_fold(stream, scratch, h, np + kEscapeSlots, FoldAddU32RowsEscaped{rows, np, d_escaped + k0});
            else rc_hist_fold(stream, scratch, h, np, rows);
        });
    });
}
void rc_launch_illumination_points(rc_scene* s, const RcRay* d_sources, uint32_t n_sources, uint32_t grid, uint64_t seed, uint32_t first_source,
                                   uint32_t* d_counts, uint64_t row_stride, uint32_t* d_escaped, hipStream_t stream) {
    if (n_sources == 0 || grid == 0 || s->n_flat_prims == 0) return;
    if (d_escaped) launch_illumination_points<true>(s, d_sources, n_sources, grid, seed, first_source, d_counts, row_stride, d_escaped, stream);
    else launch_illumination_points<false>(s, d_sources, n_sources, grid, seed, first_source, d_counts, row_stride, nullptr, stream);
}

// RC_VF_SOURCES_BY_METADATA: the flat primitives' indices sorted by (metadata, index) -- and the sorted metadata themselves on the host --
// cached until the next rebuild or geometry update.  Built on the scene's own stream, which also owns the sort scratch, behind every EAGER
// asynchronous update (host wait, as the host-buffer queries do).  A graph that captured a geometry update re-sorts the
// primitives on every replay, at times the library does not see -- the order is rebuilt on every use, like the root boxes
// (rc_ensure_blas_bounds); the caller has waited for the replay (raycore_mi355x.h).  for_stream: the stream the order is wanted for; while it
// is being captured nothing can be sorted, read back or waited for.
// The sort lands in scratch and is COPIED into vf_order: a launch of an earlier call that still reads the order on another stream sees
// the same words before, during and after the copy unless the primitives moved -- and then its caller had to wait for it first anyway.
void rc_ensure_vf_order(rc_scene* s, hipStream_t for_stream) {
    std::lock_guard<std::mutex> g(s->launch_mu);
    if (s->state.vf_order_current()) return;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (for_stream && hipStreamIsCapturing(for_stream, &cap) == hipSuccess && cap == hipStreamCaptureStatusActive)
        throw RcError(6, s->state.deform_captured()
                             ? "stale view-factor source order: a graph that captured rc_update_geometry_device_async may have re-sorted the primitives, and the order cannot be rebuilt while the stream is being captured -- release the graph (\"release_captures\") or address the sources by primitive"
                             : "stale view-factor source order: it cannot be built while the stream is being captured -- call rc_view_factors_device with RC_VF_SOURCES_BY_METADATA once before the capture");
    (void)hipGetLastError();
    rc_wait_async_mutations(s);  // (an eager geometry update on a caller's stream may still be writing the primitives sorted here)
    const uint32_t np = s->n_flat_prims;
    s->vf_meta_sorted.assign(np, 0u);
    if (np) {
        s->keys_a.reserve(np); s->keys_b.reserve(np); s->vals_a.reserve(np); s->vals_b.reserve(np); s->vf_order.reserve(np);
        hipLaunchKernelGGL(k_meta_keys, dim3((np + 255) / 256), dim3(256), 0, s->stream, s->flat_prims.p, np, s->keys_a.p, s->vals_a.p);
        size_t tmp = 0;
        RC_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, s->keys_a.p, s->keys_b.p, s->vals_a.p, s->vals_b.p, (int)np, 0, 32, s->stream));
        s->sort_tmp.reserve(tmp ? tmp : 1);
        RC_HIP(hipcub::DeviceRadixSort::SortPairs(s->sort_tmp.p, tmp, s->keys_a.p, s->keys_b.p, s->vals_a.p, s->vals_b.p, (int)np, 0, 32, s->stream));  // stable: ties keep the flat order
        RC_HIP(hipMemcpyAsync(s->vf_order.p, s->vals_b.p, sizeof(uint32_t) * np, hipMemcpyDeviceToDevice, s->stream));
        RC_HIP(hipMemcpyAsync(s->vf_meta_sorted.data(), s->keys_b.p, sizeof(uint32_t) * np, hipMemcpyDeviceToHost, s->stream));
        RC_HIP(hipStreamSynchronize(s->stream));  // the launches that read the order run on other streams
    }
    s->state.vf_order_built();
}
void rc_vf_source_range(rc_scene* s, uint32_t row_begin, uint32_t row_end, uint32_t& pos_begin, uint32_t& pos_end) {
    const auto& m = s->vf_meta_sorted;  // row r <=> metadata r + 1
    pos_begin = (uint32_t)(std::lower_bound(m.begin(), m.end(), row_begin + 1u) - m.begin());
    pos_end = (uint32_t)(std::lower_bound(m.begin(), m.end(), row_end + 1u) - m.begin());
}

void rc_launch_view_factors(rc_scene* s, uint32_t rays_per_triangle, uint64_t seed, uint32_t src_begin, uint32_t src_end,
                            uint32_t ray_begin, uint32_t ray_end, uint32_t* d_matrix, uint64_t row_stride, uint64_t col_stride,
                            uint32_t row_offset, uint32_t flags, hipStream_t stream) {
    VfShard sh;
    const uint64_t total = vf_shard(s, rays_per_triangle, seed, src_begin, src_end, ray_begin, ray_end, sh);
    if (!total) return;
    const uint32_t* order = (flags & 2u) ? s->vf_order.p : nullptr;  // RC_VF_SOURCES_BY_METADATA: the caller has called rc_ensure_vf_order, once per job
    DriverLaunch(s, stream, total).go<false>(ViewFactorJob{sh, d_matrix, row_stride, col_stride, row_offset, flags, order});
}

// Totals of rays [ray_begin, ray_end) of the sources with flat indices [src_begin, src_end), ACCUMULATED into d_received / d_emitted
// (n_prims u64 each, device; either may be nullptr).
void rc_launch_vf_totals(rc_scene* s, uint32_t rays_per_triangle, uint64_t seed, uint32_t src_begin, uint32_t src_end, uint32_t ray_begin,
                         uint32_t ray_end, unsigned long long* d_received, unsigned long long* d_emitted, hipStream_t stream) {
    VfShard sh;
    const uint64_t total = vf_shard(s, rays_per_triangle, seed, src_begin, src_end, ray_begin, ray_end, sh);
    if (!total || (!d_received && !d_emitted)) return;
    DriverLaunch launch(s, stream, total);
    const uint32_t np = s->n_flat_prims;
    const CopyHist h = CopyHist::of(np);
    // the private copies of the hot vector (see ViewFactorTotalsSink): one scratch area per stream, launches on one stream are ordered
    unsigned long long* scratch = d_received ? rc_hist_scratch<unsigned long long>(launch.guard, h).hist : nullptr;
    launch.go<false>(ViewFactorTotalsJob{sh, scratch, h, d_emitted}, Nothing(),
                     [&] { if (d_received) rc_hist_fold(stream, scratch, h, np, FoldAddU64{{}, d_received}); });
}

// The products (M x, M^T x) of the same shard with the device vector d_x (n_prims u32), ACCUMULATED into d_mx / d_mtx (n_prims u64 each, device;
// either may be nullptr).  The launch of rc_launch_vf_totals with ViewFactorProductsJob: d_mtx takes `received`'s copy histogram and fold.
void rc_launch_vf_products(rc_scene* s, uint32_t rays_per_triangle, uint64_t seed, uint32_t src_begin, uint32_t src_end, uint32_t ray_begin,
                           uint32_t ray_end, const uint32_t* d_x, unsigned long long* d_mx, unsigned long long* d_mtx, hipStream_t stream) {
    VfShard sh;
    const uint64_t total = vf_shard(s, rays_per_triangle, seed, src_begin, src_end, ray_begin, ray_end, sh);
    if (!total || (!d_mx && !d_mtx)) return;
    DriverLaunch launch(s, stream, total);
    const uint32_t np = s->n_flat_prims;
    const CopyHist h = CopyHist::of(np);
    unsigned long long* scratch = d_mtx ? rc_hist_scratch<unsigned long long>(launch.guard, h).hist : nullptr;
    launch.go<false>(ViewFactorProductsJob{sh, d_x, scratch, h, d_mx}, Nothing(),
                     [&] { if (d_mtx) rc_hist_fold(stream, scratch, h, np, FoldAddU64{{}, d_mtx}); });
}

// The G x G matrix of weighted counts between groups of primitives (rc_view_factor_groups_device): the shard of rc_launch_vf_totals with
// ViewFactorGroupsJob, ACCUMULATED into d_matrix (G * G u64, row = source group) and d_escaped (G u64, may be nullptr).  The kernel counts
// into kHistCopies private copies of the G * G (+ G) words when they fit kVfGroupsCopyBytes and k_hist_fold adds them; otherwise it adds
// straight onto the caller's words.  The bound is 256 MiB (G <= 1447 with escapes): the copies cost about 0.45 ms per GiB to zero and fold,
// and stop paying at about 32 MiB for a 5.5 M-ray job and at about 2 GiB for a 205 M-ray one (docs/EXPERIMENTS.md, "Form factors between
// surface groups").  Both paths give the same words.  d_groups, d_weights and the scene are read when the kernel runs.  1 <= G <= 65535
// (checked by the caller): wave_add indexes in 32 bits.
constexpr unsigned long long kVfGroupsCopyBytes = 256ull << 20;
// make(matrix, h): the job that counts into `matrix` under the copy layout h ({0}: the caller's own words).
template <class MakeJob>
static void launch_vf_groups(rc_scene* s, uint64_t total, uint32_t n_groups, unsigned long long* d_matrix, unsigned long long* d_escaped, hipStream_t stream, MakeJob make) {
    DriverLaunch launch(s, stream, total);
    const uint32_t gg = n_groups * n_groups, n = gg + (d_escaped ? n_groups : 0u);
    CopyHist h = CopyHist::of(n);
    const bool copies = sizeof(unsigned long long) * h.words() <= kVfGroupsCopyBytes;
    unsigned long long* scratch = copies ? rc_hist_scratch<unsigned long long>(launch.guard, h).hist : nullptr;
    if (!copies) h = CopyHist{0u};
    launch.go<false>(make(copies ? scratch : d_matrix, h), Nothing(), [&] { if (copies) rc_hist_fold(stream, scratch, h, n, FoldAddU64Groups{{}, d_matrix, d_escaped, gg}); });
}
void rc_launch_vf_groups(rc_scene* s, uint32_t rays_per_triangle, uint64_t seed, uint32_t sampling, uint32_t src_begin, uint32_t src_end,
                         uint32_t ray_begin, uint32_t ray_end, const uint32_t* d_groups, uint32_t n_groups, const uint32_t* d_weights,
                         unsigned long long* d_matrix, unsigned long long* d_escaped, hipStream_t stream) {
    VfShard sh;
    const uint64_t total = vf_shard(s, rays_per_triangle, seed, src_begin, src_end, ray_begin, ray_end, sh);
    if (!total) return;
    if (sampling) launch_vf_groups(s, total, n_groups, d_matrix, d_escaped, stream, [&](unsigned long long* m, CopyHist h) { return ViewFactorGroupsJob<true>{sh, n_groups, d_groups, d_weights, m, d_escaped, h}; });
    else launch_vf_groups(s, total, n_groups, d_matrix, d_escaped, stream, [&](unsigned long long* m, CopyHist h) { return ViewFactorGroupsJob<false>{sh, n_groups, d_groups, d_weights, m, d_escaped, h}; });
}

// Form factors between instances (rc_placed_*): the scene arrays of a placed source, the two composed stages, and rc_launch_vf_groups with
// PlacedViewFactorGroupsJob over placed primitives [placed_begin, placed_end) clamped to P -- the same copy bound, scratch and fold.
// The callers have checked P < 2^32 and the ranges of the stages.
static PlacedView placed_view(const rc_scene* s) {
    return PlacedView{s->d_instances.p, s->inst_recs.p, s->flat_prims.p, s->d_placed_base.p, s->n_static_instances};
}
void rc_launch_placed_triangles(rc_scene* s, uint32_t placed_begin, uint32_t n, float* d_verts, hipStream_t stream) {
    launch_stage(s, stream, n, k_placed_triangles, placed_view(s), placed_begin, n, d_verts);
}
void rc_launch_placed_view_factor_rays(rc_scene* s, uint64_t seed, uint32_t sampling, uint32_t placed_prim, uint32_t ray_begin, uint32_t n_ray, RcRay* d_out, hipStream_t stream) {
    launch_stage(s, stream, n_ray, sampling ? k_placed_view_factor_rays<true> : k_placed_view_factor_rays<false>, placed_view(s), rc_philox_key(seed), placed_prim,
                 ray_begin, n_ray, d_out);
}
void rc_launch_placed_vf_groups(rc_scene* s, uint32_t rays_per_triangle, uint64_t seed, uint32_t sampling, uint32_t placed_begin, uint32_t placed_end,
                                uint32_t ray_begin, uint32_t ray_end, const uint32_t* d_groups, uint32_t n_groups, const uint32_t* d_weights,
                                unsigned long long* d_matrix, unsigned long long* d_escaped, hipStream_t stream) {
    VfShard sh;
    const uint64_t total = vf_shard((uint32_t)s->n_placed, rays_per_triangle, seed, placed_begin, placed_end, ray_begin, ray_end, sh);
    if (!total) return;
    const RcInstanceDesc* instances = s->d_instances.p;
    const uint32_t* base = s->d_placed_base.p;
    if (sampling) launch_vf_groups(s, total, n_groups, d_matrix, d_escaped, stream, [&](unsigned long long* m, CopyHist h) { return PlacedViewFactorGroupsJob<true>{instances, base, sh, n_groups, d_groups, d_weights, m, d_escaped, h}; });
    else launch_vf_groups(s, total, n_groups, d_matrix, d_escaped, stream, [&](unsigned long long* m, CopyHist h) { return PlacedViewFactorGroupsJob<false>{instances, base, sh, n_groups, d_groups, d_weights, m, d_escaped, h}; });
}
// Radiosity between instances (rc_placed_view_factor_products_device): the products of the same shard with the device vector d_x (P u32,
// nullptr: x = 1), ACCUMULATED into d_mx / d_mtx / d_escaped (P u64 each, device; each may be nullptr).  d_mtx takes the copy histogram and
// FoldAddU64 of rc_launch_vf_products while 8 bytes x the copies' words fit option "placed_copy_bytes" -- P reaches 2 x 10^7 on the
// 4800-instance scene, where 16 copies are 2.5 GB --, and is added straight onto the caller's words above that, the way launch_vf_groups
// does.  Both paths give the same words.  Nothing is read on the host.
template <bool COSINE>
static void launch_placed_vf_products(rc_scene* s, const VfShard& sh, uint64_t total, const uint32_t* d_x, unsigned long long* d_mx, unsigned long long* d_mtx,
                                      unsigned long long* d_escaped, hipStream_t stream) {
    DriverLaunch launch(s, stream, total);
    const uint32_t P = (uint32_t)s->n_placed;
    CopyHist h = CopyHist::of(P);
    const bool copies = d_mtx && sizeof(unsigned long long) * h.words() <= (unsigned long long)s->opt.placed_copy_bytes;
    unsigned long long* scratch = copies ? rc_hist_scratch<unsigned long long>(launch.guard, h).hist : nullptr;
    if (!copies) h = CopyHist{0u};
    const PlacedView pv = placed_view(s);  // (the kernel's own SceneView supplies inst, prims and n_inst)
    launch.go<false>(PlacedViewFactorProductsJob<COSINE>{pv.instances, pv.base, sh, d_x, copies ? scratch : d_mtx, h, d_mx, d_escaped}, Nothing(),
                     [&] { if (copies) rc_hist_fold(stream, scratch, h, P, FoldAddU64{{}, d_mtx}); });
}
void rc_launch_placed_vf_products(rc_scene* s, uint32_t rays_per_triangle, uint64_t seed, uint32_t sampling, uint32_t placed_begin, uint32_t placed_end,
                                  uint32_t ray_begin, uint32_t ray_end, const uint32_t* d_x, unsigned long long* d_mx, unsigned long long* d_mtx,
                                  unsigned long long* d_escaped, hipStream_t stream) {
    VfShard sh;
    const uint64_t total = vf_shard((uint32_t)s->n_placed, rays_per_triangle, seed, placed_begin, placed_end, ray_begin, ray_end, sh);
    if (!total || (!d_mx && !d_mtx && !d_escaped)) return;
    (sampling ? launch_placed_vf_products<true> : launch_placed_vf_products<false>)(s, sh, total, d_x, d_mx, d_mtx, d_escaped, stream);
}

// Rows [row_begin, row_end) of the view-factor matrix in canonical CSR (rc_view_factors_sparse_device), all on `stream`, no host wait.
// The sources are addressed in metadata order (the caller has called rc_ensure_vf_order): a range of rows is a contiguous range of source
// positions, and metadata 0 or above N lie outside every range.  The job is cut HERE, on the host, into chunks of WHOLE rows whose rays x 8
// bytes fit option "vf_sparse_scratch_bytes" (a single row above it gets a chunk of its own).  Per chunk (vf_sparse_chain, shared with the
// placed family): the trace stores one key per ray (ViewFactorPairsJob); a radix sort over the bits that can vary -- ceil(log2 rows of
// the chunk) + ceil(log2 N) + the sentinel's --; a run-length encoding whose run count stays on the device; k_vf_sparse_append.  The
// chunks are whole rows in ascending order, so what they append is the sorted result.  d_row_ptr holds the rows' COUNTS until an exclusive scan behind the last chunk turns them into offsets.
// The running nnz alternates between *d_nnz and d_row_ptr[rows] (which no count uses), so that the append kernel reads one word and
// writes another; the last chunk writes *d_nnz.  Every word that crosses a chunk boundary lives in the caller's arrays: the scratch is
// the stream's (rc_totals_scratch), sized once for the largest chunk, and holds nothing between two launches.
namespace {
struct SparseChunk { uint32_t row0, row1, pos0, pos1; };  // matrix rows [row0, row1) = source positions [pos0, pos1)
uint32_t ceil_log2(uint64_t n) { uint32_t b = 0; while (b < 64u && (1ull << b) < n) ++b; return b; }
size_t round16(size_t b) { return (b + 15u) & ~(size_t)15u; }
// What follows the plan, the same for both families (rc_launch_vf_sparse, rc_launch_placed_vf_sparse): the limits of every chunk (before
// anything is enqueued), the zeroed counts, the scratch sized for the largest chunk, and per chunk trace -> sort -> run-length encoding ->
// append, with the scan behind the last one.  `chunks`: whole rows in ascending order, rows within [row_begin, row_begin + rows); n_cols:
// the matrix's column count.  trace(launch, sh, chunk, col_bits, sentinel, keys, behind) launches the family's pairs job over the chunk's
// items (sh: the chunk's source positions, all R rays) with `behind` as the launch's last step.
template <class Trace>
void vf_sparse_chain(rc_scene* s, const char* who, const std::vector<SparseChunk>& chunks, uint32_t R, uint64_t seed, uint64_t n_cols, uint32_t row_begin, uint32_t rows,
                     unsigned long long* d_row_ptr, uint32_t* d_cols, uint32_t* d_vals, uint64_t capacity, unsigned long long* d_nnz, hipStream_t stream, Trace trace) {
    const uint32_t col_bits = ceil_log2(n_cols);
    uint64_t most_items = 0;
    for (const SparseChunk& c : chunks) {
        const uint64_t items = (uint64_t)(c.pos1 - c.pos0) * R;
        if (items >> 32) throw RcError(1, std::string(who) + ": a chunk's sources x rays_per_triangle reaches 2^32");
        if (ceil_log2(c.row1 - c.row0) + col_bits + 1u > 64u) throw RcError(1, std::string(who) + ": a chunk's (row, column) keys need more than 64 bits");
        most_items = std::max(most_items, items);
    }
    RC_HIP(hipMemsetAsync(d_row_ptr, 0, sizeof(unsigned long long) * ((size_t)rows + 1u), stream));
    RC_HIP(hipMemsetAsync(d_nnz, 0, sizeof(unsigned long long), stream));
    if (chunks.empty()) return;
    // the scratch of one chunk, sized for the largest: keys, sorted keys (the unique keys then overwrite the unsorted ones), run lengths,
    // the run count, the scanned row pointers, and the primitives' own temporary storage
    size_t tmp_bytes = 1;
    for (const SparseChunk& c : chunks) {
        const uint64_t items = (uint64_t)(c.pos1 - c.pos0) * R;
        const int end_bit = (int)(ceil_log2(c.row1 - c.row0) + col_bits + 1u);
        size_t b = 0;
        RC_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, b, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, items, 0, end_bit, stream));
        tmp_bytes = std::max(tmp_bytes, b);
        b = 0;
        RC_HIP(::rocprim::run_length_encode(nullptr, b, (const unsigned long long*)nullptr, (unsigned int)items, (unsigned long long*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, stream));
        tmp_bytes = std::max(tmp_bytes, b);
    }
    {
        size_t b = 0;
        RC_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)(rows + 1u), stream));
        tmp_bytes = std::max(tmp_bytes, b);
    }
    const size_t key_bytes = round16(sizeof(unsigned long long) * most_items), len_bytes = round16(sizeof(uint32_t) * most_items),
                 ptr_bytes = round16(sizeof(unsigned long long) * ((size_t)rows + 1u));
    const size_t total_bytes = 2u * key_bytes + len_bytes + 16u + ptr_bytes + round16(tmp_bytes);
    unsigned long long* const running[2] = {d_nnz, d_row_ptr + rows};
    const size_t n_chunks = chunks.size();
    for (size_t ci = 0; ci < n_chunks; ++ci) {
        const SparseChunk& c = chunks[ci];
        const VfShard sh{rc_philox_key(seed), c.pos0, 0u, R};  // whole rows of a non-empty chunk
        const uint64_t items = (uint64_t)(c.pos1 - c.pos0) * R;
        const uint32_t row_bits = ceil_log2(c.row1 - c.row0);
        const unsigned long long sentinel = 1ull << (row_bits + col_bits);
        DriverLaunch launch(s, stream, items);
        unsigned char* base = reinterpret_cast<unsigned char*>(rc_totals_scratch(launch.guard, total_bytes / 8u));
        unsigned long long* keys = reinterpret_cast<unsigned long long*>(base);
        unsigned long long* sorted = reinterpret_cast<unsigned long long*>(base + key_bytes);
        uint32_t* lengths = reinterpret_cast<uint32_t*>(base + 2u * key_bytes);
        uint32_t* n_runs = reinterpret_cast<uint32_t*>(base + 2u * key_bytes + len_bytes);
        unsigned long long* scanned = reinterpret_cast<unsigned long long*>(base + 2u * key_bytes + len_bytes + 16u);
        void* tmp = base + 2u * key_bytes + len_bytes + 16u + ptr_bytes;
        trace(launch, sh, c, col_bits, sentinel, keys, [&] {
            size_t b = tmp_bytes;
            RC_HIP(hipcub::DeviceRadixSort::SortKeys(tmp, b, (const unsigned long long*)keys, sorted, items, 0, (int)(row_bits + col_bits + 1u), stream));
            b = tmp_bytes;
            RC_HIP(::rocprim::run_length_encode(tmp, b, (const unsigned long long*)sorted, (unsigned int)items, keys, lengths, n_runs, stream));
            const uint32_t blocks = (uint32_t)std::min<uint64_t>((items + 255u) / 256u, (uint64_t)std::max(s->n_cus, 1) * 8u);
            hipLaunchKernelGGL(k_vf_sparse_append, dim3(blocks), dim3(256), 0, stream, (const unsigned long long*)keys, (const uint32_t*)lengths,
                               (const uint32_t*)n_runs, sentinel, col_bits, c.row0 - row_begin, (const unsigned long long*)running[(n_chunks - ci) & 1u],
                               running[(n_chunks - ci - 1u) & 1u], d_cols, d_vals, (unsigned long long)capacity, d_row_ptr);
            RC_HIP(hipGetLastError());
            if (ci + 1u == n_chunks) {  // counts -> offsets
                b = tmp_bytes;
                RC_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, b, (const unsigned long long*)d_row_ptr, scanned, (int)(rows + 1u), stream));
                RC_HIP(hipMemcpyAsync(d_row_ptr, scanned, sizeof(unsigned long long) * ((size_t)rows + 1u), hipMemcpyDeviceToDevice, stream));
            }
        });
    }
}
}  // namespace
void rc_launch_vf_sparse(rc_scene* s, uint32_t rays_per_triangle, uint64_t seed, uint32_t row_begin, uint32_t row_end, unsigned long long* d_row_ptr,
                         uint32_t* d_cols, uint32_t* d_vals, uint64_t capacity, unsigned long long* d_nnz, hipStream_t stream) {
    const uint32_t np = s->n_flat_prims, R = rays_per_triangle;
    if (row_end > np) row_end = np;
    if (row_begin > row_end) row_begin = row_end;
    const uint32_t rows = row_end - row_begin;
    // the plan: chunks of whole rows
    std::vector<SparseChunk> chunks;
    const uint64_t max_items = std::max<uint64_t>((uint64_t)s->opt.vf_sparse_scratch_bytes / 8u, 1u);
    if (rows && R) {
        uint32_t p0 = 0, p1 = 0;
        rc_vf_source_range(s, row_begin, row_end, p0, p1);
        const std::vector<uint32_t>& m = s->vf_meta_sorted;
        for (uint32_t i = p0; i < p1;) {
            SparseChunk c{m[i] - 1u, 0u, i, i};
            while (i < p1) {
                uint32_t j = i;
                while (j < p1 && m[j] == m[i]) ++j;  // the sources of one row
                if (((uint64_t)(j - i) * R) >> 32) throw RcError(1, "rc_view_factors_sparse: one row's sources x rays_per_triangle reaches 2^32");
                if (i != c.pos0 && (uint64_t)(j - c.pos0) * R > max_items) break;
                c.row1 = m[i];
                i = j;
            }
            c.pos1 = i;
            chunks.push_back(c);
        }
    }
    const uint32_t* order = s->vf_order.p;
    vf_sparse_chain(s, "rc_view_factors_sparse", chunks, R, seed, np, row_begin, rows, d_row_ptr, d_cols, d_vals, capacity, d_nnz, stream,
                    [&](DriverLaunch& launch, const VfShard& sh, const SparseChunk& c, uint32_t col_bits, unsigned long long sentinel, unsigned long long* keys, auto behind) {
                        launch.go<false>(ViewFactorPairsJob{sh, c.row0, col_bits, sentinel, keys, order}, Nothing(), behind);
                    });
}

// Rows [placed_begin, placed_end) (clamped to P) of the matrix between PLACED primitives in canonical CSR
// (rc_placed_view_factors_sparse_device): Mp[a, b] = the rays of placed primitive a that hit placed primitive b != a first, the matrix that
// rc_launch_placed_vf_products applies.  Row a has exactly one source, placed primitive a, so the plan needs no metadata order: chunks of
// max(1, option "vf_sparse_scratch_bytes" / (8 R)) consecutive rows, a row is never split.  The trace is PlacedViewFactorPairsJob, everything
// behind it is vf_sparse_chain.  The transforms are read when the kernels run; nothing is read on the host.  The caller has checked P < 2^32.
void rc_launch_placed_vf_sparse(rc_scene* s, uint32_t rays_per_triangle, uint64_t seed, uint32_t sampling, uint32_t placed_begin, uint32_t placed_end,
                                unsigned long long* d_row_ptr, uint32_t* d_cols, uint32_t* d_vals, uint64_t capacity, unsigned long long* d_nnz, hipStream_t stream) {
    const uint32_t P = (uint32_t)s->n_placed, R = rays_per_triangle;
    if (placed_end > P) placed_end = P;
    if (placed_begin > placed_end) placed_begin = placed_end;
    const uint32_t rows = placed_end - placed_begin;
    std::vector<SparseChunk> chunks;
    if (rows && R) {
        const uint64_t max_items = std::max<uint64_t>((uint64_t)s->opt.vf_sparse_scratch_bytes / 8u, 1u);
        const uint32_t per_chunk = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(max_items / R, 1u), rows);
        for (uint32_t r0 = placed_begin; r0 < placed_end;) {
            const uint32_t r1 = r0 + std::min(per_chunk, placed_end - r0);
            chunks.push_back(SparseChunk{r0, r1, r0, r1});
            r0 = r1;
        }
    }
    const PlacedView pv = placed_view(s);  // (the kernel's own SceneView supplies inst, prims and n_inst)
    vf_sparse_chain(s, "rc_placed_view_factors_sparse_device", chunks, R, seed, P, placed_begin, rows, d_row_ptr, d_cols, d_vals, capacity, d_nnz, stream,
                    [&](DriverLaunch& launch, const VfShard& sh, const SparseChunk&, uint32_t col_bits, unsigned long long sentinel, unsigned long long* keys, auto behind) {
                        if (sampling) launch.go<false>(PlacedViewFactorPairsJob<true>{pv.instances, pv.base, sh, col_bits, sentinel, keys}, Nothing(), behind);
                        else launch.go<false>(PlacedViewFactorPairsJob<false>{pv.instances, pv.base, sh, col_bits, sentinel, keys}, Nothing(), behind);
                    });
}

// mx += M x, mtx += M^T x for rows [row_offset, row_offset + n_rows) of a CSR block (k_vf_sparse_products): nothing is read on the host, so
// the call may be captured and needs no wait behind the build.  Four rows per workgroup; at most 64 workgroups per CU, the rest by stride.
void rc_launch_vf_sparse_products(rc_scene* s, uint32_t n_rows, uint32_t row_offset, const unsigned long long* d_row_ptr, const uint32_t* d_cols,
                                  const uint32_t* d_vals, const uint32_t* d_x, unsigned long long* d_mx, unsigned long long* d_mtx, hipStream_t stream) {
    if (n_rows == 0 || (!d_mx && !d_mtx)) return;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)n_rows + 3u) / 4u, (uint64_t)std::max(s->n_cus, 1) * 64u);
    hipLaunchKernelGGL(k_vf_sparse_products, dim3(blocks), dim3(256), 0, stream, n_rows, row_offset, d_row_ptr, d_cols, d_vals, d_x, d_mx, d_mtx);
    RC_HIP(hipGetLastError());
}

// Kernels outside RcLaunchGuard that read scene memory on a caller's stream (the wavefront stages): remember the stream's latest such
// launch.  rc_scene_destroy waits for these events and for the launch slots' -- not for the whole device, which HIP refuses while any
// stream of the process is being captured.
void rc_note_stage_launch(rc_scene* s, hipStream_t stream) {
    if (stream == s->stream) return;  // the scene's own streams are synchronised at destruction
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (stream && hipStreamIsCapturing(stream, &st) == hipSuccess && st == hipStreamCaptureStatusActive) return;  // (a replay in flight is the caller's to wait for)
    std::lock_guard<std::mutex> lk(s->stage_mu);
    auto it = s->stage_events.find(stream);
    if (it == s->stage_events.end()) {
        if (s->stage_events.size() >= 64) {  // a caller that keeps making streams: retire one whose work is done
            for (auto jt = s->stage_events.begin(); jt != s->stage_events.end(); ++jt)
                if (hipEventQuery(jt->second) == hipSuccess) { (void)hipEventDestroy(jt->second); s->stage_events.erase(jt); break; }
            (void)hipGetLastError();
            if (s->stage_events.size() >= 64) { auto jt = s->stage_events.begin(); (void)hipEventSynchronize(jt->second); (void)hipEventDestroy(jt->second); s->stage_events.erase(jt); }
        }
        hipEvent_t ev = nullptr;
        RC_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        it = s->stage_events.emplace(stream, ev).first;
    }
    RC_HIP(hipEventRecord(it->second, stream));
}

// The rays [ray_begin, ray_begin + n_ray) of one source primitive (sampling 0 = the reference's uniform hemisphere, 1 = cosine)
void rc_launch_view_factor_rays(rc_scene* s, uint64_t seed, uint32_t sampling, uint32_t src, uint32_t ray_begin, uint32_t n_ray, RcRay* d_out, hipStream_t stream) {
    if (n_ray == 0) return;
    hipLaunchKernelGGL(sampling ? k_view_factor_rays<true> : k_view_factor_rays<false>, dim3((n_ray + 255) / 256), dim3(256), 0, stream, rc_scene_view_static(s),
                       rc_philox_key(seed), src, ray_begin, n_ray, d_out);
    RC_HIP(hipGetLastError());
    rc_note_stage_launch(s, stream);
}

void rc_launch_hit_points(rc_scene* s, const RcRay* d_rays, const RcHit* d_hits, uint64_t n, float* d_points, float* d_normals, hipStream_t stream) {
    launch_stage(s, stream, n, k_hit_points, rc_scene_view_static(s), d_rays, d_hits, n, d_points, d_normals);
}

// The hit-sample family (ShadowParams, SoftShadowParams, AoParams: rc_internal.h).  A composed stage writes one ray per item; a driver is
// one persistent launch over the same items in natural claim order -- the rays are generated, there is no batch to recognise.  Every item
// count is below 2^32 (checked by the caller).
void rc_launch_shadow_rays(rc_scene* s, const ShadowParams& q, const float light[3], uint64_t n, RcRay* d_out, hipStream_t stream) {
    launch_stage(s, stream, n, k_hit_item_rays<ShadowItems<true>>, rc_scene_view_static(s), ShadowItems<true>{q, {light[0], light[1], light[2]}}, n, d_out);
}
void rc_launch_shadow_visibility(rc_scene* s, const ShadowParams& q, uint64_t n, uint8_t* d_visible, hipStream_t stream) {
    if (n * q.n_lights) DriverLaunch(s, stream, n * q.n_lights).go<true>(ShadowJob{q, d_visible});
}
void rc_launch_soft_shadow_rays(rc_scene* s, const SoftShadowParams& q, uint64_t n, RcRay* d_out, hipStream_t stream) {
    const uint64_t total = n * q.n_lights * q.samples;
    launch_stage(s, stream, total, k_hit_item_rays<SoftShadowItems>, rc_scene_view_static(s), SoftShadowItems{q}, total, d_out);
}
// ACCUMULATES the visible samples into d_count[i * n_lights + l]
void rc_launch_soft_shadow_visibility(rc_scene* s, const SoftShadowParams& q, uint64_t n, uint32_t* d_count, hipStream_t stream) {
    const uint64_t total = n * q.n_lights * q.samples;
    if (total) DriverLaunch(s, stream, total).go<true>(SoftShadowJob{q, d_count});
}
void rc_launch_ao_rays(rc_scene* s, const AoParams& q, uint64_t n, RcRay* d_out, hipStream_t stream) {
    launch_stage(s, stream, n * q.samples, k_hit_item_rays<AoItems>, rc_scene_view_static(s), AoItems{q}, n * q.samples, d_out);
}
// ACCUMULATES the visible samples into d_count[i]
void rc_launch_ambient_occlusion(rc_scene* s, const AoParams& q, uint64_t n, uint32_t* d_count, hipStream_t stream) {
    if (n * q.samples) DriverLaunch(s, stream, n * q.samples).go<true>(AoJob{q, d_count});
}
// The final gather: the same items and rays in one persistent CLOSEST-hit launch that ACCUMULATES x at the hit primitives' metadata
// (miss_value for an escaped sample) into d_sum[i] and the escaped samples into d_open[i] (may be null).
void rc_launch_final_gather(rc_scene* s, const AoParams& q, uint64_t n, const uint32_t* d_x, uint32_t miss_value, uint64_t* d_sum, uint32_t* d_open, hipStream_t stream) {
    if (n * q.samples) DriverLaunch(s, stream, n * q.samples).go<false>(GatherJob{q, d_x, miss_value, reinterpret_cast<unsigned long long*>(d_sum), d_open});
}
// The placed final gather: the same launch with d_x indexed by placed primitive (PlacedGatherSink); and the placed index of hit records.
void rc_launch_placed_final_gather(rc_scene* s, const AoParams& q, uint64_t n, const uint32_t* d_x, uint32_t miss_value, uint64_t* d_sum, uint32_t* d_open, hipStream_t stream) {
    if (n * q.samples)
        DriverLaunch(s, stream, n * q.samples).go<false>(PlacedGatherJob{q, s->d_placed_base.p, d_x, miss_value, reinterpret_cast<unsigned long long*>(d_sum), d_open});
}
void rc_launch_placed_hit_indices(rc_scene* s, const RcHit* d_hits, uint64_t n, uint32_t* d_q, hipStream_t stream) {
    launch_stage(s, stream, n, k_placed_hit_indices, rc_scene_view_static(s), s->d_placed_base.p, d_hits, n, d_q);
}

void rc_launch_bounce_rays(rc_scene* s, const RcRay* d_rays, const RcHit* d_hits, const uint32_t* d_src, const uint32_t* d_src_count, int wrap,
                           const uint32_t* d_path_in, uint32_t* d_path_out, uint64_t path_base, uint64_t n, uint64_t seed, uint32_t bounce, float bias,
                           RcRay* d_out, hipStream_t stream) {
    const RcPhiloxKey key = rc_philox_key(seed);
    launch_stage(s, stream, n, k_bounce_rays, rc_scene_view_static(s), d_rays, d_hits, d_src, d_src_count, wrap ? 1 : 0, d_path_in, d_path_out, path_base,
                 (uint32_t)n, key.k0, key.k1, 0x424E0000u | bounce, bias, d_out);
}

void rc_launch_primary_rays(rc_scene* s, const float pos[3], const float right[3], const float up[3], const float forward[3], float half_width,
                            float half_height, uint32_t width, uint32_t height, uint32_t samples, uint64_t seed, int jitter, RcRay* d_out, hipStream_t stream) {
    const uint64_t n = (uint64_t)width * height * samples;
    if (n == 0) return;
    CameraParams c;
    for (int k = 0; k < 3; ++k) { c.pos[k] = pos[k]; c.right[k] = right[k]; c.up[k] = up[k]; c.forward[k] = forward[k]; }
    c.half_width = half_width; c.half_height = half_height;
    c.width = width; c.height = height; c.samples = samples; c.jitter = jitter ? 1u : 0u;
    c.key = rc_philox_key(seed);
    launch_stage<16, false>(s, stream, n, k_primary_rays, c, n, d_out);  // (reads no scene memory)
}

// Indices of the rays that hit, ascending, and their number: the compaction step between wavefront stages (the reference's
// demo renderer keeps dummy rays instead, docs/src/wavefront-renderer.jl:445, so every later stage runs over all slots).
void rc_launch_compact_hits(rc_scene* s, const RcHit* d_hits, uint64_t n, uint32_t* d_indices, uint32_t* d_count, hipStream_t stream) {
    if (n == 0) { RC_HIP(hipMemsetAsync(d_count, 0, 4, stream)); return; }
    if (n > 0x7FFFFFFFull) throw RcError(1, "rc_compact_hits: more than 2^31 - 1 rays");
    s->compact_flags.reserve(n);
    s->compact_pos.reserve(n);
    const uint32_t blocks = (uint32_t)((n + 255) / 256);
    hipLaunchKernelGGL(k_hit_flags, dim3(blocks), dim3(256), 0, stream, d_hits, n, s->compact_flags.p);
    size_t tmp = 0;
    RC_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, s->compact_flags.p, s->compact_pos.p, (int)n, stream));
    s->compact_tmp.reserve(tmp ? tmp : 1);
    RC_HIP(hipcub::DeviceScan::ExclusiveSum(s->compact_tmp.p, tmp, s->compact_flags.p, s->compact_pos.p, (int)n, stream));
    hipLaunchKernelGGL(k_scatter_hit_indices, dim3(blocks), dim3(256), 0, stream, s->compact_flags.p, s->compact_pos.p, n, d_indices, d_count);
    RC_HIP(hipGetLastError());
    rc_note_stage_launch(s, stream);
}
