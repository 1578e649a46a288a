// rc_build.hip -- device-side LBVH construction for BLAS and TLAS (gfx950).
//
// Replaces the KernelAbstractions build/refit kernels of src/instanced-bvh-kernels.jl and their drivers
// build_blas (src/instanced-bvh.jl:1376-1443), build_tlas_topology (:1485-1594), refit_tlas! (:2197-2222).
// The output node arrays are bit-identical to the reference algorithm's (tests compare them with the
// CPU oracle byte for byte): same Morton keys, same stable sort, same Karras topology, same min/max refit.
//
// Device design: one pass of small kernels on the scene's stream, no host round trip except the final
// 64-byte root read-back.  Scene bounds are reduced with order-preserving integer atomics (exact: min/max
// do not round), the sort is rocPRIM's stable LSD radix sort over the 30 key bits, topology is one thread
// per internal node, refit is the classic second-arrival walk with agent-scope acq_rel counters.
#include <hipcub/hipcub.hpp>
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "rc_traverse_core.h"

namespace {

constexpr int kBlock = 256;
inline unsigned grid_for(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// ---- order-preserving float <-> uint encoding for atomicMin/atomicMax ------------------------------
__host__ __device__ inline uint32_t enc_f32(float f) {
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float dec_f32(uint32_t e) {
    uint32_t u = (e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e;
    return __builtin_bit_cast(float, u);
}

// Scene bounds without atomics: a few thousand waves hitting the same six words with atomicMin/Max serialise in the L2 (measured:
// 270 us for ANY triangle count -- half of a 250 k-triangle build).  Stage 1 leaves one partial per block (wave shuffles, then LDS
// across the block's waves), stage 2 folds the partials in one small block.  Integer min/max on the order-preserving encoding:
// exact and independent of the reduction order.
__device__ inline void block_reduce_bounds(float3_ mn, float3_ mx, uint32_t* partials) {
    uint32_t e[6] = {enc_f32(mn.x), enc_f32(mn.y), enc_f32(mn.z), enc_f32(mx.x), enc_f32(mx.y), enc_f32(mx.z)};
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            uint32_t o = __shfl_xor(e[k], off);
            e[k] = o < e[k] ? o : e[k];
            uint32_t p = __shfl_xor(e[3 + k], off);
            e[3 + k] = p > e[3 + k] ? p : e[3 + k];
        }
    }
    __shared__ uint32_t sh[kBlock / 64][6];
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) sh[threadIdx.x >> 6][k] = e[k];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        uint32_t v = sh[0][k];
        for (int w = 1; w < kBlock / 64; ++w) v = k < 3 ? (sh[w][k] < v ? sh[w][k] : v) : (sh[w][k] > v ? sh[w][k] : v);
        partials[blockIdx.x * 6 + k] = v;
    }
}

// stage 2: wave k folds component k of all partials (launch with 6 waves)
__global__ void k_reduce_partials(const uint32_t* partials, uint32_t n_blocks, uint32_t* enc) {
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t v = k < 3 ? 0xFFFFFFFFu : 0u;
    for (uint32_t b = lane; b < n_blocks; b += 64) {
        const uint32_t x = partials[b * 6 + k];
        v = k < 3 ? (x < v ? x : v) : (x > v ? x : v);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = __shfl_xor(v, off);
        v = k < 3 ? (o < v ? o : v) : (o > v ? o : v);
    }
    if (lane == 0) enc[k] = v;
}

// world_bound(tri) (src/triangle_mesh.jl:37)
__device__ inline void tri_bounds(const RcPrim& p, float3_& mn, float3_& mx) {
    float3_ v0 = mk3(p.v[0], p.v[1], p.v[2]), v1 = mk3(p.v[3], p.v[4], p.v[5]), v2 = mk3(p.v[6], p.v[7], p.v[8]);
    mn = min3v(min3v(v0, v1), v2);
    mx = max3v(max3v(v0, v1), v2);
}

// is_degenerate_face (src/instanced-bvh.jl:573-577, src/triangle_mesh.jl:14-17): ((v3-v1) x (v2-v1)) . itself == 0
// exactly (isapprox against an exact 0 with the default tolerances).  flags[i] = 1 keeps face i.
__global__ void k_flag_valid_faces(const float* verts, uint32_t n, uint32_t* flags) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* p = verts + 9 * (size_t)i;
    float3_ a = mk3(p[0], p[1], p[2]), b = mk3(p[3], p[4], p[5]), c = mk3(p[6], p[7], p[8]);
    float3_ v = cross3(sub3(c, a), sub3(b, a));
    flags[i] = dot3(v, v) == 0.0f ? 0u : 1u;
}

// cpu_triangles of build_and_append_blas! (:593-600) as a stream compaction: face i goes to slot pos[i] (exclusive scan
// of the flags), order preserved; default metadata = face index BEFORE filtering (:595).
__global__ void k_compact_faces(const float* verts, const uint32_t* meta, const uint32_t* flags, const uint32_t* pos, uint32_t n, RcPrim* out, uint32_t* slot_face) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flags[i]) return;
    if (slot_face) slot_face[pos[i]] = i;
    RcPrim t;
    const float* p = verts + 9 * (size_t)i;
#pragma unroll
    for (int k = 0; k < 9; ++k) t.v[k] = p[k];
    t.meta = meta ? meta[i] : (i + 1);
    out[pos[i]] = t;
}

// mapreduce(world_bound, U, primitives) (src/instanced-bvh.jl:1386)
__global__ void k_blas_scene_bounds(const RcPrim* prims, uint32_t n, uint32_t* partials) {
    float3_ mn = mk3(INFINITY, INFINITY, INFINITY), mx = mk3(-INFINITY, -INFINITY, -INFINITY);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {  // grid-stride: few atomics
        float3_ a, b;
        tri_bounds(prims[i], a, b);
        mn = min3v(mn, a); mx = max3v(mx, b);
    }
    block_reduce_bounds(mn, mx, partials);
}

// expand_bits / morton_code_30bit (src/instanced-bvh.jl:1177-1200)
__device__ inline uint32_t expand_bits(uint32_t x) {
    x = (x * 0x00010001u) & 0xFF0000FFu;
    x = (x * 0x00000101u) & 0x0F00F00Fu;
    x = (x * 0x00000011u) & 0xC30C30C3u;
    x = (x * 0x00000005u) & 0x49249249u;
    return x;
}
__device__ inline uint32_t trunc_u32(float x) { return (x != x) ? 0u : (uint32_t)x; }  // unsafe_trunc; NaN -> 0
__device__ inline float clampf(float x, float lo, float hi) { return x > hi ? hi : (x < lo ? lo : x); }
__device__ inline uint32_t morton30(float3_ p) {
    const float unit_side = 1024.0f;
    float x = clampf(p.x * unit_side, 0.0f, unit_side - 1.0f);
    float y = clampf(p.y * unit_side, 0.0f, unit_side - 1.0f);
    float z = clampf(p.z * unit_side, 0.0f, unit_side - 1.0f);
    return (expand_bits(trunc_u32(x)) << 2) | (expand_bits(trunc_u32(y)) << 1) | expand_bits(trunc_u32(z));
}

// calculate_morton_codes_kernel! (src/instanced-bvh-kernels.jl:88-109); extent NOT clamped for a BLAS
__global__ void k_blas_morton(const RcPrim* prims, uint32_t n, const uint32_t* enc, uint32_t* keys, uint32_t* vals) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float3_ smin = mk3(dec_f32(enc[0]), dec_f32(enc[1]), dec_f32(enc[2]));
    float3_ smax = mk3(dec_f32(enc[3]), dec_f32(enc[4]), dec_f32(enc[5]));
    float3_ extent = sub3(smax, smin);
    float3_ mn, mx;
    tri_bounds(prims[i], mn, mx);
    float3_ c = scale3(add3(mn, mx), 0.5f);
    float3_ d = sub3(c, smin);
    keys[i] = morton30(mk3(d.x / extent.x, d.y / extent.y, d.z / extent.z));
    vals[i] = i;
}

__global__ void k_gather_prims(const RcPrim* in, const uint32_t* perm, uint32_t n, RcPrim* out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[perm[i]];
}

__global__ void k_gather_u32(const uint32_t* in, const uint32_t* perm, uint32_t n, uint32_t* out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[perm[i]];
}

// build_and_append_blas! after the mesh decomposition (src/instanced-bvh.jl:591-600): face i -> three vertices by index;
// metadata = face_meta[first vertex of the face] (per-vertex after expand_faceviews, :595) or the face index.
__global__ void k_expand_mesh(const float* verts, const uint32_t* indices, const uint32_t* vertex_meta, bool meta_per_face, uint32_t nf, float* soup, uint32_t* meta) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nf) return;
    const uint32_t i0 = indices[3 * (size_t)i], i1 = indices[3 * (size_t)i + 1], i2 = indices[3 * (size_t)i + 2];
    float* o = soup + 9 * (size_t)i;
    o[0] = verts[3 * (size_t)i0]; o[1] = verts[3 * (size_t)i0 + 1]; o[2] = verts[3 * (size_t)i0 + 2];
    o[3] = verts[3 * (size_t)i1]; o[4] = verts[3 * (size_t)i1 + 1]; o[5] = verts[3 * (size_t)i1 + 2];
    o[6] = verts[3 * (size_t)i2]; o[7] = verts[3 * (size_t)i2 + 1]; o[8] = verts[3 * (size_t)i2 + 2];
    // face_meta[first vertex of the face] (push! path, :595), or one word per face (TLAS(items, metadata_fn), :2300-2306), or the face index
    meta[i] = vertex_meta ? vertex_meta[meta_per_face ? i : i0] : (i + 1);
}

// normals (9 floats) + uv (6 floats) of every primitive of one BLAS: build_triangle (:555-566).  Soup geometry has no mesh
// attributes: geometric normal on all three vertices, default uv.
// (a device function: k_fill_attrs runs it over a whole BLAS, k_deform_commit over the primitives it is committing; face = the source face of primitive `p`)
__device__ inline void fill_attrs_one(const RcPrim& p, const float* normals, const float* uvs, const uint32_t* indices, uint32_t face, float* o) {
    o[9] = 0.f; o[10] = 0.f; o[11] = 1.f; o[12] = 0.f; o[13] = 1.f; o[14] = 1.f;  // default uv (:561-565)
    if (normals) {
        const uint32_t* idx = indices + 3 * (size_t)face;
        for (int k = 0; k < 3; ++k) {
            const size_t v = idx[k];
            o[3 * k] = normals[3 * v]; o[3 * k + 1] = normals[3 * v + 1]; o[3 * k + 2] = normals[3 * v + 2];
            if (uvs) { o[9 + 2 * k] = uvs[2 * v]; o[10 + 2 * k] = uvs[2 * v + 1]; }
        }
    } else {
        const float3_ v0 = mk3(p.v[0], p.v[1], p.v[2]), v1 = mk3(p.v[3], p.v[4], p.v[5]), v2 = mk3(p.v[6], p.v[7], p.v[8]);
        const float3_ c = cross3(sub3(v1, v0), sub3(v2, v0));
        const float len = __builtin_sqrtf(dot3(c, c));
        for (int k = 0; k < 3; ++k) { o[3 * k] = c.x / len; o[3 * k + 1] = c.y / len; o[3 * k + 2] = c.z / len; }
    }
}
__global__ void k_fill_attrs(const RcPrim* prims, uint32_t n, const float* normals, const float* uvs, const uint32_t* indices,
                             const uint32_t* src_face, float* out) {
    uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    fill_attrs_one(prims[j], normals, uvs, indices, normals ? src_face[j] : 0u, out + 15 * (size_t)j);
}

// Triangle{UInt32} (src/triangle_mesh.jl:1-7), 136 bytes = 34 words: vertices 9, normals 9, tangents 9 (NaN), uv 6, metadata
__global__ void k_export_triangles(const RcPrim* prims, const float* attrs, uint32_t n, uint32_t* out) {
    uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const RcPrim p = prims[j];
    const float* a = attrs + 15 * (size_t)j;
    uint32_t* o = out + 34 * (size_t)j;
    for (int k = 0; k < 9; ++k) o[k] = __float_as_uint(p.v[k]);
    for (int k = 0; k < 9; ++k) o[9 + k] = __float_as_uint(a[k]);
    for (int k = 0; k < 9; ++k) o[18 + k] = 0x7FC00000u;  // Vec3f(NaN)
    for (int k = 0; k < 6; ++k) o[27 + k] = __float_as_uint(a[9 + k]);
    o[33] = p.meta;
}

// shading epilogue (docs/src/wavefront-renderer.jl:382-387): normalize(n0*b1 + n1*b2 + n2*b3), uv0*b1 + uv1*b2 + uv2*b3
__global__ void k_shading_attributes(const RcHit* hits, uint64_t n, const float* attrs, float* normals, float* uvs) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const RcHit h = hits[i];
    float nx = 0.f, ny = 0.f, nz = 0.f, tu = 0.f, tv = 0.f;
    if (h.hit) {
        const float* a = attrs + 15 * (size_t)h.primitive_id;
        const float b1 = (1.0f - h.bary_u) - h.bary_v, b2 = h.bary_u, b3 = h.bary_v;  // :2015
        const float sx = (a[0] * b1 + a[3] * b2) + a[6] * b3, sy = (a[1] * b1 + a[4] * b2) + a[7] * b3, sz = (a[2] * b1 + a[5] * b2) + a[8] * b3;
        const float len = __builtin_sqrtf((sx * sx + sy * sy) + sz * sz);
        nx = sx / len; ny = sy / len; nz = sz / len;
        tu = (a[9] * b1 + a[11] * b2) + a[13] * b3;
        tv = (a[10] * b1 + a[12] * b2) + a[14] * b3;
    }
    if (normals) { normals[3 * i] = nx; normals[3 * i + 1] = ny; normals[3 * i + 2] = nz; }
    if (uvs) { uvs[2 * i] = tu; uvs[2 * i + 1] = tv; }
}

// generate_reflection_rays! with roughness 0 (docs/src/wavefront-renderer.jl:431-476) on reflect (src/math.jl:80)
__global__ void k_reflection_rays(const RcRay* rays, const RcHit* hits, uint64_t n, const float* attrs, float bias, RcRay* out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const RcHit h = hits[i];
    RcRay rr = RC_DUMMY_RAY;
    if (h.hit) {
        const RcRay r = rays[i];
        const float* a = attrs + 15 * (size_t)h.primitive_id;
        const float b1 = (1.0f - h.bary_u) - h.bary_v, b2 = h.bary_u, b3 = h.bary_v;
        const float sx = (a[0] * b1 + a[3] * b2) + a[6] * b3, sy = (a[1] * b1 + a[4] * b2) + a[7] * b3, sz = (a[2] * b1 + a[5] * b2) + a[8] * b3;
        const float len = __builtin_sqrtf((sx * sx + sy * sy) + sz * sz);
        const float3_ nrm = mk3(sx / len, sy / len, sz / len);
        const float3_ o = mk3(r.ox, r.oy, r.oz), d = mk3(r.dx, r.dy, r.dz);
        const float3_ hp = add3(o, scale3(d, h.t));
        const float3_ wo = mk3(-d.x, -d.y, -d.z);
        const float k = 2.0f * dot3(wo, nrm);
        const float3_ rd = add3(mk3(-wo.x, -wo.y, -wo.z), scale3(nrm, k));
        const float3_ ro = add3(hp, scale3(nrm, bias));
        rr = RcRay{ro.x, ro.y, ro.z, 0.0f, rd.x, rd.y, rd.z, INFINITY};
    }
    rc::store_ray(out, i, rr);
}

// The optional GATE of the TLAS chain's kernels (rc_refit_or_rebuild_tlas_async): a word an EARLIER kernel on the same stream wrote.  Every
// kernel that writes anything outside the rebuild scratch -- TLAS nodes, topology records, instance -> leaf table, top renumbering,
// traversal copy -- returns when it reads 0, the whole grid alike and before any barrier; nullptr = run, which every other caller passes.
__device__ inline bool gate_closed(const uint32_t* gate) { return gate && *gate == 0u; }

// fill_bvhnode2_kernel! (src/instanced-bvh-kernels.jl:19-22) with the empty node of :1407-1410
__global__ void k_fill_nodes(RcNode* nodes, uint32_t n_nodes, const uint32_t* gate) {
    if (gate_closed(gate)) return;
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    RcNode e;
#pragma unroll
    for (int k = 0; k < 12; ++k) e.f[k] = 0.0f;
    e.child0 = e.child1 = e.parent = RC_INVALID_NODE;
    e.pad = 0;
    nodes[i] = e;
}

// clz32 / delta (src/instanced-bvh.jl:1203-1229); indices are 1-based like the reference
__device__ inline int clz32(uint32_t x) { return x == 0 ? 32 : __clz((int)x); }
__device__ inline int delta(int i1, int i2, const uint32_t* codes, int n) {
    int left = i1 < i2 ? i1 : i2, right = i1 < i2 ? i2 : i1;
    if (left < 1 || right > n) return -1;
    uint32_t lc = codes[left - 1], rc = codes[right - 1];
    if (lc != rc) return clz32(lc ^ rc);
    return 32 + clz32((uint32_t)left ^ (uint32_t)right);
}

// emit_topology_kernel! (src/instanced-bvh-kernels.jl:119-152) = find_span_for_node + find_split_in_span
// (src/instanced-bvh.jl:1232-1290)
// (a device function: k_topology runs it over arrays in memory, k_rebuild_tlas_fused over arrays in LDS)
__device__ inline void topology_node(int idx, RcNode* nodes, const uint32_t* codes, int n, uint4* meta) {
    int d_left = delta(idx, idx - 1, codes, n);
    int d_right = delta(idx, idx + 1, codes, n);
    int d = d_right > d_left ? 1 : -1;
    int delta_min = delta(idx, idx - d, codes, n);
    int l_max = 2;
    while (delta(idx, idx + l_max * d, codes, n) > delta_min) l_max *= 2;
    int l = 0, t = l_max;
    while (t > 1) {
        t = t / 2;
        if (delta(idx, idx + (l + t) * d, codes, n) > delta_min) l = l + t;
    }
    int j = idx + l * d;
    int span_left = d > 0 ? idx : j, span_right = d > 0 ? j : idx;
    int numidentical = delta(span_left, span_right, codes, n);
    int left = span_left, right = span_right;
    while (right > left + 1) {
        int newsplit = (right + left) / 2;
        if (delta(left, newsplit, codes, n) > numidentical) left = newsplit; else right = newsplit;
    }
    int split = left;
    int child0 = (split == span_left) ? (n - 1 + split) : split;
    int c1 = split + 1;
    int child1 = (c1 == span_right) ? (n - 1 + c1) : c1;
    nodes[idx - 1].child0 = (uint32_t)child0;
    nodes[idx - 1].child1 = (uint32_t)child1;
    nodes[idx - 1].pad = 0;
    // Compact copy of the topology for the refit (16 bytes per internal node: sorted-leaf range, child0, parent; 4 per leaf: parent), so
    // that it reads 20 MB per million leaves instead of one word each out of 2 x 64 MB of node records.
    uint32_t* mw = reinterpret_cast<uint32_t*>(meta);
    uint32_t* leaf_parent = mw + 4 * (size_t)(n - 1);
    mw[4 * (size_t)(idx - 1) + 0] = (uint32_t)span_left;
    mw[4 * (size_t)(idx - 1) + 1] = (uint32_t)span_right;
    mw[4 * (size_t)(idx - 1) + 2] = (uint32_t)child0;
    if (child0 < n) mw[4 * (size_t)(child0 - 1) + 3] = (uint32_t)idx; else leaf_parent[child0 - n] = (uint32_t)idx;
    if (child1 < n) mw[4 * (size_t)(child1 - 1) + 3] = (uint32_t)idx; else leaf_parent[child1 - n] = (uint32_t)idx;
    if (idx == 1) mw[3] = RC_INVALID_NODE;
    // set_parent_pointers_kernel! (src/instanced-bvh-kernels.jl:159-191) folded in: a node's parent word is written exactly once, by
    // its parent's thread (the root's by its own), so no separate pass and no fill pass are needed -- every other word of every node is
    // written by this kernel (child words), the leaf kernels (leaf payload) or the refit (both boxes of every internal node).
    nodes[child0 - 1].parent = (uint32_t)idx;
    nodes[child1 - 1].parent = (uint32_t)idx;
    if (idx == 1) nodes[0].parent = RC_INVALID_NODE;
}
__global__ void k_topology(RcNode* nodes, const uint32_t* codes, int n, uint4* meta, const uint32_t* gate) {
    if (gate_closed(gate)) return;
    int idx = blockIdx.x * blockDim.x + threadIdx.x + 1;
    if (idx >= n) return;
    topology_node(idx, nodes, codes, n, meta);
}

// create_leaf_nodes_kernel! (src/instanced-bvh-kernels.jl:198-226)
__global__ void k_blas_leaves(RcNode* nodes, const RcPrim* prims, uint32_t n) {
    uint32_t j = blockIdx.x * blockDim.x + threadIdx.x + 1;
    if (j > n) return;
    // 16-byte stores instead of one store per word (a wave's 64 leaves are 4 KiB apart word by word); the parent word (14) belongs to
    // the topology kernel and is left alone
    const float2* pv = reinterpret_cast<const float2*>(prims + (j - 1));  // RcPrim is 40 bytes: 8-byte aligned
    const float2 a = pv[0], b = pv[1], c = pv[2], d = pv[3], e = pv[4];   // v[0..9]: nine vertex floats, then the metadata word
    uint4* q = reinterpret_cast<uint4*>(&nodes[(n - 1 + j) - 1]);
    q[0] = make_uint4(__float_as_uint(a.x), __float_as_uint(a.y), __float_as_uint(b.x), __float_as_uint(b.y));
    q[1] = make_uint4(__float_as_uint(c.x), __float_as_uint(c.y), __float_as_uint(d.x), __float_as_uint(d.y));
    q[2] = make_uint4(__float_as_uint(e.x), 0u, 0u, 0u);  // f[8], f[9..11] = 0
    uint32_t* w = reinterpret_cast<uint32_t*>(q + 3);
    *reinterpret_cast<uint2*>(w) = make_uint2(RC_INVALID_NODE, j);  // child0, child1
    w[3] = 0u;                                                      // pad
}

// Device-coherent 8/16-byte accesses for data exchanged between workgroups inside one launch: sc0 sc1 loads and
// stores on both sides go past the (non-coherent) per-CU L1 and per-XCD L2 (CDNA guide, Guideline 16).
typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));
__device__ inline void store_coherent(float* p, f4v v) { asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" ::"v"(p), "v"(v) : "memory"); }
__device__ inline void store_coherent(float* p, f2v v) { asm volatile("global_store_dwordx2 %0, %1, off sc0 sc1" ::"v"(p), "v"(v) : "memory"); }
__device__ inline f4v load4_coherent(const float* p) {
    f4v v;
    asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
    return v;
}
__device__ inline f2v load2_coherent(const float* p) {
    f2v v;
    asm volatile("global_load_dwordx2 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
    return v;
}

// refit_aabbs_kernel! / refit_tlas_aabbs_kernel! (src/instanced-bvh-kernels.jl:239-286, 381-428): one thread per
// leaf walks up; the SECOND arrival at a node (atomic counter) continues.  The reference's second arrival re-reads
// both children and writes both child boxes; here every arriving thread carries its subtree box in registers and
// publishes it straight into its slot of the parent (aabb0 if it came from child0, aabb1 otherwise), so the second
// arrival only has to read the sibling's 24 bytes.  Same min/max over the same values => identical node contents.
//
// Most of the tree never needs that cross-workgroup machinery: a workgroup owns kRefitBlock consecutive sorted leaves, and every
// internal node whose leaf range (kept by k_topology) lies inside that window is met only by the workgroup's own threads -- its
// index lies in the window too (a Karras node's index is inside its range).  Those nodes use an LDS arrival counter and LDS box
// slots, and the second arrival writes the finished node with plain stores.  Only the few nodes that span windows (about
// 2 log2(window) per workgroup) go through device-scope atomics and write-through stores.  Measured on 4 M triangles: 0.79 ms -> see DESIGN.
//
// join_boxes: the union of a subtree box with its sibling's in the reference's operand order, min.(aabb0, aabb1) (:1144-1147)
__device__ inline void join_boxes(bool first_slot, float3_& mn, float3_& mx, float3_ smn, float3_ smx) {
    mn = first_slot ? min3v(mn, smn) : min3v(smn, mn);
    mx = first_slot ? max3v(mx, smx) : max3v(smx, mx);
}
constexpr int kRefitBlock = 1024;
__global__ __launch_bounds__(kRefitBlock) void k_refit(RcNode* nodes, const RcPrim* prims, uint32_t* flags, const uint4* meta, uint32_t n, int tlas, const uint32_t* gate) {
    if (gate_closed(gate)) return;
    __shared__ uint32_t l_flags[kRefitBlock];
    __shared__ float l_box[kRefitBlock][2][6];
    // Topology of the window's own internal nodes (indices base+1 .. base+kRefitBlock), fetched once with every thread's loads in
    // flight together: the walk below then takes each in-window step from LDS instead of paying a dependent global load per level.
    // l_c0 = child0 with bit 31 set when the node's leaf range lies inside the window (=> only this workgroup ever visits it).
    __shared__ uint32_t l_parent[kRefitBlock], l_c0[kRefitBlock];
    const uint32_t base = blockIdx.x * kRefitBlock;  // this workgroup's leaves are sorted positions base+1 .. base+kRefitBlock
    l_flags[threadIdx.x] = 0u;
    {
        const uint32_t idx = base + threadIdx.x + 1;  // 1-based internal node index
        uint32_t par = RC_INVALID_NODE, c0 = 0u;
        if (idx < n) {
            const uint4 m = meta[idx - 1];  // range, child0, parent
            par = m.w;
            c0 = m.z | ((m.x > base && m.y <= base + kRefitBlock) ? 0x80000000u : 0u);
        }
        l_parent[threadIdx.x] = par;
        l_c0[threadIdx.x] = c0;
    }
    __syncthreads();
    const uint32_t j = base + threadIdx.x + 1;
    if (j > n) return;
    uint32_t cur = n - 1 + j;
    float3_ mn, mx;
    if (tlas) {
        const RcNode& lf = nodes[cur - 1];  // leaf boxes were written by an earlier launch
        mn = mk3(lf.f[0], lf.f[1], lf.f[2]); mx = mk3(lf.f[3], lf.f[4], lf.f[5]);
    } else {
        tri_bounds(prims[j - 1], mn, mx);   // get_node_aabb of a BLAS leaf (:1149-1158)
    }
    uint32_t parent = reinterpret_cast<const uint32_t*>(meta + (n - 1))[j - 1];  // the leaf's parent
    while (parent != RC_INVALID_NODE) {
        RcNode* nd = &nodes[parent - 1];
        const uint32_t li = parent - 1u - base;  // < kRefitBlock iff the node's index is in the window
        const uint32_t c0w = li < (uint32_t)kRefitBlock ? l_c0[li] : 0u;
        uint32_t next_parent;
        if (c0w >> 31) {
            // ---- inside the window: LDS protocol
            const bool first_slot = (c0w & 0x7FFFFFFFu) == cur;
            next_parent = l_parent[li];
            float* mine = l_box[li][first_slot ? 0 : 1];
            mine[0] = mn.x; mine[1] = mn.y; mine[2] = mn.z; mine[3] = mx.x; mine[4] = mx.y; mine[5] = mx.z;
            const uint32_t old = __hip_atomic_fetch_add(&l_flags[li], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (old != 1u) break;
            const float* sib = l_box[li][first_slot ? 1 : 0];
            const float3_ smn = mk3(sib[0], sib[1], sib[2]), smx = mk3(sib[3], sib[4], sib[5]);
            float4* q = reinterpret_cast<float4*>(nd->f);  // the finished node: child0's box, then child1's
            if (first_slot) {
                q[0] = make_float4(mn.x, mn.y, mn.z, mx.x); q[1] = make_float4(mx.y, mx.z, smn.x, smn.y); q[2] = make_float4(smn.z, smx.x, smx.y, smx.z);
            } else {
                q[0] = make_float4(smn.x, smn.y, smn.z, smx.x); q[1] = make_float4(smx.y, smx.z, mn.x, mn.y); q[2] = make_float4(mn.z, mx.x, mx.y, mx.z);
            }
            join_boxes(first_slot, mn, mx, smn, smx);
        } else {
            // ---- spans windows: device-scope protocol
            const uint4 m = meta[parent - 1];  // topology was written by earlier launches
            const bool first_slot = m.z == cur;
            next_parent = m.w;
            float* mine = nd->f + (first_slot ? 0 : 6);
            const float* sib = nd->f + (first_slot ? 6 : 0);
            if (first_slot) { store_coherent(mine, f4v{mn.x, mn.y, mn.z, mx.x}); store_coherent(mine + 4, f2v{mx.y, mx.z}); }
            else { store_coherent(mine, f2v{mn.x, mn.y}); store_coherent(mine + 2, f4v{mn.z, mx.x, mx.y, mx.z}); }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // my box is out before my arrival is counted
            uint32_t old = __hip_atomic_fetch_add(&flags[parent - 1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (old != 1u) break;
            float3_ smn, smx;
            if (first_slot) { f2v a = load2_coherent(sib); f4v b = load4_coherent(sib + 2); smn = mk3(a.x, a.y, b.x); smx = mk3(b.y, b.z, b.w); }
            else { f4v a = load4_coherent(sib); f2v b = load2_coherent(sib + 4); smn = mk3(a.x, a.y, a.z); smx = mk3(a.w, b.x, b.y); }
            join_boxes(first_slot, mn, mx, smn, smx);
        }
        cur = parent;
        parent = next_parent;
    }
}

// corner(b, c) (src/bounds.jl:53-59)
__device__ inline float3_ corner(const float* mn, const float* mx, int c) {
    c -= 1;
    return mk3((c & 1) == 0 ? mn[0] : mx[0], (c & 2) == 0 ? mn[1] : mx[1], (c & 4) == 0 ? mn[2] : mx[2]);
}

// compute_instance_aabbs_kernel! (src/instanced-bvh-kernels.jl:38-78) + scene reduction (:1502-1511)
__device__ inline void instance_world_box(const float* transform, const RcBlasDesc& b, float3_& mn, float3_& mx) {
    float3_ c1 = xf_point(transform, corner(b.root_min, b.root_max, 1));
    mn = c1; mx = c1;
    for (int c = 2; c <= 8; ++c) {
        float3_ wc = xf_point(transform, corner(b.root_min, b.root_max, c));
        mn = min3v(mn, wc); mx = max3v(mx, wc);
    }
}
__global__ void k_instance_aabbs(const RcInstanceDesc* inst, const RcBlasDesc* descs, uint32_t n, float* aabbs,
                                 uint32_t* partials) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    float3_ mn = mk3(INFINITY, INFINITY, INFINITY), mx = mk3(-INFINITY, -INFINITY, -INFINITY);
    if (i < n) {
        const RcInstanceDesc& in = inst[i];
        instance_world_box(in.transform, descs[in.blas_index - 1], mn, mx);
        aabbs[6 * i + 0] = mn.x; aabbs[6 * i + 1] = mn.y; aabbs[6 * i + 2] = mn.z;
        aabbs[6 * i + 3] = mx.x; aabbs[6 * i + 4] = mx.y; aabbs[6 * i + 5] = mx.z;
    }
    block_reduce_bounds(mn, mx, partials);
}

// calculate_tlas_morton_codes_kernel! (src/instanced-bvh-kernels.jl:295-327); extent clamped >= 1e-6 (:1517-1521)
__device__ inline uint32_t tlas_morton_of(const float* transform, const RcBlasDesc& b, const uint32_t* enc) {
    float3_ smin = mk3(dec_f32(enc[0]), dec_f32(enc[1]), dec_f32(enc[2]));
    float3_ smax = mk3(dec_f32(enc[3]), dec_f32(enc[4]), dec_f32(enc[5]));
    float3_ e = sub3(smax, smin);
    float3_ extent = mk3(jl_max(e.x, 1e-6f), jl_max(e.y, 1e-6f), jl_max(e.z, 1e-6f));
    float3_ lc = scale3(add3(mk3(b.root_min[0], b.root_min[1], b.root_min[2]), mk3(b.root_max[0], b.root_max[1], b.root_max[2])), 0.5f);
    float3_ wc = xf_point(transform, lc);
    float3_ d = sub3(wc, smin);
    return morton30(mk3(d.x / extent.x, d.y / extent.y, d.z / extent.z));
}
__global__ void k_tlas_morton(const RcInstanceDesc* inst, const RcBlasDesc* descs, uint32_t n, const uint32_t* enc,
                              uint32_t* keys, uint32_t* vals) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const RcInstanceDesc& in = inst[i];
    keys[i] = tlas_morton_of(in.transform, descs[in.blas_index - 1], enc);
    vals[i] = i;
}

// The world box of an instance as a TLAS leaf keeps it: the eight corners of the BLAS's root box under `transform`, in corner order.
__device__ inline void tlas_leaf_box(const float* transform, const RcBlasDesc& b, float3_& mn, float3_& mx) {
    mn = mk3(INFINITY, INFINITY, INFINITY); mx = mk3(-INFINITY, -INFINITY, -INFINITY);
    for (int c = 1; c <= 8; ++c) {
        float3_ wc = xf_point(transform, corner(b.root_min, b.root_max, c));
        mn = min3v(mn, wc); mx = max3v(mx, wc);
    }
}
// (every word of the leaf but `parent`, which belongs to the topology)
__device__ inline void tlas_leaf_node(RcNode* nd, uint32_t orig, const float* transform, const RcBlasDesc& b) {
    float3_ mn, mx;
    tlas_leaf_box(transform, b, mn, mx);
    nd->f[0] = mn.x; nd->f[1] = mn.y; nd->f[2] = mn.z; nd->f[3] = mx.x; nd->f[4] = mx.y; nd->f[5] = mx.z;
    nd->f[6] = nd->f[7] = nd->f[8] = nd->f[9] = nd->f[10] = nd->f[11] = 0.0f;
    nd->child0 = RC_INVALID_NODE;
    nd->child1 = orig;
    nd->pad = 0;
}
// create_tlas_leaf_nodes_kernel! (src/instanced-bvh-kernels.jl:332-375).  sorted == nullptr => refit path:
// update_tlas_leaf_aabbs_kernel! (:487-519), the instance index is read back from child1.
__global__ void k_tlas_leaves(RcNode* nodes, const uint32_t* sorted, const RcInstanceDesc* inst, const RcBlasDesc* descs,
                              uint32_t n, const uint32_t* gate) {
    if (gate_closed(gate)) return;
    uint32_t j = blockIdx.x * blockDim.x + threadIdx.x + 1;
    if (j > n) return;
    RcNode* nd = &nodes[(n - 1 + j) - 1];
    uint32_t orig = sorted ? sorted[j - 1] : nd->child1;
    const RcInstanceDesc& in = inst[orig];
    tlas_leaf_node(nd, orig, in.transform, descs[in.blas_index - 1]);
}

// ---- single-BLAS scenes: breadth-first renumbering of the BLAS's top internal nodes in the traversal copy (rc_traverse_core.h,
// kLdsPlaneNodes).  remap[old - 1] = new index of internal node `old`: the first K nodes of a breadth-first walk (child0 before
// child1, internal nodes only) get 1..K in that order, the nodes they displace take the vacated indices, everything else stays.
__global__ void k_iota1(uint32_t* out, uint32_t n, const uint32_t* gate) {
    if (gate_closed(gate)) return;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = i + 1u;
}
constexpr int kTopBlock = 1024;
__global__ __launch_bounds__(kTopBlock) void k_top_remap(const RcNode* nodes, uint32_t n_leaves, uint32_t K, uint32_t* remap, const uint32_t* gate) {
    if (gate_closed(gate)) return;
    typedef hipcub::BlockScan<uint32_t, kTopBlock> Scan;
    __shared__ typename Scan::TempStorage tmp;
    __shared__ uint32_t top[rc::kPartialPlaneNodes16], in_top[rc::kPartialPlaneNodes16 + 1], d_list[rc::kPartialPlaneNodes16], v_list[rc::kPartialPlaneNodes16];  // K <= kPartialPlaneNodes16 < kTopBlock
    const uint32_t t = threadIdx.x;
    if (t == 0) top[0] = 1u;
    if (t <= K) in_top[t] = 0u;
    __syncthreads();
    uint32_t begin = 0, end = 1;
    while (end < K && begin < end) {  // one tree level per round
        uint32_t c0 = 0, c1 = 0, k0 = 0, k1 = 0;
        if (t < end - begin) {
            const RcNode& nd = nodes[top[begin + t] - 1];
            c0 = nd.child0; c1 = nd.child1;
            k0 = c0 < n_leaves ? 1u : 0u; k1 = c1 < n_leaves ? 1u : 0u;  // internal nodes are 1..n-1
        }
        uint32_t off, total;
        Scan(tmp).ExclusiveSum(k0 + k1, off, total);
        if (k0 && end + off < K) top[end + off] = c0;
        if (k1 && end + off + k0 < K) top[end + off + k0] = c1;
        begin = end;
        end = end + total < K ? end + total : K;
        __syncthreads();
    }
    const uint32_t n_top = end;  // == K whenever the tree has K internal nodes (the caller guarantees it)
    if (t < n_top && top[t] <= n_top) in_top[top[t]] = 1u;
    __syncthreads();
    // displaced = indices 1..n_top that are not top nodes (ascending); vacated = top nodes with an index above n_top (walk order)
    const uint32_t is_d = (t >= 1 && t <= n_top && !in_top[t]) ? 1u : 0u;
    uint32_t rank, total;
    Scan(tmp).ExclusiveSum(is_d, rank, total);
    if (is_d) d_list[rank] = t;
    __syncthreads();
    const uint32_t is_v = (t < n_top && top[t] > n_top) ? 1u : 0u;
    Scan(tmp).ExclusiveSum(is_v, rank, total);
    if (is_v) v_list[rank] = top[t];
    __syncthreads();
    if (t < total) remap[d_list[t] - 1] = v_list[t];
    if (t < n_top) remap[top[t] - 1] = t + 1u;
}
// Node i (0-based) into the traversal copy through the renumbering (remap == nullptr: none): an internal node moves to its new slot and
// names its internal children by their new indices
// (the leaves -- nodes n_leaves .. 2 n_leaves - 1 --: tlas_cull == nullptr, a BLAS: they hold triangles and take the leaf packing; else a
// TLAS: its leaves take the entry data of their instance, rc_pack_tlas_leaf, from the entry-cull spheres at tlas_cull)
// (a device function: k_pack_nodes_remap runs it over a finished tree, k_deform_commit over the staged one it is committing)
__device__ inline RcNode pack_node_or_leaf(const RcNode& nd, bool leaf, const float4* tlas_cull) {
    if (!leaf) return rc_pack_node(nd);
    return tlas_cull ? rc_pack_tlas_leaf(nd, tlas_cull + 2 * (size_t)nd.child1) : rc_pack_leaf(nd);
}
__device__ inline void pack_node_renumbered(RcNode nd, uint32_t i, uint32_t n_leaves, const uint32_t* remap, const float4* tlas_cull, RcNode* dst) {
    uint32_t at = i;
    if (remap && i + 1u < n_leaves) {
        if (nd.child0 < n_leaves) nd.child0 = remap[nd.child0 - 1];
        if (nd.child1 < n_leaves) nd.child1 = remap[nd.child1 - 1];
        at = remap[i] - 1u;
    }
    dst[at] = pack_node_or_leaf(nd, i + 1u >= n_leaves, tlas_cull);
}
__global__ void k_pack_nodes_remap(const RcNode* src, RcNode* dst, uint32_t n_nodes, uint32_t n_leaves, const uint32_t* remap, const float4* tlas_cull,
                                   const uint32_t* gate) {
    if (gate_closed(gate)) return;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    pack_node_renumbered(src[i], i, n_leaves, remap, tlas_cull, dst);
}

// Traversal copy of a node array: interior nodes in the packed order of rc_pack_node, the leaves -- nodes n_leaves .. of a tree with n_leaves
// leaves -- as rc_pack_leaf (the triangles of a BLAS: tlas_cull == nullptr) or rc_pack_tlas_leaf (a TLAS).
__global__ void k_pack_nodes(const RcNode* src, RcNode* dst, uint32_t n, uint32_t n_leaves, const float4* tlas_cull, const uint32_t* gate) {
    if (gate_closed(gate)) return;
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = pack_node_or_leaf(src[i], i + 1u >= n_leaves, tlas_cull);
}

// Per BLAS: the radius, about the centre of its root AABB, of the sphere that holds every LEAF AABB (for a triangle: the distance from the
// centre to the farthest corner of the triangle's own box).  The reference reaches a triangle only through a slab test of that box, so a
// ray that stays clear of this sphere -- by more than the slab test's rounding and its 1e-5 direction clamp can move it, see
// k_inst_recs -- reaches no triangle of the BLAS.  Radii are >= 0: their bit patterns order like the values, and a NaN sorts above all.
// (one primitive's share, as float bits; a device function: k_cull_radius folds it over every BLAS of the scene, k_deform_commit over the one it commits)
__device__ inline uint32_t cull_radius_bits(const float* v, const float* root_min, const float* root_max) {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float c = 0.5f * (root_min[k] + root_max[k]);
        const float a = fminf(fminf(v[k], v[3 + k]), v[6 + k]), b = fmaxf(fmaxf(v[k], v[3 + k]), v[6 + k]);
        const float m = fmaxf(fabsf(a - c), fabsf(b - c));
        acc += m * m;
        if (!(v[k] == v[k]) || !(v[3 + k] == v[3 + k]) || !(v[6 + k] == v[6 + k])) acc = NAN;  // (fmin / fmax drop NaNs: keep them)
    }
    return __float_as_uint(sqrtf(acc) * 1.000001f);
}
__global__ void k_cull_radius(const RcPrim* prims, uint32_t n, const RcBlasDesc* descs, uint32_t nb, uint32_t* out_bits) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool tail = i >= n;  // (threads past the end repeat the last primitive: every thread reaches the barriers below)
    if (tail) i = n - 1;
    uint32_t lo = 0, hi = nb;  // the BLAS whose primitive range holds i: the last one whose offset is <= i
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (descs[mid].primitives_offset <= i) lo = mid; else hi = mid; }
    const RcBlasDesc& d = descs[lo];
    // one atomic per workgroup when the whole workgroup sits in one BLAS (the usual case: a 34 M-triangle BLAS would otherwise queue
    // 34 M atomics on one address), per lane otherwise
    const uint32_t bits = cull_radius_bits(prims[i].v, d.root_min, d.root_max);
    __shared__ uint32_t sh_first, sh_same, sh_max;
    if (threadIdx.x == 0) { sh_first = lo; sh_same = 1u; sh_max = 0u; }
    __syncthreads();
    if (lo != sh_first) sh_same = 0u;
    __syncthreads();
    if (sh_same) {
        atomicMax(&sh_max, bits);
        __syncthreads();
        if (threadIdx.x == 0) atomicMax(out_bits + lo, sh_max);
    } else {
        atomicMax(out_bits + lo, bits);
    }
}

// Traversal-side instance records: inverse transform + the BLAS offsets it would otherwise chase -- and the instance's ENTRY-CULL sphere.
//
// Entry cull (option "entry_cull").  A TLAS leaf's box is the world AABB of the instance's rotated root box: for round geometry most rays
// that pass it miss the instance (C3: 72 % of the instance entries reach no triangle), and every such entry costs the ray transform, the
// three exact reciprocals and a descent that finds nothing.  A skipped entry is exact iff the reference's own traversal of the instance
// would have tested no triangle: its state after leaving the instance (closest hit, stack, world ray) is then its state before.
//   (1) In a BLAS of >= 2 triangles every triangle sits in a leaf that is reached only as a child whose box passed the parent's slab
//       test (intersect_internal_node, :1807-1832); the box is the min / max of the three vertices (exact).
//   (2) fast_intersect_bbox (:1841-1859) passes only if, for some t in [t_min, closest_t], the ray o' + t e is within 3 eps (|o'| + |box|)
//       per axis of the box -- o' the computed local origin, e the computed local direction with every component below 1e-5 in magnitude
//       replaced by +-1e-5 (safe_invdir); NaNs fail the test (NaN-propagating min / max).
//   (3) |e - d'| < 1.74e-5, and o', d' are the exact images of the world ray under the inverse transform the traversal applies up to
//       4 eps (|Minv| |o| + |t'|) and 3 eps |Minv| |d|.
//   So at that t the TRUE world ray is within
//       r_w + sigma(W) 1.74e-5 |t| + 3 eps kappa |d| |t| + 6 eps (kappa (|o| + |c_w|) + sigma(W) (2 |c'| + r'))
//   of c_w, with W = Minv^-1, (c', r') the sphere about the root box's centre that holds every leaf box (k_cull_radius), c_w = W (c' - t'),
//   r_w = sigma(W) r', kappa = sigma(W) sigma(Minv).  The kernel skips the entry only when the SEGMENT t in [t_min, closest_t] of the ray
//   stays outside the sphere of radius  A + A_ray + (B + 5e-6 |d|) t_bound  around c_w, where
//       A = 1.01 r_w + 8e-5 (|c_w|_1 + r_w + sigma(W) |c'|_1),  A_ray = 8e-5 |o|_1,  B = 4e-5 sigma(W),
//       t_bound = 2 (|t_c| + (A + A_ray) / |d|) >= every t at which the ray is that close (t_c = the parameter of closest approach),
//   and the squared distance is first reduced by 4e-6 |c_w - o|^2 (16x its own rounding): 2.3x the clamp's reach, > 10x every rounding
//   term (kappa <= 16: 8e-5 / 16 = 80 eps).  The sphere comes from the INVERSE transform the traversal uses, not from the forward one (a
//   caller may pass an inverse of its own).  Outside the regime these bounds assume nothing is skipped: instances with non-finite or
//   ill-conditioned transforms (kappa > 16), stretch above 100 or a single-triangle BLAS (that triangle is tested without any box test:
//   a coplanar ray anywhere in the TLAS leaf's box gets the reference's NaN hit) get A = +inf; rays with a non-finite component or |d|^2
//   outside [1e-2, 1e6] carry a NaN that fails the comparison (rc_traverse_core.h).  tests/test_gpu_entry_cull.py aims rays at every one of
//   these edges and compares cull on / off / oracle bit for bit; mutants of the constants are caught by it.
// (one derivation, two callers: k_inst_recs over descriptors that are in memory, k_update_instances over the ones it is writing)
__device__ inline RcInstRec inst_rec_of(const float* inv, uint32_t blas_index, uint32_t instance_id, const RcBlasDesc& bd, const uint32_t* blas_nprims) {
    RcInstRec r;
#pragma unroll
    for (int k = 0; k < 12; ++k) r.inv[k] = inv[k];
    r.nodes_offset = bd.nodes_offset;
    r.prims_offset = bd.primitives_offset;
    r.custom_index = instance_id;
    r.n_prims = blas_nprims[blas_index - 1];
    return r;
}
__device__ inline void entry_cull_sphere(const float* m, const RcBlasDesc& bd, uint32_t n_prims, uint32_t r_bits, float4& out0, float4& out1) {
    // m = the inverse transform, rows [a b c | t]: local = Minv * world + t
    const double a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[4], a11 = m[5], a12 = m[6], a20 = m[8], a21 = m[9], a22 = m[10];
    const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
    const double det = a00 * c00 + a01 * c01 + a02 * c02;
    const double id = 1.0 / det;
    const double w[9] = {c00 * id, (a02 * a21 - a01 * a22) * id, (a01 * a12 - a02 * a11) * id,
                         c01 * id, (a00 * a22 - a02 * a20) * id, (a02 * a10 - a00 * a12) * id,
                         c02 * id, (a01 * a20 - a00 * a21) * id, (a00 * a11 - a01 * a10) * id};  // W = Minv^-1, row-major
    const double mi[9] = {a00, a01, a02, a10, a11, a12, a20, a21, a22};
    auto sigma_ub = [](const double* q) {  // sqrt(||Q^T Q||_inf) >= the largest singular value; exact for rotation x uniform scale
        double best = 0.0;
        for (int r0 = 0; r0 < 3; ++r0) {
            double row = 0.0;
            for (int c0 = 0; c0 < 3; ++c0) row += fabs(q[0 + r0] * q[0 + c0] + q[3 + r0] * q[3 + c0] + q[6 + r0] * q[6 + c0]);
            best = row > best ? row : best;
        }
        return sqrt(best);
    };
    const double sW = sigma_ub(w), sI = sigma_ub(mi);
    const double lx = 0.5 * ((double)bd.root_min[0] + bd.root_max[0]) - m[3], ly = 0.5 * ((double)bd.root_min[1] + bd.root_max[1]) - m[7],
                 lz = 0.5 * ((double)bd.root_min[2] + bd.root_max[2]) - m[11];
    const double cx = w[0] * lx + w[1] * ly + w[2] * lz, cy = w[3] * lx + w[4] * ly + w[5] * lz, cz = w[6] * lx + w[7] * ly + w[8] * lz;
    const double rl = (double)__uint_as_float(r_bits);
    const double rw = rl * sW * 1.00001;
    const double lc1 = fabs(0.5 * ((double)bd.root_min[0] + bd.root_max[0])) + fabs(0.5 * ((double)bd.root_min[1] + bd.root_max[1])) +
                       fabs(0.5 * ((double)bd.root_min[2] + bd.root_max[2]));  // |c'|_1: a mesh far from its own origin has large LOCAL coordinates, and the slab test rounds in those
    double A = 1.01 * rw + 8.0e-5 * (fabs(cx) + fabs(cy) + fabs(cz) + rw + sW * lc1);
    const double B = 4.0e-5 * sW;
    const bool ok = n_prims >= 2u && sW <= 100.0 && sW * sI <= 16.0 && A < 1.0e30 && fabs(cx) < 1.0e30 && fabs(cy) < 1.0e30 && fabs(cz) < 1.0e30;  // (NaN anywhere: false)
    if (!ok) A = INFINITY;
    out0 = make_float4((float)cx, (float)cy, (float)cz, (float)A * (ok ? 1.000001f : 1.0f));
    out1 = make_float4(ok ? (float)B * 1.000001f : 0.0f, 0.f, 0.f, 0.f);
}
__global__ void k_inst_recs(const RcInstanceDesc* inst, const RcBlasDesc* descs, const uint32_t* blas_nprims, uint32_t n, RcInstRec* out,
                            const uint32_t* cull_r_bits, float4* cull_out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const RcInstanceDesc& in = inst[i];
    const RcBlasDesc& bd = descs[in.blas_index - 1];
    const RcInstRec r = inst_rec_of(in.inv_transform, in.blas_index, in.instance_id, bd, blas_nprims);
    out[i] = r;
    if (!cull_out) return;
    float4 c0, c1;
    entry_cull_sphere(in.inv_transform, bd, r.n_prims, cull_r_bits[in.blas_index - 1], c0, c1);
    cull_out[2 * i] = c0;
    cull_out[2 * i + 1] = c1;
}

// Device-side update_transforms! (update_instance_transforms_offset_kernel!, src/instanced-bvh-kernels.jl:455-476) fused with everything a
// refit derives PER INSTANCE from the new transform: for instance first + i it reads xforms[i] once and writes the descriptor's transform and
// inverse (blas_index, instance_id and flags stay), the traversal record, the entry-cull sphere and the box of the instance's TLAS leaf --
// what k_update_inverses, k_inst_recs and k_tlas_leaves produce in three passes over the 108-byte descriptors, bit for bit (the same
// device functions).  leaf_of[instance] = sorted position (1-based) of its leaf, topology only (k_inst_leaf, rc_build_tlas).
// The transforms go through LDS so that a wave reads consecutive dwords whatever the alignment of `xforms`; the 108-byte descriptors are
// written dword by dword like everywhere else, the 64-byte records and nodes with 16-byte stores.
__global__ __launch_bounds__(kBlock) void k_update_instances(const float* __restrict__ xforms, uint32_t first, uint32_t m, RcInstanceDesc* inst,
                                                             const RcBlasDesc* __restrict__ descs, const uint32_t* __restrict__ blas_nprims,
                                                             const uint32_t* __restrict__ cull_r_bits, const uint32_t* __restrict__ leaf_of,
                                                             RcInstRec* recs, float4* cull_out, RcNode* nodes, uint32_t n) {
    __shared__ float l_x[kBlock * 12];
    const uint32_t base = blockIdx.x * kBlock;
    const uint32_t words = (m - base < (uint32_t)kBlock ? m - base : (uint32_t)kBlock) * 12u;
    for (uint32_t w = threadIdx.x; w < words; w += kBlock) l_x[w] = xforms[(size_t)base * 12u + w];
    __syncthreads();
    const uint32_t i = base + threadIdx.x;
    if (i >= m) return;
    const uint32_t g = first + i;
    float x[12], inv[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) x[k] = l_x[threadIdx.x * 12 + k];
    rc_mat3x4_inverse_hd(x, inv);
    RcInstanceDesc& d = inst[g];
    const uint32_t blas_index = d.blas_index, instance_id = d.instance_id;
#pragma unroll
    for (int k = 0; k < 12; ++k) { d.transform[k] = x[k]; d.inv_transform[k] = inv[k]; }
    const RcBlasDesc bd = descs[blas_index - 1];
    const RcInstRec r = inst_rec_of(inv, blas_index, instance_id, bd, blas_nprims);
    uint4* q = reinterpret_cast<uint4*>(&recs[g]);
    q[0] = make_uint4(__float_as_uint(r.inv[0]), __float_as_uint(r.inv[1]), __float_as_uint(r.inv[2]), __float_as_uint(r.inv[3]));
    q[1] = make_uint4(__float_as_uint(r.inv[4]), __float_as_uint(r.inv[5]), __float_as_uint(r.inv[6]), __float_as_uint(r.inv[7]));
    q[2] = make_uint4(__float_as_uint(r.inv[8]), __float_as_uint(r.inv[9]), __float_as_uint(r.inv[10]), __float_as_uint(r.inv[11]));
    q[3] = make_uint4(r.nodes_offset, r.prims_offset, r.custom_index, r.n_prims);
    float4 c0, c1;
    entry_cull_sphere(inv, bd, r.n_prims, cull_r_bits[blas_index - 1], c0, c1);
    cull_out[2 * (size_t)g] = c0;
    cull_out[2 * (size_t)g + 1] = c1;
    float3_ mn, mx;
    tlas_leaf_box(x, bd, mn, mx);
    const uint32_t j = leaf_of[g];  // in 1..n
    RcNode* nd = &nodes[(n - 1 + j) - 1];  // the rest of the leaf (zeros, child0 = invalid, child1 = g, parent) is topology and stays
    *reinterpret_cast<float4*>(nd->f) = make_float4(mn.x, mn.y, mn.z, mx.x);
    *reinterpret_cast<float2*>(nd->f + 4) = make_float2(mx.y, mx.z);
}
// leaf_of[sorted[j - 1]] = j: where each instance's leaf sits in the Morton order of the last rebuild
__global__ void k_inst_leaf(const uint32_t* sorted, uint32_t n, uint32_t* leaf_of, const uint32_t* gate) {
    if (gate_closed(gate)) return;
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) leaf_of[sorted[j]] = j + 1u;
}

// ---- the cost of a TLAS and the decision to rebuild it (rc_tlas_cost_async, rc_refit_or_rebuild_tlas_async).  cost = sum over the internal
// nodes i = 1 .. n - 1 of A_i / A_1, A = 2 (ex ey + ey ez + ez ex) of the union of the node's two child boxes, extents in f64 from the f32
// corners (tools/probes/tlas_rebuild_probe.py, relative_area); n == 1: exactly 1.  No floating-point atomics: a block's threads take the
// nodes in a grid-stride order fixed by n alone and fold through LDS in a fixed tree, one block folds the partials the same way, so two
// evaluations of one tree give the same 8 bytes.
constexpr int kCostBlock = 256;
enum QualityMode : int { kCostOnly = 0, kDecide = 1, kRecord = 2, kArm = 3 };
__device__ inline double node_area(const RcNode& nd) {
    const double ex = (double)jl_maxf(nd.f[3], nd.f[9]) - (double)jl_minf(nd.f[0], nd.f[6]);
    const double ey = (double)jl_maxf(nd.f[4], nd.f[10]) - (double)jl_minf(nd.f[1], nd.f[7]);
    const double ez = (double)jl_maxf(nd.f[5], nd.f[11]) - (double)jl_minf(nd.f[2], nd.f[8]);
    return 2.0 * (ex * ey + ey * ez + ez * ex);
}
// (every thread of a block of kCostBlock calls it; sh: kCostBlock doubles)
__device__ inline double block_sum_fixed(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (uint32_t w = kCostBlock / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    return sh[0];
}
// What ONE thread does with a finished cost.  kCostOnly: *out.  kDecide: the cost and the gate, cost > ratio * cost_built in f64 as written (a
// NaN never rebuilds), written on every run -- a replay must not see the previous frame's decision.  kRecord, behind a rebuild: the new
// tree's cost becomes the baseline and the gate is cleared.  kArm: kRecord as the first evaluation after a sync.
__device__ inline uint32_t quality_commit(RcTlasQuality* q, double* out, double cost, double ratio, int mode, bool may_rebuild) {
    if (mode == kCostOnly) { *out = cost; return 0u; }
    if (mode == kDecide) {
        const uint32_t g = (may_rebuild && cost > ratio * q->cost_built) ? 1u : 0u;
        q->cost = cost; q->gate = g; q->last_rebuilt = g;
        q->evaluations += 1u;
        return g;
    }
    q->cost_built = cost; q->gate = 0u;  // (`cost` stays what the evaluation measured: the refitted tree's, which led to this rebuild)
    q->rebuilds += 1u;
    if (mode == kArm) { q->cost = cost; q->evaluations += 1u; q->last_rebuilt = 1u; }
    return 0u;
}
__global__ __launch_bounds__(kCostBlock) void k_tlas_cost_partials(const RcNode* __restrict__ nodes, uint32_t n, double* __restrict__ partials) {
    __shared__ double sh[kCostBlock];
    double a = 0.0;
    for (uint32_t i = blockIdx.x * kCostBlock + threadIdx.x; i + 1u < n; i += gridDim.x * kCostBlock) a += node_area(nodes[i]);
    const double sum = block_sum_fixed(a, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}
// `gate` (kRecord behind a gated chain): nothing was rebuilt, nothing to record
__global__ __launch_bounds__(kCostBlock) void k_tlas_cost_fold(const RcNode* __restrict__ nodes, uint32_t n, const double* __restrict__ partials, uint32_t n_blocks,
                                                              double* out, RcTlasQuality* q, double ratio, int mode, const uint32_t* gate) {
    if (gate_closed(gate)) return;
    __shared__ double sh[kCostBlock];
    double a = 0.0;
    for (uint32_t b = threadIdx.x; b < n_blocks; b += kCostBlock) a += partials[b];
    const double sum = block_sum_fixed(a, sh);
    if (threadIdx.x == 0) quality_commit(q, out, n < 2u ? 1.0 : sum / node_area(nodes[0]), ratio, mode, n >= 2u);
}

// ---- the whole TLAS rebuild as ONE workgroup (rc_rebuild_tlas_async; 2 <= n <= kFusedInst = kTlasLdsInst instances, the scenes whose top
// level the trace keeps in LDS and never renumbers: tlas_top_k == 0).  The chain of rc_build_tlas is a dozen dispatches plus the sort's, each
// with microseconds of work at this size; here thread i owns instance i, then sorted leaf i + 1 and internal node i + 1, and the tree is
// assembled in LDS and written out once.  Same bytes as the chain, because the arithmetic IS the chain's (the device functions above):
//  * scene bounds: min / max on the order-preserving encoding is exact in any order; with one block, k_reduce_partials folds a single
//    partial, which is the identity;
//  * sort: thread i counts the pairs (code, index) below its own -- a total order, so the result is the one stable permutation by code,
//    rocPRIM's; n broadcast reads of LDS per thread;
//  * refit: the in-window protocol of k_refit (LDS arrival counters, the second arrival carries the union up) with the box slots in the
//    LDS copy of the node itself.  Every word of nodes 1..2n-1 is written before the copy-out: child / pad / parent words by topology_node,
//    leaves by tlas_leaf_node, both boxes of every internal node by its two arrivals.
// kQuality (rc_refit_or_rebuild_tlas_async; rc_rebuild_tlas_async on an armed scene): the same workgroup does the whole conditional step.
// kDecide: it first takes the cost of the tree in memory -- the refit's, an earlier kernel on the stream -- decides (quality_commit) and
// returns, all of it, unless the gate is set; then, as in kRecord / kArm, it builds as always, takes the new tree's cost from the LDS copy
// before the copy-out and records it.  The decision crosses no launch: it is shared inside one workgroup, behind a barrier.
constexpr int kFusedInst = rc::kTlasLdsInst;
static_assert(kFusedInst == kCostBlock, "block_sum_fixed folds kCostBlock slots");
template <bool kQuality>
__global__ __launch_bounds__(kFusedInst) void k_rebuild_tlas_fused(const RcInstanceDesc* __restrict__ inst, const RcBlasDesc* __restrict__ descs, uint32_t n,
                                                                   RcNode* __restrict__ nodes, RcNode* __restrict__ packed, uint4* __restrict__ ranges,
                                                                   uint32_t* __restrict__ leaf_of, const float4* __restrict__ cull,
                                                                   RcTlasQuality* quality, double ratio, int mode) {
    __shared__ RcNode l_nodes[2 * kFusedInst - 1];
    __shared__ uint4 l_meta[(kFusedInst - 1) + kFusedInst / 4];  // k_topology's compact records, then one parent word per leaf
    __shared__ alignas(8) float l_x[kFusedInst * 12];  // (8-byte aligned: the quality form folds its f64 partial sums through it)
    __shared__ uint32_t l_blas[kFusedInst], l_codes[kFusedInst], l_sorted_codes[kFusedInst], l_sorted[kFusedInst], l_flags[kFusedInst];
    __shared__ uint32_t l_enc[8];
    const uint32_t t = threadIdx.x;
    if constexpr (kQuality) {
        if (mode == kDecide) {
            double* l_red = reinterpret_cast<double*>(l_x);  // (the transforms are staged after the decision)
            const double sum = block_sum_fixed(t + 1u < n ? node_area(nodes[t]) : 0.0, l_red);
            if (t == 0) l_enc[7] = quality_commit(quality, nullptr, sum / node_area(nodes[0]), ratio, kDecide, true);
            __syncthreads();
            if (l_enc[7] == 0u) return;
            __syncthreads();  // (l_red is l_x)
        }
    }
    for (uint32_t w = t; w < n * 12u; w += kFusedInst) l_x[w] = inst[w / 12u].transform[w % 12u];
    if (t < n) l_blas[t] = inst[t].blas_index;
    l_flags[t] = 0u;
    __syncthreads();
    float3_ mn = mk3(INFINITY, INFINITY, INFINITY), mx = mk3(-INFINITY, -INFINITY, -INFINITY);
    if (t < n) instance_world_box(&l_x[t * 12u], descs[l_blas[t] - 1], mn, mx);
    block_reduce_bounds(mn, mx, l_enc);  // (block 0's partial: words 0..5)
    __syncthreads();
    uint32_t code = 0u;
    if (t < n) { code = tlas_morton_of(&l_x[t * 12u], descs[l_blas[t] - 1], l_enc); l_codes[t] = code; }
    __syncthreads();
    if (t < n) {
        uint32_t rank = 0u;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t c = l_codes[j];
            rank += (c < code || (c == code && j < t)) ? 1u : 0u;
        }
        l_sorted_codes[rank] = code;
        l_sorted[rank] = t;
    }
    __syncthreads();
    if (t + 1u < n) topology_node((int)t + 1, l_nodes, l_sorted_codes, (int)n, l_meta);
    if (t < n) {
        const uint32_t orig = l_sorted[t];
        tlas_leaf_node(&l_nodes[n - 1u + t], orig, &l_x[orig * 12u], descs[l_blas[orig] - 1]);
        leaf_of[orig] = t + 1u;  // k_inst_leaf
    }
    __syncthreads();
    if (t < n) {
        uint32_t cur = n + t;  // 1-based index of sorted leaf t + 1
        const RcNode& lf = l_nodes[cur - 1u];
        mn = mk3(lf.f[0], lf.f[1], lf.f[2]); mx = mk3(lf.f[3], lf.f[4], lf.f[5]);
        uint32_t parent = reinterpret_cast<const uint32_t*>(l_meta + (n - 1u))[t];
        while (parent != RC_INVALID_NODE) {
            const uint4 m = l_meta[parent - 1u];  // range, child0, parent
            const bool first_slot = m.z == cur;
            float* mine = l_nodes[parent - 1u].f + (first_slot ? 0 : 6);
            mine[0] = mn.x; mine[1] = mn.y; mine[2] = mn.z; mine[3] = mx.x; mine[4] = mx.y; mine[5] = mx.z;
            const uint32_t old = __hip_atomic_fetch_add(&l_flags[parent - 1u], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (old != 1u) break;
            const float* sib = l_nodes[parent - 1u].f + (first_slot ? 6 : 0);
            join_boxes(first_slot, mn, mx, mk3(sib[0], sib[1], sib[2]), mk3(sib[3], sib[4], sib[5]));
            cur = parent;
            parent = m.w;
        }
    }
    __syncthreads();
    if constexpr (kQuality) {  // the new tree's cost, from the LDS copy (l_x is free: the leaves were made from it before the refit)
        const double sum = block_sum_fixed(t + 1u < n ? node_area(l_nodes[t]) : 0.0, reinterpret_cast<double*>(l_x));
        if (t == 0) quality_commit(quality, nullptr, sum / node_area(l_nodes[0]), ratio, mode == kDecide ? (int)kRecord : mode, true);
    }
    for (uint32_t i = t; i < 2u * n - 1u; i += kFusedInst) {  // canonical node and traversal copy (k_pack_nodes), 16-byte stores
        const RcNode nd = l_nodes[i];
        const RcNode pk = pack_node_or_leaf(nd, i + 1u >= n, cull);  // (the spheres are in place before the rebuild: k_inst_recs / k_update_instances)
        uint4* q = reinterpret_cast<uint4*>(&nodes[i]);
        uint4* r = reinterpret_cast<uint4*>(&packed[i]);
        q[0] = make_uint4(__float_as_uint(nd.f[0]), __float_as_uint(nd.f[1]), __float_as_uint(nd.f[2]), __float_as_uint(nd.f[3]));
        q[1] = make_uint4(__float_as_uint(nd.f[4]), __float_as_uint(nd.f[5]), __float_as_uint(nd.f[6]), __float_as_uint(nd.f[7]));
        q[2] = make_uint4(__float_as_uint(nd.f[8]), __float_as_uint(nd.f[9]), __float_as_uint(nd.f[10]), __float_as_uint(nd.f[11]));
        q[3] = make_uint4(nd.child0, nd.child1, nd.parent, nd.pad);
        r[0] = make_uint4(__float_as_uint(pk.f[0]), __float_as_uint(pk.f[1]), __float_as_uint(pk.f[2]), __float_as_uint(pk.f[3]));
        r[1] = make_uint4(__float_as_uint(pk.f[4]), __float_as_uint(pk.f[5]), __float_as_uint(pk.f[6]), __float_as_uint(pk.f[7]));
        r[2] = make_uint4(__float_as_uint(pk.f[8]), __float_as_uint(pk.f[9]), __float_as_uint(pk.f[10]), __float_as_uint(pk.f[11]));
        r[3] = make_uint4(pk.child0, pk.child1, pk.parent, pk.pad);
    }
    if (t + 1u < n) ranges[t] = l_meta[t];  // the topology the later refits read
    if (t < n) reinterpret_cast<uint32_t*>(ranges + (n - 1u))[t] = reinterpret_cast<const uint32_t*>(l_meta + (n - 1u))[t];
}

// Non-owning view of the scratch ONE build chain runs on: a chain body below receives (stream, view) and nothing about who calls it.
// Three sets exist, so that chains on different streams never share a word: the scene's loose members (the builds on the scene's own
// stream), s->rebuild (rc_rebuild_tlas_async) and s->deform (rc_update_geometry_async), both on a caller's stream.
struct ChainBufs {
    uint32_t *keys_a, *keys_b, *vals_a, *vals_b;  // the sort's input pairs; the sorted keys and the permutation
    uint32_t *partials, *enc;                     // scene bounds: one partial per block, their fold
    uint32_t *zeroed, *arrive;   // run_refit zeroes from `zeroed` through its n - 1 arrival counters at `arrive` in one memset (words in front of the counters are the owner's)
    uint4* ranges;               // topology records: topology_records(n)
    float* aabbs;                // TLAS only: 6 floats per instance
    DevBuf<unsigned char>* tmp;  // the sort's temporary storage
    size_t sort_bytes;           // its size where it was reserved earlier (a chain that may not allocate); 0: query and reserve at the sort
    bool onesweep;
};
// stable sortperm of the 30-bit keys (Base.sortperm / AK.sortperm, src/instanced-bvh.jl:1399, 1533-1540).  rocPRIM's default switches
// from Onesweep to a merge sort at <= 1 Mi items (block sort + log2(n / 1024) partition/merge launch pairs: 146 us for 1 M keys); both
// are stable, so the permutation is the same and the switch point is ours to choose (opt.onesweep_min).
// The size query is a host call that depends on n and the configuration alone.  bytes == nullptr (the chains): the view's size, or query,
// reserve, sort where it brings none.  *bytes == 0: query and reserve only, the size is returned (rc_build_tlas, on behalf of the rebuild
// that may not allocate).  Otherwise: sort with storage of that size, reserved earlier -- no query, no allocation.
template <size_t MergeLimit>
static void sort_pairs_cfg(const ChainBufs& b, uint32_t n, hipStream_t st, size_t* bytes) {
    using Cfg = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, MergeLimit>;
    size_t tmp = bytes ? *bytes : b.sort_bytes;
    if (!tmp) {
        RC_HIP(rocprim::radix_sort_pairs<Cfg>(nullptr, tmp, b.keys_a, b.keys_b, b.vals_a, b.vals_b, n, 0u, 30u, st));
        if (!tmp) tmp = 1;
        b.tmp->reserve(tmp);
        if (bytes) { *bytes = tmp; return; }
    }
    RC_HIP(rocprim::radix_sort_pairs<Cfg>(b.tmp->p, tmp, b.keys_a, b.keys_b, b.vals_a, b.vals_b, n, 0u, 30u, st));
}
void sort_pairs(hipStream_t st, const ChainBufs& b, uint32_t n, size_t* bytes = nullptr) {
    if (b.onesweep) sort_pairs_cfg<4096>(b, n, st, bytes);
    else sort_pairs_cfg<(size_t)1 << 30>(b, n, st, bytes);
}

void reserve_build_scratch(rc_scene* s, uint32_t n) {
    s->keys_a.reserve(n); s->keys_b.reserve(n); s->vals_a.reserve(n); s->vals_b.reserve(n);
    s->flags.reserve(n);
    s->scene_enc.reserve(8);
}
inline size_t topology_records(uint32_t n) { return n > 1 ? (size_t)(n - 1) + (n + 3) / 4 : 1; }  // one record per internal node, then the leaves' parent words
inline unsigned blas_bounds_blocks(uint32_t n) { return std::min(grid_for(n), 1024u); }

// The scene's own scratch for a build of n items on the scene's stream, reserved here: a host call that may allocate
ChainBufs scene_bufs(rc_scene* s, uint32_t n, unsigned partial_blocks, DevBuf<uint4>& ranges) {
    reserve_build_scratch(s, n);
    s->bounds_partials.reserve((size_t)partial_blocks * 6); ranges.reserve(topology_records(n));
    return ChainBufs{s->keys_a.p, s->keys_b.p, s->vals_a.p, s->vals_b.p, s->bounds_partials.p, s->scene_enc.p, s->flags.p, s->flags.p, ranges.p,
                     s->aabb_tmp.p, &s->sort_tmp, 0, (int64_t)n >= s->opt.onesweep_min};
}
// The TLAS's scratch on a caller's stream.  Arrival counters of its own (s->tlas_flags), because s->flags is also the BLAS builds' (other stream)
ChainBufs rebuild_bufs(rc_scene* s) {
    auto& r = s->rebuild;
    return ChainBufs{r.keys_a.p, r.keys_b.p, r.vals_a.p, r.vals_b.p, r.partials.p, r.enc.p, s->tlas_flags.p, s->tlas_flags.p, s->tlas_ranges.p,
                     r.aabbs.p, &r.sort_tmp, r.sort_bytes, r.onesweep};
}

// Karras topology + parents for n items with sorted keys in b.keys_b
void emit_tree(hipStream_t st, const ChainBufs& b, RcNode* nodes, uint32_t n, const uint32_t* gate = nullptr) {
    if (n > 1) hipLaunchKernelGGL(k_topology, dim3(grid_for(n - 1)), dim3(kBlock), 0, st, nodes, b.keys_b, (int)n, b.ranges, gate);
    else hipLaunchKernelGGL(k_fill_nodes, dim3(1), dim3(kBlock), 0, st, nodes, 1u, gate);  // single leaf: empty node, the leaf kernel fills the payload
}

// The arrival counters are zeroed by a kernel, not by hipMemsetAsync: as a node of a captured graph the memset left the counters of a
// 1 520-primitive BLAS (6 080 bytes) partly at their old values on the second and later replays, and k_refit then took a first arrival for
// a second one (docs/EXPERIMENTS.md, "Kernel shapes after device-side updates"); a kernel node is ordered like every other kernel of the chain.
__global__ void k_zero_words(uint32_t* p, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0u;
}
// (the arrival counters are the refit's own scratch: zeroed whatever the gate says)
void run_refit(hipStream_t st, const ChainBufs& b, RcNode* nodes, const RcPrim* prims, uint32_t n, int tlas, const uint32_t* gate = nullptr) {
    const size_t words = (size_t)(b.arrive - b.zeroed) + (n - 1);
    if (words) hipLaunchKernelGGL(k_zero_words, dim3(grid_for(words)), dim3(kBlock), 0, st, b.zeroed, words);
    if (n < 2) return;
    hipLaunchKernelGGL(k_refit, dim3((n + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, st, nodes, prims, b.arrive, b.ranges, n, tlas, gate);
}

// old -> new index of a tree's internal nodes when its top K go to the front in breadth-first order (k_top_remap); depends on the topology only
void top_renumber(hipStream_t st, const RcNode* nodes, uint32_t n_leaves, uint32_t K, uint32_t* remap, const uint32_t* gate = nullptr) {
    hipLaunchKernelGGL(k_iota1, dim3(grid_for(n_leaves - 1)), dim3(kBlock), 0, st, remap, n_leaves - 1, gate);
    hipLaunchKernelGGL(k_top_remap, dim3(1), dim3(kTopBlock), 0, st, nodes, n_leaves, K, remap, gate);
}

// The degenerate filter over n faces: flags, their exclusive scan `pos` (storage `tmp`, sized by the caller), the valid ones compacted into `out`
void ingest_chain(hipStream_t st, const float* verts, const uint32_t* meta, uint32_t n, uint32_t* flags, uint32_t* pos, void* tmp, size_t tmp_bytes,
                  RcPrim* out, uint32_t* slot_face) {
    hipLaunchKernelGGL(k_flag_valid_faces, dim3(grid_for(n)), dim3(kBlock), 0, st, verts, n, flags);
    RC_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, flags, pos, (int)n, st));
    hipLaunchKernelGGL(k_compact_faces, dim3(grid_for(n)), dim3(kBlock), 0, st, verts, meta, flags, pos, n, out, slot_face);
}

// build_blas (src/instanced-bvh.jl:1376-1443) over the n compacted primitives `in`, in two steps; between them a caller may gather more
// than the primitives through the sorted permutation (b.vals_b).  First the Morton order: `prims` = `in` sorted ...
void blas_sort_chain(hipStream_t st, const ChainBufs& b, const RcPrim* in, uint32_t n, RcPrim* prims) {
    const unsigned nb = blas_bounds_blocks(n);
    hipLaunchKernelGGL(k_blas_scene_bounds, dim3(nb), dim3(kBlock), 0, st, in, n, b.partials);
    hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(384), 0, st, b.partials, nb, b.enc);
    hipLaunchKernelGGL(k_blas_morton, dim3(grid_for(n)), dim3(kBlock), 0, st, in, n, b.enc, b.keys_a, b.vals_a);
    sort_pairs(st, b, n);
    hipLaunchKernelGGL(k_gather_prims, dim3(grid_for(n)), dim3(kBlock), 0, st, in, b.vals_b, n, prims);
}
// ... then the tree over them: topology from the sorted keys, leaves, bottom-up boxes
void blas_tree_chain(hipStream_t st, const ChainBufs& b, const RcPrim* prims, uint32_t n, RcNode* nodes) {
    emit_tree(st, b, nodes, n);
    hipLaunchKernelGGL(k_blas_leaves, dim3(grid_for(n)), dim3(kBlock), 0, st, nodes, prims, n);
    run_refit(st, b, nodes, prims, n, 0);
}

// The box of the tree at d_root, behind everything enqueued on the scene's stream: the one host wait of a synchronous build or refit
void read_root_aabb(rc_scene* s, const RcNode* d_root, bool tlas, float mn[3], float mx[3]) {
    RcNode root;
    RC_HIP(hipMemcpyAsync(&root, d_root, sizeof(RcNode), hipMemcpyDeviceToHost, s->stream));
    RC_HIP(hipStreamSynchronize(s->stream));
    RC_HIP(hipGetLastError());
    host_root_aabb(root, tlas, mn, mx);
}

// What a TLAS derives per instance from the descriptors in s->d_instances: with `recs` the traversal records and entry-cull spheres, with
// `leaves` the leaf nodes -- in the order of `sorted` (a build), or each leaf for the instance it already names (a refit: nullptr).
void per_instance_pass(rc_scene* s, hipStream_t st, uint32_t n, bool recs, bool leaves, const uint32_t* sorted = nullptr, const uint32_t* gate = nullptr) {
    if (recs) hipLaunchKernelGGL(k_inst_recs, dim3(grid_for(n)), dim3(kBlock), 0, st, s->d_instances.p, s->d_descs.p, s->d_blas_nprims.p, n, s->inst_recs.p,
                                 (const uint32_t*)s->blas_cull_bits.p, s->inst_cull.p);
    if (leaves) hipLaunchKernelGGL(k_tlas_leaves, dim3(grid_for(n)), dim3(kBlock), 0, st, s->tlas_nodes.p, sorted, s->d_instances.p, s->d_descs.p, n, gate);
}

// The TLAS part of the traversal copy (behind the BLAS nodes), renumbered when the scene keeps the TLAS's top in LDS (tlas_top_k).  Its
// leaves copy the entry-cull spheres: every chain that changes a sphere (k_inst_recs, k_update_instances, k_deform_instances) ends here
// or in the fused rebuild's copy-out before a trace may run.
void pack_tlas(rc_scene* s, hipStream_t st, const uint32_t* gate = nullptr) {
    const uint32_t n = (s->n_tlas_nodes + 1) / 2;
    if (s->tlas_top_k) hipLaunchKernelGGL(k_pack_nodes_remap, dim3(grid_for(s->n_tlas_nodes)), dim3(kBlock), 0, st, s->tlas_nodes.p, s->flat_nodes.p + s->n_flat_nodes, s->n_tlas_nodes, n, s->tlas_remap.p, (const float4*)s->inst_cull.p, gate);
    else hipLaunchKernelGGL(k_pack_nodes, dim3(grid_for(s->n_tlas_nodes)), dim3(kBlock), 0, st, s->tlas_nodes.p, s->flat_nodes.p + s->n_flat_nodes, s->n_tlas_nodes, n, (const float4*)s->inst_cull.p, gate);
}

// build_tlas_topology (src/instanced-bvh.jl:1485-1594) from the n descriptors in s->d_instances, into the scene's TLAS arrays: tree,
// instance -> leaf table, top renumbering, traversal copy.  Every array it writes was reserved by rc_build_tlas.
// `gate` (see gate_closed): the kernels that write any of those arrays return when it reads 0; the ones that touch only the chain's scratch,
// the sort included, run regardless -- a skipped rebuild costs their time and nothing else.
void tlas_chain(rc_scene* s, hipStream_t st, const ChainBufs& b, uint32_t n, const uint32_t* gate = nullptr) {
    hipLaunchKernelGGL(k_instance_aabbs, dim3(grid_for(n)), dim3(kBlock), 0, st, s->d_instances.p, s->d_descs.p, n, b.aabbs, b.partials);
    hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(384), 0, st, b.partials, grid_for(n), b.enc);
    hipLaunchKernelGGL(k_tlas_morton, dim3(grid_for(n)), dim3(kBlock), 0, st, s->d_instances.p, s->d_descs.p, n, b.enc, b.keys_a, b.vals_a);
    sort_pairs(st, b, n);
    emit_tree(st, b, s->tlas_nodes.p, n, gate);
    // n == 1 (:1553-1570): the single leaf holds the scene AABB == the instance's world AABB (same min/max set)
    per_instance_pass(s, st, n, false, true, b.vals_b, gate);
    run_refit(st, b, s->tlas_nodes.p, nullptr, n, 1, gate);
    hipLaunchKernelGGL(k_inst_leaf, dim3(grid_for(n)), dim3(kBlock), 0, st, b.vals_b, n, s->inst_leaf.p, gate);  // instance -> leaf (rc_update_instances_async)
    if (s->tlas_top_k) top_renumber(st, s->tlas_nodes.p, n, s->tlas_top_k, s->tlas_remap.p, gate);  // topology only: computed here, reused by every refit
    pack_tlas(s, st, gate);
}

// refit_tlas! (src/instanced-bvh.jl:2197-2222) in place: per-instance data (unless it is in place already) -> bottom-up refit -> traversal copy
void refit_chain(rc_scene* s, hipStream_t st, const ChainBufs& b, uint32_t n, bool per_instance) {
    if (per_instance) per_instance_pass(s, st, n, true, true);
    run_refit(st, b, s->tlas_nodes.p, nullptr, n, 1);
    pack_tlas(s, st);
}

}  // namespace

// mat3x4_inverse (src/instanced-bvh.jl:1675-1687) with StaticArrays' 3x3 inverse (columns x0,x1,x2;
// y0 = x1 x x2; d = x0.y0; x0/=d; y0/=d; y1 = x2 x x0; y2 = x0 x x1).  Host code, -ffp-contract=off.
void rc_mat3x4_inverse(const float m[12], float out[12]) { rc_mat3x4_inverse_hd(m, out); }

// inv_transform = mat3x4_inverse(transform) for descriptors rewritten on the device (instance_buffer + refit, src/Raycore.jl:117-128)
__global__ void k_update_inverses(RcInstanceDesc* inst, uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float m[12], o[12];
    for (int k = 0; k < 12; ++k) m[k] = inst[i].transform[k];
    rc_mat3x4_inverse_hd(m, o);
    for (int k = 0; k < 12; ++k) inst[i].inv_transform[k] = o[k];
}

// Triangle ingestion on the device (build_and_append_blas! minus mesh decomposition, :581-601): raw n x 9 f32 soup
// (+ optional metadata) already in device memory -> degenerate filter -> compacted RcPrim array in s->prim_tmp.
// Returns the number of valid triangles (one 4-byte read-back).
uint32_t rc_ingest_faces(rc_scene* s, const float* d_verts, const uint32_t* d_meta, uint32_t n, bool keep_face_map) {
    if (n == 0) return 0;
    reserve_build_scratch(s, n);
    s->prim_tmp.reserve(n);
    if (keep_face_map) s->slot_face.reserve(n);
    size_t tmp = 0;
    RC_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, s->keys_a.p, s->keys_b.p, (int)n, s->stream));
    s->sort_tmp.reserve(tmp ? tmp : 1);
    ingest_chain(s->stream, d_verts, d_meta, n, s->keys_a.p, s->keys_b.p, s->sort_tmp.p, tmp, s->prim_tmp.p, keep_face_map ? s->slot_face.p : nullptr);
    uint32_t last[2];
    RC_HIP(hipMemcpyAsync(&last[0], s->keys_b.p + (n - 1), 4, hipMemcpyDeviceToHost, s->stream));
    RC_HIP(hipMemcpyAsync(&last[1], s->keys_a.p + (n - 1), 4, hipMemcpyDeviceToHost, s->stream));
    RC_HIP(hipStreamSynchronize(s->stream));
    RC_HIP(hipGetLastError());
    return last[0] + last[1];
}

void rc_expand_mesh(rc_scene* s, const float* d_verts, const uint32_t* d_indices, const uint32_t* d_vertex_meta, bool meta_per_face, uint32_t nf, float* d_soup, uint32_t* d_meta) {
    if (nf == 0) return;
    hipLaunchKernelGGL(k_expand_mesh, dim3(grid_for(nf)), dim3(kBlock), 0, s->stream, d_verts, d_indices, d_vertex_meta, meta_per_face, nf, d_soup, d_meta);
    RC_HIP(hipGetLastError());
}

void rc_ensure_flat_attrs(rc_scene* s) {
    if (s->state.flat_attrs_current()) return;
    if (s->state.deform_captured())  // (the graph baked "no attribute array" in: its replays would leave the one built here stale)
        throw RcError(6, "shading attributes cannot be built while a graph that captured a geometry update may live: use rc_shading_attributes_device once before the capture, or release the graph (\"release_captures\")");
    rc_wait_async_mutations(s);  // (an asynchronous geometry update on a caller's stream may still be writing the primitives read below)
    s->flat_attrs.reserve(15 * (size_t)(s->n_flat_prims ? s->n_flat_prims : 1));
    for (size_t i = 0; i < s->blas.size(); ++i) {
        const Blas& b = s->blas[i];
        hipLaunchKernelGGL(k_fill_attrs, dim3(grid_for(b.n_prims)), dim3(kBlock), 0, s->stream, b.prims.p, b.n_prims,
                           b.has_attrs ? b.m_normals.p : (const float*)nullptr, b.has_uvs ? b.m_uvs.p : (const float*)nullptr, b.m_indices.p, b.src_face.p,
                           s->flat_attrs.p + 15 * (size_t)s->descs[i].primitives_offset);
    }
    RC_HIP(hipGetLastError());
    RC_HIP(hipStreamSynchronize(s->stream));  // later launches may run on a caller's stream
    s->state.flat_attrs_built();
}

static hipStream_t rc_utility_stream() {
    static std::mutex mu;
    static std::map<int, hipStream_t> streams;
    int dev = 0;
    RC_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    auto it = streams.find(dev);
    if (it == streams.end()) {
        hipStream_t st = nullptr;
        RC_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        it = streams.emplace(dev, st).first;
    }
    return it->second;
}
void rc_copy_now(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    if (!bytes) return;
    hipStream_t st = rc_utility_stream();
    RC_HIP(hipMemcpyAsync(dst, src, bytes, kind, st));
    RC_HIP(hipStreamSynchronize(st));
}
void rc_memset_now(void* p, int value, size_t bytes) {
    if (!bytes) return;
    hipStream_t st = rc_utility_stream();
    RC_HIP(hipMemsetAsync(p, value, bytes, st));
    RC_HIP(hipStreamSynchronize(st));
}

void rc_launch_export_triangles(rc_scene* s, void* d_out, hipStream_t stream) {
    if (s->n_flat_prims == 0) return;
    rc_ensure_flat_attrs(s);
    hipLaunchKernelGGL(k_export_triangles, dim3(grid_for(s->n_flat_prims)), dim3(kBlock), 0, stream, s->flat_prims.p, s->flat_attrs.p, s->n_flat_prims, (uint32_t*)d_out);
    RC_HIP(hipGetLastError());
    rc_note_stage_launch(s, stream);
}

void rc_launch_shading_attributes(rc_scene* s, const RcHit* d_hits, uint64_t n, float* d_normals, float* d_uvs, hipStream_t stream) {
    if (n == 0) return;
    rc_ensure_flat_attrs(s);
    hipLaunchKernelGGL(k_shading_attributes, dim3(grid_for(n)), dim3(kBlock), 0, stream, d_hits, n, s->flat_attrs.p, d_normals, d_uvs);
    RC_HIP(hipGetLastError());
    rc_note_stage_launch(s, stream);
}

void rc_launch_reflection_rays(rc_scene* s, const RcRay* d_rays, const RcHit* d_hits, uint64_t n, float bias, RcRay* d_out, hipStream_t stream) {
    if (n == 0) return;
    rc_ensure_flat_attrs(s);
    hipLaunchKernelGGL(k_reflection_rays, dim3(grid_for(n)), dim3(kBlock), 0, stream, d_rays, d_hits, n, s->flat_attrs.p, bias, d_out);
    RC_HIP(hipGetLastError());
    rc_note_stage_launch(s, stream);
}

// build_blas (src/instanced-bvh.jl:1376-1443) over the n compacted primitives waiting in s->prim_tmp
void rc_build_blas(rc_scene* s, uint32_t n, Blas& out, bool keep_face_map) {
    out.prims.reserve(n);
    out.nodes.reserve(2 * (size_t)n - 1);
    if (keep_face_map) out.src_face.reserve(n);
    out.n_prims = n;
    out.n_nodes = 2 * n - 1;
    const ChainBufs b = scene_bufs(s, n, blas_bounds_blocks(n), s->range_tmp);
    rc_timing_scene_begin(s, s->stream);
    blas_sort_chain(s->stream, b, s->prim_tmp.p, n, out.prims.p);
    if (keep_face_map)  // source face of every Morton-sorted primitive: the attributes stay per vertex and are looked up through it
        hipLaunchKernelGGL(k_gather_u32, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, s->slot_face.p, s->vals_b.p, n, out.src_face.p);
    blas_tree_chain(s->stream, b, out.prims.p, n, out.nodes.p);
    rc_timing_scene_end(s, s->stream);
    read_root_aabb(s, out.nodes.p, false, out.root_min, out.root_max);
}

// rebuild_bvh! minus compaction (src/instanced-bvh.jl:968-992): build_tlas_topology (:1485-1594) +
// build_flat_blas_arrays! (:470-517) + the traversal instance records.
void rc_build_tlas(rc_scene* s) {
    const uint32_t n = (uint32_t)s->instances.size();
    const uint32_t nb = (uint32_t)s->blas.size();
    // flat BLAS arrays + descriptors
    s->descs.resize(nb);
    uint32_t tn = 0, tp = 0;
    for (uint32_t i = 0; i < nb; ++i) {
        s->descs[i].nodes_offset = tn; s->descs[i].primitives_offset = tp;
        memcpy(s->descs[i].root_min, s->blas[i].root_min, 12); memcpy(s->descs[i].root_max, s->blas[i].root_max, 12);
        tn += s->blas[i].n_nodes; tp += s->blas[i].n_prims;
    }
    s->n_flat_nodes = tn; s->n_flat_prims = tp;
    s->state.tlas_build_begun();
    s->flat_nodes.reserve((size_t)tn + 2 * (size_t)n + 1);  // + room for the TLAS copy behind the BLAS nodes
    s->flat_prims.reserve(tp ? tp : 1);
    s->d_descs.reserve(nb ? nb : 1);
    // LDS residency plan of the traversal copy (rc_internal.h).  Up to kTlasLdsInst instances: the whole top level fits (kernel 5) and a
    // single BLAS gets the remaining node-plane entries for its top.  More instances: the planes hold the breadth-first top of the TLAS
    // (renumbered below, after the TLAS is built) and, for a single BLAS, of the BLAS -- half each when both want more (kernel 6).
    s->blas_top_k = 0;
    s->tlas_top_k = 0;
    s->blas_top_k32 = 0;
    s->tlas_top_k32 = 0;
    // STACK16 (rc_internal.h): every tree below 65 534 nodes => 16-bit lane stacks and larger node planes.  The renumbering below is made for
    // the larger planes; the 32-bit kernels (option stack16 = 0, the drivers) stage a PREFIX of the same breadth-first order (*_top_k32).
    s->small_trees = n <= rc::kStack16MaxLeaves;
    for (uint32_t i = 0; i < nb; ++i) s->small_trees = s->small_trees && s->blas[i].n_prims <= rc::kStack16MaxLeaves;
    const bool full_lds = n > 0 && 2 * n - 1 <= (uint32_t)rc::kTlasLdsNodes;
    const bool small_enough = (uint64_t)tn + 2ull * n < (1ull << 26);  // the LDS kernels address nodes with 32-bit byte offsets
    uint32_t blas_room = 0, blas_room32 = 0;
    auto split = [&](uint32_t P, uint32_t& tk, uint32_t& bk) {  // planes of P entries shared by the TLAS's top and a single BLAS's: half each when both want more
        const uint32_t t_int = n - 1, b_int = (nb == 1 && s->blas[0].n_prims >= 2) ? s->blas[0].n_prims - 1 : 0;
        tk = t_int < P ? t_int : P; bk = b_int < P ? b_int : P;
        if (tk + bk > P) {
            const uint32_t half = P / 2;
            if (tk <= half) bk = P - tk; else if (bk <= half) tk = P - bk; else { tk = P - half; bk = half; }
        }
    };
    if (s->opt.blas_top && n > 0 && small_enough) {
        if (full_lds) {
            blas_room32 = (uint32_t)rc::kLdsPlaneNodes - (n - 1);
            blas_room = s->small_trees ? (uint32_t)rc::kLdsPlaneNodes16 - (n - 1) : blas_room32;
        } else {
            uint32_t tk, bk, tk32, bk32;
            split((uint32_t)rc::kPartialPlaneNodes, tk32, bk32);
            if (s->small_trees) split((uint32_t)rc::kPartialPlaneNodes16, tk, bk); else { tk = tk32; bk = bk32; }
            if (tk32 > tk) tk32 = tk;  // (prefixes of the renumbering that was made)
            if (bk32 > bk) bk32 = bk;
            s->tlas_top_k = tk; s->tlas_top_k32 = tk32;
            blas_room = bk; blas_room32 = bk32;
        }
    }
    if (nb == 1 && blas_room > 0 && s->blas[0].n_prims >= 2) {
        const uint32_t n_leaves = s->blas[0].n_prims, n_int = n_leaves - 1, room = blas_room;
        s->blas_top_k = n_int < room ? n_int : room;
        s->blas_top_k32 = s->blas_top_k < blas_room32 ? s->blas_top_k : blas_room32;
        s->top_remap.reserve(n_int);
        top_renumber(s->stream, s->blas[0].nodes.p, n_leaves, s->blas_top_k, s->top_remap.p);
    }
    for (uint32_t i = 0; i < nb; ++i) {
        if (s->blas_top_k) hipLaunchKernelGGL(k_pack_nodes_remap, dim3(grid_for(s->blas[i].n_nodes)), dim3(kBlock), 0, s->stream, s->blas[i].nodes.p, s->flat_nodes.p + s->descs[i].nodes_offset, s->blas[i].n_nodes, s->blas[i].n_prims, s->top_remap.p, (const float4*)nullptr, (const uint32_t*)nullptr);
        else hipLaunchKernelGGL(k_pack_nodes, dim3(grid_for(s->blas[i].n_nodes)), dim3(kBlock), 0, s->stream, s->blas[i].nodes.p, s->flat_nodes.p + s->descs[i].nodes_offset, s->blas[i].n_nodes, s->blas[i].n_prims, (const float4*)nullptr, (const uint32_t*)nullptr);
        RC_HIP(hipMemcpyAsync(s->flat_prims.p + s->descs[i].primitives_offset, s->blas[i].prims.p, sizeof(RcPrim) * s->blas[i].n_prims, hipMemcpyDeviceToDevice, s->stream));
    }
    if (nb) RC_HIP(hipMemcpyAsync(s->d_descs.p, s->descs.data(), sizeof(RcBlasDesc) * nb, hipMemcpyHostToDevice, s->stream));
    s->blas_nprims.resize(nb);
    for (uint32_t i = 0; i < nb; ++i) s->blas_nprims[i] = s->blas[i].n_prims;
    s->d_blas_nprims.reserve(nb ? nb : 1);
    if (nb) RC_HIP(hipMemcpyAsync(s->d_blas_nprims.p, s->blas_nprims.data(), sizeof(uint32_t) * nb, hipMemcpyHostToDevice, s->stream));
    s->blas_cull_bits.reserve(nb ? nb : 1);  // entry cull (k_inst_recs): per-BLAS radius of the sphere holding every leaf box
    RC_HIP(hipMemsetAsync(s->blas_cull_bits.p, 0, sizeof(uint32_t) * (nb ? nb : 1), s->stream));
    if (nb && tp) hipLaunchKernelGGL(k_cull_radius, dim3(grid_for(tp)), dim3(kBlock), 0, s->stream, s->flat_prims.p, tp, s->d_descs.p, nb, s->blas_cull_bits.p);
    s->n_static_instances = n;
    {   // the placed-primitive table: the exclusive prefix sum of the instances' primitive counts (what k_inst_recs writes to RcInstRec::n_prims)
        s->placed_base.assign((size_t)n + 1u, 0u);
        uint64_t placed = 0;
        for (uint32_t i = 0; i < n; ++i) { s->placed_base[i] = (uint32_t)placed; placed += s->blas[s->instances[i].blas_index - 1u].n_prims; }
        s->placed_base[n] = (uint32_t)placed;
        s->n_placed = placed;
        s->d_placed_base.reserve((size_t)n + 1u);
        RC_HIP(hipMemcpyAsync(s->d_placed_base.p, s->placed_base.data(), sizeof(uint32_t) * ((size_t)n + 1u), hipMemcpyHostToDevice, s->stream));
    }
    for (auto& b : s->blas) b.root_on_device = false;
    s->state.tlas_built(n == 0);
    if (n == 0) {  // :969-977
        s->n_tlas_nodes = 0;
        for (int k = 0; k < 3; ++k) { s->root_min[k] = INFINITY; s->root_max[k] = -INFINITY; }
        RC_HIP(hipStreamSynchronize(s->stream));
        return;
    }
    s->d_instances.reserve(n); s->inst_recs.reserve(n); s->inst_cull.reserve(2 * (size_t)n); s->aabb_tmp.reserve(6 * (size_t)n);
    s->tlas_nodes.reserve(2 * (size_t)n - 1); s->inst_leaf.reserve(n);
    if (s->tlas_top_k) s->tlas_remap.reserve(n - 1);
    s->n_tlas_nodes = 2 * n - 1;
    s->tlas_flags.reserve(n);  // arrival counters of the asynchronous refit: its own, because s->flags is also the BLAS builds' (other stream)
    {   // scratch of rc_rebuild_tlas_async, TLAS-only for the same reason; the sort's storage is sized here, where a host call may allocate
        auto& r = s->rebuild;
        r.keys_a.reserve(n); r.keys_b.reserve(n); r.vals_a.reserve(n); r.vals_b.reserve(n);
        r.enc.reserve(8); r.partials.reserve((size_t)grid_for(n) * 6); r.aabbs.reserve(6 * (size_t)n);
        r.n = n;
        r.onesweep = (int64_t)n >= s->opt.onesweep_min;
        r.sort_bytes = 0;
        sort_pairs(s->stream, rebuild_bufs(s), n, &r.sort_bytes);
        s->quality.reserve(kQualityStateWords + 2 * (size_t)kQualityMaxBlocks);  // (rc_refit_or_rebuild_tlas_async: disarmed above, zeroed here)
        RC_HIP(hipMemsetAsync(s->quality.p, 0, sizeof(RcTlasQuality), s->stream));
    }
    RC_HIP(hipMemcpyAsync(s->d_instances.p, s->instances.data(), sizeof(RcInstanceDesc) * n, hipMemcpyHostToDevice, s->stream));
    per_instance_pass(s, s->stream, n, true, false);
    tlas_chain(s, s->stream, scene_bufs(s, n, grid_for(n), s->tlas_ranges), n);
    read_root_aabb(s, s->tlas_nodes.p, true, s->root_min, s->root_max);
    s->state.world_bound_read();
}

// refit_tlas! (src/instanced-bvh.jl:2197-2222): new transforms -> leaf AABBs -> bottom-up refit, in place
// from_device: the descriptors in s->d_instances were rewritten on the device (rc_instance_buffer_device); keep them, optionally
// recompute their inverses there, and mark the host mirror stale instead of uploading it.
void rc_refit_tlas(rc_scene* s, bool from_device, bool recompute_inverse) {
    const uint32_t n = (uint32_t)s->instances.size();
    if (n == 0) return;
    if (from_device) {
        if (recompute_inverse) hipLaunchKernelGGL(k_update_inverses, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, s->d_instances.p, n);
        s->state.refit_from_device_begun();
    } else {
        RC_HIP(hipMemcpyAsync(s->d_instances.p, s->instances.data(), sizeof(RcInstanceDesc) * n, hipMemcpyHostToDevice, s->stream));
    }
    refit_chain(s, s->stream, scene_bufs(s, n, grid_for(n), s->tlas_ranges), n, true);
    read_root_aabb(s, s->tlas_nodes.p, true, s->root_min, s->root_max);
    s->state.world_bound_read();
}

// ---- the asynchronous update: everything on the caller's stream, nothing read back ------------------------------------------------------
static bool stream_capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
    return cs == hipStreamCaptureStatusActive;
}
static void note_async_mutation(rc_scene* s, hipStream_t st) {
    const bool capturing = stream_capturing(st);
    if (!capturing) s->async_stream = st;
    s->state.async_noted(capturing);
}

void rc_update_instances_async(rc_scene* s, uint32_t first, uint32_t m, const float* d_xforms, hipStream_t st) {
    const uint32_t n = (uint32_t)s->instances.size();
    if (m == 0) return;
    hipLaunchKernelGGL(k_update_instances, dim3(grid_for(m)), dim3(kBlock), 0, st, d_xforms, first, m, s->d_instances.p, (const RcBlasDesc*)s->d_descs.p,
                       (const uint32_t*)s->d_blas_nprims.p, (const uint32_t*)s->blas_cull_bits.p, (const uint32_t*)s->inst_leaf.p, s->inst_recs.p,
                       s->inst_cull.p, s->tlas_nodes.p, n);
    RC_HIP(hipGetLastError());
    s->state.instances_updated_async(stream_capturing(st));
    note_async_mutation(s, st);
}

// refit_tlas! on `st` without the root read-back.  per_instance: the descriptors were rewritten by the caller's own kernels
// (rc_instance_buffer_device), so the records, spheres and leaf boxes are derived from them first; after rc_update_instances_async they
// are already in place.
void rc_refit_tlas_async(rc_scene* s, bool per_instance, hipStream_t st) {
    const uint32_t n = (uint32_t)s->instances.size();
    if (n == 0) return;
    refit_chain(s, st, rebuild_bufs(s), n, per_instance);
    RC_HIP(hipGetLastError());
    s->state.tlas_committed_async(stream_capturing(st));
    note_async_mutation(s, st);
}

// rebuild_bvh! (src/instanced-bvh.jl:968-992, build_tlas_topology :1485-1594) on `st` from the descriptors the device holds, in place --
// same buffers, same addresses, so captured updates, refits and traces stay valid -- with the scratch reserved at sync time and without
// the root read-back.  per_instance as for rc_refit_tlas_async.
static RcTlasQuality* quality_block(rc_scene* s) { return reinterpret_cast<RcTlasQuality*>(s->quality.p); }
// The cost of the tree in s->tlas_nodes (n >= 1 leaves) as it is when the kernels run, committed in `mode` (quality_commit).  area: which of
// the two partial areas behind the block -- 0 the rebuild's, 1 rc_tlas_cost_async's, so that the two may run on different streams
static void cost_pass(rc_scene* s, hipStream_t st, uint32_t n, int area, double* out, double ratio, int mode, const uint32_t* gate) {
    double* partials = s->quality.p + kQualityStateWords + (size_t)area * kQualityMaxBlocks;
    const uint32_t nb = n >= 2 ? std::min(grid_for(n - 1), (unsigned)kQualityMaxBlocks) : 0u;
    if (nb) hipLaunchKernelGGL(k_tlas_cost_partials, dim3(nb), dim3(kCostBlock), 0, st, (const RcNode*)s->tlas_nodes.p, n, partials);
    hipLaunchKernelGGL(k_tlas_cost_fold, dim3(1), dim3(kCostBlock), 0, st, (const RcNode*)s->tlas_nodes.p, n, (const double*)partials, nb, out, quality_block(s),
                       ratio, mode, gate);
}
// The rebuild itself, on either device path.  mode < 0: what rc_rebuild_tlas_async always did.  kRecord / kArm: followed by the record step.
// kDecide: taken only if the tree in memory costs more than ratio x the baseline -- decided on the device, in front
static void rebuild_launch(rc_scene* s, hipStream_t st, uint32_t n, int mode, double ratio) {
    if (s->opt.tlas_rebuild_fused && n >= 2 && n <= (uint32_t)kFusedInst && s->tlas_top_k == 0) {
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(1), dim3(kFusedInst), 0, st, (const RcInstanceDesc*)s->d_instances.p, (const RcBlasDesc*)s->d_descs.p, n, s->tlas_nodes.p,
                               s->flat_nodes.p + s->n_flat_nodes, s->tlas_ranges.p, s->inst_leaf.p, (const float4*)s->inst_cull.p, quality_block(s), ratio, mode);
        };
        if (mode < 0) launch(k_rebuild_tlas_fused<false>); else launch(k_rebuild_tlas_fused<true>);
        return;
    }
    const uint32_t* gate = nullptr;
    if (mode == kDecide) {
        cost_pass(s, st, n, 0, nullptr, ratio, kDecide, nullptr);
        if (n < 2) return;  // (a single leaf: cost 1, never rebuilt)
        gate = &quality_block(s)->gate;  // written by the kernel above, read by the ones below: a kernel boundary on one stream
    }
    tlas_chain(s, st, rebuild_bufs(s), n, gate);
    if (mode >= 0) cost_pass(s, st, n, 0, nullptr, ratio, mode == kDecide ? (int)kRecord : mode, gate);
}
static void after_async_commit(rc_scene* s, hipStream_t st) {
    RC_HIP(hipGetLastError());
    s->state.tlas_committed_async(stream_capturing(st));
    note_async_mutation(s, st);
}
void rc_rebuild_tlas_async(rc_scene* s, bool per_instance, hipStream_t st) {
    const uint32_t n = (uint32_t)s->instances.size();
    if (n == 0) return;
    if (s->rebuild.n != n) throw RcError(4, "rebuild scratch does not match the instance count");  // (reserved by every rebuilding rc_sync)
    if (per_instance) per_instance_pass(s, st, n, true, false);
    rebuild_launch(s, st, n, s->state.quality_is_armed() ? (int)kRecord : -1, 0.0);  // (armed: the baseline follows explicit rebuilds)
    after_async_commit(s, st);
}

// rc_refit_tlas_async, then the rebuild above if the refitted tree has degraded: cost > ratio x cost_built, evaluated and acted on by the
// device (RcTlasQuality, rc_internal.h).  The first call after a rebuilding rc_sync arms the block: the host cannot know what an earlier
// sequence of refits left, so it enqueues refit -> unconditional rebuild -> record, eagerly.
void rc_refit_or_rebuild_tlas_async(rc_scene* s, bool per_instance, double ratio, hipStream_t st) {
    const uint32_t n = (uint32_t)s->instances.size();
    if (n == 0) return;
    if (s->rebuild.n != n) throw RcError(4, "rebuild scratch does not match the instance count");
    if (!s->state.quality_is_armed() && stream_capturing(st))
        throw RcError(6, "the first rc_refit_or_rebuild_tlas_device_async after a rebuilding rc_sync records the tree's baseline cost and must run eagerly: call it once before capturing it");
    refit_chain(s, st, rebuild_bufs(s), n, per_instance);
    rebuild_launch(s, st, n, s->state.quality_is_armed() ? (int)kDecide : (int)kArm, ratio);
    s->state.quality_armed_now();
    after_async_commit(s, st);
}

void rc_tlas_cost_async(rc_scene* s, double* d_cost, hipStream_t st) {
    const uint32_t n = (uint32_t)s->instances.size();
    if (n == 0) return;
    cost_pass(s, st, n, 1, d_cost, 0.0, kCostOnly, nullptr);
    RC_HIP(hipGetLastError());
    if (!s->state.async_work_pending() || s->async_stream == st) note_async_mutation(s, st);  // no mutation, but rc_scene_destroy waits for it like one (a flag, no event; with work pending on another stream that stream stays the one waited for: the header's LIFETIME note)
}

void rc_tlas_quality_read(rc_scene* s, RcTlasQuality* out) {
    memset(out, 0, sizeof(*out));
    if (s->instances.empty() || !s->quality.p) return;
    rc_wait_async_mutations(s);
    rc_copy_now(out, s->quality.p, sizeof(*out), hipMemcpyDeviceToHost);
}

// Host wait for the EAGER asynchronous updates and refits enqueued so far.  Replays of a graph that captured them are the caller's to
// wait for (a graph can be launched on any stream): the readers below then re-read what the device holds.
void rc_wait_async_mutations(rc_scene* s) {
    if (!s->state.async_work_pending()) return;
    RC_HIP(hipSetDevice(s->device));
    if (stream_capturing(s->async_stream))
        throw RcError(6, "the scene was updated asynchronously on a stream that is now being captured: its host-side state (world bound, instance mirror) is stale and cannot be refreshed during the capture");
    if (hipStreamSynchronize(s->async_stream) != hipSuccess) {  // (the caller destroyed the stream: its work is waited for with the device's)
        (void)hipGetLastError();
        RC_HIP(hipDeviceSynchronize());
    }
    s->state.async_waited();
}

void rc_ensure_world_bound(rc_scene* s, hipStream_t for_stream) {
    if (!s->state.world_bound_needs_read()) return;
    std::lock_guard<std::mutex> lk(s->launch_mu);  // queries are re-entrant: one of them refreshes, the others find it done (callers take no launch guard before this)
    if (!s->state.world_bound_needs_read()) return;
    if (s->n_tlas_nodes == 0) { s->state.world_bound_read(); return; }
    if (for_stream && stream_capturing(for_stream))
        throw RcError(6, "stale world bound: the scene was refitted asynchronously (rc_refit_device_async) and this call lays its rays out from the world bound, which cannot be read back while the stream is being captured -- call rc_world_bound before the capture");
    RC_HIP(hipSetDevice(s->device));
    rc_wait_async_mutations(s);
    RcNode root;
    rc_copy_now(&root, s->tlas_nodes.p, sizeof(RcNode), hipMemcpyDeviceToHost);
    host_root_aabb(root, true, s->root_min, s->root_max);
    s->state.world_bound_read();
}

// ---- update!(tlas, handle, new_geometry) (src/instanced-bvh.jl:808-857) on the caller's stream: build_blas (:1376-1443) from a device soup,
// committed IN PLACE.  The chain runs over scratch of its own (s->deform), without a read-back, into
// a staged tree; the host cannot learn the valid-face count without waiting, so the chain runs with the BLAS's current count and the three
// kernels below -- the only ones that touch anything a trace, an export or a later sync reads -- first compare it with the count the
// filter found (deform_ok: the scan's last element + the last flag).  On a mismatch they write nothing but the sticky status word; the
// staged tree was then built over the wrong number of slots, which costs time and nothing else (every index stays inside the scratch).
namespace {

__device__ inline bool deform_ok(const uint32_t* flags, const uint32_t* pos, uint32_t n, uint32_t n_prims) {
    return pos[n - 1] + flags[n - 1] == n_prims;  // (n_prims >= 1: zero valid faces never match)
}

struct DeformCommit {
    const uint32_t *flags, *pos;  // the filter's flags and their exclusive scan, n entries
    uint32_t n, n_prims;
    const RcNode* new_nodes;      // staged tree (2 n_prims - 1) and Morton-sorted primitives
    const RcPrim* new_prims;
    const uint32_t *perm, *slot_face;  // sorted slot -> compacted slot -> source face (mesh only)
    RcNode *blas_nodes, *flat_nodes;   // the geometry's own arrays and its slices of the flat ones
    RcPrim *blas_prims, *flat_prims;
    uint32_t* src_face;           // mesh only
    float* flat_attrs;            // nullptr: the attribute array is not valid, leave it
    const float *normals, *uvs;   // per vertex, nullptr for a soup; normals = the NEW ones when the call brings some
    const uint32_t* indices;
    float* normals_keep;          // where new normals are kept for later structural syncs (nullptr: none given)
    uint32_t n_normal_words;
    const uint32_t* remap;        // breadth-first renumbering of the top (single-BLAS scenes), or nullptr
    RcBlasDesc* desc;
    uint32_t *cull_accum, *status;
};

// The commit of ONE BLAS: thread i copies node i into the geometry's own array and, packed (and renumbered), into the traversal copy;
// threads below n_prims also commit primitive i, its attributes and source face, and fold its share of the entry-cull radius -- about the
// centre of the NEW root box, which every thread derives from the staged root -- into one word (zeroed by the chain's memset); thread 0
// writes the root box into the device descriptor.
__global__ __launch_bounds__(kBlock) void k_deform_commit(DeformCommit c) {
    __shared__ uint32_t sh_max;
    const bool ok = deform_ok(c.flags, c.pos, c.n, c.n_prims);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, n_nodes = 2u * c.n_prims - 1u;
    if (!ok) {
        if (i == 0) atomicOr(c.status, 1u);
        return;  // (uniform: every thread of the grid reads the same two words)
    }
    if (threadIdx.x == 0) sh_max = 0u;
    __syncthreads();
    float rmin[3], rmax[3];
    host_root_aabb(c.new_nodes[0], false, rmin, rmax);
    if (i < n_nodes) {
        const RcNode nd = c.new_nodes[i];
        c.blas_nodes[i] = nd;
        pack_node_renumbered(nd, i, c.n_prims, c.remap, nullptr, c.flat_nodes);
    }
    if (i < c.n_prims) {
        const RcPrim p = c.new_prims[i];
        c.blas_prims[i] = p;
        c.flat_prims[i] = p;
        uint32_t face = 0u;
        if (c.src_face) { face = c.slot_face[c.perm[i]]; c.src_face[i] = face; }
        if (c.flat_attrs) fill_attrs_one(p, c.normals, c.uvs, c.indices, face, c.flat_attrs + 15 * (size_t)i);
        atomicMax(&sh_max, cull_radius_bits(p.v, rmin, rmax));
    }
    if (c.normals_keep)
        for (uint32_t w = i; w < c.n_normal_words; w += gridDim.x * blockDim.x) c.normals_keep[w] = c.normals[w];
    if (i == 0) {
        for (int k = 0; k < 3; ++k) { c.desc->root_min[k] = rmin[k]; c.desc->root_max[k] = rmax[k]; }
    }
    __syncthreads();
    if (threadIdx.x == 0 && blockIdx.x * blockDim.x < c.n_prims) atomicMax(c.cull_accum, sh_max);
}

// What k_inst_recs and k_tlas_leaves derive from a BLAS's descriptor and cull radius, for the instances of ONE BLAS (through whichever
// handle): traversal record, entry-cull sphere, TLAS leaf box.  Thread 0 also publishes the radius the commit folded.
__global__ void k_deform_instances(const uint32_t* flags, const uint32_t* pos, uint32_t n_faces, uint32_t n_prims, uint32_t blas_index,
                                   const RcInstanceDesc* inst, const RcBlasDesc* descs, const uint32_t* blas_nprims, const uint32_t* cull_accum,
                                   uint32_t* blas_cull_bits, const uint32_t* leaf_of, RcInstRec* recs, float4* cull_out, RcNode* nodes, uint32_t n) {
    if (!deform_ok(flags, pos, n_faces, n_prims)) return;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t r_bits = *cull_accum;
    if (i == 0) blas_cull_bits[blas_index - 1] = r_bits;
    if (i >= n) return;
    const RcInstanceDesc& in = inst[i];
    if (in.blas_index != blas_index) return;
    const RcBlasDesc bd = descs[blas_index - 1];
    const RcInstRec r = inst_rec_of(in.inv_transform, blas_index, in.instance_id, bd, blas_nprims);
    recs[i] = r;
    float4 c0, c1;
    entry_cull_sphere(in.inv_transform, bd, r.n_prims, r_bits, c0, c1);
    cull_out[2 * (size_t)i] = c0;
    cull_out[2 * (size_t)i + 1] = c1;
    float3_ mn, mx;
    tlas_leaf_box(in.transform, bd, mn, mx);
    RcNode* nd = &nodes[(n - 1 + leaf_of[i]) - 1];  // the box only: the rest of the leaf is topology (k_update_instances)
    nd->f[0] = mn.x; nd->f[1] = mn.y; nd->f[2] = mn.z; nd->f[3] = mx.x; nd->f[4] = mx.y; nd->f[5] = mx.z;
}

// metadata by source face out of the sorted primitives (the word k_expand_mesh gave each face when the mesh was added); faces the filter
// dropped keep the default the caller put there
__global__ void k_face_meta_of(const RcPrim* prims, const uint32_t* src_face, uint32_t n, uint32_t* face_meta) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) face_meta[src_face[j]] = prims[j].meta;
}

}  // namespace

void rc_update_geometry_async(rc_scene* s, uint32_t blas_idx, const float* d_verts, const uint32_t* d_meta, uint32_t n, const float* d_mesh_verts,
                              const float* d_mesh_normals, hipStream_t st) {
    Blas& b = s->blas[blas_idx];
    auto& D = s->deform;
    const uint32_t np = b.n_prims, cap_n = std::max(n, np);
    const bool mesh = d_mesh_verts != nullptr, capturing = stream_capturing(st);
    const bool renumber = s->blas_top_k > 0 && s->blas.size() == 1;
    // ---- scratch: grown by eager calls only
    auto need = [&](auto& buf, size_t count) {
        if (count <= buf.cap) return;
        if (capturing) throw RcError(1, "the scratch of the geometry update is too small for this call and cannot grow while the stream is being captured: run the call eagerly once first");
        buf.reserve(count);
    };
    need(D.flags, cap_n); need(D.pos, cap_n); need(D.compact, cap_n);
    if (mesh) { need(D.slot_face, cap_n); need(D.soup, 9 * (size_t)n); }
    need(D.keys_a, np); need(D.keys_b, np); need(D.vals_a, np); need(D.vals_b, np);
    need(D.enc, 8); need(D.partials, (size_t)blas_bounds_blocks(np) * 6); need(D.arrive, np);
    if (renumber) need(D.remap, np - 1);
    need(D.prims, np); need(D.nodes, 2 * (size_t)np - 1); need(D.ranges, topology_records(np));
    // word 0 of D.arrive: the cull radius k_deform_commit folds into, zeroed with the refit's arrival counters behind it
    ChainBufs bufs{D.keys_a.p, D.keys_b.p, D.vals_a.p, D.vals_b.p, D.partials.p, D.enc.p, D.arrive.p, D.arrive.p + 1, D.ranges.p,
                   nullptr, &D.tmp, 0, (int64_t)np >= s->opt.onesweep_min};
    if (!D.scan_bytes.count(n) || !D.sort_bytes.count(np)) {
        if (capturing) throw RcError(1, "the geometry update has not run eagerly with these counts yet: its scan / sort storage cannot be sized while the stream is being captured");
        size_t scan = 0, sort = 0;
        RC_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan, D.flags.p, D.pos.p, (int)n, st));
        sort_pairs(st, bufs, np, &sort);  // (size query + reserve, nothing enqueued)
        D.scan_bytes[n] = scan ? scan : 1;
        D.sort_bytes[np] = sort;
    }
    const size_t scan_bytes = D.scan_bytes[n];
    bufs.sort_bytes = D.sort_bytes[np];
    need(D.tmp, std::max(scan_bytes, bufs.sort_bytes));
    if (mesh && b.m_face_meta.cap < b.n_mesh_faces) {
        // a scene loaded from a file carries no per-face metadata: recovered from the surviving primitives through the face map (faces the
        // filter had dropped get the default, their index)
        if (capturing) throw RcError(1, "the first rc_update_mesh_vertices_device_async of a loaded geometry recovers its per-face metadata and cannot be captured: run the call eagerly once first");
        b.m_face_meta.reserve(b.n_mesh_faces);
        hipLaunchKernelGGL(k_iota1, dim3(grid_for(b.n_mesh_faces)), dim3(kBlock), 0, st, b.m_face_meta.p, b.n_mesh_faces, (const uint32_t*)nullptr);
        hipLaunchKernelGGL(k_face_meta_of, dim3(grid_for(np)), dim3(kBlock), 0, st, (const RcPrim*)b.prims.p, (const uint32_t*)b.src_face.p, np, b.m_face_meta.p);
    }
    // ---- the filter over the n faces, then the build over np slots into the staged arrays
    if (mesh) {  // (the kernel's per-face metadata output is not needed -- the compaction reads m_face_meta itself -- and lands in D.pos, which the scan overwrites)
        hipLaunchKernelGGL(k_expand_mesh, dim3(grid_for(n)), dim3(kBlock), 0, st, d_mesh_verts, (const uint32_t*)b.m_indices.p, (const uint32_t*)nullptr, true, n, D.soup.p, D.pos.p);
        d_verts = D.soup.p;
        d_meta = b.m_face_meta.p;
    }
    ingest_chain(st, d_verts, d_meta, n, D.flags.p, D.pos.p, D.tmp.p, scan_bytes, D.compact.p, mesh ? D.slot_face.p : nullptr);
    blas_sort_chain(st, bufs, D.compact.p, np, D.prims.p);
    blas_tree_chain(st, bufs, D.prims.p, np, D.nodes.p);
    if (renumber) top_renumber(st, D.nodes.p, np, s->blas_top_k, D.remap.p);  // the renumbering follows the new topology (rc_build_tlas): staged too, the commit packs through it
    // ---- commit, then the instances of this BLAS
    const RcBlasDesc& hd = s->descs[blas_idx];
    DeformCommit c;
    c.flags = D.flags.p; c.pos = D.pos.p; c.n = n; c.n_prims = np;
    c.new_nodes = D.nodes.p; c.new_prims = D.prims.p; c.perm = D.vals_b.p; c.slot_face = D.slot_face.p;
    c.blas_nodes = b.nodes.p; c.flat_nodes = s->flat_nodes.p + hd.nodes_offset;
    c.blas_prims = b.prims.p; c.flat_prims = s->flat_prims.p + hd.primitives_offset;
    c.src_face = mesh ? b.src_face.p : nullptr;
    c.flat_attrs = s->state.flat_attrs_current() ? s->flat_attrs.p + 15 * (size_t)hd.primitives_offset : nullptr;
    c.normals = b.has_attrs ? (d_mesh_normals ? d_mesh_normals : b.m_normals.p) : nullptr;
    c.uvs = b.has_uvs ? b.m_uvs.p : nullptr;
    c.indices = b.m_indices.p;
    c.normals_keep = d_mesh_normals ? b.m_normals.p : nullptr;
    c.n_normal_words = 3 * b.n_mesh_verts;
    c.remap = renumber ? D.remap.p : nullptr;
    c.desc = s->d_descs.p + blas_idx;
    c.cull_accum = D.arrive.p;
    c.status = rc_geometry_status_word(s);
    hipLaunchKernelGGL(k_deform_commit, dim3(grid_for(2 * (uint64_t)np - 1)), dim3(kBlock), 0, st, c);
    const uint32_t ni = (uint32_t)s->instances.size();
    hipLaunchKernelGGL(k_deform_instances, dim3(grid_for(ni)), dim3(kBlock), 0, st, (const uint32_t*)D.flags.p, (const uint32_t*)D.pos.p, n, np, blas_idx + 1,
                       (const RcInstanceDesc*)s->d_instances.p, (const RcBlasDesc*)s->d_descs.p, (const uint32_t*)s->d_blas_nprims.p, (const uint32_t*)D.arrive.p,
                       s->blas_cull_bits.p, (const uint32_t*)s->inst_leaf.p, s->inst_recs.p, s->inst_cull.p, s->tlas_nodes.p, ni);
    RC_HIP(hipGetLastError());
    b.root_on_device = true;
    s->state.geometry_updated_async(capturing);
    note_async_mutation(s, st);
}

// The host copies of the root boxes an asynchronous geometry update left on the device (descs, Blas::root_min / root_max): read back for
// the geometries that were updated in place since, after a host wait for the eager updates.  While a graph that captured one may live, on
// every use.
void rc_ensure_blas_bounds(rc_scene* s) {
    if (!s->state.blas_bounds_need_read()) return;
    std::lock_guard<std::mutex> lk(s->launch_mu);  // exports are re-entrant: one of them refreshes, the others find it done (rc_ensure_world_bound)
    if (!s->state.blas_bounds_need_read()) return;
    RC_HIP(hipSetDevice(s->device));
    rc_wait_async_mutations(s);
    const size_t nb = std::min(s->descs.size(), s->blas.size());
    std::vector<RcBlasDesc> dev(nb);
    rc_copy_now(dev.data(), s->d_descs.p, sizeof(RcBlasDesc) * nb, hipMemcpyDeviceToHost);
    for (size_t i = 0; i < nb; ++i) {
        Blas& b = s->blas[i];
        if (!b.root_on_device) continue;  // (a geometry replaced on the host since holds the newer box)
        memcpy(b.root_min, dev[i].root_min, 12); memcpy(b.root_max, dev[i].root_max, 12);
        memcpy(s->descs[i].root_min, dev[i].root_min, 12); memcpy(s->descs[i].root_max, dev[i].root_max, 12);
        if (!s->state.deform_captured()) b.root_on_device = false;
    }
    s->state.blas_bounds_read();
}
