// swr_raycast.hip.h -- Physics.Raycast on the GPU: batched ray queries against retained meshes.
//
// Reference (file:line under the C# repo):
//   Physics.Raycast             Physics.cs:19-52    world vertices / normals of the whole mesh, per call
//   Physics.RaycastInternal     :54-134             Parallel.For over the triangles, nearest hit under strict '<'
//   Physics.RayIntersectsTriangle  :136-179         Moeller-Trumbore with the face mask
// The reference's Parallel.For keeps the first of equally distant hits of whatever partition finishes first; the serial
// one-partition schedule is reproduced: the smallest distance under float '<' among distances below float.MaxValue, the LOWEST
// triangle index on ties (-0.0 and +0.0 tie), the winner's own distance word returned.
//
//   k_ray_cast    one lane per triangle of one target, 32 rays per block: the lane transforms its three vertices once, keeps
//                 v0 / edge1 / edge2 in registers and walks the rays, which are uniform across the wave; a hitting lane does one
//                 64-bit atomicMin on best[ray * n_targets + target] with the key (distance bits, +-0 -> 0) << 32 | triangle
//   k_ray_finish  one lane per (ray, target) pair -- or, NEAREST, per ray, folding its targets in order under strict '<' --:
//                 recomputes the winning triangle through the same ray_triangle (the same distance bits, -0.0 included), adds
//                 normal and point, and puts the pair's key back to "nothing" for the next call
// No LDS, no inline assembly; nothing here is shared with the render kernels but the helpers of swr_device.h.
#pragma once
#include "swr_device.h"

#define SWR_RAY_BLOCK 256                 // triangles per k_ray_cast block
#define SWR_RAY_CHUNK 32                  // rays per k_ray_cast block (<= 64: one lane of every wave normalises one direction)
#define SWR_RAY_NO_HIT 0xffffffffffffffffull
#define SWR_FLOAT_MAXVALUE 3.40282347e+38f    // float.MaxValue, Physics.cs:65,72

namespace swr {

struct RayTarget {                        // one swr_ray_target as the kernels read it
    const swr_vertex* verts;
    const uint16_t* idx;
    uint32_t n_tris, pad;
    float model[16];
    float normal_matrix[16];              // Transpose(Invert(model)), the caller's (Physics.cs:30-38)
};
static_assert(sizeof(RayTarget) == 152, "RayTarget is uploaded as an array");
static_assert(sizeof(swr_ray) == 24 && sizeof(swr_ray_hit) == 40 && sizeof(swr_ray_target) == 136, "ABI sizes of include/swr.h");

// Vector3.Normalize(v) = v / v.Length()
__device__ __forceinline__ void normalize3(const float v[3], float out[3]) {
    const float len = sqrtf(dot3(v[0], v[1], v[2], v[0], v[1], v[2]));
    out[0] = v[0] / len; out[1] = v[1] / len; out[2] = v[2] / len;
}

// transformedVertices[i] = Vector3.Transform(vert.Position, model), Physics.cs:46
__device__ __forceinline__ void ray_world_vertex(const swr_vertex* __restrict__ v, const float* __restrict__ model, bool fma_t, float out[3]) {
    const float p[4] = { v->position[0], v->position[1], v->position[2], 1.0f };
    float w[4];
    vec4_transform(p, model, w, fma_t);
    out[0] = w[0]; out[1] = w[1]; out[2] = w[2];
}
// transformedNormals[i] = Normalize(Vector4.Transform((normal, 0), normalMatrix).xyz), :47-48 (the 0 x row4 term is kept)
__device__ __forceinline__ void ray_world_normal(const swr_vertex* __restrict__ v, const float* __restrict__ nmat, bool fma_t, float out[3]) {
    const float n[4] = { v->normal[0], v->normal[1], v->normal[2], 0.0f };
    float w[4];
    vec4_transform(n, nmat, w, fma_t);
    normalize3(w, out);
}

// RayIntersectsTriangle, Physics.cs:136-179 (e1 = v1 - v0, e2 = v2 - v0), followed by RaycastInternal's `if (distance < 0)` (:93).
// Every comparison keeps the reference's sense, so a NaN falls through exactly where it does in C#.
template <bool FUSED>
__device__ __forceinline__ bool ray_triangle(const float o[3], const float d[3], const float v0[3], const float e1[3], const float e2[3],
                                             uint32_t mask, float& distance, float& u, float& v) {
    const float eps = 1e-8f;
    float pvec[3], qvec[3];
    cross3<FUSED>(d, e2, pvec);                                                     // :153
    const float det = dot3(e1[0], e1[1], e1[2], pvec[0], pvec[1], pvec[2]);         // :154
    if ((mask & SWR_RAY_IGNORE_BACKFACES) && det < eps) return false;               // :160
    if ((mask & SWR_RAY_IGNORE_FRONTFACES) && det > -eps) return false;             // :161
    if (fabsf(det) < eps) return false;                                             // :162
    const float inv_det = 1.0f / det;                                               // :164
    const float tvec[3] = { o[0] - v0[0], o[1] - v0[1], o[2] - v0[2] };             // :165
    u = dot3(tvec[0], tvec[1], tvec[2], pvec[0], pvec[1], pvec[2]) * inv_det;       // :167
    if (u < 0.0f || u > 1.0f) return false;                                         // :168
    cross3<FUSED>(tvec, e1, qvec);                                                  // :170
    v = dot3(d[0], d[1], d[2], qvec[0], qvec[1], qvec[2]) * inv_det;                // :171
    if (v < 0.0f || u + v > 1.0f) return false;                                     // :172
    distance = dot3(e2[0], e2[1], e2[2], qvec[0], qvec[1], qvec[2]) * inv_det;      // :174
    if (distance < 0.0f) return false;                                              // :175 (and :93)
    return true;
}

// the three world vertices of triangle `tri` as v0, edge1, edge2 (:86-88, :151-152)
__device__ __forceinline__ void ray_triangle_edges(const RayTarget& t, uint32_t tri, bool fma_t, float v0[3], float e1[3], float e2[3]) {
    float v1[3], v2[3];
    ray_world_vertex(t.verts + t.idx[3u * tri], t.model, fma_t, v0);
    ray_world_vertex(t.verts + t.idx[3u * tri + 1u], t.model, fma_t, v1);
    ray_world_vertex(t.verts + t.idx[3u * tri + 2u], t.model, fma_t, v2);
#pragma unroll
    for (int k = 0; k < 3; ++k) { e1[k] = v1[k] - v0[k]; e2[k] = v2[k] - v0[k]; }
}

// The order of `if (distance < local.Distance)` (:102,114) over triangles 0, 1, 2, ... as one unsigned word: distances that can win
// are +-0 or positive and below float.MaxValue, where the bit pattern orders as the value does once -0.0 is mapped to +0.0; the
// lower triangle index breaks ties.  NaN, +Inf and MaxValue itself fail `distance < MaxValue` and have no key.
__device__ __forceinline__ unsigned long long ray_key(float distance, uint32_t tri) {
    if (!(distance < SWR_FLOAT_MAXVALUE)) return SWR_RAY_NO_HIT;
    const uint32_t b = __float_as_uint(distance);
    return ((unsigned long long)(b == 0x80000000u ? 0u : b) << 32) | (unsigned long long)tri;
}

// grid = (triangle blocks of the largest target, ray chunks, targets)
template <bool FUSED>
__global__ __launch_bounds__(SWR_RAY_BLOCK) void k_ray_cast(const swr_ray* __restrict__ rays, uint32_t n_rays, const RayTarget* __restrict__ targets,
                                                            uint32_t n_targets, uint32_t mask, uint32_t nm_flags,
                                                            unsigned long long* __restrict__ best) {
    const RayTarget& t = targets[blockIdx.z];
    const uint32_t n_tris = t.n_tris;
    if (blockIdx.x * SWR_RAY_BLOCK >= n_tris) return;                      // (uniform over the block; a mesh without triangles misses)
    const bool fma_t = (nm_flags & SWR_NM_TRANSFORM_FMA) != 0u;
    const uint32_t tri_raw = blockIdx.x * SWR_RAY_BLOCK + threadIdx.x;
    const bool live = tri_raw < n_tris;
    const uint32_t tri = live ? tri_raw : n_tris - 1u;                     // every lane stays in the loop: the rays are read lane to lane
    float v0[3], e1[3], e2[3];
    ray_triangle_edges(t, tri, fma_t, v0, e1, e2);
    // rayDirection = Normalize(rayDirection), :69 -- once per ray, not per triangle: lane l of every wave holds ray l of the chunk
    const uint32_t r0 = blockIdx.y * SWR_RAY_CHUNK;
    const uint32_t n_here = min((uint32_t)SWR_RAY_CHUNK, n_rays - r0);
    const uint32_t mine = r0 + min(threadIdx.x & 63u, n_here - 1u);
    const float my_o[3] = { rays[mine].origin[0], rays[mine].origin[1], rays[mine].origin[2] };
    const float my_raw[3] = { rays[mine].direction[0], rays[mine].direction[1], rays[mine].direction[2] };
    float my_d[3];
    normalize3(my_raw, my_d);
    for (uint32_t j = 0; j < n_here; ++j) {
        float o[3], d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_o[k]), (int)j));
            d[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_d[k]), (int)j));
        }
        float distance, u, v;
        if (ray_triangle<FUSED>(o, d, v0, e1, e2, mask, distance, u, v) && live) {
            const unsigned long long key = ray_key(distance, tri);
            if (key != SWR_RAY_NO_HIT) atomicMin(&best[(size_t)(r0 + j) * n_targets + blockIdx.z], key);
        }
    }
}

// the record of (ray, target) whose key is `key`: what Physics.Raycast returns, and the winning triangle (build-defined)
template <bool FUSED>
__device__ __forceinline__ void ray_record(const swr_ray& ray, const RayTarget& t, int target, unsigned long long key, uint32_t mask, bool fma_t,
                                           swr_ray_hit* __restrict__ out) {
    swr_ray_hit h;
    h.found = 0; h.target = target; h.triangle = -1;
    h.distance = SWR_FLOAT_MAXVALUE;                                        // :65-67
    h.point[0] = h.point[1] = h.point[2] = 0.0f;
    h.normal[0] = h.normal[1] = h.normal[2] = 0.0f;
    if (key != SWR_RAY_NO_HIT) {
        const uint32_t tri = (uint32_t)key;
        const float o[3] = { ray.origin[0], ray.origin[1], ray.origin[2] };
        const float raw[3] = { ray.direction[0], ray.direction[1], ray.direction[2] };
        float d[3], v0[3], e1[3], e2[3];
        normalize3(raw, d);
        ray_triangle_edges(t, tri, fma_t, v0, e1, e2);
        float distance = 0.0f, u = 0.0f, v = 0.0f;
        (void)ray_triangle<FUSED>(o, d, v0, e1, e2, mask, distance, u, v);  // (the hit k_ray_cast found: the same code on the same operands)
        const float b[3] = { (1.0f - u) - v, u, v };                        // :177
        float n0[3], n1[3], n2[3], ni[3], nn[3];
        ray_world_normal(t.verts + t.idx[3u * tri], t.normal_matrix, fma_t, n0);
        ray_world_normal(t.verts + t.idx[3u * tri + 1u], t.normal_matrix, fma_t, n1);
        ray_world_normal(t.verts + t.idx[3u * tri + 2u], t.normal_matrix, fma_t, n2);
#pragma unroll
        for (int k = 0; k < 3; ++k) {                                       // n0 * bary.X + n1 * bary.Y + n2 * bary.Z, :99
            const float a0 = n0[k] * b[0], a1 = n1[k] * b[1], a2 = n2[k] * b[2];
            ni[k] = (a0 + a1) + a2;
        }
        normalize3(ni, nn);
        h.found = 1; h.triangle = (int32_t)tri; h.distance = distance;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float s = d[k] * distance;                                // rayOrigin + rayDirection * distance, :100
            h.point[k] = o[k] + s;
            h.normal[k] = nn[k];
        }
    }
    *out = h;
}

// NEAREST = false: one lane per pair, out[pair].  NEAREST = true: one lane per ray, out[ray] = the fold of its pairs in target order
// under `if (hit && distance < best)` from "not found" (the callers' lock blocks, CharacterController.cs:260-301,308-389): the first
// of equally near targets wins; a ray that misses everything gives the miss record with target -1.
template <bool FUSED, bool NEAREST>
__global__ __launch_bounds__(64) void k_ray_finish(const swr_ray* __restrict__ rays, uint32_t n_rays, const RayTarget* __restrict__ targets,
                                                   uint32_t n_targets, uint32_t mask, uint32_t nm_flags,
                                                   unsigned long long* __restrict__ best, swr_ray_hit* __restrict__ out) {
    const bool fma_t = (nm_flags & SWR_NM_TRANSFORM_FMA) != 0u;
    const size_t i = (size_t)blockIdx.x * 64u + threadIdx.x;
    if (NEAREST) {
        if (i >= n_rays) return;
        unsigned long long win = SWR_RAY_NO_HIT;
        uint32_t win_t = 0u;
        for (uint32_t t = 0; t < n_targets; ++t) {
            const unsigned long long key = best[i * n_targets + t];
            best[i * n_targets + t] = SWR_RAY_NO_HIT;
            // (keys order as their distances do; equal distances -- +-0 included -- keep the earlier target: strict '<')
            if (key != SWR_RAY_NO_HIT && (win == SWR_RAY_NO_HIT || (uint32_t)(key >> 32) < (uint32_t)(win >> 32))) { win = key; win_t = t; }
        }
        ray_record<FUSED>(rays[i], targets[win_t], win == SWR_RAY_NO_HIT ? -1 : (int)win_t, win, mask, fma_t, out + i);
    } else {
        if (i >= (size_t)n_rays * n_targets) return;
        const uint32_t r = (uint32_t)(i / n_targets), t = (uint32_t)(i - (size_t)r * n_targets);
        const unsigned long long key = best[i];
        best[i] = SWR_RAY_NO_HIT;
        ray_record<FUSED>(rays[r], targets[t], (int)t, key, mask, fma_t, out + i);
    }
}

}  // namespace swr
