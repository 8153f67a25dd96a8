// swr_mesh_deform.hip.h -- deforming a retained mesh on the GPU: a blend of two key frames and linear-blend
// skinning by a joint palette.  Both write the swr_vertex array a retained mesh holds (what make_mesh uploads), so every reader of a
// mesh -- the vertex stage, the ray queries, the bounding sphere -- sees the pose.  No kernel of the frame is touched.
//
// What is restated (file:line under the C# repo) and what is build-defined:
//   key frames       Model.AnimationFrames / PlayAnimation, ModelLoader.cs:79-115,331-348: the reference swaps whole frames; the blend
//                    between two of them is this library's, in its Lerp model (nm_lerp: Shaders.Lerp's a*(1-t) + b*t, fused or not as
//                    the build's SWR_NUMERICS_FMA says)
//   skinning         build-defined (the reference has none), in the System.Numerics model of swr_device.h: Vector3.Transform and
//                    Vector3.TransformNormal per influence under the context's two flags (swr_set_transform_fma), the weighted sum in
//                    the accumulation shape of vec4_transform_t, Vector3.Normalize as normalize3 (swr_raycast.hip.h: v / v.Length(), dot3
//                    in the build's order -- the expression k_vertex applies to the world normal)
//
// A record is 48 bytes = three 16-byte words, and hipMalloc's alignment makes every record 16-byte aligned.
//   k_mesh_blend     lerps all twelve scalars alike, so it never looks at a record: one thread per 16-byte WORD of the array, consecutive
//                    lanes on consecutive words (three fully coalesced streams, no LDS)
//   k_mesh_skin      needs the whole record per lane: one thread per vertex, each lane loading and storing its own three words, 48
//                    bytes from its neighbour's -- three partial touches of every line, which stays in the vector cache between
//                    them.  The other mapping -- a wave's 64 records in three loads of 1 KB each, handed out through an LDS slab as
//                    k_vertex does -- was built and measured at 65,535 vertices and at a few hundred: the same time within the
//                    spread (profiles/r23_mesh_deform.md), for 6 KB of LDS per block and 80 more instructions.  LDS is what a
//                    front-stream kernel competes for beside a raster kernel (SWR_FRONT_MAX_LDS), so it is not kept
// The palette is read from global memory by joint index (64 bytes per influence, 16-byte loads): 16 players' palettes are a few KB and
// stay in the caches; a copy in LDS would cost LDS for nothing at these sizes.
#pragma once
#include "swr_device.h"
#include "swr_raycast.hip.h"      // normalize3

#define SWR_DEFORM_BLOCK 128      // threads per block: 128 words of k_mesh_blend, 128 vertices of k_mesh_skin

namespace swr {

static_assert(sizeof(swr_vertex) == 48, "a record is three 16-byte words");

// dst = nm_lerp(a, b, t) for every scalar of every record; n_words = 3 x vertices.  dst aliases neither source (the host refuses it).
__global__ __launch_bounds__(SWR_DEFORM_BLOCK) void k_mesh_blend(const float4* __restrict__ a, const float4* __restrict__ b,
                                                                 float4* __restrict__ dst, uint32_t n_words, float t) {
    SWR_FRONT_ENTER();
    const uint32_t i = blockIdx.x * (uint32_t)SWR_DEFORM_BLOCK + threadIdx.x;
    if (i >= n_words) return;
    const float4 x = a[i], y = b[i];
    dst[i] = make_float4(nm_lerp(x.x, y.x, t), nm_lerp(x.y, y.y, t), nm_lerp(x.z, y.z, t), nm_lerp(x.w, y.w, t));
}

// r = w * v (rounded) for the first influence, r = nm_madd<fused>(w, v, r) for the others: vec4_transform_t's accumulation
__device__ __forceinline__ float skin_accumulate(int k, float w, float v, float r, bool fused) {
    if (k == 0) return w * v;
    return fused ? nm_madd<true>(w, v, r) : nm_madd<false>(w, v, r);
}

// One vertex: position and normal through the four joint matrices, summed by weight, the normal normalised; uv and colour as they are.
// All four influences are evaluated: a zero weight is multiplied (0 x Inf = NaN is the defined result), weights are used as given.
__device__ __forceinline__ void skin_vertex(float4& q0, float4& q1, ushort4 j, float4 w, const float* __restrict__ palette, uint32_t nm_flags) {
    const bool fma_t = (nm_flags & SWR_NM_TRANSFORM_FMA) != 0u, fma_tn = (nm_flags & SWR_NM_TRANSFORM_NORMAL_FMA) != 0u;
    const float p[4] = { q0.x, q0.y, q0.z, 1.0f }, n[3] = { q1.y, q1.z, q1.w };
    const uint32_t joint[4] = { j.x, j.y, j.z, j.w };
    const float weight[4] = { w.x, w.y, w.z, w.w };
    float rp[3] = { 0.f, 0.f, 0.f }, rn[3] = { 0.f, 0.f, 0.f };
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // the joint's matrix in registers first: vec4_transform and vec3_transform_normal index it by component
        const float4* __restrict__ m4 = reinterpret_cast<const float4*>(palette + (size_t)joint[k] * 16u);
        const float4 r0 = m4[0], r1 = m4[1], r2 = m4[2], r3 = m4[3];
        const float m[16] = { r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w };
        float pk[4], nk[3];
        vec4_transform(p, m, pk, fma_t);                 // Vector3.Transform(position, M): x, y, z of Vector4.Transform((position, 1), M)
        vec3_transform_normal(n, m, nk, fma_tn);         // Vector3.TransformNormal(normal, M): the matrix's upper 3 x 3
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            rp[c] = skin_accumulate(k, weight[k], pk[c], rp[c], fma_t);
            rn[c] = skin_accumulate(k, weight[k], nk[c], rn[c], fma_tn);
        }
    }
    float un[3];
    normalize3(rn, un);
    q0.x = rp[0]; q0.y = rp[1]; q0.z = rp[2];
    q1.y = un[0]; q1.z = un[1]; q1.w = un[2];
}

// dst[v] = skin(src[v]) for v < n_verts; joints / weights: four per vertex, every joint index below the palette's count (the host checked)
__global__ __launch_bounds__(SWR_DEFORM_BLOCK) void k_mesh_skin(const swr_vertex* __restrict__ src, const ushort4* __restrict__ joints,
                                                                const float4* __restrict__ weights, const float* __restrict__ palette,
                                                                swr_vertex* __restrict__ dst, uint32_t n_verts, uint32_t nm_flags) {
    SWR_FRONT_ENTER();
    const uint32_t v = blockIdx.x * (uint32_t)SWR_DEFORM_BLOCK + threadIdx.x;
    if (v >= n_verts) return;
    const float4* __restrict__ in = reinterpret_cast<const float4*>(src + v);
    float4 q0 = in[0], q1 = in[1];                                  // pos.xyz uv.x | uv.y normal.xyz
    const float4 q2 = in[2];                                        // colour
    skin_vertex(q0, q1, joints[v], weights[v], palette, nm_flags);
    float4* out = reinterpret_cast<float4*>(dst + v);
    out[0] = q0; out[1] = q1; out[2] = q2;
}

}  // namespace swr
