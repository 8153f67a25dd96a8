// swr_animation.hip.h -- skeletal animation on the GPU: clips sampled and joint hierarchies evaluated for a whole
// crowd in one launch, into a palette set that stays on the device; every mesh of the crowd skinned from that set in one launch.
//
// Everything here is build-defined (the reference has no skeletal animation) and has ONE definition for every numerics build and
// either Transform flag: plain float32, no fused multiply-add (csrc is compiled with -ffp-contract=off), sums left to right as
// written, true divisions and sqrtf.  Only the skinning itself follows the context's flags, because it is skin_vertex.
//   key search       !(t > T[0]) -> key 0; t >= T[n-1] -> key n-1; else k = the largest index with T[k] <= t (binary search), so
//                    T[k+1] > t and u = (t - T[k]) / (T[k+1] - T[k]) has a positive divisor even among duplicate times
//   LINEAR           a * (1 - u) + b * u per scalar (T, S); Quaternion.Lerp's scalar form (R): the normalised lerp, not a slerp
//   two clips        each path from either clip (the node's rest value where a clip has no channel), then the same two lerps at
//                    u = weight, unclamped
//   local            a node no channel of the request's clips targets keeps its rest matrix's words; a targeted one composes
//                    S x Matrix4x4.CreateFromQuaternion(R) x T: row i of the rotation times s_i, row 4 = (t, 1), column 4 = (0, 0, 0, 1)
//   hierarchy        world[i] = local[i] x world[parent[i]] with the parent's world FINISHED first (right-nested up the chain),
//                    Matrix4x4.Multiply's element order; palette[j] = inverse_bind[j] x world[node(j)]
//
//   k_pose_sample    one block of 256 threads (four waves) per instance.  Phase 1: threads stride over the nodes, search the keys,
//                    compose and store `local` into the set's node array in GLOBAL memory.  Phase 2: the levels of equal depth in
//                    order (the host sorted them, swr_skeleton_create), a block barrier between levels, each thread multiplying its
//                    node's local (in place) by its parent's finished world.  Phase 3: threads stride over the joints.  With the worlds
//                    in global memory the kernel needs no LDS and the node count is not bounded by it.
//   k_mesh_skin_batch one launch over all jobs of a call: a block of SWR_DEFORM_BLOCK vertices finds its job in a table of block
//                    prefix sums (binary search on wave-uniform values: scalar loads), then does what k_mesh_skin does through the same
//                    skin_vertex.
// Both run on the front stream beside a raster kernel: SWR_FRONT_ENTER first, no LDS, <= SWR_FRONT_MAX_VGPRS, <= 4 waves
// (tests/test_animation_budget.py).
#pragma once
#include "swr_device.h"
#include "swr_mesh_deform.hip.h"

#define SWR_POSE_BLOCK 256                 // threads per k_pose_sample block: four waves
#define SWR_ANIM_NO_CLIP 0xffffffffu       // PoseRequestDev::base_b of a request without a second clip

namespace swr {

// A skeleton as the kernels read it: one device blob, these pointers into it (swr_skeleton_create).
struct SkeletonDev {
    const int32_t* parent;                  // n_nodes: parent[i] < i, -1 for a root
    const int32_t* order;                   // n_nodes: the nodes sorted by depth (stable)
    const int32_t* level_start;             // n_levels + 1: order[level_start[l] .. level_start[l + 1]) is level l
    const float* rest_local;                // n_nodes x 16
    const float* rest_t;                    // n_nodes x 3
    const float* rest_r;                    // n_nodes x 4 (xyzw)
    const float* rest_s;                    // n_nodes x 3
    const int32_t* joint_node;              // n_joints
    const float* inverse_bind;              // n_joints x 16
    uint32_t n_nodes, n_joints, n_levels;
};

// A request as the host resolved it: word offsets of the clips' node tables in the clip blob.
struct PoseRequestDev { uint32_t base_a; float time_a; uint32_t base_b; float time_b; float weight; };
static_assert(sizeof(PoseRequestDev) == 20, "five words per request");

// One job of k_mesh_skin_batch (48 bytes).  first_block: the launch's first block of this job; jobs without vertices are not listed.
struct SkinJob {
    const swr_vertex* src; const ushort4* joints; const float4* weights; swr_vertex* dst;
    uint32_t n_verts, first_block, palette_offset, pad;      // palette_offset: floats from the set's first matrix to the instance's
};
static_assert(sizeof(SkinJob) == 48, "a job is three 16-byte words");

// The clip blob (32-bit words; word 0 is never a channel, so 0 means "no channel"):
//   clip    n_nodes x 3 words: the word offset of the channel on (node, path), or 0
//   channel interpolation, n_keys, n_keys key times, n_keys x (3 | 4) key values

// Quaternion.Lerp(a, b, u), scalar form
__device__ __forceinline__ void quaternion_lerp(const float* a, const float* b, float u, float* r) {
    const float u1 = 1.0f - u;
    const float dot = ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3];
    if (dot >= 0.0f) {
#pragma unroll
        for (int c = 0; c < 4; ++c) r[c] = u1 * a[c] + u * b[c];
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) r[c] = u1 * a[c] - u * b[c];
    }
    const float ls = ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3];
    const float inv = 1.0f / sqrtf(ls);
#pragma unroll
    for (int c = 0; c < 4; ++c) r[c] *= inv;
}

template <int N> __device__ __forceinline__ void anim_lerp(const float* a, const float* b, float u, float* r) {
    if (N == 4) { quaternion_lerp(a, b, u, r); return; }
    const float u1 = 1.0f - u;
#pragma unroll
    for (int c = 0; c < N; ++c) r[c] = a[c] * u1 + b[c] * u;
}

// One channel (N = 3: T or S, N = 4: R) at time t.
template <int N> __device__ __forceinline__ void sample_channel(const uint32_t* __restrict__ ch, float t, float* out) {
    const uint32_t interpolation = ch[0], n = ch[1];
    const float* __restrict__ T = reinterpret_cast<const float*>(ch + 2);
    const float* __restrict__ V = T + n;
    uint32_t k;
    bool between = false;
    if (!(t > T[0])) k = 0u;                        // (a NaN t lands here)
    else if (t >= T[n - 1u]) k = n - 1u;
    else {
        uint32_t lo = 0u, hi = n - 1u;              // T[lo] <= t < T[hi]
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (T[mid] <= t) lo = mid; else hi = mid;
        }
        k = lo;
        between = interpolation == SWR_ANIM_LINEAR;
    }
    float a[N];
#pragma unroll
    for (int c = 0; c < N; ++c) a[c] = V[(size_t)k * N + c];
    if (!between) {
#pragma unroll
        for (int c = 0; c < N; ++c) out[c] = a[c];
        return;
    }
    float b[N];
#pragma unroll
    for (int c = 0; c < N; ++c) b[c] = V[(size_t)(k + 1u) * N + c];
    const float u = (t - T[k]) / (T[k + 1u] - T[k]);
    anim_lerp<N>(a, b, u, out);
}

// One path of one node under a request: the clip's channel, or the rest value; two clips combined at the weight.
template <int N> __device__ __forceinline__ void sample_path(const uint32_t* __restrict__ clips, uint32_t ch_a, uint32_t ch_b, bool two,
                                                             const PoseRequestDev& rq, const float* __restrict__ rest, float* out) {
    float a[N];
    if (ch_a) sample_channel<N>(clips + ch_a, rq.time_a, a);
    else {
#pragma unroll
        for (int c = 0; c < N; ++c) a[c] = rest[c];
    }
    if (!two) {
#pragma unroll
        for (int c = 0; c < N; ++c) out[c] = a[c];
        return;
    }
    float b[N];
    if (ch_b) sample_channel<N>(clips + ch_b, rq.time_b, b);
    else {
#pragma unroll
        for (int c = 0; c < N; ++c) b[c] = rest[c];
    }
    anim_lerp<N>(a, b, rq.weight, out);
}

// S x Matrix4x4.CreateFromQuaternion(R) x T, row-major for row vectors, stored as four 16-byte words
__device__ __forceinline__ void compose_trs(const float* t, const float* q, const float* s, float4* __restrict__ out) {
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    const float xx = x * x, yy = y * y, zz = z * z;
    const float xy = x * y, wz = z * w, xz = z * x, wy = y * w, yz = y * z, wx = x * w;
    const float m11 = 1.0f - 2.0f * (yy + zz), m12 = 2.0f * (xy + wz), m13 = 2.0f * (xz - wy);
    const float m21 = 2.0f * (xy - wz), m22 = 1.0f - 2.0f * (zz + xx), m23 = 2.0f * (yz + wx);
    const float m31 = 2.0f * (xz + wy), m32 = 2.0f * (yz - wx), m33 = 1.0f - 2.0f * (yy + xx);
    out[0] = make_float4(m11 * s[0], m12 * s[0], m13 * s[0], 0.0f);
    out[1] = make_float4(m21 * s[1], m22 * s[1], m23 * s[1], 0.0f);
    out[2] = make_float4(m31 * s[2], m32 * s[2], m33 * s[2], 0.0f);
    out[3] = make_float4(t[0], t[1], t[2], 1.0f);
}

// Matrix4x4.Multiply: one row of a x b, element j = ((a1 b_1j + a2 b_2j) + a3 b_3j) + a4 b_4j
__device__ __forceinline__ float4 mul_row(const float4 a, const float4 b0, const float4 b1, const float4 b2, const float4 b3) {
    return make_float4(((a.x * b0.x + a.y * b1.x) + a.z * b2.x) + a.w * b3.x, ((a.x * b0.y + a.y * b1.y) + a.z * b2.y) + a.w * b3.y,
                       ((a.x * b0.z + a.y * b1.z) + a.z * b2.z) + a.w * b3.z, ((a.x * b0.w + a.y * b1.w) + a.z * b2.w) + a.w * b3.w);
}
// out = a x b (out may be a)
__device__ __forceinline__ void mul_4x4(const float4* a, const float4* b, float4* out) {
    const float4 b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
    const float4 a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
    out[0] = mul_row(a0, b0, b1, b2, b3); out[1] = mul_row(a1, b0, b1, b2, b3);
    out[2] = mul_row(a2, b0, b1, b2, b3); out[3] = mul_row(a3, b0, b1, b2, b3);
}

// Instance blockIdx.x of a pose set: palettes[instance] from requests[instance].  worlds: n_instances x n_nodes matrices of the set
// (scratch that only this kernel touches; one block owns one instance's slice).  palette_stride: floats per instance.
__global__ __launch_bounds__(SWR_POSE_BLOCK) void k_pose_sample(SkeletonDev sk, const uint32_t* __restrict__ clips,
                                                                const PoseRequestDev* __restrict__ requests, float4* worlds,
                                                                float4* __restrict__ palettes, uint32_t palette_stride) {
    SWR_FRONT_ENTER();
    const uint32_t inst = blockIdx.x;
    const PoseRequestDev rq = requests[inst];
    const bool two = rq.base_b != SWR_ANIM_NO_CLIP;
    float4* world = worlds + (size_t)inst * sk.n_nodes * 4u;
    const float4* __restrict__ rest_local = reinterpret_cast<const float4*>(sk.rest_local);

    // phase 1: local matrices
    for (uint32_t i = threadIdx.x; i < sk.n_nodes; i += SWR_POSE_BLOCK) {
        const uint32_t* __restrict__ ta = clips + rq.base_a + 3u * i;
        const uint32_t at = ta[0], ar = ta[1], as = ta[2];
        uint32_t bt = 0u, br = 0u, bs = 0u;
        if (two) { const uint32_t* __restrict__ tb = clips + rq.base_b + 3u * i; bt = tb[0]; br = tb[1]; bs = tb[2]; }
        float4* out = world + 4u * (size_t)i;
        if ((at | ar | as | bt | br | bs) == 0u) {      // untargeted: the rest matrix's words
            const float4* __restrict__ r = rest_local + 4u * (size_t)i;
            out[0] = r[0]; out[1] = r[1]; out[2] = r[2]; out[3] = r[3];
            continue;
        }
        float t[3], q[4], s[3];
        sample_path<3>(clips, at, bt, two, rq, sk.rest_t + 3u * (size_t)i, t);
        sample_path<4>(clips, ar, br, two, rq, sk.rest_r + 4u * (size_t)i, q);
        sample_path<3>(clips, as, bs, two, rq, sk.rest_s + 3u * (size_t)i, s);
        compose_trs(t, q, s, out);
    }
    // phase 2: level by level, the parents' worlds finished and visible to the block before their children read them (level 0 holds
    // the roots, whose world is their local)
    for (uint32_t l = 1u; l < sk.n_levels; ++l) {
        __threadfence_block();
        __syncthreads();
        const uint32_t lo = (uint32_t)sk.level_start[l], hi = (uint32_t)sk.level_start[l + 1u];
        for (uint32_t k = lo + threadIdx.x; k < hi; k += SWR_POSE_BLOCK) {
            const uint32_t i = (uint32_t)sk.order[k];
            const uint32_t p = (uint32_t)sk.parent[i];
            mul_4x4(world + 4u * (size_t)i, world + 4u * (size_t)p, world + 4u * (size_t)i);
        }
    }
    __threadfence_block();
    __syncthreads();
    // phase 3: the palette
    const float4* __restrict__ ib = reinterpret_cast<const float4*>(sk.inverse_bind);
    float4* pal = palettes + (size_t)inst * (palette_stride / 4u);
    for (uint32_t j = threadIdx.x; j < sk.n_joints; j += SWR_POSE_BLOCK) {
        const uint32_t node = (uint32_t)sk.joint_node[j];
        float4 m[4];
        mul_4x4(ib + 4u * (size_t)j, world + 4u * (size_t)node, m);
        float4* out = pal + 4u * (size_t)j;
        out[0] = m[0]; out[1] = m[1]; out[2] = m[2]; out[3] = m[3];
    }
}

// dst_k[v] = skin(src_k[v]) by the palette of job k's instance, for every job of the table; grid = the jobs' blocks, summed
__global__ __launch_bounds__(SWR_DEFORM_BLOCK) void k_mesh_skin_batch(const SkinJob* __restrict__ jobs, uint32_t n_jobs,
                                                                      const float* __restrict__ palettes, uint32_t nm_flags) {
    SWR_FRONT_ENTER();
    const uint32_t b = blockIdx.x;
    uint32_t lo = 0u, hi = n_jobs;                  // jobs[lo].first_block <= b < jobs[hi].first_block (jobs[0].first_block = 0)
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (jobs[mid].first_block <= b) lo = mid; else hi = mid;
    }
    const SkinJob job = jobs[lo];
    const uint32_t v = (b - job.first_block) * (uint32_t)SWR_DEFORM_BLOCK + threadIdx.x;
    if (v >= job.n_verts) return;
    const float4* __restrict__ in = reinterpret_cast<const float4*>(job.src + v);
    float4 q0 = in[0], q1 = in[1];                                  // pos.xyz uv.x | uv.y normal.xyz
    const float4 q2 = in[2];                                        // colour
    skin_vertex(q0, q1, job.joints[v], job.weights[v], palettes + job.palette_offset, nm_flags);
    float4* out = reinterpret_cast<float4*>(job.dst + v);
    out[0] = q0; out[1] = q1; out[2] = q2;
}

}  // namespace swr
