// swr_character.hip.h -- CharacterController.Update on the GPU for a batch of controllers, one call per step.
//
// Reference (file:line under the C# repo):
//   CharacterController.Update         CharacterController.cs:50-140
//   ProjectOnPlane                     :142-155   scalar C#, NOT Vector3.Dot: left to right, plain rounded operations in every build
//   ApplyFriction .. AirControlFunc    :157-226
//   CheckPlane                         :228-306   9 rays per direction; fold: rays outer in offsets[] order, targets inner
//   MoveWithSlide                      :308-393   (verticalSteps + 1) x horizontalRays rays per attempt; fold: TARGETS outer, then vStep, hStep
// Both folds keep the first of equally distant hits of the serial schedule (strict '<'); they are reproduced as a 64-bit minimum over
// (distance word << 32 | position in the serial order), which is the same winner.
//
//   k_char_begin   a lane per controller: noclip (:52-61) ends the step; else gravity, cooldown, jump (:63-80) and the 18 CheckPlane
//                  rays (ground and ceiling share position and velocity); `active` = the bit mask of the rays that take part (:270)
//   k_char_cast    k_ray_cast over the rays of ONE controller per block, behind a uniform test of that controller's active word
//   k_char_planes  a wave per controller: both CheckPlane folds, Movement / MoveXZ, ground and ceiling response (:86-115), then the
//                  rays of the first slide attempt -- chain 1 (:96) with the ActualStepSize the controller CAME IN with, or chain 2
//   k_char_slide   a wave per controller, six times: folds the attempt, applies :375-392, and either emits the next attempt, or ends
//                  chain 1 and starts chain 2 (:98-118, with the new ActualStepSize), or ends the step (:121-139) and writes state
//                  and trace.  A controller walks its own way through the six rounds; one that is done has active = 0.
// Every key a fold reads is put back to "nothing" by the lane that read it, so the key buffer is clean for the next call.
// No LDS, no inline assembly.  The wave reductions are __shfl_xor.
#pragma once
#include "swr_raycast.hip.h"

#define SWR_CHAR_PLANE_RAYS 18            // 9 offsets x (ground, ceiling), :236-247
#define SWR_CHAR_SLIDE_ROUNDS 6           // 2 chains x MaxSlideAttempts (:311)
#define SWR_CHAR_MAX_RAYS 4096            // rays per slide attempt
#define SWR_NEG_INF (-__builtin_huge_valf())

namespace swr {

static_assert(sizeof(swr_character_params) == 52 && sizeof(swr_character) == 44 && sizeof(swr_character_input) == 16 &&
              sizeof(swr_character_trace) == 48, "ABI sizes of include/swr.h");

struct CharWork {                         // a controller between the kernels of one call
    float pos[3], vel[3], cooldown, step_in, step_now;      // step_in: ActualStepSize on entry; step_now: what MoveWithSlide reads
    float input[3];                       // MoveInput with Y = 0
    float max_distance;                   // CheckPlane's, the same for both directions (:258)
    float move_xz[3];
    float cur[3], desired[3], dir[3], move_distance;        // the running MoveWithSlide call
    int32_t grounded, ceiling;
    uint32_t phase;                       // 0 done, 1 chain 1, 2 chain 2, 3 CheckPlane pending
    uint32_t depth;
    swr_character_trace tr;
};

struct CharCall {                         // what every kernel of a call reads
    swr_character_params p;
    float dt;
    uint32_t n, n_targets, stride;        // stride: rays per controller in the ray buffers, max(18, slide_rays)
    uint32_t v_steps, h_rays, slide_rays; // slide_rays = (v_steps + 1) * h_rays
    uint32_t nm_flags;
};

// MathF.Max / MathF.Min: a NaN operand comes back, and of +-0 the positive / negative one
__device__ __forceinline__ float cs_max(float a, float b) {
    if (a != b) { if (!(a != a)) return b < a ? a : b; return a; }
    return (__float_as_uint(b) >> 31) ? a : b;
}
__device__ __forceinline__ float cs_min(float a, float b) {
    if (a != b) { if (!(a != a)) return a < b ? a : b; return a; }
    return (__float_as_uint(a) >> 31) ? a : b;
}
__device__ __forceinline__ float length3(const float v[3]) { return sqrtf(dot3(v[0], v[1], v[2], v[0], v[1], v[2])); }

// ProjectOnPlane, :142-155
__device__ __forceinline__ void project_on_plane(const float v[3], const float n[3], float out[3]) {
    const float len_sqr = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    if (len_sqr < 1e-6f) { out[0] = v[0]; out[1] = v[1]; out[2] = v[2]; return; }
    const float dot = (v[0] * n[0] + v[1] * n[1]) + v[2] * n[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = v[k] - (dot * n[k]) / len_sqr;
}

// ray `i` of CheckPlane (:262-273): i / 9 = 0 ground (direction -1), 1 ceiling (+1).  false: the ray takes no part (:270)
__device__ __forceinline__ bool plane_ray(const swr_character_params& p, const float pos[3], float vel_y, float dt, uint32_t i, swr_ray* out) {
    const float off[9][3] = { { 0, 0, 0 }, { -1, 0, 0 }, { 1, 0, 0 }, { 0, 0, -1 }, { 0, 0, 1 }, { -1, 0, -1 }, { -1, 0, 1 }, { 1, 0, -1 }, { 1, 0, 1 } };
    const uint32_t o = i % 9u;
    const float direction = i < 9u ? -1.0f : 1.0f;
    const float fe[3] = { pos[0] + 0.0f * dt, pos[1] + vel_y * dt, pos[2] + 0.0f * dt };          // :257
    float so[3] = { 0.0f, 0.0f, 0.0f };
    if (o != 0u) {
        float nrm[3];
        normalize3(off[o], nrm);
        const float s = p.radius - 0.01f;
        so[0] = nrm[0] * s; so[1] = nrm[1] * s; so[2] = nrm[2] * s;                               // :263
    }
    const float h = (p.height / 2.0f) - 0.01f;
    const float ho[3] = { (0.0f * direction) * h, (1.0f * direction) * h, (0.0f * direction) * h };   // :264
    float rd[3], nd[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float start = (pos[k] + so[k]) - ho[k], end = (fe[k] + so[k]) + ho[k];              // :266-267
        out->origin[k] = start;
        rd[k] = end - start;
    }
    const bool live = !(dot3(rd[0], rd[1], rd[2], rd[0], rd[1], rd[2]) < 0.0001f);                // :270
    normalize3(rd, nd);
    out->direction[0] = nd[0]; out->direction[1] = nd[1]; out->direction[2] = nd[2];
    return live;
}

// the start of a MoveWithSlide call (:318-321) from w.cur to w.desired, and its rays (:340-355), a lane to every 64th ray
__device__ __forceinline__ void slide_begin(const CharCall& cc, const float* __restrict__ ring, CharWork& w, swr_ray* __restrict__ rays, uint32_t lane) {
    const float mv[3] = { w.desired[0] - w.cur[0], w.desired[1] - w.cur[1], w.desired[2] - w.cur[2] };
    w.move_distance = length3(mv);
    normalize3(mv, w.dir);
    const float radius = cc.p.radius + 0.001f;
    const float half = cc.p.height * 0.5f;                                                        // :326
    const float bottom = -half + w.step_now;                                                      // :342
    const uint32_t vden = cc.v_steps > 1u ? cc.v_steps : 1u;
    for (uint32_t i = lane; i < cc.slide_rays; i += 64u) {
        const uint32_t vs = i / cc.h_rays, hs = i - vs * cc.h_rays;
        const float ho = nm_lerp(bottom, half, (float)vs / (float)vden);                          // :343
        const float hx = radius * ring[2u * hs], hz = radius * ring[2u * hs + 1u];                // :349-353
        swr_ray r;
        r.origin[0] = (w.cur[0] + 0.0f) + hx; r.origin[1] = (w.cur[1] + ho) + 0.0f; r.origin[2] = (w.cur[2] + 0.0f) + hz;   // :355
        r.direction[0] = w.dir[0]; r.direction[1] = w.dir[1]; r.direction[2] = w.dir[2];
        rays[i] = r;
    }
}

// :98-118 once chain 1 has returned (ground = true) or was not run: velocity, ActualStepSize, ceiling response, chain 2's first attempt
__device__ __forceinline__ void chain2_begin(const CharCall& cc, const float* __restrict__ ring, CharWork& w, bool ground, swr_ray* __restrict__ rays, uint32_t lane) {
    if (ground) {
        if (w.vel[1] < 0.0f) w.vel[1] = 0.0f;                                                     // :98-101
        w.step_now = cc.p.step_size;                                                              // :103
    } else {
        w.step_now = 0.0f;                                                                        // :107
    }
    if (w.ceiling && w.vel[1] > 0.0f) { w.vel[1] = 0.0f; w.cooldown = 0.0f; }                     // :111-115
#pragma unroll
    for (int k = 0; k < 3; ++k) { w.cur[k] = w.pos[k]; w.desired[k] = w.pos[k] + w.move_xz[k]; }  // :118
    w.phase = 2u; w.depth = 0u;
    w.tr.chain_attempts[1] = 1;
    slide_begin(cc, ring, w, rays, lane);
}

// :121-139, the controller's state and its trace
__device__ __forceinline__ void step_end(const CharCall& cc, CharWork& w, swr_character* __restrict__ out, swr_character_trace* __restrict__ trace, bool write) {
    const swr_character_params& p = cc.p;
    const float dt = cc.dt;
    const float add[3] = { 0.0f * dt, w.vel[1] * dt, 0.0f * dt };
    w.pos[0] += add[0]; w.pos[1] += add[1]; w.pos[2] += add[2];                                   // :121
    float wish[3];
    project_on_plane(w.input, w.tr.ground_normal, wish);                                          // :124
    float wish_speed = length3(wish);
    if (wish_speed > 1.0f) { wish[0] /= wish_speed; wish[1] /= wish_speed; wish[2] /= wish_speed; }
    wish_speed *= p.move_speed;
    float* v = w.vel;
    if (w.grounded) {
        bool stopped = false;
        {                                                                                         // ApplyFriction, :157-171
            const float hv[3] = { v[0], 0.0f, v[2] };
            const float speed = length3(hv);
            if (speed < 0.1f) { v[0] = 0.0f; v[2] = 0.0f; stopped = true; }
            if (!stopped) {
                const float drop = (speed * p.ground_friction) * dt;
                const float new_speed = cs_max(speed - drop, 0.0f);
                const float scale = new_speed / speed;
                v[0] = v[0] * scale; v[2] = v[2] * scale;
            }
        }
        {                                                                                         // GroundAccelerate, :173-182
            const float current = dot3(v[0], 0.0f, v[2], wish[0], wish[1], wish[2]);
            const float add_speed = wish_speed - current;
            if (!(add_speed <= 0.0f)) {
                const float accel = cs_min((p.ground_acceleration * wish_speed) * dt, add_speed);
                v[0] += wish[0] * accel; v[1] += 0.0f; v[2] += wish[2] * accel;
            }
        }
    } else {
        {                                                                                         // AirAccelerate, :184-203
            const float hv[3] = { v[0], 0.0f, v[2] };
            const float current = dot3(hv[0], hv[1], hv[2], wish[0], wish[1], wish[2]);
            const float add_speed = wish_speed - current;
            if (!(add_speed <= 0.0f)) {
                const float accel = cs_min((p.air_acceleration * wish_speed) * dt, add_speed);
                const float pv[3] = { hv[0] + wish[0] * accel, hv[1] + wish[1] * accel, hv[2] + wish[2] * accel };
                if (length3(pv) > p.max_air_speed) {
                    float pn[3];
                    normalize3(pv, pn);
                    v[0] = pn[0] * p.max_air_speed; v[2] = pn[2] * p.max_air_speed;
                } else {
                    v[0] += wish[0] * accel; v[1] += 0.0f; v[2] += wish[2] * accel;
                }
            }
        }
        if (!(dot3(wish[0], wish[1], wish[2], wish[0], wish[1], wish[2]) < 0.001f)) {             // AirControlFunc, :216-226
            const float hv[3] = { v[0], 0.0f, v[2] };
            if (!(length3(hv) < 0.1f)) {
                const float k = p.air_control * dt;
                v[0] += wish[0] * k; v[1] += 0.0f; v[2] += wish[2] * k;
            }
        }
        {                                                                                         // ClampAirSpeed, :205-214
            const float hv[3] = { v[0], 0.0f, v[2] };
            if (length3(hv) > p.max_air_speed) {
                float hn[3];
                normalize3(hv, hn);
                v[0] = hn[0] * p.max_air_speed; v[2] = hn[2] * p.max_air_speed;
            }
        }
    }
    w.phase = 0u;
    if (write) {
        swr_character c;
#pragma unroll
        for (int k = 0; k < 3; ++k) { c.position[k] = w.pos[k]; c.velocity[k] = w.vel[k]; }
        c.jump_cooldown = w.cooldown; c.actual_step_size = w.step_now;
        c.grounded = w.grounded; c.ceiling = w.ceiling; c.noclip = 0;
        *out = c;
        if (trace) *trace = w.tr;
    }
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(v, m, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, m, 64);
        v = o < v ? o : v;
    }
    return v;
}

// a lane per controller
__global__ __launch_bounds__(64) void k_char_begin(CharCall cc, const swr_character* __restrict__ chars, const swr_character_input* __restrict__ inputs,
                                                   CharWork* __restrict__ work, uint32_t* __restrict__ active, swr_ray* __restrict__ rays,
                                                   swr_character* __restrict__ out, swr_character_trace* __restrict__ trace) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= cc.n) return;
    const swr_character c = chars[i];
    const swr_character_input in = inputs[i];
    const swr_character_params& p = cc.p;
    const float dt = cc.dt;
    if (c.noclip) {                                                                               // :52-61
        float dir[3] = { in.move[0], in.move[1], in.move[2] };
        const float mag = length3(dir);
        if (mag > 1.0f) { dir[0] /= mag; dir[1] /= mag; dir[2] /= mag; }
        swr_character o = c;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o.velocity[k] = dir[k] * p.move_speed;
            o.position[k] = c.position[k] + o.velocity[k] * dt;
        }
        out[i] = o;
        if (trace) { swr_character_trace t; memset(&t, 0, sizeof(t)); trace[i] = t; }
        work[i].phase = 0u;
        active[i] = 0u;
        return;
    }
    CharWork w;
    memset(&w, 0, sizeof(w));
    w.input[0] = in.move[0]; w.input[1] = 0.0f; w.input[2] = in.move[2];                          // :63
#pragma unroll
    for (int k = 0; k < 3; ++k) { w.pos[k] = c.position[k]; w.vel[k] = c.velocity[k] + p.gravity[k] * dt; }   // :66
    w.cooldown = c.jump_cooldown;
    if (w.cooldown > 0.0f) w.cooldown -= dt;                                                      // :69-72
    w.grounded = c.grounded != 0;
    if (in.jump && w.grounded && w.cooldown <= 0.0f) {                                            // :75-80
        w.vel[1] = p.jump_force; w.grounded = 0; w.cooldown = 0.25f;
    }
    w.step_in = c.actual_step_size; w.step_now = c.actual_step_size;
    const float fe_y = w.pos[1] + w.vel[1] * dt;
    w.max_distance = fabsf(fe_y - w.pos[1]) + p.height;                                           // :258
    w.phase = 3u;
    uint32_t mask = 0u;
    for (uint32_t r = 0; r < SWR_CHAR_PLANE_RAYS; ++r) {
        swr_ray ray;
        if (plane_ray(p, w.pos, w.vel[1], dt, r, &ray)) mask |= 1u << r;
        rays[(size_t)i * cc.stride + r] = ray;
    }
    work[i] = w;
    active[i] = mask;
}

// k_ray_cast for the rays of one controller per block: grid = (controllers x ray chunks, triangle blocks of the largest target, targets).
// MASKED: `active` is the bit mask of the (at most 32) rays that take part; else every ray of an active controller does.
template <bool FUSED, bool MASKED>
__global__ __launch_bounds__(SWR_RAY_BLOCK) void k_char_cast(const swr_ray* __restrict__ rays, uint32_t stride, uint32_t n_per, uint32_t chunks,
                                                             const uint32_t* __restrict__ active, const RayTarget* __restrict__ targets,
                                                             uint32_t n_targets, uint32_t nm_flags, unsigned long long* __restrict__ best) {
    const uint32_t ctrl = blockIdx.x / chunks, chunk = blockIdx.x - ctrl * chunks;
    const uint32_t act = active[ctrl];
    if (!act) return;                                                      // (uniform: a finished controller costs its blocks this load)
    const RayTarget& t = targets[blockIdx.z];
    const uint32_t n_tris = t.n_tris;
    if (blockIdx.y * SWR_RAY_BLOCK >= n_tris) return;
    const bool fma_t = (nm_flags & SWR_NM_TRANSFORM_FMA) != 0u;
    const uint32_t tri_raw = blockIdx.y * SWR_RAY_BLOCK + threadIdx.x;
    const bool live = tri_raw < n_tris;
    const uint32_t tri = live ? tri_raw : n_tris - 1u;
    float v0[3], e1[3], e2[3];
    ray_triangle_edges(t, tri, fma_t, v0, e1, e2);
    const uint32_t r0 = chunk * SWR_RAY_CHUNK;
    const uint32_t n_here = min((uint32_t)SWR_RAY_CHUNK, n_per - r0);
    const size_t base = (size_t)ctrl * stride;
    const swr_ray* mine = rays + base + r0 + min(threadIdx.x & 63u, n_here - 1u);
    const float my_o[3] = { mine->origin[0], mine->origin[1], mine->origin[2] };
    const float my_raw[3] = { mine->direction[0], mine->direction[1], mine->direction[2] };
    float my_d[3];
    normalize3(my_raw, my_d);                                              // Physics.cs:69, on the caller's normalised direction
    for (uint32_t j = 0; j < n_here; ++j) {
        if (MASKED && !((act >> (r0 + j)) & 1u)) continue;
        float o[3], d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_o[k]), (int)j));
            d[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_d[k]), (int)j));
        }
        float distance, u, v;
        if (ray_triangle<FUSED>(o, d, v0, e1, e2, SWR_RAY_IGNORE_BACKFACES, distance, u, v) && live) {
            const unsigned long long key = ray_key(distance, tri);
            if (key != SWR_RAY_NO_HIT) atomicMin(&best[(base + r0 + j) * n_targets + blockIdx.z], key);
        }
    }
}

// The fold of one controller's keys by its wave: `n_rays` rays x n_targets keys at best[(ray0 + ray) * n_targets + target], every key
// read is put back.  A key takes part if `group(ray)` is `want` and its distance passes the limit (INCLUSIVE: d <= limit, CheckPlane
// :285; else d < limit, MoveWithSlide :362 from moveDistance).  TARGET_MAJOR: the serial order is targets outer, rays inner.
// Returns the winner's key (SWR_RAY_NO_HIT: none) and its ray and target.
struct FoldWin { unsigned long long key; uint32_t ray, target; };

template <bool TARGET_MAJOR, bool INCLUSIVE, bool TWO_GROUPS>
__device__ __forceinline__ void fold_keys(unsigned long long* __restrict__ best, size_t ray0, uint32_t n_rays, uint32_t n_targets, float limit,
                                          uint32_t lane, FoldWin win[TWO_GROUPS ? 2 : 1]) {
    constexpr int G = TWO_GROUPS ? 2 : 1;
    unsigned long long mine[G];
    uint32_t mine_tri[G];
#pragma unroll
    for (int g = 0; g < G; ++g) { mine[g] = SWR_RAY_NO_HIT; mine_tri[g] = 0xffffffffu; }
    const uint32_t total = n_rays * n_targets;
    unsigned long long* keys = best + ray0 * n_targets;
    for (uint32_t i = lane; i < total; i += 64u) {
        const unsigned long long key = keys[i];
        if (key == SWR_RAY_NO_HIT) continue;
        keys[i] = SWR_RAY_NO_HIT;
        const uint32_t ray = i / n_targets, t = i - ray * n_targets;
        const float d = __uint_as_float((uint32_t)(key >> 32));
        if (!(INCLUSIVE ? d <= limit : d < limit)) continue;
        const uint32_t serial = TARGET_MAJOR ? t * n_rays + ray : i;
        const unsigned long long cand = (key & 0xffffffff00000000ull) | serial;
        const int g = TWO_GROUPS ? (ray >= 9u ? 1 : 0) : 0;
#pragma unroll
        for (int q = 0; q < G; ++q)
            if (q == g && cand < mine[q]) { mine[q] = cand; mine_tri[q] = (uint32_t)key; }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const unsigned long long w = wave_min_u64(mine[g]);
        const uint32_t tri = wave_min_u32(mine[g] == w ? mine_tri[g] : 0xffffffffu);      // (serial positions are unique: one lane holds it)
        if (w == SWR_RAY_NO_HIT) { win[g].key = SWR_RAY_NO_HIT; win[g].ray = 0u; win[g].target = 0u; continue; }
        const uint32_t serial = (uint32_t)w;
        win[g].key = (w & 0xffffffff00000000ull) | tri;
        if (TARGET_MAJOR) { win[g].target = serial / n_rays; win[g].ray = serial - win[g].target * n_rays; }
        else { win[g].ray = serial / n_targets; win[g].target = serial - win[g].ray * n_targets; }
    }
}

// a wave per controller; rays_in: what the last cast read, rays_out: the next cast's
template <bool FUSED>
__global__ __launch_bounds__(64) void k_char_planes(CharCall cc, const float* __restrict__ ring, CharWork* __restrict__ work, uint32_t* __restrict__ active,
                                                    const swr_ray* __restrict__ rays_in, swr_ray* __restrict__ rays_out, const RayTarget* __restrict__ targets,
                                                    unsigned long long* __restrict__ best) {
    const uint32_t c = blockIdx.x, lane = threadIdx.x;
    if (work[c].phase != 3u) return;
    CharWork w = work[c];
    const bool fma_t = (cc.nm_flags & SWR_NM_TRANSFORM_FMA) != 0u;
    const size_t ray0 = (size_t)c * cc.stride;
    FoldWin win[2];
    fold_keys<false, true, true>(best, ray0, SWR_CHAR_PLANE_RAYS, cc.n_targets, w.max_distance, lane, win);
    float gp[3] = { SWR_NEG_INF, SWR_NEG_INF, SWR_NEG_INF }, gn[3] = { 0.0f, 1.0f, 0.0f };         // :231-232
    const bool ground = win[0].key != SWR_RAY_NO_HIT;
    if (ground) {
        swr_ray_hit h;
        ray_record<FUSED>(rays_in[ray0 + win[0].ray], targets[win[0].target], (int)win[0].target, win[0].key, SWR_RAY_IGNORE_BACKFACES, fma_t, &h);
#pragma unroll
        for (int k = 0; k < 3; ++k) { gp[k] = h.point[k]; gn[k] = h.normal[k]; }
    }
    w.grounded = ground ? 1 : 0;                                                                  // :83
    w.ceiling = win[1].key != SWR_RAY_NO_HIT ? 1 : 0;                                             // :90
    w.tr.ground_found = w.grounded; w.tr.ceiling_found = w.ceiling;
#pragma unroll
    for (int k = 0; k < 3; ++k) { w.tr.ground_point[k] = gp[k]; w.tr.ground_normal[k] = gn[k]; }
    const float movement[3] = { w.vel[0] * cc.dt, 0.0f, w.vel[2] * cc.dt };                       // :86-87
    project_on_plane(movement, gn, w.move_xz);
    swr_ray* out = rays_out + ray0;
    const bool not_neg_inf = !(gp[0] == SWR_NEG_INF && gp[1] == SWR_NEG_INF && gp[2] == SWR_NEG_INF);
    if (ground && not_neg_inf && w.cooldown <= 0.0f) {                                            // :93-96
        w.cur[0] = w.pos[0]; w.cur[1] = w.pos[1]; w.cur[2] = w.pos[2];
        w.desired[0] = w.pos[0]; w.desired[1] = gp[1] + cc.p.height * 0.5f; w.desired[2] = w.pos[2];
        w.phase = 1u; w.depth = 0u;
        w.tr.chain_attempts[0] = 1;
        w.step_now = w.step_in;                      // (:96 runs before :103: chain 1 reads the ActualStepSize of the previous step)
        slide_begin(cc, ring, w, out, lane);
    } else {
        chain2_begin(cc, ring, w, false, out, lane);
    }
    if (lane == 0u) { work[c] = w; active[c] = 1u; }
}

template <bool FUSED>
__global__ __launch_bounds__(64) void k_char_slide(CharCall cc, const float* __restrict__ ring, CharWork* __restrict__ work, uint32_t* __restrict__ active,
                                                   const swr_ray* __restrict__ rays_in, swr_ray* __restrict__ rays_out, const RayTarget* __restrict__ targets,
                                                   unsigned long long* __restrict__ best, swr_character* __restrict__ out, swr_character_trace* __restrict__ trace) {
    const uint32_t c = blockIdx.x, lane = threadIdx.x;
    const uint32_t phase = work[c].phase;
    if (phase != 1u && phase != 2u) return;
    CharWork w = work[c];
    const bool fma_t = (cc.nm_flags & SWR_NM_TRANSFORM_FMA) != 0u;
    const size_t ray0 = (size_t)c * cc.stride;
    const int chain = (int)phase - 1;
    FoldWin win[1];
    fold_keys<true, false, false>(best, ray0, cc.slide_rays, cc.n_targets, w.move_distance, lane, win);
    float result[3];
    int stop = 0;
    bool again = false;
    if (win[0].key == SWR_RAY_NO_HIT) {                                                           // :375-376
        result[0] = w.desired[0]; result[1] = w.desired[1]; result[2] = w.desired[2];
        stop = 1;
    } else {
        swr_ray_hit h;
        ray_record<FUSED>(rays_in[ray0 + win[0].ray], targets[win[0].target], (int)win[0].target, win[0].key, SWR_RAY_IGNORE_BACKFACES, fma_t, &h);
        float hn[3], safe[3], remaining[3];
        normalize3(h.normal, hn);                                                                 // :365
        const float back = h.distance - 0.001f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            safe[k] = w.cur[k] + w.dir[k] * back;                                                 // :378
            remaining[k] = w.desired[k] - safe[k];                                                // :379
            result[k] = safe[k];
        }
        const float alignment = dot3(w.dir[0], w.dir[1], w.dir[2], hn[0], hn[1], hn[2]);          // :381
        if (fabsf(alignment) > 0.9f) stop = 2;
        else {
            float inner[3], sd[3];
            cross3<FUSED>(remaining, hn, inner);
            cross3<FUSED>(hn, inner, sd);                                                         // :385
            if (sd[0] == 0.0f && sd[1] == 0.0f && sd[2] == 0.0f) stop = 3;
            else if (w.depth + 1u >= 3u) stop = 4;                                                // :314 of the call at :392
            else {
                float sn[3];
                normalize3(sd, sn);
                const float len = length3(remaining);
#pragma unroll
                for (int k = 0; k < 3; ++k) { w.cur[k] = safe[k]; w.desired[k] = safe[k] + sn[k] * len; }   // :389-392
                again = true;
            }
        }
    }
    swr_ray* next = rays_out + ray0;
    uint32_t act = 1u;
    if (again) {
        w.depth += 1u;
        if (chain == 0) w.tr.chain_attempts[0] += 1; else w.tr.chain_attempts[1] += 1;      // (no dynamic index: w stays in registers)
        slide_begin(cc, ring, w, next, lane);
    } else {
        if (chain == 0) w.tr.chain_stop[0] = stop; else w.tr.chain_stop[1] = stop;
        w.pos[0] = result[0]; w.pos[1] = result[1]; w.pos[2] = result[2];
        if (chain == 0) chain2_begin(cc, ring, w, true, next, lane);
        else { step_end(cc, w, out + c, trace ? trace + c : nullptr, lane == 0u); act = 0u; }
    }
    if (lane == 0u) { work[c] = w; active[c] = act; }
}

}  // namespace swr
