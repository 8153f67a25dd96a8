// swr_query.h -- host side of the ray queries and the character update (swr_raycast, swr_raycast_nearest, swr_character_update).
// Everything runs on the context's ray stream, which is idle between calls (a call waits for its own result under the context mutex):
// one copy up, the kernels, one copy down, one wait.  No allocation in the steady state (hipMalloc / hipFree would wait for the frame in flight).
#pragma once
#include "swr_query_layout.h"

namespace {
static_assert(sizeof(RayTarget) == kRayTargetBytes && sizeof(CharWork) == kCharWorkBytes, "the record sizes swr_query_layout.h lays out");
int ensure_ray_stream(swr_context* c) { if (!c->ray_stream) SWR_HIP(c, hipStreamCreateWithFlags(&c->ray_stream, hipStreamNonBlocking)); return SWR_OK; }
// one key per (ray, target) pair, all SWR_RAY_NO_HIT: a grown buffer is filled once, from then on the kernels that fold the keys leave it clean
int ensure_best_keys(swr_context* c, size_t pairs) {
    if (c->d_ray_best.cap >= pairs * 8) return SWR_OK;
    int rc = ensure(c, c->d_ray_best, pairs * 8); if (rc) return rc;
    SWR_HIP(c, hipMemsetAsync(c->d_ray_best.p, 0xff, c->d_ray_best.cap, c->ray_stream));
    return SWR_OK;
}

// The host block a call's upload is assembled in (*up; a staged call's download lands behind it): the context's pinned block for a
// staged call, grown to the exact size with a floor of 64 KiB, else `pageable` at the size the caller gives.
int query_host_block(swr_context* c, size_t up_bytes, size_t down_bytes, size_t pageable_bytes, std::vector<char>& pageable, char** up) {
    const bool staged = query_is_staged(up_bytes, down_bytes);
    if (staged) SWR_HIP(c, ensure_pinned(c->ray_host, std::max<size_t>(up_bytes + down_bytes, (size_t)1 << 16)));
    else pageable.resize(pageable_bytes);
    *up = staged ? static_cast<char*>(c->ray_host.p) : pageable.data();
    return SWR_OK;
}

// swr_ray_target[] as the kernels read it; the ray stream waits (once per mesh) for the mesh's upload
int stage_targets(swr_context* c, const swr_ray_target* targets, int n, RayTarget* out, uint32_t* max_tris) {
    *max_tris = 0;
    for (int t = 0; t < n; ++t) {
        swr_mesh* m = const_cast<swr_mesh*>(targets[t].mesh);
        if (m->uploaded && !m->upload_seen) { SWR_HIP(c, hipStreamWaitEvent(c->ray_stream, m->posed ? m->posed->ev : m->uploaded, 0)); m->upload_seen = true; }
        out[t].verts = m->d_verts; out[t].idx = m->d_idx; out[t].n_tris = (uint32_t)(m->n_idx / 3); out[t].pad = 0u;
        memcpy(out[t].model, targets[t].model, 64); memcpy(out[t].normal_matrix, targets[t].normal_matrix, 64);
        *max_tris = std::max(*max_tris, out[t].n_tris);
    }
    return SWR_OK;
}

// swr_raycast / swr_raycast_nearest: rays and targets go up, k_ray_cast and k_ray_finish run, the records come back
int raycast(swr_context* c, const swr_ray* rays, int n_rays, const swr_ray_target* targets, int n_targets, int flags, swr_ray_hit* out, bool nearest) {
    if (n_rays < 0 || n_targets < 0) return fail(c, SWR_ERR_INVALID_ARG, "negative ray or target count");
    if (flags & ~(SWR_RAY_IGNORE_BACKFACES | SWR_RAY_IGNORE_FRONTFACES | SWR_RAY_CROSS_FUSED)) return fail(c, SWR_ERR_INVALID_ARG, "unknown raycast flag bits");
    if (n_rays == 0 || n_targets == 0) return SWR_OK;
    if (!rays || !targets || !out) return fail(c, SWR_ERR_INVALID_ARG, "null argument to raycast");
    if (n_rays > (1 << 20) || n_targets > 65535 || (uint64_t)n_rays * (uint64_t)n_targets > (1ull << 24))
        return fail(c, SWR_ERR_UNSUPPORTED, "raycast: at most 2^20 rays, 65535 targets and 2^24 (ray, target) pairs per call: split the rays");
    for (int t = 0; t < n_targets; ++t) if (!targets[t].mesh) return fail(c, SWR_ERR_INVALID_ARG, "raycast target without a mesh");
    int rc = ensure_ray_stream(c); if (rc) return rc;
    const RayLayout L = ray_layout(n_rays, n_targets, nearest);
    if ((rc = ensure(c, c->d_ray, L.up_bytes + L.down_bytes))) return rc;
    if ((rc = ensure_best_keys(c, L.pairs))) return rc;
    const bool staged = query_is_staged(L.up_bytes, L.down_bytes);
    std::vector<char> pageable; char* up = nullptr; uint32_t max_tris = 0;
    if ((rc = query_host_block(c, L.up_bytes, L.down_bytes, L.up_bytes, pageable, &up))) return rc;      // (pageable: the records go straight to `out`)
    memcpy(up, rays, (size_t)n_rays * sizeof(swr_ray));
    if ((rc = stage_targets(c, targets, n_targets, reinterpret_cast<RayTarget*>(up + L.off_targets), &max_tris))) return rc;
    char* base = static_cast<char*>(c->d_ray.p);
    const swr_ray* d_rays = reinterpret_cast<const swr_ray*>(base);
    const RayTarget* d_targets = reinterpret_cast<const RayTarget*>(base + L.off_targets);
    swr_ray_hit* d_out = reinterpret_cast<swr_ray_hit*>(base + L.up_bytes);
    unsigned long long* d_best = c->d_ray_best.as<unsigned long long>();
    const uint32_t mask = (uint32_t)flags & 3u, nr = (uint32_t)n_rays, nt = (uint32_t)n_targets;
    hipStream_t s = c->ray_stream;
    SWR_HIP(c, hipMemcpyAsync(base, up, L.up_bytes, hipMemcpyHostToDevice, s));
    with_flag((flags & SWR_RAY_CROSS_FUSED) != 0, [&](auto fused_t) {
        constexpr bool FUSED = decltype(fused_t)::value;
        if (max_tris) {
            const dim3 grid((max_tris + SWR_RAY_BLOCK - 1) / SWR_RAY_BLOCK, (nr + SWR_RAY_CHUNK - 1) / SWR_RAY_CHUNK, nt);
            hipLaunchKernelGGL(k_ray_cast<FUSED>, grid, dim3(SWR_RAY_BLOCK), 0, s, d_rays, nr, d_targets, nt, mask, c->nm_flags, d_best);
        }
        with_flag(nearest, [&](auto nearest_t) {
            hipLaunchKernelGGL((k_ray_finish<FUSED, decltype(nearest_t)::value>), dim3((unsigned)((L.n_out + 63) / 64)), dim3(64), 0, s,
                               d_rays, nr, d_targets, nt, mask, c->nm_flags, d_best, d_out);
        });
    });
    SWR_HIP(c, hipGetLastError());
    void* down = staged ? static_cast<void*>(up + L.up_bytes) : static_cast<void*>(out);
    SWR_HIP(c, hipMemcpyAsync(down, d_out, L.down_bytes, hipMemcpyDeviceToHost, s));
    SWR_HIP(c, hipStreamSynchronize(s));
    if (staged) memcpy(out, down, L.down_bytes);
    return SWR_OK;
}

// Math.Max(1, (int)(Height / (radius * 2))) and Math.Max(4, (int)(4 * MathF.PI * radius / 0.1f)), CharacterController.cs:327-328, radius = Radius + 0.001f
// (:96,118): float arithmetic in the reference's order.  false: a count that is not a number or does not fit the limits.
bool character_ray_counts(const swr_character_params* p, int* v_steps, int* h_rays) {
    const float radius = p->radius + 0.001f;
    const float two_r = radius * 2.0f;
    const float v = p->height / two_r;
    const float four_pi = 4.0f * 3.14159274f;
    const float h = (four_pi * radius) / 0.1f;
    const bool ok = v == v && h == h && v < 65536.0f && h < 65536.0f;
    *v_steps = ok ? std::max(1, (int)v) : 1;
    *h_rays = ok ? std::max(4, (int)h) : 4;
    return ok;
}
// swr_character_update: one upload, k_char_begin, (cast, planes), 6 x (cast, slide), one download, one wait -- nothing between the
// kernels is read by the host, and no grid depends on a value computed on the device.
int character_update(swr_context* c, const swr_character_params* params, swr_character* chars, const swr_character_input* inputs, int n, float dt,
                     const float* ring, int n_ring, const swr_ray_target* targets, int n_targets, int flags, swr_character_trace* trace) {
    if (n < 0 || n_targets < 0 || n_ring < 0) return fail(c, SWR_ERR_INVALID_ARG, "negative count in character update");
    if (flags & ~SWR_RAY_CROSS_FUSED) return fail(c, SWR_ERR_INVALID_ARG, "character update accepts SWR_RAY_CROSS_FUSED only");
    if (n == 0) return SWR_OK;
    if (!params || !chars || !inputs || !ring || (n_targets > 0 && !targets)) return fail(c, SWR_ERR_INVALID_ARG, "null argument to character update");
    int v_steps = 0, h_rays = 0;
    const bool counts_ok = character_ray_counts(params, &v_steps, &h_rays);
    const uint64_t slide_rays = (uint64_t)(v_steps + 1) * (uint64_t)h_rays;
    const uint64_t stride = std::max<uint64_t>(slide_rays, SWR_CHAR_PLANE_RAYS);
    static const char* limits = "character update: at most 65536 controllers, 4096 rays per slide attempt, 2^22 rays (controllers x rays per attempt), 65535 targets and 2^24 (ray, target) pairs per call: split the controllers";
    if (!counts_ok || slide_rays > SWR_CHAR_MAX_RAYS) return fail(c, SWR_ERR_UNSUPPORTED, limits);
    if (n_ring != h_rays) return fail(c, SWR_ERR_INVALID_ARG, "n_ring must equal horizontal_rays of swr_character_ray_counts");
    if (n > 65536 || n_targets > 65535 || (uint64_t)n * stride > (1ull << 22) || (uint64_t)n * stride * (uint64_t)n_targets > (1ull << 24)) return fail(c, SWR_ERR_UNSUPPORTED, limits);
    for (int t = 0; t < n_targets; ++t) if (!targets[t].mesh) return fail(c, SWR_ERR_INVALID_ARG, "character update target without a mesh");
    int rc = ensure_ray_stream(c); if (rc) return rc;
    const CharLayout L = char_layout(n, n_ring, n_targets, (size_t)stride);
    const size_t N = (size_t)n;
    if ((rc = ensure(c, c->d_char, L.total))) return rc;
    if ((rc = ensure_best_keys(c, L.pairs))) return rc;
    std::vector<char> pageable; char* up = nullptr; uint32_t max_tris = 0;
    if ((rc = query_host_block(c, L.up_bytes, L.down_bytes, L.up_bytes + L.down_bytes, pageable, &up))) return rc;
    memcpy(up + L.off_chars, chars, N * sizeof(swr_character));
    memcpy(up + L.off_in, inputs, N * sizeof(swr_character_input));
    memcpy(up + L.off_ring, ring, (size_t)n_ring * 8);
    if ((rc = stage_targets(c, targets, n_targets, reinterpret_cast<RayTarget*>(up + L.off_targets), &max_tris))) return rc;
    char* base = static_cast<char*>(c->d_char.p);
    const swr_character* d_chars = reinterpret_cast<const swr_character*>(base + L.off_chars);
    const swr_character_input* d_in = reinterpret_cast<const swr_character_input*>(base + L.off_in);
    const float* d_ring = reinterpret_cast<const float*>(base + L.off_ring);
    const RayTarget* d_targets = reinterpret_cast<const RayTarget*>(base + L.off_targets);
    CharWork* d_work = reinterpret_cast<CharWork*>(base + L.off_work);
    uint32_t* d_active = reinterpret_cast<uint32_t*>(base + L.off_active);
    swr_ray* d_rays[2] = { reinterpret_cast<swr_ray*>(base + L.off_rays), reinterpret_cast<swr_ray*>(base + L.off_rays + L.rays_bytes) };
    swr_character* d_out = reinterpret_cast<swr_character*>(base + L.off_down);
    swr_character_trace* d_trace = trace ? reinterpret_cast<swr_character_trace*>(base + L.off_down + L.off_trace) : nullptr;
    unsigned long long* d_best = c->d_ray_best.as<unsigned long long>();
    CharCall cc;
    cc.p = *params; cc.dt = dt; cc.n = (uint32_t)n; cc.n_targets = (uint32_t)n_targets; cc.stride = (uint32_t)stride;
    cc.v_steps = (uint32_t)v_steps; cc.h_rays = (uint32_t)h_rays; cc.slide_rays = (uint32_t)slide_rays; cc.nm_flags = c->nm_flags;
    const uint32_t tri_blocks = (max_tris + SWR_RAY_BLOCK - 1) / SWR_RAY_BLOCK, nt = cc.n_targets, st = cc.stride;
    hipStream_t s = c->ray_stream;
    SWR_HIP(c, hipMemcpyAsync(base, up, L.up_bytes, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_char_begin, dim3((cc.n + 63u) / 64u), dim3(64), 0, s, cc, d_chars, d_in, d_work, d_active, d_rays[0], d_out, d_trace);
    with_flag((flags & SWR_RAY_CROSS_FUSED) != 0, [&](auto fused_t) {
        constexpr bool FUSED = decltype(fused_t)::value;
        if (tri_blocks)
            hipLaunchKernelGGL((k_char_cast<FUSED, true>), dim3(cc.n, tri_blocks, nt), dim3(SWR_RAY_BLOCK), 0, s, d_rays[0], st, (uint32_t)SWR_CHAR_PLANE_RAYS, 1u,
                               d_active, d_targets, nt, cc.nm_flags, d_best);
        hipLaunchKernelGGL(k_char_planes<FUSED>, dim3(cc.n), dim3(64), 0, s, cc, d_ring, d_work, d_active, d_rays[0], d_rays[1], d_targets, d_best);
        const uint32_t chunks = (cc.slide_rays + SWR_RAY_CHUNK - 1) / SWR_RAY_CHUNK;
        for (int round = 0; round < SWR_CHAR_SLIDE_ROUNDS; ++round) {
            swr_ray* in = d_rays[(round + 1) & 1];
            swr_ray* next = d_rays[round & 1];
            if (tri_blocks)
                hipLaunchKernelGGL((k_char_cast<FUSED, false>), dim3(cc.n * chunks, tri_blocks, nt), dim3(SWR_RAY_BLOCK), 0, s, in, st, cc.slide_rays, chunks,
                                   d_active, d_targets, nt, cc.nm_flags, d_best);
            hipLaunchKernelGGL(k_char_slide<FUSED>, dim3(cc.n), dim3(64), 0, s, cc, d_ring, d_work, d_active, in, next, d_targets, d_best, d_out, d_trace);
        }
    });
    SWR_HIP(c, hipGetLastError());
    const size_t down_now = trace ? L.down_bytes : N * sizeof(swr_character);
    char* down = up + L.up_bytes;
    SWR_HIP(c, hipMemcpyAsync(down, d_out, down_now, hipMemcpyDeviceToHost, s));
    SWR_HIP(c, hipStreamSynchronize(s));
    memcpy(chars, down, N * sizeof(swr_character));
    if (trace) memcpy(trace, down + L.off_trace, N * sizeof(swr_character_trace));
    return SWR_OK;
}

}  // namespace
