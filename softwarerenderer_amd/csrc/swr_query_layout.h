// swr_query_layout.h -- where the pieces of a ray query and of a character update lie in their device blocks (d_ray, d_char) and in
// the host block that mirrors them, in bytes, which host block a call goes through, and where a batched probe's records lie in d_scratch.  No HIP types: pure functions of a call's
// counts (tests/test_query_layout_host.py builds them with the host compiler).  swr_query.h asserts the two record sizes.
#pragma once
#include <cstddef>
#include "swr.h"

namespace swr {
constexpr size_t kRayTargetBytes = 152;      // sizeof(RayTarget), swr_raycast.hip.h
constexpr size_t kCharWorkBytes = 168;       // sizeof(CharWork), swr_character.hip.h
constexpr size_t query_align(size_t b) { return (b + 15) & ~(size_t)15; }
// d_scratch of a batched probe (swr_texture.h): n input records at 0, then each output array at the next multiple of 16
// (out_bytes[1] == 0: one output).  total: what the block must hold.
struct ProbeLayout { size_t off_out[2], total; };
inline ProbeLayout probe_layout(int n, size_t in_bytes, size_t out0_bytes, size_t out1_bytes) {
    const size_t N = (size_t)n;
    ProbeLayout l;
    l.off_out[0] = query_align(N * in_bytes); l.off_out[1] = l.off_out[0] + query_align(N * out0_bytes);
    l.total = out1_bytes ? l.off_out[1] + N * out1_bytes : l.off_out[0] + N * out0_bytes;
    return l;
}
// small queries (a slide attempt: 111 rays x 11 meshes, 4.4 KB each way) go through one pinned block; large ones use pageable memory
constexpr size_t kQueryStagedBytes = (size_t)1 << 20;
constexpr bool query_is_staged(size_t up_bytes, size_t down_bytes) { return up_bytes + down_bytes <= kQueryStagedBytes; }
// d_ray: rays | targets | hit records.  The first up_bytes go up in one copy, down_bytes come back from behind them.
struct RayLayout { size_t pairs, n_out, off_targets, up_bytes, down_bytes; };    // pairs: the keys in d_ray_best; n_out: records that come back
inline RayLayout ray_layout(int n_rays, int n_targets, bool nearest) {
    RayLayout l;
    l.pairs = (size_t)n_rays * (size_t)n_targets; l.n_out = nearest ? (size_t)n_rays : l.pairs;
    l.off_targets = query_align((size_t)n_rays * sizeof(swr_ray));
    l.up_bytes = l.off_targets + query_align((size_t)n_targets * kRayTargetBytes); l.down_bytes = l.n_out * sizeof(swr_ray_hit);
    return l;
}
// d_char: controllers | inputs | ring | targets (these go up) | work | active | rays x 2 | results | traces (these come down; off_trace
// is relative to off_down).  The host block holds the upload and, behind it, the download.
struct CharLayout {
    size_t pairs;                            // controllers x stride x targets
    size_t off_chars, off_in, off_ring, off_targets, up_bytes;
    size_t off_work, off_active, off_rays, rays_bytes;
    size_t off_down, off_trace, down_bytes, total;
};
inline CharLayout char_layout(int n, int n_ring, int n_targets, size_t stride) {
    const size_t N = (size_t)n, NT = (size_t)n_targets;
    CharLayout l;
    l.pairs = N * stride * NT;
    l.off_chars = 0; l.off_in = l.off_chars + query_align(N * sizeof(swr_character)); l.off_ring = l.off_in + query_align(N * sizeof(swr_character_input));
    l.off_targets = l.off_ring + query_align((size_t)n_ring * 8); l.up_bytes = l.off_targets + query_align(NT * kRayTargetBytes);
    l.off_work = l.up_bytes; l.off_active = l.off_work + query_align(N * kCharWorkBytes); l.off_rays = l.off_active + query_align(N * 4);
    l.rays_bytes = query_align(N * stride * sizeof(swr_ray));
    l.off_down = l.off_rays + 2 * l.rays_bytes; l.off_trace = query_align(N * sizeof(swr_character));
    l.down_bytes = l.off_trace + N * sizeof(swr_character_trace); l.total = l.off_down + l.down_bytes;
    return l;
}
}  // namespace swr
