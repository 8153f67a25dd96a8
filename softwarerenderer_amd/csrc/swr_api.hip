// swr_api.hip -- host side of libswr_hip.so: the C ABI of include/swr.h over the gfx950 kernels.
//
// A context records draws (Rasterizer.RenderMesh calls, Rasterizer.cs:163-174) in submission order
// and executes them as ONE batch per flush:
//     [k_frustum_cull ->] k_vertex -> k_setup -> k_bin<count> -> k_scan_sums/apply -> k_bin<fill> -> k_sort_tiles
//     (+ the tile order in its last blocks) -> k_cover -> k_raster_c
// There is no CPU fallback anywhere in this file: every pixel is produced by the HIP kernels.
//
// Frames in flight (swr_set_pipelining, on by default): the reference's loop renders frames back to back (Renderer.cs:404-419,
// Rasterizer.cs:163-230), and a frame here has two halves with different bounds -- a front end of record traffic and latency
// (vertex .. k_cover) and an issue-bound raster kernel.  The front end of flush N+1 therefore runs on a stream of its own
// (`front_stream`) beside the raster kernel of flush N: everything a raster kernel reads lives in one of two RasterSets that
// alternate per flush, two events per set order the hand-overs (front_done: F -> R, raster_done: R -> the front end that reuses
// the set two flushes later), the tile order's history comes from flush N-1, and the poison / replay protocol is per batch
// (batch_poisoned in swr_device.h).  The framebuffer is touched by the raster stream only, so everything a caller orders against
// `stream` (flatten, read-back, collectives) still sees frames in submission order.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>            // (types only: the run-time compiler is loaded with dlopen, see RtcLib)
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#if defined(SWR_RTC_FLAGS)
#include "swr_rtc_sources.inc"     // the headers user fragment programs compile against (Makefile: RTC_INC)
#endif

#include "swr.h"
#include "swr_device.h"
#include "swr_geometry.hip.h"
#include "swr_binning.hip.h"
#include "swr_raster.hip.h"
#include "swr_raster_c.hip.h"
#include "swr_cull.hip.h"
#include "swr_raycast.hip.h"
#include "swr_character.hip.h"
#include "swr_deliver.hip.h"
#include "swr_post.hip.h"
#include "swr_mesh_deform.hip.h"
#include "swr_animation.hip.h"

using namespace swr;

#define SWR_STR2(x) #x
#define SWR_STR(x) SWR_STR2(x)

#include "swr_host.h"
#include "swr_rtc.h"
#include "swr_flush.h"
#include "swr_query.h"

namespace {      // shapes several entry points share
// the band's colour plane as packed RGB floats in device memory, on the context's stream
int launch_flatten(swr_context* c, float* d_rgb, size_t n) {
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 2048 * 8);
    hipLaunchKernelGGL(k_flatten_rgb, dim3(blocks), dim3(256), 0, c->stream, (const float4*)c->color, d_rgb, n);
    SWR_HIP(c, hipGetLastError());
    return SWR_OK;
}

// What a present call delivers: the flatten (k_flatten_rgb, one RGB triple per band pixel), the kx x ky box-filter resolve
// (k_resolve_rgb, one triple per kx x ky block of band pixels), or the resolve quantised to bytes (k_present8: RGB8 or RGBX8, factors
// (1, 1) being the plain frame) -- or, with a post-process program, what the program makes of the resolved frame (k_resolve_rgba unless
// the factors are (1, 1), then the program's k_post), in any of the three formats.  Every present shape below is defined once over
// this, in bytes of the payload's format.
enum PayloadFormat { PAYLOAD_RGB32F, PAYLOAD_RGB8, PAYLOAD_RGBX8, PAYLOAD_NO_FORMAT };
struct Payload {
    bool resolve; int kx, ky; PayloadFormat format;
    bool posted = false;                 // swr_*_post*: `post` runs on the resolved frame ...
    const PostProg* post = nullptr;      // ... (null: the id is unknown or destroyed); the context's table holds it for the call
};
constexpr Payload FLATTEN = {false, 1, 1, PAYLOAD_RGB32F};
constexpr Payload resolved(int kx, int ky) { return Payload{true, kx, ky, PAYLOAD_RGB32F}; }
constexpr Payload quantised(int kx, int ky, int bpp) { return Payload{true, kx, ky, bpp == 3 ? PAYLOAD_RGB8 : bpp == 4 ? PAYLOAD_RGBX8 : PAYLOAD_NO_FORMAT}; }
// a post program by id and SWR_POST_* format
Payload posted(const swr_context* c, int post_id, int kx, int ky, int format) {
    Payload p{true, kx, ky, format == SWR_POST_RGB32F ? PAYLOAD_RGB32F : format == SWR_POST_RGB8 ? PAYLOAD_RGB8 : format == SWR_POST_RGBX8 ? PAYLOAD_RGBX8 : PAYLOAD_NO_FORMAT};
    p.posted = true;
    const auto it = c->posts.find(post_id);
    if (it != c->posts.end()) p.post = it->second.get();
    return p;
}
size_t payload_bpp(const Payload& p) { return p.format == PAYLOAD_RGB32F ? 12 : p.format == PAYLOAD_RGB8 ? 3 : 4; }

bool resolve_factor_ok(int k) { return k == 1 || k == 2 || k == 4 || k == 8; }
// a zero-size target resolves to nothing under any factor pair; otherwise the frame must divide (then every band's rows do too:
// the factors divide the tile, and the last tile row holds H - 16 * (tiles_y - 1) pixel rows)
// (delivery false: swr_post_size, which names no program and sizes a band's payload like every *_size call)
int payload_check(swr_context* c, const Payload& p, bool delivery = true) {
    if (!p.resolve) return SWR_OK;
    if (p.format == PAYLOAD_NO_FORMAT)
        return fail(c, SWR_ERR_INVALID_ARG, p.posted ? "format must be SWR_POST_RGB32F (0), SWR_POST_RGB8 (3) or SWR_POST_RGBX8 (4)" : "bpp must be 3 (RGB8) or 4 (RGBX8)");
    if (!resolve_factor_ok(p.kx) || !resolve_factor_ok(p.ky)) return fail(c, SWR_ERR_INVALID_ARG, "resolve factors must be 1, 2, 4 or 8");
    if (p.posted && delivery && !p.post) return fail(c, SWR_ERR_INVALID_ARG, "unknown or destroyed post program id");
    if (c->W <= 0 || c->H <= 0) return SWR_OK;
    if (c->W % p.kx || c->H % p.ky) return fail(c, SWR_ERR_INVALID_ARG, "the render target's width and height must be multiples of the resolve factors");
    // a post program may fetch any pixel of the frame: a neighbour across a band's edge is not in this context
    if (p.posted && delivery && (c->band_ty0 != 0 || band_rows(c) != c->H))
        return fail(c, SWR_ERR_UNSUPPORTED, "the context holds only a band of its frame (swr_set_band*): post programs need the whole frame");
    return SWR_OK;
}
int payload_width(const swr_context* c, const Payload& p) { return std::max(0, c->W) / p.kx; }
int payload_rows(const swr_context* c, const Payload& p) { return band_rows(c) / p.ky; }
size_t payload_pixels(const swr_context* c, const Payload& p) { return (size_t)payload_width(c, p) * (size_t)payload_rows(c, p); }
size_t payload_bytes(const swr_context* c, const Payload& p) { return payload_pixels(c, p) * payload_bpp(p); }

// the delivery kernels' launch: one thread per output pixel, SWR_RESOLVE_BLOCK_X x _Y of them per block (swr_deliver.hip.h)
struct DeliverShape { dim3 grid, block; };
DeliverShape deliver_shape(uint32_t ow, uint32_t orows) {       // a frame is at most 65535 x 65535
    return { dim3((ow + SWR_RESOLVE_BLOCK_X - 1) / SWR_RESOLVE_BLOCK_X, (orows + SWR_RESOLVE_BLOCK_Y - 1) / SWR_RESOLVE_BLOCK_Y),
             dim3(SWR_RESOLVE_BLOCK_X, SWR_RESOLVE_BLOCK_Y) };
}

using ResolveKernel = void (*)(const float4*, float*, int, int);
ResolveKernel resolve_kernel(int kx, int ky) {
    return with_factors<ResolveKernel>(kx, ky, [](auto x, auto y) -> ResolveKernel { return k_resolve_rgb<decltype(x)::value, decltype(y)::value>; });
}
using Present8Kernel = void (*)(const float4*, uint8_t*, uint32_t, uint32_t);
template <int BPP> Present8Kernel present8_kernel(int kx, int ky) {
    return with_factors<Present8Kernel>(kx, ky, [](auto x, auto y) -> Present8Kernel { return k_present8<decltype(x)::value, decltype(y)::value, BPP>; });
}

int launch_present8(swr_context* c, const Payload& p, uint8_t* d_out) {
    const uint32_t ow = (uint32_t)payload_width(c, p), orows = (uint32_t)payload_rows(c, p);
    const auto [grid, block] = deliver_shape(ow, orows);
    const Present8Kernel k = p.format == PAYLOAD_RGB8 ? present8_kernel<3>(p.kx, p.ky) : present8_kernel<4>(p.kx, p.ky);
    hipLaunchKernelGGL(k, grid, block, 0, c->stream, (const float4*)c->color, d_out, ow, orows);
    SWR_HIP(c, hipGetLastError());
    return SWR_OK;
}

using ResolveRgbaKernel = void (*)(const float4*, float4*, uint32_t, uint32_t);
ResolveRgbaKernel resolve_rgba_kernel(int kx, int ky) {
    return with_factors<ResolveRgbaKernel>(kx, ky, [](auto x, auto y) -> ResolveRgbaKernel { return k_resolve_rgba<decltype(x)::value, decltype(y)::value>; });
}

// a program's texture slots as they are NOW, in the encoding a draw records (swr_flush.h: h < 0 the bilinear filter, w < 0 as well
// the block-linear copy)
void capture_post_textures(const PostProg* post, PostConstants& k) {
    for (int i = 0; i < SWR_POST_TEXTURES; ++i) k.tex[i] = texture_slot_of(post->tex[i]);
}

// A post program over s's whole frame, on c's stream (s == c for a present): the frame resolved into s's RGBA plane (under (1, 1) the
// frame is that plane), then k_post `fn` of the program over it, with the constants and the texture slots as they are now.
// d_blocked: the texel formats' second destination, or null.
int launch_post_over(swr_context* c, swr_context* s, const PostProg* post, PostKernel fn, int kx, int ky, void* d_out, uint32_t* d_blocked) {
    const uint32_t ow = (uint32_t)(std::max(0, s->W) / kx), orows = (uint32_t)(band_rows(s) / ky);
    const auto [grid, block] = deliver_shape(ow, orows);
    const float4* plane = s->color;
    if (kx != 1 || ky != 1) {
        const size_t bytes = (size_t)ow * orows * sizeof(float4);
        if (s->post_plane.cap < bytes) {
            // growing frees the old block: an earlier k_post may still read it (first use / after a resize only).  s's stream is behind
            // every such reader: its own presents, and another context's swr_texture_update_from_post through rtt_done_ev
            SWR_HIP(c, hipStreamSynchronize(s->stream));
            int rc = ensure(c, s->post_plane, bytes); if (rc) return rc;
        }
        hipLaunchKernelGGL(resolve_rgba_kernel(kx, ky), grid, block, 0, c->stream, (const float4*)s->color, s->post_plane.as<float4>(), ow, orows);
        SWR_HIP(c, hipGetLastError());
        plane = s->post_plane.as<float4>();
    }
    const float* depth = s->depth;
    uint32_t w = ow, rows = orows;
    PostConstants constants = post->constants;
    capture_post_textures(post, constants);
    constants.blocked = d_blocked;
    void* args[] = { &plane, &depth, &d_out, &w, &rows, &kx, &ky, &constants };
    SWR_HIP(c, hipModuleLaunchKernel(post->fn[fn], grid.x, grid.y, 1, block.x, block.y, 1, 0, c->stream, args, nullptr));
    return SWR_OK;
}
int launch_post(swr_context* c, const Payload& p, void* d_out) {
    const PostKernel fn = p.format == PAYLOAD_RGB32F ? POST_RGB32F : p.format == PAYLOAD_RGB8 ? POST_RGB8 : POST_RGBX8;
    return launch_post_over(c, c, p.post, fn, p.kx, p.ky, d_out, nullptr);
}

// the payload of the band's colour plane in device memory (4-byte aligned), on the context's stream (checked, and not empty)
int launch_payload(swr_context* c, const Payload& p, void* d_out) {
    if (p.posted) return launch_post(c, p, d_out);
    if (p.format != PAYLOAD_RGB32F) return launch_present8(c, p, (uint8_t*)d_out);
    float* d_rgb = (float*)d_out;
    if (!p.resolve) return launch_flatten(c, d_rgb, band_pixels(c));
    const int ow = payload_width(c, p), orows = payload_rows(c, p);
    const auto [grid, block] = deliver_shape((uint32_t)ow, (uint32_t)orows);
    hipLaunchKernelGGL(resolve_kernel(p.kx, p.ky), grid, block, 0, c->stream, (const float4*)c->color, d_rgb, ow, orows);
    SWR_HIP(c, hipGetLastError());
    return SWR_OK;
}

// swr_flatten_rgb_device / swr_resolve_rgb_device / swr_resolve_rgb8_device / swr_post_device [_async].  Stream order puts the payload kernel after the frame's kernels; a batch that
// has to be replayed (optimistic flush) is replayed by the caller's swr_sync BEFORE the result is consumed -- and then the kernel must
// run again, which sync does not know about: so `validate` first (cheap when nothing overflowed: one pinned-flag read after the stream
// drains)
int payload_device(swr_context* c, const Payload& p, void* d_out, bool validate) {
    if (!d_out) return fail(c, SWR_ERR_INVALID_ARG, "the device destination is null");
    // k_present8 stores whole dwords (the float kernels' float stores have always needed this much)
    if ((p.format != PAYLOAD_RGB32F || p.posted) && ((uintptr_t)d_out & 3u)) return fail(c, SWR_ERR_INVALID_ARG, "the device destination must be 4-byte aligned");
    int rc = payload_check(c, p); if (rc) return rc;
    if ((rc = flush_locked(c))) return rc;
    if (!payload_pixels(c, p)) return SWR_OK;
    if (validate && (rc = sync_locked(c))) return rc;
    return launch_payload(c, p, d_out);
}

// swr_readback_rgb / swr_readback_rgb_resolved / swr_readback_rgb8 / swr_readback_post: the payload into host memory (of any alignment: the copy comes
// from the scratch block), between two host syncs
int payload_readback(swr_context* c, const Payload& p, void* out) {
    if (!out) return fail(c, SWR_ERR_INVALID_ARG, "the destination is null");
    int rc = payload_check(c, p); if (rc) return rc;
    if ((rc = flush_and_sync_locked(c))) return rc;
    const size_t bytes = payload_bytes(c, p);
    if (!bytes) return SWR_OK;
    if ((rc = ensure(c, c->d_scratch, bytes))) return rc;
    if ((rc = launch_payload(c, p, c->d_scratch.p))) return rc;
    SWR_HIP(c, hipMemcpyAsync(out, c->d_scratch.p, bytes, hipMemcpyDeviceToHost, c->stream));
    return sync_locked(c);
}

// swr_present_rgb_async / swr_present_rgb_resolved_async / swr_present_rgb8_async / swr_present_post_async: every kind shares the two slots, the tickets and
// the staging buffers (sized in bytes); a ticket does not say which kind it was
int payload_present(swr_context* c, const Payload& p, void* out, uint64_t* ticket) {
    if (!out || !ticket) return fail(c, SWR_ERR_INVALID_ARG, "the destination or ticket is null");
    int rc = payload_check(c, p); if (rc) return rc;
    if ((rc = flush_locked(c))) return rc;
    const size_t bytes = payload_bytes(c, p);
    const int slot = (int)(c->next_ticket & 1ull);
    if (!c->copy_stream) SWR_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        if (!c->present_flat[i]) SWR_HIP(c, hipEventCreateWithFlags(&c->present_flat[i], hipEventDisableTiming));
        if (!c->present_done[i]) SWR_HIP(c, hipEventCreateWithFlags(&c->present_done[i], hipEventDisableTiming));
    }
    // the slot's previous copy (two presents ago) must be over before its staging buffer is overwritten: back-pressure, not
    // steady-state waiting -- a caller that waits for ticket i before it presents frame i + 2 never blocks here
    if (c->present_ticket[slot]) {
        SWR_HIP(c, hipEventSynchronize(c->present_done[slot]));
        // the ticket is dropped unwaited: if a batch at or before that present poisoned itself, its pixels were stale -- remember it
        // for the swr_present_wait that may still come
        bool stale = false;
        if ((rc = present_is_stale(c, slot, stale))) return rc;
        if (stale) c->stale_dropped[slot] = c->present_ticket[slot];
        c->present_ticket[slot] = 0;
    }
    if (bytes) {
        if (c->present_buf[slot].cap < bytes) {
            // growing frees the old block: make sure neither stream still uses it (first frame / after a resize only)
            SWR_HIP(c, hipStreamSynchronize(c->copy_stream));
            if ((rc = ensure(c, c->present_buf[slot], bytes))) return rc;
        }
        if ((rc = launch_payload(c, p, c->present_buf[slot].p))) return rc;
    }
    SWR_HIP(c, hipEventRecord(c->present_flat[slot], c->stream));
    SWR_HIP(c, hipStreamWaitEvent(c->copy_stream, c->present_flat[slot], 0));
    if (bytes) SWR_HIP(c, hipMemcpyAsync(out, c->present_buf[slot].p, bytes, hipMemcpyDeviceToHost, c->copy_stream));
    SWR_HIP(c, hipEventRecord(c->present_done[slot], c->copy_stream));
    c->present_ticket[slot] = ++c->next_ticket;
    c->present_seq[slot] = c->next_seq - 1u;
    *ticket = c->present_ticket[slot];
    return SWR_OK;
}

// swr_readback / swr_upload: the band's planes (either may be null) to or from the host, between two host syncs: optimistic batches are
// validated BEFORE pixels are observed or replaced
int planes_transfer(swr_context* c, float* color, float* depth, bool to_host) {
    int rc = flush_and_sync_locked(c); if (rc) return rc;
    const size_t n = band_pixels(c);
    const hipMemcpyKind kind = to_host ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice;
    if (n && color) SWR_HIP(c, hipMemcpyAsync(to_host ? (void*)color : c->color, to_host ? (void*)c->color : color, n * 16, kind, c->stream));
    if (n && depth) SWR_HIP(c, hipMemcpyAsync(to_host ? depth : c->depth, to_host ? c->depth : depth, n * 4, kind, c->stream));
    return sync_locked(c);
}

// swr_get / set_pixel / depth: one pixel of `plane` (`bytes` each) to or from the host, after everything recorded has been rendered
// and validated and with a wait behind the copy; a pixel outside the band is left alone
int pixel_transfer(swr_context* c, int x, int y, void* plane, size_t bytes, void* host, bool to_host) {
    if (x < 0 || x >= c->W || band_local_pixel_row(c, y) < 0) return SWR_OK;
    int rc = flush_and_sync_locked(c); if (rc) return rc;
    void* dev = static_cast<char*>(plane) + ((size_t)band_local_pixel_row(c, y) * c->W + x) * bytes;
    if (to_host) SWR_HIP(c, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    else SWR_HIP(c, hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, c->stream));
    return sync_locked(c);
}

// swr_texture_update_from_frame: k_frame_to_texture by factors, alpha mode and whether the block-linear copy exists
using RttKernel = void (*)(const float4*, uint32_t*, uint32_t*, uint32_t, uint32_t);
RttKernel rtt_kernel(int kx, int ky, bool alpha, bool blocked) {
    using K = RttKernel;
    return with_flag<K>(alpha, [&](auto a) -> K { return with_flag<K>(blocked, [&](auto b) -> K { return with_factors<K>(kx, ky, [](auto x, auto y) -> K {
        return k_frame_to_texture<decltype(x)::value, decltype(y)::value, decltype(a)::value, decltype(b)::value>; }); }); });
}

// swr_texture_update_from_depth: k_depth_to_texture by factors and whether the block-linear copy exists (the reduction is an argument)
using DepthTextureKernel = void (*)(const float*, uint32_t*, uint32_t*, uint32_t, uint32_t, int);
DepthTextureKernel depth_texture_kernel(int kx, int ky, bool blocked) {
    using K = DepthTextureKernel;
    return with_flag<K>(blocked, [&](auto b) -> K { return with_factors<K>(kx, ky, [](auto x, auto y) -> K {
        return k_depth_to_texture<decltype(x)::value, decltype(y)::value, decltype(b)::value>; }); });
}

// does the call suit the texture's format?  (the texels of both formats are 4 bytes: nothing else tells them apart)
int texture_format_check(swr_context* c, const swr_texture* t, int format) {
    if (t->format == format) return SWR_OK;
    return fail(c, SWR_ERR_INVALID_ARG, format == SWR_TEXTURE_FORMAT_DEPTH32F ? "the texture is not a depth texture (SWR_TEXTURE_FORMAT_DEPTH32F): this call reads or writes depth words"
                                                                              : "the texture is a depth texture (SWR_TEXTURE_FORMAT_DEPTH32F): use the swr_texture_*_depth calls");
}

// MIP CHAINS.  offset[l] of a w x h texture's chain of `levels` levels: level l's first texel in the tail
void mip_offsets(const swr_texture* t, int levels, uint32_t* offset) {
    uint32_t at = 0;
    offset[0] = 0;
    for (int l = 1; l < levels; ++l) { offset[l] = at; at += (uint32_t)mip_level_side(t->w, l) * (uint32_t)mip_level_side(t->h, l); }
}
// the record in front of one of t's texel arrays (d_rgba or d_blocked) as t's chain is now, on the context's stream: in front of the
// texels' own upload at creation, behind the flushed draws (which read the old record) when a chain appears
hipError_t texture_header_write(swr_context* c, const swr_texture* t, uint8_t* texels) {
    TextureHeader h = {};
    h.levels = (uint32_t)t->levels;
    h.tail = t->levels > 1 ? t->d_tail : nullptr;
    mip_offsets(t, t->levels, h.offset);
    hipLaunchKernelGGL(k_texture_header, dim3(1), dim3(64), 0, c->stream, reinterpret_cast<uint32_t*>(texels - SWR_TEXTURE_HEADER_BYTES), h);
    return hipGetLastError();
}
// levels 1 .. L - 1 from the row-major level 0, on the context's stream: two levels per launch (k_mip_downsample<true>) wherever the
// source level's sides are multiples of 4 and the alignments of its 16-byte loads and 8-byte stores hold, else one
int mip_generate(swr_context* c, const swr_texture* t) {
    uint32_t off[SWR_TEXTURE_MAX_LEVELS];
    mip_offsets(t, t->levels, off);
    uint32_t* tail = reinterpret_cast<uint32_t*>(t->d_tail);
    for (int l = 0; l + 1 < t->levels;) {
        const uint32_t sw = (uint32_t)mip_level_side(t->w, l), sh = (uint32_t)mip_level_side(t->h, l);
        const uint32_t* src = l == 0 ? reinterpret_cast<const uint32_t*>(t->d_rgba) : tail + off[l];
        const bool two = l + 2 < t->levels && (sw & 3u) == 0 && (sh & 3u) == 0 && (l == 0 || (off[l] & 3u) == 0) && (off[l + 1] & 1u) == 0;
        if (two) {
            const auto [grid, block] = deliver_shape(sw >> 2, sh >> 2);
            hipLaunchKernelGGL(k_mip_downsample<true>, grid, block, 0, c->stream, src, sw, sh, tail + off[l + 1], tail + off[l + 2]);
        } else {
            const auto [grid, block] = deliver_shape((uint32_t)mip_level_side(t->w, l + 1), (uint32_t)mip_level_side(t->h, l + 1));
            hipLaunchKernelGGL(k_mip_downsample<false>, grid, block, 0, c->stream, src, sw, sh, tail + off[l + 1], (uint32_t*)nullptr);
        }
        SWR_HIP(c, hipGetLastError());
        l += two ? 2 : 1;
    }
    // Vertex programs sample textures too, and a pipelined batch runs its k_vertex_user on the front stream: the next such front end
    // starts behind this point of the raster stream (the hand-over an unpipelined batch leaves, execute_batch).  Front ends flushed
    // EARLIER need nothing: the raster stream already waits for each of them (front_done), so these writes are behind them
    if (c->pipelining && c->front_stream && c->r_front_ev) {
        SWR_HIP(c, hipEventRecord(c->r_front_ev, c->stream));
        c->r_front_pending = true;
    }
    return SWR_OK;
}

// swr_texture_create / _create_target / _create_depth: w x h 4-byte texels on the context's stream, the caller's or (texels null) the
// format's empty word: zeros, or float.MinValue.  The array's header (no chain: one level) goes in front of it on the same stream.
int texture_create(swr_context* c, const void* texels, int w, int h, swr_texture** out, const char* what_failed, int format = SWR_TEXTURE_FORMAT_RGBA8) {
    if (w <= 0 || h <= 0 || !out) return fail(c, SWR_ERR_INVALID_ARG, "bad texture arguments");
    if ((uint64_t)w * (uint64_t)h >= (1ull << 30)) return fail(c, SWR_ERR_UNSUPPORTED, "textures of 2^30 texels or more are not supported (32-bit texel index)");
    swr_texture* t = new swr_texture();
    t->w = w; t->h = h; t->format = format;
    const size_t bytes = (size_t)w * h * 4;
    const float empty_depth = SWR_FLOAT_MINVALUE;
    int empty = 0;
    if (format == SWR_TEXTURE_FORMAT_DEPTH32F) memcpy(&empty, &empty_depth, 4);
    hipError_t e = texels_alloc(&t->d_rgba, bytes);
    if (e == hipSuccess) e = texture_header_write(c, t, t->d_rgba);
    if (e == hipSuccess) e = texels ? hipMemcpyAsync(t->d_rgba, texels, bytes, hipMemcpyHostToDevice, c->stream)
                                    : hipMemsetD32Async((hipDeviceptr_t)t->d_rgba, empty, (size_t)w * h, c->stream);
    if (e != hipSuccess) {
        texels_free(t->d_rgba);
        delete t;
        c->err = std::string(what_failed) + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? SWR_ERR_OOM : SWR_ERR_HIP;
    }
    *out = t;
    return SWR_OK;
}

// What a texture is updated from: src's colour plane (swr_texture_update_from_frame), program post_id of src between the resolve and
// the quantiser (_from_post), or src's depth plane (_from_depth).  mode: the alpha mode, or the depth reduction.
enum UpdateFrom { FROM_FRAME, FROM_POST, FROM_DEPTH };
// by_face: one face of a cube (swr_texture_update_face_from_*), `face` as the caller gave it -- the same kernels
// over the face's n x n texels, which start face * n * n texels into the row-major array and into the block-linear copy alike
struct TextureUpdate { UpdateFrom from; int kx, ky, mode, post_id; int face = 0; bool by_face = false; };

// Both contexts' mutexes are held (one when src == c).  Nothing here waits for a stream (but a first use or growth of src's resolved
// plane, launch_post_over).
int texture_update(swr_context* c, swr_texture* t, swr_context* src, const TextureUpdate& u) {
    const int kx = u.kx, ky = u.ky;
    const bool posted = u.from == FROM_POST, from_depth = u.from == FROM_DEPTH;
    if (!t) return fail(c, SWR_ERR_INVALID_ARG, "texture is null");
    if (u.by_face && !t->cube) return fail(c, SWR_ERR_INVALID_ARG, "the texture is not a cube map (swr_texture_create_cube, swr_texture_create_cube_depth)");
    if (u.by_face && (u.face < 0 || u.face > 5)) return fail(c, SWR_ERR_INVALID_ARG, "face must be 0 .. 5 (+X, -X, +Y, -Y, +Z, -Z)");
    const int tw = t->w, th = u.by_face ? t->w : t->h;                             // what the kernel writes: the texture, or one face of it
    const size_t first = u.by_face ? (size_t)u.face * (size_t)t->w * (size_t)t->w : 0;   // its first texel, in texels
    if (!from_depth && u.mode != SWR_TEXTURE_ALPHA_OPAQUE && u.mode != SWR_TEXTURE_ALPHA_KEEP)
        return fail(c, SWR_ERR_INVALID_ARG, "alpha_mode must be SWR_TEXTURE_ALPHA_OPAQUE (0) or SWR_TEXTURE_ALPHA_KEEP (1)");
    if (from_depth && u.mode != SWR_DEPTH_REDUCE_MAX && u.mode != SWR_DEPTH_REDUCE_MIN && u.mode != SWR_DEPTH_REDUCE_FIRST)
        return fail(c, SWR_ERR_INVALID_ARG, "reduce must be SWR_DEPTH_REDUCE_MAX (0), SWR_DEPTH_REDUCE_MIN (1) or SWR_DEPTH_REDUCE_FIRST (2)");
    if (int rc = texture_format_check(c, t, from_depth ? SWR_TEXTURE_FORMAT_DEPTH32F : SWR_TEXTURE_FORMAT_RGBA8)) return rc;
    if (!resolve_factor_ok(kx) || !resolve_factor_ok(ky)) return fail(c, SWR_ERR_INVALID_ARG, "resolve factors must be 1, 2, 4 or 8");
    if (src->device != c->device) return fail(c, SWR_ERR_UNSUPPORTED, "the source frame lives on another device");
    if (src->W > 0 && src->H > 0 && (src->band_ty0 != 0 || band_rows(src) != src->H))
        return fail(c, SWR_ERR_UNSUPPORTED, "the source context holds only a band of its frame (swr_set_band*)");
    if ((long long)tw * kx != (long long)src->W || (long long)th * ky != (long long)src->H)
        return fail(c, SWR_ERR_INVALID_ARG, u.by_face ? "the source frame must measure n * kx by n * ky for a cube map of side n"
                                                      : "the source frame must measure texture width * kx by texture height * ky");
    const PostProg* post = nullptr;
    if (posted) {
        const auto it = src->posts.find(u.post_id);
        if (it == src->posts.end()) return fail(c, SWR_ERR_INVALID_ARG, "unknown or destroyed post program id");
        post = it->second.get();
        for (const swr_texture* bound : post->tex)
            if (bound == t) return fail(c, SWR_ERR_INVALID_ARG, "the texture is bound to a slot of the program: a pass may not sample the texture it writes");
    }
    // (k_depth_to_texture loads kx words at once; the context's own plane is an allocation's start)
    if (from_depth && ((uintptr_t)src->depth & 15u)) return fail(c, SWR_ERR_INVALID_ARG, "the source's bound depth buffer must be 16-byte aligned");
    int rc;
    // the frame is complete behind this point of src's stream, and c's recorded draws are in front of the kernel on c's stream: they
    // sample the old texels (raster kernels and k_texture_sample, the only readers of a texture, run on `stream`, never on the front stream)
    if ((rc = flush_locked(src))) { if (src != c) c->err = src->err; return rc; }
    if (src != c && (rc = flush_locked(c))) return rc;
    if (src != c && src->stream != c->stream) {
        if (!src->rtt_frame_ev) SWR_HIP(c, hipEventCreateWithFlags(&src->rtt_frame_ev, hipEventDisableTiming));
        SWR_HIP(c, hipEventRecord(src->rtt_frame_ev, src->stream));
        SWR_HIP(c, hipStreamWaitEvent(c->stream, src->rtt_frame_ev, 0));
    }
    const bool blocked = t->d_blocked != nullptr;         // (made by swr_texture_set_filter: both sides are multiples of 4)
    uint32_t* const d_rgba = reinterpret_cast<uint32_t*>(t->d_rgba) + first;
    uint32_t* const d_blocked = blocked ? reinterpret_cast<uint32_t*>(t->d_blocked) + first : nullptr;
    if (post) {
        // (the resolve writes src's plane and the program may sample src's textures: both behind rtt_frame_ev, and src's later work --
        // a present, an update of such a texture -- behind rtt_done_ev)
        if ((rc = launch_post_over(c, src, post, u.mode == SWR_TEXTURE_ALPHA_KEEP ? POST_TEXELS_KEEP : POST_TEXELS_OPAQUE, kx, ky, d_rgba, d_blocked))) return rc;
    } else {
        const auto [grid, block] = deliver_shape((uint32_t)tw, (uint32_t)th);
        if (from_depth)
            hipLaunchKernelGGL(depth_texture_kernel(kx, ky, blocked), grid, block, 0, c->stream, (const float*)src->depth,
                               d_rgba, d_blocked, (uint32_t)tw, (uint32_t)th, u.mode);
        else
            hipLaunchKernelGGL(rtt_kernel(kx, ky, u.mode == SWR_TEXTURE_ALPHA_KEEP, blocked), grid, block, 0, c->stream, (const float4*)src->color,
                               d_rgba, d_blocked, (uint32_t)tw, (uint32_t)th);
        SWR_HIP(c, hipGetLastError());
    }
    // a chain is a property of the texture: its levels follow the new level 0, on the same stream (a texture without one: nothing)
    if (t->levels > 1 && (rc = mip_generate(c, t))) return rc;
    if (src != c && src->stream != c->stream) {
        // src's next raster, clear or upload may not overwrite the frame under the kernel
        if (!c->rtt_done_ev) SWR_HIP(c, hipEventCreateWithFlags(&c->rtt_done_ev, hipEventDisableTiming));
        SWR_HIP(c, hipEventRecord(c->rtt_done_ev, c->stream));
        SWR_HIP(c, hipStreamWaitEvent(src->stream, c->rtt_done_ev, 0));
    }
    return SWR_OK;
}

// swr_program_validate* / swr_post_validate: the compiler's messages, NUL-terminated and truncated to the caller's buffer
void copy_log(const std::string& msg, char* log, int log_len) {
    if (!log || log_len <= 0) return;
    const size_t n = std::min(msg.size(), (size_t)log_len - 1);
    memcpy(log, msg.data(), n); log[n] = '\0';
}
}  // namespace

extern "C" {

int swr_abi_version(void) { return SWR_ABI_VERSION; }

// set by csrc/Makefile: the compiler's version line and bench.py --print-src-hash (sha256 over the kernel sources)
#ifndef SWR_BUILD_HIPCC
#define SWR_BUILD_HIPCC "unknown"
#endif
#ifndef SWR_BUILD_SRC_SHA
#define SWR_BUILD_SRC_SHA "unknown"
#endif
#ifndef SWR_BUILD_EXTRA
#define SWR_BUILD_EXTRA ""
#endif
const char* swr_build_info(void) {
    return "hipcc=" SWR_BUILD_HIPCC "; csrc_sha256=" SWR_BUILD_SRC_SHA "; fma=" SWR_STR(SWR_NUMERICS_FMA) "; dot=" SWR_STR(SWR_DOT_PAIRWISE) "; extra=" SWR_BUILD_EXTRA;
}

int swr_numerics_mode(int* fma, int* dot_order) {
    if (!fma || !dot_order) return SWR_ERR_INVALID_ARG;
    *fma = SWR_NUMERICS_FMA; *dot_order = SWR_DOT_PAIRWISE;
    return SWR_OK;
}

int swr_set_transform_fma(swr_context* c, int transform_fused, int transform_normal_fused) {
    if (!c) return SWR_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock_(c->mu);
    // (draws recorded so far keep the model they were recorded under: DrawParams::nm_flags)
    c->nm_flags = (transform_fused ? SWR_NM_TRANSFORM_FMA : 0u) | (transform_normal_fused ? SWR_NM_TRANSFORM_NORMAL_FMA : 0u);
    return SWR_OK;
}

int swr_get_transform_fma(swr_context* c, int* transform_fused, int* transform_normal_fused) {
    if (!c || !transform_fused || !transform_normal_fused) return SWR_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock_(c->mu);
    *transform_fused = (c->nm_flags & SWR_NM_TRANSFORM_FMA) ? 1 : 0;
    *transform_normal_fused = (c->nm_flags & SWR_NM_TRANSFORM_NORMAL_FMA) ? 1 : 0;
    return SWR_OK;
}

const char* swr_last_error(const swr_context* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int swr_create(int device_id, swr_context** out) {
    if (!out) { g_create_error = "out is null"; return SWR_ERR_INVALID_ARG; }
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        g_create_error = std::string("no HIP device available: ") + hipGetErrorString(e) + " (this backend has no CPU fallback)";
        return SWR_ERR_NO_DEVICE;
    }
    if (device_id < 0 || device_id >= n) { g_create_error = "device id out of range"; return SWR_ERR_INVALID_ARG; }
    if ((e = hipSetDevice(device_id)) != hipSuccess) { g_create_error = hipGetErrorString(e); return SWR_ERR_HIP; }
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess) { g_create_error = hipGetErrorString(e); return SWR_ERR_HIP; }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_create_error = std::string("device is ") + prop.gcnArchName + "; libswr_hip.so carries gfx950 code objects only";
        return SWR_ERR_NO_DEVICE;
    }
    swr_context* c = new swr_context();
    c->device = device_id;
    snprintf(c->dev_name, sizeof c->dev_name, "%s (%s)", prop.name, prop.gcnArchName);
    if ((e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess) {
        g_create_error = hipGetErrorString(e); delete c; return SWR_ERR_HIP;
    }
    c->stream = c->own_stream;
    if (ensure_front_stream(c)) { g_create_error = c->err; (void)hipStreamDestroy(c->own_stream); delete c; return SWR_ERR_HIP; }
    { const char* sf = getenv("SWR_SYNC_FLUSH"); c->sync_flush = sf && sf[0] == '1'; }
#ifdef SWR_TEST_HOOKS       // libswr_hip_test.so only: the FILL pass of optimistic flushes sees a list of n entries (forces the list-overflow path)
    { const char* df = getenv("SWR_DEBUG_FILL_CAPACITY"); c->debug_fill_capacity = df ? (uint32_t)strtoul(df, nullptr, 10) : 0u; }
#endif
    int rc = ensure(c, c->d_counters, 65 * sizeof(Counters));
    if (!rc) rc = ensure(c, c->d_ctrl, 64);
    if (!rc && hipHostMalloc((void**)&c->host_poison, 64, hipHostMallocDefault) != hipSuccess) rc = SWR_ERR_OOM;
    if (!rc) { memset(c->host_poison, 0, 64); rc = reset_ctrl(c); }
    if (!rc) rc = ensure(c, c->d_total, 256 + 4096 * 8);
    if (!rc && hipMemsetAsync(c->d_total.p, 0, 256 + 4096 * 8, c->stream) != hipSuccess) rc = SWR_ERR_HIP;
    if (!rc && hipMemsetAsync(c->d_counters.p, 0, 65 * sizeof(Counters), c->stream) != hipSuccess) rc = SWR_ERR_HIP;
    if (rc) { g_create_error = c->err; swr_destroy(c); return rc; }
    *out = c;
    return SWR_OK;
}

void swr_destroy(swr_context* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->front_stream) (void)hipStreamSynchronize(c->front_stream);
    for (auto& d : c->draws) if (d.mesh && d.mesh->transient) c->garbage.push_back(d.mesh);
    for (auto& b : c->inflight) retire_batch(c, b);
    c->inflight.clear();
    collect_spans(c);
    free_garbage(c);
    c->draws.clear();
    c->progs.clear();                        // (streams idle: the modules unload here)
    c->posts.clear();
    for (swr_mesh* m : c->mesh_pool) destroy_mesh(m);
    c->mesh_pool.clear();
    for (hipEvent_t e : c->event_pool) (void)hipEventDestroy(e);
    for (auto& fs : c->slots) { release(fs.host); if (fs.done) (void)hipEventDestroy(fs.done); }
    if (c->host_poison) (void)hipHostFree(c->host_poison);
    if (c->copy_stream) { (void)hipStreamSynchronize(c->copy_stream); (void)hipStreamDestroy(c->copy_stream); }
    if (c->ray_stream) { (void)hipStreamSynchronize(c->ray_stream); (void)hipStreamDestroy(c->ray_stream); }
    release(c->ray_host);
    for (auto& ps : c->palettes) { release(ps.host); release(ps.dev); if (ps.done) (void)hipEventDestroy(ps.done); }
    c->pose_events.clear();
    if (c->rtt_frame_ev) (void)hipEventDestroy(c->rtt_frame_ev);
    if (c->rtt_done_ev) (void)hipEventDestroy(c->rtt_done_ev);
    for (int i = 0; i < 2; ++i) {
        if (c->present_flat[i]) (void)hipEventDestroy(c->present_flat[i]);
        if (c->present_done[i]) (void)hipEventDestroy(c->present_done[i]);
        release(c->present_buf[i]);
    }
    DevBuf* bufs[] = { &c->post_plane, &c->own_color, &c->own_depth, &c->d_slot_tb, &c->d_want, &c->d_ctrl, &c->d_pair_tile, &c->d_tile_list, &c->d_tile_stats,
                       &c->d_counters, &c->d_total, &c->d_scratch, &c->d_ray, &c->d_ray_best, &c->d_char };
    for (DevBuf* b : bufs) release(*b);
    for (auto& s : c->sets) {
        DevBuf* sb[] = { &s.d_upload, &s.d_vout, &s.d_vnorm, &s.d_recs, &s.d_masks, &s.d_pcounts, &s.d_pair_refs, &s.d_tile_count, &s.d_tile_start, &s.d_order };
        for (DevBuf* b : sb) release(*b);
        if (s.front_done) (void)hipEventDestroy(s.front_done);
        if (s.raster_done) (void)hipEventDestroy(s.raster_done);
    }
    if (c->front_stream) (void)hipStreamDestroy(c->front_stream);
    if (c->f_tail_ev) (void)hipEventDestroy(c->f_tail_ev);
    if (c->r_front_ev) (void)hipEventDestroy(c->r_front_ev);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

#define SWR_ENTER(c)                                   \
    if (!(c)) return SWR_ERR_INVALID_ARG;              \
    std::lock_guard<std::mutex> lock_((c)->mu);        \
    (void)hipSetDevice((c)->device)

int swr_resize(swr_context* c, int width, int height) {
    SWR_ENTER(c);
    if (width > 65535 || height > 65535) return fail(c, SWR_ERR_INVALID_ARG, "render target larger than 65535");
    if (c->geometry_applied && width == c->W && height == c->H) return SWR_OK;      // nothing changes: no flush, no wait
    int rc = flush_and_sync_locked(c); if (rc) return rc;
    c->W = width; c->H = height;
    c->geometry_applied = true;
    return apply_geometry(c);
}

int swr_set_band(swr_context* c, int first_tile_row, int n_tile_rows) {
    SWR_ENTER(c);
    const bool want_band = !(first_tile_row < 0 || n_tile_rows < 0);
    if (c->il_k == 0 && want_band == c->band_set && (!want_band || (first_tile_row == c->band_first && n_tile_rows == c->band_count)))
        return SWR_OK;                                                             // the same band again: no flush, no wait
    int rc = flush_and_sync_locked(c); if (rc) return rc;
    c->il_k = 0; c->il_world = 1; c->il_rank = 0;
    c->band_set = want_band;
    if (want_band) { c->band_first = first_tile_row; c->band_count = n_tile_rows; }
    return apply_geometry(c);
}

int swr_set_band_interleaved(swr_context* c, int rank, int world, int stripe_tile_rows) {
    SWR_ENTER(c);
    if (world < 1 || rank < 0 || rank >= world || stripe_tile_rows < 1) return fail(c, SWR_ERR_INVALID_ARG, "bad interleaved band arguments");
    if (c->il_k == stripe_tile_rows && c->il_world == world && c->il_rank == rank) return SWR_OK;     // unchanged: no flush, no wait
    int rc = flush_and_sync_locked(c); if (rc) return rc;
    c->band_set = false;
    c->il_k = stripe_tile_rows; c->il_world = world; c->il_rank = rank;
    return apply_geometry(c);
}

int swr_bind_framebuffer(swr_context* c, void* color, void* depth) {
    SWR_ENTER(c);
    if ((color == nullptr) != (depth == nullptr)) return fail(c, SWR_ERR_INVALID_ARG, "bind both colour and depth, or neither");
    // draws recorded so far belong to the buffers bound so far: launch them (asynchronously -- a batch remembers its
    // target, so neither the switch nor a later replay needs the stream to drain; a frame loop that alternates two band
    // buffers pays no host round trip here)
    int rc = flush_locked(c); if (rc) return rc;
    // back to internal storage: apply_geometry may have to (re)allocate it, which must not happen under batches that could
    // still be replayed against the old allocation -- drain and validate first (binding caller memory never allocates)
    if (!color && (rc = sync_locked(c))) return rc;
    c->ext_color = color; c->ext_depth = depth;
    return apply_geometry(c);
}

int swr_set_stream(swr_context* c, void* s) {
    SWR_ENTER(c);
    int rc = flush_and_sync_locked(c); if (rc) return rc;
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return SWR_OK;
}

int swr_clear_color(swr_context* c, const float rgba[4]) {
    SWR_ENTER(c);
    if (!rgba) return fail(c, SWR_ERR_INVALID_ARG, "rgba is null");
    if (!c->draws.empty()) { int rc = flush_locked(c); if (rc) return rc; }
    memcpy(c->clear_rgba, rgba, 16);
    c->pend_clear_color = true;
    return SWR_OK;
}

int swr_clear_depth(swr_context* c) {
    SWR_ENTER(c);
    if (!c->draws.empty()) { int rc = flush_locked(c); if (rc) return rc; }
    c->pend_clear_depth = true;
    return SWR_OK;
}

int swr_flush(swr_context* c) { SWR_ENTER(c); return flush_locked(c); }

int swr_set_pipelining(swr_context* c, int mode) {
    SWR_ENTER(c);
    if (mode < 0 || mode > 2) return fail(c, SWR_ERR_INVALID_ARG, "pipelining mode must be 0 (off), 1 (every batch) or 2 (only frames of up to 2^15 tiles or batches of up to 2^17 triangles)");
    if (mode == c->pipelining) return SWR_OK;
    int rc = flush_and_sync_locked(c); if (rc) return rc;   // nothing in flight while the streams and the set in use change
    c->pipelining = mode;
    return ensure_front_stream(c);
}

int swr_get_pipelining(swr_context* c, int* mode) { SWR_ENTER(c); if (!mode) return SWR_ERR_INVALID_ARG; *mode = c->pipelining; return SWR_OK; }

int swr_sync(swr_context* c) {
    SWR_ENTER(c);
    return flush_and_sync_locked(c);
}

int swr_readback(swr_context* c, float* color, float* depth) { SWR_ENTER(c); return planes_transfer(c, color, depth, true); }

int swr_readback_rgb(swr_context* c, float* rgb) { SWR_ENTER(c); return payload_readback(c, FLATTEN, rgb); }
int swr_readback_rgb_resolved(swr_context* c, int kx, int ky, float* rgb) { SWR_ENTER(c); return payload_readback(c, resolved(kx, ky), rgb); }
int swr_readback_rgb8(swr_context* c, int kx, int ky, int bpp, uint8_t* out) { SWR_ENTER(c); return payload_readback(c, quantised(kx, ky, bpp), out); }

int swr_resolved_size(swr_context* c, int kx, int ky, int* out_width, int* out_rows) {
    SWR_ENTER(c);
    if (!out_width || !out_rows) return fail(c, SWR_ERR_INVALID_ARG, "out_width or out_rows is null");
    const Payload p = resolved(kx, ky);
    int rc = payload_check(c, p); if (rc) return rc;
    *out_width = payload_width(c, p); *out_rows = payload_rows(c, p);
    return SWR_OK;
}

int swr_present8_size(swr_context* c, int kx, int ky, int bpp, int* out_width, int* out_rows, size_t* out_bytes) {
    SWR_ENTER(c);
    if (!out_width || !out_rows || !out_bytes) return fail(c, SWR_ERR_INVALID_ARG, "out_width, out_rows or out_bytes is null");
    const Payload p = quantised(kx, ky, bpp);
    int rc = payload_check(c, p); if (rc) return rc;
    *out_width = payload_width(c, p); *out_rows = payload_rows(c, p); *out_bytes = payload_bytes(c, p);
    return SWR_OK;
}

int swr_present_rgb_async(swr_context* c, float* rgb, uint64_t* ticket) { SWR_ENTER(c); return payload_present(c, FLATTEN, rgb, ticket); }
int swr_present_rgb_resolved_async(swr_context* c, int kx, int ky, float* rgb, uint64_t* ticket) {
    SWR_ENTER(c);
    return payload_present(c, resolved(kx, ky), rgb, ticket);
}
int swr_present_rgb8_async(swr_context* c, int kx, int ky, int bpp, uint8_t* out, uint64_t* ticket) {
    SWR_ENTER(c);
    return payload_present(c, quantised(kx, ky, bpp), out, ticket);
}

int swr_present_wait(swr_context* c, uint64_t ticket) {
    SWR_ENTER(c);
    int slot = -1;
    for (int i = 0; i < 2; ++i) if (c->present_ticket[i] == ticket && ticket) slot = i;
    if (slot < 0) {
        if (!ticket || ticket > c->next_ticket) return fail(c, SWR_ERR_INVALID_ARG, "unknown present ticket");
        for (int i = 0; i < 2; ++i)
            if (c->stale_dropped[i] == ticket) { c->stale_dropped[i] = 0; return SWR_STALE; }     // dropped by back-pressure, and it was stale
        return SWR_OK;                                                                             // already waited for
    }
    SWR_HIP(c, hipEventSynchronize(c->present_done[slot]));
    c->present_ticket[slot] = 0;
    bool stale = false;
    int rc = present_is_stale(c, slot, stale); if (rc) return rc;
    if (stale) {
        // a batch flushed at or before this present did not fit its pair buffers and poisoned itself (and everything after it): the
        // copied pixels predate it.  Drain, replay (validate_locked) and tell the caller to present again.
        rc = sync_locked(c);
        return rc ? rc : SWR_STALE;
    }
    // Every batch flushed before this present has completed (the flatten ran behind them): retire them without draining the stream,
    // and without freeing anything -- their transient meshes go to the pool (hipFree would wait for frame i + 1, which is rendering).
    // (A batch poisoned AFTER this present leaves this frame good: it is replayed at the next synchronisation point.)
    const uint32_t upto = c->present_seq[slot];
    size_t k = 0;
    while (k < c->inflight.size() && c->inflight[k].seq <= upto) { retire_batch(c, c->inflight[k], true); ++k; }
    c->inflight.erase(c->inflight.begin(), c->inflight.begin() + (std::ptrdiff_t)k);
    return SWR_OK;
}

int swr_host_register(swr_context* c, void* ptr, size_t bytes) {
    SWR_ENTER(c);
    if (!ptr || !bytes) return fail(c, SWR_ERR_INVALID_ARG, "null or empty host buffer");
    SWR_HIP(c, hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    return SWR_OK;
}

int swr_host_unregister(swr_context* c, void* ptr) {
    SWR_ENTER(c);
    if (!ptr) return fail(c, SWR_ERR_INVALID_ARG, "null host buffer");
    int rc = flush_and_sync_locked(c); if (rc) return rc;   // nothing in flight may still target the buffer
    SWR_HIP(c, hipHostUnregister(ptr));
    return SWR_OK;
}

int swr_flatten_rgb_device(swr_context* c, float* d_rgb) { SWR_ENTER(c); return payload_device(c, FLATTEN, d_rgb, true); }
int swr_flatten_rgb_device_async(swr_context* c, float* d_rgb) { SWR_ENTER(c); return payload_device(c, FLATTEN, d_rgb, false); }
int swr_resolve_rgb_device(swr_context* c, int kx, int ky, float* d_rgb) { SWR_ENTER(c); return payload_device(c, resolved(kx, ky), d_rgb, true); }
int swr_resolve_rgb_device_async(swr_context* c, int kx, int ky, float* d_rgb) { SWR_ENTER(c); return payload_device(c, resolved(kx, ky), d_rgb, false); }
int swr_resolve_rgb8_device(swr_context* c, int kx, int ky, int bpp, uint8_t* d_out) { SWR_ENTER(c); return payload_device(c, quantised(kx, ky, bpp), d_out, true); }
int swr_resolve_rgb8_device_async(swr_context* c, int kx, int ky, int bpp, uint8_t* d_out) {
    SWR_ENTER(c);
    return payload_device(c, quantised(kx, ky, bpp), d_out, false);
}

int swr_replay_count(swr_context* c, uint64_t* out) { SWR_ENTER(c); if (!out) return SWR_ERR_INVALID_ARG; *out = c->replays; return SWR_OK; }
int swr_sync_count(swr_context* c, uint64_t* out) { SWR_ENTER(c); if (!out) return SWR_ERR_INVALID_ARG; *out = c->host_syncs; return SWR_OK; }

int swr_upload(swr_context* c, const float* color, const float* depth) {
    SWR_ENTER(c);
    return planes_transfer(c, const_cast<float*>(color), const_cast<float*>(depth), false);
}

int swr_color_device_ptr(swr_context* c, void** out) { SWR_ENTER(c); if (!out) return SWR_ERR_INVALID_ARG; *out = c->color; return SWR_OK; }
int swr_depth_device_ptr(swr_context* c, void** out) { SWR_ENTER(c); if (!out) return SWR_ERR_INVALID_ARG; *out = c->depth; return SWR_OK; }

int swr_get_pixel(swr_context* c, int x, int y, float rgba[4]) {
    SWR_ENTER(c);
    if (!rgba) return SWR_ERR_INVALID_ARG;
    rgba[0] = rgba[1] = rgba[2] = rgba[3] = 0.0f;                 // Vector4.Zero out of bounds, MainWindow.cs:397
    return pixel_transfer(c, x, y, c->color, 16, rgba, true);
}
int swr_set_pixel(swr_context* c, int x, int y, const float rgba[4]) {
    SWR_ENTER(c);
    if (!rgba) return SWR_ERR_INVALID_ARG;
    return pixel_transfer(c, x, y, c->color, 16, const_cast<float*>(rgba), false);
}
int swr_get_depth(swr_context* c, int x, int y, float* d) {
    SWR_ENTER(c);
    if (!d) return SWR_ERR_INVALID_ARG;
    *d = SWR_FLOAT_MINVALUE;                                       // MainWindow.cs:425
    return pixel_transfer(c, x, y, c->depth, 4, d, true);
}
int swr_set_depth(swr_context* c, int x, int y, float d) {
    SWR_ENTER(c);
    return pixel_transfer(c, x, y, c->depth, 4, &d, false);
}

int swr_texture_create(swr_context* c, const uint8_t* rgba8, int w, int h, swr_texture** out) {
    SWR_ENTER(c);
    return rgba8 ? texture_create(c, rgba8, w, h, out, "texture upload failed: ") : fail(c, SWR_ERR_INVALID_ARG, "bad texture arguments");
}
int swr_texture_create_target(swr_context* c, int w, int h, swr_texture** out) { SWR_ENTER(c); return texture_create(c, nullptr, w, h, out, "texture allocation failed: "); }
int swr_texture_create_depth(swr_context* c, const float* depth, int w, int h, swr_texture** out) {
    SWR_ENTER(c);
    return texture_create(c, depth, w, h, out, depth ? "texture upload failed: " : "texture allocation failed: ", SWR_TEXTURE_FORMAT_DEPTH32F);
}

namespace {
// swr_texture_update_from_frame / _from_post / _from_depth under the mutexes of both contexts
int texture_update_locked(swr_context* c, swr_texture* t, swr_context* src, const TextureUpdate& u) {
    if (!c) return SWR_ERR_INVALID_ARG;
    if (!src || src == c) {
        std::lock_guard<std::mutex> lock_(c->mu);
        (void)hipSetDevice(c->device);
        return texture_update(c, t, c, u);
    }
    std::lock(c->mu, src->mu);                            // (both, in an order that cannot deadlock against the opposite call)
    std::lock_guard<std::mutex> lock_c(c->mu, std::adopt_lock), lock_s(src->mu, std::adopt_lock);
    (void)hipSetDevice(c->device);
    return texture_update(c, t, src, u);
}

// swr_texture_readback / _readback_depth: the row-major texels of a texture of `format`
int texture_readback(swr_context* c, const swr_texture* t, void* out, int format) {
    if (!t || !out) return fail(c, SWR_ERR_INVALID_ARG, "bad texture_readback arguments");
    if (int rc = texture_format_check(c, t, format)) return rc;
    SWR_HIP(c, hipMemcpyAsync(out, t->d_rgba, (size_t)t->w * t->h * 4, hipMemcpyDeviceToHost, c->stream));
    return sync_locked(c);
}
}  // namespace

int swr_texture_update_from_frame(swr_context* c, swr_texture* t, swr_context* src, int kx, int ky, int alpha_mode) {
    return texture_update_locked(c, t, src, TextureUpdate{ FROM_FRAME, kx, ky, alpha_mode, 0 });
}
int swr_texture_update_from_post(swr_context* c, swr_texture* t, swr_context* src, int post_id, int kx, int ky, int alpha_mode) {
    return texture_update_locked(c, t, src, TextureUpdate{ FROM_POST, kx, ky, alpha_mode, post_id });
}
int swr_texture_update_from_depth(swr_context* c, swr_texture* t, swr_context* src, int kx, int ky, int reduce) {
    return texture_update_locked(c, t, src, TextureUpdate{ FROM_DEPTH, kx, ky, reduce, 0 });
}

int swr_texture_readback(swr_context* c, const swr_texture* t, uint8_t* rgba8) { SWR_ENTER(c); return texture_readback(c, t, rgba8, SWR_TEXTURE_FORMAT_RGBA8); }
int swr_texture_readback_depth(swr_context* c, const swr_texture* t, float* out) { SWR_ENTER(c); return texture_readback(c, t, out, SWR_TEXTURE_FORMAT_DEPTH32F); }

int swr_texture_format(swr_context* c, const swr_texture* t, int* format) {
    SWR_ENTER(c);
    if (!t || !format) return fail(c, SWR_ERR_INVALID_ARG, "bad texture_format arguments");
    *format = t->format;
    return SWR_OK;
}

int swr_texture_set_filter(swr_context* c, swr_texture* t, int bilinear) {
    SWR_ENTER(c);
    if (!t) return fail(c, SWR_ERR_INVALID_ARG, "texture is null");
    t->bilinear = bilinear != 0;          // read when a draw is recorded
    if (t->bilinear && !t->d_blocked && (t->w & 3) == 0 && (t->h & 3) == 0) {
        // the four taps of a bilinear fetch: one 64-byte line 9 times out of 16 from a block-linear copy, two lines always from the
        // row-major original (same stream as the upload and as the raster kernels that will read it)
        SWR_HIP(c, texels_alloc(&t->d_blocked, (size_t)t->w * t->h * 4));
        SWR_HIP(c, texture_header_write(c, t, t->d_blocked));          // (a copy of d_rgba's: the same levels, the same tail)
        const int blocks = (int)std::min<size_t>(((size_t)t->w * t->h + 255) / 256, 2048 * 8);
        hipLaunchKernelGGL(k_block_texture, dim3(blocks), dim3(256), 0, c->stream, (const uint32_t*)t->d_rgba, (uint32_t*)t->d_blocked, t->w, t->h);
        SWR_HIP(c, hipGetLastError());
    }
    return SWR_OK;
}

int swr_texture_destroy(swr_context* c, swr_texture* t) {
    SWR_ENTER(c);
    if (!t) return SWR_OK;
    int rc = flush_and_sync_locked(c); if (rc) return rc;
    for (auto& p : c->posts)                              // a later present reads "no texture" there
        for (const swr_texture*& bound : p.second->tex) if (bound == t) bound = nullptr;
    for (auto& p : c->progs)                              // a later draw captures "no texture" there (recorded ones were flushed above)
        for (const swr_texture*& bound : p.second->tex) if (bound == t) bound = nullptr;
    texels_free(t->d_rgba);
    texels_free(t->d_blocked);
    if (t->d_tail) (void)hipFree(t->d_tail);
    delete t;
    return SWR_OK;
}

int swr_texture_sample(swr_context* c, const swr_texture* t, const float* uv, int n, float* out) {
    SWR_ENTER(c);
    if (!t || !uv || !out || n < 0) return fail(c, SWR_ERR_INVALID_ARG, "bad texture_sample arguments");
    if (int rc = texture_format_check(c, t, SWR_TEXTURE_FORMAT_RGBA8)) return rc;
    if (n == 0) return SWR_OK;
    const size_t off_out = ((size_t)n * 8 + 15) & ~(size_t)15;
    int rc = ensure(c, c->d_scratch, off_out + (size_t)n * 16);
    if (rc) return rc;
    float2* d_uv = c->d_scratch.as<float2>();
    float4* d_out = reinterpret_cast<float4*>(reinterpret_cast<char*>(c->d_scratch.p) + off_out);
    SWR_HIP(c, hipMemcpyAsync(d_uv, uv, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_texture_sample, dim3((n + 255) / 256), dim3(256), 0, c->stream, t->d_rgba, t->w, t->h, d_uv, n, d_out);
    SWR_HIP(c, hipGetLastError());
    SWR_HIP(c, hipMemcpyAsync(out, d_out, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
    return sync_locked(c);
}

int swr_texture_sample_depth(swr_context* c, const swr_texture* t, const float* uv_ref, int n, float* out) {
    SWR_ENTER(c);
    if (!t || !uv_ref || !out || n < 0) return fail(c, SWR_ERR_INVALID_ARG, "bad texture_sample_depth arguments");
    if (int rc = texture_format_check(c, t, SWR_TEXTURE_FORMAT_DEPTH32F)) return rc;
    if (n == 0) return SWR_OK;
    const size_t off_out = ((size_t)n * 12 + 15) & ~(size_t)15;
    int rc = ensure(c, c->d_scratch, off_out + (size_t)n * 8);
    if (rc) return rc;
    float* d_in = c->d_scratch.as<float>();
    float2* d_out = reinterpret_cast<float2*>(reinterpret_cast<char*>(c->d_scratch.p) + off_out);
    SWR_HIP(c, hipMemcpyAsync(d_in, uv_ref, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_texture_sample_depth, dim3((n + 255) / 256), dim3(256), 0, c->stream, texture_slot_of(t), (const float*)d_in, n, d_out);
    SWR_HIP(c, hipGetLastError());
    SWR_HIP(c, hipMemcpyAsync(out, d_out, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    return sync_locked(c);
}

// ---- mip chains
int swr_texture_generate_mipmaps(swr_context* c, swr_texture* t) {
    SWR_ENTER(c);
    if (!t) return fail(c, SWR_ERR_INVALID_ARG, "texture is null");
    if (int rc = texture_format_check(c, t, SWR_TEXTURE_FORMAT_RGBA8)) return rc;
    if (t->cube && (t->w & (t->w - 1)) != 0)
        return fail(c, SWR_ERR_UNSUPPORTED, "a cube map's chain needs a power-of-two side (per-face level sizes are out of scope, DESIGN.md section 27)");
    const int L = texture_full_levels(t);                    // (a cube's chain ends where a face is one texel)
    if (L == 1) return SWR_OK;                               // 1 x 1: a chain of one level, which it has
    // immediate-mode semantics without a host wait (swr_texture_update_from_frame's): the recorded draws go first and read the old
    // record -- the device reads it when a kernel runs, so the order on the stream is what "earlier" and "later" mean
    int rc = flush_locked(c); if (rc) return rc;
    if (!t->d_tail) {
        uint32_t off[SWR_TEXTURE_MAX_LEVELS];
        mip_offsets(t, L, off);
        const size_t texels = (size_t)off[L - 1] + (size_t)mip_level_side(t->w, L - 1) * (size_t)mip_level_side(t->h, L - 1);
        SWR_HIP(c, hipMalloc((void**)&t->d_tail, texels * 4));
    }
    if (t->levels != L) {
        t->levels = L;
        SWR_HIP(c, texture_header_write(c, t, t->d_rgba));
        if (t->d_blocked) SWR_HIP(c, texture_header_write(c, t, t->d_blocked));
    }
    return mip_generate(c, t);
}

int swr_texture_levels(swr_context* c, const swr_texture* t, int* levels) {
    SWR_ENTER(c);
    if (!t || !levels) return fail(c, SWR_ERR_INVALID_ARG, "bad texture_levels arguments");
    *levels = t->levels;
    return SWR_OK;
}

int swr_texture_level_size(swr_context* c, const swr_texture* t, int level, int* w, int* h) {
    SWR_ENTER(c);
    if (!t || !w || !h) return fail(c, SWR_ERR_INVALID_ARG, "bad texture_level_size arguments");
    if (level < 0 || level >= texture_full_levels(t)) return fail(c, SWR_ERR_INVALID_ARG, "the level is outside the texture's full chain (0 .. floor(log2(max(w, h))))");
    *w = mip_level_side(t->w, level); *h = mip_level_side(t->h, level);
    return SWR_OK;
}

int swr_texture_readback_level(swr_context* c, const swr_texture* t, int level, uint8_t* rgba8) {
    SWR_ENTER(c);
    if (!t || !rgba8) return fail(c, SWR_ERR_INVALID_ARG, "bad texture_readback_level arguments");
    if (int rc = texture_format_check(c, t, SWR_TEXTURE_FORMAT_RGBA8)) return rc;
    if (level < 0 || level >= t->levels) return fail(c, SWR_ERR_INVALID_ARG, "the level is outside the levels the texture has (swr_texture_levels)");
    if (level == 0) return texture_readback(c, t, rgba8, SWR_TEXTURE_FORMAT_RGBA8);
    uint32_t off[SWR_TEXTURE_MAX_LEVELS];
    mip_offsets(t, t->levels, off);
    const size_t bytes = (size_t)mip_level_side(t->w, level) * (size_t)mip_level_side(t->h, level) * 4;
    SWR_HIP(c, hipMemcpyAsync(rgba8, t->d_tail + (size_t)off[level] * 4, bytes, hipMemcpyDeviceToHost, c->stream));
    return sync_locked(c);
}

int swr_texture_sample_lod(swr_context* c, const swr_texture* t, const float* uv_lod, int n, float* out_rgba) {
    SWR_ENTER(c);
    if (!t || !uv_lod || !out_rgba || n < 0) return fail(c, SWR_ERR_INVALID_ARG, "bad texture_sample_lod arguments");
    if (int rc = texture_format_check(c, t, SWR_TEXTURE_FORMAT_RGBA8)) return rc;
    if (n == 0) return SWR_OK;
    const size_t off_out = ((size_t)n * 12 + 15) & ~(size_t)15;
    int rc = ensure(c, c->d_scratch, off_out + (size_t)n * 16);
    if (rc) return rc;
    float* d_in = c->d_scratch.as<float>();
    float4* d_out = reinterpret_cast<float4*>(reinterpret_cast<char*>(c->d_scratch.p) + off_out);
    SWR_HIP(c, hipMemcpyAsync(d_in, uv_lod, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_texture_sample_lod, dim3((n + 255) / 256), dim3(256), 0, c->stream, texture_slot_of(t), (const float*)d_in, n, d_out);
    SWR_HIP(c, hipGetLastError());
    SWR_HIP(c, hipMemcpyAsync(out_rgba, d_out, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
    return sync_locked(c);
}

int swr_texture_lod(swr_context* c, const swr_texture* t, const float* grads, int n, float* out_lod) {
    SWR_ENTER(c);
    if (!t || !grads || !out_lod || n < 0) return fail(c, SWR_ERR_INVALID_ARG, "bad texture_lod arguments");
    if (int rc = texture_format_check(c, t, SWR_TEXTURE_FORMAT_RGBA8)) return rc;
    if (n == 0) return SWR_OK;
    const size_t off_out = (size_t)n * 16;
    int rc = ensure(c, c->d_scratch, off_out + (size_t)n * 4);
    if (rc) return rc;
    float4* d_in = c->d_scratch.as<float4>();
    float* d_out = reinterpret_cast<float*>(reinterpret_cast<char*>(c->d_scratch.p) + off_out);
    SWR_HIP(c, hipMemcpyAsync(d_in, grads, (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_texture_lod, dim3((n + 255) / 256), dim3(256), 0, c->stream, texture_slot_of(t), (const float4*)d_in, n, d_out);
    SWR_HIP(c, hipGetLastError());
    SWR_HIP(c, hipMemcpyAsync(out_lod, d_out, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    return sync_locked(c);
}

// ---- cube maps: an n x 6 n texture, face f in rows [f n, (f + 1) n)
namespace {
int cube_create(swr_context* c, const void* texels, int n, swr_texture** out, int format) {
    if (n < 1 || !out) return fail(c, SWR_ERR_INVALID_ARG, "bad cube map arguments");
    if (6ull * (uint64_t)n * (uint64_t)n >= (1ull << 30)) return fail(c, SWR_ERR_INVALID_ARG, "cube maps of 2^30 texels or more are not supported (32-bit texel index)");
    const int rc = texture_create(c, texels, n, 6 * n, out, texels ? "texture upload failed: " : "texture allocation failed: ", format);
    if (rc == SWR_OK) (*out)->cube = true;
    return rc;
}
}  // namespace

int swr_texture_create_cube(swr_context* c, const uint8_t* rgba8, int n, swr_texture** out) { SWR_ENTER(c); return cube_create(c, rgba8, n, out, SWR_TEXTURE_FORMAT_RGBA8); }
int swr_texture_create_cube_depth(swr_context* c, const float* depth, int n, swr_texture** out) { SWR_ENTER(c); return cube_create(c, depth, n, out, SWR_TEXTURE_FORMAT_DEPTH32F); }

int swr_texture_is_cube(swr_context* c, const swr_texture* t, int* n) {
    SWR_ENTER(c);
    if (!t || !n) return fail(c, SWR_ERR_INVALID_ARG, "bad texture_is_cube arguments");
    *n = t->cube ? t->w : 0;
    return SWR_OK;
}

int swr_texture_update_face_from_frame(swr_context* c, swr_texture* t, int face, swr_context* src, int kx, int ky, int alpha_mode) {
    return texture_update_locked(c, t, src, TextureUpdate{ FROM_FRAME, kx, ky, alpha_mode, 0, face, true });
}
int swr_texture_update_face_from_depth(swr_context* c, swr_texture* t, int face, swr_context* src, int kx, int ky, int reduce) {
    return texture_update_locked(c, t, src, TextureUpdate{ FROM_DEPTH, kx, ky, reduce, 0, face, true });
}
int swr_texture_update_face_from_post(swr_context* c, swr_texture* t, int face, swr_context* src, int post_id, int kx, int ky, int alpha_mode) {
    return texture_update_locked(c, t, src, TextureUpdate{ FROM_POST, kx, ky, alpha_mode, post_id, face, true });
}

int swr_texture_readback_face(swr_context* c, const swr_texture* t, int face, int level, void* out) {
    SWR_ENTER(c);
    if (!t || !out) return fail(c, SWR_ERR_INVALID_ARG, "bad texture_readback_face arguments");
    if (!t->cube) return fail(c, SWR_ERR_INVALID_ARG, "the texture is not a cube map (swr_texture_create_cube, swr_texture_create_cube_depth)");
    if (face < 0 || face > 5) return fail(c, SWR_ERR_INVALID_ARG, "face must be 0 .. 5 (+X, -X, +Y, -Y, +Z, -Z)");
    if (level < 0 || level >= t->levels) return fail(c, SWR_ERR_INVALID_ARG, "the level is outside the levels the texture has (swr_texture_levels)");
    const size_t n = (size_t)(t->w >> level);
    const uint8_t* from = t->d_rgba;
    if (level > 0) {
        uint32_t off[SWR_TEXTURE_MAX_LEVELS];
        mip_offsets(t, t->levels, off);
        from = t->d_tail + (size_t)off[level] * 4;
    }
    SWR_HIP(c, hipMemcpyAsync(out, from + (size_t)face * n * n * 4, n * n * 4, hipMemcpyDeviceToHost, c->stream));
    return sync_locked(c);
}

int swr_cube_face_view(int face, const float* eye, float* view) {
    if (face < 0 || face > 5 || !eye || !view) return SWR_ERR_INVALID_ARG;
    // Matrix4x4.CreateLookAt(eye, eye + axis, up) with up = +Y (+Y: +Z, -Y: -Z): the camera's x, y and z axes in the world
    static const float X[6][3] = { { 0, 0, 1 }, { 0, 0, -1 }, { 1, 0, 0 }, { 1, 0, 0 }, { -1, 0, 0 }, { 1, 0, 0 } };
    static const float Y[6][3] = { { 0, 1, 0 }, { 0, 1, 0 }, { 0, 0, 1 }, { 0, 0, -1 }, { 0, 1, 0 }, { 0, 1, 0 } };
    static const float Z[6][3] = { { -1, 0, 0 }, { 1, 0, 0 }, { 0, -1, 0 }, { 0, 1, 0 }, { 0, 0, -1 }, { 0, 0, 1 } };
    const float (*axes[3])[3] = { X, Y, Z };
    for (int k = 0; k < 3; ++k) {
        const float* a = axes[k][face];
        for (int r = 0; r < 3; ++r) view[4 * r + k] = a[r];
        // (Vector3.Dot(axis, eye) in float32: two of the products are zeros, so the sum is +-eye's component whatever fuses)
        view[12 + k] = -((a[0] * eye[0] + a[1] * eye[1]) + a[2] * eye[2]);
    }
    view[3] = view[7] = view[11] = 0.0f; view[15] = 1.0f;
    return SWR_OK;
}

int swr_texture_cube_face(swr_context* c, const float* dirs, int n, int* out_face, float* out_st) {
    SWR_ENTER(c);
    if (!dirs || !out_face || !out_st || n < 0) return fail(c, SWR_ERR_INVALID_ARG, "bad texture_cube_face arguments");
    if (n == 0) return SWR_OK;
    // faces and (s, t) come back in one block: n x (face, s, t) would interleave types, so two blocks, the second 16-byte aligned
    const size_t off_face = ((size_t)n * 12 + 15) & ~(size_t)15, off_st = off_face + (((size_t)n * 4 + 15) & ~(size_t)15);
    int rc = ensure(c, c->d_scratch, off_st + (size_t)n * 8);
    if (rc) return rc;
    char* base = reinterpret_cast<char*>(c->d_scratch.p);
    SWR_HIP(c, hipMemcpyAsync(base, dirs, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_texture_cube_face, dim3((n + 255) / 256), dim3(256), 0, c->stream, (const float*)base, n, (int*)(base + off_face), (float2*)(base + off_st));
    SWR_HIP(c, hipGetLastError());
    SWR_HIP(c, hipMemcpyAsync(out_face, base + off_face, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    SWR_HIP(c, hipMemcpyAsync(out_st, base + off_st, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    return sync_locked(c);
}

int swr_texture_sample_cube(swr_context* c, const swr_texture* t, const float* dir_lod, int n, float* out_rgba) {
    SWR_ENTER(c);
    if (!t || !dir_lod || !out_rgba || n < 0) return fail(c, SWR_ERR_INVALID_ARG, "bad texture_sample_cube arguments");
    if (!t->cube) return fail(c, SWR_ERR_INVALID_ARG, "the texture is not a cube map (swr_texture_create_cube)");
    if (int rc = texture_format_check(c, t, SWR_TEXTURE_FORMAT_RGBA8)) return rc;
    if (n == 0) return SWR_OK;
    const size_t off_out = (size_t)n * 16;
    int rc = ensure(c, c->d_scratch, off_out + (size_t)n * 16);
    if (rc) return rc;
    float4* d_in = c->d_scratch.as<float4>();
    float4* d_out = d_in + n;
    SWR_HIP(c, hipMemcpyAsync(d_in, dir_lod, (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_texture_sample_cube, dim3((n + 255) / 256), dim3(256), 0, c->stream, texture_slot_of(t), (const float4*)d_in, n, d_out);
    SWR_HIP(c, hipGetLastError());
    SWR_HIP(c, hipMemcpyAsync(out_rgba, d_out, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
    return sync_locked(c);
}

int swr_texture_sample_cube_depth(swr_context* c, const swr_texture* t, const float* dir_ref, int n, float* out) {
    SWR_ENTER(c);
    if (!t || !dir_ref || !out || n < 0) return fail(c, SWR_ERR_INVALID_ARG, "bad texture_sample_cube_depth arguments");
    if (!t->cube) return fail(c, SWR_ERR_INVALID_ARG, "the texture is not a cube map (swr_texture_create_cube_depth)");
    if (int rc = texture_format_check(c, t, SWR_TEXTURE_FORMAT_DEPTH32F)) return rc;
    if (n == 0) return SWR_OK;
    const size_t off_out = (size_t)n * 16;
    int rc = ensure(c, c->d_scratch, off_out + (size_t)n * 8);
    if (rc) return rc;
    float4* d_in = c->d_scratch.as<float4>();
    float2* d_out = reinterpret_cast<float2*>(d_in + n);
    SWR_HIP(c, hipMemcpyAsync(d_in, dir_ref, (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_texture_sample_cube_depth, dim3((n + 255) / 256), dim3(256), 0, c->stream, texture_slot_of(t), (const float4*)d_in, n, d_out);
    SWR_HIP(c, hipGetLastError());
    SWR_HIP(c, hipMemcpyAsync(out, d_out, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    return sync_locked(c);
}

int swr_mesh_create(swr_context* c, const swr_vertex* v, int nv, const uint16_t* idx, int ni, swr_mesh** out) { SWR_ENTER(c); return make_mesh(c, v, nv, idx, ni, false, out); }

int swr_mesh_destroy(swr_context* c, swr_mesh* m) {
    SWR_ENTER(c);
    if (!m) return SWR_OK;
    int rc = flush_and_sync_locked(c); if (rc) return rc;
    destroy_mesh(m);
    return SWR_OK;
}

// ---- deforming meshes: key-frame blend and matrix-palette skinning into a retained mesh
namespace {
// a retained mesh of this context, or the message why not
int deform_mesh_check(swr_context* c, const swr_mesh* m, const char* null_msg) {
    if (!m) return fail(c, SWR_ERR_INVALID_ARG, null_msg);
    if (m->transient) return fail(c, SWR_ERR_INVALID_ARG, "a transient mesh (swr_render_mesh_arrays) cannot be deformed, copied or read back");
    if (m->owner != c) return fail(c, SWR_ERR_INVALID_ARG, "the mesh belongs to another context");
    return SWR_OK;
}

bool batch_reads(const std::vector<DrawCmd>& draws, const swr_mesh* m) {
    for (const DrawCmd& d : draws) if (d.mesh == m) return true;
    return false;
}

// Everything that must happen before a kernel may WRITE dst's vertices; returns the stream it runs on.
//   A. immediate-mode semantics: draws recorded so far that reference dst are launched first (they see the old vertices) -- and only
//      then: a loop that deforms sixteen players and draws them stays one batch;
//   B. an optimistic batch in flight that references dst may be replayed later (validate_locked), and a replay runs the front end
//      again: it must read the vertices the batch saw, so the streams are drained and the batches validated before the first write
//      (transient meshes solve the same problem through c->garbage: their buffers are not reused before the streams were idle).
//      A loop that presents every frame has retired those batches in swr_present_wait: nothing to wait for there.
// The deform runs where make_mesh uploads (use_front_stream): only front-end kernels read a mesh, and every front end issued later
// is behind it -- on the front stream by stream order, on the context's stream through f_tail_pending (execute_batch).
int deform_begin(swr_context* c, const swr_mesh* dst, hipStream_t* stream) {
    int rc;
    if (batch_reads(c->draws, dst) && (rc = flush_locked(c))) return rc;
    bool in_flight = false;
    for (const Batch& b : c->inflight) in_flight = in_flight || batch_reads(b.draws, dst);
    if (in_flight && (rc = sync_locked(c))) return rc;
    if ((rc = ensure_front_stream(c))) return rc;
    *stream = use_front_stream(c);
    return SWR_OK;
}

// ... and after it: what the host knows about dst's old vertices is void.
//   C. readers on the ray stream (swr_raycast, swr_character_update, swr_mesh_readback) are ordered behind swr_mesh::uploaded: it is
//      recorded again behind the deform.  The query entry points return only after their kernels finished (they wait for their own
//      result under the context mutex), so no ray-stream reader of dst is in flight when a deform is issued;
//   D. the bounding sphere is computed again on first use (swr_mesh_bounds, swr_render_mesh_culled follow the pose);
//   E. the host-side box is gone: band_rejects keeps the draw on every rank (conservative and correct).
int deform_end(swr_context* c, swr_mesh* dst, hipStream_t stream) {
    SWR_HIP(c, hipEventRecord(dst->uploaded, stream));
    dst->posed.reset();
    dst->upload_seen = false;
    dst->bounds_ready = false;
    dst->has_box = false;
    return SWR_OK;
}

// A palette's way to the device without a wait (F): the first slot whose last kernel is over, else a new one.
int palette_slot(swr_context* c, size_t bytes, PaletteSlot** out, bool device_copy = true) {
    PaletteSlot* s = nullptr;
    const size_t n = c->palettes.size();
    for (size_t k = 0; k < n && !s; ++k) {
        PaletteSlot& q = c->palettes[(c->palette_next + k) % n];
        if (q.busy && hipEventQuery(q.done) == hipSuccess) q.busy = false;
        if (!q.busy) { s = &q; c->palette_next = (c->palette_next + k + 1) % n; }
    }
    if (!s && n < SWR_PALETTE_SLOTS_MAX) {
        c->palettes.emplace_back();
        s = &c->palettes.back();
        SWR_HIP(c, hipEventCreateWithFlags(&s->done, hipEventDisableTiming));
    }
    if (!s) {       // back-pressure: SWR_PALETTE_SLOTS_MAX palettes queued and none read yet
        s = &c->palettes[c->palette_next % n];
        c->palette_next = (c->palette_next + 1) % n;
        SWR_HIP(c, hipEventSynchronize(s->done));
        s->busy = false;
    }
    // (a free slot's buffers are idle: growing them frees nothing a kernel reads)
    if (s->host.cap < bytes) SWR_HIP(c, ensure_pinned(s->host, std::max<size_t>(bytes, 4096)));
    // (device_copy = false: staging for a copy that goes elsewhere, swr_pose_set_upload)
    if (device_copy) { int rc = ensure(c, s->dev, std::max<size_t>(bytes, 4096)); if (rc) return rc; }
    *out = s;
    return SWR_OK;
}
}  // namespace

int swr_mesh_create_like(swr_context* c, const swr_mesh* src, swr_mesh** out) {
    SWR_ENTER(c);
    if (!out) return fail(c, SWR_ERR_INVALID_ARG, "out is null");
    int rc = deform_mesh_check(c, src, "the source mesh is null"); if (rc) return rc;
    if ((rc = ensure_front_stream(c))) return rc;
    swr_mesh* m = new swr_mesh();
    m->n_verts = src->n_verts; m->n_idx = src->n_idx; m->owner = c;
    memcpy(m->box_lo, src->box_lo, sizeof m->box_lo); memcpy(m->box_hi, src->box_hi, sizeof m->box_hi);
    m->has_box = src->has_box;
    const size_t vbytes = (size_t)src->n_verts * sizeof(swr_vertex), ibytes = (size_t)src->n_idx * 2;
    // behind src's upload or its last deform, on their stream: the arrays do not cross PCIe again
    const hipStream_t s = use_front_stream(c);
    hipError_t e = hipSuccess;
    if (vbytes) { e = hipMalloc((void**)&m->d_verts, vbytes); if (e == hipSuccess) m->cap_verts = vbytes; }
    if (e == hipSuccess && ibytes) { e = hipMalloc((void**)&m->d_idx, ibytes + 8); if (e == hipSuccess) m->cap_idx = ibytes + 8; }
    if (e == hipSuccess && vbytes) e = hipMemcpyAsync(m->d_verts, src->d_verts, vbytes, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && ibytes) e = hipMemcpyAsync(m->d_idx, src->d_idx, ibytes, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&m->uploaded, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(m->uploaded, s);
    if (e != hipSuccess) {
        destroy_mesh(m);
        c->err = std::string("mesh copy failed: ") + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? SWR_ERR_OOM : SWR_ERR_HIP;
    }
    *out = m;
    return SWR_OK;
}

int swr_mesh_readback(swr_context* c, const swr_mesh* mesh, swr_vertex* out) {
    SWR_ENTER(c);
    int rc = deform_mesh_check(c, mesh, "the mesh is null"); if (rc) return rc;
    if (!out) return fail(c, SWR_ERR_INVALID_ARG, "the destination is null");
    if (mesh->n_verts == 0) return SWR_OK;
    // a reader on the ray stream: behind the upload or the last deform (swr_mesh::uploaded) and behind nothing else -- recorded draws
    // are not flushed, a frame in flight is not waited for
    if ((rc = ensure_ray_stream(c))) return rc;
    swr_mesh* m = const_cast<swr_mesh*>(mesh);
    if (!m->upload_seen) { SWR_HIP(c, hipStreamWaitEvent(c->ray_stream, m->posed ? m->posed->ev : m->uploaded, 0)); m->upload_seen = true; }
    SWR_HIP(c, hipMemcpyAsync(out, m->d_verts, (size_t)m->n_verts * sizeof(swr_vertex), hipMemcpyDeviceToHost, c->ray_stream));
    SWR_HIP(c, hipStreamSynchronize(c->ray_stream));
    return SWR_OK;
}

int swr_mesh_blend(swr_context* c, swr_mesh* dst, const swr_mesh* a, const swr_mesh* b, float t) {
    SWR_ENTER(c);
    int rc;
    if ((rc = deform_mesh_check(c, dst, "the destination mesh is null"))) return rc;
    if ((rc = deform_mesh_check(c, a, "key frame a is null"))) return rc;
    if ((rc = deform_mesh_check(c, b, "key frame b is null"))) return rc;
    if (dst == a || dst == b) return fail(c, SWR_ERR_INVALID_ARG, "the destination mesh is one of the key frames (make a target with swr_mesh_create_like)");
    if (a->n_verts != dst->n_verts || b->n_verts != dst->n_verts) return fail(c, SWR_ERR_INVALID_ARG, "the key frames and the destination must have equal vertex counts");
    if (dst->n_verts == 0) return SWR_OK;
    hipStream_t s = nullptr;
    if ((rc = deform_begin(c, dst, &s))) return rc;
    const uint32_t n_words = 3u * (uint32_t)dst->n_verts;
    hipLaunchKernelGGL(k_mesh_blend, dim3((n_words + SWR_DEFORM_BLOCK - 1u) / SWR_DEFORM_BLOCK), dim3(SWR_DEFORM_BLOCK), 0, s,
                       reinterpret_cast<const float4*>(a->d_verts), reinterpret_cast<const float4*>(b->d_verts),
                       reinterpret_cast<float4*>(dst->d_verts), n_words, t);
    SWR_HIP(c, hipGetLastError());
    return deform_end(c, dst, s);
}

int swr_mesh_set_skin(swr_context* c, swr_mesh* m, const uint16_t* joints4, const float* weights4) {
    SWR_ENTER(c);
    int rc = deform_mesh_check(c, m, "the mesh is null"); if (rc) return rc;
    if ((joints4 == nullptr) != (weights4 == nullptr)) return fail(c, SWR_ERR_INVALID_ARG, "pass both joints4 and weights4, or NULL for both (which removes the attributes)");
    if (!joints4) {
        // (hipFree waits for the device: a queued k_mesh_skin has read them by then)
        if (m->d_joints) SWR_HIP(c, hipFree(m->d_joints));
        m->d_joints = nullptr;
        if (m->d_weights) SWR_HIP(c, hipFree(m->d_weights));
        m->d_weights = nullptr;
        m->max_joint = -1; m->has_skin = false;
        return SWR_OK;
    }
    const size_t nv = (size_t)m->n_verts;
    int max_joint = -1;
    for (size_t i = 0; i < 4 * nv; ++i) max_joint = std::max(max_joint, (int)joints4[i]);
    if ((rc = ensure_front_stream(c))) return rc;
    if (nv) {
        // a second call replaces the attributes in place, on the stream the skinning kernels run on (behind those queued so far)
        if (!m->d_joints) SWR_HIP(c, hipMalloc((void**)&m->d_joints, nv * sizeof(ushort4)));
        if (!m->d_weights) SWR_HIP(c, hipMalloc((void**)&m->d_weights, nv * sizeof(float4)));
        const hipStream_t s = use_front_stream(c);
        SWR_HIP(c, hipMemcpyAsync(m->d_joints, joints4, nv * sizeof(ushort4), hipMemcpyHostToDevice, s));
        SWR_HIP(c, hipMemcpyAsync(m->d_weights, weights4, nv * sizeof(float4), hipMemcpyHostToDevice, s));
    }
    m->max_joint = max_joint; m->has_skin = true;
    return SWR_OK;
}

int swr_mesh_skin(swr_context* c, swr_mesh* dst, const swr_mesh* src, const float* palette, int n_joints) {
    SWR_ENTER(c);
    int rc;
    if ((rc = deform_mesh_check(c, dst, "the destination mesh is null"))) return rc;
    if ((rc = deform_mesh_check(c, src, "the source mesh is null"))) return rc;
    if (!palette) return fail(c, SWR_ERR_INVALID_ARG, "the palette is null");
    if (dst == src) return fail(c, SWR_ERR_INVALID_ARG, "the destination mesh is the source (make a target with swr_mesh_create_like)");
    if (src->n_verts != dst->n_verts) return fail(c, SWR_ERR_INVALID_ARG, "the source and the destination must have equal vertex counts");
    if (!src->has_skin) return fail(c, SWR_ERR_INVALID_ARG, "the source mesh has no skin attributes (swr_mesh_set_skin)");
    if (n_joints > 65535) return fail(c, SWR_ERR_UNSUPPORTED, "a palette holds at most 65535 joints (16-bit joint indices)");
    if (n_joints <= src->max_joint) return fail(c, SWR_ERR_INVALID_ARG, "n_joints must exceed the largest joint index the source's skin attributes use");
    if (dst->n_verts == 0) return SWR_OK;
    hipStream_t s = nullptr;
    if ((rc = deform_begin(c, dst, &s))) return rc;
    const size_t bytes = (size_t)n_joints * 64;
    PaletteSlot* slot = nullptr;
    if ((rc = palette_slot(c, bytes, &slot))) return rc;
    memcpy(slot->host.p, palette, bytes);
    SWR_HIP(c, hipMemcpyAsync(slot->dev.p, slot->host.p, bytes, hipMemcpyHostToDevice, s));
    const dim3 grid(((uint32_t)dst->n_verts + SWR_DEFORM_BLOCK - 1u) / SWR_DEFORM_BLOCK), block(SWR_DEFORM_BLOCK);
    hipLaunchKernelGGL(k_mesh_skin, grid, block, 0, s, (const swr_vertex*)src->d_verts, (const ushort4*)src->d_joints,
                       (const float4*)src->d_weights, (const float*)slot->dev.p, dst->d_verts, (uint32_t)dst->n_verts, c->nm_flags);
    SWR_HIP(c, hipGetLastError());
    SWR_HIP(c, hipEventRecord(slot->done, s));
    slot->busy = true;
    return deform_end(c, dst, s);
}

// ---- skeletal animation: clips to palettes on the GPU, one skin launch for a crowd
namespace {
int skeleton_check(swr_context* c, const swr_skeleton* k) {
    if (!k) return fail(c, SWR_ERR_INVALID_ARG, "the skeleton is null");
    if (k->owner != c) return fail(c, SWR_ERR_INVALID_ARG, "the skeleton belongs to another context");
    return SWR_OK;
}
int pose_set_check(swr_context* c, const swr_pose_set* p) {
    if (!p) return fail(c, SWR_ERR_INVALID_ARG, "the pose set is null");
    if (p->owner != c) return fail(c, SWR_ERR_INVALID_ARG, "the pose set belongs to another context");
    return SWR_OK;
}
// behind a write of the set on stream s: what swr_pose_set_readback orders itself by
int pose_set_written(swr_context* c, swr_pose_set* p, hipStream_t s) {
    SWR_HIP(c, hipEventRecord(p->written, s));
    p->written_seen = false;
    return SWR_OK;
}
void destroy_skeleton(swr_skeleton* k) {
    if (k->d_static) (void)hipFree(k->d_static);
    if (k->d_clips) (void)hipFree(k->d_clips);
    delete k;
}
void destroy_pose_set(swr_pose_set* p) {
    if (p->d_palettes) (void)hipFree(p->d_palettes);
    if (p->d_worlds) (void)hipFree(p->d_worlds);
    if (p->written) (void)hipEventDestroy(p->written);
    delete p;
}
}  // namespace

int swr_skeleton_create(swr_context* c, int n_nodes, const int32_t* parent, const float* rest_local, const float* rest_t,
                        const float* rest_r, const float* rest_s, int n_joints, const int32_t* joint_node, const float* inverse_bind,
                        swr_skeleton** out) {
    SWR_ENTER(c);
    if (!out || !parent || !rest_local || !rest_t || !rest_r || !rest_s) return fail(c, SWR_ERR_INVALID_ARG, "a skeleton array is null");
    if (n_nodes < 1 || n_joints < 0) return fail(c, SWR_ERR_INVALID_ARG, "a skeleton has at least one node and no negative joint count");
    if (n_joints > 0 && (!joint_node || !inverse_bind)) return fail(c, SWR_ERR_INVALID_ARG, "joint_node or inverse_bind is null");
    if (n_nodes > SWR_SKELETON_MAX_NODES || n_joints > 65535) return fail(c, SWR_ERR_UNSUPPORTED, "a skeleton holds at most 65535 nodes and 65535 joints");
    const size_t nn = (size_t)n_nodes, nj = (size_t)n_joints;
    std::vector<int32_t> depth(nn), order(nn);
    int n_levels = 0;
    for (size_t i = 0; i < nn; ++i) {
        if (parent[i] < -1 || parent[i] >= (int32_t)i) return fail(c, SWR_ERR_INVALID_ARG, "nodes must be in topological order: parent[i] < i, or -1 for a root");
        depth[i] = parent[i] < 0 ? 0 : depth[(size_t)parent[i]] + 1;
        n_levels = std::max(n_levels, depth[i] + 1);
    }
    for (size_t j = 0; j < nj; ++j)
        if (joint_node[j] < 0 || joint_node[j] >= n_nodes) return fail(c, SWR_ERR_INVALID_ARG, "a joint's node index is out of range");
    // the level table: nodes by depth, in index order within a level (a counting sort)
    std::vector<int32_t> level_start((size_t)n_levels + 1, 0);
    for (size_t i = 0; i < nn; ++i) ++level_start[(size_t)depth[i] + 1];
    for (int l = 0; l < n_levels; ++l) level_start[(size_t)l + 1] += level_start[(size_t)l];
    { std::vector<int32_t> at(level_start.begin(), level_start.end() - 1); for (size_t i = 0; i < nn; ++i) order[(size_t)at[(size_t)depth[i]]++] = (int32_t)i; }
    // one blob of 32-bit words, the matrices first (16-byte loads)
    const size_t o_local = 0, o_ib = o_local + 16 * nn, o_t = o_ib + 16 * nj, o_r = o_t + 3 * nn, o_s = o_r + 4 * nn, o_parent = o_s + 3 * nn,
                 o_order = o_parent + nn, o_level = o_order + nn, o_joint = o_level + (size_t)n_levels + 1, words = o_joint + nj;
    std::vector<uint32_t> blob(words);
    memcpy(&blob[o_local], rest_local, 64 * nn); memcpy(&blob[o_t], rest_t, 12 * nn); memcpy(&blob[o_r], rest_r, 16 * nn);
    memcpy(&blob[o_s], rest_s, 12 * nn); memcpy(&blob[o_parent], parent, 4 * nn); memcpy(&blob[o_order], order.data(), 4 * nn);
    memcpy(&blob[o_level], level_start.data(), 4 * ((size_t)n_levels + 1));
    if (nj) { memcpy(&blob[o_ib], inverse_bind, 64 * nj); memcpy(&blob[o_joint], joint_node, 4 * nj); }
    swr_skeleton* k = new swr_skeleton();
    k->owner = c; k->n_nodes = n_nodes; k->n_joints = n_joints; k->n_levels = n_levels;
    k->clips.assign(1, 0u);
    hipError_t e = hipMalloc(&k->d_static, words * 4);
    if (e == hipSuccess) e = hipMemcpy(k->d_static, blob.data(), words * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        destroy_skeleton(k);
        c->err = std::string("skeleton upload failed: ") + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? SWR_ERR_OOM : SWR_ERR_HIP;
    }
    *out = k;
    return SWR_OK;
}

int swr_skeleton_destroy(swr_context* c, swr_skeleton* k) {
    SWR_ENTER(c);
    if (!k) return SWR_OK;
    int rc = skeleton_check(c, k); if (rc) return rc;
    destroy_skeleton(k);                       // (hipFree waits for the device: a queued k_pose_sample has read it by then)
    return SWR_OK;
}

int swr_skeleton_add_clip(swr_context* c, swr_skeleton* k, const swr_anim_channel* channels, int n_channels, int* clip_index) {
    SWR_ENTER(c);
    int rc = skeleton_check(c, k); if (rc) return rc;
    if (!clip_index || n_channels < 0 || (n_channels > 0 && !channels)) return fail(c, SWR_ERR_INVALID_ARG, "channels or clip_index is null, or n_channels is negative");
    const size_t nn = (size_t)k->n_nodes;
    size_t words = k->clips.size() + 3 * nn;
    std::vector<uint8_t> taken(3 * nn, 0);
    for (int i = 0; i < n_channels; ++i) {
        const swr_anim_channel& ch = channels[i];
        if (ch.interpolation == SWR_ANIM_CUBICSPLINE) return fail(c, SWR_ERR_UNSUPPORTED, "CUBICSPLINE interpolation is not supported (STEP and LINEAR are)");
        if (ch.interpolation != SWR_ANIM_STEP && ch.interpolation != SWR_ANIM_LINEAR) return fail(c, SWR_ERR_INVALID_ARG, "unknown interpolation");
        if (ch.node < 0 || ch.node >= k->n_nodes) return fail(c, SWR_ERR_INVALID_ARG, "a channel's node index is out of range");
        if (ch.path < SWR_ANIM_PATH_TRANSLATION || ch.path > SWR_ANIM_PATH_SCALE) return fail(c, SWR_ERR_INVALID_ARG, "a channel's path is none of translation, rotation, scale");
        if (ch.n_keys < 1) return fail(c, SWR_ERR_INVALID_ARG, "a channel needs at least one key");
        if (!ch.times || !ch.values) return fail(c, SWR_ERR_INVALID_ARG, "a channel's times or values are null");
        uint8_t& t = taken[3 * (size_t)ch.node + (size_t)ch.path];
        if (t) return fail(c, SWR_ERR_INVALID_ARG, "two channels target the same node and path");
        t = 1;
        for (int q = 0; q + 1 < ch.n_keys; ++q)
            if (!(ch.times[q + 1] >= ch.times[q])) return fail(c, SWR_ERR_INVALID_ARG, "key times must not decrease (or be NaN)");
        words += 2 + (size_t)ch.n_keys * (ch.path == SWR_ANIM_PATH_ROTATION ? 5 : 4);
    }
    if (words >= ((size_t)1 << 30)) return fail(c, SWR_ERR_UNSUPPORTED, "the skeleton's clips exceed 2^30 words");
    // the new blob on the host, then in a new allocation; the old one is freed once the device is idle (a queued k_pose_sample may
    // read it) -- a load-time call
    std::vector<uint32_t> blob = k->clips;
    const uint32_t base = (uint32_t)blob.size();
    blob.resize(words, 0u);
    size_t at = base + 3 * nn;
    for (int i = 0; i < n_channels; ++i) {
        const swr_anim_channel& ch = channels[i];
        const size_t comps = ch.path == SWR_ANIM_PATH_ROTATION ? 4 : 3, nk = (size_t)ch.n_keys;
        blob[base + 3 * (size_t)ch.node + (size_t)ch.path] = (uint32_t)at;
        blob[at] = (uint32_t)ch.interpolation; blob[at + 1] = (uint32_t)ch.n_keys;
        memcpy(&blob[at + 2], ch.times, 4 * nk);
        memcpy(&blob[at + 2 + nk], ch.values, 4 * nk * comps);
        at += 2 + nk * (1 + comps);
    }
    uint32_t* d_new = nullptr;
    SWR_HIP(c, hipMalloc((void**)&d_new, words * 4));
    hipError_t e = hipMemcpy(d_new, blob.data(), words * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && k->d_clips) { e = hipDeviceSynchronize(); ++c->host_syncs; }
    if (e != hipSuccess) { (void)hipFree(d_new); SWR_HIP(c, e); }
    if (k->d_clips) (void)hipFree(k->d_clips);
    k->d_clips = d_new;
    k->clips.swap(blob);
    *clip_index = (int)k->clip_base.size();
    k->clip_base.push_back(base);
    return SWR_OK;
}

int swr_pose_set_create(swr_context* c, int n_instances, int n_joints, swr_pose_set** out) {
    SWR_ENTER(c);
    if (!out) return fail(c, SWR_ERR_INVALID_ARG, "out is null");
    if (n_instances < 1 || n_joints < 1) return fail(c, SWR_ERR_INVALID_ARG, "a pose set has at least one instance and one joint");
    if (n_joints > 65535 || (size_t)n_instances * (size_t)n_joints > ((size_t)1 << 24))
        return fail(c, SWR_ERR_UNSUPPORTED, "a pose set holds at most 65535 joints per instance and 2^24 matrices");
    swr_pose_set* p = new swr_pose_set();
    p->owner = c; p->n_instances = n_instances; p->n_joints = n_joints;
    const size_t bytes = (size_t)n_instances * (size_t)n_joints * 64;
    hipError_t e = hipMalloc((void**)&p->d_palettes, bytes);
    if (e == hipSuccess) e = hipMemset(p->d_palettes, 0, bytes);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);          // (the streams of a context do not wait for the null stream)
    if (e == hipSuccess) e = hipEventCreateWithFlags(&p->written, hipEventDisableTiming);
    if (e != hipSuccess) {
        destroy_pose_set(p);
        c->err = std::string("pose set allocation failed: ") + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? SWR_ERR_OOM : SWR_ERR_HIP;
    }
    *out = p;
    return SWR_OK;
}

int swr_pose_set_destroy(swr_context* c, swr_pose_set* p) {
    SWR_ENTER(c);
    if (!p) return SWR_OK;
    int rc = pose_set_check(c, p); if (rc) return rc;
    destroy_pose_set(p);                       // (hipFree waits for the device: the kernels queued on the set are over by then)
    return SWR_OK;
}

int swr_pose_set_sample(swr_context* c, swr_pose_set* p, const swr_skeleton* k, const swr_pose_request* requests, int n) {
    SWR_ENTER(c);
    int rc;
    if ((rc = pose_set_check(c, p)) || (rc = skeleton_check(c, k))) return rc;
    if (n < 0 || n > p->n_instances) return fail(c, SWR_ERR_INVALID_ARG, "n must be within 0 .. n_instances");
    if (n > 0 && !requests) return fail(c, SWR_ERR_INVALID_ARG, "requests is null");
    if (k->n_joints != p->n_joints) return fail(c, SWR_ERR_INVALID_ARG, "the pose set's joint count is not the skeleton's");
    const int n_clips = (int)k->clip_base.size();
    for (int i = 0; i < n; ++i)
        if (requests[i].clip_a < 0 || requests[i].clip_a >= n_clips || requests[i].clip_b >= n_clips)
            return fail(c, SWR_ERR_INVALID_ARG, "a request names a clip the skeleton does not have");
    if (n == 0) return SWR_OK;
    if ((rc = ensure_front_stream(c))) return rc;
    if (p->world_nodes < k->n_nodes) {
        // the node matrices grow to the largest skeleton the set was sampled with (hipFree waits for the device: the first sample, once)
        if (p->d_worlds) { SWR_HIP(c, hipFree(p->d_worlds)); p->d_worlds = nullptr; p->world_nodes = 0; }
        SWR_HIP(c, hipMalloc((void**)&p->d_worlds, (size_t)p->n_instances * (size_t)k->n_nodes * 64));
        p->world_nodes = k->n_nodes;
    }
    const hipStream_t s = use_front_stream(c);
    const size_t bytes = (size_t)n * sizeof(PoseRequestDev);
    PaletteSlot* slot = nullptr;
    if ((rc = palette_slot(c, bytes, &slot))) return rc;
    PoseRequestDev* rq = static_cast<PoseRequestDev*>(slot->host.p);
    for (int i = 0; i < n; ++i) {
        const swr_pose_request& r = requests[i];
        rq[i] = PoseRequestDev{ k->clip_base[(size_t)r.clip_a], r.time_a, r.clip_b < 0 ? SWR_ANIM_NO_CLIP : k->clip_base[(size_t)r.clip_b], r.time_b, r.weight };
    }
    SWR_HIP(c, hipMemcpyAsync(slot->dev.p, slot->host.p, bytes, hipMemcpyHostToDevice, s));
    const size_t nn = (size_t)k->n_nodes, nj = (size_t)k->n_joints;
    const float* f = static_cast<const float*>(k->d_static);
    SkeletonDev sk{};
    sk.rest_local = f; sk.inverse_bind = f + 16 * nn; sk.rest_t = sk.inverse_bind + 16 * nj; sk.rest_r = sk.rest_t + 3 * nn; sk.rest_s = sk.rest_r + 4 * nn;
    sk.parent = reinterpret_cast<const int32_t*>(sk.rest_s + 3 * nn); sk.order = sk.parent + nn; sk.level_start = sk.order + nn;
    sk.joint_node = sk.level_start + (size_t)k->n_levels + 1;
    sk.n_nodes = (uint32_t)k->n_nodes; sk.n_joints = (uint32_t)k->n_joints; sk.n_levels = (uint32_t)k->n_levels;
    hipLaunchKernelGGL(k_pose_sample, dim3((uint32_t)n), dim3(SWR_POSE_BLOCK), 0, s, sk, (const uint32_t*)k->d_clips,
                       (const PoseRequestDev*)slot->dev.p, reinterpret_cast<float4*>(p->d_worlds), reinterpret_cast<float4*>(p->d_palettes),
                       (uint32_t)p->n_joints * 16u);
    SWR_HIP(c, hipGetLastError());
    SWR_HIP(c, hipEventRecord(slot->done, s));
    slot->busy = true;
    return pose_set_written(c, p, s);
}

int swr_pose_set_upload(swr_context* c, swr_pose_set* p, int first, int n, const float* palettes) {
    SWR_ENTER(c);
    int rc = pose_set_check(c, p); if (rc) return rc;
    if (first < 0 || n < 0 || first > p->n_instances || n > p->n_instances - first) return fail(c, SWR_ERR_INVALID_ARG, "first .. first + n - 1 must be instances of the set");
    if (n > 0 && !palettes) return fail(c, SWR_ERR_INVALID_ARG, "palettes is null");
    if (n == 0) return SWR_OK;
    if ((rc = ensure_front_stream(c))) return rc;
    const hipStream_t s = use_front_stream(c);
    const size_t stride = (size_t)p->n_joints * 16, bytes = (size_t)n * stride * 4;
    PaletteSlot* slot = nullptr;
    if ((rc = palette_slot(c, bytes, &slot, false))) return rc;
    memcpy(slot->host.p, palettes, bytes);
    SWR_HIP(c, hipMemcpyAsync(p->d_palettes + (size_t)first * stride, slot->host.p, bytes, hipMemcpyHostToDevice, s));
    SWR_HIP(c, hipEventRecord(slot->done, s));
    slot->busy = true;
    return pose_set_written(c, p, s);
}

int swr_pose_set_readback(swr_context* c, const swr_pose_set* set, float* out) {
    SWR_ENTER(c);
    int rc = pose_set_check(c, set); if (rc) return rc;
    if (!out) return fail(c, SWR_ERR_INVALID_ARG, "the destination is null");
    // a reader on the ray stream, as swr_mesh_readback: behind the set's last write and behind nothing else
    if ((rc = ensure_ray_stream(c))) return rc;
    swr_pose_set* p = const_cast<swr_pose_set*>(set);
    if (!p->written_seen) { SWR_HIP(c, hipStreamWaitEvent(c->ray_stream, p->written, 0)); p->written_seen = true; }
    SWR_HIP(c, hipMemcpyAsync(out, p->d_palettes, (size_t)p->n_instances * (size_t)p->n_joints * 64, hipMemcpyDeviceToHost, c->ray_stream));
    SWR_HIP(c, hipStreamSynchronize(c->ray_stream));
    return SWR_OK;
}

int swr_mesh_skin_batch(swr_context* c, int n, swr_mesh* const* dst, const swr_mesh* const* src, const swr_pose_set* set, const int32_t* instance) {
    SWR_ENTER(c);
    int rc = pose_set_check(c, set); if (rc) return rc;
    if (n < 0) return fail(c, SWR_ERR_INVALID_ARG, "n is negative");
    if (n == 0) return SWR_OK;
    if (!dst || !src || !instance) return fail(c, SWR_ERR_INVALID_ARG, "dst, src or instance is null");
    std::vector<const swr_mesh*> dsts((size_t)n);
    uint64_t blocks = 0;
    for (int k = 0; k < n; ++k) {
        if ((rc = deform_mesh_check(c, dst[k], "a destination mesh is null"))) return rc;
        if ((rc = deform_mesh_check(c, src[k], "a source mesh is null"))) return rc;
        if (src[k]->n_verts != dst[k]->n_verts) return fail(c, SWR_ERR_INVALID_ARG, "a job's source and destination must have equal vertex counts");
        if (!src[k]->has_skin) return fail(c, SWR_ERR_INVALID_ARG, "a source mesh has no skin attributes (swr_mesh_set_skin)");
        if (instance[k] < 0 || instance[k] >= set->n_instances) return fail(c, SWR_ERR_INVALID_ARG, "an instance is not one of the pose set's");
        if (set->n_joints <= src[k]->max_joint) return fail(c, SWR_ERR_INVALID_ARG, "the pose set's n_joints must exceed the largest joint index a source's skin attributes use");
        dsts[(size_t)k] = dst[k];
        blocks += ((uint64_t)dst[k]->n_verts + SWR_DEFORM_BLOCK - 1u) / SWR_DEFORM_BLOCK;
    }
    std::sort(dsts.begin(), dsts.end());
    if (std::adjacent_find(dsts.begin(), dsts.end()) != dsts.end()) return fail(c, SWR_ERR_INVALID_ARG, "a destination mesh appears twice in the batch");
    for (int k = 0; k < n; ++k)
        if (std::binary_search(dsts.begin(), dsts.end(), src[k])) return fail(c, SWR_ERR_INVALID_ARG, "a destination mesh is a job's source (make a target with swr_mesh_create_like)");
    if (blocks == 0) return SWR_OK;
    if (blocks > 0x7fffffffull) return fail(c, SWR_ERR_UNSUPPORTED, "the batch exceeds 2^31 blocks of vertices");
    // deform_begin's rules A and B, once over all destinations
    const auto reads_a_dst = [&](const std::vector<DrawCmd>& draws) {
        for (const DrawCmd& d : draws) if (std::binary_search(dsts.begin(), dsts.end(), (const swr_mesh*)d.mesh)) return true;
        return false;
    };
    if (reads_a_dst(c->draws) && (rc = flush_locked(c))) return rc;
    bool in_flight = false;
    for (const Batch& b : c->inflight) in_flight = in_flight || reads_a_dst(b.draws);
    if (in_flight && (rc = sync_locked(c))) return rc;
    if ((rc = ensure_front_stream(c))) return rc;
    const hipStream_t s = use_front_stream(c);
    // the job table: jobs with vertices, by first block
    PaletteSlot* slot = nullptr;
    if ((rc = palette_slot(c, (size_t)n * sizeof(SkinJob), &slot))) return rc;
    SkinJob* jobs = static_cast<SkinJob*>(slot->host.p);
    uint32_t n_jobs = 0, first_block = 0;
    for (int k = 0; k < n; ++k) {
        if (dst[k]->n_verts == 0) continue;
        jobs[n_jobs++] = SkinJob{ src[k]->d_verts, src[k]->d_joints, src[k]->d_weights, dst[k]->d_verts, (uint32_t)dst[k]->n_verts, first_block,
                                  (uint32_t)instance[k] * (uint32_t)set->n_joints * 16u, 0u };
        first_block += ((uint32_t)dst[k]->n_verts + SWR_DEFORM_BLOCK - 1u) / SWR_DEFORM_BLOCK;
    }
    SWR_HIP(c, hipMemcpyAsync(slot->dev.p, slot->host.p, (size_t)n_jobs * sizeof(SkinJob), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_mesh_skin_batch, dim3(first_block), dim3(SWR_DEFORM_BLOCK), 0, s, (const SkinJob*)slot->dev.p, n_jobs,
                       (const float*)set->d_palettes, c->nm_flags);
    SWR_HIP(c, hipGetLastError());
    SWR_HIP(c, hipEventRecord(slot->done, s));
    slot->busy = true;
    // deform_end for every destination, with ONE event behind the kernel for rule C instead of one per mesh: the destinations share it
    std::shared_ptr<SharedEvent> ev;
    for (auto& e : c->pose_events) if (e.use_count() == 1) { ev = e; break; }          // no mesh holds it: its waits were issued long ago
    if (!ev) {
        ev = std::make_shared<SharedEvent>();
        SWR_HIP(c, hipEventCreateWithFlags(&ev->ev, hipEventDisableTiming));
        c->pose_events.push_back(ev);
    }
    SWR_HIP(c, hipEventRecord(ev->ev, s));
    for (int k = 0; k < n; ++k) {
        if (dst[k]->n_verts == 0) continue;
        dst[k]->posed = ev;
        dst[k]->upload_seen = false;
        dst[k]->bounds_ready = false;
        dst[k]->has_box = false;
    }
    return SWR_OK;
}

int swr_set_state(swr_context* c, float near_clip, float far_clip, int debug_mode) {
    SWR_ENTER(c);
    if (debug_mode != SWR_DEBUG_NONE && debug_mode != SWR_DEBUG_WIREFRAME) return fail(c, SWR_ERR_INVALID_ARG, "bad debug mode");
    if (!c->draws.empty() && (near_clip != c->near_clip || debug_mode != c->debug_mode)) {
        int rc = flush_locked(c); if (rc) return rc;     // NearClip is read at clip time (Rasterizer.cs:112)
    }
    c->near_clip = near_clip; c->far_clip = far_clip; c->debug_mode = debug_mode;
    return SWR_OK;
}

int swr_initialize_tile_locks(swr_context* c, int width, int height) {
    SWR_ENTER(c);
    if (width <= 0 || height <= 0)                                 // Rasterizer.cs:71-74
        return fail(c, SWR_ERR_INVALID_ARG, "Width and height must be positive non-zero values.");
    return SWR_OK;    // tiles need no locks here: one wave owns one tile
}

int swr_render_mesh(swr_context* c, const swr_mesh* mesh, const float model[16], const float view[16], const float proj[16],
                    int program, const swr_uniforms* u, const swr_texture* tex, int cull, int depth_test, int blend) {
    SWR_ENTER(c); return record_draw(c, const_cast<swr_mesh*>(mesh), model, view, proj, program, u, tex, cull, depth_test, blend);
}

int swr_render_mesh_culled(swr_context* c, const swr_mesh* mesh, const float model[16], const float view[16], const float proj[16],
                           int program, const swr_uniforms* u, const swr_texture* tex, int cull, int depth_test, int blend) {
    SWR_ENTER(c); return record_draw(c, const_cast<swr_mesh*>(mesh), model, view, proj, program, u, tex, cull, depth_test, blend, true);
}

int swr_mesh_bounds(swr_context* c, const swr_mesh* mesh, float center_radius[4]) {
    SWR_ENTER(c);
    if (!mesh || !center_radius) return fail(c, SWR_ERR_INVALID_ARG, "bad mesh_bounds arguments");
    int rc = ensure_bounds(c, const_cast<swr_mesh*>(mesh));
    if (rc) return rc;
    SWR_HIP(c, hipMemcpyAsync(center_radius, mesh->d_bounds, 16, hipMemcpyDeviceToHost, use_front_stream(c)));
    SWR_HIP(c, hipStreamSynchronize(use_front_stream(c)));
    return SWR_OK;
}

int swr_raycast(swr_context* c, const swr_ray* rays, int n_rays, const swr_ray_target* targets, int n_targets, int flags, swr_ray_hit* out) {
    SWR_ENTER(c); return raycast(c, rays, n_rays, targets, n_targets, flags, out, false);
}
int swr_raycast_nearest(swr_context* c, const swr_ray* rays, int n_rays, const swr_ray_target* targets, int n_targets, int flags, swr_ray_hit* out) {
    SWR_ENTER(c); return raycast(c, rays, n_rays, targets, n_targets, flags, out, true);
}
int swr_character_ray_counts(const swr_character_params* params, int* vertical_steps, int* horizontal_rays) {
    if (!params || !vertical_steps || !horizontal_rays) return SWR_ERR_INVALID_ARG;
    return character_ray_counts(params, vertical_steps, horizontal_rays) ? SWR_OK : SWR_ERR_UNSUPPORTED;
}
int swr_character_update(swr_context* c, const swr_character_params* params, swr_character* chars, const swr_character_input* inputs, int n, float delta_time,
                         const float* ring, int n_ring, const swr_ray_target* targets, int n_targets, int flags, swr_character_trace* trace) {
    SWR_ENTER(c); return character_update(c, params, chars, inputs, n, delta_time, ring, n_ring, targets, n_targets, flags, trace);
}

int swr_is_sphere_in_frustum(swr_context* c, const float center_radius[4], const float model[16], const float view[16],
                             const float proj[16], int* inside) {
    SWR_ENTER(c);
    if (!center_radius || !model || !view || !proj || !inside) return fail(c, SWR_ERR_INVALID_ARG, "bad is_sphere_in_frustum arguments");
    int rc = ensure(c, c->d_scratch, 256);
    if (rc) return rc;
    float h[48];
    memcpy(h, model, 64); memcpy(h + 16, view, 64); memcpy(h + 32, proj, 64);
    char* base = reinterpret_cast<char*>(c->d_scratch.p);
    SWR_HIP(c, hipMemcpyAsync(base, h, sizeof h, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_frustum_test, dim3(1), dim3(64), 0, c->stream,
                       make_float4(center_radius[0], center_radius[1], center_radius[2], center_radius[3]),
                       (const float*)base, (uint32_t*)(base + 192), c->nm_flags);
    SWR_HIP(c, hipGetLastError());
    uint32_t r = 0;
    SWR_HIP(c, hipMemcpyAsync(&r, base + 192, 4, hipMemcpyDeviceToHost, c->stream));
    SWR_HIP(c, hipStreamSynchronize(c->stream));
    *inside = (int)r;
    return SWR_OK;
}

int swr_program_validate(const char* src, char* log, int log_len) { return swr_program_validate_vf(nullptr, src, log, log_len); }

int swr_program_validate_vf(const char* vertex_src, const char* src, char* log, int log_len) {
    if (!src) return SWR_ERR_INVALID_ARG;
    std::shared_ptr<const RtcCode> code;
    std::string msg;
    const int rc = rtc_compile(vertex_src, src, code, msg);
    copy_log(msg, log, log_len);
    return rc;
}

int swr_program_create(swr_context* c, const char* src, int* program_id) { return swr_program_create_vf(c, nullptr, src, program_id); }

int swr_program_create_vf(swr_context* c, const char* vertex_src, const char* src, int* program_id) {
    SWR_ENTER(c);
    if (!src || !program_id) return fail(c, SWR_ERR_INVALID_ARG, "null argument to swr_program_create");
    std::shared_ptr<const RtcCode> code;
    std::string log;
    const int rc = rtc_compile(vertex_src, src, code, log);
    if (rc) { c->err = log; return rc; }
    auto p = std::make_shared<UserProg>();
    SWR_HIP(c, hipModuleLoadData(&p->mod, code->code.data()));
    for (int k = 0; k < 2; ++k) SWR_HIP(c, hipModuleGetFunction(&p->fn[k], p->mod, code->names[k].c_str()));
    if (code->has_vertex) {
        SWR_HIP(c, hipModuleGetFunction(&p->vertex_fn, p->mod, code->names[2].c_str()));
        SWR_HIP(c, hipModuleGetFunction(&p->setup_fn, p->mod, code->names[3].c_str()));
    }
    const int id = c->next_prog++;
    c->progs[id] = std::move(p);
    *program_id = id;
    return SWR_OK;
}

int swr_program_destroy(swr_context* c, int program_id) {
    SWR_ENTER(c);
    auto it = c->progs.find(program_id);
    if (it == c->progs.end()) return fail(c, SWR_ERR_INVALID_ARG, "unknown or destroyed user program id");
    c->progs.erase(it);                  // draws already recorded hold the program until their batch is over
    return SWR_OK;
}

int swr_program_set_constants(swr_context* c, int program_id, const float* values, int n) {
    SWR_ENTER(c);
    auto it = c->progs.find(program_id);
    if (it == c->progs.end()) return fail(c, SWR_ERR_INVALID_ARG, "unknown or destroyed user program id");
    if (n < 0 || n > 64 || (n > 0 && !values)) return fail(c, SWR_ERR_INVALID_ARG, "between 0 and 64 constants");
    float* k = it->second->constants;
    for (int i = 0; i < 64; ++i) k[i] = i < n ? values[i] : 0.0f;
    return SWR_OK;
}

int swr_program_set_texture(swr_context* c, int program_id, int slot, const swr_texture* tex) {
    SWR_ENTER(c);
    auto it = c->progs.find(program_id);         // (user ids only: a built-in id is never in the table)
    if (it == c->progs.end()) return fail(c, SWR_ERR_INVALID_ARG, "unknown or destroyed user program id");
    if (slot < 1 || slot >= SWR_PROGRAM_TEXTURES)
        return fail(c, SWR_ERR_INVALID_ARG, "a user program owns texture slots 1 to 3 (slot 0 is the render call's texture)");
    it->second->tex[slot - 1] = tex;      // read, with the texture's filter, when a draw is recorded
    return SWR_OK;
}

int swr_post_validate(const char* src, char* log, int log_len) {
    if (!src) return SWR_ERR_INVALID_ARG;
    std::shared_ptr<const RtcCode> code;
    std::string msg;
    const int rc = rtc_compile_post(src, code, msg);
    copy_log(msg, log, log_len);
    return rc;
}

int swr_post_create(swr_context* c, const char* src, int* post_id) {
    SWR_ENTER(c);
    if (!src || !post_id) return fail(c, SWR_ERR_INVALID_ARG, "null argument to swr_post_create");
    std::shared_ptr<const RtcCode> code;
    std::string log;
    const int rc = rtc_compile_post(src, code, log);
    if (rc) { c->err = log; return rc; }
    auto p = std::make_shared<PostProg>();
    SWR_HIP(c, hipModuleLoadData(&p->mod, code->code.data()));
    for (int k = 0; k < POST_KERNELS; ++k) SWR_HIP(c, hipModuleGetFunction(&p->fn[k], p->mod, code->names[k].c_str()));
    static std::atomic<int> next_post{1};                   // one sequence for the process: another context's id is unknown here
    const int id = next_post++;
    c->posts[id] = std::move(p);
    *post_id = id;
    return SWR_OK;
}

int swr_post_destroy(swr_context* c, int post_id) {
    SWR_ENTER(c);
    auto it = c->posts.find(post_id);
    if (it == c->posts.end()) return fail(c, SWR_ERR_INVALID_ARG, "unknown or destroyed post program id");
    c->post_garbage.push_back(std::move(it->second));      // its k_post may be in flight: the module stays loaded until the streams are idle
    c->posts.erase(it);
    return SWR_OK;
}

int swr_post_set_constants(swr_context* c, int post_id, const float* values, int n) {
    SWR_ENTER(c);
    auto it = c->posts.find(post_id);
    if (it == c->posts.end()) return fail(c, SWR_ERR_INVALID_ARG, "unknown or destroyed post program id");
    if (n < 0 || n > SWR_POST_CONSTANTS || (n > 0 && !values)) return fail(c, SWR_ERR_INVALID_ARG, "between 0 and 64 constants");
    float* k = it->second->constants.v;
    for (int i = 0; i < SWR_POST_CONSTANTS; ++i) k[i] = i < n ? values[i] : 0.0f;
    return SWR_OK;
}

int swr_post_set_texture(swr_context* c, int post_id, int slot, const swr_texture* tex) {
    SWR_ENTER(c);
    auto it = c->posts.find(post_id);
    if (it == c->posts.end()) return fail(c, SWR_ERR_INVALID_ARG, "unknown or destroyed post program id");
    if (slot < 0 || slot >= SWR_POST_TEXTURES) return fail(c, SWR_ERR_INVALID_ARG, "a post program has texture slots 0 to 3");
    it->second->tex[slot] = tex;          // read, with the texture's filter, when a present is called
    return SWR_OK;
}

int swr_post_size(swr_context* c, int kx, int ky, int format, int* out_width, int* out_rows, size_t* out_bytes) {
    SWR_ENTER(c);
    if (!out_width || !out_rows || !out_bytes) return fail(c, SWR_ERR_INVALID_ARG, "out_width, out_rows or out_bytes is null");
    const Payload p = posted(c, 0, kx, ky, format);
    int rc = payload_check(c, p, false); if (rc) return rc;
    *out_width = payload_width(c, p); *out_rows = payload_rows(c, p); *out_bytes = payload_bytes(c, p);
    return SWR_OK;
}

int swr_readback_post(swr_context* c, int post_id, int kx, int ky, int format, void* out) {
    SWR_ENTER(c);
    return payload_readback(c, posted(c, post_id, kx, ky, format), out);
}
int swr_present_post_async(swr_context* c, int post_id, int kx, int ky, int format, void* out, uint64_t* ticket) {
    SWR_ENTER(c);
    return payload_present(c, posted(c, post_id, kx, ky, format), out, ticket);
}
int swr_post_device(swr_context* c, int post_id, int kx, int ky, int format, void* d_out) {
    SWR_ENTER(c);
    return payload_device(c, posted(c, post_id, kx, ky, format), d_out, true);
}
int swr_post_device_async(swr_context* c, int post_id, int kx, int ky, int format, void* d_out) {
    SWR_ENTER(c);
    return payload_device(c, posted(c, post_id, kx, ky, format), d_out, false);
}

int swr_render_mesh_arrays(swr_context* c, const swr_vertex* v, int nv, const uint16_t* idx, int ni,
                           const float model[16], const float view[16], const float proj[16],
                           int program, const swr_uniforms* u, const swr_texture* tex, int cull, int depth_test, int blend) {
    SWR_ENTER(c);
    if (c->W <= 0 || c->H <= 0) return SWR_OK;                     // Rasterizer.cs:176
    swr_mesh* m = nullptr;
    int rc = make_mesh(c, v, nv, idx, ni, true, &m);
    if (rc) return rc;
    rc = record_draw(c, m, model, view, proj, program, u, tex, cull, depth_test, blend);
    // by identity (record_draw may have flushed the pending list first): a draw references m iff it is the last one recorded
    if (rc || c->draws.empty() || c->draws.back().mesh != m) c->garbage.push_back(m);
    return rc;
}

int swr_interpolate(swr_context* c, const float* verts60, const float* w, int n, int interpolate, float* out) {
    SWR_ENTER(c);
    if (!verts60 || !w || !out || n < 0) return fail(c, SWR_ERR_INVALID_ARG, "bad interpolate arguments");
    if (n == 0) return SWR_OK;
    const size_t off_w = 256, off_o = 256 + (((size_t)n * 12 + 15) & ~(size_t)15);
    int rc = ensure(c, c->d_scratch, off_o + (size_t)n * 96);
    if (rc) return rc;
    char* base = reinterpret_cast<char*>(c->d_scratch.p);
    SWR_HIP(c, hipMemcpyAsync(base, verts60, 240, hipMemcpyHostToDevice, c->stream));
    SWR_HIP(c, hipMemcpyAsync(base + off_w, w, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_interpolate, dim3((n + 255) / 256), dim3(256), 0, c->stream,
                       (const float*)base, (const float*)(base + off_w), n, interpolate, (float*)(base + off_o));
    SWR_HIP(c, hipGetLastError());
    SWR_HIP(c, hipMemcpyAsync(out, base + off_o, (size_t)n * 96, hipMemcpyDeviceToHost, c->stream));
    return sync_locked(c);
}

int swr_get_stats(swr_context* c, swr_stats* out) {
    SWR_ENTER(c);
    if (!out) return SWR_ERR_INVALID_ARG;
    int rc = flush_and_sync_locked(c); if (rc) return rc;   // validate (and replay) optimistic batches BEFORE the counters are gathered
    Counters host[65];
    unsigned long long frag[3] = { 0, 0, 0 };
    if (c->tile_stats_tiles) {
        unsigned long long* d3 = c->d_total.as<unsigned long long>() + 1;
        hipLaunchKernelGGL(k_reduce_tile_stats, dim3(1), dim3(1024), 0, c->stream, c->d_tile_stats.as<uint32_t>(),
                           (uint32_t)c->tile_stats_tiles, d3, 0);
        SWR_HIP(c, hipGetLastError());
        SWR_HIP(c, hipMemcpyAsync(frag, d3, 24, hipMemcpyDeviceToHost, c->stream));
    }
    unsigned long long carry[3] = { 0, 0, 0 };      // counters of earlier geometries (see the tile_stats_tiles change in the flush)
    SWR_HIP(c, hipMemcpyAsync(carry, c->d_total.as<unsigned long long>() + 4, 24, hipMemcpyDeviceToHost, c->stream));
    SWR_HIP(c, hipMemcpyAsync(host, c->d_counters.p, sizeof host, hipMemcpyDeviceToHost, c->stream));
    if ((rc = sync_locked(c))) return rc;
    swr_stats s = {};
    for (int i = 0; i < 65; ++i) {
        s.triangles_in += host[i].triangles_in; s.triangles_setup += host[i].triangles_setup;
        s.triangles_clipped += host[i].triangles_clipped; s.tile_pairs += host[i].tile_pairs;
    }
    s.fragments_tested = frag[0] + carry[0]; s.fragments_shaded = frag[1] + carry[1]; s.fragments_written = frag[2] + carry[2];
    s.tile_pairs += c->host_tile_pairs;
    s.flushes = c->totals.flushes;
    *out = s;
    return SWR_OK;
}

int swr_reset_stats(swr_context* c) {
    SWR_ENTER(c);
    int rc = flush_locked(c); if (rc) return rc;
    SWR_HIP(c, hipMemsetAsync(c->d_counters.p, 0, 65 * sizeof(Counters), c->stream));
    if (c->tile_stats_tiles) SWR_HIP(c, hipMemsetAsync(c->d_tile_stats.p, 0, c->tile_stats_tiles * 12, c->stream));
    SWR_HIP(c, hipMemsetAsync(c->d_total.as<unsigned long long>() + 4, 0, 24, c->stream));
    c->totals = {}; c->host_tile_pairs = 0;
    return sync_locked(c);
}

int swr_profile_enable(swr_context* c, int on) {
    SWR_ENTER(c);
    int rc = flush_and_sync_locked(c); if (rc) return rc;
    c->profiling = on < 0 ? 0 : (on > 3 ? 1 : on);
    c->raster_span_no = 0;
    return SWR_OK;
}
int swr_profile_get(swr_context* c, swr_profile* out) {
    SWR_ENTER(c);
    if (!out) return SWR_ERR_INVALID_ARG;
    int rc = flush_and_sync_locked(c); if (rc) return rc;
    c->prof.flushes = c->totals.flushes;
    *out = c->prof;
    return SWR_OK;
}
int swr_profile_reset(swr_context* c) {
    SWR_ENTER(c);
    int rc = flush_and_sync_locked(c); if (rc) return rc;
    c->prof = {};
    c->raster_samples.clear();
    return SWR_OK;
}
int swr_profile_raster_samples(swr_context* c, float* out_ms, int capacity, int* n) {
    SWR_ENTER(c);
    if (!n || capacity < 0 || (capacity > 0 && !out_ms)) return SWR_ERR_INVALID_ARG;
    int rc = flush_and_sync_locked(c); if (rc) return rc;
    const int have = (int)c->raster_samples.size();
    for (int i = 0; i < std::min(have, capacity); ++i) out_ms[i] = c->raster_samples[(size_t)i];
    *n = have;
    return SWR_OK;
}

int swr_debug_counters(swr_context* c, uint64_t out[8]) {
    SWR_ENTER(c);
    if (!out) return SWR_ERR_INVALID_ARG;
    int rc = flush_and_sync_locked(c); if (rc) return rc;
    SWR_HIP(c, hipMemcpyAsync(out, c->d_total.as<unsigned long long>() + 8, 64, hipMemcpyDeviceToHost, c->stream));
    if ((rc = sync_locked(c))) return rc;
    SWR_HIP(c, hipMemsetAsync(c->d_total.as<unsigned long long>() + 8, 0, 64, c->stream));
    return SWR_OK;
}

int swr_selftest_division(swr_context* c, uint64_t samples, uint64_t seed, uint64_t out[8]) {
    SWR_ENTER(c);
    if (!out) return SWR_ERR_INVALID_ARG;
    int rc = flush_locked(c); if (rc) return rc;
    if ((rc = ensure(c, c->d_scratch, 64))) return rc;
    SWR_HIP(c, hipMemsetAsync(c->d_scratch.p, 0, 64, c->stream));
    const int iters = 1024;
    const uint64_t per_block = 256ull * (uint64_t)iters;
    const unsigned blocks = (unsigned)std::min<uint64_t>((samples + per_block - 1) / per_block, 1u << 20);
    if (blocks) hipLaunchKernelGGL(k_selftest_division, dim3(blocks), dim3(256), 0, c->stream, (unsigned long long)seed, iters,
                                   c->d_scratch.as<unsigned long long>());
    SWR_HIP(c, hipGetLastError());
    // reciprocals (recip_core): exhaustive over its whole range, whatever `samples` says
    hipLaunchKernelGGL(k_selftest_recip, dim3(16384), dim3(256), 0, c->stream, c->d_scratch.as<unsigned long long>());
    SWR_HIP(c, hipGetLastError());
    SWR_HIP(c, hipMemcpyAsync(out, c->d_scratch.p, 64, hipMemcpyDeviceToHost, c->stream));
    return sync_locked(c);
}

int swr_device_name(swr_context* c, char* buf, int buflen) {
    SWR_ENTER(c);
    if (!buf || buflen <= 0) return SWR_ERR_INVALID_ARG;
    snprintf(buf, (size_t)buflen, "%s", c->dev_name);
    return SWR_OK;
}

}  // extern "C"
