// swr_api.hip -- host side of libswr_hip.so: the C ABI of include/swr.h over the gfx950 kernels.
//
// A context records draws (Rasterizer.RenderMesh calls, Rasterizer.cs:163-174) in submission order
// and executes them as ONE batch per flush:
//     [k_frustum_cull ->] k_vertex -> k_setup -> k_bin<count> -> k_scan_sums/apply -> k_bin<fill> -> k_sort_tiles
//     (+ the tile order in its last blocks) -> k_cover -> k_raster_c
// There is no CPU fallback anywhere in this file: every pixel is produced by the HIP kernels.
// The host side is this file -- the payload and present shapes and the entry points -- over swr_host.h (the types), swr_rtc.h (run-time
// compilation), swr_flush.h (the flush path), swr_query.h (ray queries, the character update), swr_texture.h (textures and their probes)
// and swr_deform.h (deforming meshes, skeletal animation); swr_query_layout.h and swr_animation_layout.h hold their layouts without HIP types.
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
#include "swr_query.h"        // (swr_texture.h and swr_deform.h follow the payload shapes they use, below)

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

// swr_program_validate* / swr_post_validate: the compiler's messages, NUL-terminated and truncated to the caller's buffer
void copy_log(const std::string& msg, char* log, int log_len) {
    if (!log || log_len <= 0) return;
    const size_t n = std::min(msg.size(), (size_t)log_len - 1);
    memcpy(log, msg.data(), n); log[n] = '\0';
}
}  // namespace

#include "swr_texture.h"
#include "swr_deform.h"

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

int swr_texture_format(swr_context* c, const swr_texture* t, int* format) { SWR_ENTER(c); return texture_format(c, t, format); }
int swr_texture_set_filter(swr_context* c, swr_texture* t, int bilinear) { SWR_ENTER(c); return texture_set_filter(c, t, bilinear); }
int swr_texture_destroy(swr_context* c, swr_texture* t) { SWR_ENTER(c); return texture_destroy(c, t); }
int swr_texture_sample(swr_context* c, const swr_texture* t, const float* uv, int n, float* out) { SWR_ENTER(c); return texture_sample(c, t, uv, n, out); }
int swr_texture_sample_depth(swr_context* c, const swr_texture* t, const float* uv_ref, int n, float* out) { SWR_ENTER(c); return texture_sample_depth(c, t, uv_ref, n, out); }
int swr_texture_generate_mipmaps(swr_context* c, swr_texture* t) { SWR_ENTER(c); return texture_generate_mipmaps(c, t); }
int swr_texture_levels(swr_context* c, const swr_texture* t, int* levels) { SWR_ENTER(c); return texture_levels(c, t, levels); }
int swr_texture_level_size(swr_context* c, const swr_texture* t, int level, int* w, int* h) { SWR_ENTER(c); return texture_level_size(c, t, level, w, h); }
int swr_texture_readback_level(swr_context* c, const swr_texture* t, int level, uint8_t* rgba8) { SWR_ENTER(c); return texture_readback_level(c, t, level, rgba8); }
int swr_texture_sample_lod(swr_context* c, const swr_texture* t, const float* uv_lod, int n, float* out_rgba) { SWR_ENTER(c); return texture_sample_lod(c, t, uv_lod, n, out_rgba); }
int swr_texture_lod(swr_context* c, const swr_texture* t, const float* grads, int n, float* out_lod) { SWR_ENTER(c); return texture_lod(c, t, grads, n, out_lod); }
int swr_texture_create_cube(swr_context* c, const uint8_t* rgba8, int n, swr_texture** out) { SWR_ENTER(c); return cube_create(c, rgba8, n, out, SWR_TEXTURE_FORMAT_RGBA8); }
int swr_texture_create_cube_depth(swr_context* c, const float* depth, int n, swr_texture** out) { SWR_ENTER(c); return cube_create(c, depth, n, out, SWR_TEXTURE_FORMAT_DEPTH32F); }
int swr_texture_is_cube(swr_context* c, const swr_texture* t, int* n) { SWR_ENTER(c); return texture_is_cube(c, t, n); }
int swr_texture_update_face_from_frame(swr_context* c, swr_texture* t, int face, swr_context* src, int kx, int ky, int alpha_mode) {
    return texture_update_locked(c, t, src, TextureUpdate{ FROM_FRAME, kx, ky, alpha_mode, 0, face, true });
}
int swr_texture_update_face_from_depth(swr_context* c, swr_texture* t, int face, swr_context* src, int kx, int ky, int reduce) {
    return texture_update_locked(c, t, src, TextureUpdate{ FROM_DEPTH, kx, ky, reduce, 0, face, true });
}
int swr_texture_update_face_from_post(swr_context* c, swr_texture* t, int face, swr_context* src, int post_id, int kx, int ky, int alpha_mode) {
    return texture_update_locked(c, t, src, TextureUpdate{ FROM_POST, kx, ky, alpha_mode, post_id, face, true });
}

int swr_texture_readback_face(swr_context* c, const swr_texture* t, int face, int level, void* out) { SWR_ENTER(c); return texture_readback_face(c, t, face, level, out); }

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

int swr_texture_cube_face(swr_context* c, const float* dirs, int n, int* out_face, float* out_st) { SWR_ENTER(c); return texture_cube_face(c, dirs, n, out_face, out_st); }
int swr_texture_sample_cube(swr_context* c, const swr_texture* t, const float* dir_lod, int n, float* out_rgba) { SWR_ENTER(c); return texture_sample_cube(c, t, dir_lod, n, out_rgba); }
int swr_texture_sample_cube_depth(swr_context* c, const swr_texture* t, const float* dir_ref, int n, float* out) { SWR_ENTER(c); return texture_sample_cube_depth(c, t, dir_ref, n, out); }

int swr_mesh_create(swr_context* c, const swr_vertex* v, int nv, const uint16_t* idx, int ni, swr_mesh** out) { SWR_ENTER(c); return make_mesh(c, v, nv, idx, ni, false, out); }

int swr_mesh_destroy(swr_context* c, swr_mesh* m) {
    SWR_ENTER(c);
    if (!m) return SWR_OK;
    int rc = flush_and_sync_locked(c); if (rc) return rc;
    destroy_mesh(m);
    return SWR_OK;
}

// ---- deforming meshes and skeletal animation (section 29): swr_deform.h
int swr_mesh_create_like(swr_context* c, const swr_mesh* src, swr_mesh** out) { SWR_ENTER(c); return mesh_create_like(c, src, out); }
int swr_mesh_readback(swr_context* c, const swr_mesh* mesh, swr_vertex* out) { SWR_ENTER(c); return mesh_readback(c, mesh, out); }
int swr_mesh_blend(swr_context* c, swr_mesh* dst, const swr_mesh* a, const swr_mesh* b, float t) { SWR_ENTER(c); return mesh_blend(c, dst, a, b, t); }
int swr_mesh_set_skin(swr_context* c, swr_mesh* m, const uint16_t* joints4, const float* weights4) { SWR_ENTER(c); return mesh_set_skin(c, m, joints4, weights4); }
int swr_mesh_skin(swr_context* c, swr_mesh* dst, const swr_mesh* src, const float* palette, int n_joints) { SWR_ENTER(c); return mesh_skin(c, dst, src, palette, n_joints); }
int swr_mesh_skin_batch(swr_context* c, int n, swr_mesh* const* dst, const swr_mesh* const* src, const swr_pose_set* set, const int32_t* instance) {
    SWR_ENTER(c); return mesh_skin_batch(c, n, dst, src, set, instance);
}
int swr_skeleton_create(swr_context* c, int n_nodes, const int32_t* parent, const float* rest_local, const float* rest_t,
                        const float* rest_r, const float* rest_s, int n_joints, const int32_t* joint_node, const float* inverse_bind,
                        swr_skeleton** out) {
    SWR_ENTER(c); return skeleton_create(c, n_nodes, parent, rest_local, rest_t, rest_r, rest_s, n_joints, joint_node, inverse_bind, out);
}
int swr_skeleton_destroy(swr_context* c, swr_skeleton* k) { SWR_ENTER(c); return skeleton_destroy(c, k); }
int swr_skeleton_add_clip(swr_context* c, swr_skeleton* k, const swr_anim_channel* channels, int n_channels, int* clip_index) {
    SWR_ENTER(c); return skeleton_add_clip(c, k, channels, n_channels, clip_index);
}
int swr_pose_set_create(swr_context* c, int n_instances, int n_joints, swr_pose_set** out) { SWR_ENTER(c); return pose_set_create(c, n_instances, n_joints, out); }
int swr_pose_set_destroy(swr_context* c, swr_pose_set* p) { SWR_ENTER(c); return pose_set_destroy(c, p); }
int swr_pose_set_sample(swr_context* c, swr_pose_set* p, const swr_skeleton* k, const swr_pose_request* requests, int n) { SWR_ENTER(c); return pose_set_sample(c, p, k, requests, n); }
int swr_pose_set_upload(swr_context* c, swr_pose_set* p, int first, int n, const float* palettes) { SWR_ENTER(c); return pose_set_upload(c, p, first, n, palettes); }
int swr_pose_set_readback(swr_context* c, const swr_pose_set* set, float* out) { SWR_ENTER(c); return pose_set_readback(c, set, out); }

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
    const size_t off_w = 256, off_o = 256 + query_align((size_t)n * 12);
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
