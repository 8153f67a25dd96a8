// swr_texture.h -- host side of textures: creation, the updates from a frame (render to texture, depth textures, post passes), mip
// chains, cube maps and the batched probes (swr_texture_sample* / _lod / _cube_face).  Included by swr_api.hip only, behind the payload
// shapes it shares with the presents (deliver_shape, launch_post_over): that is also where the kernels its selectors instantiate have
// always stood in the translation unit, behind the resolve and present kernels.  The entry points in swr_api.hip are a call each.
#pragma once
#include "swr_query_layout.h"

namespace {
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

// MIP CHAINS.  Level l's first texel in the tail of t's chain, in texels (l >= 1) -- and, with l the chain's
// length, the texels the tail holds
uint32_t mip_tail_offset(const swr_texture* t, int l) {
    uint32_t at = 0;
    for (int k = 1; k < l; ++k) at += (uint32_t)mip_level_side(t->w, k) * (uint32_t)mip_level_side(t->h, k);
    return at;
}
// the device address of level `level`'s first texel: d_rgba for level 0, into d_tail otherwise
uint32_t* mip_level_texels(const swr_texture* t, int level) {
    return level == 0 ? reinterpret_cast<uint32_t*>(t->d_rgba) : reinterpret_cast<uint32_t*>(t->d_tail) + mip_tail_offset(t, level);
}
// the record in front of one of t's texel arrays (d_rgba or d_blocked) as t's chain is now, on the context's stream: in front of the
// texels' own upload at creation, behind the flushed draws (which read the old record) when a chain appears
hipError_t texture_header_write(swr_context* c, const swr_texture* t, uint8_t* texels) {
    TextureHeader h = {};
    h.levels = (uint32_t)t->levels;
    h.tail = t->levels > 1 ? t->d_tail : nullptr;
    for (int l = 1; l < t->levels; ++l) h.offset[l] = mip_tail_offset(t, l);
    hipLaunchKernelGGL(k_texture_header, dim3(1), dim3(64), 0, c->stream, reinterpret_cast<uint32_t*>(texels - SWR_TEXTURE_HEADER_BYTES), h);
    return hipGetLastError();
}
// levels 1 .. L - 1 from the row-major level 0, on the context's stream: two levels per launch (k_mip_downsample<true>) wherever the
// source level's sides are multiples of 4 and the alignments of its 16-byte loads and 8-byte stores hold, else one
int mip_generate(swr_context* c, const swr_texture* t) {
    for (int l = 0; l + 1 < t->levels;) {
        const uint32_t sw = (uint32_t)mip_level_side(t->w, l), sh = (uint32_t)mip_level_side(t->h, l);
        const uint32_t* src = mip_level_texels(t, l);
        uint32_t* const dst = mip_level_texels(t, l + 1);             // (both allocations are 256-byte aligned: a pointer's alignment is its offset's)
        const bool two = l + 2 < t->levels && (sw & 3u) == 0 && (sh & 3u) == 0 && ((uintptr_t)src & 15u) == 0 && ((uintptr_t)dst & 7u) == 0;
        if (two) {
            const auto [grid, block] = deliver_shape(sw >> 2, sh >> 2);
            hipLaunchKernelGGL(k_mip_downsample<true>, grid, block, 0, c->stream, src, sw, sh, dst, mip_level_texels(t, l + 2));
        } else {
            const auto [grid, block] = deliver_shape((uint32_t)mip_level_side(t->w, l + 1), (uint32_t)mip_level_side(t->h, l + 1));
            hipLaunchKernelGGL(k_mip_downsample<false>, grid, block, 0, c->stream, src, sw, sh, dst, (uint32_t*)nullptr);
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
        return fail_hip(c, what_failed, e);
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

int texture_format(swr_context* c, const swr_texture* t, int* format) {
    if (!t || !format) return fail(c, SWR_ERR_INVALID_ARG, "bad texture_format arguments");
    *format = t->format;
    return SWR_OK;
}

int texture_set_filter(swr_context* c, swr_texture* t, int bilinear) {
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

int texture_destroy(swr_context* c, swr_texture* t) {
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

// ---- mip chains
int texture_generate_mipmaps(swr_context* c, swr_texture* t) {
    if (!t) return fail(c, SWR_ERR_INVALID_ARG, "texture is null");
    if (int rc = texture_format_check(c, t, SWR_TEXTURE_FORMAT_RGBA8)) return rc;
    if (t->cube && (t->w & (t->w - 1)) != 0)
        return fail(c, SWR_ERR_UNSUPPORTED, "a cube map's chain needs a power-of-two side (per-face level sizes are out of scope, DESIGN.md section 27)");
    const int L = texture_full_levels(t);                    // (a cube's chain ends where a face is one texel)
    if (L == 1) return SWR_OK;                               // 1 x 1: a chain of one level, which it has
    // immediate-mode semantics without a host wait (swr_texture_update_from_frame's): the recorded draws go first and read the old
    // record -- the device reads it when a kernel runs, so the order on the stream is what "earlier" and "later" mean
    int rc = flush_locked(c); if (rc) return rc;
    if (!t->d_tail) SWR_HIP(c, hipMalloc((void**)&t->d_tail, (size_t)mip_tail_offset(t, L) * 4));
    if (t->levels != L) {
        t->levels = L;
        SWR_HIP(c, texture_header_write(c, t, t->d_rgba));
        if (t->d_blocked) SWR_HIP(c, texture_header_write(c, t, t->d_blocked));
    }
    return mip_generate(c, t);
}

int texture_levels(swr_context* c, const swr_texture* t, int* levels) {
    if (!t || !levels) return fail(c, SWR_ERR_INVALID_ARG, "bad texture_levels arguments");
    *levels = t->levels;
    return SWR_OK;
}

int texture_level_size(swr_context* c, const swr_texture* t, int level, int* w, int* h) {
    if (!t || !w || !h) return fail(c, SWR_ERR_INVALID_ARG, "bad texture_level_size arguments");
    if (level < 0 || level >= texture_full_levels(t)) return fail(c, SWR_ERR_INVALID_ARG, "the level is outside the texture's full chain (0 .. floor(log2(max(w, h))))");
    *w = mip_level_side(t->w, level); *h = mip_level_side(t->h, level);
    return SWR_OK;
}

int texture_readback_level(swr_context* c, const swr_texture* t, int level, uint8_t* rgba8) {
    if (!t || !rgba8) return fail(c, SWR_ERR_INVALID_ARG, "bad texture_readback_level arguments");
    if (int rc = texture_format_check(c, t, SWR_TEXTURE_FORMAT_RGBA8)) return rc;
    if (level < 0 || level >= t->levels) return fail(c, SWR_ERR_INVALID_ARG, "the level is outside the levels the texture has (swr_texture_levels)");
    const size_t bytes = (size_t)mip_level_side(t->w, level) * (size_t)mip_level_side(t->h, level) * 4;
    SWR_HIP(c, hipMemcpyAsync(rgba8, mip_level_texels(t, level), bytes, hipMemcpyDeviceToHost, c->stream));
    return sync_locked(c);
}

// ---- cube maps: an n x 6 n texture, face f in rows [f n, (f + 1) n)
int cube_create(swr_context* c, const void* texels, int n, swr_texture** out, int format) {
    if (n < 1 || !out) return fail(c, SWR_ERR_INVALID_ARG, "bad cube map arguments");
    if (6ull * (uint64_t)n * (uint64_t)n >= (1ull << 30)) return fail(c, SWR_ERR_INVALID_ARG, "cube maps of 2^30 texels or more are not supported (32-bit texel index)");
    const int rc = texture_create(c, texels, n, 6 * n, out, texels ? "texture upload failed: " : "texture allocation failed: ", format);
    if (rc == SWR_OK) (*out)->cube = true;
    return rc;
}

int texture_is_cube(swr_context* c, const swr_texture* t, int* n) {
    if (!t || !n) return fail(c, SWR_ERR_INVALID_ARG, "bad texture_is_cube arguments");
    *n = t->cube ? t->w : 0;
    return SWR_OK;
}

int texture_readback_face(swr_context* c, const swr_texture* t, int face, int level, void* out) {
    if (!t || !out) return fail(c, SWR_ERR_INVALID_ARG, "bad texture_readback_face arguments");
    if (!t->cube) return fail(c, SWR_ERR_INVALID_ARG, "the texture is not a cube map (swr_texture_create_cube, swr_texture_create_cube_depth)");
    if (face < 0 || face > 5) return fail(c, SWR_ERR_INVALID_ARG, "face must be 0 .. 5 (+X, -X, +Y, -Y, +Z, -Z)");
    if (level < 0 || level >= t->levels) return fail(c, SWR_ERR_INVALID_ARG, "the level is outside the levels the texture has (swr_texture_levels)");
    const size_t n = (size_t)(t->w >> level);
    const uint8_t* from = reinterpret_cast<const uint8_t*>(mip_level_texels(t, level));
    SWR_HIP(c, hipMemcpyAsync(out, from + (size_t)face * n * n * 4, n * n * 4, hipMemcpyDeviceToHost, c->stream));
    return sync_locked(c);
}

// ---- the batched probes: n records up, one kernel of one thread per record, one or two arrays of n records down, one host wait.
// A probe is its record sizes, its refusals and its launch; the steps are probe()'s.
constexpr int PROBE_NO_TEXTURE = -1;
struct ProbeSpec {
    size_t in_bytes, out_bytes[2];       // per record (out_bytes[1] == 0: one output)
    const char* bad_args;                // the refusal of a null pointer or a negative n
    int format;                          // what the texture must hold (SWR_TEXTURE_FORMAT_*), or PROBE_NO_TEXTURE: the call has none
    const char* not_cube = nullptr;      // set: the texture must be a cube map, and this refuses another
};
// The checks in the order every probe has had them (arguments, cube, format, then n == 0: SWR_OK without touching the device), the
// records through d_scratch as probe_layout (swr_query_layout.h) places them, and launch(grid, block, d_in, d_out0, d_out1) on the
// context's stream between the copies.
template <class Launch>
int probe(swr_context* c, const ProbeSpec& s, const swr_texture* t, const void* in, int n, void* out0, void* out1, Launch&& launch) {
    const bool textured = s.format != PROBE_NO_TEXTURE;
    if ((textured && !t) || !in || !out0 || (s.out_bytes[1] && !out1) || n < 0) return fail(c, SWR_ERR_INVALID_ARG, s.bad_args);
    if (s.not_cube && !t->cube) return fail(c, SWR_ERR_INVALID_ARG, s.not_cube);
    if (textured) { if (int rc = texture_format_check(c, t, s.format)) return rc; }
    if (n == 0) return SWR_OK;
    const ProbeLayout l = probe_layout(n, s.in_bytes, s.out_bytes[0], s.out_bytes[1]);
    int rc = ensure(c, c->d_scratch, l.total);
    if (rc) return rc;
    char* const base = static_cast<char*>(c->d_scratch.p);
    SWR_HIP(c, hipMemcpyAsync(base, in, (size_t)n * s.in_bytes, hipMemcpyHostToDevice, c->stream));
    launch(dim3((n + 255) / 256), dim3(256), base, base + l.off_out[0], base + l.off_out[1]);
    SWR_HIP(c, hipGetLastError());
    SWR_HIP(c, hipMemcpyAsync(out0, base + l.off_out[0], (size_t)n * s.out_bytes[0], hipMemcpyDeviceToHost, c->stream));
    if (s.out_bytes[1]) SWR_HIP(c, hipMemcpyAsync(out1, base + l.off_out[1], (size_t)n * s.out_bytes[1], hipMemcpyDeviceToHost, c->stream));
    return sync_locked(c);
}

int texture_sample(swr_context* c, const swr_texture* t, const float* uv, int n, float* out) {
    return probe(c, ProbeSpec{ 8, { 16, 0 }, "bad texture_sample arguments", SWR_TEXTURE_FORMAT_RGBA8 }, t, uv, n, out, nullptr,
                 [&](dim3 grid, dim3 block, char* in, char* out0, char*) {       // (the row-major texels whatever the filter, as always)
        hipLaunchKernelGGL(k_texture_sample, grid, block, 0, c->stream, t->d_rgba, t->w, t->h, (float2*)in, n, (float4*)out0); });
}
int texture_sample_depth(swr_context* c, const swr_texture* t, const float* uv_ref, int n, float* out) {
    return probe(c, ProbeSpec{ 12, { 8, 0 }, "bad texture_sample_depth arguments", SWR_TEXTURE_FORMAT_DEPTH32F }, t, uv_ref, n, out, nullptr,
                 [&](dim3 grid, dim3 block, char* in, char* out0, char*) {
        hipLaunchKernelGGL(k_texture_sample_depth, grid, block, 0, c->stream, texture_slot_of(t), (const float*)in, n, (float2*)out0); });
}
int texture_sample_lod(swr_context* c, const swr_texture* t, const float* uv_lod, int n, float* out_rgba) {
    return probe(c, ProbeSpec{ 12, { 16, 0 }, "bad texture_sample_lod arguments", SWR_TEXTURE_FORMAT_RGBA8 }, t, uv_lod, n, out_rgba, nullptr,
                 [&](dim3 grid, dim3 block, char* in, char* out0, char*) {
        hipLaunchKernelGGL(k_texture_sample_lod, grid, block, 0, c->stream, texture_slot_of(t), (const float*)in, n, (float4*)out0); });
}
int texture_lod(swr_context* c, const swr_texture* t, const float* grads, int n, float* out_lod) {
    return probe(c, ProbeSpec{ 16, { 4, 0 }, "bad texture_lod arguments", SWR_TEXTURE_FORMAT_RGBA8 }, t, grads, n, out_lod, nullptr,
                 [&](dim3 grid, dim3 block, char* in, char* out0, char*) {
        hipLaunchKernelGGL(k_texture_lod, grid, block, 0, c->stream, texture_slot_of(t), (const float4*)in, n, (float*)out0); });
}
// (faces and (s, t) come back as two arrays: n x (face, s, t) would interleave types)
int texture_cube_face(swr_context* c, const float* dirs, int n, int* out_face, float* out_st) {
    return probe(c, ProbeSpec{ 12, { 4, 8 }, "bad texture_cube_face arguments", PROBE_NO_TEXTURE }, nullptr, dirs, n, out_face, out_st,
                 [&](dim3 grid, dim3 block, char* in, char* out0, char* out1) {
        hipLaunchKernelGGL(k_texture_cube_face, grid, block, 0, c->stream, (const float*)in, n, (int*)out0, (float2*)out1); });
}
int texture_sample_cube(swr_context* c, const swr_texture* t, const float* dir_lod, int n, float* out_rgba) {
    return probe(c, ProbeSpec{ 16, { 16, 0 }, "bad texture_sample_cube arguments", SWR_TEXTURE_FORMAT_RGBA8, "the texture is not a cube map (swr_texture_create_cube)" },
                 t, dir_lod, n, out_rgba, nullptr, [&](dim3 grid, dim3 block, char* in, char* out0, char*) {
        hipLaunchKernelGGL(k_texture_sample_cube, grid, block, 0, c->stream, texture_slot_of(t), (const float4*)in, n, (float4*)out0); });
}
int texture_sample_cube_depth(swr_context* c, const swr_texture* t, const float* dir_ref, int n, float* out) {
    return probe(c, ProbeSpec{ 16, { 8, 0 }, "bad texture_sample_cube_depth arguments", SWR_TEXTURE_FORMAT_DEPTH32F, "the texture is not a cube map (swr_texture_create_cube_depth)" },
                 t, dir_ref, n, out, nullptr, [&](dim3 grid, dim3 block, char* in, char* out0, char*) {
        hipLaunchKernelGGL(k_texture_sample_cube_depth, grid, block, 0, c->stream, texture_slot_of(t), (const float4*)in, n, (float2*)out0); });
}
}  // namespace
