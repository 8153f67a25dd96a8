// swr_deliver.hip.h -- how a frame leaves the raster stage: the band's colour plane box-filtered by kx x ky on the device and stored as
// RGB floats (supersampled present), as bytes (8-bit present, section 18), as a texture's RGBA8 texels (render
// to texture, section 19) or as the RGBA plane a post program reads (section 20; k_post itself is swr_post.hip.h, over the same grid
// and the same stores).  All of it is build-defined: the reference has no supersampling (its RenderScale stops at 1,
// MainWindow.cs:93,313-315), uploads floats into a texture with Nearest filters (:82-83) that GL then clamps to [0, 1] and rounds to
// 8 bits (:157-169), and has no link between a Texture (Texture.cs:31-41) and MainWindow's float buffers (:25-31).
//
// THE RESOLVE (tests/resolve_cases.py restates it in numpy).  Every sample is a pixel of a larger reference frame; the filter adds
// nothing but this arithmetic, per output pixel and per channel R, G, B, A, in float32:
//   1. in each of the ky source rows the kx adjacent samples are summed as a balanced pairwise tree, left to right:
//      a0+a1, (a0+a1)+(a2+a3), ((a0+a1)+(a2+a3))+((a4+a5)+(a6+a7));
//   2. the ky row sums are summed by the same tree, top to bottom;
//   3. the sum is multiplied by the float 1/(kx*ky) (a power of two).
// Additions and one multiply: nothing fuses (-ffp-contract=off), denormals are kept, non-finite values follow IEEE.  Channels never
// mix, so a kernel that drops alpha (as k_flatten_rgb does) delivers the same R, G, B words as one that keeps it -- and the compiler
// drops the unused channel's loads and adds with it.  Under (1, 1) the result is the pixel's own floats.
//
// THE QUANTISER (tests/present8_cases.py restates it in numpy).  The input is a resolved channel c, rounded to float32 before anything else:
//   NaN                      -> 0
//   c <= 0 (-0, < 0, -Inf)   -> 0
//   c >= 1 (+Inf)            -> 255
//   otherwise                -> (uint8) rintf(c * 255.0f): the product rounded to float32 (nothing fuses), ties to even.
// No gamma and no dither: the reference has neither.  The GL specification prefers round-to-nearest for float -> unorm8 and leaves
// ties open, so this is a choice, not a pin.  What follows from it: quantise(float32(k) / 255) == k for all 256 k, so under the
// preferred rounding these bytes, uploaded as UnsignedByte into the reference's Rgba32f texture and drawn with Nearest, display the
// byte that was uploaded.
// Formats: BPP = 3 is R, G, B; BPP = 4 is R, G, B, 255 (alpha is dropped as in the flatten; the opaque byte makes the block RGBA8).
// Rows are tightly packed: a band's payload is out_rows * out_w * BPP contiguous bytes.
//
// RENDER TO TEXTURE (tests/render_to_texture_cases.py restates it in numpy).  Texel (x, y) of a w x h texture updated from a source
// plane of w * KX x h * KY pixels:
//   R, G, B  the bytes k_present8<KX, KY, 4> delivers for output pixel (x, y): the resolve, then the quantiser.
//   A        255 without ALPHA; with ALPHA the plane's .w through the same resolve and the same quantiser.
//
// THE KERNELS.  One thread per OUTPUT pixel on a plain 2-D grid, 64 x 4 threads per block, no stride loop (deliver_pixel).  The thread
// reads its KX adjacent samples of each of its KY rows -- 12-byte loads where alpha is dropped, 16-byte loads where it is kept; a
// wave's KX load instructions per row together read 64 * KX * 16 contiguous bytes, so every fetched line is consumed by the wave that
// fetched it -- and stores once:
//   k_resolve_rgb<KX, KY>        three floats
//   k_present8<KX, KY, BPP>      three bytes (BPP 3) or one dword (BPP 4).  `out` must be 4-byte aligned (staging buffers are;
//                                swr_resolve_rgb8_device checks)
//   k_frame_to_texture<KX, KY, ALPHA, BLOCKED>  one dword row-major into `rgba`: a wave's store instruction writes 256 contiguous
//                                bytes.  With BLOCKED the same dword goes to bilinear_texel_offset<true>(w, x, y) in `blocked` as well: a
//                                wave's 64 texels of one row are 16 runs of 16 B, one per 64-byte block line, and the four rows of a
//                                64 x 4 block of threads together complete each of those lines, so the copy the bilinear filter reads is
//                                never stale and needs no second pass over the texture
//   k_resolve_rgba<KX, KY>       one float4 into a window-sized plane of the context, for k_post.  Not launched under (1, 1), where the
//                                frame is that plane already.  The plane is deliberate: a program that fetches neighbours would
//                                otherwise redo a tree of up to 64 samples per tap.
//   k_depth_to_texture<KX, KY, BLOCKED>  the DEPTH plane's KX x KY words reduced to one by a select tree (at the end of this file, with
//                                its definition) and stored as k_frame_to_texture stores its dword: a depth texture's texel
//   k_mip_downsample<TWO>        a texture's next mip level, or its next two, from the level before (at the end of this file, with its
//                                definition): the one kernel here that reads texels instead of a frame
// Two other thread mappings were measured and removed: one lane per SOURCE pixel with in-wave adds for the resolve, and four
// consecutive pixels per thread with whole-dword stores for the 8-bit present.  DESIGN.md sections 17 and 18 have the figures.
// No LDS, no scratch, no inline assembly; nothing here is shared with the render kernels.  KX, KY in {1, 2, 4, 8} divide the
// 16-pixel tile, so a band's stored rows are a multiple of KY and a block of samples never straddles a band or a stripe.  A frame is
// at most 65535 x 65535 (swr_resize) and a texture has fewer than 2^30 texels (swr_texture_create): pixel and texel indices fit 32
// bits, plane and payload offsets are size_t.
#pragma once
#include "swr_device.h"

#define SWR_RESOLVE_BLOCK_X 64            // output pixels per block row: one wave
#define SWR_RESOLVE_BLOCK_Y 4             // output rows per block

namespace swr {

// ---- the grid: this thread's output pixel; false outside out_w x out_rows
__device__ __forceinline__ bool deliver_pixel(uint32_t out_w, uint32_t out_rows, uint32_t& ox, uint32_t& oy) {
    ox = blockIdx.x * SWR_RESOLVE_BLOCK_X + threadIdx.x;
    oy = blockIdx.y * SWR_RESOLVE_BLOCK_Y + threadIdx.y;
    return ox < out_w && oy < out_rows;
}
// its index in a row-major payload
__device__ __forceinline__ size_t deliver_index(uint32_t out_w, uint32_t ox, uint32_t oy) { return (size_t)oy * out_w + ox; }

// ---- the resolve
struct Rgba { float r, g, b, a; };

__device__ __forceinline__ Rgba rgba_add(const Rgba a, const Rgba b) { return Rgba{a.r + b.r, a.g + b.g, a.b + b.b, a.a + b.a}; }

// stage 1: N adjacent samples of one row, pairwise
template <int N>
__device__ __forceinline__ Rgba resolve_row(const float4* __restrict__ p) {
    if constexpr (N == 1) {
        const float4 v = p[0];
        return Rgba{v.x, v.y, v.z, v.w};
    } else {
        const Rgba left = resolve_row<N / 2>(p);
        const Rgba right = resolve_row<N / 2>(p + N / 2);
        return rgba_add(left, right);
    }
}

// stage 2: the sums of N rows (`pitch` pixels apart), pairwise
template <int KX, int N>
__device__ __forceinline__ Rgba resolve_rows(const float4* __restrict__ p, size_t pitch) {
    if constexpr (N == 1) {
        return resolve_row<KX>(p);
    } else {
        const Rgba top = resolve_rows<KX, N / 2>(p, pitch);
        const Rgba bottom = resolve_rows<KX, N / 2>(p + (size_t)(N / 2) * pitch, pitch);
        return rgba_add(top, bottom);
    }
}

// output pixel (ox, oy) of a plane out_w * KX pixels wide: the tree, then the scale
template <int KX, int KY>
__device__ __forceinline__ Rgba resolve_pixel(const float4* __restrict__ color, uint32_t out_w, uint32_t ox, uint32_t oy) {
    static_assert((KX == 1 || KX == 2 || KX == 4 || KX == 8) && (KY == 1 || KY == 2 || KY == 4 || KY == 8), "factors divide the tile");
    const size_t pitch = (size_t)out_w * KX;
    const Rgba s = resolve_rows<KX, KY>(color + (size_t)oy * KY * pitch + (size_t)ox * KX, pitch);
    constexpr float scale = 1.0f / (float)(KX * KY);
    return Rgba{s.r * scale, s.g * scale, s.b * scale, s.a * scale};
}

// ---- the quantiser and the stores
__device__ __forceinline__ uint32_t quantise8(float c) {
    if (!(c > 0.0f)) return 0u;           // NaN, -0, +0, negatives, -Inf
    if (c >= 1.0f) return 255u;           // +Inf too
    return (uint32_t)rintf(c * 255.0f);
}

// a pixel as bytes R | G << 8 | B << 16 | A << 24, A the quantised alpha (ALPHA) or 255
template <bool ALPHA>
__device__ __forceinline__ uint32_t pack8(float r, float g, float b, float a) {
    return quantise8(r) | quantise8(g) << 8 | quantise8(b) << 16 | (ALPHA ? quantise8(a) << 24 : 0xff000000u);
}

__device__ __forceinline__ void store_rgb32f(float* __restrict__ out, size_t pixel, float r, float g, float b) {
    float* o = out + pixel * 3;
    o[0] = r; o[1] = g; o[2] = b;
}
// (three byte stores: a pixel's bytes share a dword with its neighbours')
__device__ __forceinline__ void store_rgb8(uint8_t* __restrict__ out, size_t pixel, uint32_t px) {
    uint8_t* o = out + pixel * 3;
    o[0] = (uint8_t)px; o[1] = (uint8_t)(px >> 8); o[2] = (uint8_t)(px >> 16);
}
__device__ __forceinline__ void store_rgbx8(uint8_t* __restrict__ out, size_t pixel, uint32_t px) {
    *reinterpret_cast<uint32_t*>(out + pixel * 4) = px;
}
// texel (x, y) of a w-wide texture, row-major and (copy) where the bilinear filter reads it; w and h multiples of 4 then
__device__ __forceinline__ void store_texel(uint32_t* __restrict__ rgba, uint32_t* __restrict__ blocked, bool copy, uint32_t w, uint32_t x, uint32_t y, uint32_t px) {
    rgba[y * w + x] = px;
    if (copy) blocked[bilinear_texel_offset<true>((int)w, (int)x, (int)y)] = px;
}
__device__ __forceinline__ void store_plane(float4* __restrict__ plane, size_t pixel, const Rgba c) {
    plane[pixel] = make_float4(c.r, c.g, c.b, c.a);
}

// ---- the kernels.  color: the source plane, out_w * KX pixels wide and out_rows * KY rows high
// rgb: out_rows x out_w x 3 floats
template <int KX, int KY>
__global__ __launch_bounds__(SWR_RESOLVE_BLOCK_X * SWR_RESOLVE_BLOCK_Y)
void k_resolve_rgb(const float4* __restrict__ color, float* __restrict__ rgb, int out_w, int out_rows) {
    uint32_t ox, oy;
    if (!deliver_pixel((uint32_t)out_w, (uint32_t)out_rows, ox, oy)) return;
    const Rgba c = resolve_pixel<KX, KY>(color, (uint32_t)out_w, ox, oy);
    store_rgb32f(rgb, deliver_index((uint32_t)out_w, ox, oy), c.r, c.g, c.b);
}

// out: out_rows * out_w pixels of BPP bytes
template <int KX, int KY, int BPP>
__global__ __launch_bounds__(SWR_RESOLVE_BLOCK_X * SWR_RESOLVE_BLOCK_Y)
void k_present8(const float4* __restrict__ color, uint8_t* __restrict__ out, uint32_t out_w, uint32_t out_rows) {
    static_assert(BPP == 3 || BPP == 4, "RGB8 or RGBX8");
    uint32_t ox, oy;
    if (!deliver_pixel(out_w, out_rows, ox, oy)) return;
    const Rgba c = resolve_pixel<KX, KY>(color, out_w, ox, oy);
    const uint32_t px = pack8<false>(c.r, c.g, c.b, c.a);
    if constexpr (BPP == 3) store_rgb8(out, deliver_index(out_w, ox, oy), px);
    else store_rgbx8(out, deliver_index(out_w, ox, oy), px);
}

// rgba: h x w texels row-major; blocked (BLOCKED only): the same texels block-linear
template <int KX, int KY, bool ALPHA, bool BLOCKED>
__global__ __launch_bounds__(SWR_RESOLVE_BLOCK_X * SWR_RESOLVE_BLOCK_Y)
void k_frame_to_texture(const float4* __restrict__ color, uint32_t* __restrict__ rgba, uint32_t* __restrict__ blocked, uint32_t w, uint32_t h) {
    uint32_t x, y;
    if (!deliver_pixel(w, h, x, y)) return;
    const Rgba c = resolve_pixel<KX, KY>(color, w, x, y);
    store_texel(rgba, blocked, BLOCKED, w, x, y, pack8<ALPHA>(c.r, c.g, c.b, c.a));
}

// plane: out_rows x out_w float4
template <int KX, int KY>
__global__ __launch_bounds__(SWR_RESOLVE_BLOCK_X * SWR_RESOLVE_BLOCK_Y)
void k_resolve_rgba(const float4* __restrict__ color, float4* __restrict__ plane, uint32_t out_w, uint32_t out_rows) {
    uint32_t ox, oy;
    if (!deliver_pixel(out_w, out_rows, ox, oy)) return;
    store_plane(plane, deliver_index(out_w, ox, oy), resolve_pixel<KX, KY>(color, out_w, ox, oy));
}

// ---- depth to texture (tests/depth_texture_cases.py restates it in numpy).  Texel (x, y) of a w x h depth texture
// updated from a depth plane of w * KX by h * KY words is ONE of the block's own words, bit for bit -- no scale, no quantiser --, chosen
// by the resolve's tree shape with a select in the addition's place: a balanced pairwise tree over the KX adjacent words of each row,
// left to right, then the same tree over the KY row results, top to bottom, of
//   SWR_DEPTH_REDUCE_MAX    pick(a, b) = b > a ? b : a     the nearest sample under the default test (new >= old, Rasterizer.cs:545)
//   SWR_DEPTH_REDUCE_MIN    pick(a, b) = b < a ? b : a
//   SWR_DEPTH_REDUCE_FIRST  pick(a, b) = a                 the top-left sample, the word swr_post_depth reads
// The selects are pure: a NaN on the left stays, a NaN on the right is never taken, of +0 and -0 the left one stays -- which is why
// the tree order is part of the definition, and why these are compares and selects, never a max or min instruction.  Under (1, 1)
// all three copy the plane.
template <int REDUCE>
__device__ __forceinline__ float depth_pick(float a, float b) {
    static_assert(REDUCE == SWR_DEPTH_REDUCE_MAX || REDUCE == SWR_DEPTH_REDUCE_MIN || REDUCE == SWR_DEPTH_REDUCE_FIRST, "a reduction of include/swr.h");
    if constexpr (REDUCE == SWR_DEPTH_REDUCE_MAX) return b > a ? b : a;
    else if constexpr (REDUCE == SWR_DEPTH_REDUCE_MIN) return b < a ? b : a;
    else return a;
}
// the tree over N values in registers
template <int REDUCE, int N>
__device__ __forceinline__ float depth_tree(const float* v) {
    if constexpr (N == 1) return v[0];
    else return depth_pick<REDUCE>(depth_tree<REDUCE, N / 2>(v), depth_tree<REDUCE, N / 2>(v + N / 2));
}
// KX adjacent words of one row in one load of KX * 4 bytes (two of 16 under KX = 8): p is KX * 4-byte aligned, because the plane is
// (swr_texture_update_from_depth checks a bound one) and the row pitch w * KX and the offset x * KX are multiples of KX words
template <int KX>
__device__ __forceinline__ void depth_load_row(const float* __restrict__ p, float* v) {
    if constexpr (KX == 1) v[0] = p[0];
    else if constexpr (KX == 2) { const float2 a = *reinterpret_cast<const float2*>(p); v[0] = a.x; v[1] = a.y; }
    else {
#pragma unroll
        for (int i = 0; i < KX / 4; ++i) {
            const float4 a = reinterpret_cast<const float4*>(p)[i];
            v[4 * i] = a.x; v[4 * i + 1] = a.y; v[4 * i + 2] = a.z; v[4 * i + 3] = a.w;
        }
    }
}
// the word of the KX x KY block at p, rows `pitch` words apart (under FIRST the compiler drops every load but the first word's)
template <int REDUCE, int KX, int KY>
__device__ __forceinline__ float depth_block(const float* __restrict__ p, size_t pitch) {
    float rows[KY];
#pragma unroll
    for (int r = 0; r < KY; ++r) {
        float v[KX];
        depth_load_row<KX>(p + (size_t)r * pitch, v);
        rows[r] = depth_tree<REDUCE, KX>(v);
    }
    return depth_tree<REDUCE, KY>(rows);
}

// depth: the source plane, w * KX words wide and h * KY rows high; words: h x w texels row-major; blocked (BLOCKED only): the same
// texels block-linear.  One thread per texel on deliver_pixel's grid; a wave's loads of one row cover 64 * KX * 4 contiguous bytes and
// its store 256.  `reduce` is a run-time argument -- one scalar branch per wave in front of the loads -- and not a template parameter:
// 32 instantiations instead of 96 (k_frame_to_texture has 64 already), and the kernel's time is its loads either way.
template <int KX, int KY, bool BLOCKED>
__global__ __launch_bounds__(SWR_RESOLVE_BLOCK_X * SWR_RESOLVE_BLOCK_Y)
void k_depth_to_texture(const float* __restrict__ depth, uint32_t* __restrict__ words, uint32_t* __restrict__ blocked, uint32_t w, uint32_t h, int reduce) {
    static_assert((KX == 1 || KX == 2 || KX == 4 || KX == 8) && (KY == 1 || KY == 2 || KY == 4 || KY == 8), "factors divide the tile");
    uint32_t x, y;
    if (!deliver_pixel(w, h, x, y)) return;
    const size_t pitch = (size_t)w * KX;
    const float* __restrict__ p = depth + (size_t)y * KY * pitch + (size_t)x * KX;
    const float d = reduce == SWR_DEPTH_REDUCE_MAX ? depth_block<SWR_DEPTH_REDUCE_MAX, KX, KY>(p, pitch)
                  : reduce == SWR_DEPTH_REDUCE_MIN ? depth_block<SWR_DEPTH_REDUCE_MIN, KX, KY>(p, pitch)
                  : depth_block<SWR_DEPTH_REDUCE_FIRST, KX, KY>(p, pitch);
    store_texel(words, blocked, BLOCKED, w, x, y, __float_as_uint(d));
}

// ---- mip chains (tests/mipmap_cases.py restates the downsample in numpy).  Texel (x, y) of level l + 1,
// max(1, w_l >> 1) by max(1, h_l >> 1), is per byte channel, all four channels, in integers
//   (p(x0, y0) + p(x1, y0) + p(x0, y1) + p(x1, y1) + 2) >> 2      taps from level l, x0 = 2x, x1 = min(2x + 1, w_l - 1), y likewise:
// a box filter that rounds half up.  The clamp only bites where a side is already 1 (the tap is taken twice); an odd side >= 3 DROPS
// its last column or row: no tap reaches it.  Levels are row-major words R | G << 8 | B << 16 | A << 24.
// The four sums of a texel are taken two channels at a time: the even bytes and the odd bytes of a word each sit in 16-bit fields, where
// four bytes and the 2 add up to at most 1022 and cannot carry into the neighbour.
__device__ __forceinline__ uint32_t mip_average(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    const uint32_t m = 0x00ff00ffu, two = 0x00020002u;
    const uint32_t even = (a & m) + (b & m) + (c & m) + (d & m) + two;
    const uint32_t odd = ((a >> 8) & m) + ((b >> 8) & m) + ((c >> 8) & m) + ((d >> 8) & m) + two;
    return ((even >> 2) & m) | (((odd >> 2) & m) << 8);
}
// src: level l, sw x sh texels row-major.  One thread per deliver_pixel cell, no LDS, no scratch, no stride loop.
//   TWO = false  a cell is one texel of level l + 1 (dst1, max(1, sw >> 1) wide): four dword loads with the clamps above.  Any size.
//   TWO = true   a cell is a 4 x 4 block of level l: four 16-byte loads, one per row -- a wave's load instruction reads 1024 contiguous
//                bytes, eight whole 128-byte lines --, then the block's 2 x 2 texels of level l + 1 as two 8-byte stores (dst1, sw / 2
//                wide: 512 contiguous bytes per wave and row) and, from those four ROUNDED words, its one texel of level l + 2 (dst2,
//                sw / 4 wide): byte for byte what two TWO = false launches write, with half the launches and level l + 1 never read
//                back.  The host launches it only where sw and sh are multiples of 4 -- no clamp bites, nothing is dropped -- and src
//                is 16-byte, dst1 8-byte aligned (mip_generate, swr_api.hip).
template <bool TWO>
__global__ __launch_bounds__(SWR_RESOLVE_BLOCK_X * SWR_RESOLVE_BLOCK_Y)
void k_mip_downsample(const uint32_t* __restrict__ src, uint32_t sw, uint32_t sh, uint32_t* __restrict__ dst1, uint32_t* __restrict__ dst2) {
    uint32_t x, y;
    if constexpr (TWO) {
        const uint32_t bw = sw >> 2;
        if (!deliver_pixel(bw, sh >> 2, x, y)) return;
        uint4 r[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = *reinterpret_cast<const uint4*>(src + (size_t)(4u * y + (uint32_t)i) * sw + 4u * x);
        const uint32_t t00 = mip_average(r[0].x, r[0].y, r[1].x, r[1].y), t10 = mip_average(r[0].z, r[0].w, r[1].z, r[1].w);
        const uint32_t t01 = mip_average(r[2].x, r[2].y, r[3].x, r[3].y), t11 = mip_average(r[2].z, r[2].w, r[3].z, r[3].w);
        uint32_t* o = dst1 + (size_t)(2u * y) * (sw >> 1) + 2u * x;
        *reinterpret_cast<uint2*>(o) = make_uint2(t00, t10);
        *reinterpret_cast<uint2*>(o + (sw >> 1)) = make_uint2(t01, t11);
        dst2[(size_t)y * bw + x] = mip_average(t00, t10, t01, t11);
    } else {
        const uint32_t dw = (sw >> 1) > 1u ? (sw >> 1) : 1u, dh = (sh >> 1) > 1u ? (sh >> 1) : 1u;
        if (!deliver_pixel(dw, dh, x, y)) return;
        const uint32_t x0 = 2u * x, x1 = 2u * x + 1u < sw ? 2u * x + 1u : sw - 1u;
        const uint32_t y0 = 2u * y, y1 = 2u * y + 1u < sh ? 2u * y + 1u : sh - 1u;
        const uint32_t* __restrict__ r0 = src + (size_t)y0 * sw;
        const uint32_t* __restrict__ r1 = src + (size_t)y1 * sw;
        dst1[(size_t)y * dw + x] = mip_average(r0[x0], r0[x1], r1[x0], r1[x1]);
    }
}

#if !defined(SWR_RTC_POST) && !defined(SWR_RTC_PROGRAM)        // (the library's own small launches: no run-time unit needs them)
// the record in front of a texel array (TextureHeader, swr_device.h) and the zeros behind it: 64 words, one per thread.  The record
// travels as a kernel argument, so no host buffer has to outlive the call
__global__ __launch_bounds__(64) void k_texture_header(uint32_t* __restrict__ header_words, const TextureHeader h) {
    const uint32_t* hw = reinterpret_cast<const uint32_t*>(&h);
    const uint32_t i = threadIdx.x;
    header_words[i] = i < sizeof(TextureHeader) / 4 ? hw[i] : 0u;
}
// swr_texture_sample_lod: uv_lod: n x (u, v, lod), out: n x RGBA, through the slot as the texture is now (filter and layout included)
__global__ __launch_bounds__(256) void k_texture_sample_lod(TextureSlot t, const float* __restrict__ uv_lod, int n, float4* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = texture_slot_sample_lod(t, uv_lod[3 * i], uv_lod[3 * i + 1], uv_lod[3 * i + 2]);
}
// swr_texture_lod: grads: n x (dudx, dvdx, dudy, dvdy), out: n lods
__global__ __launch_bounds__(256) void k_texture_lod(TextureSlot t, const float4* __restrict__ grads, int n, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 g = grads[i];
    out[i] = texture_slot_lod(t, g.x, g.y, g.z, g.w);
}
// cube maps.  swr_texture_cube_face: dirs: n x (x, y, z) -> n faces and n x (s, t)
__global__ __launch_bounds__(256) void k_texture_cube_face(const float* __restrict__ dirs, int n, int* __restrict__ out_face, float2* __restrict__ out_st) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int face; float s, t;
    texture_cube_face(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], face, s, t);
    out_face[i] = face;
    out_st[i] = make_float2(s, t);
}
// swr_texture_sample_cube: dir_lod: n x (x, y, z, lod), out: n x RGBA, through the slot as the texture is now
__global__ __launch_bounds__(256) void k_texture_sample_cube(TextureSlot t, const float4* __restrict__ dir_lod, int n, float4* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 d = dir_lod[i];
    out[i] = texture_slot_sample_cube_lod(t, d.x, d.y, d.z, d.w);
}
// swr_texture_sample_cube_depth: dir_ref: n x (x, y, z, ref), out: n x (word, shadow)
__global__ __launch_bounds__(256) void k_texture_sample_cube_depth(TextureSlot t, const float4* __restrict__ dir_ref, int n, float2* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 d = dir_ref[i];
    out[i] = make_float2(texture_slot_cube_depth_sample(t, d.x, d.y, d.z), texture_slot_shadow_cube(t, d.x, d.y, d.z, d.w));
}
#endif

}  // namespace swr
