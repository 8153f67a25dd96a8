// swr_rtt.hip.h -- render to texture: a frame's colour plane becomes a texture's RGBA8 texels on the device.
//
// The reference has both types -- Texture over Image<Rgba32> (Texture.cs:31-41), MainWindow's float buffers (MainWindow.cs:25-31) --
// and no link between them.  Build-defined: the link is the 8-bit present (section 18) written where the texture filters read.
//
// THE DEFINITION (tests/render_to_texture_cases.py restates it in numpy).  Texel (x, y) of a w x h texture updated from a source
// plane of w * KX x h * KY pixels:
//   R, G, B  the bytes k_present8<KX, KY, 4> delivers for output pixel (x, y): resolve_rows and the multiply by 1 / (KX KY) of
//            swr_resolve.hip.h rounded to float32 (the pixel's own floats under (1, 1)), then quantise8.
//   A        255 without ALPHA; with ALPHA the plane's .w through the same balanced pairwise tree, the same scale and quantise8
//            (NaN and <= 0 give 0, >= 1 gives 255, ties to even).
//
//   k_frame_to_texture<KX, KY, ALPHA, BLOCKED>  one thread per TEXEL on k_resolve_rgb's plain 2-D grid (64 x 4 threads per block, no
//                            stride loop; swr_present8.hip.h records why four texels per thread lost).  The thread reads what
//                            k_present8 reads -- the load is a float4 either way, ALPHA keeps the .w the present discards -- and stores
//                            ONE dword row-major into `rgba`: a wave's store instruction writes 256 contiguous bytes.  With BLOCKED the
//                            same dword goes to bilinear_texel_offset<true>(w, x, y) in `blocked` as well: a wave's 64 texels of one
//                            row are 16 runs of 16 B, one per 64-byte block line, and the four rows of a 64 x 4 block of threads
//                            together complete each of those lines, so the copy the bilinear filter reads is never stale and needs no
//                            second pass over the texture.
// The four-channel tree (resolve_rows4) has the shape of resolve_rows: channels never mix, so R, G and B are the same words.
// No LDS, no scratch, no inline assembly.  A texture has fewer than 2^30 texels (swr_texture_create), a plane at most 65535 x 65535
// pixels: texel indices fit 32 bits, plane offsets are size_t.
#pragma once
#include "swr_present8.hip.h"

namespace swr {

struct Rgba { float r, g, b, a; };

__device__ __forceinline__ Rgba rgba_add(const Rgba a, const Rgba b) { return Rgba{a.r + b.r, a.g + b.g, a.b + b.b, a.a + b.a}; }

// stage 1: N adjacent samples of one row, pairwise (resolve_row with the fourth channel kept)
template <int N>
__device__ __forceinline__ Rgba resolve_row4(const float4* __restrict__ p) {
    if constexpr (N == 1) {
        const float4 v = p[0];
        return Rgba{v.x, v.y, v.z, v.w};
    } else {
        const Rgba left = resolve_row4<N / 2>(p);
        const Rgba right = resolve_row4<N / 2>(p + N / 2);
        return rgba_add(left, right);
    }
}

// stage 2: the sums of N rows (`pitch` pixels apart), pairwise
template <int KX, int N>
__device__ __forceinline__ Rgba resolve_rows4(const float4* __restrict__ p, size_t pitch) {
    if constexpr (N == 1) {
        return resolve_row4<KX>(p);
    } else {
        const Rgba top = resolve_rows4<KX, N / 2>(p, pitch);
        const Rgba bottom = resolve_rows4<KX, N / 2>(p + (size_t)(N / 2) * pitch, pitch);
        return rgba_add(top, bottom);
    }
}

// color: the source plane, w * KX pixels wide and h * KY rows high; rgba: h x w texels row-major; blocked (BLOCKED only): the same
// texels block-linear, w and h multiples of 4
template <int KX, int KY, bool ALPHA, bool BLOCKED>
__global__ __launch_bounds__(SWR_RESOLVE_BLOCK_X * SWR_RESOLVE_BLOCK_Y)
void k_frame_to_texture(const float4* __restrict__ color, uint32_t* __restrict__ rgba, uint32_t* __restrict__ blocked, uint32_t w, uint32_t h) {
    static_assert((KX == 1 || KX == 2 || KX == 4 || KX == 8) && (KY == 1 || KY == 2 || KY == 4 || KY == 8), "factors divide the tile");
    const uint32_t x = blockIdx.x * SWR_RESOLVE_BLOCK_X + threadIdx.x;
    const uint32_t y = blockIdx.y * SWR_RESOLVE_BLOCK_Y + threadIdx.y;
    if (x >= w || y >= h) return;
    uint32_t px;
    if constexpr (ALPHA) {
        const size_t pitch = (size_t)w * KX;
        const Rgba s = resolve_rows4<KX, KY>(color + (size_t)y * KY * pitch + (size_t)x * KX, pitch);
        constexpr float scale = 1.0f / (float)(KX * KY);
        px = quantise8(s.r * scale) | quantise8(s.g * scale) << 8 | quantise8(s.b * scale) << 16 | quantise8(s.a * scale) << 24;
    } else {
        px = present8_pixel<KX, KY>(color, w, x, y);
    }
    rgba[y * w + x] = px;
    if constexpr (BLOCKED) blocked[bilinear_texel_offset<true>((int)w, (int)x, (int)y)] = px;
}

}  // namespace swr
