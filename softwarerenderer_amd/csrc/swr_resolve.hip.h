// swr_resolve.hip.h -- supersampled present: the band's colour plane box-filtered by kx x ky on the device.
//
// Build-defined (the reference has no supersampling: its RenderScale stops at 1, MainWindow.cs:93,313-315): a frame rendered at
// kx x ky times the window is averaged block by block and only window-sized RGB floats leave the device.  Every sample is a pixel
// of a larger reference frame; the filter adds nothing but the arithmetic below, which tests/resolve_cases.py restates in numpy:
//   per output pixel and per channel R, G, B (alpha is dropped, as in k_flatten_rgb), in float32,
//   1. in each of the ky source rows the kx adjacent samples are summed as a balanced pairwise tree, left to right:
//      a0+a1, (a0+a1)+(a2+a3), ((a0+a1)+(a2+a3))+((a4+a5)+(a6+a7));
//   2. the ky row sums are summed by the same tree, top to bottom;
//   3. the sum is multiplied by the float 1/(kx*ky) (a power of two).
// Additions and one multiply: nothing fuses (-ffp-contract=off), denormals are kept, non-finite values follow IEEE.  The tree is what
// an xor-butterfly across lanes computes as well, so a lane-per-source-pixel mapping gives the same words.
//
//   k_resolve_rgb<KX, KY>  one thread per OUTPUT pixel on a plain 2-D grid (64 x 4 threads per block, no stride loop): the thread
//                          reads its KX adjacent float4 of each of its KY rows (16-B loads; a wave reads 64 * KX * 16 contiguous
//                          bytes per row, every fetched line is consumed by the wave that fetched it) and stores 12 B.
//                          The mapping with one lane per SOURCE pixel and in-wave adds sits behind SWR_RESOLVE_LANE_PER_SOURCE for the
//                          A/B of tools/resolve_rate.py; DESIGN.md section 17 has the figures and why this one is the product's.
// No LDS, no scratch, no inline assembly; nothing here is shared with the render kernels.  KX, KY in {1, 2, 4, 8} divide the
// 16-pixel tile, so a band's stored rows are a multiple of KY and a block of samples never straddles a band or a stripe.
#pragma once
#include "swr_device.h"

#define SWR_RESOLVE_BLOCK_X 64            // output pixels per block row: one wave
#define SWR_RESOLVE_BLOCK_Y 4             // output rows per block

namespace swr {

struct Rgb { float r, g, b; };

__device__ __forceinline__ Rgb rgb_add(const Rgb a, const Rgb b) { return Rgb{a.r + b.r, a.g + b.g, a.b + b.b}; }

// stage 1: N adjacent samples of one row, pairwise
template <int N>
__device__ __forceinline__ Rgb resolve_row(const float4* __restrict__ p) {
    if constexpr (N == 1) {
        const float4 v = p[0];
        return Rgb{v.x, v.y, v.z};
    } else {
        const Rgb left = resolve_row<N / 2>(p);
        const Rgb right = resolve_row<N / 2>(p + N / 2);
        return rgb_add(left, right);
    }
}

// stage 2: the sums of N rows (`pitch` pixels apart), pairwise
template <int KX, int N>
__device__ __forceinline__ Rgb resolve_rows(const float4* __restrict__ p, size_t pitch) {
    if constexpr (N == 1) {
        return resolve_row<KX>(p);
    } else {
        const Rgb top = resolve_rows<KX, N / 2>(p, pitch);
        const Rgb bottom = resolve_rows<KX, N / 2>(p + (size_t)(N / 2) * pitch, pitch);
        return rgb_add(top, bottom);
    }
}

#if !defined(SWR_RESOLVE_LANE_PER_SOURCE)
// output pixels a block covers in x
constexpr int resolve_block_out_x(int kx) { return SWR_RESOLVE_BLOCK_X; }

// color: the band's plane, out_w * KX pixels wide and out_rows * KY rows high; rgb: out_rows x out_w x 3 floats
template <int KX, int KY>
__global__ __launch_bounds__(SWR_RESOLVE_BLOCK_X * SWR_RESOLVE_BLOCK_Y)
void k_resolve_rgb(const float4* __restrict__ color, float* __restrict__ rgb, int out_w, int out_rows) {
    static_assert((KX == 1 || KX == 2 || KX == 4 || KX == 8) && (KY == 1 || KY == 2 || KY == 4 || KY == 8), "factors divide the tile");
    const int ox = (int)blockIdx.x * SWR_RESOLVE_BLOCK_X + (int)threadIdx.x;
    const int oy = (int)blockIdx.y * SWR_RESOLVE_BLOCK_Y + (int)threadIdx.y;
    if (ox >= out_w || oy >= out_rows) return;
    const size_t pitch = (size_t)out_w * KX;
    const Rgb s = resolve_rows<KX, KY>(color + (size_t)oy * KY * pitch + (size_t)ox * KX, pitch);
    constexpr float scale = 1.0f / (float)(KX * KY);
    float* o = rgb + ((size_t)oy * (size_t)out_w + (size_t)ox) * 3;
    o[0] = s.r * scale; o[1] = s.g * scale; o[2] = s.b * scale;
}
#else
// THE OTHER MAPPING, kept for the A/B of DESIGN.md section 17 (make EXTRA=-DSWR_RESOLVE_LANE_PER_SOURCE): one lane per SOURCE column.  A
// wave reads 64 adjacent float4 of each of its KY rows (1 KiB per load instruction), stage 1 is an xor-butterfly over the KX adjacent
// lanes of a block of samples (lane i adds lane i ^ 1, then i ^ 2, then i ^ 4: IEEE addition is commutative, so every lane of the
// group holds the tree's sum), stage 2 runs in the lane, and the first lane of each group stores.  KX divides 64 and the plane's
// width, so a group is never split between waves or by the plane's edge; lanes past the edge carry zeros and store nothing.
constexpr int resolve_block_out_x(int kx) { return SWR_RESOLVE_BLOCK_X / kx; }

template <int KX>
__device__ __forceinline__ Rgb resolve_butterfly(Rgb v) {
#pragma unroll
    for (int m = 1; m < KX; m <<= 1) {
        const Rgb o = Rgb{__shfl_xor(v.r, m), __shfl_xor(v.g, m), __shfl_xor(v.b, m)};
        v = rgb_add(v, o);
    }
    return v;
}

template <int KX, int N>
__device__ __forceinline__ Rgb resolve_rows_lanes(const float4* __restrict__ p, size_t pitch, bool valid) {
    if constexpr (N == 1) {
        const float4 v = valid ? p[0] : make_float4(0.f, 0.f, 0.f, 0.f);
        return resolve_butterfly<KX>(Rgb{v.x, v.y, v.z});
    } else {
        const Rgb top = resolve_rows_lanes<KX, N / 2>(p, pitch, valid);
        const Rgb bottom = resolve_rows_lanes<KX, N / 2>(p + (size_t)(N / 2) * pitch, pitch, valid);
        return rgb_add(top, bottom);
    }
}

template <int KX, int KY>
__global__ __launch_bounds__(SWR_RESOLVE_BLOCK_X * SWR_RESOLVE_BLOCK_Y)
void k_resolve_rgb(const float4* __restrict__ color, float* __restrict__ rgb, int out_w, int out_rows) {
    static_assert((KX == 1 || KX == 2 || KX == 4 || KX == 8) && (KY == 1 || KY == 2 || KY == 4 || KY == 8), "factors divide the tile");
    const int sx = (int)blockIdx.x * SWR_RESOLVE_BLOCK_X + (int)threadIdx.x;       // source column
    const int oy = (int)blockIdx.y * SWR_RESOLVE_BLOCK_Y + (int)threadIdx.y;
    const int src_w = out_w * KX;
    const bool valid = sx < src_w && oy < out_rows;
    const size_t pitch = (size_t)src_w;
    const Rgb s = resolve_rows_lanes<KX, KY>(color + (valid ? (size_t)oy * KY * pitch + (size_t)sx : 0), pitch, valid);
    if (!valid || (sx & (KX - 1))) return;
    constexpr float scale = 1.0f / (float)(KX * KY);
    float* o = rgb + ((size_t)oy * (size_t)out_w + (size_t)(sx / KX)) * 3;
    o[0] = s.r * scale; o[1] = s.g * scale; o[2] = s.b * scale;
}
#endif

}  // namespace swr
