// swr_present8.hip.h -- 8-bit present: the float payload of the present calls quantised to bytes on the device.
//
// The window the floats end up in is an 8-bit framebuffer: the reference uploads them into a texture with Nearest filters
// (MainWindow.cs:82-83) and draws it with a pass-through shader (:157-169); GL then clamps to [0, 1] and rounds to 8 bits.  Doing
// that here lets 3 or 4 bytes per pixel leave the device instead of 12.
//
// THE DEFINITION (build-defined; tests/present8_cases.py restates it in numpy).  The input per output pixel is the three float32
// values the float payload delivers: under factors (1, 1) the flatten's R, G, B, otherwise k_resolve_rgb's result (resolve_rows and
// the multiply by 1 / (kx ky) of swr_resolve.hip.h, rounded to float32 before anything else).  Per channel c:
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
//   k_present8<KX, KY, BPP>  one thread per OUTPUT pixel on k_resolve_rgb's plain 2-D grid (64 x 4 threads per block, no stride
//                            loop): the thread reads exactly what k_resolve_rgb reads (a wave's KX load instructions per row
//                            together consume every line they touch) and stores three bytes (BPP 3) or one dword (BPP 4).
//                            The mapping with one thread per FOUR consecutive pixels of the band's flat pixel index (12 or 16 B
//                            stored as whole dwords, the frame's 1-3 pixel tail bytewise, a 1-D grid) sits behind
//                            SWR_PRESENT8_FOUR_PER_THREAD for the A/B of tools/resolve_rate.py.  It was built to spare every lane
//                            its partial-dword stores and is the slower one, 1.2-1.3 x at (1, 1) and 3 x at (2, 2): its lanes read
//                            64 KX bytes apart, so one load instruction touches 64 lines.  DESIGN.md section 18 has the figures.
// No LDS, no scratch, no inline assembly.  `out` must be 4-byte aligned (staging buffers are; swr_resolve_rgb8_device checks).
// A frame is at most 65535 x 65535 (swr_resize), so pixel indices fit 32 bits; byte offsets are size_t.
#pragma once
#include "swr_resolve.hip.h"

#define SWR_PRESENT8_BLOCK 256            // the four-pixel mapping: threads per block ...
#define SWR_PRESENT8_GROUP 4              // ... and output pixels per thread

namespace swr {

__device__ __forceinline__ uint32_t quantise8(float c) {
    if (!(c > 0.0f)) return 0u;           // NaN, -0, +0, negatives, -Inf
    if (c >= 1.0f) return 255u;           // +Inf too
    return (uint32_t)rintf(c * 255.0f);
}

// one output pixel of the band as bytes R | G << 8 | B << 16 | 255 << 24
template <int KX, int KY>
__device__ __forceinline__ uint32_t present8_pixel(const float4* __restrict__ color, uint32_t out_w, uint32_t ox, uint32_t oy) {
    const size_t pitch = (size_t)out_w * KX;
    const Rgb s = resolve_rows<KX, KY>(color + (size_t)oy * KY * pitch + (size_t)ox * KX, pitch);
    constexpr float scale = 1.0f / (float)(KX * KY);
    return quantise8(s.r * scale) | quantise8(s.g * scale) << 8 | quantise8(s.b * scale) << 16 | 0xff000000u;
}

#if defined(SWR_PRESENT8_FOUR_PER_THREAD)
// THE OTHER MAPPING, kept for the A/B of DESIGN.md section 18 (make EXTRA=-DSWR_PRESENT8_FOUR_PER_THREAD).  The payload is contiguous,
// so a group of four may straddle a row; each of its pixels is located on its own.
// threads the launch needs for n output pixels
constexpr uint32_t present8_threads(uint32_t n) { return n / SWR_PRESENT8_GROUP + (n % SWR_PRESENT8_GROUP ? 1u : 0u); }

// color: the band's plane, out_w * KX pixels wide and out_rows * KY rows high; out: out_rows * out_w pixels of BPP bytes
template <int KX, int KY, int BPP>
__global__ __launch_bounds__(SWR_PRESENT8_BLOCK)
void k_present8(const float4* __restrict__ color, uint8_t* __restrict__ out, uint32_t out_w, uint32_t out_rows) {
    static_assert((KX == 1 || KX == 2 || KX == 4 || KX == 8) && (KY == 1 || KY == 2 || KY == 4 || KY == 8), "factors divide the tile");
    static_assert(BPP == 3 || BPP == 4, "RGB8 or RGBX8");
    const uint32_t n = out_w * out_rows;
    const uint32_t g = blockIdx.x * SWR_PRESENT8_BLOCK + threadIdx.x;
    if (g >= present8_threads(n)) return;
    const uint32_t first = g * SWR_PRESENT8_GROUP;
    const uint32_t count = n - first < SWR_PRESENT8_GROUP ? n - first : SWR_PRESENT8_GROUP;
    uint32_t oy = first / out_w, ox = first - oy * out_w;
    uint32_t px[SWR_PRESENT8_GROUP] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < SWR_PRESENT8_GROUP; ++j) {
        if ((uint32_t)j < count) px[j] = present8_pixel<KX, KY>(color, out_w, ox, oy);
        if (++ox == out_w) { ox = 0u; ++oy; }
    }
    uint8_t* o = out + (size_t)first * BPP;
    if (count == SWR_PRESENT8_GROUP) {
        uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
        if constexpr (BPP == 3) {
            o32[0] = (px[0] & 0xffffffu) | px[1] << 24;
            o32[1] = ((px[1] >> 8) & 0xffffu) | px[2] << 16;
            o32[2] = ((px[2] >> 16) & 0xffu) | px[3] << 8;
        } else {
            o32[0] = px[0]; o32[1] = px[1]; o32[2] = px[2]; o32[3] = px[3];
        }
    } else {
        // the frame's tail, 1-3 pixels: one thread of the launch
#pragma unroll
        for (int j = 0; j < SWR_PRESENT8_GROUP - 1; ++j) {
            if ((uint32_t)j >= count) break;
#pragma unroll
            for (int k = 0; k < BPP; ++k) o[j * BPP + k] = (uint8_t)(px[j] >> (8 * k));
        }
    }
}
#else
// color: the band's plane, out_w * KX pixels wide and out_rows * KY rows high; out: out_rows * out_w pixels of BPP bytes
template <int KX, int KY, int BPP>
__global__ __launch_bounds__(SWR_RESOLVE_BLOCK_X * SWR_RESOLVE_BLOCK_Y)
void k_present8(const float4* __restrict__ color, uint8_t* __restrict__ out, uint32_t out_w, uint32_t out_rows) {
    static_assert((KX == 1 || KX == 2 || KX == 4 || KX == 8) && (KY == 1 || KY == 2 || KY == 4 || KY == 8), "factors divide the tile");
    static_assert(BPP == 3 || BPP == 4, "RGB8 or RGBX8");
    const uint32_t ox = blockIdx.x * SWR_RESOLVE_BLOCK_X + threadIdx.x;
    const uint32_t oy = blockIdx.y * SWR_RESOLVE_BLOCK_Y + threadIdx.y;
    if (ox >= out_w || oy >= out_rows) return;
    const uint32_t px = present8_pixel<KX, KY>(color, out_w, ox, oy);
    uint8_t* o = out + ((size_t)oy * out_w + ox) * BPP;
    if constexpr (BPP == 3) {
        o[0] = (uint8_t)px; o[1] = (uint8_t)(px >> 8); o[2] = (uint8_t)(px >> 16);
    } else {
        *reinterpret_cast<uint32_t*>(o) = px;
    }
}
#endif

}  // namespace swr
