// swr_device.h -- device-side structs and .NET-semantics scalar helpers for the gfx950 backend.
//
// Everything here is compiled with -ffp-contract=off: the reference's C# is JIT-compiled
// without FMA contraction, and depth words must match bit for bit.
// Division and sqrt are the correctly rounded IEEE forms (hipcc default
// -fhip-fp32-correctly-rounded-divide-sqrt); f32 denormals are kept (hipcc default).
#pragma once

#ifndef __HIPCC_RTC__               // (run-time compiled user programs: swr_user_math.hip.h declares these)
#include <hip/hip_runtime.h>
#include <stdint.h>
#endif
#include "swr.h"

// System.Numerics models.  Whether .NET 9 fuses the multiply-adds of Vector4.Transform / Vector3.TransformNormal /
// Matrix4x4.Multiply and of Vector4.Lerp cannot be settled here, and nothing says the answer is the same for both families:
//   * Lerp (Shaders.Lerp in the clipper, Renderer.cs:858 in the fragment stage) sits in the hot kernels: COMPILE-TIME, SWR_NUMERICS_FMA;
//   * Transform / TransformNormal live in the vertex stage and the frustum test only: RUN-TIME flags per context
//     (swr_set_transform_fma -> DrawParams::nm_flags), whose default is SWR_NUMERICS_FMA for both, so libswr_hip_fma.so alone still
//     models "everything fused".
// With the three dot orders (SWR_DOT_PAIRWISE) that is six libraries x four flag settings: every combination the C# start-up probe
// can observe is served.
#ifndef SWR_NUMERICS_FMA
#define SWR_NUMERICS_FMA 0   // 1 models a fused MultiplyAddEstimate inside System.Numerics Lerp (and is the default of the run-time Transform flags)
#endif
#define SWR_NM_TRANSFORM_FMA        1u    // DrawParams::nm_flags: Vector4.Transform / Vector3.Transform / Matrix4x4.Multiply fuse
#define SWR_NM_TRANSFORM_NORMAL_FMA 2u    // Vector3.TransformNormal fuses
#ifndef SWR_DOT_PAIRWISE
#define SWR_DOT_PAIRWISE 0   // summation order of Vector3.Dot / LengthSquared (Renderer.cs:835,851, Rasterizer.cs:684) on the
#endif                       // (x, y, z, 0) lanes of a Vector128: 0 sequential (xx + yy) + zz; 1 dpps order (xx + yy) + (zz + 0);
                             // 2 two shuffle-adds (Vector128.Sum) (xx + zz) + (yy + 0)

// k_raster_c's program parameter for a USER fragment program (swr_program_create, include/swr.h): the instantiation exists only in
// the code objects compiled at run time (swr_program.hip.h, SWR_RTC_PROGRAM); draws carry the user id (>= SWR_PROG_USER_BASE)
#define SWR_PROG_CUSTOM 5
#define SWR_TILE 16                      // Rasterizer.cs:53 TileSize -- part of the numerical contract
#define SWR_FLOAT_MINVALUE (-3.40282347e+38f)   // float.MinValue, MainWindow.cs:425,434
#define SWR_EPSILON 1e-6f                // Rasterizer.cs:52
#define SWR_FLAG_INTERP 0x80000000u
#define SWR_FLAG_LINE   0x40000000u      // record is one DrawLine edge of DebugMode.Wireframe: sx/sy[0..1] = p0, p1
#define SWR_FLAG_FASTDIV 0x20000000u     // k_raster_c staging only: the pair's three clip.W and its draw's fog range are in div_operand_safe()'s range
#define SWR_FLAG_SIMPLE 0x10000000u      // k_raster_c staging only: every row of the pair's coverage mask is one run of pixels (k_cover's SWR_INFO_SIMPLE)
#define SWR_DRAW_MASK   0x0fffffffu
#define SWR_INFO_SIMPLE 0x80000000u      // k_cover's info.x: count | SWR_INFO_SIMPLE

#define SWR_TB_INVALID 0xffffffffffffffffull     // slot_tb word of a slot with nothing to rasterise

// Co-residency budget of the FRONT-END kernels (frames in flight, swr_api.hip).  The raster kernel of the previous flush fills every
// CU with 16 one-wave workgroups of 10,240 B of LDS each (all 160 KB) at <= 104 allocated VGPRs (k_raster_c<DUST2>: 103; 4 waves per
// SIMD: 96 of 512 registers left per SIMD lane).  A front-end workgroup is placed when one raster wave retires -- so it runs BESIDE
// the raster kernel only if it fits what that leaves: at most 10,240 B of LDS, 96 VGPRs per wave, 4 waves.  Measured
// (profiles/r04_frames_in_flight.md): k_vertex with 16 KB of LDS per block sat out the whole raster kernel (385-408 us), without LDS
// it ran beside it in 40 us; with the raster kernel at 106 registers (112 allocated: 64 left) k_bin (69 / 79) waited for its tail
// and, capped at 64, spilled (+29 us alone) -- three registers fewer in the raster kernel are what let the whole front end in.
// tests/test_resource_budget.py holds every kernel to this budget from the compiler's resource remarks (a register more in the wrong
// place costs the overlap, silently; this hipcc ignores amdgpu_num_vgpr, so the budget cannot be declared on the kernels themselves).
#define SWR_FRONT_MAX_LDS 10240
#define SWR_FRONT_MAX_VGPRS 96
#define SWR_RASTER_MAX_VGPRS 104
// ... and its waves issue ahead of the raster kernel's on the SIMDs they share (s_setprio 3, first statement of every front-end kernel):
// with frames in flight the front end of frame N+1, stretched across the raster kernel of frame N, is the critical path (cfg3: 547 us
// against 492), and on small frames it is starved outright.  Same-box A/B (tools/ab/r4_prio.sh): cfg2 0.138 -> 0.120 ms (-13 %), cfg3
// 0.563 -> 0.558, cfg5 +-0; priority 1 and 3 measure alike.  Alone on the chip the instruction changes nothing.
#define SWR_FRONT_ENTER() __builtin_amdgcn_s_setprio(3)
#define SWR_GEOM_BLOCK 128                       // threads per k_vertex / k_setup block (vertices / triangles of ONE draw per block)

namespace swr {

// ---------------------------------------------------------------- device records ----
// Vertex-stage output kept in HBM: only the varyings a built-in fragment program can read
// (Shaders.VertexOutput, Shaders.cs:26-47, minus Normal/ScreenCoords/Barycentric which no
// built-in FS consumes).  64 B = one 16-dword scalar load per vertex in the raster kernel.
struct VOut {
    float clip[4];     // ClipPosition
    float color[4];    // Color
    float uv[2];       // TexCoord
    float wn[3];       // Data["WorldNormal"]
    float wpos[3];     // Data["WorldPos"].xyz (PHONG_4POINT only)
};
static_assert(sizeof(VOut) == 64, "VOut must be 64 bytes");

// Triangle setup record: what RasterizeTriangle (Rasterizer.cs:401-460) has in locals when
// it enters the tile loop.  Vertex order is the reference's outputs[] order {v2, v1, v0}.
struct TriRec {
    float sx[3], sy[3];     // screen[0..2]
    float depth[3];         // depths[0..2]
    float inv_area;         // 1 / EdgeFunction(s0,s1,s2)
    uint32_t vref[3];       // index of outputs[0..2] in the VOut array (clip pool follows the VS outputs)
    uint32_t bbox_x;        // minX | maxX << 16   (pixel bbox, already clamped to the frame)
    uint32_t bbox_y;        // minY | maxY << 16
    uint32_t draw_flags;    // draw index | SWR_FLAG_LINE (wireframe edge) | SWR_FLAG_INTERP (outputs[0].Interpolate)
};
static_assert(sizeof(TriRec) == 64, "TriRec must be 64 bytes");

// Per-draw constants (one RenderMesh call), read with scalar loads.
struct DrawParams {
    float model[16], view[16], proj[16];
    swr_uniforms u;
    const swr_vertex* verts;
    const uint16_t* idx;
    const uint8_t* tex;
    int tex_w, tex_h;          // tex_h < 0: build-defined bilinear filter on a texture of height -tex_h (reference = nearest)
    int program, cull, depth_test, blend;
    uint32_t n_verts, n_tris;
    uint32_t vert_base;     // first VOut of this draw
    uint32_t tri_base;      // first global triangle number of this draw
    float fog_r1;           // rcp_refined(u.fog_end - u.fog_start), or 0 when that range is outside div_operand_safe():
                            // written on the device by k_vertex (the fragment program's fog division, Renderer.cs:855)
    float tex_wf, tex_hf;   // (float)tex_w, (float)|tex_h|: Texture.Sample's `u * Width` / `v * Height` operands (Texture.cs:50-51)
    float fog_den;          // u.fog_end - u.fog_start, written next to fog_r1 by k_vertex: one float subtraction per draw, not per fragment
    uint32_t frag_draw;     // index of the FIRST draw of the batch whose fragment-stage state (program, blend, depth test, texture,
                            // uniforms) equals this draw's (execute_batch): k_setup writes it into TriRec::draw_flags instead of the
                            // draw's own index, so k_raster_c -- which cuts a fragment chunk where the draw changes, because the
                            // per-draw constants are wave-uniform -- sees the 16 meshes of one model with one material as ONE draw
    uint32_t nm_flags;      // SWR_NM_*: the context's System.Numerics model of Transform / TransformNormal when the draw was recorded
};
static_assert(offsetof(DrawParams, fog_den) == offsetof(DrawParams, fog_r1) + 12, "k_vertex writes fog_den three floats after fog_r1");

struct Counters {           // device-side swr_stats accumulators
    unsigned long long triangles_in, triangles_setup, triangles_clipped;
    unsigned long long fragments_tested, fragments_shaded, fragments_written;
    unsigned long long tile_pairs;
    unsigned int overflow;  // set when a tile list did not fit
    unsigned int pad;
};

// Optimistic execution control block (one per context, in HBM).  A flush is launched without reading the pair
// total back: k_scan_apply compares it with the list capacity and, if it does not fit, sets `poison`; every
// kernel of that batch and of every later one that would touch the pair lists or the framebuffer returns at once
// (batch_poisoned), so the framebuffer stays exactly as it was before the first batch that did not fit.  The host looks
// at this block at its next synchronisation point, grows the buffers and replays from `first_bad`.
struct Ctrl {
    uint32_t poison;
    uint32_t first_bad;              // sequence number of the first batch that did not fit (atomicMin)
    unsigned long long need;         // largest pair total seen by a batch that did not fit (atomicMax)
    uint32_t* host_flag;             // pinned host word, set to 1 together with `poison`: the host polls it without a copy
};
// Must batch `seq` leave the pair lists and the framebuffer alone?  Yes when it, or a batch before it, did not fit.  Decided by
// `first_bad`, not by the sticky `poison` word: with frames pipelined (swr_api.hip: the front end of flush N+1 runs beside the
// raster kernel of flush N) a LATER batch may poison itself while this one's raster kernel is half way through its tiles, and
// that must not stop the tiles that have not started yet -- the host replays from `first_bad` only.
__device__ __forceinline__ bool batch_poisoned(const Ctrl* __restrict__ c, uint32_t seq) { return c->first_bad <= seq; }
// Batch `seq` does not fit its pair lists (`need`: a capacity that would hold it): it and every later batch are poisoned, and the host's
// polled word goes up with the device's
__device__ __forceinline__ void poison_batch(Ctrl* __restrict__ c, uint32_t seq, unsigned long long need) {
    atomicMin(&c->first_bad, seq);
    atomicMax(&c->need, need);
    __hip_atomic_store(&c->poison, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (c->host_flag) __hip_atomic_store(c->host_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

struct FrameParams {
    int width, height;          // full frame
    int tiles_x, tiles_y;       // full frame, in 16x16 tiles
    int band_ty0, band_ty1;     // this context renders tile rows [band_ty0, band_ty1) ...
    int band_y0;                // = band_ty0 * 16: first pixel row stored in the buffers (contiguous band)
    int band_rows;              // pixel rows stored
    int il_k, il_world, il_rank;   // ... or, when il_k > 0, the stripes of il_k tile rows whose stripe number s has s % il_world == il_rank
    int band_tile_rows;         // tile rows stored (either form); the buffers hold them in ascending order, 16 pixel rows each
    float near_clip;
};

// Tile-row ownership of a context (multi-GPU): a contiguous band, or interleaved stripes (load balance for clustered
// scenes).  local row = position of the tile row in this context's buffers, -1 = not ours.
struct BandMap { int ty0, ty1, il_k, il_world, il_rank; };
__host__ __device__ __forceinline__ int band_local_row(const BandMap& b, int ty) {
    if (b.il_k <= 0) return (ty >= b.ty0 && ty < b.ty1) ? ty - b.ty0 : -1;
    const int stripe = ty / b.il_k;
    if (stripe % b.il_world != b.il_rank) return -1;
    return (stripe / b.il_world) * b.il_k + (ty - stripe * b.il_k);
}
__host__ __device__ __forceinline__ int band_global_row(const BandMap& b, int local) {
    if (b.il_k <= 0) return b.ty0 + local;
    const int ls = local / b.il_k;
    return (ls * b.il_world + b.il_rank) * b.il_k + (local - ls * b.il_k);
}
__host__ __device__ __forceinline__ BandMap band_map(const FrameParams& fp) {
    BandMap b; b.ty0 = fp.band_ty0; b.ty1 = fp.band_ty1; b.il_k = fp.il_k; b.il_world = fp.il_world; b.il_rank = fp.il_rank;
    return b;
}

// ---------------------------------------------------------------- slots, records and the binning decisions ----
// A batch numbers its primitives by SLOT in submission order (k_setup): `spt` slots per submitted triangle -- filled mode 2 (slot 2t =
// the triangle, or the first fan triangle of its near-clipped polygon; slot 2t+1 = the second fan triangle, which exists only where the
// near plane cuts a triangle into a quad), wireframe 6 (three DrawLine edges per fan triangle).  slot_tb[] (tile bbox word) and want[]
// (below) are indexed by slot, and the slot is the key by which k_sort_tiles restores submission order.
//
// WHERE THE RECORD OF A SLOT IS: the single definition.  Filled batches store the records densely -- odd slots are almost always
// empty, and records indexed by slot would sit 128 B apart with a dead 64 B between them --: even slots at s >> 1, odd slots in a
// second region at odd_base + (s >> 1), odd_base = the batch's triangle count rounded up to a whole 128 B line (record_odd_base).
// odd_base == 0 is the identity (wireframe batches).  Batch-uniform: an argument of k_setup, k_bin and k_cover; the raster kernel never
// sees slots -- k_cover hands it the record index in refs[].x.
__host__ __device__ __forceinline__ uint32_t rec_index(uint32_t slot, uint32_t odd_base) {
    if (odd_base == 0u) return slot;
    return (slot & 1u) ? odd_base + (slot >> 1) : (slot >> 1);
}
__host__ __device__ __forceinline__ uint32_t record_odd_base(uint64_t triangles) { return (uint32_t)((triangles + 1u) & ~(uint64_t)1u); }

// Can triangle (sx, sy, pixel bbox) cover ANY pixel of tile (tx, ty)?  Conservative: returns false only when
// provably no pixel of bbox /\ tile can pass the reference's coverage test (all three incrementally stepped
// float32 edge values >= 0, or all three <= 0; Rasterizer.cs:481-494).  The reference visits such tiles and
// finds nothing, so dropping the pair changes no pixel and no counter.
//
// Proof sketch.  Let R be the pixel rectangle bbox /\ tile and, for edge k with float coefficients (a, b) and
// reference vertex (rx, ry), E(x,y) = a*(x-rx) + b*(y-ry) in real arithmetic; u = 2^-24.  Every value the
// reference's float chain takes is fl-arithmetic on points of R: the start value costs <= 5 roundings of
// quantities bounded by M = |a|*max|x-rx| + |b|*max|y-ry| over R, and each of the <= 30 chain adds rounds a value
// of magnitude <= M(1+tiny); so |W - E| <= 35uM(1+tiny) at every pixel of R.  E is linear, so its extrema over R
// are at corners; evaluating them in float32 as below costs <= 3 roundings per term, |Efl - E| <= 6uM, and the
// float M' satisfies M' >= M(1-4u).  With delta = 64uM':
//   Efl_max < -delta  =>  W <= E_max + 35uM <= Efl_max + 41uM < -64uM(1-4u) + 41uM < 0 on all of R  (kills "all >= 0")
//   Efl_min >  delta  =>  W > 0 on all of R                                                          (kills "all <= 0")
// The analysis needs every product and sum finite: screen coordinates below 1e15 in magnitude (tested once per triangle, not
// per tile and edge as in round 2) bound every term by 1e31; anything else (NaN / Inf included) means "keep".
__device__ __forceinline__ bool pair_may_cover(const float sx[3], const float sy[3], int minX, int maxX, int minY, int maxY,
                                               int tx, int ty, int width, int height, bool is_line) {
    if (is_line) return true;         // DrawLine edges: keep every tile of the line's bbox (the test below is for triangles)
    const int x0 = tx * SWR_TILE, y0 = ty * SWR_TILE;
    const int startX = max(minX, x0), endX = min(maxX, min(x0 + SWR_TILE - 1, width - 1));
    const int startY = max(minY, y0), endY = min(maxY, min(y0 + SWR_TILE - 1, height - 1));
    if (startX > endX || startY > endY) return false;                 // Rasterizer.cs:476: nothing visited
    // edge k: coefficients exactly as RasterizeTriangle forms them (Rasterizer.cs:445-447), reference vertex :481-483
    const float ea[3] = { sy[1] - sy[2], sy[2] - sy[0], sy[0] - sy[1] };   // a12, a20, a01
    const float eb[3] = { sx[2] - sx[1], sx[0] - sx[2], sx[1] - sx[0] };   // b12, b20, b01
    const float rx[3] = { sx[1], sx[2], sx[0] };
    const float ry[3] = { sy[1], sy[2], sy[0] };
    const float fxs = (float)startX, fxe = (float)endX, fys = (float)startY, fye = (float)endY;
    const float lim = 1.0e15f;
    const bool tame = fabsf(sx[0]) < lim && fabsf(sx[1]) < lim && fabsf(sx[2]) < lim && fabsf(sy[0]) < lim && fabsf(sy[1]) < lim && fabsf(sy[2]) < lim;
    if (!tame) return true;
    bool any_neg = false, any_pos = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float a = ea[k], b = eb[k];
        const float dxs = fxs - rx[k], dxe = fxe - rx[k], dys = fys - ry[k], dye = fye - ry[k];
        const float ax_s = a * dxs, ax_e = a * dxe, by_s = b * dys, by_e = b * dye;
        const float emax = fmaxf(ax_s, ax_e) + fmaxf(by_s, by_e);
        const float emin = fminf(ax_s, ax_e) + fminf(by_s, by_e);
        const float m = fabsf(a) * fmaxf(fabsf(dxs), fabsf(dxe)) + fabsf(b) * fmaxf(fabsf(dys), fabsf(dye));
        const float delta = m * (64.0f / 16777216.0f);
        any_neg = any_neg || emax < -delta;
        any_pos = any_pos || emin > delta;
    }
    return !(any_neg && any_pos);
}

// The tile bbox word of a slot (k_setup: tminx | tmaxx << 16 | tminy << 32 | tmaxy << 48), clamped to the tile rows the context bins:
// [band.ty0, band.ty1) -- the contiguous band, or the whole frame under interleaved stripes, where band_local_row decides row by row.
// false (and nx = ny = 0) when the slot has nothing there.  One definition for k_setup, which writes want[], and k_bin, which reads it.
struct SlotTiles { int tminx, tminy, nx, ny; };
__device__ __forceinline__ bool slot_tiles(const BandMap& band, unsigned long long tb, SlotTiles& s) {
    s.tminx = s.tminy = s.nx = s.ny = 0;
    if (tb == SWR_TB_INVALID) return false;
    s.tminx = (int)(tb & 0xffff);
    const int tmaxx = (int)((tb >> 16) & 0xffff);
    s.tminy = max((int)((tb >> 32) & 0xffff), band.ty0);
    const int tmaxy = min((int)((tb >> 48) & 0xffff), band.ty1 - 1);
    s.nx = tmaxx - s.tminx + 1;
    s.ny = tmaxy - s.tminy + 1;
    if (s.ny <= 0) { s.nx = 0; s.ny = 0; return false; }
    return true;
}
// A slot of at most SWR_SMALL_TILES clamped tiles is SMALL (nearly all are): bit i of its byte want[slot] says whether its i-th tile,
// in the row-major order of SmallTileWalk, is binned -- the row is this context's and pair_may_cover holds.  k_setup decides that where
// it has the triangle in registers (small_want_mask); both k_bin passes replay the byte and read no record of a small slot.  Writer
// and readers walk the tiles with the same SmallTileWalk over the same slot_tiles() clamp: a disagreement would drop or duplicate a pair.
#define SWR_SMALL_TILES 8
struct SmallTileWalk {              // row-major over the clamped tile bbox, without integer division
    int tx, ty, x_lo, x_end;
    __device__ __forceinline__ explicit SmallTileWalk(const SlotTiles& s) : tx(s.tminx), ty(s.tminy), x_lo(s.tminx), x_end(s.tminx + s.nx) {}
    __device__ __forceinline__ void next() { ++tx; if (tx >= x_end) { tx = x_lo; ++ty; } }
};
__device__ __forceinline__ uint32_t small_want_mask(const BandMap& band, unsigned long long tb, const float sx[3], const float sy[3],
                                                    int minX, int maxX, int minY, int maxY, int width, int height, bool is_line) {
    SlotTiles st;
    if (!slot_tiles(band, tb, st)) return 0u;
    const int nt = st.nx * st.ny;
    if (nt > SWR_SMALL_TILES) return 0u;                    // big: k_bin spreads it over a wave and tests there (bin_big)
    uint32_t mask = 0u;
    SmallTileWalk w(st);
    // two tiles per trip: their tests are independent chains, and in a small batch (one wave per SIMD) k_setup's time is the length
    // of that chain (cfg2: -0.7 us against one tile per trip; four and eight measured no better, profiles/r07_front_end_records.md)
#pragma unroll 1
    for (int i0 = 0; i0 < nt; i0 += 2) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = i0 + j;
            const bool want = i < nt && band_local_row(band, w.ty) >= 0 && pair_may_cover(sx, sy, minX, maxX, minY, maxY, w.tx, w.ty, width, height, is_line);
            mask |= want ? (1u << i) : 0u;
            w.next();
        }
    }
    return mask;
}

// ---------------------------------------------------------------- .NET scalar semantics ----
__device__ __forceinline__ bool is_neg_bits(float f) { return (__float_as_uint(f) >> 31) != 0u; }
__device__ __forceinline__ bool is_nan(float f) { return f != f; }
__device__ __forceinline__ bool is_nan_or_inf(float f) { return (__float_as_uint(f) & 0x7f800000u) == 0x7f800000u; }

// (int)float, .NET 9 x64: truncating, saturating, NaN -> 0.  That is exactly v_cvt_i32_f32 on gfx9 (round toward
// zero, out-of-range and infinities saturate, NaN -> 0); C++ `(int)f` is undefined out of range, so name the instruction.
__device__ __forceinline__ int f2i(float f) {
    int r;
    asm("v_cvt_i32_f32 %0, %1" : "=v"(r) : "v"(f));
    return r;
}
// MathF.Min / MathF.Max: NaN-propagating, -0 < +0
__device__ __forceinline__ float mathf_min(float a, float b) {
    if (a != b) { if (!is_nan(a)) return a < b ? a : b; return a; }
    return is_neg_bits(a) ? a : b;
}
__device__ __forceinline__ float mathf_max(float a, float b) {
    if (a != b) { if (!is_nan(a)) return b < a ? a : b; return a; }
    return is_neg_bits(b) ? a : b;
}
__device__ __forceinline__ float math_clamp(float v, float lo, float hi) {   // Math.Clamp
    if (v < lo) return lo;
    else if (v > hi) return hi;
    return v;
}

// ---------------------------------------------------------------- exact division / sqrt without the scaling steps ----
// hipcc expands a correctly rounded f32 division n / d (the flag above) to
//     d' = v_div_scale(d)   n' = v_div_scale(n)          (a power-of-two rescue for extreme exponents; vcc = "rescaled")
//     r0 = v_rcp_f32(d')    e = fma(-d', r0, 1)    r1 = fma(e, r0, r0)
//     q0 = n' * r1          e2 = fma(-d', q0, n')  q1 = fma(e2, r1, q0)    e3 = fma(-d', q1, n')
//     q  = v_div_fmas(e3, r1, q1)   (= fma, times 2^+-64 if vcc)           result = v_div_fixup(q, d, n)   (NaN / Inf / 0 / denormal cases)
// When |n| and |d| lie in [2^-40, 2^40] none of v_div_scale's rescue conditions holds (they need an exponent
// difference >= 96, a denormal operand or quotient, or |n| < 2^-103), so d' = d, n' = n, vcc = 0, v_div_fmas is a
// plain fma and v_div_fixup returns q: the division IS the eight-instruction core below.  r1 depends on d only, so a
// denominator shared by many fragments (a vertex's clip.W, a draw's fog range) pays rcp_refined ONCE and each quotient
// costs 1 mul + 4 fma instead of 11 instructions -- bit for bit the same quotient, because it is the same instruction
// sequence on the same operands (fma used inside a correctly rounded division is not a contraction of reference
// arithmetic).  swr_selftest_division compares it with the compiler's `/` over random, near-midpoint and boundary
// operands on the GPU (tests/test_gpu_api.py::test_exact_division_core_matches_ieee_division).
__device__ __forceinline__ float rcp_refined(float d) {
    const float r0 = __builtin_amdgcn_rcpf(d);
    const float e = __builtin_fmaf(-d, r0, 1.0f);
    return __builtin_fmaf(e, r0, r0);
}
__device__ __forceinline__ float div_core(float n, float d, float r1) {
    const float q0 = n * r1;
    const float e2 = __builtin_fmaf(-d, q0, n);
    const float q1 = __builtin_fmaf(e2, r1, q0);
    const float e3 = __builtin_fmaf(-d, q1, n);
    return __builtin_fmaf(e3, r1, q1);
}
// |v| in [2^-40, 2^40], by its bit pattern (NaN, Inf, zero and denormals are all outside)
#define SWR_DIV_LO_BITS 0x2B800000u      // 2^-40
#define SWR_DIV_HI_BITS 0x53800000u      // 2^40
__device__ __forceinline__ bool div_operand_safe(float v) {
    return __builtin_fabsf(v) >= 0x1p-40f && __builtin_fabsf(v) <= 0x1p40f;       // two compares with the |.| source modifier; NaN fails both
}
__device__ __forceinline__ bool div_operands_safe3(float a, float b, float c) {
    const uint32_t ua = __float_as_uint(a) & 0x7fffffffu, ub = __float_as_uint(b) & 0x7fffffffu, uc = __float_as_uint(c) & 0x7fffffffu;
    return min(min(ua, ub), uc) >= SWR_DIV_LO_BITS && max(max(ua, ub), uc) <= SWR_DIV_HI_BITS;
}
// The same guard for three values that are results of float arithmetic (canonical, so min/add need no quieting):
// 5 instructions instead of 7.  The sum of the magnitudes is >= each of them and carries NaN / Inf (a NaN is dropped by
// v_min3 but not by the sum), so `sum <= 2^40` bounds all three from above -- slightly conservative, which a guard may be.
__device__ __forceinline__ bool div_operands_safe3_arith(float a, float b, float c) {
    const float fa = __builtin_fabsf(a), fb = __builtin_fabsf(b), fc = __builtin_fabsf(c);
    const float sum = (fa + fb) + fc;
    const float lo = __builtin_fminf(__builtin_fminf(fa, fb), fc);
    return lo >= 0x1p-40f && sum <= 0x1p40f;
}
// 1 / d: the division core with n = 1 (q0 = 1 * r1 is r1 itself): 7 instructions instead of 11.  With n = 1 the range is
// wider on the large side: |d| in [2^-40, 2^83] (v_div_scale rescues only |d| >= 2^126, |d| <= 2^-96 and denormals).
// swr_selftest_division checks EVERY float of that range, both signs, against the compiler's 1.0f / d.
#define SWR_RCP_HI_BITS 0x69000000u      // 2^83
__device__ __forceinline__ float recip_core(float d) {
    const float r1 = rcp_refined(d);
    const float e2 = __builtin_fmaf(-d, r1, 1.0f);
    const float q1 = __builtin_fmaf(e2, r1, r1);
    const float e3 = __builtin_fmaf(-d, q1, 1.0f);
    return __builtin_fmaf(e3, r1, q1);
}
// hipcc's correctly rounded sqrtf is: scale x by 2^32 if x < 2^-96; s = v_sqrt_f32(x); step s down one ulp if
// fma(-(s-1ulp), s, x) <= 0, up one ulp if fma(-(s+1ulp), s, x) > 0; unscale; return x itself for +-0 / +inf.
// For x in [2^-40, 2^40] the scaling and the class test are no-ops: the five-instruction core below is the same sqrt.
__device__ __forceinline__ float sqrt_core(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const float sd = __uint_as_float(__float_as_uint(s) - 1u), su = __uint_as_float(__float_as_uint(s) + 1u);
    const float rd = __builtin_fmaf(-sd, s, x), ru = __builtin_fmaf(-su, s, x);
    float r = rd <= 0.0f ? sd : s;
    r = ru > 0.0f ? su : r;
    return r;
}

// ---------------------------------------------------------------- System.Numerics ----
template <bool FUSED>
__device__ __forceinline__ float nm_madd(float a, float b, float c) {
    if (FUSED) return __builtin_fmaf(a, b, c);
    float p = a * b;
    return p + c;
}
// Vector4.Transform(v, M): ((x*row1 + y*row2) + z*row3) + w*row4 ; M row-major M11..M44
template <bool FUSED>
__device__ __forceinline__ void vec4_transform_t(const float v[4], const float* __restrict__ m, float out[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float r = m[j] * v[0];
        r = nm_madd<FUSED>(m[4 + j], v[1], r);
        r = nm_madd<FUSED>(m[8 + j], v[2], r);
        r = nm_madd<FUSED>(m[12 + j], v[3], r);
        out[j] = r;
    }
}
template <bool FUSED>
__device__ __forceinline__ void vec3_transform_normal_t(const float n[3], const float* __restrict__ m, float out[3]) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float r = m[j] * n[0];
        r = nm_madd<FUSED>(m[4 + j], n[1], r);
        r = nm_madd<FUSED>(m[8 + j], n[2], r);
        out[j] = r;
    }
}
// `fused` is uniform over a draw (DrawParams::nm_flags): one scalar branch per call site
__device__ __forceinline__ void vec4_transform(const float v[4], const float* __restrict__ m, float out[4], bool fused) {
    if (fused) vec4_transform_t<true>(v, m, out); else vec4_transform_t<false>(v, m, out);
}
__device__ __forceinline__ void vec3_transform_normal(const float n[3], const float* __restrict__ m, float out[3], bool fused) {
    if (fused) vec3_transform_normal_t<true>(n, m, out); else vec3_transform_normal_t<false>(n, m, out);
}
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
#if SWR_DOT_PAIRWISE == 1
    const float p = ax * bx + ay * by, q = az * bz + 0.0f;
    return p + q;
#elif SWR_DOT_PAIRWISE == 2
    const float p = ax * bx + az * bz, q = ay * by + 0.0f;
    return p + q;
#else
    return (ax * bx + ay * by) + az * bz;
#endif
}
// Vector3.Cross(a, b) (Physics.cs:153,170): FUSED = false, two rounded products per component, (a.y*b.z) - (a.z*b.y); FUSED = true,
// fma(-a.z, b.y, round(a.y*b.z)) -- one more unpinned System.Numerics switch, chosen per call by
// SWR_RAY_CROSS_FUSED (include/swr.h).  The fma is spelled out: it is the model, not a contraction.
template <bool FUSED>
__device__ __forceinline__ void cross3(const float a[3], const float b[3], float out[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = (k + 1) % 3, j = (k + 2) % 3;           // x: (y, z)   y: (z, x)   z: (x, y)
        const float p = a[i] * b[j];
        if (FUSED) out[k] = __builtin_fmaf(-a[j], b[i], p);
        else { const float q = a[j] * b[i]; out[k] = p - q; }
    }
}
__device__ __forceinline__ float nm_lerp(float a, float b, float t) {   // a*(1-t) + b*t
#if SWR_NUMERICS_FMA
    return __builtin_fmaf(a, 1.0f - t, b * t);
#else
    float x = a * (1.0f - t);
    float y = b * t;
    return x + y;
#endif
}

// EdgeFunction, Rasterizer.cs:562-563
__device__ __forceinline__ float edge_function(float ax, float ay, float bx, float by, float cx, float cy) {
    float p = (cx - ax) * (by - ay);
    float q = (cy - ay) * (bx - ax);
    return p - q;
}

// GetDepthTestFunction, Rasterizer.cs:543-559
__device__ __forceinline__ bool depth_func(int test, float nd, float od) {
    switch (test) {
    case SWR_DEPTH_LESSEQUAL:    return nd >= od;
    case SWR_DEPTH_LESS:         return nd > od;
    case SWR_DEPTH_GREATER:      return nd < od;
    case SWR_DEPTH_GREATEREQUAL: return nd <= od;
    case SWR_DEPTH_EQUAL:        return fabsf(nd - od) < SWR_EPSILON;
    case SWR_DEPTH_NOTEQUAL:     return fabsf(nd - od) >= SWR_EPSILON;
    default:                     return true;    // Disabled, Always, anything else
    }
}

// Blend, Rasterizer.cs:58-65
__device__ __forceinline__ float4 blend(float4 s, float4 d, int mode) {
    float4 o;
    switch (mode) {
    case SWR_BLEND_ALPHA: {
        float a = s.w, ia = 1.0f - s.w;
        float x;
        x = s.x * a; o.x = x + d.x * ia;
        x = s.y * a; o.y = x + d.y * ia;
        x = s.z * a; o.z = x + d.z * ia;
        x = s.w * a; o.w = x + d.w * ia;
        return o; }
    case SWR_BLEND_ADDITIVE:
        o.x = mathf_min(s.x + d.x, 1.0f); o.y = mathf_min(s.y + d.y, 1.0f);
        o.z = mathf_min(s.z + d.z, 1.0f); o.w = mathf_min(s.w + d.w, 1.0f);
        return o;
    case SWR_BLEND_MULTIPLY:
        o.x = s.x * d.x; o.y = s.y * d.y; o.z = s.z * d.z; o.w = s.w * d.w;
        return o;
    default:
        return s;
    }
}

// DrawLine's per-pixel test, Rasterizer.cs:296-313: parameter t of the closest point of segment p0->p1 to the
// pixel centre (x+0.5, y+0.5) and whether the centre lies within 0.5 px of the segment
__device__ __forceinline__ bool line_test(float p0x, float p0y, float p1x, float p1y, int x, int y, float& t_out) {
    const float dx = p1x - p0x, dy = p1y - p0y;                       // :257-258
    const float len_sq = dx * dx + dy * dy;                          // :259
    const float px = (float)x + 0.5f - p0x, py = (float)y + 0.5f - p0y;   // :296-297
    float t = 0.0f;
    if (len_sq > 0) t = (px * dx + py * dy) / len_sq;                // :300-301
    t = mathf_max(0.0f, mathf_min(1.0f, t));                         // :303
    const float cx = p0x + t * dx, cy = p0y + t * dy;                // :305-306
    const float ddx = ((float)x + 0.5f) - cx, ddy = ((float)y + 0.5f) - cy;
    const float dist_sq = ddx * ddx + ddy * ddy;                     // :310
    t_out = t;
    return dist_sq <= 0.5f * 0.5f;                                   // :312-313
}

// Texture.Sample, Texture.cs:43-63 -- nearest, wrap; texels RGBA8 row-major
// Texture.Sample in two halves, so that a caller can put independent work between the texel load and its use
// (k_raster_c: the fetch is a dependent gather with a long latency)
__device__ __forceinline__ float4 texture_unpack(uint32_t p) {              // Texture.cs:55-62: byte * (1f / 255f)
    const float inv255 = 1.0f / 255.0f;
    float4 o;
    o.x = (float)(p & 0xffu) * inv255;
    o.y = (float)((p >> 8) & 0xffu) * inv255;
    o.z = (float)((p >> 16) & 0xffu) * inv255;
    o.w = (float)(p >> 24) * inv255;
    return o;
}
// wf, hf = (float)Width, (float)Height as C# converts them in `u * Width` (exact for sizes below 2^24; passed in so that the raster
// kernel gets them from the draw's constants instead of converting per fragment).  32-bit texel index: swr_texture_create refuses
// textures of 2^30 texels or more, so index * 4 fits the unsigned 32-bit offset of a global load with a scalar base.
__device__ __forceinline__ uint32_t texture_nearest_index(int w, int h, float wf, float hf, float tu, float tv) {      // Texture.cs:43-54
    float u = tu - (float)f2i(tu);
    float v = tv - (float)f2i(tv);
    u += (u < 0) ? 1.0f : 0.0f;
    v += (v < 0) ? 1.0f : 0.0f;
    int x = f2i(u * wf);
    int y = f2i(v * hf);
    // C# '%' truncates toward zero, then `if (x < 0) x += Width`; the common case 0 <= x < w needs neither
    if ((uint32_t)x >= (uint32_t)w) { x = (x == w) ? 0 : x % w; if (x < 0) x += w; }
    if ((uint32_t)y >= (uint32_t)h) { y = (y == h) ? 0 : y % h; if (y < 0) y += h; }
    return (uint32_t)y * (uint32_t)w + (uint32_t)x;
}
__device__ __forceinline__ uint32_t texture_nearest_index(int w, int h, float tu, float tv) {
    return texture_nearest_index(w, h, (float)w, (float)h, tu, tv);
}
__device__ __forceinline__ float4 texture_sample(const uint8_t* __restrict__ tex, int w, int h, float tu, float tv) {
    return texture_unpack(reinterpret_cast<const uint32_t*>(tex)[texture_nearest_index(w, h, tu, tv)]);
}

// BUILD-DEFINED bilinear filter with wrap (row N4; no reference semantics -- the formula is stated in
// oracle/swr_oracle.c:oswr_texture_sample_bilinear and reproduced operation for operation)
// BLOCKED: the texels are stored block-linear -- 4 x 4-texel blocks of 64 B, blocks row-major (swr_texture_set_filter makes that copy
// for textures whose sides are multiples of 4; k_block_texture) -- so the 2 x 2 taps of a fragment share ONE 64-byte line 9 times out
// of 16 instead of never (row-major: two rows, one line each, W * 4 bytes apart).  The result is layout-independent by construction:
// only the address of texel (x, y) changes.
template <bool BLOCKED>
__device__ __forceinline__ uint32_t bilinear_texel_offset(int w, int x, int y) {
    if (BLOCKED) return ((((uint32_t)y >> 2) * ((uint32_t)w >> 2) + ((uint32_t)x >> 2)) << 4) + (((uint32_t)y & 3u) << 2) + ((uint32_t)x & 3u);
    return (uint32_t)y * (uint32_t)w + (uint32_t)x;
}
template <bool BLOCKED>
__device__ __forceinline__ float4 texture_sample_bilinear(const uint8_t* __restrict__ tex, int w, int h, float tu, float tv) {
    const float x = tu * (float)w - 0.5f, y = tv * (float)h - 0.5f;
    const float x0 = floorf(x), y0 = floorf(y);
    const float fx = x - x0, fy = y - y0;
    int ix0 = f2i(x0) % w; if (ix0 < 0) ix0 += w;
    int iy0 = f2i(y0) % h; if (iy0 < 0) iy0 += h;
    const int ix1 = ix0 + 1 == w ? 0 : ix0 + 1, iy1 = iy0 + 1 == h ? 0 : iy0 + 1;
    // (texel index < 2^30: swr_texture_create refuses larger textures)
    const uint32_t* __restrict__ t32 = reinterpret_cast<const uint32_t*>(tex);
    const uint32_t p00 = t32[bilinear_texel_offset<BLOCKED>(w, ix0, iy0)];
    const uint32_t p10 = t32[bilinear_texel_offset<BLOCKED>(w, ix1, iy0)];
    const uint32_t p01 = t32[bilinear_texel_offset<BLOCKED>(w, ix0, iy1)];
    const uint32_t p11 = t32[bilinear_texel_offset<BLOCKED>(w, ix1, iy1)];
    const float inv255 = 1.0f / 255.0f;
    float o[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float c00 = (float)((p00 >> (8 * c)) & 0xffu) * inv255, c10 = (float)((p10 >> (8 * c)) & 0xffu) * inv255;
        const float c01 = (float)((p01 >> (8 * c)) & 0xffu) * inv255, c11 = (float)((p11 >> (8 * c)) & 0xffu) * inv255;
        const float top = c00 * (1.0f - fx) + c10 * fx;
        const float bot = c01 * (1.0f - fx) + c11 * fx;
        o[c] = top * (1.0f - fy) + bot * fy;
    }
    return make_float4(o[0], o[1], o[2], o[3]);
}
// w_signed < 0 (bilinear only): `tex` is the block-linear copy of a texture of width -w_signed
__device__ __forceinline__ float4 texture_fetch(const uint8_t* __restrict__ tex, int w_signed, int h_signed, float tu, float tv) {
    if (h_signed >= 0) return texture_sample(tex, w_signed, h_signed, tu, tv);
    return w_signed < 0 ? texture_sample_bilinear<true>(tex, -w_signed, -h_signed, tu, tv) : texture_sample_bilinear<false>(tex, w_signed, -h_signed, tu, tv);
}

// One texture slot of a run-time compiled program as a draw (user programs, slots 1 .. SWR_PROGRAM_TEXTURES - 1) or a present (post
// programs) captured it, in texture_fetch's sign convention, which is also DrawParams::tex / tex_w / tex_h's: h < 0: the bilinear
// filter; w < 0 as well: `texels` is the block-linear copy; texels null: nothing bound.  The host fills it (texture_slot_of, swr_host.h).
struct TextureSlot { const uint8_t* texels; int w, h; };
static_assert(sizeof(TextureSlot) == 16 && alignof(TextureSlot) == 8, "three of them follow the 64 constants of a user block");
__device__ __forceinline__ bool texture_slot_bound(const TextureSlot& t) { return t.texels != nullptr; }
// Texture.Sample of a slot; (1, 1, 1, 1) from an unbound one, as a draw without a texture samples
__device__ __forceinline__ float4 texture_slot_sample(const TextureSlot& t, float tu, float tv) {
    if (!texture_slot_bound(t)) return make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    return texture_fetch(t.texels, t.w, t.h, tu, tv);
}
// the size, positive whatever the filter and the layout; (0, 0) of an unbound slot
__device__ __forceinline__ int2 texture_slot_size(const TextureSlot& t) {
    if (!texture_slot_bound(t)) return make_int2(0, 0);
    return make_int2(t.w < 0 ? -t.w : t.w, t.h < 0 ? -t.h : t.h);
}
// texel (x, y), x clamped to [0, w - 1] and y to [0, h - 1], each byte times the float 1 / 255 (Texture.cs:57-62): no filter, no uv
__device__ __forceinline__ float4 texture_slot_texel(const TextureSlot& t, int x, int y) {
    if (!texture_slot_bound(t)) return make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    const int w = t.w < 0 ? -t.w : t.w, h = t.h < 0 ? -t.h : t.h;
    x = x < 0 ? 0 : (x > w - 1 ? w - 1 : x); y = y < 0 ? 0 : (y > h - 1 ? h - 1 : y);
    const uint32_t* __restrict__ t32 = reinterpret_cast<const uint32_t*>(t.texels);
    return texture_unpack(t32[t.w < 0 ? bilinear_texel_offset<true>(w, x, y) : bilinear_texel_offset<false>(w, x, y)]);
}

// DEPTH TEXTURES (build-defined; include/swr.h; tests/depth_texture_cases.py restates these in numpy).  A slot
// that holds a depth texture has the same record: its 4-byte texels are float32 depth words as the raster stage stores them.  The
// program says what the words mean by which function it calls, as a GLSL program does with sampler2DShadow; the functions above read
// the same words as RGBA8, which is defined and memory-safe.  None of these is called by a kernel of the product library.
// The word of texel (x, y) in either layout:
__device__ __forceinline__ float texture_slot_depth_word(const TextureSlot& t, int w, int x, int y) {
    const float* __restrict__ f = reinterpret_cast<const float*>(t.texels);
    return f[t.w < 0 ? bilinear_texel_offset<true>(w, x, y) : bilinear_texel_offset<false>(w, x, y)];
}
// texel (x, y), x clamped to [0, w - 1] and y to [0, h - 1]; float.MinValue -- the cleared depth: nothing was drawn -- from an unbound slot
__device__ __forceinline__ float texture_slot_depth_texel(const TextureSlot& t, int x, int y) {
    if (!texture_slot_bound(t)) return SWR_FLOAT_MINVALUE;
    const int w = t.w < 0 ? -t.w : t.w, h = t.h < 0 ? -t.h : t.h;
    x = x < 0 ? 0 : (x > w - 1 ? w - 1 : x); y = y < 0 ? 0 : (y > h - 1 ? h - 1 : y);
    return texture_slot_depth_word(t, w, x, y);
}
// the texel Texture.Sample's addressing picks (Texture.cs:43-54: texture_nearest_index), ALWAYS nearest whatever the filter: depth
// words are not blended.  (Its x and y are taken back out of the index only where the slot holds the block-linear copy.)
__device__ __forceinline__ float texture_slot_depth_sample(const TextureSlot& t, float tu, float tv) {
    if (!texture_slot_bound(t)) return SWR_FLOAT_MINVALUE;
    const int w = t.w < 0 ? -t.w : t.w, h = t.h < 0 ? -t.h : t.h;
    const uint32_t i = texture_nearest_index(w, h, tu, tv);
    if (t.w >= 0) return reinterpret_cast<const float*>(t.texels)[i];
    const uint32_t y = i / (uint32_t)w;
    return texture_slot_depth_word(t, w, (int)(i - y * (uint32_t)w), (int)y);
}
// 1 where a fragment of depth `ref` would pass the default test (LessEqual: new >= old, Rasterizer.cs:545; false for NaN) against the
// stored depth, else 0; the bias is the caller's, added into ref.  Nearest filter (h >= 0): the one texel texture_slot_depth_sample
// reads.  Bilinear filter (h < 0): the footprint and the fractions of texture_sample_bilinear, the four RESULTS in {0, 1} blended
// (percentage-closer filtering) -- as lerps, so that where all four agree every difference is exactly 0 and the result exactly 0 or 1
// (the colour filter's c (1 - fx) + c fx does not promise that, and programs branch on == 1.0f).  An unbound slot: 1, lit.
__device__ __forceinline__ float texture_slot_shadow(const TextureSlot& t, float tu, float tv, float ref) {
    if (!texture_slot_bound(t)) return 1.0f;
    if (t.h >= 0) return ref >= texture_slot_depth_sample(t, tu, tv) ? 1.0f : 0.0f;
    const int w = t.w < 0 ? -t.w : t.w, h = -t.h;
    const float x = tu * (float)w - 0.5f, y = tv * (float)h - 0.5f;
    const float x0 = floorf(x), y0 = floorf(y);
    const float fx = x - x0, fy = y - y0;
    int ix0 = f2i(x0) % w; if (ix0 < 0) ix0 += w;
    int iy0 = f2i(y0) % h; if (iy0 < 0) iy0 += h;
    const int ix1 = ix0 + 1 == w ? 0 : ix0 + 1, iy1 = iy0 + 1 == h ? 0 : iy0 + 1;
    const float c00 = ref >= texture_slot_depth_word(t, w, ix0, iy0) ? 1.0f : 0.0f, c10 = ref >= texture_slot_depth_word(t, w, ix1, iy0) ? 1.0f : 0.0f;
    const float c01 = ref >= texture_slot_depth_word(t, w, ix0, iy1) ? 1.0f : 0.0f, c11 = ref >= texture_slot_depth_word(t, w, ix1, iy1) ? 1.0f : 0.0f;
    const float top = c00 + (c10 - c00) * fx;
    const float bot = c01 + (c11 - c01) * fx;
    return top + (bot - top) * fy;
}

// MIP CHAINS (build-defined; include/swr.h; tests/mipmap_cases.py restates these in numpy).  A slot is 16 bytes
// and stays so, so "how many levels, and where" travels in the texture's memory: every texel array the library allocates -- row-major
// or block-linear, either format, created from the host or as a target -- has this record in the 256 bytes in front of texel 0
// (the rest of them zero), written on the context's stream with the texels.  Without a chain: levels 1, tail null.  With one
// (swr_texture_generate_mipmaps): L = 1 + floor(log2(max(w, h))) levels, level l measuring max(1, w >> l) by max(1, h >> l); level 0
// stays where the slot points, in the slot's layout, and levels 1 .. L - 1 lie row-major, one behind the other, in `tail`.
// None of the functions below is called by a kernel of the product library; the device reads the record when a kernel runs.
#define SWR_TEXTURE_HEADER_BYTES 256
#define SWR_TEXTURE_MAX_LEVELS 32
struct TextureHeader {
    uint32_t levels;                            // 1: no chain
    uint32_t reserved;                          // 0
    const uint8_t* tail;                        // texel 0 of level 1; null without a chain
    uint32_t offset[SWR_TEXTURE_MAX_LEVELS];    // offset[l], l >= 1: level l's first texel, in texels from `tail`; offset[0] = 0
};
static_assert(sizeof(TextureHeader) == 144 && sizeof(TextureHeader) <= SWR_TEXTURE_HEADER_BYTES && __builtin_offsetof(TextureHeader, levels) == 0 &&
              __builtin_offsetof(TextureHeader, reserved) == 4 && __builtin_offsetof(TextureHeader, tail) == 8 && __builtin_offsetof(TextureHeader, offset) == 16,
              "the record in front of every texel array");
// the record of a BOUND slot
__device__ __forceinline__ const TextureHeader* texture_slot_header(const TextureSlot& t) {
    return reinterpret_cast<const TextureHeader*>(t.texels - SWR_TEXTURE_HEADER_BYTES);
}
// 0 for an unbound slot (answered before any load), else 1 or L
__device__ __forceinline__ int texture_slot_levels(const TextureSlot& t) {
    if (!texture_slot_bound(t)) return 0;
    return (int)texture_slot_header(t)->levels;
}
// One level, `level` clamped to [0, levels - 1].  Level 0 is texture_slot_sample itself; a level >= 1 applies the slot's filter inside
// that level, with that level's size, over its row-major texels.  (1, 1, 1, 1) from an unbound slot.
__device__ __forceinline__ float4 texture_slot_sample_level(const TextureSlot& t, int level, float tu, float tv) {
    if (!texture_slot_bound(t)) return make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    const TextureHeader* __restrict__ hd = texture_slot_header(t);
    const int top = (int)hd->levels - 1;
    level = level < 0 ? 0 : (level > top ? top : level);
    if (level == 0) return texture_slot_sample(t, tu, tv);
    const int w = t.w < 0 ? -t.w : t.w, h = t.h < 0 ? -t.h : t.h;
    const int wl = (w >> level) > 1 ? (w >> level) : 1, hl = (h >> level) > 1 ? (h >> level) : 1;
    const uint8_t* __restrict__ texels = hd->tail + 4u * (size_t)hd->offset[level];
    return t.h >= 0 ? texture_sample(texels, wl, hl, tu, tv) : texture_sample_bilinear<false>(texels, wl, hl, tu, tv);
}
// The level of detail of a fragment whose uv moves by (dudx, dvdx) per pixel step in x and (dudy, dvdy) in y: the longer of the two
// steps measured in level-0 texels, rho, through a piecewise-linear log2 taken from rho's bits -- exponent + (significand - 1): exact at
// powers of two, never above log2(rho) and never more than 0.0861 below it (the maximum of log2 m - (m - 1), at m = 1 / ln 2).  Nothing
// fuses and nothing transcendental is called, so numpy restates it bit for bit.  !(rho > 1) -- magnification, zero, any NaN -- is 0;
// the result is clamped to levels - 1 (+Inf too); an unbound slot gives 0.
__device__ __forceinline__ float texture_slot_lod(const TextureSlot& t, float dudx, float dvdx, float dudy, float dvdy) {
    if (!texture_slot_bound(t)) return 0.0f;
    const float wf = (float)(t.w < 0 ? -t.w : t.w), hf = (float)(t.h < 0 ? -t.h : t.h);
    const float ax = dudx * wf, ay = dvdx * hf, bx = dudy * wf, by = dvdy * hf;
    const float rx = ax * ax + ay * ay, ry = bx * bx + by * by;
    const float r2 = (ry > rx || ry != ry) ? ry : rx;                          // the larger; a NaN from either side
    const float rho = sqrtf(r2);
    if (!(rho > 1.0f)) return 0.0f;
    const uint32_t bits = __float_as_uint(rho);
    const int e = (int)(bits >> 23) - 127;                                     // (rho > 1: the sign bit is clear)
    const float m = __uint_as_float((bits & 0x007fffffu) | 0x3f800000u);
    const float lod = (float)e + (m - 1.0f);
    const float top = (float)((int)texture_slot_header(t)->levels - 1);
    return lod > top ? top : lod;
}
// Between two levels: a NaN or negative lod counts as 0, one above levels - 1 as levels - 1; l0 = (int)lod, f = lod - l0.  f == 0 fetches
// level l0 alone; otherwise each channel is c0 (1 - f) + c1 f in the bilinear filter's form, c1 from level min(l0 + 1, levels - 1).
__device__ __forceinline__ float4 texture_slot_sample_lod(const TextureSlot& t, float tu, float tv, float lod) {
    if (!texture_slot_bound(t)) return make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    const int top = (int)texture_slot_header(t)->levels - 1;
    if (!(lod > 0.0f)) lod = 0.0f;
    if (lod > (float)top) lod = (float)top;
    const int l0 = (int)lod;
    const float f = lod - (float)l0;
    const float4 c0 = texture_slot_sample_level(t, l0, tu, tv);
    if (f == 0.0f) return c0;
    const float4 c1 = texture_slot_sample_level(t, l0 + 1 > top ? top : l0 + 1, tu, tv);
    return make_float4(c0.x * (1.0f - f) + c1.x * f, c0.y * (1.0f - f) + c1.y * f, c0.z * (1.0f - f) + c1.z * f, c0.w * (1.0f - f) + c1.w * f);
}

// CUBE MAPS (build-defined; include/swr.h; tests/cubemap_cases.py restates these in numpy).  A cube of side n is
// an ordinary texture n wide and 6 n high: face f (0..5 = +X, -X, +Y, -Y, +Z, -Z) is rows [f n, (f + 1) n), in either format and either
// layout (n % 4 == 0: face f starts f n^2 texels into the block-linear copy too).  The slot's record does not say "cube": the program
// does, by the function it calls.  A slot that is unbound or whose |h| != 6 |w| is NOT A CUBE, which is answered before any load: the
// colour functions give (1, 1, 1, 1), the depth word is float.MinValue, the shadow 1, the size 0.  None of these is called by a kernel of
// the product library.
// The face a direction points at and where in it, (s, t) in [0, 1]^2 with t growing downwards: a right-handed world seen from inside;
// face f is the image of a camera along the face's axis with up +Y (+Y: up +Z, -Y: up -Z) under the reference's screen mapping
// (Rasterizer.cs:383-386).  The larger magnitude wins, ties in the order X, Y, Z; -0 counts as positive.  A direction with a NaN or an
// Inf, and the zero vector: face 0, s = t = 0.5.  s and t are exactly 0 or 1 on a face's edge (the divide is correctly rounded).
__device__ __forceinline__ void texture_cube_face(float x, float y, float z, int& face, float& s, float& t) {
    const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
    const float flt_max = 3.402823466e+38f;
    face = 0; s = 0.5f; t = 0.5f;
    if (!(ax <= flt_max && ay <= flt_max && az <= flt_max)) return;
    if (ax == 0.0f && ay == 0.0f && az == 0.0f) return;
    float ma, sc, tc;
    if (ax >= ay && ax >= az) { ma = ax; face = x < 0 ? 1 : 0; sc = x < 0 ? -z : z; tc = -y; }
    else if (ay >= az)        { ma = ay; face = y < 0 ? 3 : 2; sc = x;              tc = y < 0 ? z : -z; }
    else                      { ma = az; face = z < 0 ? 5 : 4; sc = z < 0 ? x : -x; tc = -y; }
    const float qs = sc / ma, qt = tc / ma;
    s = (qs + 1.0f) * 0.5f;
    t = (qt + 1.0f) * 0.5f;
}
// n of a cube, 0 of anything else (no load)
__device__ __forceinline__ int texture_slot_cube_size(const TextureSlot& t) {
    if (!texture_slot_bound(t)) return 0;
    const int w = t.w < 0 ? -t.w : t.w, h = t.h < 0 ? -t.h : t.h;
    return (w >= 1 && h % 6 == 0 && h / 6 == w) ? w : 0;
}
// one level of a cube as the functions below address it: 6 faces of n x n four-byte texels, face-major
struct CubeLevel { const uint32_t* texels; int n; bool blocked; };
__device__ __forceinline__ CubeLevel cube_level0(const TextureSlot& t, int n) {
    return CubeLevel{ reinterpret_cast<const uint32_t*>(t.texels), n, t.w < 0 };
}
__device__ __forceinline__ uint32_t cube_word(const CubeLevel& c, int face, int x, int y) {       // x, y inside the face
    const int row = face * c.n + y;
    return c.texels[c.blocked ? bilinear_texel_offset<true>(c.n, x, row) : bilinear_texel_offset<false>(c.n, x, row)];
}
// the nearest texel of (s, t): (min((int)(s n), n - 1), min((int)(t n), n - 1))
__device__ __forceinline__ void cube_nearest(int n, float s, float t, int& x, int& y) {
    x = (int)(s * (float)n); y = (int)(t * (float)n);
    x = x > n - 1 ? n - 1 : x; y = y > n - 1 ? n - 1 : y;
}
// the bilinear footprint of (s, t): X = s n - 0.5, x0 = floor(X), fx = X - x0, taps x0 and x0 + 1 each clamped to [0, n - 1] -- the
// footprint never leaves the face (filtering across face edges is out of scope: a seam of up to one texel of clamped colour)
__device__ __forceinline__ void cube_footprint(int n, float s, float t, int& x0, int& x1, int& y0, int& y1, float& fx, float& fy) {
    const float X = s * (float)n - 0.5f, Y = t * (float)n - 0.5f;
    const float fx0 = floorf(X), fy0 = floorf(Y);
    fx = X - fx0; fy = Y - fy0;
    const int ix = (int)fx0, iy = (int)fy0;
    x0 = ix < 0 ? 0 : (ix > n - 1 ? n - 1 : ix); x1 = ix + 1 < 0 ? 0 : (ix + 1 > n - 1 ? n - 1 : ix + 1);
    y0 = iy < 0 ? 0 : (iy > n - 1 ? n - 1 : iy); y1 = iy + 1 < 0 ? 0 : (iy + 1 > n - 1 ? n - 1 : iy + 1);
}
// the slot's filter inside one level: nearest unpacked as Texture.Sample unpacks it, bilinear blended in texture_sample_bilinear's form
__device__ __forceinline__ float4 cube_level_sample(const CubeLevel& c, bool bilinear, float x, float y, float z) {
    int face; float s, t;
    texture_cube_face(x, y, z, face, s, t);
    if (!bilinear) {
        int tx, ty;
        cube_nearest(c.n, s, t, tx, ty);
        return texture_unpack(cube_word(c, face, tx, ty));
    }
    int x0, x1, y0, y1; float fx, fy;
    cube_footprint(c.n, s, t, x0, x1, y0, y1, fx, fy);
    const uint32_t p00 = cube_word(c, face, x0, y0), p10 = cube_word(c, face, x1, y0);
    const uint32_t p01 = cube_word(c, face, x0, y1), p11 = cube_word(c, face, x1, y1);
    const float inv255 = 1.0f / 255.0f;
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float c00 = (float)((p00 >> (8 * k)) & 0xffu) * inv255, c10 = (float)((p10 >> (8 * k)) & 0xffu) * inv255;
        const float c01 = (float)((p01 >> (8 * k)) & 0xffu) * inv255, c11 = (float)((p11 >> (8 * k)) & 0xffu) * inv255;
        const float top = c00 * (1.0f - fx) + c10 * fx;
        const float bot = c01 * (1.0f - fx) + c11 * fx;
        o[k] = top * (1.0f - fy) + bot * fy;
    }
    return make_float4(o[0], o[1], o[2], o[3]);
}
// level 0 by direction, with the slot's filter
__device__ __forceinline__ float4 texture_slot_sample_cube(const TextureSlot& t, float x, float y, float z) {
    const int n = texture_slot_cube_size(t);
    if (n == 0) return make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    return cube_level_sample(cube_level0(t, n), t.h < 0, x, y, z);
}
// texel (x, y) of a face: face clamped to [0, 5], x and y to [0, n - 1]; no filter, no direction
__device__ __forceinline__ float4 texture_slot_cube_texel(const TextureSlot& t, int face, int x, int y) {
    const int n = texture_slot_cube_size(t);
    if (n == 0) return make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    face = face < 0 ? 0 : (face > 5 ? 5 : face);
    x = x < 0 ? 0 : (x > n - 1 ? n - 1 : x); y = y < 0 ? 0 : (y > n - 1 ? n - 1 : y);
    return texture_unpack(cube_word(cube_level0(t, n), face, x, y));
}
// the last level a cube lookup may name: what the record says (texture_slot_sample_level's clamp), and never past floor(log2 n) -- a
// cube's chain ends there (swr_texture_generate_mipmaps), and in the longer chain of an n x 6 n texture that was not created as a cube
// the levels beyond it hold fewer than six faces' rows
__device__ __forceinline__ int cube_top_level(const TextureSlot& t, int n) {
    const int top = (int)texture_slot_header(t)->levels - 1, cap = 31 - __builtin_clz((unsigned)n);
    return top < cap ? (top < 0 ? 0 : top) : cap;
}
// One level of a cube's chain, `level` clamped to [0, top]: level l is the n_l x 6 n_l atlas with n_l = n >> l, row-major behind the
// header's tail; the slot's filter is applied inside it.  Level 0 is texture_slot_sample_cube.
__device__ __forceinline__ float4 texture_slot_sample_cube_level(const TextureSlot& t, int level, float x, float y, float z) {
    const int n = texture_slot_cube_size(t);
    if (n == 0) return make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    const int top = cube_top_level(t, n);
    level = level < 0 ? 0 : (level > top ? top : level);
    if (level == 0) return cube_level_sample(cube_level0(t, n), t.h < 0, x, y, z);
    const TextureHeader* __restrict__ hd = texture_slot_header(t);
    const CubeLevel c{ reinterpret_cast<const uint32_t*>(hd->tail) + hd->offset[level], n >> level, false };
    return cube_level_sample(c, t.h < 0, x, y, z);
}
// between two levels, blended as texture_slot_sample_lod blends them
__device__ __forceinline__ float4 texture_slot_sample_cube_lod(const TextureSlot& t, float x, float y, float z, float lod) {
    const int n = texture_slot_cube_size(t);
    if (n == 0) return make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    const int top = cube_top_level(t, n);
    if (!(lod > 0.0f)) lod = 0.0f;
    if (lod > (float)top) lod = (float)top;
    const int l0 = (int)lod;
    const float f = lod - (float)l0;
    const float4 c0 = texture_slot_sample_cube_level(t, l0, x, y, z);
    if (f == 0.0f) return c0;
    const float4 c1 = texture_slot_sample_cube_level(t, l0 + 1 > top ? top : l0 + 1, x, y, z);
    return make_float4(c0.x * (1.0f - f) + c1.x * f, c0.y * (1.0f - f) + c1.y * f, c0.z * (1.0f - f) + c1.z * f, c0.w * (1.0f - f) + c1.w * f);
}
// A DEPTH cube (swr_texture_create_cube_depth): the word of the nearest texel, ALWAYS nearest whatever the filter
__device__ __forceinline__ float texture_slot_cube_depth_sample(const TextureSlot& t, float x, float y, float z) {
    const int n = texture_slot_cube_size(t);
    if (n == 0) return SWR_FLOAT_MINVALUE;
    int face, tx, ty; float s, tt;
    texture_cube_face(x, y, z, face, s, tt);
    cube_nearest(n, s, tt, tx, ty);
    return __uint_as_float(cube_word(cube_level0(t, n), face, tx, ty));
}
// texture_slot_shadow by direction: nearest filter, ref >= word ? 1 : 0 of the one texel; bilinear filter, the four comparisons over
// the clamped footprint blended as lerps -- exactly 0 or 1 where the four agree.  Not a cube: 1, lit.
__device__ __forceinline__ float texture_slot_shadow_cube(const TextureSlot& t, float x, float y, float z, float ref) {
    const int n = texture_slot_cube_size(t);
    if (n == 0) return 1.0f;
    if (t.h >= 0) return ref >= texture_slot_cube_depth_sample(t, x, y, z) ? 1.0f : 0.0f;
    int face; float s, tt;
    texture_cube_face(x, y, z, face, s, tt);
    int x0, x1, y0, y1; float fx, fy;
    cube_footprint(n, s, tt, x0, x1, y0, y1, fx, fy);
    const CubeLevel c = cube_level0(t, n);
    const float c00 = ref >= __uint_as_float(cube_word(c, face, x0, y0)) ? 1.0f : 0.0f, c10 = ref >= __uint_as_float(cube_word(c, face, x1, y0)) ? 1.0f : 0.0f;
    const float c01 = ref >= __uint_as_float(cube_word(c, face, x0, y1)) ? 1.0f : 0.0f, c11 = ref >= __uint_as_float(cube_word(c, face, x1, y1)) ? 1.0f : 0.0f;
    const float top = c00 + (c10 - c00) * fx;
    const float bot = c01 + (c11 - c01) * fx;
    return top + (bot - top) * fy;
}

// The per-draw block of a user-program batch (RasterArgs::user_consts, k_vertex_user's last argument): the draw's 64 captured constants,
// then its captured texture slots 1 .. SWR_PROGRAM_TEXTURES - 1 as TextureSlot records (slot 0 is the draw's texture, in DrawParams).
// Only run-time compiled kernels read it.  76 words, 304 bytes: every block and every record in it is 16-byte aligned.
#define SWR_USER_CONSTANTS 64
#define SWR_USER_BLOCK_WORDS (SWR_USER_CONSTANTS + 4 * (SWR_PROGRAM_TEXTURES - 1))
static_assert(SWR_USER_BLOCK_WORDS == 64 + 3 * 4 && SWR_USER_BLOCK_WORDS % 4 == 0, "64 constants and three 16-byte slots");

}  // namespace swr
