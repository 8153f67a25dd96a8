// swr_post.hip.h -- post-process programs: a user's per-pixel pass between the frame and its delivery.
//
// Build-defined (the reference presents the frame as rendered, MainWindow.cs:234-240): the text a caller hands to swr_post_create
// runs once per OUTPUT pixel of a present, on the resolved frame, and its result leaves the device in the present's format.
//
// THE DEFINITION (tests/post_cases.py restates it in numpy).  The user's text defines
//     __device__ float4 swr_post(const swr_post_in& in, const swr_post_env& env);
//   in.x, in.y    the output pixel, in window coordinates after the resolve
//   in.color      the resolved pixel: R, G, B the floats swr_readback_rgb_resolved(kx, ky) delivers (the flatten's under (1, 1)), A the
//                 frame's alpha through the same balanced pairwise tree and the same multiply by 1 / (kx ky) (resolve_pixel,
//                 swr_deliver.hip.h)
//   env.width, env.height   the resolved size;  env.kx, env.ky  the factors
//   env.constants           64 floats, captured when the present call is made (swr_post_set_constants; zeros if never set)
//   swr_post_fetch(env, x, y)   the resolved RGBA of output pixel (x, y), x clamped to [0, width - 1] and y to [0, height - 1]
//   swr_post_depth(env, x, y)   the depth word of sample (x kx, y ky), the top-left sample of the pixel's block, clamped the same way;
//                               not averaged; float.MinValue where the depth plane was cleared
//   swr_lerp, swr_max, swr_clamp   swr_user_math.hip.h: the definitions fragment programs call
//   swr_post_has_texture / _sample / _texel / _texture_size (env, slot, ..)   the program's SWR_POST_TEXTURES texture slots as they were
//                               when the present call was made (tests/post_texture_cases.py restates them)
// What the result becomes:
//   SWR_POST_RGB32F   x, y, z stored as they are (no clamp)
//   SWR_POST_RGB8     quantise8 of x, y, z (swr_deliver.hip.h), three bytes
//   SWR_POST_RGBX8    the same and a fourth byte of 255, one dword
//   w is ignored -- except by swr_texture_update_from_post (SWR_POST_TEXELS_KEEP below), where quantise8(w) is the texel's alpha.
//
//   k_post<FORMAT>  (run-time compiled with the user's text, SWR_RTC_POST; five instantiations per program) one thread per OUTPUT pixel on
//                   the delivery kernels' grid (deliver_pixel, swr_deliver.hip.h): the thread loads its pixel of the resolved plane
//                   (k_resolve_rgba's; the frame itself under (1, 1)), calls the inlined swr_post and stores with the stores of
//                   k_resolve_rgb / k_present8.  The constants and the texture slots are a by-value kernel argument: no device buffer
//                   outlives the call.
//                   SWR_POST_TEXELS_OPAQUE / _KEEP (swr_texture_update_from_post; not present formats): k_frame_to_texture's store,
//                   the dword row-major into `out`, its alpha 255 or quantise8(w) -- and, where the argument carries a block-linear
//                   copy, the same dword at bilinear_texel_offset<true>.
// No LDS, no scratch, no inline assembly.  A frame is at most 65535 x 65535 (swr_resize), so pixel indices fit 32 bits; offsets are size_t.
#pragma once
#include "swr_user_math.hip.h"
#include "swr_deliver.hip.h"

#define SWR_POST_CONSTANTS 64
// k_post's internal formats behind swr_texture_update_from_post: RGBA8 texels, alpha 255 or the result's w
#define SWR_POST_TEXELS_OPAQUE 16
#define SWR_POST_TEXELS_KEEP 17

namespace swr {

// k_post's last argument, by value: the program's constants and texture slots (TextureSlot, swr_device.h) as they were when the present
// call was made, and for the texel formats the target's block-linear copy (null: it has none)
struct PostConstants {
    float v[SWR_POST_CONSTANTS];
    TextureSlot tex[SWR_POST_TEXTURES];
    uint32_t* blocked;
};

}  // namespace swr

#ifdef SWR_RTC_POST
struct swr_post_in {
    int x, y;                    // the output pixel
    float4 color;                // the resolved pixel: swr_post_fetch(env, x, y)
};

struct swr_post_env {
    int width, height;           // the resolved size
    int kx, ky;                  // the resolve factors
    const float* constants;      // constants[0..63] (swr_post_set_constants when the present call was made; zeros if never set)
    // the library's own, behind the helpers below:
    const float4* plane_;        // height x width resolved pixels (the frame itself under (1, 1))
    const float* depth_;         // the frame's depth plane, height * ky rows of width * kx words
    const swr::TextureSlot* textures_;    // the SWR_POST_TEXTURES slots (kernel arguments: constant memory)
};

__device__ __forceinline__ int swr_post_clamp_index(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }
__device__ __forceinline__ float4 swr_post_fetch(const swr_post_env& env, int x, int y) {
    x = swr_post_clamp_index(x, env.width); y = swr_post_clamp_index(y, env.height);
    return env.plane_[(size_t)y * (size_t)env.width + (size_t)x];
}
__device__ __forceinline__ float swr_post_depth(const swr_post_env& env, int x, int y) {
    x = swr_post_clamp_index(x, env.width); y = swr_post_clamp_index(y, env.height);
    return env.depth_[(size_t)y * (size_t)env.ky * ((size_t)env.width * (size_t)env.kx) + (size_t)x * (size_t)env.kx];
}

// The texture slots.  A slot outside 0 .. SWR_POST_TEXTURES - 1 is an unbound one.
__device__ __forceinline__ bool swr_post_has_texture(const swr_post_env& env, int slot) {
    return (unsigned)slot < (unsigned)SWR_POST_TEXTURES && env.textures_[slot].texels != nullptr;
}
// Texture.Sample as a draw sees it (swr_sample): nearest with wrap, or the build-defined bilinear filter if the texture was switched to
// it when the present call was made; (1, 1, 1, 1) from an unbound slot
__device__ __forceinline__ float4 swr_post_sample(const swr_post_env& env, int slot, float2 uv) {
    if (!swr_post_has_texture(env, slot)) return make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    return swr::texture_slot_sample(env.textures_[slot], uv.x, uv.y);
}
__device__ __forceinline__ int2 swr_post_texture_size(const swr_post_env& env, int slot) {
    if (!swr_post_has_texture(env, slot)) return make_int2(0, 0);
    return swr::texture_slot_size(env.textures_[slot]);
}
// texel (x, y), x clamped to [0, w - 1] and y to [0, h - 1], each byte times the float 1 / 255 (Texture.cs:57-62): no filter, no uv
__device__ __forceinline__ float4 swr_post_texel(const swr_post_env& env, int slot, int x, int y) {
    if (!swr_post_has_texture(env, slot)) return make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    return swr::texture_slot_texel(env.textures_[slot], x, y);
}
// A slot that holds a DEPTH texture: swr_texel_depth, swr_sample_depth and swr_shadow of a user program
// (swr_program.hip.h; definitions in swr_device.h).  An unbound slot reads float.MinValue and shadows nothing (1).
__device__ __forceinline__ swr::TextureSlot swr_post_slot_(const swr_post_env& env, int slot) {
    return (unsigned)slot < (unsigned)SWR_POST_TEXTURES ? env.textures_[slot] : swr::TextureSlot{ nullptr, 0, 0 };
}
__device__ __forceinline__ float swr_post_texel_depth(const swr_post_env& env, int slot, int x, int y) { return swr::texture_slot_depth_texel(swr_post_slot_(env, slot), x, y); }
__device__ __forceinline__ float swr_post_sample_depth(const swr_post_env& env, int slot, float2 uv) { return swr::texture_slot_depth_sample(swr_post_slot_(env, slot), uv.x, uv.y); }
__device__ __forceinline__ float swr_post_shadow(const swr_post_env& env, int slot, float2 uv, float ref) { return swr::texture_slot_shadow(swr_post_slot_(env, slot), uv.x, uv.y, ref); }
// A slot's MIP CHAIN: swr_texture_levels, swr_sample_level, swr_sample_lod and swr_lod of a user program.  A post
// pass has no gradient field: it knows its own scale.  An unbound or out-of-range slot: 0 levels, lod 0, samples (1, 1, 1, 1).
__device__ __forceinline__ int swr_post_texture_levels(const swr_post_env& env, int slot) { return swr::texture_slot_levels(swr_post_slot_(env, slot)); }
__device__ __forceinline__ float4 swr_post_sample_level(const swr_post_env& env, int slot, float2 uv, int level) { return swr::texture_slot_sample_level(swr_post_slot_(env, slot), level, uv.x, uv.y); }
__device__ __forceinline__ float4 swr_post_sample_lod(const swr_post_env& env, int slot, float2 uv, float lod) { return swr::texture_slot_sample_lod(swr_post_slot_(env, slot), uv.x, uv.y, lod); }
__device__ __forceinline__ float swr_post_lod(const swr_post_env& env, int slot, float4 grad) { return swr::texture_slot_lod(swr_post_slot_(env, slot), grad.x, grad.y, grad.z, grad.w); }
// A slot's CUBE MAP: swr_cube_face, swr_sample_cube, swr_sample_cube_level, swr_sample_cube_lod, swr_cube_texel,
// swr_cube_size, swr_sample_cube_depth and swr_shadow_cube of a user program.  Not a cube (unbound, out of range, not n by 6 n):
// (1, 1, 1, 1), float.MinValue, shadow 1, size 0.
__device__ __forceinline__ void swr_post_cube_face(float3 dir, int* face, float2* uv) { swr::texture_cube_face(dir.x, dir.y, dir.z, *face, uv->x, uv->y); }
__device__ __forceinline__ float4 swr_post_sample_cube(const swr_post_env& env, int slot, float3 dir) { return swr::texture_slot_sample_cube(swr_post_slot_(env, slot), dir.x, dir.y, dir.z); }
__device__ __forceinline__ float4 swr_post_sample_cube_level(const swr_post_env& env, int slot, float3 dir, int level) { return swr::texture_slot_sample_cube_level(swr_post_slot_(env, slot), level, dir.x, dir.y, dir.z); }
__device__ __forceinline__ float4 swr_post_sample_cube_lod(const swr_post_env& env, int slot, float3 dir, float lod) { return swr::texture_slot_sample_cube_lod(swr_post_slot_(env, slot), dir.x, dir.y, dir.z, lod); }
__device__ __forceinline__ float4 swr_post_cube_texel(const swr_post_env& env, int slot, int face, int x, int y) { return swr::texture_slot_cube_texel(swr_post_slot_(env, slot), face, x, y); }
__device__ __forceinline__ int swr_post_cube_size(const swr_post_env& env, int slot) { return swr::texture_slot_cube_size(swr_post_slot_(env, slot)); }
__device__ __forceinline__ float swr_post_sample_cube_depth(const swr_post_env& env, int slot, float3 dir) { return swr::texture_slot_cube_depth_sample(swr_post_slot_(env, slot), dir.x, dir.y, dir.z); }
__device__ __forceinline__ float swr_post_shadow_cube(const swr_post_env& env, int slot, float3 dir, float ref) { return swr::texture_slot_shadow_cube(swr_post_slot_(env, slot), dir.x, dir.y, dir.z, ref); }

// the user's program (always inlined into k_post)
__device__ __attribute__((always_inline)) float4 swr_post(const swr_post_in& in, const swr_post_env& env);

namespace swr {

// plane: out_rows x out_w resolved pixels; depth: the frame's depth plane; out: out_rows * out_w pixels of 12 (RGB32F), 3 or 4 bytes
// (the texel formats: 4, a texture's d_rgba)
template <int FORMAT>
__global__ __launch_bounds__(SWR_RESOLVE_BLOCK_X * SWR_RESOLVE_BLOCK_Y)
void k_post(const float4* __restrict__ plane, const float* __restrict__ depth, void* __restrict__ out, uint32_t out_w, uint32_t out_rows,
            int kx, int ky, const PostConstants constants) {
    static_assert(FORMAT == SWR_POST_RGB32F || FORMAT == SWR_POST_RGB8 || FORMAT == SWR_POST_RGBX8 || FORMAT == SWR_POST_TEXELS_OPAQUE ||
                  FORMAT == SWR_POST_TEXELS_KEEP, "a present format or a texel format");
    uint32_t ox, oy;
    if (!deliver_pixel(out_w, out_rows, ox, oy)) return;
    const swr_post_env env = { (int)out_w, (int)out_rows, kx, ky, constants.v, plane, depth, constants.tex };
    const size_t pixel = deliver_index(out_w, ox, oy);
    const swr_post_in in = { (int)ox, (int)oy, plane[pixel] };
    const float4 c = swr_post(in, env);
    if constexpr (FORMAT == SWR_POST_RGB32F) store_rgb32f(static_cast<float*>(out), pixel, c.x, c.y, c.z);
    else if constexpr (FORMAT == SWR_POST_RGB8) store_rgb8(static_cast<uint8_t*>(out), pixel, pack8<false>(c.x, c.y, c.z, c.w));
    else if constexpr (FORMAT == SWR_POST_RGBX8) store_rgbx8(static_cast<uint8_t*>(out), pixel, pack8<false>(c.x, c.y, c.z, c.w));
    else store_texel(static_cast<uint32_t*>(out), constants.blocked, constants.blocked != nullptr, out_w, ox, oy, pack8<FORMAT == SWR_POST_TEXELS_KEEP>(c.x, c.y, c.z, c.w));
}

}  // namespace swr
#endif
