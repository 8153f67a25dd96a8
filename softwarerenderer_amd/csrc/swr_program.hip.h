// swr_program.hip.h -- the source contract of USER programs (swr_program_create / swr_program_create_vf, include/swr.h).  Compiled
// only at run time (hiprtc, SWR_RTC_PROGRAM defined): the library embeds this header and the kernel headers, the prelude below comes
// first, then the user's text(s), then k_raster_c (and, for a program with a vertex half, k_vertex_user and its k_setup).  The product
// library never includes it.
//
// The user defines the fragment half:
//     __device__ float4 swr_fragment(const swr_fs_in& in, const swr_fs_env& env);
// `in` is Shaders.VertexOutput after Rasterizer.Interpolate (Rasterizer.cs:566-640) with Interpolate = true, computed with the
// arithmetic the built-in programs use.  The function is inlined into the raster kernel, so varyings it never reads are never
// interpolated (or loaded).  A result with W <= 0 or NaN writes nothing (Rasterizer.cs:511): swr_discard() is such a result.
//
// ... and, optionally (SWR_USER_VERTEX defined), the vertex half -- any Shaders.VertexShader delegate:
//     __device__ void swr_vertex(const swr_vs_in& in, const swr_vs_env& env, swr_vs_out& out);
// `out` is `new Shaders.VertexOutput()`, all zeros, Interpolate = true.  Without a vertex half the vertex stage is Renderer.VertexShader
// (Renderer.cs:830-846, k_vertex), as for SWR_PROG_DUST2_LAMBERT_FOG, and swr_fs_in::data4 reads (0, 0, 0, 0).
#pragma once

// include/swr.h calls the 48-byte input vertex `swr_vertex`, the name the contract gives the user's vertex function: in the code
// object of a program with a vertex half the record goes by another name (only DrawParams::verts refers to it)
#ifdef SWR_USER_VERTEX
#define swr_vertex swr_vertex_record
#endif
#include "swr_user_math.hip.h"           // hiprtc's fixed-width types; swr_lerp, swr_max, swr_clamp (shared with swr_post.hip.h)
#include "swr_raster.hip.h"
#ifdef SWR_USER_VERTEX
#undef swr_vertex
#endif

// Shaders.VertexOutput after Interpolate
struct swr_fs_in {
    float4 clip_position;        // ClipPosition (x, y, z, w)
    float4 color;                // Color
    float2 tex_coord;            // TexCoord
    float3 normal;               // Normal (object space, VertexInput.Normal interpolated)
    float2 screen_coords;        // ScreenCoords (pixel position / (width - 1, height - 1) at the vertices, Rasterizer.cs:390)
    float3 barycentric;          // Barycentric (the perspective-correct weights wa, wb, wc, Rasterizer.cs:583-585,638)
    float3 world_normal;         // Data["WorldNormal"]: weighted sum renormalised (Rasterizer.cs:680-688)
    float4 data4;                // the user's own Vector4 key of VertexOutput.Data (swr_vs_out::data4): weighted sum with the normalised
                                 // weights, nothing else (Rasterizer.cs:690-693); zeros when the program has no vertex half
    float4 tex_coord_grad;       // build-defined (mip chains): (du/dx, dv/dx, du/dy, dv/dy), the analytic derivative of
                                 // tex_coord per pixel step in x and in y at this fragment -- what swr_sample_grad takes.  Per fragment:
                                 // there are no quads and no neighbours (a chunk's fragments are compacted), so no finite differences
};

// what a fragment program closes over: the draw's uniform block, its captured constants, the pixel
struct swr_fs_env {
    const swr_uniforms& uniforms;
    const float* constants;      // constants[0..63] (swr_program_set_constants when the draw was recorded; zeros if never set)
    int x, y;                    // pixel
    const uint8_t* tex;          // the draw's texture (null: none) in the layout texture_fetch reads
    int tex_w, tex_h;            // (their signs carry the filter and the layout: swr_texture_size(env, 0) is the size)
    // the library's own, behind the slot helpers below:
    const swr::TextureSlot* slots_;      // the draw's captured texture slots 1 .. SWR_PROGRAM_TEXTURES - 1
};

// Texture.Sample (Texture.cs:43-63): nearest, or the build-defined bilinear filter when the texture was switched to it -- the function
// the built-in programs call.  Without a texture: Vector4.One.
__device__ __forceinline__ bool swr_has_texture(const swr_fs_env& env) { return env.tex != nullptr && env.tex_h != 0; }
__device__ __forceinline__ float4 swr_sample(const swr_fs_env& env, float2 uv) {
    if (!swr_has_texture(env)) return make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    return swr::texture_fetch(env.tex, env.tex_w, env.tex_h, uv.x, uv.y);
}
// THE TEXTURE SLOTS (swr_program_set_texture).  Slot 0 is the draw's texture, slots 1 .. SWR_PROGRAM_TEXTURES - 1
// are the program's, as they were when the draw was recorded.  An unbound slot, and a slot outside 0 .. SWR_PROGRAM_TEXTURES - 1, has no
// texture: it samples and reads (1, 1, 1, 1) and measures (0, 0).  The slot may be computed per fragment.  A program that calls none of
// these loads nothing of the slots.
//   swr_has_texture(env, slot)
//   swr_sample(env, slot, uv)         Texture.Sample exactly as swr_sample(env, uv) computes it for slot 0 (swr::texture_fetch)
//   swr_texel(env, slot, x, y)        the row-major texel (x, y), x clamped to [0, w - 1] and y to [0, h - 1], each byte times 1 / 255
//   swr_texture_size(env, slot)       (w, h), positive whatever the filter
// swr_slot_: the slot's record, for either half's env (slot0 = the draw's texture as that half holds it)
__device__ __forceinline__ swr::TextureSlot swr_slot_(const swr::TextureSlot& slot0, const swr::TextureSlot* slots, int slot) {
    if (slot == 0) return slot0;
    if ((unsigned)(slot - 1) < (unsigned)(SWR_PROGRAM_TEXTURES - 1)) return slots[slot - 1];
    return swr::TextureSlot{ nullptr, 0, 0 };
}
__device__ __forceinline__ swr::TextureSlot swr_slot_(const swr_fs_env& env, int slot) {
    return swr_slot_(swr::TextureSlot{ swr_has_texture(env) ? env.tex : nullptr, env.tex_w, env.tex_h }, env.slots_, slot);
}
__device__ __forceinline__ bool swr_has_texture(const swr_fs_env& env, int slot) { return swr::texture_slot_bound(swr_slot_(env, slot)); }
__device__ __forceinline__ float4 swr_sample(const swr_fs_env& env, int slot, float2 uv) { return swr::texture_slot_sample(swr_slot_(env, slot), uv.x, uv.y); }
__device__ __forceinline__ float4 swr_texel(const swr_fs_env& env, int slot, int x, int y) { return swr::texture_slot_texel(swr_slot_(env, slot), x, y); }
__device__ __forceinline__ int2 swr_texture_size(const swr_fs_env& env, int slot) { return swr::texture_slot_size(swr_slot_(env, slot)); }
// A slot that holds a DEPTH texture (swr_texture_create_depth, swr_texture_update_from_depth) is read through
// these three (swr_device.h has the definitions); an unbound slot has nothing drawn in it: float.MinValue, and every fragment is lit.
//   swr_texel_depth(env, slot, x, y)   the float32 depth word of texel (x, y), clamped as swr_texel clamps
//   swr_sample_depth(env, slot, uv)    the word of the texel Texture.Sample's addressing picks: nearest whatever the filter
//   swr_shadow(env, slot, uv, ref)     1 where ref >= the stored depth (a fragment of depth ref passes LessEqual), else 0: one texel
//                                      under the nearest filter, the 2 x 2 footprint's four results blended under the bilinear one
__device__ __forceinline__ float swr_texel_depth(const swr_fs_env& env, int slot, int x, int y) { return swr::texture_slot_depth_texel(swr_slot_(env, slot), x, y); }
__device__ __forceinline__ float swr_sample_depth(const swr_fs_env& env, int slot, float2 uv) { return swr::texture_slot_depth_sample(swr_slot_(env, slot), uv.x, uv.y); }
__device__ __forceinline__ float swr_shadow(const swr_fs_env& env, int slot, float2 uv, float ref) { return swr::texture_slot_shadow(swr_slot_(env, slot), uv.x, uv.y, ref); }
// A slot's MIP CHAIN (swr_texture_generate_mipmaps; definitions in swr_device.h).  The record is read when the
// kernel runs.  An unbound or out-of-range slot: 0 levels, lod 0, samples (1, 1, 1, 1).
//   swr_texture_levels(env, slot)             1 without a chain, L with one
//   swr_sample_level(env, slot, uv, level)    one level, clamped to [0, levels - 1], the slot's filter applied inside it; level 0 is swr_sample
//   swr_sample_lod(env, slot, uv, lod)        between levels (int)lod and the next: c0 (1 - f) + c1 f; one fetch where f == 0
//   swr_lod(env, slot, grad)                  grad = (dudx, dvdx, dudy, dvdy): the piecewise-linear log2 of the longer step in texels
//   swr_sample_grad(env, slot, uv, grad)      swr_sample_lod(env, slot, uv, swr_lod(env, slot, grad)); grad = in.tex_coord_grad for in.tex_coord
__device__ __forceinline__ int swr_texture_levels(const swr_fs_env& env, int slot) { return swr::texture_slot_levels(swr_slot_(env, slot)); }
__device__ __forceinline__ float4 swr_sample_level(const swr_fs_env& env, int slot, float2 uv, int level) { return swr::texture_slot_sample_level(swr_slot_(env, slot), level, uv.x, uv.y); }
__device__ __forceinline__ float4 swr_sample_lod(const swr_fs_env& env, int slot, float2 uv, float lod) { return swr::texture_slot_sample_lod(swr_slot_(env, slot), uv.x, uv.y, lod); }
__device__ __forceinline__ float swr_lod(const swr_fs_env& env, int slot, float4 grad) { return swr::texture_slot_lod(swr_slot_(env, slot), grad.x, grad.y, grad.z, grad.w); }
__device__ __forceinline__ float4 swr_sample_grad(const swr_fs_env& env, int slot, float2 uv, float4 grad) { return swr_sample_lod(env, slot, uv, swr_lod(env, slot, grad)); }
// A slot that holds a CUBE MAP (swr_texture_create_cube, swr_texture_update_face_from_frame; definitions in
// swr_device.h): six faces +X, -X, +Y, -Y, +Z, -Z looked up by a direction from the cube's centre, of any length.  A slot that is unbound,
// out of range or not n by 6 n is not a cube: it samples (1, 1, 1, 1), reads float.MinValue, shadows nothing (1) and measures 0.
//   swr_cube_face(dir, &face, &uv)              the face the direction points at and where in it, uv in [0, 1]^2, v downwards
//   swr_sample_cube(env, slot, dir)             the slot's filter inside that face: nearest, or bilinear with its 2 x 2 taps clamped to the face
//   swr_sample_cube_level / _lod(env, slot, dir, level | lod)   the same inside the levels of the cube's chain (swr_sample_level / _lod)
//   swr_cube_texel(env, slot, face, x, y)       one texel, face clamped to [0, 5] and x, y to the face
//   swr_cube_size(env, slot)                    n
//   swr_sample_cube_depth(env, slot, dir)       a DEPTH cube's word, always nearest
//   swr_shadow_cube(env, slot, dir, ref)        swr_shadow by direction (a point light: dir = world - light)
__device__ __forceinline__ void swr_cube_face(float3 dir, int* face, float2* uv) { swr::texture_cube_face(dir.x, dir.y, dir.z, *face, uv->x, uv->y); }
__device__ __forceinline__ float4 swr_sample_cube(const swr_fs_env& env, int slot, float3 dir) { return swr::texture_slot_sample_cube(swr_slot_(env, slot), dir.x, dir.y, dir.z); }
__device__ __forceinline__ float4 swr_sample_cube_level(const swr_fs_env& env, int slot, float3 dir, int level) { return swr::texture_slot_sample_cube_level(swr_slot_(env, slot), level, dir.x, dir.y, dir.z); }
__device__ __forceinline__ float4 swr_sample_cube_lod(const swr_fs_env& env, int slot, float3 dir, float lod) { return swr::texture_slot_sample_cube_lod(swr_slot_(env, slot), dir.x, dir.y, dir.z, lod); }
__device__ __forceinline__ float4 swr_cube_texel(const swr_fs_env& env, int slot, int face, int x, int y) { return swr::texture_slot_cube_texel(swr_slot_(env, slot), face, x, y); }
__device__ __forceinline__ int swr_cube_size(const swr_fs_env& env, int slot) { return swr::texture_slot_cube_size(swr_slot_(env, slot)); }
__device__ __forceinline__ float swr_sample_cube_depth(const swr_fs_env& env, int slot, float3 dir) { return swr::texture_slot_cube_depth_sample(swr_slot_(env, slot), dir.x, dir.y, dir.z); }
__device__ __forceinline__ float swr_shadow_cube(const swr_fs_env& env, int slot, float3 dir, float ref) { return swr::texture_slot_shadow_cube(swr_slot_(env, slot), dir.x, dir.y, dir.z, ref); }
// the build's System.Numerics model (SWR_DOT_PAIRWISE): Vector3.Dot.  (swr_lerp, swr_max and swr_clamp: swr_user_math.hip.h)
__device__ __forceinline__ float swr_dot3(float3 a, float3 b) { return swr::dot3(a.x, a.y, a.z, b.x, b.y, b.z); }
// a null result: nothing is written (and under BlendMode.None the row's early-out applies)
__device__ __forceinline__ float4 swr_discard() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

// the user's program (always inlined into the raster kernel)
__device__ __attribute__((always_inline)) float4 swr_fragment(const swr_fs_in& in, const swr_fs_env& env);

#ifdef SWR_USER_VERTEX
// Shaders.VertexInput (Shaders.cs:10-24)
struct swr_vs_in {
    float3 position;
    float2 uv;
    float3 normal;
    float4 color;
};
// what a vertex delegate receives and closes over.  Everything here is uniform over the draw: the kernel reads it with scalar loads.
struct swr_vs_env {
    const float* model;          // 16 floats each, row-major M11..M44 as include/swr.h lays them out
    const float* view;
    const float* projection;
    const swr_uniforms& uniforms;
    const float* constants;      // constants[0..63]: the SAME captured constants the fragment half reads
    uint32_t nm_flags;           // the context's System.Numerics model of Transform / TransformNormal (swr_set_transform_fma) when the
                                 // draw was recorded: the helpers below read it
    // the library's own, behind the slot helpers below:
    const swr::DrawParams* draw_;        // slot 0: the draw's texture
    const swr::TextureSlot* slots_;      // the draw's captured texture slots 1 .. SWR_PROGRAM_TEXTURES - 1
};
// The texture slots in the vertex half: the four functions of the fragment half over the same four slots, the same bytes and the same
// sampler -- a value sampled here and one sampled in the fragment half at the same uv are the same words.
__device__ __forceinline__ swr::TextureSlot swr_slot_(const swr_vs_env& env, int slot) {
    return swr_slot_(swr::TextureSlot{ env.draw_->tex_h != 0 ? env.draw_->tex : nullptr, env.draw_->tex_w, env.draw_->tex_h }, env.slots_, slot);
}
__device__ __forceinline__ bool swr_has_texture(const swr_vs_env& env, int slot) { return swr::texture_slot_bound(swr_slot_(env, slot)); }
__device__ __forceinline__ float4 swr_sample(const swr_vs_env& env, int slot, float2 uv) { return swr::texture_slot_sample(swr_slot_(env, slot), uv.x, uv.y); }
__device__ __forceinline__ float4 swr_texel(const swr_vs_env& env, int slot, int x, int y) { return swr::texture_slot_texel(swr_slot_(env, slot), x, y); }
__device__ __forceinline__ int2 swr_texture_size(const swr_vs_env& env, int slot) { return swr::texture_slot_size(swr_slot_(env, slot)); }
__device__ __forceinline__ float swr_texel_depth(const swr_vs_env& env, int slot, int x, int y) { return swr::texture_slot_depth_texel(swr_slot_(env, slot), x, y); }
__device__ __forceinline__ float swr_sample_depth(const swr_vs_env& env, int slot, float2 uv) { return swr::texture_slot_depth_sample(swr_slot_(env, slot), uv.x, uv.y); }
__device__ __forceinline__ float swr_shadow(const swr_vs_env& env, int slot, float2 uv, float ref) { return swr::texture_slot_shadow(swr_slot_(env, slot), uv.x, uv.y, ref); }
__device__ __forceinline__ int swr_texture_levels(const swr_vs_env& env, int slot) { return swr::texture_slot_levels(swr_slot_(env, slot)); }
__device__ __forceinline__ float4 swr_sample_level(const swr_vs_env& env, int slot, float2 uv, int level) { return swr::texture_slot_sample_level(swr_slot_(env, slot), level, uv.x, uv.y); }
__device__ __forceinline__ float4 swr_sample_lod(const swr_vs_env& env, int slot, float2 uv, float lod) { return swr::texture_slot_sample_lod(swr_slot_(env, slot), uv.x, uv.y, lod); }
__device__ __forceinline__ float swr_lod(const swr_vs_env& env, int slot, float4 grad) { return swr::texture_slot_lod(swr_slot_(env, slot), grad.x, grad.y, grad.z, grad.w); }
__device__ __forceinline__ float4 swr_sample_grad(const swr_vs_env& env, int slot, float2 uv, float4 grad) { return swr_sample_lod(env, slot, uv, swr_lod(env, slot, grad)); }
__device__ __forceinline__ float4 swr_sample_cube(const swr_vs_env& env, int slot, float3 dir) { return swr::texture_slot_sample_cube(swr_slot_(env, slot), dir.x, dir.y, dir.z); }
__device__ __forceinline__ float4 swr_sample_cube_level(const swr_vs_env& env, int slot, float3 dir, int level) { return swr::texture_slot_sample_cube_level(swr_slot_(env, slot), level, dir.x, dir.y, dir.z); }
__device__ __forceinline__ float4 swr_sample_cube_lod(const swr_vs_env& env, int slot, float3 dir, float lod) { return swr::texture_slot_sample_cube_lod(swr_slot_(env, slot), dir.x, dir.y, dir.z, lod); }
__device__ __forceinline__ float4 swr_cube_texel(const swr_vs_env& env, int slot, int face, int x, int y) { return swr::texture_slot_cube_texel(swr_slot_(env, slot), face, x, y); }
__device__ __forceinline__ int swr_cube_size(const swr_vs_env& env, int slot) { return swr::texture_slot_cube_size(swr_slot_(env, slot)); }
__device__ __forceinline__ float swr_sample_cube_depth(const swr_vs_env& env, int slot, float3 dir) { return swr::texture_slot_cube_depth_sample(swr_slot_(env, slot), dir.x, dir.y, dir.z); }
__device__ __forceinline__ float swr_shadow_cube(const swr_vs_env& env, int slot, float3 dir, float ref) { return swr::texture_slot_shadow_cube(swr_slot_(env, slot), dir.x, dir.y, dir.z, ref); }
// new Shaders.VertexOutput() (Shaders.cs:26-47): zero-initialised before swr_vertex is called, Interpolate = true
struct swr_vs_out {
    float4 clip_position;        // ClipPosition
    float4 color;                // Color
    float2 tex_coord;            // TexCoord
    float3 normal;               // Normal
    float3 world_normal;         // Data["WorldNormal"] (Vector3 key: the raster stage renormalises its weighted sum)
    float4 data4;                // one Vector4 key of the user's own: lerped in the clipper, weighted sum in the raster stage
};
// Vector4.Transform(v, M), Vector3.TransformNormal(n, M), Vector3.Normalize(v) = v / v.Length(): the functions k_vertex calls, under
// the draw's run-time flags, so a restated Renderer.VertexShader gives k_vertex's bits in every library build and flag setting
__device__ __forceinline__ float4 swr_transform(float4 v, const float* m, const swr_vs_env& env) {
    const float p[4] = { v.x, v.y, v.z, v.w };
    float o[4];
    swr::vec4_transform(p, m, o, (env.nm_flags & SWR_NM_TRANSFORM_FMA) != 0u);
    return make_float4(o[0], o[1], o[2], o[3]);
}
__device__ __forceinline__ float3 swr_transform_normal(float3 n, const float* m, const swr_vs_env& env) {
    const float p[3] = { n.x, n.y, n.z };
    float o[3];
    swr::vec3_transform_normal(p, m, o, (env.nm_flags & SWR_NM_TRANSFORM_NORMAL_FMA) != 0u);
    return make_float3(o[0], o[1], o[2]);
}
__device__ __forceinline__ float3 swr_normalize(float3 v) {
    const float len = sqrtf(swr::dot3(v.x, v.y, v.z, v.x, v.y, v.z));
    return make_float3(v.x / len, v.y / len, v.z / len);
}
// the user's vertex program (always inlined into k_vertex_user, swr_geometry.hip.h)
__device__ __attribute__((always_inline)) void swr_vertex(const swr_vs_in& in, const swr_vs_env& env, swr_vs_out& out);
#endif

namespace swr {

// Rasterizer.Interpolate (Interpolate = true) of everything swr_fs_in holds, from the three outputs as the raster kernel loads them:
// clip / colour / uv + wn.xy / wn.z rows of VOut, Normal from the side array, the screen positions from the TriRec.  The divisions
// are the IEEE ones (shade_fragment's division cores return the same quotients), the sums in the reference's order.  d4 = the user
// vertex program's data4 at the three outputs (zeros without a vertex half).
__device__ __forceinline__ swr_fs_in interpolate_fs_in(float w0f, float w1f, float w2f, const float4 clip[3], const float4 col[3],
                                                       const float4 uvn[3], const float wnz[3], const float4 nrm[3], const float4 d4[3], const float sx[3],
                                                       const float sy[3], float inv_width, float inv_height) {
    const float ra = w0f / clip[0].w, rb = w1f / clip[1].w, rc = w2f / clip[2].w;        // :576-578
    const float inv_sum = (ra + rb) + rc;                                                 // :579
    const float w = 1.0f / inv_sum;                                                       // :582
    const float wa = ra * w, wb = rb * w, wc = rc * w;                                    // :583-585
    auto persp = [&](float a_, float b_, float c_) { return (((a_ * ra + b_ * rb) + c_ * rc) * w); };      // Vector4.Multiply / Add / Multiply
    swr_fs_in in;
    in.clip_position = make_float4(persp(clip[0].x, clip[1].x, clip[2].x), persp(clip[0].y, clip[1].y, clip[2].y),
                                   persp(clip[0].z, clip[1].z, clip[2].z), persp(clip[0].w, clip[1].w, clip[2].w));
    in.color = make_float4(persp(col[0].x, col[1].x, col[2].x), persp(col[0].y, col[1].y, col[2].y),
                           persp(col[0].z, col[1].z, col[2].z), persp(col[0].w, col[1].w, col[2].w));
    in.tex_coord = make_float2(persp(uvn[0].x, uvn[1].x, uvn[2].x), persp(uvn[0].y, uvn[1].y, uvn[2].y));
    in.normal = make_float3(persp(nrm[0].x, nrm[1].x, nrm[2].x), persp(nrm[0].y, nrm[1].y, nrm[2].y), persp(nrm[0].z, nrm[1].z, nrm[2].z));
    // outputs[i].ScreenCoords = (screenCoords[i].X * invWidth, screenCoords[i].Y * invHeight), :390
    const float s0x = sx[0] * inv_width, s1x = sx[1] * inv_width, s2x = sx[2] * inv_width;
    const float s0y = sy[0] * inv_height, s1y = sy[1] * inv_height, s2y = sy[2] * inv_height;
    in.screen_coords = make_float2(persp(s0x, s1x, s2x), persp(s0y, s1y, s2y));
    in.barycentric = make_float3(wa, wb, wc);
    // InterpolateData, Vector3 key: weighted sum with the normalised weights, then 1 / MathF.Sqrt(lengthSquared) (:680-688)
    float n0 = (uvn[0].z * wa + uvn[1].z * wb) + uvn[2].z * wc;
    float n1 = (uvn[0].w * wa + uvn[1].w * wb) + uvn[2].w * wc;
    float n2 = (wnz[0] * wa + wnz[1] * wb) + wnz[2] * wc;
    const float len_sq = dot3(n0, n1, n2, n0, n1, n2);
    if (len_sq > 1e-6f) {
        const float s = 1.0f / sqrtf(len_sq);
        n0 = n0 * s; n1 = n1 * s; n2 = n2 * s;
    }
    in.world_normal = make_float3(n0, n1, n2);
    // InterpolateData, Vector4 key: (a * wa + b * wb) + c * wc, no division and no renormalisation (:690-693)
    in.data4 = make_float4((d4[0].x * wa + d4[1].x * wb) + d4[2].x * wc, (d4[0].y * wa + d4[1].y * wb) + d4[2].y * wc,
                           (d4[0].z * wa + d4[1].z * wb) + d4[2].z * wc, (d4[0].w * wa + d4[1].w * wb) + d4[2].w * wc);
    // tex_coord_grad: tex_coord = N / D with N = sum u_i b_i / w_i and D = sum b_i / w_i, b_i the screen-space barycentrics, which are
    // linear in the pixel: their steps are the edge coefficients over the area (Rasterizer.cs:445-447, 527-534), so d(N / D) = (dN - (N / D) dD) / D
    // with 1 / D = w.  A program that never reads the field computes none of this (the program is inlined).
    const float area = (sx[2] - sx[0]) * (sy[1] - sy[0]) - (sy[2] - sy[0]) * (sx[1] - sx[0]);        // EdgeFunction, :411
    const float ia = 1.0f / area;                                                                    // :427
    const float g0x = (sy[1] - sy[2]) * ia, g0y = (sx[2] - sx[1]) * ia;
    const float g1x = (sy[2] - sy[0]) * ia, g1y = (sx[0] - sx[2]) * ia;
    const float g2x = (sy[0] - sy[1]) * ia, g2y = (sx[1] - sx[0]) * ia;
    const float q0x = g0x / clip[0].w, q1x = g1x / clip[1].w, q2x = g2x / clip[2].w;
    const float q0y = g0y / clip[0].w, q1y = g1y / clip[1].w, q2y = g2y / clip[2].w;
    const float dx = (q0x + q1x) + q2x, dy = (q0y + q1y) + q2y;
    const float nux = (uvn[0].x * q0x + uvn[1].x * q1x) + uvn[2].x * q2x, nuy = (uvn[0].x * q0y + uvn[1].x * q1y) + uvn[2].x * q2y;
    const float nvx = (uvn[0].y * q0x + uvn[1].y * q1x) + uvn[2].y * q2x, nvy = (uvn[0].y * q0y + uvn[1].y * q1y) + uvn[2].y * q2y;
    in.tex_coord_grad = make_float4((nux - in.tex_coord.x * dx) * w, (nvx - in.tex_coord.y * dx) * w,
                                    (nuy - in.tex_coord.x * dy) * w, (nvy - in.tex_coord.y * dy) * w);
    return in;
}

}  // namespace swr
