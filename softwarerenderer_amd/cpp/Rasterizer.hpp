// Rasterizer.hpp -- C++ host-side mirror of the reference's raster API over the C ABI of include/swr.h.
//
// The reference is C# (no .NET toolchain in this image), so the compiled-language host above the ABI is C++.
// Same names, argument meaning and error behaviour as the reference (file:line under OCSYT/SoftwareRenderer):
//   SoftwareRenderer::Rasterizer::RenderMesh / InitializeTileLocks, enums, statics   Rasterizer.cs:14-50,69,163
//   SoftwareRenderer::Shaders::VertexInput                                           Shaders.cs:10-24
//   SoftwareRenderer::Texture (Width/Height/Sample/Dispose)                          Texture.cs:31-68
//   SoftwareRenderer::MainWindow (RenderWidth/Height, buffers, Get/Set*, Clear*)     MainWindow.cs:25-31,378-436
// C# delegates cannot cross the ABI: a ShaderProgram {program id, uniforms, texture} stands in for the
// (VertexShader, FragmentShader) pair.  Header-only; link with -lswr_hip (softwarerenderer_amd/libswr_hip.so).
#pragma once

#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "swr.h"

namespace SoftwareRenderer {

struct SwrError : std::runtime_error {
    int code;
    SwrError(int c, const std::string& m) : std::runtime_error("swr error " + std::to_string(c) + ": " + m), code(c) {}
};

using Matrix4x4 = std::array<float, 16>;     // M11..M44 row-major, row-vector convention (System.Numerics layout)
using Vector4 = std::array<float, 4>;

class Texture;
class Mesh;
class PoseSet;
class Device {                                // one swr_context = one GPU
public:
    explicit Device(int device_id = 0) {
        int rc = swr_create(device_id, &ctx_);
        if (rc != SWR_OK) throw SwrError(rc, swr_last_error(nullptr));
    }
    ~Device() { if (ctx_) swr_destroy(ctx_); }
    Device(const Device&) = delete;
    Device& operator=(const Device&) = delete;
    swr_context* ctx() const { return ctx_; }
    void check(int rc) const {
        if (rc == SWR_OK) return;
        std::string msg = swr_last_error(ctx_);
        if (rc == SWR_ERR_INVALID_ARG) throw std::invalid_argument(msg);   // C#: ArgumentException / IndexOutOfRangeException
        throw SwrError(rc, msg);
    }
    void Flush() const { check(swr_flush(ctx_)); }
    void Sync() const { check(swr_sync(ctx_)); }
    swr_stats Stats() const { swr_stats s; check(swr_get_stats(ctx_, &s)); return s; }
    void ResetStats() const { check(swr_reset_stats(ctx_)); }
    // user fragment programs (contract in swr.h): compile errors throw std::invalid_argument carrying the compiler's log
    int CompileProgram(const std::string& source) const { int id = 0; check(swr_program_create(ctx_, source.c_str(), &id)); return id; }
    // ... with a vertex half (swr_vertex, include/swr.h): any Shaders.VertexShader restated in C++
    int CompileProgram(const std::string& vertex_source, const std::string& source) const {
        int id = 0; check(swr_program_create_vf(ctx_, vertex_source.c_str(), source.c_str(), &id)); return id;
    }
    void DestroyProgram(int id) const { check(swr_program_destroy(ctx_, id)); }
    void SetProgramConstants(int id, const std::vector<float>& values) const {
        check(swr_program_set_constants(ctx_, id, values.empty() ? nullptr : values.data(), (int)values.size()));
    }
    // a texture of this device in slot 1 .. SWR_PROGRAM_TEXTURES - 1 of a user program (null unbinds; slot 0 is the draw's texture),
    // read in both halves with swr_sample / swr_texel(env, slot, ..); captured, with the texture's filter, by each draw when recorded
    inline void SetProgramTexture(int id, int slot, const Texture* texture) const;
    // dsts[k] = srcs[k] skinned by the palette of instances[k] of `set`, all jobs in ONE kernel launch (swr_mesh_skin_batch): word for
    // word what Mesh::SkinFrom gives with that palette; two jobs may share a source or an instance
    inline void SkinBatch(const std::vector<Mesh*>& dsts, const std::vector<const Mesh*>& srcs, const PoseSet& set,
                          const std::vector<int32_t>& instances) const;
private:
    swr_context* ctx_ = nullptr;
};

struct ShaderProgram;
struct Shaders {
    using VertexInput = swr_vertex;           // Shaders.cs:10-24, 48 bytes
    enum class Program { FlatColor = SWR_PROG_FLAT_COLOR, Gouraud = SWR_PROG_GOURAUD,
                         Dust2LambertFog = SWR_PROG_DUST2_LAMBERT_FOG, Phong4Point = SWR_PROG_PHONG_4POINT };
    // any Shaders.FragmentShader restated in C++ against the contract of swr.h, compiled for `dev` (a user program)
    static ShaderProgram Custom(const Device& dev, const std::string& source, const swr_uniforms& uniforms = swr_uniforms{},
                                const Texture* texture = nullptr, std::vector<float> constants = {});
    // ... and any (Shaders.VertexShader, Shaders.FragmentShader) pair: the vertex half (swr_vertex) runs as a vertex kernel of its own
    static ShaderProgram Custom(const Device& dev, const std::string& vertex_source, const std::string& source,
                                const swr_uniforms& uniforms = swr_uniforms{}, const Texture* texture = nullptr,
                                std::vector<float> constants = {});
};
static_assert(sizeof(Shaders::VertexInput) == 48, "VertexInput must match Shaders.cs:10-24");

class MainWindow;
class PostProgram;
class Texture {                               // Texture.cs:31-68
public:
    Texture(const Device& dev, const uint8_t* rgba8, int width, int height) : dev_(dev), Width(width), Height(height) {
        dev_.check(swr_texture_create(dev_.ctx(), rgba8, width, height, &h_));
    }
    ~Texture() { Dispose(); }
    // render to texture (build-defined, swr.h): a texture of zeros without host data, to be filled by UpdateFrom
    static Texture Target(const Device& dev, int width, int height) { return Texture(dev, width, height); }
    // the texels become the window's frame of Width * kx by Height * ky pixels, box-filtered and quantised as the 8-bit present; the
    // window may belong to another Device on the same GPU.  Immediate-mode semantics, no wait for the GPU
    inline void UpdateFrom(const MainWindow& window, int kx = 1, int ky = 1, bool keepAlpha = false);
    // ... with `post`, a program of the window's Device, between the resolve and the quantiser (swr_texture_update_from_post): alpha
    // 255, or the quantised w of the program's result.  The texture may not be bound to a slot of `post`
    inline void UpdateFromPost(const MainWindow& window, const PostProgram& post, int kx = 1, int ky = 1, bool keepAlpha = false);
    // depth textures (build-defined, swr.h): float32 depth words as the raster stage stores them -- `depth` (Width * Height floats) or,
    // null, float.MinValue everywhere; filled by UpdateFromDepth, read in programs through swr_shadow / swr_sample_depth / swr_texel_depth
    static Texture Depth(const Device& dev, int width, int height, const float* depth = nullptr) { return Texture(dev, width, height, depth, DepthTag{}); }
    // each texel becomes one word of its kx x ky block of the window's depth plane: SWR_DEPTH_REDUCE_MAX (the nearest under LessEqual),
    // _MIN or _FIRST (top-left).  Otherwise UpdateFrom's contract
    inline void UpdateFromDepth(const MainWindow& window, int kx = 1, int ky = 1, int reduce = SWR_DEPTH_REDUCE_MAX);
    std::vector<float> ReadDepth() const {    // depth words row-major; waits for the GPU
        std::vector<float> out((size_t)Width * (size_t)Height);
        dev_.check(swr_texture_readback_depth(dev_.ctx(), h_, out.data()));
        return out;
    }
    // (the word Texture.Sample's addressing picks, swr_shadow of it against ref) with the texture's filter as it is now (runs on the GPU)
    std::array<float, 2> SampleDepth(float u, float v, float ref) const {
        float in[3] = { u, v, ref }; std::array<float, 2> out{};
        dev_.check(swr_texture_sample_depth(dev_.ctx(), h_, in, 1, out.data()));
        return out;
    }
    int Format() const { int f = -1; dev_.check(swr_texture_format(dev_.ctx(), h_, &f)); return f; }   // SWR_TEXTURE_FORMAT_*
    void SetBilinear(bool on) { dev_.check(swr_texture_set_filter(dev_.ctx(), h_, on ? 1 : 0)); }      // depth: 2 x 2 shadow lookups
    // mip chains (build-defined, swr.h): 1 + floor(log2(max(Width, Height))) levels, each a 2 x 2 box filter of the one before, made on the
    // GPU in UpdateFrom's order and without a wait; kept up to date by UpdateFrom / UpdateFromPost from then on.  Programs read them
    // through swr_sample_grad / swr_sample_lod / swr_sample_level; Sample and the built-in programs stay on level 0
    void GenerateMipmaps() { dev_.check(swr_texture_generate_mipmaps(dev_.ctx(), h_)); }
    int Levels() const { int n = -1; dev_.check(swr_texture_levels(dev_.ctx(), h_, &n)); return n; }    // 1, or L once the chain exists
    std::array<int, 2> LevelSize(int level) const {           // (w, h) of a level of the full chain, generated or not
        std::array<int, 2> wh{}; dev_.check(swr_texture_level_size(dev_.ctx(), h_, level, &wh[0], &wh[1])); return wh;
    }
    std::vector<uint8_t> ReadLevel(int level) const {         // a level the texture has, RGBA8 row-major; waits for the GPU
        const std::array<int, 2> wh = LevelSize(level);
        std::vector<uint8_t> out((size_t)wh[0] * (size_t)wh[1] * 4);
        dev_.check(swr_texture_readback_level(dev_.ctx(), h_, level, out.data()));
        return out;
    }
    Vector4 SampleLod(float u, float v, float lod) const {    // swr_sample_lod as a program computes it (runs on the GPU)
        float in[3] = { u, v, lod }; Vector4 out{};
        dev_.check(swr_texture_sample_lod(dev_.ctx(), h_, in, 1, out.data()));
        return out;
    }
    float Lod(float dudx, float dvdx, float dudy, float dvdy) const {    // swr_lod likewise
        float in[4] = { dudx, dvdx, dudy, dvdy }; float out = 0.0f;
        dev_.check(swr_texture_lod(dev_.ctx(), h_, in, 1, &out));
        return out;
    }
    // cube maps (build-defined, swr.h): a cube of side n is a texture n wide and 6 n high, face f (0..5 = +X, -X, +Y, -Y, +Z, -Z) in rows
    // [f n, (f + 1) n); programs read it through swr_sample_cube / swr_shadow_cube.  The factories are below (Cube, CubeTarget, CubeDepth)
    static Texture Cube(const Device& dev, const uint8_t* faces_rgba8, int n) { return Texture(dev, n, faces_rgba8, CubeTag{}); }   // six faces of n x n, face-major
    static Texture CubeTarget(const Device& dev, int n) { return Texture(dev, n, (const uint8_t*)nullptr, CubeTag{}); }                // zeros, for UpdateFaceFrom
    static Texture CubeDepth(const Device& dev, int n, const float* words = nullptr) { return Texture(dev, n, words, CubeTag{}); }      // float.MinValue without words
    // Matrix4x4.CreateLookAt of a face's camera at `eye` (host only): with CreatePerspectiveFieldOfView(pi / 2, 1, near, far) the pixel
    // whose centre lies in direction d from eye is the texel swr_sample_cube reads for d
    static std::array<float, 16> CubeFaceView(int face, const float eye[3]) {
        std::array<float, 16> view{};
        if (swr_cube_face_view(face, eye, view.data()) != SWR_OK) throw std::invalid_argument("face must be 0 .. 5");
        return view;
    }
    // swr_cube_face as a program computes it (runs on the GPU): the face of a direction and (s, t) in it
    static int CubeFace(const Device& dev, float x, float y, float z, float st[2]) {
        float in[3] = { x, y, z }; int face = -1;
        dev.check(swr_texture_cube_face(dev.ctx(), in, 1, &face, st));
        return face;
    }
    int IsCube() const { int n = -1; dev_.check(swr_texture_is_cube(dev_.ctx(), h_, &n)); return n; }   // n, or 0
    void UpdateFaceFrom(int face, int kx = 1, int ky = 1, bool keep_alpha = false, swr_context* source = nullptr) {
        dev_.check(swr_texture_update_face_from_frame(dev_.ctx(), h_, face, source, kx, ky, keep_alpha ? SWR_TEXTURE_ALPHA_KEEP : SWR_TEXTURE_ALPHA_OPAQUE));
    }
    void UpdateFaceFromDepth(int face, int kx = 1, int ky = 1, int reduce = SWR_DEPTH_REDUCE_MAX, swr_context* source = nullptr) {
        dev_.check(swr_texture_update_face_from_depth(dev_.ctx(), h_, face, source, kx, ky, reduce));
    }
    void UpdateFaceFromPost(int face, int post_id, int kx = 1, int ky = 1, bool keep_alpha = false, swr_context* source = nullptr) {
        dev_.check(swr_texture_update_face_from_post(dev_.ctx(), h_, face, source, post_id, kx, ky, keep_alpha ? SWR_TEXTURE_ALPHA_KEEP : SWR_TEXTURE_ALPHA_OPAQUE));
    }
    std::vector<uint8_t> ReadFace(int face, int level = 0) const {      // (n >> level)^2 texels of 4 bytes: RGBA8, or depth words; waits for the GPU
        const size_t n = (size_t)(Width >> level);
        std::vector<uint8_t> out(n * n * 4);
        dev_.check(swr_texture_readback_face(dev_.ctx(), h_, face, level, out.data()));
        return out;
    }
    Vector4 SampleCube(float x, float y, float z, float lod = 0.0f) const {   // swr_sample_cube_lod as a program computes it (runs on the GPU)
        float in[4] = { x, y, z, lod }; Vector4 out{};
        dev_.check(swr_texture_sample_cube(dev_.ctx(), h_, in, 1, out.data()));
        return out;
    }
    std::array<float, 2> SampleCubeDepth(float x, float y, float z, float ref) const {   // (word, shadow): swr_sample_cube_depth, swr_shadow_cube
        float in[4] = { x, y, z, ref }; std::array<float, 2> out{};
        dev_.check(swr_texture_sample_cube_depth(dev_.ctx(), h_, in, 1, out.data()));
        return out;
    }
    std::vector<uint8_t> Read() const {       // RGBA8 row-major; waits for the GPU
        std::vector<uint8_t> out((size_t)Width * (size_t)Height * 4);
        dev_.check(swr_texture_readback(dev_.ctx(), h_, out.data()));
        return out;
    }
    Vector4 Sample(float u, float v) const {  // Texture.cs:43-63 (runs on the GPU)
        float uv[2] = { u, v }; Vector4 out{};
        dev_.check(swr_texture_sample(dev_.ctx(), h_, uv, 1, out.data()));
        return out;
    }
    void Dispose() { if (h_) { swr_texture_destroy(dev_.ctx(), h_); h_ = nullptr; } }
    swr_texture* handle() const { return h_; }
    const int Width, Height;
private:
    Texture(const Device& dev, int width, int height) : dev_(dev), Width(width), Height(height) {
        dev_.check(swr_texture_create_target(dev_.ctx(), width, height, &h_));
    }
    struct CubeTag {};
    Texture(const Device& dev, int n, const uint8_t* faces, CubeTag) : dev_(dev), Width(n), Height(6 * n) {
        dev_.check(swr_texture_create_cube(dev_.ctx(), faces, n, &h_));
    }
    Texture(const Device& dev, int n, const float* words, CubeTag) : dev_(dev), Width(n), Height(6 * n) {
        dev_.check(swr_texture_create_cube_depth(dev_.ctx(), words, n, &h_));
    }
    struct DepthTag {};
    Texture(const Device& dev, int width, int height, const float* depth, DepthTag) : dev_(dev), Width(width), Height(height) {
        dev_.check(swr_texture_create_depth(dev_.ctx(), depth, width, height, &h_));
    }
    const Device& dev_;
    swr_texture* h_ = nullptr;
};

struct ShaderProgram {                        // stands in for (VertexShader, FragmentShader), Shaders.cs:97-98
    Shaders::Program program = Shaders::Program::Gouraud;   // a built-in, or a user program id (>= SWR_PROG_USER_BASE)
    swr_uniforms uniforms{};
    const Texture* texture = nullptr;
    std::vector<float> constants;             // user programs: set before each draw (each draw captures them when recorded)
    const Texture* textures[SWR_PROGRAM_TEXTURES - 1] = {};   // ... and slots 1 .. 3, likewise (`texture` is slot 0)
};

inline void Device::SetProgramTexture(int id, int slot, const Texture* texture) const {
    check(swr_program_set_texture(ctx_, id, slot, texture ? texture->handle() : nullptr));
}

inline ShaderProgram Shaders::Custom(const Device& dev, const std::string& source, const swr_uniforms& uniforms,
                                     const Texture* texture, std::vector<float> constants) {
    ShaderProgram p;
    p.program = static_cast<Shaders::Program>(dev.CompileProgram(source));
    p.uniforms = uniforms; p.texture = texture; p.constants = std::move(constants);
    return p;
}

inline ShaderProgram Shaders::Custom(const Device& dev, const std::string& vertex_source, const std::string& source,
                                     const swr_uniforms& uniforms, const Texture* texture, std::vector<float> constants) {
    ShaderProgram p;
    p.program = static_cast<Shaders::Program>(dev.CompileProgram(vertex_source, source));
    p.uniforms = uniforms; p.texture = texture; p.constants = std::move(constants);
    return p;
}

inline swr_uniforms DefaultUniforms() {      // Renderer.cs:39-44
    swr_uniforms u{};
    u.light_direction[0] = 0.5f; u.light_direction[1] = -0.70710678f; u.light_direction[2] = -0.5f;
    for (int i = 0; i < 4; ++i) u.light_color[i] = 1.0f;
    u.fog_color[0] = 1.0f; u.fog_color[1] = 0.62f; u.fog_color[2] = 0.5f; u.fog_color[3] = 1.0f;
    u.fog_start = 1.0f; u.fog_end = 25.0f; u.shininess = 16.0f;
    return u;
}

// A post-process program (contract in swr.h: swr_post): a per-pixel pass between the frame and its delivery, compiled for `dev`.
// Compile errors throw std::invalid_argument carrying the compiler's log (post.hip:LINE:).
class PostProgram {
public:
    PostProgram(const Device& dev, const std::string& source) : dev_(dev) { dev_.check(swr_post_create(dev_.ctx(), source.c_str(), &id_)); }
    ~PostProgram() { if (id_) swr_post_destroy(dev_.ctx(), id_); }            // a present in flight with the program still completes
    PostProgram(const PostProgram&) = delete;
    PostProgram& operator=(const PostProgram&) = delete;
    void SetConstants(const std::vector<float>& values) const {               // captured by each present when it is called
        dev_.check(swr_post_set_constants(dev_.ctx(), id_, values.empty() ? nullptr : values.data(), (int)values.size()));
    }
    // a texture of `dev` in slot 0 .. SWR_POST_TEXTURES - 1 (null unbinds), read with swr_post_sample / swr_post_texel; captured,
    // with the texture's filter, by each present when it is called
    void SetTexture(int slot, const Texture* texture) const {
        dev_.check(swr_post_set_texture(dev_.ctx(), id_, slot, texture ? texture->handle() : nullptr));
    }
    int id() const { return id_; }
private:
    const Device& dev_;
    int id_ = 0;
};

class MainWindow {                            // framebuffer part of MainWindow.cs
public:
    MainWindow(const Device& dev, int renderWidth, int renderHeight) : dev_(dev) { Resize(renderWidth, renderHeight); }
    void Resize(int w, int h) { dev_.check(swr_resize(dev_.ctx(), w, h)); RenderWidth = w; RenderHeight = h; }
    void ClearColorBuffer(const Vector4& c) { dev_.check(swr_clear_color(dev_.ctx(), c.data())); }     // MainWindow.cs:400-407
    void ClearDepthBuffer() { dev_.check(swr_clear_depth(dev_.ctx())); }                                // :429-436
    Vector4 GetPixel(int x, int y) const { Vector4 o{}; dev_.check(swr_get_pixel(dev_.ctx(), x, y, o.data())); return o; }
    void SetPixel(int x, int y, const Vector4& c) { dev_.check(swr_set_pixel(dev_.ctx(), x, y, c.data())); }
    float GetDepth(int x, int y) const { float d; dev_.check(swr_get_depth(dev_.ctx(), x, y, &d)); return d; }
    void SetDepth(int x, int y, float d) { dev_.check(swr_set_depth(dev_.ctx(), x, y, d)); }
    // ColorBuffer / DepthBuffer: read the HBM buffers back (Vector4[W*H], float[W*H], idx = y*W + x)
    void ReadBuffers(std::vector<float>* color, std::vector<float>* depth) const {
        size_t n = (size_t)(RenderWidth > 0 ? RenderWidth : 0) * (size_t)(RenderHeight > 0 ? RenderHeight : 0);
        if (color) color->resize(n * 4);
        if (depth) depth->resize(n);
        dev_.check(swr_readback(dev_.ctx(), color ? color->data() : nullptr, depth ? depth->data() : nullptr));
    }
    // The frame after `post`, resolved by kx x ky: format SWR_POST_RGB32F fills float triples, SWR_POST_RGB8 / SWR_POST_RGBX8 bytes
    // (swr_readback_post); `out` is resized to swr_post_size's bytes
    void PostBuffer(const PostProgram& post, int kx, int ky, int format, std::vector<unsigned char>* out) const {
        int w = 0, rows = 0; size_t bytes = 0;
        dev_.check(swr_post_size(dev_.ctx(), kx, ky, format, &w, &rows, &bytes));
        out->resize(bytes);
        if (bytes) dev_.check(swr_readback_post(dev_.ctx(), post.id(), kx, ky, format, out->data()));
    }
    // ... asynchronously into caller memory that stays put until PresentWait(ticket) (swr_present_post_async; shares the slots and
    // tickets of every other present)
    uint64_t PresentPostAsync(const PostProgram& post, int kx, int ky, int format, void* out) const {
        uint64_t t = 0; dev_.check(swr_present_post_async(dev_.ctx(), post.id(), kx, ky, format, out, &t)); return t;
    }
    bool PresentWait(uint64_t ticket) const { int rc = swr_present_wait(dev_.ctx(), ticket); if (rc == SWR_STALE) return false; dev_.check(rc); return true; }
    // ... or into caller DEVICE memory, 4-byte aligned (swr_post_device; wait = false: swr_post_device_async)
    void PostTo(const PostProgram& post, int kx, int ky, int format, void* d_out, bool wait = true) const {
        dev_.check(wait ? swr_post_device(dev_.ctx(), post.id(), kx, ky, format, d_out) : swr_post_device_async(dev_.ctx(), post.id(), kx, ky, format, d_out));
    }
    const Device& device() const { return dev_; }
    int RenderWidth = 0, RenderHeight = 0;
private:
    const Device& dev_;
};

inline void Texture::UpdateFrom(const MainWindow& window, int kx, int ky, bool keepAlpha) {
    swr_context* src = window.device().ctx() == dev_.ctx() ? nullptr : window.device().ctx();
    dev_.check(swr_texture_update_from_frame(dev_.ctx(), h_, src, kx, ky, keepAlpha ? SWR_TEXTURE_ALPHA_KEEP : SWR_TEXTURE_ALPHA_OPAQUE));
}
inline void Texture::UpdateFromDepth(const MainWindow& window, int kx, int ky, int reduce) {
    swr_context* src = window.device().ctx() == dev_.ctx() ? nullptr : window.device().ctx();
    dev_.check(swr_texture_update_from_depth(dev_.ctx(), h_, src, kx, ky, reduce));
}
inline void Texture::UpdateFromPost(const MainWindow& window, const PostProgram& post, int kx, int ky, bool keepAlpha) {
    swr_context* src = window.device().ctx() == dev_.ctx() ? nullptr : window.device().ctx();
    dev_.check(swr_texture_update_from_post(dev_.ctx(), h_, src, post.id(), kx, ky, keepAlpha ? SWR_TEXTURE_ALPHA_KEEP : SWR_TEXTURE_ALPHA_OPAQUE));
}

// A retained mesh (Mesh.Vertices / Mesh.Indices, ModelLoader.cs:45-47, uploaded once) and its deforms on the GPU (build-defined,
// include/swr.h "DEFORMING MESHES"): a blend of two key frames, linear-blend skinning by a joint palette.  Draws, ray queries and
// the bounding sphere follow the pose.
class Mesh {
public:
    Mesh(const Device& dev, const std::vector<Shaders::VertexInput>& vertices, const std::vector<uint16_t>& indices)
        : dev_(dev), n_vertices_((int)vertices.size()) {
        dev_.check(swr_mesh_create(dev_.ctx(), vertices.data(), (int)vertices.size(), indices.data(), (int)indices.size(), &h_));
    }
    ~Mesh() { if (h_) swr_mesh_destroy(dev_.ctx(), h_); }
    Mesh(const Mesh&) = delete;
    Mesh& operator=(const Mesh&) = delete;
    Mesh(Mesh&& o) noexcept : dev_(o.dev_), h_(o.h_), n_vertices_(o.n_vertices_) { o.h_ = nullptr; }
    swr_mesh* handle() const { return h_; }
    int VertexCount() const { return n_vertices_; }
    Vector4 SphereBounds() const { Vector4 o{}; dev_.check(swr_mesh_bounds(dev_.ctx(), h_, o.data())); return o; }   // ModelLoader.cs:291
    // a deform target: this mesh's vertices and indices copied on the GPU
    Mesh Like() const { Mesh m(dev_, n_vertices_); dev_.check(swr_mesh_create_like(dev_.ctx(), h_, &m.h_)); return m; }
    // the vertices as the device holds them (flushes nothing)
    std::vector<Shaders::VertexInput> Read() const {
        std::vector<Shaders::VertexInput> out((size_t)n_vertices_);
        dev_.check(swr_mesh_readback(dev_.ctx(), h_, out.data()));
        return out;
    }
    // vertices = a * (1 - t) + b * t, every scalar, in the build's Lerp model; t is not clamped
    void BlendFrom(const Mesh& a, const Mesh& b, float t) { dev_.check(swr_mesh_blend(dev_.ctx(), h_, a.h_, b.h_, t)); }
    // four joint indices and four weights per vertex, retained; two empty vectors remove them
    void SetSkin(const std::vector<uint16_t>& joints4, const std::vector<float>& weights4) {
        if (joints4.empty() && weights4.empty() && n_vertices_ > 0) { dev_.check(swr_mesh_set_skin(dev_.ctx(), h_, nullptr, nullptr)); return; }
        if (joints4.size() != 4 * (size_t)n_vertices_ || weights4.size() != 4 * (size_t)n_vertices_)
            throw std::invalid_argument("joints4 and weights4 must hold four entries per vertex");
        static const uint16_t no_joint = 0; static const float no_weight = 0.0f;              // (a mesh without vertices: valid pointers)
        dev_.check(swr_mesh_set_skin(dev_.ctx(), h_, joints4.empty() ? &no_joint : joints4.data(), weights4.empty() ? &no_weight : weights4.data()));
    }
    // vertices = src's, skinned by `palette` (glTF's jointMatrix per joint, row-major for row vectors) with src's skin attributes
    void SkinFrom(const Mesh& src, const std::vector<Matrix4x4>& palette) {
        dev_.check(swr_mesh_skin(dev_.ctx(), h_, src.h_, palette.empty() ? nullptr : palette[0].data(), (int)palette.size()));
    }
private:
    Mesh(const Device& dev, int n_vertices) : dev_(dev), n_vertices_(n_vertices) {}
    const Device& dev_;
    swr_mesh* h_ = nullptr;
    int n_vertices_ = 0;
};

// Skeletal animation (build-defined, include/swr.h "SKELETAL ANIMATION"): a skeleton with its clips, sampled on the GPU into a pose
// set -- one palette per instance of a crowd -- that Device::SkinBatch skins every mesh of the crowd from in one launch.
struct AnimationChannel {                      // one glTF animation channel with its sampler
    int node = 0;
    int path = SWR_ANIM_PATH_TRANSLATION;      // SWR_ANIM_PATH_*
    int interpolation = SWR_ANIM_LINEAR;       // SWR_ANIM_STEP | SWR_ANIM_LINEAR (CUBICSPLINE is refused)
    std::vector<float> times;                  // n_keys, non-decreasing
    std::vector<float> values;                 // n_keys x 3 (x 4 for a rotation, xyzw)
};
using PoseRequest = swr_pose_request;          // { clip_a, time_a, clip_b (-1: none), time_b, weight }

class Skeleton {
public:
    // parent[i] < i or -1; restLocal one Matrix4x4 per node; restT / restS 3 floats per node, restR 4 (xyzw); jointNode the node each
    // joint is, inverseBind one Matrix4x4 per joint
    Skeleton(const Device& dev, const std::vector<int32_t>& parent, const std::vector<Matrix4x4>& restLocal, const std::vector<float>& restT,
             const std::vector<float>& restR, const std::vector<float>& restS, const std::vector<int32_t>& jointNode,
             const std::vector<Matrix4x4>& inverseBind)
        : dev_(dev), n_nodes_((int)parent.size()), n_joints_((int)jointNode.size()) {
        const size_t n = parent.size();
        if (restLocal.size() != n || restT.size() != 3 * n || restR.size() != 4 * n || restS.size() != 3 * n || inverseBind.size() != jointNode.size())
            throw std::invalid_argument("the skeleton's arrays do not match its node and joint counts");
        dev_.check(swr_skeleton_create(dev_.ctx(), (int)n, parent.data(), n ? restLocal[0].data() : nullptr, restT.data(), restR.data(), restS.data(),
                                       n_joints_, jointNode.data(), n_joints_ ? inverseBind[0].data() : nullptr, &h_));
    }
    ~Skeleton() { if (h_) swr_skeleton_destroy(dev_.ctx(), h_); }
    Skeleton(const Skeleton&) = delete;
    Skeleton& operator=(const Skeleton&) = delete;
    swr_skeleton* handle() const { return h_; }
    int NodeCount() const { return n_nodes_; }
    int JointCount() const { return n_joints_; }
    // the clip's index; a load-time call (it may wait for the device)
    int AddClip(const std::vector<AnimationChannel>& channels) {
        std::vector<swr_anim_channel> recs;
        for (const AnimationChannel& c : channels) {
            if (c.values.size() != c.times.size() * (c.path == SWR_ANIM_PATH_ROTATION ? 4u : 3u))
                throw std::invalid_argument("a channel's values must hold 3 floats per key (4 for a rotation)");
            recs.push_back(swr_anim_channel{ c.node, c.path, c.interpolation, (int32_t)c.times.size(), c.times.data(), c.values.data() });
        }
        int index = -1;
        dev_.check(swr_skeleton_add_clip(dev_.ctx(), h_, recs.data(), (int)recs.size(), &index));
        return index;
    }
private:
    const Device& dev_;
    swr_skeleton* h_ = nullptr;
    int n_nodes_ = 0, n_joints_ = 0;
};

class PoseSet {
public:
    PoseSet(const Device& dev, int nInstances, int nJoints) : dev_(dev), n_instances_(nInstances), n_joints_(nJoints) {
        dev_.check(swr_pose_set_create(dev_.ctx(), nInstances, nJoints, &h_));
    }
    ~PoseSet() { if (h_) swr_pose_set_destroy(dev_.ctx(), h_); }
    PoseSet(const PoseSet&) = delete;
    PoseSet& operator=(const PoseSet&) = delete;
    swr_pose_set* handle() const { return h_; }
    int InstanceCount() const { return n_instances_; }
    int JointCount() const { return n_joints_; }
    // instance i from requests[i], sampled and composed on the GPU; no host wait
    void Sample(const Skeleton& skeleton, const std::vector<PoseRequest>& requests) {
        dev_.check(swr_pose_set_sample(dev_.ctx(), h_, skeleton.handle(), requests.data(), (int)requests.size()));
    }
    // host-made palettes into instances first .. first + palettes.size() / JointCount() - 1; no host wait
    void Upload(int first, const std::vector<Matrix4x4>& palettes) {
        if (palettes.size() % (size_t)n_joints_) throw std::invalid_argument("palettes must hold JointCount() matrices per instance");
        dev_.check(swr_pose_set_upload(dev_.ctx(), h_, first, (int)(palettes.size() / (size_t)n_joints_), palettes.empty() ? nullptr : palettes[0].data()));
    }
    // InstanceCount() x JointCount() matrices as the device holds them
    std::vector<Matrix4x4> Read() const {
        std::vector<Matrix4x4> out((size_t)n_instances_ * (size_t)n_joints_);
        dev_.check(swr_pose_set_readback(dev_.ctx(), h_, out[0].data()));
        return out;
    }
private:
    const Device& dev_;
    swr_pose_set* h_ = nullptr;
    int n_instances_ = 0, n_joints_ = 0;
};

inline void Device::SkinBatch(const std::vector<Mesh*>& dsts, const std::vector<const Mesh*>& srcs, const PoseSet& set,
                              const std::vector<int32_t>& instances) const {
    if (srcs.size() != dsts.size() || instances.size() != dsts.size()) throw std::invalid_argument("dsts, srcs and instances must have equal lengths");
    std::vector<swr_mesh*> d;
    std::vector<const swr_mesh*> s;
    for (const Mesh* m : dsts) d.push_back(m ? m->handle() : nullptr);
    for (const Mesh* m : srcs) s.push_back(m ? m->handle() : nullptr);
    check(swr_mesh_skin_batch(ctx_, (int)d.size(), d.data(), s.data(), set.handle(), instances.data()));
}

class Rasterizer {                            // public static class Rasterizer, Rasterizer.cs:12
public:
    enum class DebugMode { None = 0, Wireframe = 1 };                                              // :14-18
    enum class BlendMode { None = 0, Alpha = 1, Additive = 2, Multiply = 3 };                      // :25-31
    enum class DepthTest { Disabled = 0, Less, LessEqual, Greater, GreaterEqual, Equal, NotEqual, Always };   // :33-43
    enum class CullMode { None = 0, Back = 1, Front = 2 };                                         // :45-50
    static inline float NearClip = 0.1f;                                                           // :20
    static inline float FarClip = 1000.0f;                                                         // :21
    static inline DebugMode RenderDebugMode = DebugMode::None;                                     // :22

    static void InitializeTileLocks(const MainWindow& w, int width, int height) {                  // :69-93
        w.device().check(swr_initialize_tile_locks(w.device().ctx(), width, height));
    }
    // Rasterizer.RenderMesh, Rasterizer.cs:163-174 (same defaults)
    static void RenderMesh(MainWindow& window, const std::vector<Shaders::VertexInput>& vertices,
                           const std::vector<uint16_t>& indices, const Matrix4x4& model, const Matrix4x4& view,
                           const Matrix4x4& projection, const ShaderProgram& shader,
                           CullMode cullMode = CullMode::Back, DepthTest depthTest = DepthTest::LessEqual,
                           BlendMode blendMode = BlendMode::Alpha) {
        const Device& d = window.device();
        d.check(swr_set_state(d.ctx(), NearClip, FarClip, (int)RenderDebugMode));
        if ((int)shader.program >= SWR_PROG_USER_BASE) {
            d.SetProgramConstants((int)shader.program, shader.constants);
            for (int k = 1; k < SWR_PROGRAM_TEXTURES; ++k) d.SetProgramTexture((int)shader.program, k, shader.textures[k - 1]);
        }
        d.check(swr_render_mesh_arrays(d.ctx(), vertices.data(), (int)vertices.size(), indices.data(), (int)indices.size(),
                                       model.data(), view.data(), projection.data(), (int)shader.program, &shader.uniforms,
                                       shader.texture ? shader.texture->handle() : nullptr,
                                       (int)cullMode, (int)depthTest, (int)blendMode));
    }
    // ... from a retained mesh (no per-draw upload; a deformed mesh is drawn in its pose)
    static void RenderMesh(MainWindow& window, const Mesh& mesh, const Matrix4x4& model, const Matrix4x4& view,
                           const Matrix4x4& projection, const ShaderProgram& shader,
                           CullMode cullMode = CullMode::Back, DepthTest depthTest = DepthTest::LessEqual,
                           BlendMode blendMode = BlendMode::Alpha) {
        const Device& d = window.device();
        d.check(swr_set_state(d.ctx(), NearClip, FarClip, (int)RenderDebugMode));
        if ((int)shader.program >= SWR_PROG_USER_BASE) {
            d.SetProgramConstants((int)shader.program, shader.constants);
            for (int k = 1; k < SWR_PROGRAM_TEXTURES; ++k) d.SetProgramTexture((int)shader.program, k, shader.textures[k - 1]);
        }
        d.check(swr_render_mesh(d.ctx(), mesh.handle(), model.data(), view.data(), projection.data(), (int)shader.program, &shader.uniforms,
                                shader.texture ? shader.texture->handle() : nullptr, (int)cullMode, (int)depthTest, (int)blendMode));
    }
};

}  // namespace SoftwareRenderer
