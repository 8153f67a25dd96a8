/*
 * swr.h -- C ABI of the MI355X-native rasterizer backend (libswr_hip.so).
 *
 * Drop-in boundary for the raster hot path of OCSYT/SoftwareRenderer.  The
 * reference has no FFI of its own: the C# host calls
 * `Rasterizer.RenderMesh` directly with delegates and a MainWindow object.  Each
 * entry point below names the reference interface it replaces (file:line under
 * the C# repo); INTEGRATION.md shows the P/Invoke stub a maintainer would add.
 *
 * Conventions
 *  - plain pointers and sizes only; no C++/torch types; every function returns an
 *    int status (SWR_OK = 0, negative = error) and never unwinds across the ABI.
 *    swr_last_error() gives the text of the last failure on that context.
 *  - matrices are 16 floats M11..M44, row-major, row-vector convention
 *    (v' = v * M) exactly as System.Numerics.Matrix4x4 is laid out in memory.
 *  - caller owns every input array for the duration of the call; retained meshes
 *    and textures are copied to HBM and owned by the context until destroyed.
 *  - draw calls are RECORDED in submission order under a context mutex and
 *    executed on the GPU at swr_flush / swr_readback / any accessor that needs
 *    pixels, so concurrent callers (Renderer.cs:444 Parallel.ForEach) are safe and
 *    the result equals the serial schedule mesh 0,1,2... triangle 0,1,2...
 *  - one context drives one GPU (one process per GPU); for multi-GPU frames each
 *    rank owns a band of 16-pixel tile rows (swr_set_band) and the host gathers
 *    the colour bands (RCCL) -- see softwarerenderer_amd/multigpu.py.
 *  - there is NO CPU fallback: without a usable HIP device swr_create fails.
 */
#ifndef SWR_H
#define SWR_H

#ifndef __HIPCC_RTC__
#include <stdint.h>
#include <stddef.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define SWR_ABI_VERSION 3     /* 2: swr_bind_framebuffer no longer drains (lifetime rule below); swr_resize / swr_set_band* are no-ops when
                               * nothing changes; new: swr_sync_count, swr_build_info, swr_numerics_mode, swr_present_rgb_async / swr_present_wait
                               * 3: frames in flight (swr_set_pipelining / swr_get_pipelining, on by default); swr_set_transform_fma;
                               *    one batch holds fewer than 2^26 vertex-stage records (see swr_render_mesh) */

/* status codes */
#define SWR_OK                 0
#define SWR_ERR_INVALID_ARG   (-1)  /* C#: ArgumentException (Rasterizer.cs:71-74) / IndexOutOfRangeException */
#define SWR_ERR_HIP           (-2)  /* a HIP runtime call failed */
#define SWR_ERR_OOM           (-3)  /* hipMalloc failed */
#define SWR_ERR_NO_DEVICE     (-4)  /* no gfx950 device / runtime missing */
#define SWR_ERR_UNSUPPORTED   (-5)
#define SWR_STALE              1    /* swr_present_wait only (not an error): the copied frame predates a replayed batch, present again */

/* Rasterizer.DebugMode, Rasterizer.cs:14-18 */
enum { SWR_DEBUG_NONE = 0, SWR_DEBUG_WIREFRAME = 1 };
/* Rasterizer.BlendMode, Rasterizer.cs:25-31 */
enum { SWR_BLEND_NONE = 0, SWR_BLEND_ALPHA = 1, SWR_BLEND_ADDITIVE = 2, SWR_BLEND_MULTIPLY = 3 };
/* Rasterizer.DepthTest, Rasterizer.cs:33-43 */
enum { SWR_DEPTH_DISABLED = 0, SWR_DEPTH_LESS = 1, SWR_DEPTH_LESSEQUAL = 2, SWR_DEPTH_GREATER = 3,
       SWR_DEPTH_GREATEREQUAL = 4, SWR_DEPTH_EQUAL = 5, SWR_DEPTH_NOTEQUAL = 6, SWR_DEPTH_ALWAYS = 7 };
/* Rasterizer.CullMode, Rasterizer.cs:45-50 */
enum { SWR_CULL_NONE = 0, SWR_CULL_BACK = 1, SWR_CULL_FRONT = 2 };

/* Built-in shader programs: C# delegates (Shaders.cs:97-98) cannot cross the ABI, so a
 * program id selects a (vertex, fragment) pair compiled into the backend. */
enum {
    SWR_PROG_FLAT_COLOR = 0,        /* VS of Renderer.cs:830-846 with Interpolate=false; FS = input.Color */
    SWR_PROG_GOURAUD = 1,           /* same VS, Interpolate=true; FS = input.Color */
    SWR_PROG_DUST2_LAMBERT_FOG = 2, /* exactly Renderer.VertexShader/FragmentShader, Renderer.cs:830-860 */
    SWR_PROG_PHONG_4POINT = 3,      /* build-defined 4-point-light Phong (no reference semantics) */
    SWR_PROG_DEBUG_VARYINGS = 4     /* build-defined: FS returns the varyings of Shaders.VertexOutput that no other built-in reads, as
                                     * Rasterizer.Interpolate delivers them -- (ScreenCoords.x + Normal.x, ScreenCoords.y + Normal.y,
                                     * Barycentric.x + Normal.z, Barycentric.y + 0.5); Rasterizer.cs:390,598-613,638 */
};
/* USER programs (any Shaders.FragmentShader delegate, optionally with any Shaders.VertexShader delegate, restated in C++):
 * swr_program_create / swr_program_create_vf compile one at run time into the raster kernel (and a vertex kernel) and return an
 * id >= SWR_PROG_USER_BASE, which the render calls accept as `program`. */
#define SWR_PROG_USER_BASE 256

/* Shaders.VertexInput, Shaders.cs:10-24 -- 48 bytes, identical memory layout */
typedef struct swr_vertex {
    float position[3];
    float uv[2];
    float normal[3];
    float color[4];
} swr_vertex;

typedef struct swr_point_light {      /* subset of Light.cs:9-17 used by PHONG_4POINT */
    float position[3]; float range;
    float color[3];    float intensity;
} swr_point_light;

/* Uniform block: the fields Renderer.FragmentShader closes over, Renderer.cs:39-44 */
typedef struct swr_uniforms {
    float light_direction[3]; float _pad0;
    float light_color[4];
    float fog_color[4];
    float fog_start, fog_end;
    float shininess; float _pad1;
    float camera_position[3]; float _pad2;
    swr_point_light lights[4];
} swr_uniforms;

typedef struct swr_stats {            /* counters for the last flushed batch and totals since reset */
    uint64_t triangles_in;            /* index triples submitted to RenderMesh */
    uint64_t triangles_setup;         /* triangles that reached the tile loop (after clip/cull/reject) */
    uint64_t triangles_clipped;       /* went through the near-plane clipper */
    uint64_t fragments_tested;        /* passed coverage (Rasterizer.cs:493-496) */
    uint64_t fragments_shaded;        /* passed the depth test */
    uint64_t fragments_written;       /* passed alpha, pixel written (Rasterizer.cs:511-519) */
    uint64_t tile_pairs;              /* (triangle, 16x16 tile) pairs binned */
    uint64_t flushes;
} swr_stats;

/* per-stage GPU time of flushes since swr_profile_reset, from hipEvents on the context's stream */
typedef struct swr_profile {
    double vertex_ms, setup_ms, bin_ms, sort_ms, cover_ms, raster_ms, clear_ms, total_ms;
    uint64_t raster_launches, flushes;
} swr_profile;

typedef struct swr_context swr_context;
typedef struct swr_mesh swr_mesh;
typedef struct swr_texture swr_texture;

int  swr_abi_version(void);
/* Identity of this build: "hipcc=<compiler version>; csrc_sha256=<hash of the kernel sources>; fma=<0|1>; dot=<0|1|2>; extra=<extra
 * compile switches, empty for the product>".
 * The lane-to-lane LDS hand-offs of k_cover / k_raster_c are verified per compiler + source pair: the
 * pair the parity sweeps ran on is committed in profiles/verified_build.json and tests/test_gpu_api.py compares. */
const char* swr_build_info(void);
/* The System.Numerics model this library was compiled with (the reference's .NET 9 SIMD paths are not pinned by anything in
 * its repository): *fma = 1 when Vector4.Lerp (Shaders.cs:52-55, Renderer.cs:858) is modelled with fused
 * multiply-adds (SWR_NUMERICS_FMA), *dot_order = summation order of Vector3.Dot / LengthSquared (SWR_DOT_PAIRWISE: 0 sequential,
 * 1 dpps, 2 shuffle-adds).  csharp/RasterizerNative.cs probes the running .NET at start-up and loads the library that matches. */
int  swr_numerics_mode(int* fma, int* dot_order);
const char* swr_last_error(const swr_context* ctx);   /* ctx may be NULL: last swr_create failure */

/* lifetime -------------------------------------------------------------------------------- */
int  swr_create(int device_id, swr_context** out);
/* The other half of the System.Numerics model, per context and at run time (it only touches the vertex stage and the frustum
 * test): whether Vector4.Transform / Vector3.Transform / Matrix4x4.Multiply (Renderer.cs:832-834, FrustumCuller.cs:203,213) and
 * Vector3.TransformNormal (Renderer.cs:835) fuse their multiply-adds.  Default: both = the library's compile-time *fma.  Draws
 * recorded before the call keep the model they were recorded under.  The C# start-up probe sets it from what it observes, so
 * every (Transform, TransformNormal, Lerp, Dot) combination a .NET runtime can show is served by one of the six libraries. */
int  swr_set_transform_fma(swr_context* ctx, int transform_fused, int transform_normal_fused);
int  swr_get_transform_fma(swr_context* ctx, int* transform_fused, int* transform_normal_fused);
void swr_destroy(swr_context* ctx);

/* framebuffer == MainWindow.ColorBuffer / DepthBuffer (MainWindow.cs:25-31) ------------------ */
/* allocates Vector4[W*H] + float[W*H] in HBM; ≙ MainWindow.HandleResize (MainWindow.cs:320-321).
 * W or H <= 0 gives a zero-size target on which every draw is silently skipped (Rasterizer.cs:176). */
int  swr_resize(swr_context* ctx, int width, int height);
/* multi-GPU: this context renders only tile rows [first_tile_row, first_tile_row + n_tile_rows) of the
 * W x H frame; its buffers hold just those rows.  Default = whole frame. */
int  swr_set_band(swr_context* ctx, int first_tile_row, int n_tile_rows);
/* multi-GPU, interleaved variant (load balance for clustered scenes): the frame's tile rows are cut into stripes of
 * `stripe_tile_rows` rows and stripe s belongs to rank s % world; this context renders rank's stripes and its buffers hold them
 * one after the other in ascending order (16 pixel rows per tile row).  swr_set_band returns to a contiguous band / the whole frame. */
int  swr_set_band_interleaved(swr_context* ctx, int rank, int world, int stripe_tile_rows);
/* use caller-provided device memory (e.g. a torch tensor that RCCL will gather) for the band's
 * colour (float4 per pixel) and depth (float per pixel); NULL returns to internal storage.  Draws recorded before the
 * call are launched against the buffers bound before it; the call itself does not wait for the GPU.
 * LIFETIME RULE (ABI 2): a buffer that has been bound stays referenced by the batches flushed against it until the next
 * VALIDATING call on this context (swr_sync, swr_readback*, swr_get_stats, any pixel accessor, swr_destroy): an optimistic
 * batch that did not fit its pair buffers is replayed into the buffer it was flushed against at that point.  Keep previously
 * bound buffers allocated, and do not hand their contents to a consumer as final, until such a call has returned (the caller's
 * own stream synchronisation is not enough).  swr_replay_count tells whether a replay happened. */
int  swr_bind_framebuffer(swr_context* ctx, void* color_device_ptr, void* depth_device_ptr);
int  swr_set_stream(swr_context* ctx, void* hip_stream);      /* hipStream_t; NULL = context's own stream */
int  swr_clear_color(swr_context* ctx, const float rgba[4]);   /* MainWindow.ClearColorBuffer, MainWindow.cs:400-407 */
int  swr_clear_depth(swr_context* ctx);                        /* MainWindow.ClearDepthBuffer -> float.MinValue, :429-436 */
int  swr_get_pixel(swr_context* ctx, int x, int y, float rgba[4]);       /* MainWindow.GetPixel :391-398 (OOB -> 0) */
int  swr_set_pixel(swr_context* ctx, int x, int y, const float rgba[4]); /* MainWindow.SetPixel :382-388 (OOB ignored) */
int  swr_get_depth(swr_context* ctx, int x, int y, float* depth);        /* MainWindow.GetDepth :420-426 (OOB -> MinValue) */
int  swr_set_depth(swr_context* ctx, int x, int y, float depth);         /* MainWindow.SetDepth :411-417 */
/* flush, then copy the band into caller memory (either pointer may be NULL); ≙ the host reading
 * ColorBuffer/DepthBuffer in MainWindow.OnRender (MainWindow.cs:226-263) */
int  swr_readback(swr_context* ctx, float* color_rgba, float* depth);
/* flush, then copy the colour band as packed RGB floats (12 B per pixel): the Vector4 -> Vector3 flatten of
 * MainWindow.OnRender (MainWindow.cs:234-240) done on the GPU, ready for glTexSubImage2D(RGB, FLOAT) */
int  swr_readback_rgb(swr_context* ctx, float* rgb);
/* ASYNCHRONOUS PRESENT (the read-back of a 4096 x 4096 frame takes 7 x as long as rendering it): flatten on the
 * GPU behind the recorded draws and copy the band's RGB floats into `rgb` WITHOUT waiting -- the copy runs on a second stream of the
 * context, so the next frame renders while this one crosses PCIe; two device staging buffers alternate, i.e. two presents may be
 * in flight (a third first waits for the oldest).  `rgb` should be page-locked (swr_host_register) and must stay untouched until
 * swr_present_wait(ticket) returns: SWR_OK = rgb holds the frame; SWR_STALE (1) = an optimistic batch was replayed meanwhile, the
 * pixels predate it: present the frame again.  ≙ MainWindow.OnRender's upload of flatColorBuffer (MainWindow.cs:226-263), double
 * buffered: a host loop `render i+1; present_async(i+1); wait(i); upload i` costs max(render, copy) per frame, not their sum. */
int  swr_present_rgb_async(swr_context* ctx, float* rgb, uint64_t* ticket);
int  swr_present_wait(swr_context* ctx, uint64_t ticket);
/* same flatten, but into DEVICE memory supplied by the caller (band rows x W x 3 floats), enqueued after the recorded
 * draws on the context's stream and NOT synchronised: swr_sync (or the caller's own stream order) completes it.  This is
 * the present payload a multi-GPU frame gathers over xGMI (12 instead of 16 B per pixel). */
int  swr_flatten_rgb_device(swr_context* ctx, float* d_rgb);
/* The same flatten WITHOUT validating the optimistic flushes first: nothing here waits for the GPU, so a frame loop can
 * chain render -> flatten -> its own consumer (an RCCL gather, a peer-mapped store target) in stream order.  The caller
 * validates later -- swr_sync at a point where it waits anyway -- and compares swr_replay_count before / after: if it grew,
 * a batch had not fitted its pair buffers, was replayed by that swr_sync, and payloads flattened in between are stale
 * (flatten and send them again).  Steady-state frames never replay. */
int  swr_flatten_rgb_device_async(swr_context* ctx, float* d_rgb);
/* SUPERSAMPLED PRESENT (build-defined; the reference's RenderScale stops at 1, MainWindow.cs:93,313-315): render at kx x ky times the
 * window, average every kx x ky block of the band's colour plane on the GPU and deliver window-sized packed RGB floats -- the bytes
 * that leave the device fall by kx * ky.  kx, ky in {1, 2, 4, 8}, chosen independently; the render target's width must be a multiple
 * of kx and its height of ky (then every band's and stripe's rows are a multiple of ky and the concatenated band payloads are the
 * resolved frame).  Per output pixel and channel, in float32: the kx samples of each row summed as a balanced pairwise tree left to
 * right, the ky row sums by the same tree top to bottom, times the float 1 / (kx * ky); alpha is dropped; (1, 1) gives the
 * flatten's values (csrc/swr_deliver.hip.h).  Bad factors, a size that does not divide and NULL pointers:
 * SWR_ERR_INVALID_ARG, nothing written, no ticket issued.  A zero-size target: SWR_OK, nothing written. */
/* host only: the payload's size under the size and band in force, out_width = W / kx, out_rows = band rows / ky */
int  swr_resolved_size(swr_context* ctx, int kx, int ky, int* out_width, int* out_rows);
/* as swr_readback_rgb: flush, validate, resolve, copy out_rows x out_width x 3 floats into rgb, wait */
int  swr_readback_rgb_resolved(swr_context* ctx, int kx, int ky, float* rgb);
/* as swr_present_rgb_async, and sharing its two slots, tickets, staging buffers, staleness rule and back-pressure: never waits for
 * the stream; swr_present_wait serves both kinds of ticket, and the two kinds may alternate */
int  swr_present_rgb_resolved_async(swr_context* ctx, int kx, int ky, float* rgb, uint64_t* ticket);
/* as swr_flatten_rgb_device (validates first) and swr_flatten_rgb_device_async (does not wait), into out_rows x out_width x 3
 * floats of caller DEVICE memory */
int  swr_resolve_rgb_device(swr_context* ctx, int kx, int ky, float* d_rgb);
int  swr_resolve_rgb_device_async(swr_context* ctx, int kx, int ky, float* d_rgb);
/* 8-BIT PRESENT (build-defined): the payload above -- the flatten's R, G, B under kx = ky = 1, otherwise the resolve's -- quantised
 * on the GPU, so that 3 or 4 bytes per window pixel leave the device instead of 12.  Per channel c, after the resolve's arithmetic
 * has been rounded to float32: NaN -> 0; c <= 0 -> 0; c >= 1 -> 255; otherwise (uint8) rintf(c * 255.0f), the product rounded to
 * float32 and ties to even.  No gamma, no dither (the reference has neither: it hands the floats to GL, which clamps and rounds
 * them to its 8-bit framebuffer; GL prefers round-to-nearest and leaves ties open).  bpp = 3 delivers R, G, B; bpp = 4 delivers
 * R, G, B, 255.  Rows are tightly packed: out_rows x out_width x bpp contiguous bytes, and the concatenated band payloads are the
 * frame (csrc/swr_deliver.hip.h).  A bpp other than 3 or 4, bad factors, a size that does not divide and NULL
 * pointers: SWR_ERR_INVALID_ARG, nothing written, no ticket issued.  A zero-size target: SWR_OK, nothing written. */
/* host only: swr_resolved_size plus out_bytes = out_rows * out_width * bpp */
int  swr_present8_size(swr_context* ctx, int kx, int ky, int bpp, int* out_width, int* out_rows, size_t* out_bytes);
/* as swr_readback_rgb_resolved; `out` may have any alignment */
int  swr_readback_rgb8(swr_context* ctx, int kx, int ky, int bpp, uint8_t* out);
/* as swr_present_rgb_resolved_async, on the same two slots, tickets and staging buffers: the three kinds of present may alternate
 * and swr_present_wait serves every ticket; `out` may have any alignment */
int  swr_present_rgb8_async(swr_context* ctx, int kx, int ky, int bpp, uint8_t* out, uint64_t* ticket);
/* as swr_resolve_rgb_device (validates first) and its async form (does not wait), into out_bytes of caller DEVICE memory, which
 * must be 4-byte aligned (the kernel stores whole dwords): SWR_ERR_INVALID_ARG otherwise */
int  swr_resolve_rgb8_device(swr_context* ctx, int kx, int ky, int bpp, uint8_t* d_out);
int  swr_resolve_rgb8_device_async(swr_context* ctx, int kx, int ky, int bpp, uint8_t* d_out);
int  swr_replay_count(swr_context* ctx, uint64_t* out);
/* how many times an entry point has made the calling thread wait for the stream so far (hipStreamSynchronize): lets a frame
 * loop assert that its steady state never blocks (swr_bind_framebuffer, swr_flush, swr_flatten_rgb_device_async, and
 * swr_resize / swr_set_band* with unchanged arguments do not) */
int  swr_sync_count(swr_context* ctx, uint64_t* out);
/* Page-lock a long-lived host buffer (the C# side's pinned ColorBuffer / flatColorBuffer arrays) so that swr_readback /
 * swr_readback_rgb / swr_upload DMA straight into it at PCIe rate instead of going through a pageable staging copy.
 * Optional: unregistered buffers work, only slower.  Unregister before freeing the memory. */
int  swr_host_register(swr_context* ctx, void* ptr, size_t bytes);
int  swr_host_unregister(swr_context* ctx, void* ptr);
/* upload caller memory into the band (tests: resume from a known framebuffer state) */
int  swr_upload(swr_context* ctx, const float* color_rgba, const float* depth);
int  swr_color_device_ptr(swr_context* ctx, void** out);
int  swr_depth_device_ptr(swr_context* ctx, void** out);

/* retained resources -------------------------------------------------------------------------- */
/* Texture(Image<Rgba32>) ctor / Dispose, Texture.cs:31-41,65-68: RGBA8 row-major, w*h*4 bytes */
int  swr_texture_create(swr_context* ctx, const uint8_t* rgba8, int width, int height, swr_texture** out);
int  swr_texture_destroy(swr_context* ctx, swr_texture* tex);
/* BUILD-DEFINED extension (row N4): 0 = the reference's nearest filter (Texture.cs:43-63, default), 1 = bilinear with wrap
 * (formula in oracle/swr_oracle.c:oswr_texture_sample_bilinear; no reference semantics).  Applies to draws recorded later. */
int  swr_texture_set_filter(swr_context* ctx, swr_texture* tex, int bilinear);
/* Texture.Sample, Texture.cs:43-63, batched: n uv pairs -> n RGBA float4 (runs on the GPU) */
int  swr_texture_sample(swr_context* ctx, const swr_texture* tex, const float* uv, int n, float* out_rgba);
/* RENDER TO TEXTURE (build-defined: the reference has Texture over Image<Rgba32> and MainWindow's float buffers and no link between
 * them; csrc/swr_deliver.hip.h): a frame becomes a draw's texture without leaving the device -- a scope, a mirror,
 * a camera screen, a minimap, last frame's image. */
enum { SWR_TEXTURE_ALPHA_OPAQUE = 0, SWR_TEXTURE_ALPHA_KEEP = 1 };
/* a texture of zeros without host data, to be filled by swr_texture_update_from_frame; the limits of swr_texture_create */
int  swr_texture_create_target(swr_context* ctx, int width, int height, swr_texture** out);
/* Texel (x, y) of the w x h texture from src's frame of w * kx by h * ky pixels, kx, ky in {1, 2, 4, 8}: R, G, B are the bytes
 * swr_readback_rgb8(src, kx, ky, 4) delivers for output pixel (x, y); A is 255 under SWR_TEXTURE_ALPHA_OPAQUE and, under
 * SWR_TEXTURE_ALPHA_KEEP, the frame's alpha through the same pairwise tree, scale and quantiser.  src == NULL: ctx's own frame.
 * IMMEDIATE-MODE SEMANTICS, as `tex[x, y] = quantise(window.GetPixel(...))` executed at this point of the program: draws recorded
 * earlier -- flushed or not -- sample the old texels, draws recorded later the new ones; src's frame is what its draws recorded so far
 * leave.  ASYNCHRONOUS: both contexts' recorded draws are flushed, ONE kernel is enqueued on ctx's stream, and nothing waits for the GPU
 * (swr_sync_count of both contexts stays); between two contexts one event orders the kernel behind src's frame and one orders src's
 * later work behind the kernel.  The block-linear copy of a bilinear texture (swr_texture_set_filter) is written by the same kernel.
 * Reads whatever colour buffer src has bound (swr_bind_framebuffer) and honours swr_set_stream.  A texture is used with the context
 * that created it.  Like the *_device_async calls the update does not validate optimistic flushes: if swr_replay_count of src or ctx
 * grows at the next validating call, a batch in front of the update had not fitted its pair buffers and the texels were made from
 * an incomplete frame -- update (and redraw what sampled it) again; steady-state frames never replay.
 * SWR_ERR_INVALID_ARG: tex NULL, factors outside {1, 2, 4, 8}, an unknown alpha_mode, a frame that is not w * kx by h * ky.
 * SWR_ERR_UNSUPPORTED: src holds only a band of its frame (swr_set_band*), or lives on another device.  Nothing is written then and
 * the context stays usable. */
int  swr_texture_update_from_frame(swr_context* ctx, swr_texture* tex, swr_context* src, int kx, int ky, int alpha_mode);
/* the row-major texels, w * h * 4 bytes, as the kernels enqueued so far leave them; waits for the stream (screenshots, tests) */
int  swr_texture_readback(swr_context* ctx, const swr_texture* tex, uint8_t* rgba8);
/* DEPTH TEXTURES (build-defined: the reference has no link between MainWindow's depth floats and a Texture; csrc/swr_deliver.hip.h,
 * csrc/swr_device.h): a frame's depth plane becomes a texture a later draw, of this or another camera, can
 * compare against -- cast shadows, depth-tested decals, soft particles.  A depth texture is an swr_texture whose 4-byte texels are
 * float32 depth words, exactly as the raster stage stores them (float.MinValue = nothing drawn; larger = nearer under LessEqual).
 * The format is fixed at creation.  What the calls above do with a depth texture:
 *   swr_texture_set_filter   works: the switch between one-tap and 2 x 2 shadow lookups (swr_shadow below); makes the block-linear copy
 *                            under its usual rule, and swr_texture_update_from_depth writes that copy in the same pass
 *   swr_texture_destroy      works
 *   swr_program_set_texture, swr_post_set_texture, a render call's texture   accepted: the colour samplers (swr_sample, swr_texel) then
 *                            read the float's four bytes as R, G, B, A -- defined and memory-safe, rarely useful
 *   swr_texture_update_from_frame / _from_post, swr_texture_readback, swr_texture_sample   SWR_ERR_INVALID_ARG with a message, nothing
 *                            written, the context usable
 * and the *_depth calls below answer an RGBA8 texture the same way. */
enum { SWR_TEXTURE_FORMAT_RGBA8 = 0, SWR_TEXTURE_FORMAT_DEPTH32F = 1 };
/* How the kx x ky depth words of a texel's block become one: a balanced pairwise tree over the kx adjacent words of each row, left to
 * right, then the same tree over the ky row results, top to bottom (the shape of the colour resolve), of the select
 *   MAX    pick(a, b) = b > a ? b : a    the block's nearest sample under the default LessEqual test (new >= old passes)
 *   MIN    pick(a, b) = b < a ? b : a
 *   FIRST  pick(a, b) = a                the top-left sample, the word swr_post_depth reads
 * The result is one of the block's own words, bit for bit: a NaN on the left stays and one on the right is never taken; of +0 and -0
 * the left one stays.  Under (1, 1) all three copy the plane. */
enum { SWR_DEPTH_REDUCE_MAX = 0, SWR_DEPTH_REDUCE_MIN = 1, SWR_DEPTH_REDUCE_FIRST = 2 };
/* w x h float32 depth words, row-major; NULL: every texel float.MinValue (a 32-bit fill on the context's stream).  The limits and
 * codes of swr_texture_create. */
int  swr_texture_create_depth(swr_context* ctx, const float* depth_or_null, int width, int height, swr_texture** out);
/* Texel (x, y) of the w x h depth texture from the depth plane of src's frame of w * kx by h * ky pixels, reduced as above; no scale,
 * no quantiser.  Everything else is swr_texture_update_from_frame's contract with the depth plane in the colour plane's place:
 * immediate-mode semantics, both contexts' recorded draws flushed, ONE kernel on ctx's stream, nothing waits for the GPU, two events
 * between two contexts, the block-linear copy written by the same kernel, whatever depth buffer src has bound (16-byte aligned: the
 * kernel loads kx words at once), and no validation of optimistic flushes -- if swr_replay_count of src or ctx grows at the next
 * validating call, update (and redraw what sampled the texture) again; steady-state frames never replay.
 * SWR_ERR_INVALID_ARG: tex NULL, an unknown reduce, a texture that is not DEPTH32F, factors outside {1, 2, 4, 8}, a frame that is not
 * w * kx by h * ky, a misaligned bound depth buffer.  SWR_ERR_UNSUPPORTED: src holds only a band of its frame, or lives on another
 * device.  Nothing is written then and the context stays usable. */
int  swr_texture_update_from_depth(swr_context* ctx, swr_texture* tex, swr_context* src, int kx, int ky, int reduce);
/* the row-major depth words, w * h floats, as the kernels enqueued so far leave them; waits for the stream */
int  swr_texture_readback_depth(swr_context* ctx, const swr_texture* tex, float* out);
/* The device lookups of a depth texture (csrc/swr_device.h), batched, with the texture's filter as it is now: n triples (u, v, ref)
 * -> n pairs (texture_slot_depth_sample(u, v), texture_slot_shadow(u, v, ref)); runs on the GPU and waits for it. */
int  swr_texture_sample_depth(swr_context* ctx, const swr_texture* tex, const float* uv_ref, int n, float* out_depth_shadow);
/* SWR_TEXTURE_FORMAT_* of any texture */
int  swr_texture_format(swr_context* ctx, const swr_texture* tex, int* format);
/* MIP CHAINS (build-defined: the reference's Texture is one level, Texture.cs:31-41; csrc/swr_deliver.hip.h, csrc/swr_device.h,
 * DESIGN.md section 26): an RGBA8 texture -- uploaded, a render target, a pass's result -- gets the levels that let a user or post
 * program sample it minified without aliasing.  A chain has L = 1 + floor(log2(max(w, h))) levels; level l measures max(1, w >> l) by
 * max(1, h >> l).  Texel (x, y) of level l + 1 is, per byte channel, (p(2x, 2y) + p(x1, 2y) + p(2x, y1) + p(x1, y1) + 2) >> 2 over level
 * l with x1 = min(2x + 1, w_l - 1), y1 = min(2y + 1, h_l - 1): a 2 x 2 box that rounds half up; an odd side >= 3 drops its last column
 * or row.  The built-in programs and swr_sample never read a level other than 0.
 * swr_texture_generate_mipmaps has swr_texture_update_from_frame's immediate-mode semantics: the context's recorded draws are flushed
 * first and sample the texture as it was (one level, or the old levels); then the chain's record and the downsample kernels go onto
 * ctx's stream; nothing waits for the GPU (swr_sync_count does not move).  The levels' memory is allocated by the first call and kept.
 * From then on the chain is a property of the texture: swr_texture_update_from_frame / _from_post regenerate it in the same call,
 * behind the update kernel, still without a host wait.  A texture never given a chain is updated exactly as before.  A 1 x 1 texture
 * has a chain of one level: SWR_OK.  SWR_ERR_INVALID_ARG, nothing written, the context usable: tex NULL; a depth texture
 * (hierarchical depth is out of scope -- the four calls below that read texels refuse one too, swr_texture_levels answers 1). */
int  swr_texture_generate_mipmaps(swr_context* ctx, swr_texture* tex);
/* host only: 1, or L once the chain exists */
int  swr_texture_levels(swr_context* ctx, const swr_texture* tex, int* levels);
/* host only: the size of any level 0 .. L - 1 of the FULL chain, generated or not; another level: SWR_ERR_INVALID_ARG */
int  swr_texture_level_size(swr_context* ctx, const swr_texture* tex, int level, int* width, int* height);
/* the row-major texels of a level the texture HAS (0 .. levels - 1; another: SWR_ERR_INVALID_ARG), as the kernels enqueued so far leave
 * them; level 0 is swr_texture_readback; waits for the stream */
int  swr_texture_readback_level(swr_context* ctx, const swr_texture* tex, int level, uint8_t* rgba8);
/* The device lookups of a chain (csrc/swr_device.h; the program-side names are below), batched, through the texture as it is now --
 * filter and block-linear copy included; they run on the GPU and wait for it.  n < 0 or a NULL pointer: SWR_ERR_INVALID_ARG.
 *   swr_texture_sample_lod   n x (u, v, lod) -> n x RGBA: swr_sample_lod.  On a texture without a chain every lod gives level 0
 *   swr_texture_lod          n x (dudx, dvdx, dudy, dvdy) -> n lods: swr_lod */
int  swr_texture_sample_lod(swr_context* ctx, const swr_texture* tex, const float* uv_lod, int n, float* out_rgba);
int  swr_texture_lod(swr_context* ctx, const swr_texture* tex, const float* grads, int n, float* out_lod);
/* CUBE MAPS (build-defined: the reference addresses a texture by uv and clears to one colour, Renderer.cs:413; csrc/swr_device.h,
 * DESIGN.md section 27): six square faces looked up by a DIRECTION -- a skybox, a reflection, a point light's shadow.  A cube of side n
 * IS a texture n wide and 6 n high: face f (0..5 = +X, -X, +Y, -Y, +Z, -Z) occupies rows [f n, (f + 1) n), in either format.  Every
 * other call on it -- readback, set_filter, format, destroy, binding to a draw, a program or a post slot, swr_sample, swr_texel -- sees
 * that n x 6 n texture.  The block-linear copy follows its rule (made when n % 4 == 0; face f starts f n^2 texels into it as well).
 * The lookup (texture_cube_face, csrc/swr_device.h), ax = |x|, ay = |y|, az = |z|: any NaN or Inf, or all three zero: face 0,
 * s = t = 0.5.  Else X major when ax >= ay && ax >= az (ma = ax, face = x < 0 ? 1 : 0, sc = x < 0 ? -z : z, tc = -y); else Y major when
 * ay >= az (ma = ay, face = y < 0 ? 3 : 2, sc = x, tc = y < 0 ? z : -z); else Z major (ma = az, face = z < 0 ? 5 : 4,
 * sc = z < 0 ? x : -x, tc = -y); -0 counts as positive.  s = (sc / ma + 1) / 2, t = (tc / ma + 1) / 2, exactly 0 or 1 on an edge.
 * A right-handed world seen from inside: face f is the image of a camera along the face's axis with up +Y (+Y: up +Z, -Y: up -Z)
 * under the screen mapping of Rasterizer.cs:383-386 -- swr_cube_face_view is that camera.
 * Nearest filter: texel (min((int)(s n), n - 1), min((int)(t n), n - 1)) of the face.  Bilinear: X = s n - 0.5, x0 = floor(X),
 * fx = X - x0, taps x0 and x0 + 1 each CLAMPED to [0, n - 1], y likewise, blended as swr_sample blends: the footprint stays inside the
 * face.  Filtering across face edges is out of scope: a seam of up to one texel of clamped colour is the defined result.
 * rgba8 / depth: six faces of n x n, face-major (NULL: zeros, or float.MinValue).  n < 1, or 6 n^2 >= 2^30: SWR_ERR_INVALID_ARG. */
int  swr_texture_create_cube(swr_context* ctx, const uint8_t* rgba8_or_null, int n, swr_texture** out);
int  swr_texture_create_cube_depth(swr_context* ctx, const float* depth_or_null, int n, swr_texture** out);
/* host only: n of a texture created by the two calls above, 0 of any other */
int  swr_texture_is_cube(swr_context* ctx, const swr_texture* tex, int* n_or_0);
/* One face from a frame, a frame's depth or a post pass: swr_texture_update_from_frame / _from_depth / _from_post with the face's
 * n x n texels as the destination -- the same kernels, the same arguments otherwise, the same contract: one kernel on ctx's stream, no
 * host wait (swr_sync_count does not move), immediate-mode order against the draws around it, two events between two contexts; a
 * cube with a mip chain has it regenerated in the same call.  The frame must measure n kx by n ky.  SWR_ERR_INVALID_ARG, nothing
 * written, the context usable: tex NULL; not a cube; face outside 0 .. 5; the other format; factors outside {1, 2, 4, 8}; a frame of
 * another size; and what the whole-texture calls refuse.  SWR_ERR_UNSUPPORTED: a source that holds a band, or on another device. */
int  swr_texture_update_face_from_frame(swr_context* ctx, swr_texture* tex, int face, swr_context* src, int kx, int ky, int alpha_mode);
int  swr_texture_update_face_from_depth(swr_context* ctx, swr_texture* tex, int face, swr_context* src, int kx, int ky, int reduce);
int  swr_texture_update_face_from_post(swr_context* ctx, swr_texture* tex, int face, swr_context* src, int post_id, int kx, int ky, int alpha_mode);
/* one face of a level the cube has (0 .. levels - 1), (n >> level)^2 RGBA8 texels or depth words, row-major; waits for the stream */
int  swr_texture_readback_face(swr_context* ctx, const swr_texture* tex, int face, int level, void* out);
/* host only, no context: Matrix4x4.CreateLookAt(eye, eye + axis, up) of face's camera, float32, row-major as the draw calls take it.
 * With CreatePerspectiveFieldOfView(pi / 2, 1, near, far) the pixel whose centre lies in direction d from eye is the texel the lookup
 * names for d.  face outside 0 .. 5 or a NULL pointer: SWR_ERR_INVALID_ARG */
int  swr_cube_face_view(int face, const float eye[3], float view[16]);
/* The device lookups, batched, through the texture as it is now; they run on the GPU and wait for it.
 *   swr_texture_cube_face          n x (x, y, z) -> n faces, n x (s, t)
 *   swr_texture_sample_cube        n x (x, y, z, lod) -> n x RGBA: swr_sample_cube_lod (lod 0: swr_sample_cube); an RGBA8 cube
 *   swr_texture_sample_cube_depth  n x (x, y, z, ref) -> n x (word, shadow): swr_sample_cube_depth, swr_shadow_cube; a depth cube
 * MIP CHAINS: swr_texture_generate_mipmaps accepts an RGBA8 cube whose n is a power of two: L = 1 + log2(n) levels, level l the
 * (n >> l) x 6 (n >> l) atlas -- the first L levels of the n x 6 n texture's chain, since no 2 x 2 box straddles a face.
 * swr_texture_levels, _level_size and _readback_level answer for it.  Another n: SWR_ERR_UNSUPPORTED, nothing written. */
int  swr_texture_cube_face(swr_context* ctx, const float* dirs, int n, int* out_face, float* out_st);
int  swr_texture_sample_cube(swr_context* ctx, const swr_texture* tex, const float* dir_lod, int n, float* out_rgba);
int  swr_texture_sample_cube_depth(swr_context* ctx, const swr_texture* tex, const float* dir_ref, int n, float* out_depth_shadow);
/* mesh.Vertices / mesh.Indices (ModelLoader.cs:45-47): u16 indices, 3 per triangle; an index >= n_vertices
 * is SWR_ERR_INVALID_ARG (C#: IndexOutOfRangeException at Rasterizer.cs:187) */
int  swr_mesh_create(swr_context* ctx, const swr_vertex* vertices, int n_vertices,
                     const uint16_t* indices, int n_indices, swr_mesh** out);
int  swr_mesh_destroy(swr_context* ctx, swr_mesh* mesh);

/* DEFORMING MESHES (build-defined) ----------------------------------------------------------------------------
 * A retained mesh's vertices rewritten on the GPU: a blend of two key frames (Model.AnimationFrames, ModelLoader.cs:79-115; the
 * reference swaps whole frames, PlayAnimation :331-348) or linear-blend skinning by a joint palette.  The result is the mesh's own
 * swr_vertex array, so every reader follows the pose: swr_render_mesh*, swr_raycast*, swr_character_update, swr_mesh_bounds.
 * ORDER: immediate mode, as swr_texture_update_from_frame -- draws recorded before a deform see the old vertices, draws recorded after
 * it the new ones; no host wait in a loop that presents every frame.  Recorded draws are flushed first only if one of them references
 * `dst`; a batch still in flight that references `dst` (it may have to be replayed against the vertices it saw) is waited for and
 * validated before the first write.  After a deform the bounding sphere is computed again on first use.
 * SWR_ERR_INVALID_ARG, nothing written, the context usable: a NULL pointer, unequal vertex counts, `dst` being a source, a mesh of
 * another context, swr_mesh_skin on a source without skin attributes, n_joints <= the largest joint index the attributes use.
 * (A transient mesh -- the one swr_render_mesh_arrays makes per call -- is refused likewise; no call hands its handle out.)
 * SWR_ERR_UNSUPPORTED: n_joints > 65535.  A mesh without vertices: SWR_OK, nothing launched. */
/* a retained mesh with src's vertex count, its vertices and indices copied device to device: a deform target */
int  swr_mesh_create_like(swr_context* ctx, const swr_mesh* src, swr_mesh** out);
/* the n_vertices 48-byte records as the device holds them.  Flushes nothing and waits only for work that writes the mesh */
int  swr_mesh_readback(swr_context* ctx, const swr_mesh* mesh, swr_vertex* out);
/* dst = a * (1 - t) + b * t for every scalar of position, uv, normal and color: the library's Lerp model (Shaders.Lerp, fused or not as
 * the build's numerics say, swr_numerics_mode).  The normal is NOT renormalised (Renderer.VertexShader normalises the world normal): t = 0
 * and t = 1 are the identity on finite inputs, up to the sign of a zero.  Any float t, used as it is: no clamp, NaN gives NaN.  dst
 * keeps its own indices. */
int  swr_mesh_blend(swr_context* ctx, swr_mesh* dst, const swr_mesh* a, const swr_mesh* b, float t);
/* static skin attributes of a retained mesh: four joint indices and four weights per vertex, uploaded once and freed with the mesh.
 * NULL, NULL removes them (and waits for the device). */
int  swr_mesh_set_skin(swr_context* ctx, swr_mesh* src, const uint16_t* joints4, const float* weights4);
/* dst = skin(src): palette = n_joints matrices of 16 floats, row-major for row vectors (glTF's jointMatrix -- inverse bind matrix x joint
 * world x inverse mesh world -- as the caller computes it).  Per vertex, in the System.Numerics model (swr_set_transform_fma):
 *   p_k = Vector3.Transform(position, palette[j_k]), n_k = Vector3.TransformNormal(normal, palette[j_k])  for k = 0 .. 3
 *   r = w_0 * x_0, then r = w_k * x_k + r for k = 1, 2, 3 (each fused or not as the Transform / TransformNormal flag says)
 *   normal = Vector3.Normalize(r_n); uv and color are copied.
 * All four influences are evaluated (a zero weight on a matrix holding Inf gives NaN); weights are used as given, not renormalised.
 * The normal goes through the joint matrix's upper 3 x 3: right for rigid joints and uniform scale, not for a sheared or unevenly
 * scaled joint (that needs the inverse transpose, which the caller would have to supply as a second palette: not built). */
int  swr_mesh_skin(swr_context* ctx, swr_mesh* dst, const swr_mesh* src, const float* palette, int n_joints);

/* SKELETAL ANIMATION (build-defined) --------------------------------------------------------------------------
 * Clips are sampled and joint hierarchies evaluated on the GPU for a whole crowd in one call, into a POSE SET (n_instances x n_joints
 * palettes that stay on the device); every mesh of the crowd is then skinned from the set in one launch (swr_mesh_skin_batch).
 * ONE definition for every numerics build and either Transform flag: plain float32, no fused multiply-add, sums left to right.
 *   key search  times T[0 .. n-1] at time t: !(t > T[0]) gives key 0 as stored (a NaN t lands here); t >= T[n-1] gives key n-1; else
 *               k = the largest index with T[k] <= t and u = (t - T[k]) / (T[k+1] - T[k]).  STEP: key k.  LINEAR: a*(1-u) + b*u per
 *               scalar for T and S, Quaternion.Lerp(a, b, u) for R -- the NORMALISED lerp, not glTF's spherical one
 *   two clips   each of T, R, S from clip_a and clip_b (the node's rest value where a clip has no channel), combined by the same two
 *               lerps at u = weight, unclamped.  clip_b < 0: clip_a alone
 *   local       a node no channel of the request's clip(s) targets keeps its rest matrix's words; a targeted one is
 *               S x Matrix4x4.CreateFromQuaternion(R) x T
 *   hierarchy   world[i] = local[i] x world[parent[i]] (the parent's world finished first; Matrix4x4.Multiply), world = local for a
 *               root; palette[j] = inverse_bind[j] x world[node[j]]
 * Matrices are 16 floats, row-major for row vectors; quaternions are xyzw.
 * ORDER: swr_pose_set_sample, _upload and swr_mesh_skin_batch run on the stream swr_mesh_skin runs on and are ordered among themselves
 * by it alone; none waits for the device.  swr_pose_set_readback waits for the set's last write only.
 * LIMITS: n_nodes and n_joints <= 65535, n_instances x n_joints <= 2^24; beyond: SWR_ERR_UNSUPPORTED. */
typedef struct swr_skeleton swr_skeleton;
typedef struct swr_pose_set swr_pose_set;
#define SWR_ANIM_PATH_TRANSLATION 0
#define SWR_ANIM_PATH_ROTATION    1
#define SWR_ANIM_PATH_SCALE       2
#define SWR_ANIM_STEP        0
#define SWR_ANIM_LINEAR      1
#define SWR_ANIM_CUBICSPLINE 2        /* refused: SWR_ERR_UNSUPPORTED */
#define SWR_SKELETON_MAX_NODES 65535
/* n_keys >= 1 non-decreasing key times; values: n_keys x 3 floats (translation, scale) or x 4 (rotation) */
typedef struct swr_anim_channel { int32_t node, path, interpolation, n_keys; const float* times; const float* values; } swr_anim_channel;
/* instance i of a set: clip_a at time_a, blended with clip_b at time_b by weight (clip_b = -1: none) */
typedef struct swr_pose_request { int32_t clip_a; float time_a; int32_t clip_b; float time_b; float weight; } swr_pose_request;   /* 20 B */
/* parent[i] < i or -1 (several roots are allowed); rest_local n_nodes x 16, rest_t x 3, rest_r x 4, rest_s x 3; joint_node[j] is the
 * node joint j is, inverse_bind n_joints x 16.  SWR_ERR_INVALID_ARG: a NULL pointer, n_nodes < 1, n_joints < 0, a parent or a
 * joint's node out of range.  Uploads and waits: a load-time call. */
int  swr_skeleton_create(swr_context* ctx, int n_nodes, const int32_t* parent, const float* rest_local, const float* rest_t,
                         const float* rest_r, const float* rest_s, int n_joints, const int32_t* joint_node, const float* inverse_bind,
                         swr_skeleton** out);
int  swr_skeleton_destroy(swr_context* ctx, swr_skeleton* skeleton);
/* All clips of a skeleton live in one device blob, so one launch serves instances that play different clips.  Adding one may
 * reallocate the blob and wait for the device: a load-time call.  SWR_ERR_UNSUPPORTED: a CUBICSPLINE channel.  SWR_ERR_INVALID_ARG,
 * the skeleton unchanged: a node or path out of range, an unknown interpolation, two channels on one (node, path), decreasing (or
 * NaN) key times, n_keys < 1, a NULL pointer.  n_channels = 0 is a clip that leaves every node at rest. */
int  swr_skeleton_add_clip(swr_context* ctx, swr_skeleton* skeleton, const swr_anim_channel* channels, int n_channels, int* clip_index);
int  swr_pose_set_create(swr_context* ctx, int n_instances, int n_joints, swr_pose_set** out);
int  swr_pose_set_destroy(swr_context* ctx, swr_pose_set* set);
/* instance i = requests[i] for i < n <= n_instances; the other instances keep their palettes.  The set's n_joints must be the
 * skeleton's.  SWR_ERR_INVALID_ARG, nothing written: a clip index that is not a clip of the skeleton (clip_b < 0 excepted) */
int  swr_pose_set_sample(swr_context* ctx, swr_pose_set* set, const swr_skeleton* skeleton, const swr_pose_request* requests, int n);
/* palettes made on the host: instances first .. first + n - 1, n x n_joints x 16 floats (pinned staging, no wait) */
int  swr_pose_set_upload(swr_context* ctx, swr_pose_set* set, int first, int n, const float* palettes);
/* n_instances x n_joints x 16 floats as the device holds them; a set never written reads zeros */
int  swr_pose_set_readback(swr_context* ctx, const swr_pose_set* set, float* out);
/* dst[k] = skin(src[k]) by the palette of instance[k], for all k < n in ONE kernel launch: word for word what swr_mesh_skin gives
 * with that palette.  Two jobs may share a src or an instance.  ORDER: swr_mesh_skin's, applied once over all destinations.
 * SWR_ERR_INVALID_ARG, nothing written, the context usable: a NULL pointer, a dst that appears twice or is any job's src, unequal
 * vertex counts, a src without skin attributes, an instance out of range, a set whose n_joints is not above the src's largest joint
 * index, a mesh or set of another context, a transient mesh.  n = 0 or only empty meshes: SWR_OK, nothing launched. */
int  swr_mesh_skin_batch(swr_context* ctx, int n, swr_mesh* const* dst, const swr_mesh* const* src, const swr_pose_set* set,
                         const int32_t* instance);

/* state ≙ public statics Rasterizer.NearClip / FarClip / RenderDebugMode, Rasterizer.cs:20-22 */
int  swr_set_state(swr_context* ctx, float near_clip, float far_clip, int debug_mode);
/* Rasterizer.InitializeTileLocks, Rasterizer.cs:69-93: width/height <= 0 -> SWR_ERR_INVALID_ARG */
int  swr_initialize_tile_locks(swr_context* ctx, int width, int height);

/* draw ≙ Rasterizer.RenderMesh, Rasterizer.cs:163-174 --------------------------------------- */
int  swr_render_mesh(swr_context* ctx, const swr_mesh* mesh,
                     const float model[16], const float view[16], const float projection[16],
                     int program, const swr_uniforms* uniforms, const swr_texture* texture /* NULL -> white */,
                     int cull_mode, int depth_test, int blend_mode);
/* same, taking the arrays of the C# signature directly (copied to HBM for this draw only) */
int  swr_render_mesh_arrays(swr_context* ctx, const swr_vertex* vertices, int n_vertices,
                            const uint16_t* indices, int n_indices,
                            const float model[16], const float view[16], const float projection[16],
                            int program, const swr_uniforms* uniforms, const swr_texture* texture,
                            int cull_mode, int depth_test, int blend_mode);
/* FrustumCuller.cs on the GPU (row N3) ------------------------------------------------------- */
/* Mesh.SphereBounds = FrustumCuller.CalculateBoundingSphere(vertices) (FrustumCuller.cs:59-151, ModelLoader.cs:291),
 * computed once per retained mesh in the serial schedule of the reference's loops; out = {cx, cy, cz, radius} */
int  swr_mesh_bounds(swr_context* ctx, const swr_mesh* mesh, float center_radius[4]);
/* FrustumCuller.IsSphereInFrustum(bounds, model, view, projection), FrustumCuller.cs:201-218 */
int  swr_is_sphere_in_frustum(swr_context* ctx, const float center_radius[4], const float model[16], const float view[16],
                              const float projection[16], int* inside);
/* `if (!IsSphereInFrustum(mesh.SphereBounds, ...)) return; RenderMesh(...)` of Renderer.cs:446-459, with the test
 * evaluated on the device at flush time (one thread per draw): a culled mesh costs no host round trip */
/* LIMIT (ABI 3, all three render calls): one draw holds fewer than 2^26 vertex-stage records = vertices + 4 x triangles (about
 * 16.7 M triangles of a u16-indexed mesh); a larger one is refused with SWR_ERR_UNSUPPORTED when it is recorded.  Draws are batched
 * up to that same bound and flushed by themselves beyond it. */
int  swr_render_mesh_culled(swr_context* ctx, const swr_mesh* mesh,
                            const float model[16], const float view[16], const float projection[16],
                            int program, const swr_uniforms* uniforms, const swr_texture* texture,
                            int cull_mode, int depth_test, int blend_mode);
/* Physics.cs on the GPU: batched ray queries against retained meshes -------------------------------------------------------------
 * Physics.RaycastFaceMask (Physics.cs:8-14) in the low bits of `flags`; SWR_RAY_CROSS_FUSED selects the other model of
 * Vector3.Cross: default (a.y*b.z) - (a.z*b.y) with two rounded products, fused fma(-a.z, b.y, a.y*b.z) (one more System.Numerics
 * switch nothing pins; csharp/RasterizerNative.cs probes it at start-up). */
enum { SWR_RAY_FACES_ALL = 0, SWR_RAY_IGNORE_BACKFACES = 1, SWR_RAY_IGNORE_FRONTFACES = 2, SWR_RAY_CROSS_FUSED = 0x100 };
typedef struct swr_ray { float origin[3]; float direction[3]; } swr_ray;                       /* 24 B; the direction need not be normalised (Physics.cs:69) */
/* one mesh of a collision model: normal_matrix = Transpose(Invert(model)), computed by the CALLER with its own Matrix4x4.Invert
 * (Physics.cs:30-38); a model that does not invert is the caller's `return false`: leave the target out */
typedef struct swr_ray_target { const swr_mesh* mesh; float model[16]; float normal_matrix[16]; } swr_ray_target;   /* 136 B */
/* a hit: found = 1, distance, point, normal as Physics.Raycast's out parameters; a miss: found = 0, distance = float.MaxValue, point and
 * normal zero, triangle = -1 (Physics.cs:65-67).  target = index into `targets`; triangle = the winning triangle (build-defined) */
typedef struct swr_ray_hit { int32_t found, target, triangle; float distance, point[3], normal[3]; } swr_ray_hit;   /* 40 B */
/* Physics.Raycast(origin, direction, mesh.Vertices, mesh.Indices, model, out d, out p, out n, mask) (Physics.cs:19-179) for every
 * (ray, target) pair in the reference's serial schedule: the nearest hit under float `<` among distances below float.MaxValue, the
 * lowest triangle index on ties (-0.0 and +0.0 tie; the winner's own word is returned), bit for bit under this library's
 * System.Numerics model and the context's Transform flag (swr_set_transform_fma).  out[ray * n_targets + target].
 * Reads retained mesh data only: recorded draws are neither flushed nor waited for, and the query runs on a stream of its own, so
 * it does not queue behind a frame in flight.  n_rays == 0 or n_targets == 0: SWR_OK, nothing written.  NULL pointers, negative
 * counts, a NULL mesh, unknown flag bits: SWR_ERR_INVALID_ARG.  LIMITS: n_rays <= 2^20, n_targets <= 65535, n_rays * n_targets <= 2^24
 * pairs per call, beyond which SWR_ERR_UNSUPPORTED (split the rays).  A mesh without triangles misses. */
int  swr_raycast(swr_context* ctx, const swr_ray* rays, int n_rays, const swr_ray_target* targets, int n_targets,
                 int flags, swr_ray_hit* out /* n_rays * n_targets, ray-major */);
/* the same, reduced over the targets on the device in target order under `if (hit && distance < best)` starting from "not found" -- the
 * serial schedule of the callers' lock blocks (CharacterController.cs:260-301,308-389, Renderer.cs:172-216): the first of equally near
 * targets wins; a ray that misses every target gives the miss record with target = -1.  Only n_rays records cross PCIe.  A caller's
 * own distance limit (maxDistance, moveDistance) stays on the caller's side. */
int  swr_raycast_nearest(swr_context* ctx, const swr_ray* rays, int n_rays, const swr_ray_target* targets, int n_targets,
                         int flags, swr_ray_hit* out /* n_rays */);

/* CharacterController.Update on the GPU (CharacterController.cs:50-140): one call per step for a batch of controllers ------------
 * The properties of CharacterController.cs:21-32 shared by the call (CamOffset stays with the caller). */
typedef struct swr_character_params {
    float gravity[3], height, radius, step_size, move_speed, jump_force, ground_acceleration, air_acceleration, max_air_speed,
          ground_friction, air_control;
} swr_character_params;                                                                        /* 52 B */
/* one controller, in and out.  actual_step_size is the private field of CharacterController.cs:25 and is STATE: 0.03f in a new
 * controller, then StepSize or 0 as the previous step left it.  jump_cooldown is JumpCooldownTimer (:47). */
typedef struct swr_character {
    float position[3], velocity[3], jump_cooldown, actual_step_size;
    int32_t grounded, ceiling, noclip;
} swr_character;                                                                               /* 44 B */
typedef struct swr_character_input { float move[3]; int32_t jump; } swr_character_input;        /* 16 B: MoveInput, JumpRequested */
/* what a step decided, for tests and debugging: the ground CheckPlane's results (point = Vector3.NegativeInfinity, normal = UnitY
 * where nothing was found), and for the two MoveWithSlide chains (:96, :118) the number of attempts that cast rays (0..3) and why
 * the chain ended: 0 not run, 1 no collision, 2 |alignment| > 0.9, 3 zero slide direction, 4 depth limit.  All zero under noclip. */
typedef struct swr_character_trace {
    int32_t ground_found, ceiling_found;
    float ground_point[3], ground_normal[3];
    int32_t chain_attempts[2], chain_stop[2];
} swr_character_trace;                                                                         /* 48 B */
/* verticalSteps = Math.Max(1, (int)(Height / (radius * 2))) and horizontalRays = Math.Max(4, (int)(4 * MathF.PI * radius / 0.1f)) with
 * radius = Radius + 0.001f (:96,118,327-328), in float arithmetic in the reference's order.  Host code only; a slide attempt casts
 * (verticalSteps + 1) * horizontalRays rays.  NULL arguments: SWR_ERR_INVALID_ARG. */
int  swr_character_ray_counts(const swr_character_params* params, int* vertical_steps, int* horizontal_rays);
/* CharacterController.Update(delta_time, inputs[i].move, inputs[i].jump) for chars[0..n) in ONE call without a host round trip inside
 * it: both CheckPlanes, both MoveWithSlide chains of up to three attempts and the velocity update, in the reference's serial
 * schedules (CheckPlane: rays outer in offsets[] order, targets inner; MoveWithSlide: targets outer, then vStep, then hStep; strict
 * `<` in both), bit for bit under this library's System.Numerics model, the context's Transform flag and the call's Cross model.
 * ring: n_ring pairs (cos, sin) of the angle 2 * MathF.PI * hStep / horizontalRays AS THE CALLER'S RUNTIME COMPUTES THEM (MathF.Cos is
 * the C runtime's and cannot be reproduced on the device); the device multiplies by radius.  n_ring must equal horizontal_rays of
 * swr_character_ray_counts.  targets: collisionModels[i] flattened, model-major, mesh-minor; a model that does not invert is left
 * out by the caller.  flags: 0 or SWR_RAY_CROSS_FUSED; the face mask is always IgnoreBackfaces (:282,357).  trace: NULL or n records.
 * n == 0: SWR_OK, nothing written.  n_targets == 0: the step runs with every ray missing.  NULL pointers, negative counts, other
 * flag bits, a target without a mesh, n_ring != horizontal_rays: SWR_ERR_INVALID_ARG.  LIMITS: n <= 65536 controllers, at most 4096
 * rays per slide attempt, n * max(18, rays per attempt) <= 2^22 rays (two ray buffers of 24 B each: at most 192 MiB, whatever n_targets
 * is), n_targets <= 65535, n * max(18, rays per attempt) * n_targets <= 2^24 (ray, target) pairs per call, beyond which SWR_ERR_UNSUPPORTED (split the controllers).  Runs on the ray stream, like swr_raycast: recorded draws are neither flushed
 * nor waited for. */
int  swr_character_update(swr_context* ctx, const swr_character_params* params, swr_character* chars, const swr_character_input* inputs,
                          int n, float delta_time, const float* ring, int n_ring, const swr_ray_target* targets, int n_targets,
                          int flags, swr_character_trace* trace);

/* User fragment programs --------------------------------------------------------------------------------------------------------
 * Source contract (softwarerenderer_amd/csrc/swr_program.hip.h is the prelude compiled in front of the text; INTEGRATION.md has a
 * porting guide): the text defines
 *     __device__ float4 swr_fragment(const swr_fs_in& in, const swr_fs_env& env);
 * `in` = Shaders.VertexOutput after Rasterizer.Interpolate (Rasterizer.cs:566-640): clip_position, color, tex_coord, normal,
 * screen_coords, barycentric, world_normal (Data["WorldNormal"]), data4 (see swr_program_create_vf), tex_coord_grad (build-defined:
 * (du/dx, dv/dx, du/dy, dv/dy) of tex_coord per pixel step, for swr_sample_grad below); the vertex stage is Renderer.VertexShader (Renderer.cs:830-846,
 * Interpolate = true).  `env` = the draw's uniforms, constants[64], the pixel x, y; helpers swr_sample (Texture.Sample), swr_has_texture,
 * swr_dot3, swr_lerp (this library's System.Numerics model), swr_max, swr_clamp (MathF.Max, Math.Clamp), swr_discard() (a null
 * result: W <= 0 or NaN writes nothing, Rasterizer.cs:511).  Compiled with this library's switches and its numerics model; the
 * program is inlined into the raster kernel.
 * A batch holds the draws of one program: switching to, from or between user programs flushes (as SWR_PROG_DEBUG_VARYINGS does).
 * DebugMode.Wireframe with a user program is SWR_ERR_UNSUPPORTED.  `uniforms` may be NULL for a user program (it reads zeros). */
/* compile for this context's device: *program_id >= SWR_PROG_USER_BASE.  Compile error -> SWR_ERR_INVALID_ARG with the compiler's
 * log in swr_last_error(ctx); run-time compiler (libhiprtc) not loadable -> SWR_ERR_UNSUPPORTED */
int  swr_program_create(swr_context* ctx, const char* fragment_source, int* program_id);
/* the id stops being valid for new draws; draws already recorded still render with the program */
int  swr_program_destroy(swr_context* ctx, int program_id);
/* up to 64 floats the program reads as env.constants[i] (the rest read 0).  A draw takes a copy when it is RECORDED, as a C# closure
 * captures its fields: later calls do not change recorded draws */
int  swr_program_set_constants(swr_context* ctx, int program_id, const float* values, int n);
/* TEXTURE SLOTS: a user program reads SWR_PROGRAM_TEXTURES textures per draw, in both halves, through env:
 *     bool   swr_has_texture(env, slot)
 *     float4 swr_sample(env, slot, uv)        Texture.Sample exactly as swr_sample(env, uv) computes it: nearest with wrap, or the
 *                                             bilinear extension if the texture was switched to it when the draw was recorded
 *     float4 swr_texel(env, slot, x, y)       texel (x, y), x clamped to [0, w - 1] and y to [0, h - 1], each byte times the float 1 / 255
 *     int2   swr_texture_size(env, slot)      (w, h), positive whatever the filter
 *   and, of a slot that holds a DEPTH texture (swr_texture_create_depth):
 *     float  swr_texel_depth(env, slot, x, y)    the float32 depth word of texel (x, y), clamped as swr_texel clamps
 *     float  swr_sample_depth(env, slot, uv)     the word of the texel swr_sample's nearest addressing picks, whatever the filter
 *     float  swr_shadow(env, slot, uv, ref)      1 where a fragment of depth ref passes LessEqual against the stored depth (ref >= d;
 *                                             false for NaN), else 0; the bias is the caller's, added into ref.  Nearest filter: one
 *                                             texel.  Bilinear filter: the four results of the filter's 2 x 2 footprint blended as
 *                                             lerps by its fractions -- exactly 0 or 1 where all four agree (finite uv)
 *   An unbound or out-of-range slot reads float.MinValue (nothing drawn) and shadows nothing (1).
 *   and, of any slot, its MIP CHAIN (swr_texture_generate_mipmaps) -- the levels are read when the kernel RUNS:
 *     int    swr_texture_levels(env, slot)          1 without a chain, L with one; 0 for an unbound or out-of-range slot
 *     float4 swr_sample_level(env, slot, uv, level) one level, clamped to [0, levels - 1]: level 0 is swr_sample; a level >= 1 applies
 *                                             the slot's filter (nearest with wrap, or bilinear) inside that level, at that level's size
 *     float4 swr_sample_lod(env, slot, uv, lod)     NaN or negative counts as 0, above levels - 1 as levels - 1; l0 = (int)lod,
 *                                             f = lod - l0; f == 0 fetches level l0 alone, else c0 (1 - f) + c1 f per channel with c1
 *                                             from level min(l0 + 1, levels - 1)
 *     float  swr_lod(env, slot, grad)            float4 grad = (du/dx, dv/dx, du/dy, dv/dy) per pixel step: rho = the longer step in
 *                                             level-0 texels, sqrt(max((dudx w)^2 + (dvdx h)^2, (dudy w)^2 + (dvdy h)^2)); 0 unless
 *                                             rho > 1 (magnification, zero, NaN); else exponent(rho) + (significand(rho) - 1), a
 *                                             piecewise-linear log2 from rho's bits -- exact at powers of two, at most 0.0861 below
 *                                             log2(rho), never above --, clamped to levels - 1
 *     float4 swr_sample_grad(env, slot, uv, grad)   swr_sample_lod(env, slot, uv, swr_lod(env, slot, grad))
 *   An unbound or out-of-range slot has 0 levels, lod 0, and samples (1, 1, 1, 1).  The fragment half gets its own gradient as
 *   in.tex_coord_grad, the analytic derivative of in.tex_coord per pixel step (per fragment: there are no quads).
 *   and, of a slot that holds a CUBE MAP (swr_texture_create_cube), by a float3 direction of any length:
 *     void   swr_cube_face(dir, &face, &uv)         the face (int) and where in it (float2 in [0, 1]^2, v downwards)
 *     float4 swr_sample_cube(env, slot, dir)        the slot's filter inside the face (bilinear: taps clamped to the face)
 *     float4 swr_sample_cube_level(env, slot, dir, level), swr_sample_cube_lod(env, slot, dir, lod)   inside the cube's chain
 *     float4 swr_cube_texel(env, slot, face, x, y)  one texel; face clamped to [0, 5], x and y to the face
 *     int    swr_cube_size(env, slot)               n
 *     float  swr_sample_cube_depth(env, slot, dir)  a depth cube's word, always nearest
 *     float  swr_shadow_cube(env, slot, dir, ref)   swr_shadow by direction: a point light's shadow with dir = world - light
 *   A slot that is unbound, out of range or not n by 6 n is not a cube: (1, 1, 1, 1), float.MinValue, shadow 1, size 0 -- no load.
 * Slot 0 is and stays the `texture` argument of the render call.  Slots 1 .. SWR_PROGRAM_TEXTURES - 1 belong to the program, as its
 * constants do: a draw copies each slot's pointer, size and filter (the block-linear copy where the texture has one) when it is
 * RECORDED; later swr_program_set_texture and swr_texture_set_filter calls do not change recorded draws.  An unbound slot, and a slot
 * outside 0 .. SWR_PROGRAM_TEXTURES - 1, has no texture: it samples and reads (1, 1, 1, 1) and measures (0, 0).  The slot may be
 * computed per fragment.  Two draws share fragment-stage state only if their captured constants and slots are bitwise equal.
 * ORDER against texture updates: swr_texture_update_from_frame / _from_post flush the recorded draws first, so draws recorded before
 * an update of a texture bound to slot 1 .. 3 sample the old texels, and later draws sample the new ones.
 * swr_texture_destroy clears the texture out of every live user program of its context: a later draw reads "no texture" there.
 * Bind a texture of this context to slot 1 .. SWR_PROGRAM_TEXTURES - 1 of a user program (NULL unbinds).  SWR_ERR_INVALID_ARG, with
 * the slots left as they were: an unknown or destroyed id, an id below SWR_PROG_USER_BASE, a slot outside 1 .. 3. */
#define SWR_PROGRAM_TEXTURES 4
int  swr_program_set_texture(swr_context* ctx, int program_id, int slot, const swr_texture* tex /* NULL unbinds */);
/* compile only, without a context or a device: SWR_OK, SWR_ERR_INVALID_ARG (log = compiler messages, NUL-terminated, truncated to
 * log_len) or SWR_ERR_UNSUPPORTED */
int  swr_program_validate(const char* fragment_source, char* log, int log_len);
/* User VERTEX programs (any Shaders.VertexShader delegate, restated in C++) --------------------------------------------------------
 * A user program is a (vertex, fragment) pair.  The vertex text defines
 *     __device__ void swr_vertex(const swr_vs_in& in, const swr_vs_env& env, swr_vs_out& out);
 * and is compiled into a vertex kernel of its own in the same code object as the program's raster kernels; it runs in place of the
 * built-in vertex stage for the draws of this program.  `in` = Shaders.VertexInput (position, uv, normal, color).  `env` = model, view,
 * projection (16 floats each, row-major as above), the draw's uniforms, and constants[64] -- the SAME constants the fragment half
 * reads, captured when the draw is recorded.  `out` = new Shaders.VertexOutput(), all zeros: clip_position, color, tex_coord, normal,
 * world_normal (Data["WorldNormal"], a Vector3 key) and data4, ONE Vector4 key of the program's own, which the fragment half reads as
 * in.data4 -- lerped in the near-plane clipper like every varying (Shaders.cs:74-75), interpolated as (a * wa + b * wb) + c * wc with
 * the normalised weights and nothing else (Rasterizer.cs:690-693).  A program without a vertex half reads data4 = (0, 0, 0, 0).
 * Interpolate is true for every user program; a per-program Interpolate = false is out of scope, and so are further Data keys (a
 * float or a Vector2 key interpolates like Vector4 components and can ride in data4).
 * Helpers under this library's System.Numerics model and the context's run-time transform flags (swr_set_transform_fma):
 * swr_transform(v, m, env) = Vector4.Transform, swr_transform_normal(n, m, env) = Vector3.TransformNormal, swr_normalize(v) =
 * v / v.Length(), swr_dot3, swr_lerp: a restated Renderer.VertexShader gives the built-in stage's bits in every build and setting.
 * swr_render_mesh_culled still tests the MESH's bounding sphere (the application's test, Renderer.cs:446-459), whatever the vertex
 * program does; a draw with a vertex program is never dropped from a multi-GPU band by its bounding box.
 * Compile errors name the half and the line in the caller's text: `vertex.hip:LINE:` or `fragment.hip:LINE:`.  A vertex text that
 * does not define swr_vertex is SWR_ERR_INVALID_ARG.  vertex_source == NULL is Renderer.VertexShader, the built-in stage:
 * swr_program_create(ctx, fs, id) == swr_program_create_vf(ctx, NULL, fs, id). */
int  swr_program_create_vf(swr_context* ctx, const char* vertex_source, const char* fragment_source, int* program_id);
int  swr_program_validate_vf(const char* vertex_source, const char* fragment_source, char* log, int log_len);

/* POST-PROCESS programs (build-defined: the reference presents the frame as rendered) ---------------------------------------------
 * A user's per-pixel pass between the frame and its delivery -- a damage flash, a tone curve in front of the 8-bit quantiser, a
 * vignette, a depth fog or outline, a small blur -- without the frame leaving the device (csrc/swr_post.hip.h is the prelude compiled
 * in front of the text; INTEGRATION.md has a porting guide).  The text defines
 *     __device__ float4 swr_post(const swr_post_in& in, const swr_post_env& env);
 * and runs once per OUTPUT pixel of the present.  `in` = x, y (the output pixel, window coordinates after the resolve) and color (the
 * resolved pixel: R, G, B exactly the floats swr_readback_rgb_resolved(kx, ky) delivers, the flatten's under (1, 1); A the frame's
 * alpha through the same pairwise tree and scale).  `env` = width, height (the resolved size), kx, ky, constants[64].  Helpers:
 * swr_post_fetch(env, x, y), the resolved RGBA of output pixel (x, y), and swr_post_depth(env, x, y), the depth word swr_get_depth
 * returns for sample (x * kx, y * ky) -- the top-left sample of the pixel's block, not an average; float.MinValue where the depth
 * plane was cleared -- both with x clamped to [0, width - 1] and y to [0, height - 1]; swr_lerp, swr_max, swr_clamp as in fragment
 * programs.  Compiled with this library's switches and its numerics model.
 * TEXTURES: a program has SWR_POST_TEXTURES slots (swr_post_set_texture), read through env:
 *   bool   swr_post_has_texture(env, slot)
 *   float4 swr_post_sample(env, slot, uv)     Texture.Sample exactly as a draw sees it (swr_sample): nearest with wrap -- or the
 *          build-defined bilinear filter if the texture was switched to it (swr_texture_set_filter) when the present was CALLED, then
 *          from the block-linear copy where one exists
 *   float4 swr_post_texel(env, slot, x, y)    the row-major texel, x clamped to [0, w - 1] and y to [0, h - 1], each byte times the
 *          float 1 / 255 (Texture.cs:57-62): no filter, so a pixel-aligned read does not depend on a uv rounding
 *   int2   swr_post_texture_size(env, slot)
 *   float  swr_post_texel_depth(env, slot, x, y), swr_post_sample_depth(env, slot, uv), swr_post_shadow(env, slot, uv, ref)
 *          a DEPTH texture's words and the shadow comparison: swr_texel_depth, swr_sample_depth and swr_shadow of a user program,
 *          above; an unbound or out-of-range slot reads float.MinValue and shadows nothing (1)
 *   int    swr_post_texture_levels(env, slot), float4 swr_post_sample_level(env, slot, uv, level), swr_post_sample_lod(env, slot, uv, lod),
 *          float swr_post_lod(env, slot, grad)
 *          a MIP CHAIN's lookups: swr_texture_levels, swr_sample_level, swr_sample_lod and swr_lod of a user
 *          program, above.  A post pass has no gradient field: it knows its own scale (a half-size pass reads lod 1)
 *   swr_post_cube_face, swr_post_sample_cube, swr_post_sample_cube_level, swr_post_sample_cube_lod, swr_post_cube_texel,
 *          swr_post_cube_size, swr_post_sample_cube_depth, swr_post_shadow_cube
 *          a CUBE MAP's lookups: the functions of a user program without the prefix, above
 * An unbound slot, and a slot outside 0 .. SWR_POST_TEXTURES - 1, has no texture: it samples and reads (1, 1, 1, 1), as swr_sample
 * does without a texture, and measures (0, 0).
 * What the result's x, y, z become (w is ignored, except by swr_texture_update_from_post): */
enum { SWR_POST_RGB32F = 0,     /* three floats as they are, no clamp: the payload of swr_readback_rgb_resolved */
       SWR_POST_RGB8 = 3,       /* the 8-bit present's quantiser (above), three bytes: the payload of swr_readback_rgb8(.., 3) */
       SWR_POST_RGBX8 = 4 };    /* the same and a fourth byte of 255: the payload of swr_readback_rgb8(.., 4) */
/* compile for this context's device.  Compile error -> SWR_ERR_INVALID_ARG with the compiler's log in swr_last_error(ctx), naming the
 * caller's line as `post.hip:LINE:`; a text that does not define swr_post -> SWR_ERR_INVALID_ARG; libhiprtc not loadable ->
 * SWR_ERR_UNSUPPORTED.  Post ids are not program ids of swr_render_mesh, and one context's id is unknown to every other context */
int  swr_post_create(swr_context* ctx, const char* source, int* post_id);
/* the id stops being valid; a present already enqueued with the program still completes (safe with a kernel in flight) */
int  swr_post_destroy(swr_context* ctx, int post_id);
/* up to 64 floats the program reads as env.constants[i] (the rest read 0).  A present takes a copy when it is CALLED: two
 * presents in flight each keep their own */
int  swr_post_set_constants(swr_context* ctx, int post_id, const float* values, int n);
/* Bind a texture of this context to slot 0 .. SWR_POST_TEXTURES - 1 of a program of this context (NULL unbinds).  A present, of any of
 * the four deliveries, takes a copy of the four slots -- and of each texture's filter -- when it is CALLED, as it takes the constants:
 * two presents in flight each keep their own.  The texels it reads are what the work enqueued before it leaves: a
 * swr_texture_update_from_frame / _from_post before the present is seen, one after it is not (textures and presents of a context
 * share its stream: no host wait).  swr_texture_destroy clears the texture out of every live post program of its context: a later
 * present reads "no texture" there.  SWR_ERR_INVALID_ARG, the slots staying as they were: an unknown or destroyed id (or another
 * context's), a slot outside 0 .. SWR_POST_TEXTURES - 1. */
#define SWR_POST_TEXTURES 4
int  swr_post_set_texture(swr_context* ctx, int post_id, int slot, const swr_texture* tex /* NULL unbinds */);
/* compile only, without a context or a device, as swr_program_validate */
int  swr_post_validate(const char* source, char* log, int log_len);
/* host only: swr_resolved_size plus out_bytes = out_rows * out_width * (12, 3 or 4 by format) */
int  swr_post_size(swr_context* ctx, int kx, int ky, int format, int* out_width, int* out_rows, size_t* out_bytes);
/* The four deliveries, each exactly as its 8-bit counterpart -- swr_readback_rgb8, swr_present_rgb8_async (the same two slots,
 * tickets, staging buffers, swr_present_wait, staleness rule and back-pressure: all four kinds of present may alternate),
 * swr_resolve_rgb8_device and its _async form (device destinations 4-byte aligned) -- with the program's result in the payload's
 * place: recorded draws are flushed first, the _async forms never wait for the GPU, swr_set_stream and a bound framebuffer are
 * honoured, a zero-size target is SWR_OK and writes nothing.
 * SWR_ERR_INVALID_ARG: an unknown or destroyed id (or another context's), a format other than the three above, bad factors, a size
 * the factors do not divide, NULL pointers.  SWR_ERR_UNSUPPORTED: the context holds only a band of its frame (swr_set_band*): a
 * neighbour across the band's edge is not there.  Nothing is written then, no ticket is issued and the context stays usable.
 * A program must terminate and read through the helpers only. */
int  swr_readback_post(swr_context* ctx, int post_id, int kx, int ky, int format, void* out);
int  swr_present_post_async(swr_context* ctx, int post_id, int kx, int ky, int format, void* out, uint64_t* ticket);
int  swr_post_device(swr_context* ctx, int post_id, int kx, int ky, int format, void* d_out);
int  swr_post_device_async(swr_context* ctx, int post_id, int kx, int ky, int format, void* d_out);
/* A pass's result into a texture: swr_texture_update_from_frame with the program between the resolve and the quantiser.  `post_id` is
 * a program of `src` (of ctx when src is NULL).  Texel (x, y) of the w x h texture is the program's result for output pixel (x, y) of
 * src's frame, which measures w * kx by h * ky: R, G, B quantise8 of x, y, z -- the bytes swr_readback_post(.., SWR_POST_RGBX8)
 * delivers -- and A 255 under SWR_TEXTURE_ALPHA_OPAQUE, quantise8(w) under SWR_TEXTURE_ALPHA_KEEP (the one place where a post result's
 * w is read).  Everything else is swr_texture_update_from_frame's contract: immediate-mode semantics (draws and presents recorded or
 * called earlier see the old texels, later ones the new), both contexts' recorded draws are flushed, the kernels go onto ctx's
 * stream, nothing waits for the GPU in the steady state (src's resolved plane is allocated or grown on first use and after a resize,
 * behind a wait for src's stream), two contexts are ordered by the same two events -- src's later work, a present of src or an
 * update of a texture the program samples included, runs behind the kernels -- swr_set_stream and a bound framebuffer are honoured,
 * the block-linear copy of a bilinear target is fresh, and the note on optimistic flushes applies.  A chain of passes is a sequence of
 * calls: pass 1 writes texture A, pass 2 samples A.
 * Refused, with nothing written and both contexts usable: whatever swr_texture_update_from_frame refuses, with its codes; an unknown
 * or destroyed id, or one of a context other than src (SWR_ERR_INVALID_ARG); and `tex` bound to a slot of the program at the call
 * (SWR_ERR_INVALID_ARG): a pass may not sample the texture it writes -- ping-pong between two textures is the supported feedback. */
int  swr_texture_update_from_post(swr_context* ctx, swr_texture* tex, swr_context* src, int post_id,
                                  int kx, int ky, int alpha_mode);

int  swr_flush(swr_context* ctx);    /* execute recorded draws (asynchronous on the stream) */
int  swr_sync(swr_context* ctx);     /* flush + wait for the stream */
/* Frames in flight.  The reference's loop renders frames back to back (Renderer.cs:404-419: RenderScene per frame; Rasterizer.cs:
 * 163-230: RenderMesh per mesh).  A pipelined flush runs its front end -- vertex stage, clip, setup, binning, coverage -- on a second
 * stream beside the raster kernel of the flush before it (double-buffered intermediates, event-ordered hand-over); pixels, counters
 * and every ordering guarantee against the context's stream are unchanged.  mode: 0 = never (one stream: what kernel timings are
 * quoted on), 1 = every batch (default: 4096^2 / 1 M triangles -6 %, 1920x1080 -8 ... -16 % in steady state; a burst of K frames from
 * an idle context pays one un-overlapped front end, +0.2 ms / K), 2 = only frames of up to 2^15 tiles (2896^2 pixels) or batches of
 * up to 2^17 triangles (bigger ones run on the context's stream, ordered against pipelined neighbours by events).  Switching drains. */
int  swr_set_pipelining(swr_context* ctx, int mode);
int  swr_get_pipelining(swr_context* ctx, int* mode);

/* Rasterizer.Interpolate (public, Rasterizer.cs:566-640), batched on the GPU for API coverage:
 * verts = 3 vertex records of 20 floats {clip4,color4,uv2,normal3,screen2,worldNormal3,pad2};
 * w = n * 3 barycentric weights; out = n records of 24 floats
 * {clip4,color4,uv2,normal3,screen2,worldNormal3,bary3,pad3} */
int  swr_interpolate(swr_context* ctx, const float* verts60, const float* w, int n, int interpolate, float* out);

/* counters / profiling ------------------------------------------------------------------------ */
int  swr_get_stats(swr_context* ctx, swr_stats* out);   /* syncs */
int  swr_reset_stats(swr_context* ctx);
int  swr_profile_enable(swr_context* ctx, int on);       /* 0 off; 1 hipEvent pairs around every stage of a flush; 2 around the raster kernel only;
                                                           * 3 around the raster kernel of every 4th flush (a pair costs about 10 us of stream time) */
int  swr_profile_get(swr_context* ctx, swr_profile* out); /* syncs */
int  swr_profile_reset(swr_context* ctx);
/* the duration (ms) of every raster-kernel launch that carried an event pair since swr_profile_reset, in launch order: *n = how
 * many there are (at most 65,536 are kept), the first min(*n, capacity) are copied (bench.py: median / min / max).  syncs */
int  swr_profile_raster_samples(swr_context* ctx, float* out_ms, int capacity, int* n);
int  swr_device_name(swr_context* ctx, char* buf, int buflen);
/* Self-test of the kernels' exact-division shortcut (csrc/swr_device.h: div_core / rcp_refined / sqrt_core): about
 * `samples` random, near-midpoint, boundary and renderer-shaped operand pairs are divided both ways on the GPU and compared bit
 * for bit with the compiler's correctly rounded `/` and sqrtf (the IEEE results the reference's C# computes, Rasterizer.cs:576-582,
 * 684-686, Renderer.cs:855); the reciprocal core (recip_core, n = 1) is checked on EVERY float of its range, both signs, on top
 * of `samples`.  out = {divisions tested, mismatches, sqrts tested, mismatches, first bad n, d, got, want}. */
int  swr_selftest_division(swr_context* ctx, uint64_t samples, uint64_t seed, uint64_t out[8]);
/* kernel-internal work counters; all zero unless the library was built with -DSWR_DEBUG_COUNTERS (tools/) */
int  swr_debug_counters(swr_context* ctx, uint64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* SWR_H */
