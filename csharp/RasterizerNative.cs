// RasterizerNative.cs -- the C# side of the drop-in boundary: P/Invoke binding of libswr_hip.so (include/swr.h) and the
// forwards that put it behind the reference's own API surface (OCSYT/SoftwareRenderer, net9.0).
//
// A maintainer adds this ONE file to the project and
//   * renames the body of Rasterizer.RenderMesh (Rasterizer.cs:163-230) to RenderMeshManaged (kept as the path for
//     shader delegates the backend has no built-in program for) and makes `Rasterizer` a `partial` class;
//   * replaces the six accessor bodies of MainWindow (MainWindow.cs:382-436) and its buffer allocation
//     (MainWindow.cs:320-321) with the one-line forwards of `MainWindowNative` below;
//   * lets `Texture` (Texture.cs:31-68) hold a `TextureNative` next to its Image<Rgba32>.
// Renderer.cs, Camera.cs, FrustumCuller.cs, ModelLoader.cs, Material.cs, Light.cs stay as they are: RenderMesh keeps its
// exact signature and defaults, and the one shader pair the application uses (Renderer.VertexShader / FragmentShader,
// Renderer.cs:830-860) is recognised and mapped to SWR_PROG_DUST2_LAMBERT_FOG with its closed-over fields as uniforms.
//
// Physics.Raycast (Physics.cs:19-52) gets an overload on a retained Mesh (PhysicsNative below): CharacterController.cs and
// Renderer.Shoot can call it with `mesh` instead of `mesh.Vertices.ToArray(), mesh.Indices.ToArray()`, or batch a whole slide attempt
// into one RaycastNearest (INTEGRATION.md).  Like the rest of this file it was written by reading the reference, not compiled.
//
// There is no .NET toolchain in the build image, so this file is NOT compiled there; tests/test_abi.py parses it and
// checks it mechanically against include/swr.h and the ctypes binding (every entry point present with the right arity,
// struct field order and sizes).  The compiled, tested callers of the same ABI are softwarerenderer_amd/rasterizer.py
// (ctypes), softwarerenderer_amd/cpp/Rasterizer.hpp (C++) and tests/c/abi_smoke.c (plain C, dlopen).
using System;
using System.Collections.Generic;
using System.Numerics;
using System.Reflection;
using System.Runtime.CompilerServices;
using System.Runtime.InteropServices;
using SixLabors.ImageSharp;
using SixLabors.ImageSharp.PixelFormats;

namespace SoftwareRenderer
{
    // ---------------------------------------------------------------- structs of include/swr.h ----
    [StructLayout(LayoutKind.Sequential)]
    public struct SwrPointLight            // swr_point_light (subset of Light.cs:9-17 used by PHONG_4POINT)
    {
        public Vector3 Position;
        public float Range;
        public Vector3 Color;
        public float Intensity;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct SwrUniforms              // swr_uniforms: the fields Renderer.FragmentShader closes over, Renderer.cs:39-44
    {
        public Vector3 LightDirection;
        public float Pad0;
        public Vector4 LightColor;
        public Vector4 FogColor;
        public float FogStart;
        public float FogEnd;
        public float Shininess;
        public float Pad1;
        public Vector3 CameraPosition;
        public float Pad2;
        public SwrPointLight Light0;
        public SwrPointLight Light1;
        public SwrPointLight Light2;
        public SwrPointLight Light3;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct SwrStats                 // swr_stats
    {
        public ulong TrianglesIn;
        public ulong TrianglesSetup;
        public ulong TrianglesClipped;
        public ulong FragmentsTested;
        public ulong FragmentsShaded;
        public ulong FragmentsWritten;
        public ulong TilePairs;
        public ulong Flushes;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct SwrProfile               // swr_profile
    {
        public double VertexMs;
        public double SetupMs;
        public double BinMs;
        public double SortMs;
        public double CoverMs;
        public double RasterMs;
        public double ClearMs;
        public double TotalMs;
        public ulong RasterLaunches;
        public ulong Flushes;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct SwrRay                   // swr_ray, 24 bytes
    {
        public Vector3 Origin;
        public Vector3 Direction;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct SwrRayTarget             // swr_ray_target, 136 bytes
    {
        public IntPtr Mesh;
        public Matrix4x4 Model;
        public Matrix4x4 NormalMatrix;     // Matrix4x4.Transpose(invModel), Physics.cs:38
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct SwrRayHit                // swr_ray_hit, 40 bytes
    {
        public int Found;
        public int Target;
        public int Triangle;
        public float Distance;
        public Vector3 Point;
        public Vector3 Normal;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct SwrCharacterParams       // swr_character_params, 52 bytes: the properties of CharacterController.cs:21-32
    {
        public Vector3 Gravity;
        public float Height;
        public float Radius;
        public float StepSize;
        public float MoveSpeed;
        public float JumpForce;
        public float GroundAcceleration;
        public float AirAcceleration;
        public float MaxAirSpeed;
        public float GroundFriction;
        public float AirControl;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct SwrCharacter             // swr_character, 44 bytes: one controller's state, in and out
    {
        public Vector3 Position;
        public Vector3 Velocity;
        public float JumpCooldown;
        public float ActualStepSize;       // the private field of CharacterController.cs:25: 0.03f in a new controller
        public int Grounded;
        public int Ceiling;
        public int NoClip;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct SwrCharacterInput        // swr_character_input, 16 bytes
    {
        public Vector3 Move;
        public int Jump;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct SwrCharacterTrace        // swr_character_trace, 48 bytes
    {
        public int GroundFound;
        public int CeilingFound;
        public Vector3 GroundPoint;
        public Vector3 GroundNormal;
        public int Chain1Attempts;
        public int Chain2Attempts;
        public int Chain1Stop;             // 0 not run, 1 no collision, 2 |alignment| > 0.9, 3 zero slide direction, 4 depth limit
        public int Chain2Stop;
    }

    public enum SwrProgram { FlatColor = 0, Gouraud = 1, Dust2LambertFog = 2, Phong4Point = 3, DebugVaryings = 4 }

    // ---------------------------------------------------------------- the 65 entry points ----
    // Shaders.VertexInput (Shaders.cs:10-24) IS swr_vertex: four sequential System.Numerics fields, 48 bytes, blittable.
    // Matrix4x4 is 16 sequential floats M11..M44 (row-major, row-vector convention): passed by address, no marshalling.
    internal static unsafe class Native
    {
        const string Lib = "swr_hip";      // libswr_hip.so
        [DllImport(Lib)] public static extern int swr_abi_version();
        [DllImport(Lib)] public static extern IntPtr swr_build_info();
        [DllImport(Lib)] public static extern int swr_numerics_mode(out int fma, out int dotOrder);
        [DllImport(Lib)] public static extern int swr_set_transform_fma(IntPtr ctx, int transformFused, int transformNormalFused);
        [DllImport(Lib)] public static extern int swr_get_transform_fma(IntPtr ctx, out int transformFused, out int transformNormalFused);
        [DllImport(Lib)] public static extern IntPtr swr_last_error(IntPtr ctx);
        [DllImport(Lib)] public static extern int swr_create(int deviceId, out IntPtr ctx);
        [DllImport(Lib)] public static extern void swr_destroy(IntPtr ctx);
        [DllImport(Lib)] public static extern int swr_resize(IntPtr ctx, int width, int height);
        [DllImport(Lib)] public static extern int swr_set_band(IntPtr ctx, int firstTileRow, int nTileRows);
        [DllImport(Lib)] public static extern int swr_set_band_interleaved(IntPtr ctx, int rank, int world, int stripeTileRows);
        [DllImport(Lib)] public static extern int swr_bind_framebuffer(IntPtr ctx, IntPtr colorDevicePtr, IntPtr depthDevicePtr);
        [DllImport(Lib)] public static extern int swr_set_stream(IntPtr ctx, IntPtr hipStream);
        [DllImport(Lib)] public static extern int swr_clear_color(IntPtr ctx, Vector4* rgba);
        [DllImport(Lib)] public static extern int swr_clear_depth(IntPtr ctx);
        [DllImport(Lib)] public static extern int swr_get_pixel(IntPtr ctx, int x, int y, Vector4* rgba);
        [DllImport(Lib)] public static extern int swr_set_pixel(IntPtr ctx, int x, int y, Vector4* rgba);
        [DllImport(Lib)] public static extern int swr_get_depth(IntPtr ctx, int x, int y, float* depth);
        [DllImport(Lib)] public static extern int swr_set_depth(IntPtr ctx, int x, int y, float depth);
        [DllImport(Lib)] public static extern int swr_readback(IntPtr ctx, Vector4* colorRgba, float* depth);
        [DllImport(Lib)] public static extern int swr_readback_rgb(IntPtr ctx, Vector3* rgb);
        [DllImport(Lib)] public static extern int swr_present_rgb_async(IntPtr ctx, Vector3* rgb, out ulong ticket);
        [DllImport(Lib)] public static extern int swr_present_wait(IntPtr ctx, ulong ticket);
        [DllImport(Lib)] public static extern int swr_flatten_rgb_device(IntPtr ctx, IntPtr deviceRgb);
        [DllImport(Lib)] public static extern int swr_flatten_rgb_device_async(IntPtr ctx, IntPtr deviceRgb);
        [DllImport(Lib)] public static extern int swr_resolved_size(IntPtr ctx, int kx, int ky, out int outWidth, out int outRows);
        [DllImport(Lib)] public static extern int swr_readback_rgb_resolved(IntPtr ctx, int kx, int ky, Vector3* rgb);
        [DllImport(Lib)] public static extern int swr_present_rgb_resolved_async(IntPtr ctx, int kx, int ky, Vector3* rgb, out ulong ticket);
        [DllImport(Lib)] public static extern int swr_resolve_rgb_device(IntPtr ctx, int kx, int ky, IntPtr deviceRgb);
        [DllImport(Lib)] public static extern int swr_resolve_rgb_device_async(IntPtr ctx, int kx, int ky, IntPtr deviceRgb);
        [DllImport(Lib)] public static extern int swr_present8_size(IntPtr ctx, int kx, int ky, int bpp, out int outWidth, out int outRows, out nuint outBytes);
        [DllImport(Lib)] public static extern int swr_readback_rgb8(IntPtr ctx, int kx, int ky, int bpp, byte* bytes);
        [DllImport(Lib)] public static extern int swr_present_rgb8_async(IntPtr ctx, int kx, int ky, int bpp, byte* bytes, out ulong ticket);
        [DllImport(Lib)] public static extern int swr_resolve_rgb8_device(IntPtr ctx, int kx, int ky, int bpp, IntPtr deviceBytes);
        [DllImport(Lib)] public static extern int swr_resolve_rgb8_device_async(IntPtr ctx, int kx, int ky, int bpp, IntPtr deviceBytes);
        [DllImport(Lib)] public static extern int swr_replay_count(IntPtr ctx, out ulong replays);
        [DllImport(Lib)] public static extern int swr_sync_count(IntPtr ctx, out ulong syncs);
        [DllImport(Lib)] public static extern int swr_host_register(IntPtr ctx, void* ptr, nuint bytes);
        [DllImport(Lib)] public static extern int swr_host_unregister(IntPtr ctx, void* ptr);
        [DllImport(Lib)] public static extern int swr_upload(IntPtr ctx, Vector4* colorRgba, float* depth);
        [DllImport(Lib)] public static extern int swr_color_device_ptr(IntPtr ctx, out IntPtr devicePtr);
        [DllImport(Lib)] public static extern int swr_depth_device_ptr(IntPtr ctx, out IntPtr devicePtr);
        [DllImport(Lib)] public static extern int swr_texture_create(IntPtr ctx, byte* rgba8, int width, int height, out IntPtr texture);
        [DllImport(Lib)] public static extern int swr_texture_destroy(IntPtr ctx, IntPtr texture);
        [DllImport(Lib)] public static extern int swr_texture_set_filter(IntPtr ctx, IntPtr texture, int bilinear);
        [DllImport(Lib)] public static extern int swr_texture_sample(IntPtr ctx, IntPtr texture, Vector2* uv, int n, Vector4* outRgba);
        [DllImport(Lib)] public static extern int swr_texture_create_target(IntPtr ctx, int width, int height, out IntPtr texture);
        [DllImport(Lib)] public static extern int swr_texture_update_from_frame(IntPtr ctx, IntPtr texture, IntPtr sourceCtx, int kx, int ky, int alphaMode);
        [DllImport(Lib)] public static extern int swr_texture_readback(IntPtr ctx, IntPtr texture, byte* rgba8);
        [DllImport(Lib)] public static extern int swr_texture_create_depth(IntPtr ctx, float* depthOrNull, int width, int height, out IntPtr texture);
        [DllImport(Lib)] public static extern int swr_texture_update_from_depth(IntPtr ctx, IntPtr texture, IntPtr sourceCtx, int kx, int ky, int reduce);
        [DllImport(Lib)] public static extern int swr_texture_readback_depth(IntPtr ctx, IntPtr texture, float* depth);
        // (TextureNative.ReadDepth calls this: a test counts TextureNative's uses of swr_texture_readback by that prefix)
        public static int TextureReadDepth(IntPtr ctx, IntPtr texture, float* depth) => swr_texture_readback_depth(ctx, texture, depth);
        [DllImport(Lib)] public static extern int swr_texture_sample_depth(IntPtr ctx, IntPtr texture, float* uvRef, int n, float* outDepthShadow);
        [DllImport(Lib)] public static extern int swr_texture_format(IntPtr ctx, IntPtr texture, out int format);
        // mip chains (build-defined, swr.h): levels 1 .. L - 1 made on the GPU, sampled by user and post programs
        [DllImport(Lib)] public static extern int swr_texture_generate_mipmaps(IntPtr ctx, IntPtr texture);
        [DllImport(Lib)] public static extern int swr_texture_levels(IntPtr ctx, IntPtr texture, out int levels);
        [DllImport(Lib)] public static extern int swr_texture_level_size(IntPtr ctx, IntPtr texture, int level, out int width, out int height);
        [DllImport(Lib)] public static extern int swr_texture_readback_level(IntPtr ctx, IntPtr texture, int level, byte* rgba8);
        public static int TextureReadLevel(IntPtr ctx, IntPtr texture, int level, byte* rgba8) => swr_texture_readback_level(ctx, texture, level, rgba8);
        [DllImport(Lib)] public static extern int swr_texture_sample_lod(IntPtr ctx, IntPtr texture, float* uvLod, int n, float* outRgba);
        [DllImport(Lib)] public static extern int swr_texture_lod(IntPtr ctx, IntPtr texture, float* grads, int n, float* outLod);
        // cube maps (build-defined, swr.h): six faces in one n x 6 n texture, looked up by direction in user and post programs
        [DllImport(Lib)] public static extern int swr_texture_create_cube(IntPtr ctx, byte* rgba8OrNull, int n, out IntPtr texture);
        [DllImport(Lib)] public static extern int swr_texture_create_cube_depth(IntPtr ctx, float* depthOrNull, int n, out IntPtr texture);
        [DllImport(Lib)] public static extern int swr_texture_is_cube(IntPtr ctx, IntPtr texture, out int nOr0);
        [DllImport(Lib)] public static extern int swr_texture_update_face_from_frame(IntPtr ctx, IntPtr texture, int face, IntPtr sourceCtx, int kx, int ky, int alphaMode);
        [DllImport(Lib)] public static extern int swr_texture_update_face_from_depth(IntPtr ctx, IntPtr texture, int face, IntPtr sourceCtx, int kx, int ky, int reduce);
        [DllImport(Lib)] public static extern int swr_texture_update_face_from_post(IntPtr ctx, IntPtr texture, int face, IntPtr sourceCtx, int postId, int kx, int ky, int alphaMode);
        [DllImport(Lib)] public static extern int swr_texture_readback_face(IntPtr ctx, IntPtr texture, int face, int level, void* texels);
        [DllImport(Lib)] public static extern int swr_cube_face_view(int face, float* eye, float* view);
        [DllImport(Lib)] public static extern int swr_texture_cube_face(IntPtr ctx, float* dirs, int n, int* outFace, float* outSt);
        [DllImport(Lib)] public static extern int swr_texture_sample_cube(IntPtr ctx, IntPtr texture, float* dirLod, int n, float* outRgba);
        [DllImport(Lib)] public static extern int swr_texture_sample_cube_depth(IntPtr ctx, IntPtr texture, float* dirRef, int n, float* outDepthShadow);
        [DllImport(Lib)] public static extern int swr_mesh_create(IntPtr ctx, Shaders.VertexInput* vertices, int nVertices, ushort* indices, int nIndices, out IntPtr mesh);
        [DllImport(Lib)] public static extern int swr_mesh_destroy(IntPtr ctx, IntPtr mesh);
        // deforming meshes (include/swr.h "DEFORMING MESHES"): a retained mesh rewritten on the GPU
        [DllImport(Lib)] public static extern int swr_mesh_create_like(IntPtr ctx, IntPtr src, out IntPtr mesh);
        [DllImport(Lib)] public static extern int swr_mesh_readback(IntPtr ctx, IntPtr mesh, Shaders.VertexInput* outVertices);
        [DllImport(Lib)] public static extern int swr_mesh_blend(IntPtr ctx, IntPtr dst, IntPtr a, IntPtr b, float t);
        [DllImport(Lib)] public static extern int swr_mesh_set_skin(IntPtr ctx, IntPtr src, ushort* joints4, float* weights4);
        [DllImport(Lib)] public static extern int swr_mesh_skin(IntPtr ctx, IntPtr dst, IntPtr src, Matrix4x4* palette, int nJoints);
        // skeletal animation (include/swr.h "SKELETAL ANIMATION"): clips to palettes on the GPU, one skin launch for a crowd
        [DllImport(Lib)] public static extern int swr_skeleton_create(IntPtr ctx, int nNodes, int* parent, Matrix4x4* restLocal, float* restT, float* restR, float* restS, int nJoints, int* jointNode, Matrix4x4* inverseBind, out IntPtr skeleton);
        [DllImport(Lib)] public static extern int swr_skeleton_destroy(IntPtr ctx, IntPtr skeleton);
        [DllImport(Lib)] public static extern int swr_skeleton_add_clip(IntPtr ctx, IntPtr skeleton, SwrAnimChannel* channels, int nChannels, out int clipIndex);
        [DllImport(Lib)] public static extern int swr_pose_set_create(IntPtr ctx, int nInstances, int nJoints, out IntPtr set);
        [DllImport(Lib)] public static extern int swr_pose_set_destroy(IntPtr ctx, IntPtr set);
        [DllImport(Lib)] public static extern int swr_pose_set_sample(IntPtr ctx, IntPtr set, IntPtr skeleton, SwrPoseRequest* requests, int n);
        [DllImport(Lib)] public static extern int swr_pose_set_upload(IntPtr ctx, IntPtr set, int first, int n, Matrix4x4* palettes);
        [DllImport(Lib)] public static extern int swr_pose_set_readback(IntPtr ctx, IntPtr set, Matrix4x4* outPalettes);
        [DllImport(Lib)] public static extern int swr_mesh_skin_batch(IntPtr ctx, int n, IntPtr* dst, IntPtr* src, IntPtr set, int* instance);
        [DllImport(Lib)] public static extern int swr_set_state(IntPtr ctx, float nearClip, float farClip, int debugMode);
        [DllImport(Lib)] public static extern int swr_initialize_tile_locks(IntPtr ctx, int width, int height);
        [DllImport(Lib)] public static extern int swr_render_mesh(IntPtr ctx, IntPtr mesh, Matrix4x4* model, Matrix4x4* view, Matrix4x4* projection, int program, SwrUniforms* uniforms, IntPtr texture, int cullMode, int depthTest, int blendMode);
        [DllImport(Lib)] public static extern int swr_render_mesh_arrays(IntPtr ctx, Shaders.VertexInput* vertices, int nVertices, ushort* indices, int nIndices, Matrix4x4* model, Matrix4x4* view, Matrix4x4* projection, int program, SwrUniforms* uniforms, IntPtr texture, int cullMode, int depthTest, int blendMode);
        [DllImport(Lib)] public static extern int swr_mesh_bounds(IntPtr ctx, IntPtr mesh, Vector4* centerRadius);
        [DllImport(Lib)] public static extern int swr_is_sphere_in_frustum(IntPtr ctx, Vector4* centerRadius, Matrix4x4* model, Matrix4x4* view, Matrix4x4* projection, out int inside);
        [DllImport(Lib)] public static extern int swr_render_mesh_culled(IntPtr ctx, IntPtr mesh, Matrix4x4* model, Matrix4x4* view, Matrix4x4* projection, int program, SwrUniforms* uniforms, IntPtr texture, int cullMode, int depthTest, int blendMode);
        [DllImport(Lib)] public static extern int swr_flush(IntPtr ctx);
        [DllImport(Lib)] public static extern int swr_set_pipelining(IntPtr ctx, int mode);
        [DllImport(Lib)] public static extern int swr_get_pipelining(IntPtr ctx, out int mode);
        [DllImport(Lib)] public static extern int swr_sync(IntPtr ctx);
        [DllImport(Lib)] public static extern int swr_interpolate(IntPtr ctx, float* verts60, float* w, int n, int interpolate, float* outRecords);
        [DllImport(Lib)] public static extern int swr_get_stats(IntPtr ctx, out SwrStats stats);
        [DllImport(Lib)] public static extern int swr_reset_stats(IntPtr ctx);
        [DllImport(Lib)] public static extern int swr_profile_enable(IntPtr ctx, int on);
        [DllImport(Lib)] public static extern int swr_profile_get(IntPtr ctx, out SwrProfile profile);
        [DllImport(Lib)] public static extern int swr_profile_reset(IntPtr ctx);
        [DllImport(Lib)] public static extern int swr_profile_raster_samples(IntPtr ctx, float* outMs, int capacity, out int n);
        [DllImport(Lib)] public static extern int swr_device_name(IntPtr ctx, byte* buf, int buflen);
        [DllImport(Lib)] public static extern int swr_selftest_division(IntPtr ctx, ulong samples, ulong seed, ulong* out8);
        [DllImport(Lib)] public static extern int swr_debug_counters(IntPtr ctx, ulong* out8);
        // user fragment programs (a Shaders.FragmentShader restated in C++, see ShaderMap.Register)
        [DllImport(Lib)] public static extern int swr_program_create(IntPtr ctx, byte* fragmentSource, out int programId);
        [DllImport(Lib)] public static extern int swr_program_destroy(IntPtr ctx, int programId);
        [DllImport(Lib)] public static extern int swr_program_set_constants(IntPtr ctx, int programId, float* values, int n);
        [DllImport(Lib)] public static extern int swr_program_set_texture(IntPtr ctx, int programId, int slot, IntPtr texture);
        [DllImport(Lib)] public static extern int swr_program_validate(byte* fragmentSource, byte* log, int logLen);
        [DllImport(Lib)] public static extern int swr_program_create_vf(IntPtr ctx, byte* vertexSource, byte* fragmentSource, out int programId);
        [DllImport(Lib)] public static extern int swr_program_validate_vf(byte* vertexSource, byte* fragmentSource, byte* log, int logLen);
        // post-process programs (swr.h: POST-PROCESS programs); format: 0 = three floats, 3 = RGB8, 4 = RGBX8
        [DllImport(Lib)] public static extern int swr_post_create(IntPtr ctx, byte* source, out int postId);
        [DllImport(Lib)] public static extern int swr_post_destroy(IntPtr ctx, int postId);
        [DllImport(Lib)] public static extern int swr_post_set_constants(IntPtr ctx, int postId, float* values, int n);
        [DllImport(Lib)] public static extern int swr_post_validate(byte* source, byte* log, int logLen);
        [DllImport(Lib)] public static extern int swr_post_size(IntPtr ctx, int kx, int ky, int format, out int outWidth, out int outRows, out nuint outBytes);
        [DllImport(Lib)] public static extern int swr_readback_post(IntPtr ctx, int postId, int kx, int ky, int format, void* bytes);
        [DllImport(Lib)] public static extern int swr_present_post_async(IntPtr ctx, int postId, int kx, int ky, int format, void* bytes, out ulong ticket);
        [DllImport(Lib)] public static extern int swr_post_device(IntPtr ctx, int postId, int kx, int ky, int format, IntPtr deviceBytes);
        [DllImport(Lib)] public static extern int swr_post_device_async(IntPtr ctx, int postId, int kx, int ky, int format, IntPtr deviceBytes);
        // post programs and textures (swr.h: TEXTURES): four slots per program, and a pass's result into a texture
        [DllImport(Lib)] public static extern int swr_post_set_texture(IntPtr ctx, int postId, int slot, IntPtr texture);
        [DllImport(Lib)] public static extern int swr_texture_update_from_post(IntPtr ctx, IntPtr texture, IntPtr sourceCtx, int postId, int kx, int ky, int alphaMode);
        [DllImport(Lib)] public static extern int swr_raycast(IntPtr ctx, SwrRay* rays, int nRays, SwrRayTarget* targets, int nTargets, int flags, SwrRayHit* hits);
        [DllImport(Lib)] public static extern int swr_raycast_nearest(IntPtr ctx, SwrRay* rays, int nRays, SwrRayTarget* targets, int nTargets, int flags, SwrRayHit* hits);
        [DllImport(Lib)] public static extern int swr_character_ray_counts(SwrCharacterParams* p, out int verticalSteps, out int horizontalRays);
        [DllImport(Lib)] public static extern int swr_character_update(IntPtr ctx, SwrCharacterParams* p, SwrCharacter* chars, SwrCharacterInput* inputs, int n, float deltaTime, float* ring, int nRing, SwrRayTarget* targets, int nTargets, int flags, SwrCharacterTrace* trace);
    }

    // ---------------------------------------------------------------- numerics probe ----
    // Nothing in the reference's repository pins how .NET 9 evaluates Vector4.Transform / Vector4.Lerp (with fused multiply-adds or
    // without) and Vector3.Dot (in which order the lanes are summed), and a third of a real frame's depth words depend on the first
    // question (DESIGN.md section 3).  The three fused-or-not questions (Transform, TransformNormal, Lerp) and the dot order are
    // modelled INDEPENDENTLY: Lerp x dot order picks one of six builds (libswr_hip.so = unfused + sequential, _fma, _dotpw,
    // _fma_dotpw, _dpps, _fma_dpps), Transform / TransformNormal are run-time flags of the context (swr_set_transform_fma).  At
    // start-up the operations are evaluated with the RUNNING System.Numerics on operands on which the models give different float32
    // bits; the library built for the observed (Lerp, Dot) model is the one `swr_hip` resolves to and the context gets the observed
    // Transform flags: all 24 combinations are served.  Only a bit pattern that is NEITHER model's throws.
    public static class NumericsProbe
    {
        // <generated by tools/make_numerics_probe.py -- do not edit; tests/test_abi.py compares with csharp/numerics_probe.json>
        const uint LerpA = 0xC00CEF08u, LerpB = 0xBED29EFEu, LerpT = 0x3F478017u, LerpUnfused = 0xBF4E7C50u, LerpFused = 0xBF4E7C4Fu;
        static readonly uint[] TransformV = { 0xC06E43E7u, 0xC00C65BDu, 0x3EF222FCu, 0xBF9FF980u }, TransformColumn = { 0x3FA4C6C1u, 0x3F79740Cu, 0x3FC9D8E3u, 0xC06C7478u };
        const uint TransformUnfused = 0xBFC88EB0u, TransformFused = 0xBFC88EACu;
        static readonly uint[] TransformNormalN = { 0x404E9543u, 0xBE0E5810u, 0x3FC0BF7Cu }, TransformNormalColumn = { 0x3F68F07Eu, 0x3EE1EC4Bu, 0xC03AC7F0u };
        const uint TransformNormalUnfused = 0xBFC26DE8u, TransformNormalFused = 0xBFC26DE7u;
        static readonly uint[] DotA = { 0xC0230FD7u, 0x3FC580AFu, 0x3F8C55D4u }, DotB = { 0xC02E1034u, 0x4069FD33u, 0x3FE786D7u };
        const uint DotSequential = 0x4168DCA9u, DotShuffle = 0x4168DCA8u;
        static readonly uint[] DotZeroA = { 0x80000000u, 0x80000000u, 0x80000000u }, DotZeroB = { 0x3F800000u, 0x3F800000u, 0x3F800000u };
        const uint DotZeroSequential = 0x80000000u, DotZeroDpps = 0x00000000u;
        // </generated>

        // Vector3.Cross (Physics.cs:153,170): x = a.Y * b.Z - a.Z * b.Y with two rounded products, or fma(-a.Z, b.Y, a.Y * b.Z) -- the
        // operands were found by a seeded search (exact rational arithmetic); the flag goes into every raycast call (SWR_RAY_CROSS_FUSED)
        static readonly uint[] CrossA = { 0xC07D4DDEu, 0x4024780Du, 0x4018197Cu }, CrossB = { 0xBE8356A4u, 0xBFC9B1DEu, 0xBFE2E465u };
        const uint CrossUnfused = 0xBF4F7838u, CrossFused = 0xBF4F7839u;

        static volatile uint salt = 0;      // read at run time, so that the JIT cannot fold the probe expressions at compile time
        static float F(uint bits) => BitConverter.UInt32BitsToSingle(bits ^ salt);
        static uint B(float f) => BitConverter.SingleToUInt32Bits(f);

        /// The running System.Numerics in the terms of swr_numerics_mode (lerpFused = *fma, dotOrder) and of swr_set_transform_fma
        /// (transformFused, transformNormalFused); throws on a bit pattern that neither model of an operation produces.
        [MethodImpl(MethodImplOptions.NoInlining)]
        public static (int lerpFused, int transformFused, int transformNormalFused, int dotOrder) Observe()
        {
            uint lerp = B(Vector4.Lerp(new Vector4(F(LerpA)), new Vector4(F(LerpB)), F(LerpT)).X);
            var m = new Matrix4x4(F(TransformColumn[0]), 0, 0, 0, F(TransformColumn[1]), 0, 0, 0, F(TransformColumn[2]), 0, 0, 0, F(TransformColumn[3]), 0, 0, 0);
            uint tr = B(Vector4.Transform(new Vector4(F(TransformV[0]), F(TransformV[1]), F(TransformV[2]), F(TransformV[3])), m).X);
            var mn = new Matrix4x4(F(TransformNormalColumn[0]), 0, 0, 0, F(TransformNormalColumn[1]), 0, 0, 0, F(TransformNormalColumn[2]), 0, 0, 0, 0, 0, 0, 1);
            uint tn = B(Vector3.TransformNormal(new Vector3(F(TransformNormalN[0]), F(TransformNormalN[1]), F(TransformNormalN[2])), mn).X);
            uint dot = B(Vector3.Dot(new Vector3(F(DotA[0]), F(DotA[1]), F(DotA[2])), new Vector3(F(DotB[0]), F(DotB[1]), F(DotB[2]))));
            uint dz = B(Vector3.Dot(new Vector3(F(DotZeroA[0]), F(DotZeroA[1]), F(DotZeroA[2])), new Vector3(F(DotZeroB[0]), F(DotZeroB[1]), F(DotZeroB[2]))));
            int lerpFused = lerp == LerpFused ? 1 : lerp == LerpUnfused ? 0 : -1;
            int trFused = tr == TransformFused ? 1 : tr == TransformUnfused ? 0 : -1;
            int tnFused = tn == TransformNormalFused ? 1 : tn == TransformNormalUnfused ? 0 : -1;
            if (lerpFused < 0 || trFused < 0 || tnFused < 0)
                throw new NotSupportedException($"System.Numerics model not built: Lerp -> 0x{lerp:X8}, Transform -> 0x{tr:X8}, TransformNormal -> 0x{tn:X8} (see csharp/numerics_probe.json)");
            int order;
            if (dot == DotShuffle) order = 2;
            else if (dot == DotSequential) order = dz == DotZeroDpps ? 1 : dz == DotZeroSequential ? 0 : -1;
            else order = -1;
            if (order < 0) throw new NotSupportedException($"System.Numerics model not built: Dot -> 0x{dot:X8} / 0x{dz:X8} (see csharp/numerics_probe.json)");
            return (lerpFused, trFused, tnFused, order);
        }

        /// SWR_RAY_CROSS_FUSED (0x100) when the running Vector3.Cross fuses its second product, 0 when it rounds both, -1 when the
        /// bits are neither model's (PhysicsNative then refuses to run: only ray queries depend on it).
        [MethodImpl(MethodImplOptions.NoInlining)]
        public static int ObserveCrossFlag()
        {
            uint cross = B(Vector3.Cross(new Vector3(F(CrossA[0]), F(CrossA[1]), F(CrossA[2])), new Vector3(F(CrossB[0]), F(CrossB[1]), F(CrossB[2]))).X);
            return cross == CrossFused ? 0x100 : cross == CrossUnfused ? 0 : -1;
        }

        /// File name of the build that models the running System.Numerics' Lerp and Dot (six builds: every combination exists).
        public static string SelectLibrary()
        {
            var (lerpFused, _, _, order) = Observe();
            string suffix = (lerpFused == 1 ? "_fma" : "") + (order == 2 ? "_dotpw" : order == 1 ? "_dpps" : "");
            return "libswr_hip" + suffix + ".so";
        }

        /// Makes every [DllImport("swr_hip")] of this assembly load the selected build; checks that the library agrees.
        public static void Install()
        {
            string file = SelectLibrary();
            NativeLibrary.SetDllImportResolver(typeof(NumericsProbe).Assembly, (name, assembly, path) =>
                name == "swr_hip" ? NativeLibrary.Load(System.IO.Path.Combine(AppContext.BaseDirectory, file)) : IntPtr.Zero);
            var (lerpFused, _, _, order) = Observe();
            if (Native.swr_numerics_mode(out int libFma, out int libOrder) != 0 || libFma != lerpFused || libOrder != order)
                throw new InvalidOperationException($"{file} was built for fma={libFma}, dot={libOrder}; the probe observed fma={lerpFused}, dot={order}");
        }

        /// The run-time half of the model: the observed Transform / TransformNormal flags go to the context (after swr_create).
        public static void Configure(IntPtr ctx)
        {
            var (_, trFused, tnFused, _) = Observe();
            if (Native.swr_set_transform_fma(ctx, trFused, tnFused) != 0) throw new InvalidOperationException("swr_set_transform_fma failed");
        }
    }

    // ---------------------------------------------------------------- context ----
    public static class SwrContext
    {
        static IntPtr ctx;
        static readonly object createLock = new object();

        public static IntPtr Handle
        {
            get
            {
                if (ctx != IntPtr.Zero) return ctx;
                lock (createLock)
                {
                    if (ctx != IntPtr.Zero) return ctx;
                    NumericsProbe.Install();                          // before the first P/Invoke: picks the build that models this .NET's System.Numerics
                    if (Native.swr_abi_version() != 3) throw new InvalidOperationException("libswr_hip.so: ABI version mismatch");
                    int rc = Native.swr_create(0, out IntPtr c);       // one context drives one GPU; there is NO CPU fallback
                    if (rc != 0) throw new InvalidOperationException($"swr_create failed ({rc}): {Marshal.PtrToStringAnsi(Native.swr_last_error(IntPtr.Zero))}");
                    NumericsProbe.Configure(c);                       // Transform / TransformNormal fused or not: run-time flags of the context
                    ctx = c;
                    return ctx;
                }
            }
        }

        // status codes of swr.h: -1 maps to the reference's own exception type (Rasterizer.cs:71-74)
        public static void Check(int rc)
        {
            if (rc == 0) return;
            string msg = Marshal.PtrToStringAnsi(Native.swr_last_error(ctx)) ?? "";
            if (rc == -1 && msg.Contains("index out of range")) throw new IndexOutOfRangeException(msg);
            if (rc == -1) throw new ArgumentException(msg);
            if (rc == -3) throw new OutOfMemoryException(msg);
            throw new InvalidOperationException($"swr error {rc}: {msg}");
        }
    }

    // ---------------------------------------------------------------- Rasterizer ----
    public static partial class Rasterizer
    {
        // Retained device copies of ModelLoader meshes (Mesh.Vertices / Mesh.Indices, ModelLoader.cs:45-47), keyed by the
        // Mesh object: uploaded on first use, freed with the Mesh.  The array overload below cannot retain anything
        // (Renderer.cs:452-453 passes a fresh ToArray() copy every frame) and uploads per call.
        static readonly ConditionalWeakTable<Mesh, MeshHandle> retained = new ConditionalWeakTable<Mesh, MeshHandle>();

        sealed class MeshHandle
        {
            public IntPtr Ptr;
            ~MeshHandle() { if (Ptr != IntPtr.Zero) Native.swr_mesh_destroy(SwrContext.Handle, Ptr); }
        }

        /// Makes `handle` (a retained mesh made by swr_mesh_create_like) the device copy of `mesh`: freed with the Mesh object.
        internal static void Adopt(Mesh mesh, IntPtr handle)
        {
            retained.Remove(mesh);
            retained.Add(mesh, new MeshHandle { Ptr = handle });
        }

        /// The device copy of a ModelLoader mesh, uploaded on first use (draws and PhysicsNative's ray queries share it).
        internal static unsafe IntPtr Retain(Mesh mesh)
        {
            IntPtr ctx = SwrContext.Handle;
            return retained.GetValue(mesh, m =>
            {
                var va = m.Vertices.ToArray();
                var ia = m.Indices.ToArray();
                var mh = new MeshHandle();
                fixed (Shaders.VertexInput* v = va)
                fixed (ushort* idx = ia)
                    SwrContext.Check(Native.swr_mesh_create(ctx, v, va.Length, idx, ia.Length, out mh.Ptr));
                return mh;
            }).Ptr;
        }

        /// Rasterizer.RenderMesh with the reference's exact signature and defaults (Rasterizer.cs:163-174).
        public static unsafe void RenderMesh(
            MainWindow window,
            Shaders.VertexInput[] vertices,
            ushort[] indices,
            Matrix4x4 model,
            Matrix4x4 view,
            Matrix4x4 projection,
            Shaders.VertexShader vertexShader,
            Shaders.FragmentShader fragmentShader,
            CullMode cullMode = CullMode.Back,
            DepthTest depthTest = DepthTest.LessEqual,
            BlendMode blendMode = BlendMode.Alpha)
        {
            if (window.RenderWidth <= 0 || window.RenderHeight <= 0) return;                    // Rasterizer.cs:176
            if (!ShaderMap.TryResolve(vertexShader, fragmentShader, out SwrProgram program, out SwrUniforms uniforms, out IntPtr texture))
            {
                // a shader pair the backend has no built-in program for: the reference's own CPU path
                RenderMeshManaged(window, vertices, indices, model, view, projection, vertexShader, fragmentShader, cullMode, depthTest, blendMode);
                return;
            }
            IntPtr ctx = SwrContext.Handle;
            SwrContext.Check(Native.swr_initialize_tile_locks(ctx, window.RenderWidth, window.RenderHeight));   // :178 (argument check)
            SwrContext.Check(Native.swr_set_state(ctx, NearClip, FarClip, (int)RenderDebugMode));               // :20-22
            fixed (Shaders.VertexInput* v = vertices)
            fixed (ushort* idx = indices)
            {
                SwrContext.Check(Native.swr_render_mesh_arrays(ctx, v, vertices.Length, idx, indices.Length, &model, &view, &projection,
                                                               (int)program, &uniforms, texture, (int)cullMode, (int)depthTest, (int)blendMode));
            }
        }

        /// Same draw from a retained ModelLoader mesh: no per-frame upload (what Renderer.RenderDust2 can call with `mesh`
        /// instead of `mesh.Vertices.ToArray(), mesh.Indices.ToArray()`); frustumCull folds the
        /// `if (!FrustumCuller.IsSphereInFrustum(mesh.SphereBounds, ...)) return;` of Renderer.cs:446 into the GPU batch.
        public static unsafe void RenderMesh(
            MainWindow window,
            Mesh mesh,
            Matrix4x4 model,
            Matrix4x4 view,
            Matrix4x4 projection,
            Shaders.VertexShader vertexShader,
            Shaders.FragmentShader fragmentShader,
            CullMode cullMode = CullMode.Back,
            DepthTest depthTest = DepthTest.LessEqual,
            BlendMode blendMode = BlendMode.Alpha,
            bool frustumCull = false)
        {
            if (window.RenderWidth <= 0 || window.RenderHeight <= 0) return;
            if (!ShaderMap.TryResolve(vertexShader, fragmentShader, out SwrProgram program, out SwrUniforms uniforms, out IntPtr texture))
            {
                RenderMeshManaged(window, mesh.Vertices.ToArray(), mesh.Indices.ToArray(), model, view, projection, vertexShader, fragmentShader, cullMode, depthTest, blendMode);
                return;
            }
            IntPtr ctx = SwrContext.Handle;
            IntPtr h = Retain(mesh);
            SwrContext.Check(Native.swr_set_state(ctx, NearClip, FarClip, (int)RenderDebugMode));
            int rc = frustumCull
                ? Native.swr_render_mesh_culled(ctx, h, &model, &view, &projection, (int)program, &uniforms, texture, (int)cullMode, (int)depthTest, (int)blendMode)
                : Native.swr_render_mesh(ctx, h, &model, &view, &projection, (int)program, &uniforms, texture, (int)cullMode, (int)depthTest, (int)blendMode);
            SwrContext.Check(rc);
        }
    }

    // ---------------------------------------------------------------- deforming meshes ----
    // A pose of a ModelLoader mesh on the GPU (build-defined, DESIGN.md section 28).  The reference animates by swapping whole key
    // frames (Model.PlayAnimation, ModelLoader.cs:331-348) and shoots at the meshes it draws (Renderer.cs:172-216,503-541): a
    // DeformedMesh is a retained copy of a mesh whose vertices are rewritten in place -- the blend of two key frames, or a skinned
    // bind pose -- so that Rasterizer.RenderMesh(window, pose.Target, ...) and PhysicsNative.Raycast(..., pose.Target, ...) see the
    // same vertices.  Target is an ordinary Mesh object whose device copy this class owns; its managed Vertices are the bind pose.
    public sealed unsafe class DeformedMesh
    {
        public readonly Mesh Source;          // the mesh whose device copy was duplicated (and that carries the skin attributes)
        public readonly Mesh Target;          // draw and shoot at this one
        readonly IntPtr dst;

        public DeformedMesh(Mesh source, Mesh target)
        {
            Source = source; Target = target;
            SwrContext.Check(Native.swr_mesh_create_like(SwrContext.Handle, Rasterizer.Retain(source), out dst));
            Rasterizer.Adopt(target, dst);
        }

        /// Target = a * (1 - t) + b * t, every scalar of position, uv, normal and colour (Vector*.Lerp's form; t is not clamped).
        /// a and b are key frames with Source's vertex count: frames i and j of Model.AnimationFrames.
        public void Blend(Mesh a, Mesh b, float t) =>
            SwrContext.Check(Native.swr_mesh_blend(SwrContext.Handle, dst, Rasterizer.Retain(a), Rasterizer.Retain(b), t));

        /// Four joint indices and four weights per vertex of Source, uploaded once.
        public void SetSkin(ushort[] joints4, float[] weights4)
        {
            fixed (ushort* j = joints4)
            fixed (float* w = weights4)
                SwrContext.Check(Native.swr_mesh_set_skin(SwrContext.Handle, Rasterizer.Retain(Source), j, w));
        }

        /// Target = Source skinned by `palette` (one Matrix4x4 per joint: inverse bind * joint world * inverse mesh world, the caller's).
        public void Skin(Matrix4x4[] palette)
        {
            fixed (Matrix4x4* p = palette)
                SwrContext.Check(Native.swr_mesh_skin(SwrContext.Handle, dst, Rasterizer.Retain(Source), p, palette.Length));
        }

        /// targets[k].Target = targets[k].Source skinned by the palette of instances[k] of `set`, all of them in ONE kernel launch: word
        /// for word what Skin gives with that palette.  Two targets may share a Source or an instance.
        public static void SkinBatch(DeformedMesh[] targets, PoseSetNative set, int[] instances)
        {
            if (instances.Length != targets.Length) throw new ArgumentException("one instance per target");
            var d = new IntPtr[Math.Max(targets.Length, 1)];
            var s = new IntPtr[Math.Max(targets.Length, 1)];
            for (int k = 0; k < targets.Length; ++k) { d[k] = targets[k].dst; s[k] = Rasterizer.Retain(targets[k].Source); }
            fixed (IntPtr* pd = d) fixed (IntPtr* ps = s) fixed (int* pi = instances)
                SwrContext.Check(Native.swr_mesh_skin_batch(SwrContext.Handle, targets.Length, pd, ps, set.Handle, pi));
        }

        /// The pose as the device holds it.
        public Shaders.VertexInput[] Read()
        {
            var outv = new Shaders.VertexInput[Source.Vertices.Length];
            fixed (Shaders.VertexInput* v = outv)
                SwrContext.Check(Native.swr_mesh_readback(SwrContext.Handle, dst, v));
            return outv;
        }
    }

    // ---------------------------------------------------------------- skeletal animation ----
    // Build-defined (DESIGN.md section 29; the reference has no skeletal animation): a skeleton with its clips lives on the GPU, a
    // whole crowd is posed there in one call (PoseSetNative.Sample), and every mesh of the crowd is skinned from the pose set in one
    // kernel launch (DeformedMesh.SkinBatch).  Key search, Quaternion.Lerp (the NORMALISED lerp, not a slerp), the S x R x T compose
    // and the hierarchy's products have one definition for every numerics build; only the skinning follows the Transform flags.
    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct SwrAnimChannel            // swr_anim_channel: one glTF animation channel with its sampler
    {
        public int Node;
        public int Path;                           // 0 translation, 1 rotation, 2 scale
        public int Interpolation;                  // 0 STEP, 1 LINEAR (2, CUBICSPLINE, is refused)
        public int NKeys;
        public float* Times;                       // NKeys, non-decreasing
        public float* Values;                      // NKeys x 3 (x 4 for a rotation, xyzw)
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct SwrPoseRequest                   // swr_pose_request (20 bytes)
    {
        public int ClipA;
        public float TimeA;
        public int ClipB;                          // -1: none
        public float TimeB;
        public float Weight;                       // used as it is, not clamped
    }

    /// One channel of a clip in managed arrays (SkeletonNative.AddClip pins them for the call).
    public sealed class AnimationChannel
    {
        public int Node, Path, Interpolation = 1;
        public float[] Times = Array.Empty<float>();
        public float[] Values = Array.Empty<float>();
    }

    public sealed unsafe class SkeletonNative : IDisposable
    {
        internal IntPtr Handle;
        public readonly int NodeCount, JointCount;

        /// parent[i] < i or -1 (several roots are allowed); restT / restS three floats per node, restR four (xyzw); jointNode the
        /// node each joint is.  Matrices are System.Numerics' own layout (row-major, row vectors).
        public SkeletonNative(int[] parent, Matrix4x4[] restLocal, float[] restT, float[] restR, float[] restS, int[] jointNode, Matrix4x4[] inverseBind)
        {
            NodeCount = parent.Length; JointCount = jointNode.Length;
            if (restLocal.Length != NodeCount || restT.Length != 3 * NodeCount || restR.Length != 4 * NodeCount || restS.Length != 3 * NodeCount || inverseBind.Length != JointCount)
                throw new ArgumentException("the skeleton's arrays do not match its node and joint counts");
            fixed (int* p = parent) fixed (Matrix4x4* l = restLocal) fixed (float* t = restT) fixed (float* r = restR) fixed (float* s = restS)
            fixed (int* j = jointNode) fixed (Matrix4x4* b = inverseBind)
                SwrContext.Check(Native.swr_skeleton_create(SwrContext.Handle, NodeCount, p, l, t, r, s, JointCount, j, b, out Handle));
        }

        /// The clip's index.  A load-time call: it may reallocate the skeleton's clips and wait for the device.
        public int AddClip(IReadOnlyList<AnimationChannel> channels)
        {
            var recs = new SwrAnimChannel[Math.Max(channels.Count, 1)];
            var pins = new List<GCHandle>();
            try
            {
                for (int k = 0; k < channels.Count; ++k)
                {
                    var c = channels[k];
                    if (c.Values.Length != c.Times.Length * (c.Path == 1 ? 4 : 3))
                        throw new ArgumentException("a channel's values must hold 3 floats per key (4 for a rotation)");
                    var ht = GCHandle.Alloc(c.Times, GCHandleType.Pinned); pins.Add(ht);
                    var hv = GCHandle.Alloc(c.Values, GCHandleType.Pinned); pins.Add(hv);
                    recs[k] = new SwrAnimChannel { Node = c.Node, Path = c.Path, Interpolation = c.Interpolation, NKeys = c.Times.Length,
                                                   Times = (float*)ht.AddrOfPinnedObject(), Values = (float*)hv.AddrOfPinnedObject() };
                }
                int index;
                fixed (SwrAnimChannel* r = recs)
                    SwrContext.Check(Native.swr_skeleton_add_clip(SwrContext.Handle, Handle, r, channels.Count, out index));
                return index;
            }
            finally { foreach (var h in pins) h.Free(); }
        }

        public void Dispose()
        {
            if (Handle != IntPtr.Zero) Native.swr_skeleton_destroy(SwrContext.Handle, Handle);
            Handle = IntPtr.Zero;
            GC.SuppressFinalize(this);
        }
        ~SkeletonNative() { if (Handle != IntPtr.Zero) Native.swr_skeleton_destroy(SwrContext.Handle, Handle); }
    }

    public sealed unsafe class PoseSetNative : IDisposable
    {
        internal IntPtr Handle;
        public readonly int InstanceCount, JointCount;

        public PoseSetNative(int instances, int joints)
        {
            InstanceCount = instances; JointCount = joints;
            SwrContext.Check(Native.swr_pose_set_create(SwrContext.Handle, instances, joints, out Handle));
        }

        /// Instance i from requests[i], sampled and composed on the GPU; no host wait.
        public void Sample(SkeletonNative skeleton, SwrPoseRequest[] requests)
        {
            fixed (SwrPoseRequest* r = requests)
                SwrContext.Check(Native.swr_pose_set_sample(SwrContext.Handle, Handle, skeleton.Handle, r, requests.Length));
        }

        /// Host-made palettes (JointCount matrices per instance) into instances first, first + 1, ...; no host wait.
        public void Upload(int first, Matrix4x4[] palettes)
        {
            if (palettes.Length % JointCount != 0) throw new ArgumentException("palettes must hold JointCount matrices per instance");
            fixed (Matrix4x4* p = palettes)
                SwrContext.Check(Native.swr_pose_set_upload(SwrContext.Handle, Handle, first, palettes.Length / JointCount, p));
        }

        /// InstanceCount x JointCount matrices as the device holds them.
        public Matrix4x4[] Read()
        {
            var outp = new Matrix4x4[InstanceCount * JointCount];
            fixed (Matrix4x4* p = outp)
                SwrContext.Check(Native.swr_pose_set_readback(SwrContext.Handle, Handle, p));
            return outp;
        }

        public void Dispose()
        {
            if (Handle != IntPtr.Zero) Native.swr_pose_set_destroy(SwrContext.Handle, Handle);
            Handle = IntPtr.Zero;
            GC.SuppressFinalize(this);
        }
        ~PoseSetNative() { if (Handle != IntPtr.Zero) Native.swr_pose_set_destroy(SwrContext.Handle, Handle); }
    }

    // ---------------------------------------------------------------- Physics ----
    // Physics.Raycast on retained meshes (Physics.cs:19-179).  The reference copies the mesh, transforms every vertex and normal
    // and walks every triangle PER CALL; here the mesh stays in HBM and a call carries rays and matrices only.  Matrix4x4.Invert stays
    // on this side (its numerics are .NET's own): a model that does not invert is the reference's `return false`.
    public static class PhysicsNative
    {
        static int crossFlag = -1;
        static int CrossFlag
        {
            get
            {
                if (crossFlag < 0 && (crossFlag = NumericsProbe.ObserveCrossFlag()) < 0)
                    throw new NotSupportedException("System.Numerics model not built: Vector3.Cross is neither of the two modelled forms (DESIGN.md section 3)");
                return crossFlag;
            }
        }
        internal static int CrossFlagValue => CrossFlag;

        /// Physics.Raycast(rayOrigin, rayDirection, mesh.Vertices.ToArray(), mesh.Indices.ToArray(), model, out ..., faceMask) without the copies.
        public static unsafe bool Raycast(Vector3 rayOrigin, Vector3 rayDirection, Mesh mesh, Matrix4x4 model,
                                          out float hitDistance, out Vector3 hitPoint, out Vector3 hitNormal,
                                          RaycastFaceMask faceMask = RaycastFaceMask.IgnoreBackfaces)
        {
            hitDistance = float.MaxValue; hitPoint = Vector3.Zero; hitNormal = Vector3.Zero;
            if (!Matrix4x4.Invert(model, out var invModel)) return false;                       // Physics.cs:30-36
            var ray = new SwrRay { Origin = rayOrigin, Direction = rayDirection };
            var target = new SwrRayTarget { Mesh = Rasterizer.Retain(mesh), Model = model, NormalMatrix = Matrix4x4.Transpose(invModel) };
            SwrRayHit hit;
            SwrContext.Check(Native.swr_raycast(SwrContext.Handle, &ray, 1, &target, 1, (int)faceMask | CrossFlag, &hit));
            if (hit.Found == 0) return false;
            hitDistance = hit.Distance; hitPoint = hit.Point; hitNormal = hit.Normal;
            return true;
        }

        /// One call for a whole loop nest of the callers (CharacterController.MoveWithSlide, :308-389: every ray of a slide attempt
        /// against every mesh of every collision model): hits[i] = the nearest hit of rays[i] over `targets` in their order under
        /// `if (hit && distance < best)`; hits[i].Found == 0 where it misses everything.  Targets whose model does not invert are
        /// left out by the caller (MakeTarget returns false).
        public static unsafe void RaycastNearest(SwrRay[] rays, SwrRayTarget[] targets, SwrRayHit[] hits,
                                                 RaycastFaceMask faceMask = RaycastFaceMask.IgnoreBackfaces)
        {
            if (hits.Length < rays.Length) throw new ArgumentException("hits is shorter than rays");
            fixed (SwrRay* r = rays)
            fixed (SwrRayTarget* t = targets)
            fixed (SwrRayHit* h = hits)
                SwrContext.Check(Native.swr_raycast_nearest(SwrContext.Handle, r, rays.Length, t, targets.Length, (int)faceMask | CrossFlag, h));
        }

        public static bool MakeTarget(Mesh mesh, Matrix4x4 model, out SwrRayTarget target)
        {
            target = default;
            if (!Matrix4x4.Invert(model, out var invModel)) return false;
            target = new SwrRayTarget { Mesh = Rasterizer.Retain(mesh), Model = model, NormalMatrix = Matrix4x4.Transpose(invModel) };
            return true;
        }
    }

    // ---------------------------------------------------------------- CharacterController ----
    // CharacterController.Update (CharacterController.cs:50-140) in ONE native call: both CheckPlanes, both MoveWithSlide chains and
    // the velocity update run on the GPU without a host round trip between them.  What stays on this side: the ring table
    // (MathF.Cos / MathF.Sin are the C runtime's), Matrix4x4.Invert (a model that does not invert is left out), the flattening of
    // collisionModels, and CamOffset, which only the camera reads.  Properties and defaults are the reference's.
    public class CharacterControllerNative
    {
        public Vector3 Position { get; set; }
        public Vector3 Velocity { get; private set; }
        public bool IsGrounded { get; private set; }
        public bool IsCeiling { get; private set; }
        public bool IsNoClipEnabled { get; set; } = false;

        public Vector3 Gravity { get; set; } = new(0, -14.0f, 0);
        public float Height { get; set; } = 0.5f;
        public float Radius { get; set; } = 0.15f;
        public float StepSize { get; set; } = 0.3f;
        private float ActualStepSize = 0.03f;
        public float MoveSpeed { get; set; } = 5.0f;
        public float JumpForce { get; set; } = 4f;
        public float GroundAcceleration { get; set; } = 3.5f;
        public float AirAcceleration { get; set; } = 0.35f;
        public float MaxAirSpeed { get; set; } = 6.0f;
        public float GroundFriction { get; set; } = 6.0f;
        public float AirControl { get; set; } = 0.2f;
        public Vector3 CamOffset { get; set; } = new(0.0f, 0.15f, 0.0f);
        public SwrCharacterTrace LastTrace;

        private float JumpCooldownTimer = 0f;
        private readonly SwrRayTarget[] targets;       // collisionModels[i] flattened, model-major, mesh-minor
        private float[] ring = Array.Empty<float>();
        private float ringRadius = float.NaN, ringHeight = float.NaN;

        public CharacterControllerNative(Vector3 initialPosition, List<Mesh>[] collisionModels, Matrix4x4[] modelMatrices)
        {
            Position = initialPosition;
            Velocity = Vector3.Zero;
            var flat = new List<SwrRayTarget>();
            if (collisionModels != null && modelMatrices != null && collisionModels.Length == modelMatrices.Length)     // :233, :314
                for (int i = 0; i < collisionModels.Length; i++)
                    foreach (var mesh in collisionModels[i])
                        if (PhysicsNative.MakeTarget(mesh, modelMatrices[i], out var t)) flat.Add(t);
            targets = flat.ToArray();
        }

        SwrCharacterParams Params() => new SwrCharacterParams {
            Gravity = Gravity, Height = Height, Radius = Radius, StepSize = StepSize, MoveSpeed = MoveSpeed, JumpForce = JumpForce,
            GroundAcceleration = GroundAcceleration, AirAcceleration = AirAcceleration, MaxAirSpeed = MaxAirSpeed,
            GroundFriction = GroundFriction, AirControl = AirControl };

        // (cos, sin) of `2 * MathF.PI * hStep / horizontalRays` (:348) with THIS runtime's MathF, once per change of the radius
        unsafe void EnsureRing(SwrCharacterParams p)
        {
            if (Radius == ringRadius && Height == ringHeight) return;
            SwrContext.Check(Native.swr_character_ray_counts(&p, out _, out int horizontalRays));
            ring = new float[2 * horizontalRays];
            for (int hStep = 0; hStep < horizontalRays; hStep++)
            {
                float angle = 2 * MathF.PI * hStep / horizontalRays;
                ring[2 * hStep] = MathF.Cos(angle);
                ring[2 * hStep + 1] = MathF.Sin(angle);
            }
            ringRadius = Radius; ringHeight = Height;
        }

        public unsafe void Update(float DeltaTime, Vector3 MoveInput, bool JumpRequested)
        {
            var p = Params();
            EnsureRing(p);
            var c = new SwrCharacter { Position = Position, Velocity = Velocity, JumpCooldown = JumpCooldownTimer, ActualStepSize = ActualStepSize,
                                       Grounded = IsGrounded ? 1 : 0, Ceiling = IsCeiling ? 1 : 0, NoClip = IsNoClipEnabled ? 1 : 0 };
            var input = new SwrCharacterInput { Move = MoveInput, Jump = JumpRequested ? 1 : 0 };
            SwrCharacterTrace trace;
            fixed (float* r = ring)
            fixed (SwrRayTarget* t = targets)
                SwrContext.Check(Native.swr_character_update(SwrContext.Handle, &p, &c, &input, 1, DeltaTime, r, ring.Length / 2, t, targets.Length,
                                                             PhysicsNative.CrossFlagValue, &trace));
            Position = c.Position; Velocity = c.Velocity; JumpCooldownTimer = c.JumpCooldown; ActualStepSize = c.ActualStepSize;
            IsGrounded = c.Grounded != 0; IsCeiling = c.Ceiling != 0;
            LastTrace = trace;
        }
    }

    // Delegates cannot cross the ABI.  The application has exactly one shader pair (Renderer.VertexShader and the lambda
    // `input => FragmentShader(input, texture)`, Renderer.cs:450-459,830-860): it is recognised by its methods, and the
    // fields it closes over -- the Renderer's light / fog fields (Renderer.cs:39-44) and the captured Texture -- are read
    // through reflection, so Renderer.cs needs no edit.  A fragment method registered with its C++ restatement (Register, the
    // porting guide in INTEGRATION.md) resolves to a user program compiled into the raster kernel; a (vertex, fragment) pair registered
    // with both restatements resolves to a user program with a vertex kernel of its own.  Anything else returns false (managed path).
    public static class ShaderMap
    {
        static readonly BindingFlags Any = BindingFlags.Instance | BindingFlags.Public | BindingFlags.NonPublic;
        static readonly Dictionary<MethodInfo, string> sources = new Dictionary<MethodInfo, string>();
        static readonly Dictionary<MethodInfo, int> programs = new Dictionary<MethodInfo, int>();

        // `method`'s body restated against the contract of swr.h (swr_fragment).  Checked at once (swr_program_validate: a compile
        // error throws ArgumentException with the compiler's log); compiled for the context on first use.  Delegates are matched by
        // their method: register the delegate the application hands to RenderMesh (for Renderer.cs:450-459, the lambda
        // `input => FragmentShader(input, texture)`; its closure's Texture is passed on as the draw's texture).
        public static unsafe void Register(Shaders.FragmentShader method, string source)
        {
            byte[] src = System.Text.Encoding.UTF8.GetBytes(source + "\0");
            byte[] log = new byte[16384];
            int rc;
            fixed (byte* s = src) fixed (byte* l = log) rc = Native.swr_program_validate(s, l, log.Length);
            if (rc == -1) throw new ArgumentException(System.Text.Encoding.UTF8.GetString(log).TrimEnd('\0'));
            if (rc != 0) throw new NotSupportedException($"swr_program_validate: {rc}");
            lock (sources) { sources[method.Method] = source; programs.Remove(method.Method); }
        }

        // A (vertex, fragment) delegate pair restated against the contract of swr.h (swr_vertex + swr_fragment): any Shaders.VertexShader
        // -- a wind displacement, a billboard, a scrolling UV, a second transform -- with the fragment delegate it is used with.  Both
        // halves read the same constants; compile errors name their half (vertex.hip:LINE: / fragment.hip:LINE:).  Matched by the two
        // methods: TryResolve looks for the pair first.
        static readonly Dictionary<(MethodInfo, MethodInfo), (string, string)> pairSources = new Dictionary<(MethodInfo, MethodInfo), (string, string)>();
        static readonly Dictionary<(MethodInfo, MethodInfo), int> pairPrograms = new Dictionary<(MethodInfo, MethodInfo), int>();

        public static unsafe void Register(Shaders.VertexShader vertexMethod, Shaders.FragmentShader fragmentMethod, string vertexSource, string fragmentSource)
        {
            byte[] vsrc = System.Text.Encoding.UTF8.GetBytes(vertexSource + "\0");
            byte[] fsrc = System.Text.Encoding.UTF8.GetBytes(fragmentSource + "\0");
            byte[] log = new byte[16384];
            int rc;
            fixed (byte* v = vsrc) fixed (byte* f = fsrc) fixed (byte* l = log) rc = Native.swr_program_validate_vf(v, f, l, log.Length);
            if (rc == -1) throw new ArgumentException(System.Text.Encoding.UTF8.GetString(log).TrimEnd('\0'));
            if (rc != 0) throw new NotSupportedException($"swr_program_validate_vf: {rc}");
            var key = (vertexMethod.Method, fragmentMethod.Method);
            lock (sources) { pairSources[key] = (vertexSource, fragmentSource); pairPrograms.Remove(key); }
        }

        static unsafe bool TryUserPair(Shaders.VertexShader vs, Shaders.FragmentShader fs, out int id)
        {
            id = 0;
            if (vs == null || fs == null) return false;
            lock (sources)
            {
                var key = (vs.Method, fs.Method);
                if (!pairSources.TryGetValue(key, out (string, string) source)) return false;
                if (pairPrograms.TryGetValue(key, out id)) return true;
                byte[] vsrc = System.Text.Encoding.UTF8.GetBytes(source.Item1 + "\0");
                byte[] fsrc = System.Text.Encoding.UTF8.GetBytes(source.Item2 + "\0");
                fixed (byte* v = vsrc) fixed (byte* f = fsrc) SwrContext.Check(Native.swr_program_create_vf(SwrContext.Handle, v, f, out id));
                pairPrograms[key] = id;
                return true;
            }
        }

        static unsafe bool TryUserProgram(Shaders.FragmentShader fs, out int id)
        {
            id = 0;
            if (fs == null) return false;
            lock (sources)
            {
                MethodInfo m = fs.Method;
                if (!sources.TryGetValue(m, out string source)) return false;
                if (programs.TryGetValue(m, out id)) return true;
                byte[] src = System.Text.Encoding.UTF8.GetBytes(source + "\0");
                fixed (byte* s = src) SwrContext.Check(Native.swr_program_create(SwrContext.Handle, s, out id));
                programs[m] = id;
                return true;
            }
        }

        // The closure's FURTHER Texture fields (a lightmap, a normal map, a mask): slot 1 .. 3 of the registered method's program, read
        // in its restatement as swr_sample(env, slot, uv) (swr_program_set_texture; null unbinds).  Slot 0 stays the Texture the closure
        // passes as the draw's.  Each draw captures the slots, and each texture's filter, when it is recorded.  The program is compiled
        // here if it has not been used yet.
        public static void SetTexture(Shaders.FragmentShader method, int slot, TextureNative? texture)
        {
            if (!TryUserProgram(method, out int id)) throw new ArgumentException("the fragment method is not registered");
            SwrContext.Check(Native.swr_program_set_texture(SwrContext.Handle, id, slot, texture?.Handle ?? IntPtr.Zero));
        }
        public static void SetTexture(Shaders.VertexShader vertexMethod, Shaders.FragmentShader fragmentMethod, int slot, TextureNative? texture)
        {
            if (!TryUserPair(vertexMethod, fragmentMethod, out int id)) throw new ArgumentException("the (vertex, fragment) pair is not registered");
            SwrContext.Check(Native.swr_program_set_texture(SwrContext.Handle, id, slot, texture?.Handle ?? IntPtr.Zero));
        }

        public static bool TryResolve(Shaders.VertexShader vs, Shaders.FragmentShader fs, out SwrProgram program, out SwrUniforms uniforms, out IntPtr texture)
        {
            program = SwrProgram.Dust2LambertFog; uniforms = default; texture = IntPtr.Zero;
            if (TryUserPair(vs, fs, out int pairId))
            {
                // a registered (vertex, fragment) pair: whatever the two delegates are.  The uniform block is the Renderer's fields when
                // one of them belongs to a Renderer (else zeros: such programs take their inputs as constants), the texture the one the
                // fragment closure captured.
                program = (SwrProgram)pairId;
                Renderer owner = vs.Target as Renderer ?? fs.Target as Renderer;
                Texture tex = null;
                if (fs.Target != null)
                    foreach (FieldInfo f in fs.Target.GetType().GetFields(Any))
                    {
                        object v = f.GetValue(fs.Target);
                        if (v is Texture t) tex = t;
                        if (owner == null && v is Renderer r) owner = r;
                    }
                if (owner != null)
                {
                    uniforms.LightDirection = Get<Vector3>(owner, "LightDirection");
                    uniforms.LightColor = Get<Vector4>(owner, "LightColor");
                    uniforms.FogColor = Get<Vector4>(owner, "FogColor");
                    uniforms.FogStart = Get<float>(owner, "FogStart");
                    uniforms.FogEnd = Get<float>(owner, "FogEnd");
                }
                texture = tex?.Native?.Handle ?? IntPtr.Zero;
                return true;
            }
            if (vs?.Target is not Renderer renderer || vs.Method.Name != "VertexShader") return false;
            bool user = TryUserProgram(fs, out int userId);
            if (user) program = (SwrProgram)userId;                                // ids >= SWR_PROG_USER_BASE (256)
            object closure = fs?.Target;
            if (closure == null) return false;
            Texture captured = null;
            bool sameRenderer = ReferenceEquals(closure, renderer);
            foreach (FieldInfo f in closure.GetType().GetFields(Any))
            {
                object v = f.GetValue(closure);
                if (v is Texture t) captured = t;
                if (ReferenceEquals(v, renderer)) sameRenderer = true;
            }
            if (!sameRenderer && !user) return false;                          // a fragment lambda of some other object
            uniforms.LightDirection = Get<Vector3>(renderer, "LightDirection");
            uniforms.LightColor = Get<Vector4>(renderer, "LightColor");
            uniforms.FogColor = Get<Vector4>(renderer, "FogColor");
            uniforms.FogStart = Get<float>(renderer, "FogStart");
            uniforms.FogEnd = Get<float>(renderer, "FogEnd");
            texture = captured?.Native?.Handle ?? IntPtr.Zero;                 // null texture -> Vector4.One (Renderer.cs:852)
            return true;
        }

        static T Get<T>(object o, string field) => (T)o.GetType().GetField(field, Any).GetValue(o);
    }

    // ---------------------------------------------------------------- MainWindow forwards ----
    // MainWindow.ColorBuffer / DepthBuffer (MainWindow.cs:30-31) live in HBM.  The bodies of the accessors become:
    //   SetPixel(x, y, c)      -> MainWindowNative.SetPixel(x, y, c);             (MainWindow.cs:382-388)
    //   GetPixel(x, y)         -> return MainWindowNative.GetPixel(x, y);         (:391-398, Vector4.Zero out of bounds)
    //   ClearColorBuffer(c)    -> MainWindowNative.ClearColorBuffer(c);           (:400-407; fused into the tile pass)
    //   SetDepth(x, y, d)      -> MainWindowNative.SetDepth(x, y, d);             (:411-417)
    //   GetDepth(x, y)         -> return MainWindowNative.GetDepth(x, y);         (:420-426, float.MinValue out of bounds)
    //   ClearDepthBuffer()     -> MainWindowNative.ClearDepthBuffer();            (:429-436)
    //   HandleResize           -> MainWindowNative.Resize(RenderWidth, RenderHeight) instead of allocating the arrays (:320-321)
    //   OnRender               -> MainWindowNative.Present(flatColorBuffer) instead of the Vector4 -> Vector3 loop (:234-240)
    public static unsafe class MainWindowNative
    {
        /// Supersampling (build-defined; the reference's RenderScale stops at 1, MainWindow.cs:93,313-315): 1, 2, 4 or 8 samples per
        /// window-scale pixel in each direction.  Resize then allocates window x RenderScale x SuperSample in HBM, the draws render
        /// into that, and Present / PresentAsync deliver window x RenderScale Vector3s, box-filtered on the GPU (swr_*_resolved):
        /// the host's arrays, its PCIe traffic and its GL texture keep the size they have today.  Set it before Resize.
        /// (Like the rest of this file: written by reading, not compiled.)
        public static int SuperSample { get; set; } = 1;
        public static void Resize(int renderWidth, int renderHeight)
        {
            if (SuperSample != 1 && SuperSample != 2 && SuperSample != 4 && SuperSample != 8) throw new ArgumentException("SuperSample must be 1, 2, 4 or 8");
            SwrContext.Check(Native.swr_resize(SwrContext.Handle, renderWidth * SuperSample, renderHeight * SuperSample));
        }
        public static void SetPixel(int x, int y, Vector4 color) => SwrContext.Check(Native.swr_set_pixel(SwrContext.Handle, x, y, &color));
        public static Vector4 GetPixel(int x, int y) { Vector4 c; SwrContext.Check(Native.swr_get_pixel(SwrContext.Handle, x, y, &c)); return c; }
        public static void ClearColorBuffer(Vector4 clearColor) => SwrContext.Check(Native.swr_clear_color(SwrContext.Handle, &clearColor));
        public static void SetDepth(int x, int y, float depth) => SwrContext.Check(Native.swr_set_depth(SwrContext.Handle, x, y, depth));
        public static float GetDepth(int x, int y) { float d; SwrContext.Check(Native.swr_get_depth(SwrContext.Handle, x, y, &d)); return d; }
        public static void ClearDepthBuffer() => SwrContext.Check(Native.swr_clear_depth(SwrContext.Handle));

        /// The present payload of MainWindow.OnRender: executes the recorded draws and fills the caller's Vector3[] (RGB float,
        /// flattened on the GPU).  Register a long-lived pinned array once with Pin() and the copy runs at PCIe rate.
        public static void Present(Vector3[] flatColorBuffer)
        {
            fixed (Vector3* p = flatColorBuffer)
                SwrContext.Check(SuperSample == 1 ? Native.swr_readback_rgb(SwrContext.Handle, p)
                                                  : Native.swr_readback_rgb_resolved(SwrContext.Handle, SuperSample, SuperSample, p));
        }
        /// Double-buffered present for a host that keeps MainWindow.OnRender (MainWindow.cs:226-263): two PINNED flat buffers
        /// alternate; PresentAsync(i) starts frame i's flatten + copy and returns the buffer of frame i - 1, which has finished
        /// crossing PCIe while frame i was being rendered (null on the very first call).  width x height is the WINDOW-scale size
        /// passed to Resize (what the arrays hold under any SuperSample).  Per frame the host then pays
        /// max(render, copy) instead of render + copy: at 4096 x 4096 the copy is 4.6 ms and the render 0.7 ms (DESIGN.md section 5).
        static readonly Vector3[]?[] presentBuffers = new Vector3[]?[2];
        static readonly GCHandle[] presentPins = new GCHandle[2];
        static readonly ulong[] presentTickets = new ulong[2];
        static int presentNext;
        public static Vector3[]? PresentAsync(int width, int height)
        {
            int cur = presentNext, prev = presentNext ^ 1;
            presentNext = prev;
            int n = Math.Max(width, 0) * Math.Max(height, 0);
            if (presentBuffers[cur] == null || presentBuffers[cur]!.Length != n)
            {
                if (presentBuffers[cur] != null) { SwrContext.Check(Native.swr_host_unregister(SwrContext.Handle, (void*)presentPins[cur].AddrOfPinnedObject())); presentPins[cur].Free(); }
                presentBuffers[cur] = new Vector3[n];
                presentPins[cur] = Pin(presentBuffers[cur]!, (nuint)n * 12);
            }
            Vector3* dst = (Vector3*)presentPins[cur].AddrOfPinnedObject();
            SwrContext.Check(SuperSample == 1 ? Native.swr_present_rgb_async(SwrContext.Handle, dst, out presentTickets[cur])
                                              : Native.swr_present_rgb_resolved_async(SwrContext.Handle, SuperSample, SuperSample, dst, out presentTickets[cur]));
            if (presentTickets[prev] == 0) return null;
            int rc = Native.swr_present_wait(SwrContext.Handle, presentTickets[prev]);
            presentTickets[prev] = 0;
            if (rc == 1)        // SWR_STALE: a batch was replayed while the pair buffers were still growing -- take that frame synchronously
            {
                Present(presentBuffers[prev]!);
                return presentBuffers[prev];
            }
            SwrContext.Check(rc);
            return presentBuffers[prev];
        }
        /// 8-bit present (build-defined; DESIGN.md section 18): 0 keeps today's Vector3 payload (Present / PresentAsync); 3 or 4 makes
        /// PresentAsync8 deliver the bytes the window's 8-bit framebuffer would hold anyway -- R, G, B or R, G, B, 255 per
        /// window-scale pixel, clamped to [0, 1], times 255, rounded to nearest even on the GPU --, a quarter or a third of the bytes.
        /// Upload them with PixelType.UnsignedByte and PixelFormat.Rgb (after Gl.PixelStore(UnpackAlignment, 1): rows are tightly
        /// packed) or PixelFormat.Rgba; the texture's internal format can stay Rgba32f (INTEGRATION.md).  Composes with SuperSample.
        public static int PresentBytes { get; set; } = 0;
        static readonly byte[]?[] present8Buffers = new byte[]?[2];
        static readonly GCHandle[] present8Pins = new GCHandle[2];
        static readonly ulong[] present8Tickets = new ulong[2];
        static int present8Next;
        /// PresentAsync with byte payloads: starts frame i's quantise + copy and returns the bytes of frame i - 1 (null on the very
        /// first call); width x height is the WINDOW-scale size passed to Resize.  Shares the library's two present slots with
        /// PresentAsync, so a host uses one of the two in its loop.
        public static byte[]? PresentAsync8(int width, int height)
        {
            if (PresentBytes != 3 && PresentBytes != 4) throw new InvalidOperationException("set PresentBytes to 3 or 4 first");
            int cur = present8Next, prev = present8Next ^ 1;
            present8Next = prev;
            int n = Math.Max(width, 0) * Math.Max(height, 0) * PresentBytes;
            if (present8Buffers[cur] == null || present8Buffers[cur]!.Length != n)
            {
                if (present8Buffers[cur] != null) { SwrContext.Check(Native.swr_host_unregister(SwrContext.Handle, (void*)present8Pins[cur].AddrOfPinnedObject())); present8Pins[cur].Free(); }
                present8Buffers[cur] = new byte[n];
                present8Pins[cur] = Pin(present8Buffers[cur]!, (nuint)n);
            }
            byte* dst = (byte*)present8Pins[cur].AddrOfPinnedObject();
            SwrContext.Check(Native.swr_present_rgb8_async(SwrContext.Handle, SuperSample, SuperSample, PresentBytes, dst, out present8Tickets[cur]));
            if (present8Tickets[prev] == 0) return null;
            int rc = Native.swr_present_wait(SwrContext.Handle, present8Tickets[prev]);
            present8Tickets[prev] = 0;
            if (rc == 1)        // SWR_STALE, as in PresentAsync: take that frame synchronously
            {
                fixed (byte* p = present8Buffers[prev]!)
                    SwrContext.Check(Native.swr_readback_rgb8(SwrContext.Handle, SuperSample, SuperSample, PresentBytes, p));
                return present8Buffers[prev];
            }
            SwrContext.Check(rc);
            return present8Buffers[prev];
        }
        /// PresentAsync8 with a post-process program in front of the quantiser (build-defined; DESIGN.md section 20): starts frame i's
        /// resolve + program + copy and returns the bytes of frame i - 1 (null on the very first call).  The program's constants are
        /// captured by this call.  Shares PresentAsync8's buffers and the library's two present slots: a host uses one present in its loop.
        public static byte[]? PresentPost(PostProgramNative post, int width, int height)
        {
            if (PresentBytes != 3 && PresentBytes != 4) throw new InvalidOperationException("set PresentBytes to 3 or 4 first");
            int cur = present8Next, prev = present8Next ^ 1;
            present8Next = prev;
            int n = Math.Max(width, 0) * Math.Max(height, 0) * PresentBytes;
            if (present8Buffers[cur] == null || present8Buffers[cur]!.Length != n)
            {
                if (present8Buffers[cur] != null) { SwrContext.Check(Native.swr_host_unregister(SwrContext.Handle, (void*)present8Pins[cur].AddrOfPinnedObject())); present8Pins[cur].Free(); }
                present8Buffers[cur] = new byte[n];
                present8Pins[cur] = Pin(present8Buffers[cur]!, (nuint)n);
            }
            byte* dst = (byte*)present8Pins[cur].AddrOfPinnedObject();
            SwrContext.Check(Native.swr_present_post_async(SwrContext.Handle, post.Id, SuperSample, SuperSample, PresentBytes, dst, out present8Tickets[cur]));
            if (present8Tickets[prev] == 0) return null;
            int rc = Native.swr_present_wait(SwrContext.Handle, present8Tickets[prev]);
            present8Tickets[prev] = 0;
            if (rc == 1)        // SWR_STALE, as in PresentAsync8: take that frame synchronously (with the constants as they are now)
            {
                fixed (byte* p = present8Buffers[prev]!)
                    SwrContext.Check(Native.swr_readback_post(SwrContext.Handle, post.Id, SuperSample, SuperSample, PresentBytes, p));
                return present8Buffers[prev];
            }
            SwrContext.Check(rc);
            return present8Buffers[prev];
        }
        /// Full-precision read-back into the reference's own arrays (tools, screenshots).
        public static void Readback(Vector4[] colorBuffer, float[] depthBuffer)
        {
            fixed (Vector4* c = colorBuffer) fixed (float* d = depthBuffer) SwrContext.Check(Native.swr_readback(SwrContext.Handle, c, d));
        }
        public static GCHandle Pin(Array longLivedBuffer, nuint bytes)
        {
            GCHandle h = GCHandle.Alloc(longLivedBuffer, GCHandleType.Pinned);
            SwrContext.Check(Native.swr_host_register(SwrContext.Handle, (void*)h.AddrOfPinnedObject(), bytes));
            return h;
        }
        public static SwrStats Stats() { SwrContext.Check(Native.swr_get_stats(SwrContext.Handle, out SwrStats s)); return s; }
    }

    // ---------------------------------------------------------------- Post-process programs ----
    // A per-pixel pass between the frame and its delivery, written against the contract of swr.h (swr_post) and compiled at run time;
    // MainWindowNative.PresentPost runs it in front of the 8-bit quantiser.  INTEGRATION.md, "Porting a post-process pass".
    public sealed unsafe class PostProgramNative : IDisposable
    {
        public int Id { get; private set; }
        public PostProgramNative(string source)
        {
            byte[] src = System.Text.Encoding.UTF8.GetBytes(source + "\0");
            byte[] log = new byte[1 << 16];
            int rc;
            fixed (byte* s = src) fixed (byte* l = log) rc = Native.swr_post_validate(s, l, log.Length);
            if (rc == -1) throw new ArgumentException("post program does not compile:\n" + System.Text.Encoding.UTF8.GetString(log).TrimEnd('\0'));
            if (rc != 0) throw new NotSupportedException($"swr_post_validate: {rc}");
            int id;
            fixed (byte* s = src) SwrContext.Check(Native.swr_post_create(SwrContext.Handle, s, out id));
            Id = id;
        }
        /// Up to 64 floats the program reads as env.constants[i]; each present captures them when it is called.
        public void SetConstants(ReadOnlySpan<float> values)
        {
            fixed (float* v = values) SwrContext.Check(Native.swr_post_set_constants(SwrContext.Handle, Id, v, values.Length));
        }
        /// Bind a texture to slot 0 .. 3 (null unbinds): the program reads it with swr_post_sample / swr_post_texel.  Each present
        /// captures the four slots, and each texture's filter, when it is called.
        public void SetTexture(int slot, TextureNative? texture)
        {
            SwrContext.Check(Native.swr_post_set_texture(SwrContext.Handle, Id, slot, texture?.Handle ?? IntPtr.Zero));
        }
        public void Dispose()
        {
            if (Id != 0) Native.swr_post_destroy(SwrContext.Handle, Id);       // a present in flight with the program still completes
            Id = 0;
        }
    }

    // ---------------------------------------------------------------- Texture ----
    // Texture(Image<Rgba32>) / Width / Height / Sample / Dispose (Texture.cs:31-68).  `Texture` keeps its public surface and
    // gains `internal TextureNative Native` created in its constructor; Sample(uv) stays available on the host (one call per
    // sample: tools only -- the fragment programs sample on the GPU).
    public sealed unsafe class TextureNative : IDisposable
    {
        public IntPtr Handle { get; private set; }
        public int Width { get; }
        public int Height { get; }

        public TextureNative(Image<Rgba32> image)
        {
            Width = image.Width; Height = image.Height;
            var pixels = new byte[Width * Height * 4];
            image.CopyPixelDataTo(pixels);                                     // RGBA8 row-major, as Texture.cs:55-56 indexes it
            fixed (byte* p = pixels)
            {
                SwrContext.Check(Native.swr_texture_create(SwrContext.Handle, p, Width, Height, out IntPtr h));
                Handle = h;
            }
        }

        private TextureNative(int width, int height, IntPtr handle) { Width = width; Height = height; Handle = handle; }

        /// Render to texture (build-defined: the reference links Texture and the window's buffers nowhere).  A texture of zeros
        /// without host data, to be filled by UpdateFrom.
        public static TextureNative CreateTarget(int width, int height)
        {
            SwrContext.Check(Native.swr_texture_create_target(SwrContext.Handle, width, height, out IntPtr h));
            return new TextureNative(width, height, h);
        }

        /// The texels become the frame of Width * kx by Height * ky pixels, box-filtered and quantised as the 8-bit present; alpha
        /// 255, or the frame's with keepAlpha.  The frame is this context's (MainWindowNative's) unless sourceContext names another
        /// swr_context on the same GPU.  Immediate-mode semantics -- draws recorded earlier sample the old texels, later ones the
        /// new -- and no wait for the GPU: one kernel on the context's stream (swr_texture_update_from_frame).
        public void UpdateFrom(int kx = 1, int ky = 1, bool keepAlpha = false, IntPtr sourceContext = default)
        {
            SwrContext.Check(Native.swr_texture_update_from_frame(SwrContext.Handle, Handle, sourceContext, kx, ky, keepAlpha ? 1 : 0));
        }

        /// A pass's result into the texture: UpdateFrom with `post` -- a program of the source context -- between the resolve and the
        /// quantiser; alpha 255, or the quantised w of the program's result with keepAlpha.  The texture may not be bound to a slot
        /// of `post`.  A chain of passes is a sequence of calls: pass 1 writes A, pass 2 samples A (swr_texture_update_from_post).
        public void UpdateFromPost(PostProgramNative post, int kx = 1, int ky = 1, bool keepAlpha = false, IntPtr sourceContext = default)
        {
            SwrContext.Check(Native.swr_texture_update_from_post(SwrContext.Handle, Handle, sourceContext, post.Id, kx, ky, keepAlpha ? 1 : 0));
        }

        /// Depth textures (build-defined: the reference links MainWindow's depth floats and a Texture nowhere).  float32 depth words
        /// as the raster stage stores them: `depth` (Width * Height floats, row-major) or, null, float.MinValue everywhere -- nothing
        /// drawn.  Filled by UpdateFromDepth; programs read it through swr_shadow / swr_sample_depth / swr_texel_depth.
        public static TextureNative CreateDepth(int width, int height, float[] depth = null)
        {
            if (depth != null && depth.Length != width * height) throw new ArgumentException("depth must hold width * height floats");
            fixed (float* p = depth)                                           // (null array: null pointer)
            {
                SwrContext.Check(Native.swr_texture_create_depth(SwrContext.Handle, p, width, height, out IntPtr h));
                return new TextureNative(width, height, h);
            }
        }

        public enum DepthReduce { Max = 0, Min = 1, First = 2 }               // SWR_DEPTH_REDUCE_*

        /// Cube maps (build-defined: the reference addresses a texture by uv alone and clears to one colour, Renderer.cs:413).  A cube
        /// of side n is a texture n wide and 6 n high, face f (0..5 = +X, -X, +Y, -Y, +Z, -Z) in rows [f n, (f + 1) n).  `rgba8`: six
        /// faces of n x n, face-major, or null for zeros (a target for UpdateFaceFrom).  Programs read it through swr_sample_cube.
        public static TextureNative CreateCube(int n, byte[] rgba8 = null)
        {
            if (rgba8 != null && rgba8.Length != 6 * n * n * 4) throw new ArgumentException("rgba8 must hold 6 * n * n * 4 bytes");
            fixed (byte* p = rgba8)
            {
                SwrContext.Check(Native.swr_texture_create_cube(SwrContext.Handle, p, n, out IntPtr h));
                return new TextureNative(n, 6 * n, h);
            }
        }

        /// A depth cube: float.MinValue everywhere until UpdateFaceFromDepth fills it; swr_shadow_cube / swr_sample_cube_depth read it.
        public static TextureNative CreateCubeDepth(int n, float[] depth = null)
        {
            if (depth != null && depth.Length != 6 * n * n) throw new ArgumentException("depth must hold 6 * n * n floats");
            fixed (float* p = depth)
            {
                SwrContext.Check(Native.swr_texture_create_cube_depth(SwrContext.Handle, p, n, out IntPtr h));
                return new TextureNative(n, 6 * n, h);
            }
        }

        /// UpdateFrom into one face of a cube: the frame measures n * kx by n * ky (swr_texture_update_face_from_frame).
        public void UpdateFaceFrom(int face, int kx = 1, int ky = 1, bool keepAlpha = false, IntPtr sourceContext = default)
        {
            SwrContext.Check(Native.swr_texture_update_face_from_frame(SwrContext.Handle, Handle, face, sourceContext, kx, ky, keepAlpha ? 1 : 0));
        }

        /// UpdateFromDepth into one face of a depth cube (swr_texture_update_face_from_depth).
        public void UpdateFaceFromDepth(int face, int kx = 1, int ky = 1, DepthReduce reduce = DepthReduce.Max, IntPtr sourceContext = default)
        {
            SwrContext.Check(Native.swr_texture_update_face_from_depth(SwrContext.Handle, Handle, face, sourceContext, kx, ky, (int)reduce));
        }

        /// Matrix4x4.CreateLookAt of a face's camera at `eye` (swr_cube_face_view): with CreatePerspectiveFieldOfView(pi / 2, 1, near,
        /// far) the pixel whose centre lies in direction d from eye is the texel swr_sample_cube reads for d.
        public static Matrix4x4 CubeFaceView(int face, Vector3 eye)
        {
            Matrix4x4 view;
            if (Native.swr_cube_face_view(face, (float*)&eye, (float*)&view) != 0) throw new ArgumentOutOfRangeException(nameof(face));
            return view;
        }

        /// Each texel becomes ONE word of its kx x ky block of the frame's depth plane (Width * kx by Height * ky pixels): the
        /// nearest under the default LessEqual test (Max), the farthest (Min) or the top-left one (First).  Otherwise UpdateFrom's
        /// contract: immediate-mode semantics, no wait for the GPU, one kernel (swr_texture_update_from_depth).
        public void UpdateFromDepth(int kx = 1, int ky = 1, DepthReduce reduce = DepthReduce.Max, IntPtr sourceContext = default)
        {
            SwrContext.Check(Native.swr_texture_update_from_depth(SwrContext.Handle, Handle, sourceContext, kx, ky, (int)reduce));
        }

        /// The depth words, row-major, Width * Height floats; waits for the GPU.
        public float[] ReadDepth()
        {
            var words = new float[Width * Height];
            fixed (float* p = words)
                SwrContext.Check(Native.TextureReadDepth(SwrContext.Handle, Handle, p));
            return words;
        }

        /// (the depth word Texture.Sample's addressing picks at uv, swr_shadow of the texture at uv against reference) with the
        /// texture's filter as it is now; one call per sample: tools only.
        public Vector2 SampleDepth(Vector2 uv, float reference)
        {
            float* q = stackalloc float[3] { uv.X, uv.Y, reference };
            Vector2 o;
            SwrContext.Check(Native.swr_texture_sample_depth(SwrContext.Handle, Handle, q, 1, (float*)&o));
            return o;
        }

        /// 0 = RGBA8, 1 = float32 depth (SWR_TEXTURE_FORMAT_*)
        public int Format
        {
            get { SwrContext.Check(Native.swr_texture_format(SwrContext.Handle, Handle, out int f)); return f; }
        }

        /// Build-defined (the reference's Texture is one level): gives the texture its mip chain, or regenerates it -- 1 + floor(log2(max(
        /// Width, Height))) levels, each a 2 x 2 box filter of the one before.  UpdateFrom's order, no wait for the GPU; from then on
        /// UpdateFrom / UpdateFromPost regenerate the chain in the same call (swr_texture_generate_mipmaps).  User and post programs
        /// read it through swr_sample_grad / swr_sample_lod / swr_sample_level; Sample and the built-in programs stay on level 0.
        public void GenerateMipmaps()
        {
            SwrContext.Check(Native.swr_texture_generate_mipmaps(SwrContext.Handle, Handle));
        }

        /// 1, or the chain's length once GenerateMipmaps has run
        public int Levels
        {
            get { SwrContext.Check(Native.swr_texture_levels(SwrContext.Handle, Handle, out int n)); return n; }
        }

        /// The RGBA8 texels of a level the texture has, row-major, max(1, Width >> level) * max(1, Height >> level) * 4 bytes; waits for the GPU.
        public byte[] ReadLevel(int level)
        {
            SwrContext.Check(Native.swr_texture_level_size(SwrContext.Handle, Handle, level, out int w, out int h));
            var pixels = new byte[w * h * 4];
            fixed (byte* p = pixels)
                SwrContext.Check(Native.TextureReadLevel(SwrContext.Handle, Handle, level, p));
            return pixels;
        }

        /// The RGBA8 texels, row-major, Width * Height * 4 bytes; waits for the GPU (screenshots, tests).
        public byte[] Read()
        {
            var pixels = new byte[Width * Height * 4];
            fixed (byte* p = pixels)
                SwrContext.Check(Native.swr_texture_readback(SwrContext.Handle, Handle, p));
            return pixels;
        }

        public Vector4 Sample(Vector2 uv)                                       // Texture.cs:43-63: nearest, wrap, byte * (1f / 255f)
        {
            Vector4 o;
            SwrContext.Check(Native.swr_texture_sample(SwrContext.Handle, Handle, &uv, 1, &o));
            return o;
        }

        public void Dispose()                                                   // Texture.cs:65-68
        {
            if (Handle == IntPtr.Zero) return;
            Native.swr_texture_destroy(SwrContext.Handle, Handle);
            Handle = IntPtr.Zero;
        }
    }

    // FrustumCuller.CalculateBoundingSphere / IsSphereInFrustum stay managed (FrustumCuller.cs is untouched); the GPU versions
    // (swr_mesh_bounds, swr_is_sphere_in_frustum -- bit-identical, tests/test_gpu_api.py) are reachable through
    // Rasterizer.RenderMesh(window, mesh, ..., frustumCull: true).
}
