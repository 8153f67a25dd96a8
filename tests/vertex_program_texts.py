"""Program texts shared by tests/test_vertex_program_host.py and tests/test_gpu_vertex_program.py (and tools/vertex_program_numbers.py):
vertex halves against the contract of include/swr.h (swr_program_create_vf), fragment halves that read the new varying."""

# Renderer.VertexShader, Renderer.cs:830-846
RENDERER_VS = r"""
__device__ void swr_vertex(const swr_vs_in& in, const swr_vs_env& env, swr_vs_out& out) {
    const float4 world = swr_transform(make_float4(in.position.x, in.position.y, in.position.z, 1.0f), env.model, env);
    const float4 viewp = swr_transform(world, env.view, env);
    out.clip_position = swr_transform(viewp, env.projection, env);
    out.world_normal = swr_normalize(swr_transform_normal(in.normal, env.model, env));
    out.color = in.color;
    out.tex_coord = in.uv;
    out.normal = in.normal;
}
"""

# the same with the position displaced by the draw's first three constants (a wind / wobble offset): one IEEE add per component
DISPLACE_VS = RENDERER_VS.replace(
    "make_float4(in.position.x, in.position.y, in.position.z, 1.0f)",
    "make_float4(in.position.x + env.constants[0], in.position.y + env.constants[1], in.position.z + env.constants[2], 1.0f)")

# Renderer.VertexShader that also hands the world normal to the fragment half through its own Vector4 key (z once more in w)
DATA4_VS = RENDERER_VS.replace(
    "    out.color = in.color;",
    "    out.data4 = make_float4(out.world_normal.x, out.world_normal.y, out.world_normal.z, out.world_normal.z);\n"
    "    out.color = in.color;")

# InterpolateData's Vector3 branch (Rasterizer.cs:684-687) done by hand on the Vector4 key, which the raster stage only sums
_RENORM = r"""
__device__ float4 swr_fragment(const swr_fs_in& in, const swr_fs_env& env) {
    float3 n = make_float3(in.data4.x, in.data4.y, in.data4.%s);
    const float len_sq = swr_dot3(n, n);
    if (len_sq > 1e-6f) {
        const float s = 1.0f / sqrtf(len_sq);
        n = make_float3(n.x * s, n.y * s, n.z * s);
    }
    return make_float4(n.x, n.y, n.z, 1.0f);
}
"""
DATA4_XYZ_FS = _RENORM % "z"
DATA4_XYW_FS = _RENORM % "w"          # (.w travels apart from .xyz: its own lerp in the clipper, its own load in the raster kernel)
WORLD_NORMAL_FS = r"""
__device__ float4 swr_fragment(const swr_fs_in& in, const swr_fs_env& env) {
    return make_float4(in.world_normal.x, in.world_normal.y, in.world_normal.z, 1.0f);
}
"""
DATA4_PLUS_FS = r"""
__device__ float4 swr_fragment(const swr_fs_in& in, const swr_fs_env& env) {
    return make_float4(in.data4.x + 0.25f, in.data4.y + 0.5f, in.data4.z + 0.75f, in.data4.w + 1.0f);
}
"""
QUARTERS_FS = r"""
__device__ float4 swr_fragment(const swr_fs_in& in, const swr_fs_env& env) { return make_float4(0.25f, 0.5f, 0.75f, 1.0f); }
"""
