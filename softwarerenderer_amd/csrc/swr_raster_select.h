// swr_raster_select.h -- which k_raster_c instantiation a batch gets, as a pure function of its draws (no HIP types: the host
// compiler alone builds it, tests/test_raster_select_host.py checks it against tests/shade_edge_scenes.py::predicted_kernel).
#pragma once
#include "swr.h"

namespace swr {

// (in the order launch_raster's table instantiates the kernels; user programs bring their own pair, compiled at run time)
#define SWR_RASTER_KERNELS(X)                                                                                              \
    X(debug_varyings_none) X(debug_varyings) X(wireframe) X(generic_none) X(phong_default) X(generic_phong) X(dust2_default) \
    X(gouraud_default) X(generic) X(user) X(user_none)
#define SWR_X(name) name,
enum class RasterKernel { SWR_RASTER_KERNELS(SWR_X) };
#undef SWR_X
#define SWR_X(name) #name,
inline const char* raster_kernel_name(RasterKernel k) { static const char* const n[] = { SWR_RASTER_KERNELS(SWR_X) }; return n[(int)k]; }
#undef SWR_X

// What the choice looks at, gathered draw by draw.  A batch holds only DEBUG_VARYINGS draws, only draws of ONE user program, or
// neither kind, and is never wireframe with either (record_draw / flush_locked).
struct RasterTraits {
    bool wireframe = false;                    // Rasterizer.RenderDebugMode == Wireframe for the whole batch
    bool user = false, debug_varyings = false;
    bool none = false, phong = false;          // some draw has BlendMode.None (row early-out) / the Phong program
    // every draw has this program and the RenderMesh defaults (dust2: the reference's own frame, Renderer's shader pair)
    bool dust2_default = true, phong_default = true, gouraud_default = true;
    bool depth_only_grows = true;              // every draw tests Less or LessEqual (RasterArgs::depth_only_grows)

    void add(int program, int blend, int depth_test) {
        const bool defaults = blend == SWR_BLEND_ALPHA && depth_test == SWR_DEPTH_LESSEQUAL;
        gouraud_default = gouraud_default && program == SWR_PROG_GOURAUD && defaults;
        phong_default = phong_default && program == SWR_PROG_PHONG_4POINT && defaults;
        dust2_default = dust2_default && program == SWR_PROG_DUST2_LAMBERT_FOG && defaults;
        depth_only_grows = depth_only_grows && (depth_test == SWR_DEPTH_LESS || depth_test == SWR_DEPTH_LESSEQUAL);
        phong = phong || program == SWR_PROG_PHONG_4POINT;
        none = none || blend == SWR_BLEND_NONE;
        user = user || program >= SWR_PROG_USER_BASE;
        debug_varyings = debug_varyings || program == SWR_PROG_DEBUG_VARYINGS;
    }
};

inline RasterKernel select_raster_kernel(const RasterTraits& t) {
    if (t.user) return t.none ? RasterKernel::user_none : RasterKernel::user;
    if (t.debug_varyings) return t.none ? RasterKernel::debug_varyings_none : RasterKernel::debug_varyings;
    if (t.wireframe) return RasterKernel::wireframe;              // DrawLine has no early-out
    if (t.none) return RasterKernel::generic_none;
    if (t.phong_default) return RasterKernel::phong_default;
    if (t.phong) return RasterKernel::generic_phong;
    if (t.dust2_default) return RasterKernel::dust2_default;
    if (t.gouraud_default) return RasterKernel::gouraud_default;
    return RasterKernel::generic;
}

}  // namespace swr
