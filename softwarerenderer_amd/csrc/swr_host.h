// swr_host.h -- host side of libswr_hip.so: the context and batch types, device buffers, the frame-slot ring, band geometry,
// timing spans, the front stream, run-time values as kernel template arguments.  Included by swr_api.hip only (the library's one translation
// unit), in front of swr_rtc.h, swr_flush.h, swr_query.h, swr_texture.h and swr_deform.h.
#pragma once
#include <memory>
#include <type_traits>

// An event several meshes share: swr_mesh_skin_batch records ONE behind its kernel for all its destinations (an event record costs a
// few microseconds of stream time, per mesh that was most of a small batch); freed with its last holder.
struct SharedEvent {
    hipEvent_t ev = nullptr;
    ~SharedEvent() { if (ev) (void)hipEventDestroy(ev); }
};

struct swr_mesh {
    float4* d_bounds = nullptr;               // Mesh.SphereBounds (ModelLoader.cs:291), computed on first use
    bool bounds_ready = false;
    swr_vertex* d_verts = nullptr;
    uint16_t* d_idx = nullptr;
    int n_verts = 0, n_idx = 0;
    size_t cap_verts = 0, cap_idx = 0;        // bytes allocated behind d_verts / d_idx (a recycled transient mesh may hold more than it uses)
    bool transient = false;
    float box_lo[3] = { 0, 0, 0 }, box_hi[3] = { 0, 0, 0 };   // exact model-space AABB of the vertices (host, at creation)
    bool has_box = false;
    hipEvent_t uploaded = nullptr;            // retained meshes: recorded behind the upload, for readers on another stream (swr_raycast)
    bool upload_seen = false;                 // ... the ray stream has been ordered behind it
    std::shared_ptr<SharedEvent> posed;       // set: the last write was a batched skin, and THIS event is behind it (stands in for `uploaded`)
    swr_context* owner = nullptr;             // the context that made it (the deform calls refuse another context's mesh)
    // static skin attributes (swr_mesh_set_skin): four joint indices and four weights per vertex, uploaded once
    ushort4* d_joints = nullptr;
    float4* d_weights = nullptr;
    bool has_skin = false;                    // (a mesh without vertices has the attributes and no arrays)
    int max_joint = -1;                       // largest joint index used (host, at the upload): swr_mesh_skin needs a longer palette
};
// Skeletal animation.  A skeleton's static arrays are one device blob; its clips are another (the host keeps
// a copy: adding a clip re-uploads the whole blob into a new allocation).
struct swr_skeleton {
    swr_context* owner = nullptr;
    int n_nodes = 0, n_joints = 0, n_levels = 0;
    void* d_static = nullptr;                 // one blob of 32-bit words, laid out by skeleton_layout (swr_animation_layout.h)
    uint32_t* d_clips = nullptr;
    std::vector<uint32_t> clips;              // the clip blob (swr_animation.hip.h), word 0 unused
    std::vector<uint32_t> clip_base;          // word offset of each clip's node table
};
struct swr_pose_set {
    swr_context* owner = nullptr;
    int n_instances = 0, n_joints = 0;
    float* d_palettes = nullptr;              // n_instances x n_joints x 16 floats, zero at creation
    float* d_worlds = nullptr;                // k_pose_sample's node matrices: n_instances x world_nodes x 16 floats
    int world_nodes = 0;
    hipEvent_t written = nullptr;             // behind the last sample or upload, for swr_pose_set_readback on the ray stream
    bool written_seen = true;
};
struct swr_texture {
    uint8_t* d_rgba = nullptr;
    uint8_t* d_blocked = nullptr;             // block-linear copy (4 x 4-texel blocks of 64 B) for the bilinear filter, made when it is first switched on
                                              // and written beside d_rgba by swr_texture_update_from_frame from then on
    int w = 0, h = 0;
    bool bilinear = false;                    // build-defined extension; the reference's Texture.Sample is nearest
    int format = SWR_TEXTURE_FORMAT_RGBA8;    // or SWR_TEXTURE_FORMAT_DEPTH32F: the same 4-byte texels, float32 depth words (d_rgba names the
                                              // row-major copy of either).  Host-side only: a slot's record does not carry it
    // MIP CHAIN.  d_rgba and d_blocked each point at texel 0 of an allocation that begins SWR_TEXTURE_HEADER_BYTES
    // earlier with a TextureHeader (swr_device.h): texels_alloc / texels_free.  Both headers name the same tail.
    uint8_t* d_tail = nullptr;                // levels 1 .. L - 1, row-major, one behind the other: allocated by the first swr_texture_generate_mipmaps
    int levels = 1;                           // what the headers say: 1, or L once the chain exists
    // CUBE MAP: w = n, h = 6 n, face f in rows [f n, (f + 1) n).  Host-side only, like the format
    bool cube = false;
};

// the chain a w x h texture can have: L = 1 + floor(log2(max(w, h))) levels, level l measuring max(1, w >> l) by max(1, h >> l)
inline int mip_full_levels(int w, int h) { int L = 1; for (int m = w > h ? w : h; m > 1; m >>= 1) ++L; return L; }
inline int mip_level_side(int side, int level) { return (side >> level) > 1 ? (side >> level) : 1; }
// ... and a cube of power-of-two side n: L = 1 + log2(n), level l the (n >> l) x 6 (n >> l) atlas -- the first L levels of the n x 6 n
// texture's chain, where no 2 x 2 box straddles two faces.  Another side has no chain (swr_texture_generate_mipmaps refuses it)
inline int texture_full_levels(const swr_texture* t) { return t->cube ? ((t->w & (t->w - 1)) == 0 ? mip_full_levels(t->w, 1) : 1) : mip_full_levels(t->w, t->h); }
// a texel array of `bytes` behind its header: *texels is texel 0, 256-byte aligned as hipMalloc's block is
inline hipError_t texels_alloc(uint8_t** texels, size_t bytes) {
    void* base = nullptr;
    const hipError_t e = hipMalloc(&base, bytes + SWR_TEXTURE_HEADER_BYTES);
    *texels = e == hipSuccess ? static_cast<uint8_t*>(base) + SWR_TEXTURE_HEADER_BYTES : nullptr;
    return e;
}
inline void texels_free(uint8_t* texels) { if (texels) (void)hipFree(texels - SWR_TEXTURE_HEADER_BYTES); }

namespace {

thread_local std::string g_create_error;

// A texture as it is NOW, as a program's texture slot captures it (TextureSlot, swr_device.h): pointer, size and filter, the
// block-linear copy where the texture has one -- what record_draw writes into DrawParams for a draw's own texture.  Null: unbound.
TextureSlot texture_slot_of(const swr_texture* t) {
    if (!t) return TextureSlot{ nullptr, 0, 0 };
    if (t->bilinear && t->d_blocked) return TextureSlot{ t->d_blocked, -t->w, -t->h };
    return TextureSlot{ t->d_rgba, t->w, t->bilinear ? -t->h : t->h };
}

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

enum Stage { ST_VERTEX = 0, ST_SETUP, ST_BIN, ST_SORT, ST_COVER, ST_RASTER, ST_CLEAR, ST_COUNT };

struct EventSpan { int stage; hipEvent_t a, b; };

#ifndef SWR_TIMING_EVENT_FLAGS
#define SWR_TIMING_EVENT_FLAGS hipEventDisableSystemFence
#endif
#ifndef SWR_HANDOVER_EVENT_FLAGS
#define SWR_HANDOVER_EVENT_FLAGS hipEventDisableTiming
#endif
#define SWR_SLOTS 3
struct PinnedBuf { void* p = nullptr; size_t cap = 0; };      // a pinned host block (ensure_pinned)
struct FrameSlot { PinnedBuf host; hipEvent_t done = nullptr; bool busy = false; };
// one joint palette on its way to the device (swr_mesh_skin): pinned staging, its device copy, an event behind the kernel that reads it
struct PaletteSlot { PinnedBuf host; DevBuf dev; hipEvent_t done = nullptr; bool busy = false; };
#define SWR_PALETTE_SLOTS_MAX 256

// Everything of a batch that its raster kernel reads (or that a front-end kernel and the raster kernel share).  With frames
// pipelined two sets alternate per flush, so the front end of flush N+1 never writes what the raster kernel of flush N reads;
// with pipelining off only set 0 is used.  Buffers only the front end touches (slot_tb, want, tile_list, pair_tile, the scan's
// totals) are single: front ends run in order on one stream.
struct RasterSet {
    DevBuf d_upload;         // draws | vertex block map | triangle block map [| bounds pointers | visibility words] of the batch
    DevBuf d_vout, d_vnorm, d_recs;
    DevBuf d_masks, d_pcounts, d_pair_refs;
    DevBuf d_tile_count, d_tile_start;
    DevBuf d_order;          // [tile_order n_tiles] uint4 {tile, list start, pairs, -}, [tile_work n_tiles][hist 256][cursor 256] u32, [tile_bucket n_tiles] u8: heaviest-first raster order
    uint32_t hist_tiles = 0; // tile count the fragment history in d_order (tile_work) belongs to (0: none yet)
    hipEvent_t front_done = nullptr, raster_done = nullptr;
    bool raster_pending = false;      // raster_done has been recorded and the stream has not been drained since
};

// A user program loaded on the context's device (swr_program_create / _vf): the two k_raster_c<SWR_PROG_CUSTOM> instantiations
// (with / without BlendMode.None's row early-out) of its run-time compiled code object and, when it has a vertex half, the module's
// k_vertex_user and the k_setup whose clipper lerps data4.w (swr_geometry.hip.h).  Shared by the context's table and every
// recorded or in-flight draw that uses it: the module is unloaded when the last of them lets go, and a batch only lets go once its
// kernels are known to be over (retire_batch / free_garbage).
struct UserProg {
    hipModule_t mod = nullptr;
    hipFunction_t fn[2] = { nullptr, nullptr };     // [EARLYOUT]
    hipFunction_t vertex_fn = nullptr, setup_fn = nullptr;   // programs with a vertex half only: launched instead of k_vertex / k_setup
    float constants[SWR_USER_CONSTANTS] = {};        // swr_program_set_constants: copied into each draw when it is recorded
    const swr_texture* tex[SWR_PROGRAM_TEXTURES - 1] = {};   // swr_program_set_texture, slots 1 ..: captured (texture_slot_of) by each draw likewise
    ~UserProg() { if (mod) (void)hipModuleUnload(mod); }
};

// The k_post instantiations of a post program (swr_post.hip.h), by the FORMAT each is instantiated with: the three present formats
// and the two texel formats of swr_texture_update_from_post.  rtc_compile_post names them, swr_post_create loads them and the
// launches select from them, all by this list.
enum PostKernel { POST_RGB32F, POST_RGB8, POST_RGBX8, POST_TEXELS_OPAQUE, POST_TEXELS_KEEP, POST_KERNELS };
constexpr int POST_KERNEL_FORMAT[POST_KERNELS] = { SWR_POST_RGB32F, SWR_POST_RGB8, SWR_POST_RGBX8, SWR_POST_TEXELS_OPAQUE, SWR_POST_TEXELS_KEEP };

// A post-process program loaded on the context's device (swr_post_create): the k_post instantiations of its run-time compiled code
// object.  A destroyed program is parked (post_garbage) until the streams are idle: a present enqueued with it may still be running.
struct PostProg {
    hipModule_t mod = nullptr;
    hipFunction_t fn[POST_KERNELS] = {};                    // [PostKernel]
    PostConstants constants = {};                           // swr_post_set_constants: passed by value to each launch
    const swr_texture* tex[SWR_POST_TEXTURES] = {};         // swr_post_set_texture: read (with each texture's filter) at each launch
    ~PostProg() { if (mod) (void)hipModuleUnload(mod); }
};

// the per-draw block of a user-program batch as the device reads it (SWR_USER_BLOCK_WORDS, swr_device.h).  Two draws share their
// fragment-stage state only if their blocks are bitwise equal (batch_geometry), so it has no padding and is compared with memcmp.
struct UserBlock {
    float constants[SWR_USER_CONSTANTS];
    TextureSlot tex[SWR_PROGRAM_TEXTURES - 1];
};
static_assert(sizeof(UserBlock) == SWR_USER_BLOCK_WORDS * sizeof(float) && offsetof(UserBlock, tex) == SWR_USER_CONSTANTS * sizeof(float),
              "the block k_raster_c and k_vertex_user index by SWR_USER_BLOCK_WORDS");

struct DrawCmd {
    DrawParams p;
    swr_mesh* mesh;
    bool frustum_cull = false;                 // render only if IsSphereInFrustum(mesh bounds, model, view, proj)
    std::shared_ptr<UserProg> prog;            // user programs only: the program ...
    std::shared_ptr<const UserBlock> ublock;   // ... and its constants and texture slots 1 .. as they were when the draw was recorded
};

// one flush = one batch; kept until the host has seen that it fitted (optimistic execution, see swr::Ctrl)
struct Batch {
    std::vector<DrawCmd> draws;
    bool clear_color = false, clear_depth = false;
    float clear_rgba[4] = { 0, 0, 0, 0 };
    float near_clip = 0.1f;
    bool wireframe = false;                    // Rasterizer.RenderDebugMode == Wireframe for the whole batch
    uint32_t seq = 0;
    float4* color = nullptr;                   // the framebuffer bound when the batch was flushed: a replay (validate_locked) must
    float* depth = nullptr;                    // hit the same buffers even if the caller has bound others since (double buffering)
};

}  // namespace

struct swr_context {
    int device = 0;
    std::mutex mu;
    std::string err;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipStream_t front_stream = nullptr;    // front ends of pipelined flushes (and mesh uploads, which only front-end kernels read)
    int pipelining = 1;                    // swr_set_pipelining: 0 off, 1 every batch (default), 2 small frames / small batches only (see execute_batch)
    uint32_t pipeline_max_tris = 1u << 17; // mode 2: a batch is pipelined when it has at most this many triangles ...
    uint32_t pipeline_max_tiles = 1u << 15;   // ... or the band at most this many tiles (8 raster waves per wave slot of the chip)
    hipEvent_t f_tail_ev = nullptr, r_front_ev = nullptr;
    bool f_tail_pending = false;           // the front stream carries work (a front end, a mesh upload) the raster stream has not been ordered behind
    bool r_front_pending = false;          // an unpipelined batch ran its front end on the raster stream since the front stream last waited for it
    RasterSet sets[2];
    uint32_t raster_span_no = 0;           // profiling mode 3: raster launches seen since swr_profile_enable
    char dev_name[256] = { 0 };

    int W = 0, H = 0, tiles_x = 0, tiles_y = 0;
    bool geometry_applied = false;            // swr_resize has run at least once (a second call with the same size is a no-op)
    bool band_set = false;
    int band_first = 0, band_count = 0;       // as requested by swr_set_band
    int band_ty0 = 0, band_ty1 = 0;           // effective
    int il_k = 0, il_world = 1, il_rank = 0;  // swr_set_band_interleaved: stripes of il_k tile rows, stripe s belongs to rank s % il_world
    int band_tile_rows = 0;                   // tile rows this context stores (contiguous band or stripes)
    float4* color = nullptr;                  // band storage in use (own or external)
    float* depth = nullptr;
    DevBuf own_color, own_depth;
    void* ext_color = nullptr; void* ext_depth = nullptr;

    uint32_t nm_flags = SWR_NUMERICS_FMA ? (SWR_NM_TRANSFORM_FMA | SWR_NM_TRANSFORM_NORMAL_FMA) : 0u;   // swr_set_transform_fma
    float near_clip = 0.1f, far_clip = 1000.0f;   // Rasterizer.cs:20-21
    int debug_mode = SWR_DEBUG_NONE;               // Rasterizer.cs:22

    bool pend_clear_color = false, pend_clear_depth = false;
    float clear_rgba[4] = { 0, 0, 0, 0 };

    std::vector<DrawCmd> draws;
    uint64_t pend_verts = 0, pend_tris = 0;
    std::vector<swr_mesh*> garbage;           // transient meshes no recorded draw needs any more, possibly still read by kernels in flight
    std::map<int, std::shared_ptr<UserProg>> progs;     // live user programs by id (swr_program_create / _destroy)
    int next_prog = SWR_PROG_USER_BASE;
    std::vector<std::shared_ptr<UserProg>> prog_garbage; // programs of retired batches whose kernels may still run (see garbage)
    std::map<int, std::shared_ptr<PostProg>> posts;     // live post-process programs by id (swr_post_create / _destroy)
    std::vector<std::shared_ptr<PostProg>> post_garbage; // destroyed post programs whose kernel may still run (see garbage)
    DevBuf post_plane;                        // the resolved RGBA plane k_resolve_rgba hands k_post (factors other than (1, 1)): allocated on
                                              // first use, grown only with the stream idle; producer and consumer are both on `stream`
    std::vector<swr_mesh*> mesh_pool;         // transient meshes whose batches are KNOWN to be complete: their device buffers are handed to the
    size_t mesh_pool_bytes = 0;               // next swr_render_mesh_arrays call instead of hipFree / hipMalloc (both synchronise the device)
    uint64_t stale_dropped[2] = { 0, 0 };     // present tickets dropped by back-pressure whose pixels predate a replay (swr_present_wait reports them)
    std::vector<Batch> inflight;              // launched optimistically, not yet validated
    uint32_t next_seq = 1;
    bool sync_flush = false;                  // SWR_SYNC_FLUSH=1: read the pair total back in every flush
    uint32_t debug_fill_capacity = 0;         // SWR_DEBUG_FILL_CAPACITY=n: k_bin<FILL> of optimistic flushes sees a list of n entries (tests)

    DevBuf d_slot_tb;        // (the vertex-stage output, the records and the upload block live in the RasterSets)
    FrameSlot slots[SWR_SLOTS];
    uint32_t slot_next = 0;
    DevBuf d_pair_tile, d_ctrl;
    uint32_t* host_poison = nullptr;           // pinned, device-visible copy of Ctrl::poison
    DevBuf d_tile_list, d_tile_stats, d_counters, d_total, d_scratch;
    DevBuf d_want;           // 1 byte per slot: which tiles of a small slot are binned -- written by k_setup, replayed by both k_bin passes
    size_t tile_stats_tiles = 0;
    swr_stats totals = {};
    unsigned long long host_tile_pairs = 0;   // rounds sized on the host (MODE_SYNC)
    unsigned long long replays = 0;           // times an optimistic batch did not fit and was replayed
    unsigned long long host_syncs = 0;        // times an entry point made the host wait for the stream (swr_sync_count)
    // asynchronous present (swr_present_rgb_async and its resolved and 8-bit forms): two device staging buffers alternate, sized in
    // bytes for whichever payload format used them last; the payload kernel runs on `stream`, the copy to the host on `copy_stream`,
    // so the next frame renders while this one crosses PCIe
    hipStream_t copy_stream = nullptr;
    DevBuf present_buf[2];
    hipEvent_t present_flat[2] = { nullptr, nullptr }, present_done[2] = { nullptr, nullptr };
    uint64_t present_ticket[2] = { 0, 0 };    // ticket whose copy the slot carries (0 = none pending)
    uint32_t present_seq[2] = { 0, 0 };       // last batch flushed before that present: retired when the copy is known to be over
    uint64_t next_ticket = 0;

    // swr_raycast / swr_raycast_nearest: a stream of their own (a query does not queue behind a frame in flight), idle between calls
    // swr_texture_update_from_frame between two contexts: recorded on this context's stream behind its frame (the updating context's
    // stream waits for it) and, in the updating context, behind the kernel (this context's stream waits before it touches the frame again)
    hipEvent_t rtt_frame_ev = nullptr, rtt_done_ev = nullptr;

    hipStream_t ray_stream = nullptr;
    DevBuf d_ray, d_ray_best;                  // rays | targets | hit records; the pairs' keys, all SWR_RAY_NO_HIT between calls (k_ray_finish)
    PinnedBuf ray_host;                        // staging block of small queries
    DevBuf d_char;                             // swr_character_update: controllers | inputs | ring | targets | work | active | rays x 2 | results

    // swr_mesh_skin: a palette's slot is free again once the kernel that read it is over (event query, no wait); the list grows while
    // none is free, so several calls per frame never overwrite a palette a queued kernel has not read
    std::vector<PaletteSlot> palettes;
    size_t palette_next = 0;
    // swr_mesh_skin_batch: the events its destinations share; one that no mesh holds any more is recorded again
    std::vector<std::shared_ptr<SharedEvent>> pose_events;

    int profiling = 0;                         // 0 off, 1 every stage, 2 only the raster kernel (2 events per flush)
    std::vector<EventSpan> spans;
    std::vector<float> raster_samples;         // duration of every raster launch that carried an event pair since swr_profile_reset (<= 65,536)
    std::vector<hipEvent_t> event_pool;
    swr_profile prof = {};
};

namespace {

#define SWR_HIP(ctx, call)                                                                        \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            char b_[512];                                                                         \
            snprintf(b_, sizeof b_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            (ctx)->err = b_;                                                                      \
            return e_ == hipErrorOutOfMemory ? SWR_ERR_OOM : SWR_ERR_HIP;                         \
        }                                                                                         \
    } while (0)

int fail(swr_context* c, int code, const char* msg) { c->err = msg; return code; }
// ... and a HIP error behind `what` ("texture upload failed: "), for the calls that clean up before they report
int fail_hip(swr_context* c, const char* what, hipError_t e) {
    c->err = std::string(what) + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? SWR_ERR_OOM : SWR_ERR_HIP;
}

int ensure(swr_context* c, DevBuf& b, size_t bytes, bool zero_new = false) {
    if (bytes <= b.cap) return SWR_OK;
    size_t want = std::max(bytes, b.cap + b.cap / 2);
    if (b.p) { SWR_HIP(c, hipFree(b.p)); b.p = nullptr; b.cap = 0; }
    SWR_HIP(c, hipMalloc(&b.p, want));
    b.cap = want;
    if (zero_new) SWR_HIP(c, hipMemsetAsync(b.p, 0, want, c->stream));
    return SWR_OK;
}

void release(DevBuf& b) { if (b.p) (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
void release(PinnedBuf& b) { if (b.p) (void)hipHostFree(b.p); b.p = nullptr; b.cap = 0; }

// A pinned block of at least want_cap bytes (the old contents are not kept).  Sizing want_cap and what a failure means are the caller's.
hipError_t ensure_pinned(PinnedBuf& b, size_t want_cap) {
    if (b.cap >= want_cap) return hipSuccess;
    release(b);
    const hipError_t e = hipHostMalloc(&b.p, want_cap, hipHostMallocDefault);
    if (e == hipSuccess) b.cap = want_cap; else b.p = nullptr;
    return e;
}
// A run-time value that is a kernel's template argument: f gets it as a std::integral_constant (`decltype(x)::value` in a generic lambda).
// The result type is stated, not deduced: deduction would instantiate f's kernels where the call stands, ahead of the frame's kernels.
template <class R = void, class F> R with_flag(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
template <class R = void, class F> R with_factor(int k, F&& f) {            // a resolve factor: 1, 2, 4 or 8 (resolve_factor_ok)
    return k == 1 ? f(std::integral_constant<int, 1>{}) : k == 2 ? f(std::integral_constant<int, 2>{})
         : k == 4 ? f(std::integral_constant<int, 4>{}) : f(std::integral_constant<int, 8>{});
}
template <class R, class F> R with_factors(int kx, int ky, F&& f) {         // a delivery kernel's factor pair: f(x, y)
    return with_factor<R>(kx, [&](auto x) -> R { return with_factor<R>(ky, [&](auto y) -> R { return f(x, y); }); });
}

// Frame-slot ring: a batch takes the next slot = {pinned staging block for its upload, completion event}.
// Taking a slot first waits for the batch that used it SWR_SLOTS flushes ago, which (a) makes the pinned block
// safe to overwrite and (b) bounds how far the host runs ahead of the GPU (pageable uploads and unbounded
// queue depth both serialise the stream on some HIP runtimes).
void* slot_acquire(swr_context* c, size_t bytes) {
    FrameSlot& fs = c->slots[c->slot_next % SWR_SLOTS];
    if (fs.busy) { (void)hipEventSynchronize(fs.done); fs.busy = false; }
    if (fs.host.cap < bytes && ensure_pinned(fs.host, std::max<size_t>(bytes + bytes / 2, 1 << 16)) != hipSuccess) return nullptr;
    return fs.host.p;
}
void slot_submit(swr_context* c) {            // call after the batch's last launch
    FrameSlot& fs = c->slots[c->slot_next % SWR_SLOTS];
    if (!fs.done) (void)hipEventCreateWithFlags(&fs.done, hipEventDisableTiming);
    if (fs.done && hipEventRecord(fs.done, c->stream) == hipSuccess) fs.busy = true;
    c->slot_next++;
}

BandMap host_band_map(const swr_context* c) {
    BandMap b; b.ty0 = c->band_ty0; b.ty1 = c->band_ty1; b.il_k = c->il_k; b.il_world = c->il_world; b.il_rank = c->il_rank;
    return b;
}
int band_y0(const swr_context* c) { return c->band_ty0 * SWR_TILE; }     // contiguous band only
// pixel rows stored: the band's tile rows, 16 pixel rows each, the frame's last tile row possibly partial
int band_rows(const swr_context* c) {
    if (c->band_tile_rows <= 0) return 0;
    const int last_global = band_global_row(host_band_map(c), c->band_tile_rows - 1);
    const int last_rows = std::min(SWR_TILE, c->H - last_global * SWR_TILE);
    return (c->band_tile_rows - 1) * SWR_TILE + std::max(0, last_rows);
}
// row of pixel row y in the band's buffers, -1 if the band does not hold it
int band_local_pixel_row(const swr_context* c, int y) {
    if (y < 0 || y >= c->H) return -1;
    const int lr = band_local_row(host_band_map(c), y / SWR_TILE);
    return lr < 0 ? -1 : lr * SWR_TILE + y % SWR_TILE;
}
size_t band_pixels(const swr_context* c) { return (size_t)std::max(0, c->W) * (size_t)band_rows(c); }

int apply_geometry(swr_context* c) {
    c->tiles_x = c->W > 0 ? (c->W + SWR_TILE - 1) / SWR_TILE : 0;     // Rasterizer.cs:76-77
    c->tiles_y = c->H > 0 ? (c->H + SWR_TILE - 1) / SWR_TILE : 0;
    if (c->il_k > 0) {
        c->band_ty0 = 0; c->band_ty1 = c->tiles_y;                     // ownership is decided row by row (BandMap)
        int rows = 0;
        for (int ty = 0; ty < c->tiles_y; ++ty) rows += band_local_row(host_band_map(c), ty) >= 0 ? 1 : 0;
        c->band_tile_rows = rows;
    } else {
        if (c->band_set) {
            c->band_ty0 = std::min(std::max(c->band_first, 0), c->tiles_y);
            c->band_ty1 = std::min(c->band_ty0 + std::max(c->band_count, 0), c->tiles_y);
        } else {
            c->band_ty0 = 0; c->band_ty1 = c->tiles_y;
        }
        c->band_tile_rows = c->band_ty1 - c->band_ty0;
    }
    size_t n = band_pixels(c);
    if (c->ext_color) {
        c->color = (float4*)c->ext_color; c->depth = (float*)c->ext_depth;
    } else {
        int rc;
        if ((rc = ensure(c, c->own_color, std::max<size_t>(n, 1) * sizeof(float4), false))) return rc;
        if ((rc = ensure(c, c->own_depth, std::max<size_t>(n, 1) * sizeof(float), false))) return rc;
        c->color = c->own_color.as<float4>(); c->depth = c->own_depth.as<float>();
    }
    return SWR_OK;
}

FrameParams frame_params(const swr_context* c, float near_clip) {      // (a batch keeps the NearClip it was recorded under)
    FrameParams fp;
    fp.width = c->W; fp.height = c->H; fp.tiles_x = c->tiles_x; fp.tiles_y = c->tiles_y;
    fp.band_ty0 = c->band_ty0; fp.band_ty1 = c->band_ty1;
    fp.band_y0 = band_y0(c); fp.band_rows = band_rows(c);
    fp.il_k = c->il_k; fp.il_world = c->il_world; fp.il_rank = c->il_rank; fp.band_tile_rows = c->band_tile_rows;
    fp.near_clip = near_clip;
    return fp;
}

hipEvent_t get_event(swr_context* c) {
    if (!c->event_pool.empty()) { hipEvent_t e = c->event_pool.back(); c->event_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    // timing only, never ordering: no system-scope fence (the default event's cache write-back / invalidation would hit the OTHER
    // stream's kernels when frames are in flight -- measured: 20 timed frames 0.651 ms with default events, see SWR_EVENT_FLAGS)
    if (hipEventCreateWithFlags(&e, SWR_TIMING_EVENT_FLAGS) != hipSuccess) (void)hipEventCreate(&e);
    return e;
}
struct ScopedSpan {
    swr_context* c; int stage; hipEvent_t a = nullptr, b = nullptr;
    hipStream_t s;
    bool on = false;
    ScopedSpan(swr_context* c_, int st, hipStream_t s_ = nullptr) : c(c_), stage(st), s(s_ ? s_ : c_->stream) {
        // 1: every stage; 2: the raster kernel of every flush; 3: the raster kernel of every 4th flush (an event pair costs
        // about 10 us of stream time: sampling keeps a timed region within 0.5 % of its unobserved rate)
        on = c->profiling == 1 || (st == ST_RASTER && (c->profiling == 2 || (c->profiling == 3 && (c->raster_span_no++ & 3u) == 0u)));
        if (on) { a = get_event(c); b = get_event(c); (void)hipEventRecord(a, s); }
    }
    ~ScopedSpan() {
        if (on) { (void)hipEventRecord(b, s); c->spans.push_back({ stage, a, b }); }
    }
};

void collect_spans(swr_context* c) {      // stream must be idle
    for (auto& s : c->spans) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) {
            switch (s.stage) {
            case ST_VERTEX: c->prof.vertex_ms += ms; break;
            case ST_SETUP:  c->prof.setup_ms += ms; break;
            case ST_BIN:    c->prof.bin_ms += ms; break;
            case ST_SORT:   c->prof.sort_ms += ms; break;
            case ST_COVER:  c->prof.cover_ms += ms; break;
            case ST_RASTER: c->prof.raster_ms += ms; c->prof.raster_launches++;
                            if (c->raster_samples.size() < 65536) c->raster_samples.push_back(ms);
                            break;
            case ST_CLEAR:  c->prof.clear_ms += ms; break;
            }
            c->prof.total_ms += ms;
        }
        c->event_pool.push_back(s.a); c->event_pool.push_back(s.b);
    }
    c->spans.clear();
}

// the stream mesh uploads and front-end-only work go to: the front stream while frames are pipelined, else the context's stream
// (and notes that the front stream now carries work the raster stream has not been ordered behind)
hipStream_t use_front_stream(swr_context* c) {
    if (c->pipelining && c->front_stream) { c->f_tail_pending = true; return c->front_stream; }
    return c->stream;
}

// creates the front stream (once) and the hand-over events
int ensure_front_stream(swr_context* c) {
    if (!c->pipelining || c->front_stream) return SWR_OK;
    int least = 0, greatest = 0;
    SWR_HIP(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
    // high priority: the front end's short kernels go first wherever a slot frees up, the raster kernel (65,536 one-wave workgroups)
    // fills the rest (default priority measured the same within noise, profiles/r04_frames_in_flight.md)
    SWR_HIP(c, hipStreamCreateWithPriority(&c->front_stream, hipStreamNonBlocking, greatest));
    SWR_HIP(c, hipEventCreateWithFlags(&c->f_tail_ev, hipEventDisableTiming));
    SWR_HIP(c, hipEventCreateWithFlags(&c->r_front_ev, hipEventDisableTiming));
    for (auto& s : c->sets) {
        if (!s.front_done) SWR_HIP(c, hipEventCreateWithFlags(&s.front_done, SWR_HANDOVER_EVENT_FLAGS));
        if (!s.raster_done) SWR_HIP(c, hipEventCreateWithFlags(&s.raster_done, SWR_HANDOVER_EVENT_FLAGS));
    }
    return SWR_OK;
}
}  // namespace
