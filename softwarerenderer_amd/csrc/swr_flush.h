// swr_flush.h -- the flush path: recorded draws -> one batch -> kernels on the context's streams, its validation and replay,
// and the mesh pool.  Included by swr_api.hip only, after swr_host.h.
#pragma once
#include "swr_raster_select.h"

namespace {
// the batch has kernels of its own (DEBUG_VARYINGS or ONE user program): 0 for every other built-in program
int kernel_class(int program) { return program == SWR_PROG_DEBUG_VARYINGS || program >= SWR_PROG_USER_BASE ? program : 0; }

void destroy_mesh(swr_mesh* m) {
    if (m->d_verts) (void)hipFree(m->d_verts);
    if (m->d_idx) (void)hipFree(m->d_idx);
    if (m->d_bounds) (void)hipFree(m->d_bounds);
    if (m->uploaded) (void)hipEventDestroy(m->uploaded);
    if (m->d_joints) (void)hipFree(m->d_joints);
    if (m->d_weights) (void)hipFree(m->d_weights);
    delete m;
}
// A transient mesh (swr_render_mesh_arrays: the reference's RenderMesh(vertices, indices, ...) makes one per call) whose batch is
// complete goes to the pool, not to hipFree: freeing synchronises the whole device, which is exactly what an asynchronous present
// loop must not do, and the next call with arrays of that size needs the same buffers again.
const size_t kMeshPoolBytes = (size_t)1 << 30;
void trim_mesh_pool(swr_context* c) {      // keeps the newest meshes up to the byte budget (hipFree: a device-wide wait unless the streams are idle)
    while (c->mesh_pool_bytes > kMeshPoolBytes && !c->mesh_pool.empty()) {
        swr_mesh* m = c->mesh_pool.front();
        c->mesh_pool.erase(c->mesh_pool.begin());
        c->mesh_pool_bytes -= m->cap_verts + m->cap_idx;
        destroy_mesh(m);
    }
}
void pool_mesh(swr_context* c, swr_mesh* m) {
    c->mesh_pool.push_back(m);
    c->mesh_pool_bytes += m->cap_verts + m->cap_idx;
    // a present loop that never drains and whose array sizes never repeat would grow the pool for ever: past twice the budget the
    // oldest (unused: pooled meshes are complete) are freed here, at the price of one device-wide wait
    if (c->mesh_pool_bytes > 2 * kMeshPoolBytes) trim_mesh_pool(c);
}
void free_garbage(swr_context* c) {       // streams must be idle: nothing in flight reads the garbage any more
    for (swr_mesh* m : c->garbage) pool_mesh(c, m);
    c->garbage.clear();
    c->prog_garbage.clear();
    c->post_garbage.clear();
    trim_mesh_pool(c);
}

int validate_locked(swr_context* c);

// both streams idle (the raster stream waits for every front end it depends on; the front stream may carry mesh uploads beyond that)
int drain_streams(swr_context* c) {
    SWR_HIP(c, hipStreamSynchronize(c->stream));
    if (c->front_stream) SWR_HIP(c, hipStreamSynchronize(c->front_stream));
    for (auto& s : c->sets) s.raster_pending = false;
    c->f_tail_pending = c->r_front_pending = false;
    return SWR_OK;
}

int sync_locked(swr_context* c) {
    ++c->host_syncs;
    int rc = drain_streams(c);
    if (rc) return rc;
    rc = validate_locked(c);
    collect_spans(c);
    free_garbage(c);
    for (auto& fs : c->slots) fs.busy = false;     // stream idle: every slot is free
    return rc;
}

enum { MODE_SYNC = 0, MODE_ASYNC = 1 };
// The upload block of a batch (RasterSet::d_upload and its pinned staging copy): draws | vertex block map | triangle block map
// | bounds pointers | visibility words | captured user blocks (UserBlock: SWR_USER_BLOCK_WORDS words per draw), every part on a
// 256-byte boundary.  The bounds pointers and visibility words are there only when some draw is frustum-culled, the user blocks only
// in a user-program batch.
struct UploadLayout { size_t off_vb, off_tb, off_bp, off_vis, off_consts, bytes; };
static UploadLayout upload_layout(size_t nd, size_t v_blocks, size_t t_blocks, bool any_cull, bool user) {
    const auto r256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
    UploadLayout u;
    u.off_vb = r256(nd * sizeof(DrawParams));
    u.off_tb = r256(u.off_vb + v_blocks * sizeof(BlockMap));
    u.off_bp = r256(u.off_tb + t_blocks * sizeof(BlockMap));
    u.off_vis = r256(u.off_bp + (any_cull ? nd * sizeof(void*) : 0));
    const size_t vis_end = u.off_vis + (any_cull ? nd * 4 : 0);
    u.off_consts = r256(vis_end);
    u.bytes = user ? u.off_consts + nd * sizeof(UserBlock) : vis_end;
    return u;
}
template <class T> T* at(void* base, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }

// the five regions of RasterSet::d_order (16-byte records first: alignment); the buffer has always had 4 bytes per tile to spare
struct OrderView { uint4* tile_order; uint32_t* tile_work; uint32_t* hist; uint32_t* cursor; uint8_t* tile_bucket; };
static size_t order_bytes(uint32_t n_tiles) { return (size_t)n_tiles * (sizeof(uint4) + 4 + 1 + 4) + 2 * SWR_ORDER_BUCKETS * 4; }
static OrderView order_view(RasterSet& S, uint32_t n_tiles) {
    uint4* order = S.d_order.as<uint4>();
    uint32_t* work = reinterpret_cast<uint32_t*>(order + n_tiles), *hist = work + n_tiles, *cursor = hist + SWR_ORDER_BUCKETS;
    return { order, work, hist, cursor, reinterpret_cast<uint8_t*>(cursor + SWR_ORDER_BUCKETS) };
}

// one execution of a batch (a flush or its replay): what execute_batch decides once and every stage below shares
struct Pass {
    const Batch& b;
    RasterSet& S;          // what the batch's raster kernel reads
    hipStream_t F;         // the stream its front end runs on
    int mode;
    bool cc, cd;           // clears still owed: the first raster kernel pays them, or run_clear
    UploadLayout up = {};
    uint32_t odd_base = 0;  // the batch's record layout (rec_index, swr_device.h): filled batches dense, wireframe 0 = one record per slot
};

// the batch's fragment program reads VertexOutput.Normal (DEBUG_VARYINGS, every user program): k_vertex and the clipper store it
static bool b_needs_vnorm(const Batch& b) { return !b.draws.empty() && kernel_class(b.draws[0].p.program) != 0; }
static bool b_has_user_program(const Batch& b) { return !b.draws.empty() && b.draws[0].p.program >= SWR_PROG_USER_BASE; }
// ... and that program has a vertex half: its k_vertex_user and k_setup run instead of the library's
static bool b_has_user_vertex(const Batch& b) { return b_has_user_program(b) && b.draws[0].prog && b.draws[0].prog->vertex_fn; }
#ifndef SWR_DENSE_RECORDS
#define SWR_DENSE_RECORDS 1     // 0: records indexed by slot in filled batches too (A/B switch of profiles/r07_front_end_records.md)
#endif
const unsigned long long kMaxPairs = 1ull << 30;       // list entries per round (4 GiB of slot ids)

// pairs every set in use can hold (the optimistic flush is checked against this on the device)
size_t pair_capacity(const swr_context* c) {
    size_t cap = std::min(c->d_tile_list.cap / 4, c->d_pair_tile.cap / 4);
    for (int i = 0; i < (c->pipelining ? 2 : 1); ++i) {
        const RasterSet& s = c->sets[i];
        cap = std::min(cap, std::min(std::min(s.d_masks.cap / 32, s.d_pcounts.cap / 8), s.d_pair_refs.cap / 16));
    }
    return cap;
}
int ensure_pairs(swr_context* c, size_t n) {
    int rc;
    if ((rc = ensure(c, c->d_tile_list, n * 4))) return rc;
    if ((rc = ensure(c, c->d_pair_tile, n * 4))) return rc;
    for (int i = 0; i < (c->pipelining ? 2 : 1); ++i) {
        RasterSet& s = c->sets[i];
        if ((rc = ensure(c, s.d_masks, n * 32))) return rc;
        if ((rc = ensure(c, s.d_pair_refs, n * 16))) return rc;
        if ((rc = ensure(c, s.d_pcounts, n * 8 + 64))) return rc;
    }
    return SWR_OK;
}

int run_clear(swr_context* c, const Batch& b, bool& cc, bool& cd) {
    size_t n = band_pixels(c);
    if (n && (cc || cd)) {
        ScopedSpan sp(c, ST_CLEAR);
        int blocks = (int)std::min<size_t>((n + 255) / 256, 2048 * 8);
        float4 rgba = make_float4(b.clear_rgba[0], b.clear_rgba[1], b.clear_rgba[2], b.clear_rgba[3]);
        hipLaunchKernelGGL(k_clear, dim3(blocks), dim3(256), 0, c->stream, b.color, b.depth, n, rgba,
                           cc ? 1 : 0, cd ? 1 : 0, (const Ctrl*)c->d_ctrl.as<Ctrl>(), b.seq);
        SWR_HIP(c, hipGetLastError());
    }
    cc = cd = false;
    return SWR_OK;
}

int launch_raster(swr_context* c, Pass& P, uint32_t n_tiles);

// Bins slots [lo, hi) of the pass's batch on P.F -- count, scan, fill (+ the tile order in the grid's last blocks), sort, cover --,
// hands over to the context's stream and rasterises them there.  MODE_SYNC reads the pair total back (sizes buffers exactly, splits
// a range that would need more than kMaxPairs entries); MODE_ASYNC launches everything against the current capacity.
// counts_clear: k_vertex of this batch cleared the per-tile counters and the tile order's histogram (no memsets here)
int bin_and_raster(swr_context* c, Pass& P, uint32_t lo, uint32_t hi, bool counts_clear = false) {
    const uint32_t n_tiles = (uint32_t)c->tiles_x * (uint32_t)c->band_tile_rows;
    if (n_tiles == 0 || lo >= hi) return SWR_OK;
    int rc;
    const Batch& b = P.b; RasterSet& S = P.S;
    const hipStream_t F = P.F; const int mode = P.mode;
    const Ctrl* ctrl = c->d_ctrl.as<Ctrl>();
    unsigned long long* d_total = c->d_total.as<unsigned long long>();
    const OrderView ov = order_view(S, n_tiles);
    BinArgs ba;
    ba.slot_tb = c->d_slot_tb.as<unsigned long long>();
    ba.recs = S.d_recs.as<TriRec>();
    ba.odd_base = P.odd_base;
    ba.slot_lo = lo; ba.slot_hi = hi;
    ba.spt = b.wireframe ? 6u : 2u;
    ba.width = c->W; ba.height = c->H;
    ba.tiles_x = c->tiles_x;
    ba.band = host_band_map(c);               // (the same context fields frame_params() hands k_setup, which decided `want` by them)
    ba.tile_count = S.d_tile_count.as<uint32_t>();
    ba.tile_start = S.d_tile_start.as<uint32_t>();
    ba.tile_list = c->d_tile_list.as<uint32_t>();
    ba.list_capacity = (uint32_t)std::min<size_t>(pair_capacity(c), 0xffffffffu);
    ba.counters = c->d_counters.as<Counters>();
    ba.ctrl = c->d_ctrl.as<Ctrl>();
    ba.seq = b.seq; ba.replayable = mode == MODE_ASYNC ? 1u : 0u;
    ba.total = c->d_total.as<unsigned long long>();
    ba.want = c->d_want.as<uint8_t>();
    const uint32_t bin_threads = (hi - lo + ba.spt - 1u) / ba.spt;          // = triangles
    ba.tpw = 64u;                                                            // aim for >= ~1000 waves
    while (ba.tpw > 4u && bin_threads < ba.tpw * 1024u) ba.tpw >>= 1;
    const uint32_t bin_blocks = (bin_threads + 4u * ba.tpw - 1u) / (4u * ba.tpw);
    {
        ScopedSpan sp(c, ST_BIN, F);
        if (!counts_clear) {
            SWR_HIP(c, hipMemsetAsync(ba.tile_count, 0, (size_t)n_tiles * 4, F));
            SWR_HIP(c, hipMemsetAsync(ov.hist, 0, 2 * SWR_ORDER_BUCKETS * 4, F));
        }
        hipLaunchKernelGGL(k_bin<false>, dim3(bin_blocks), dim3(256), 0, F, ba);
        const unsigned scan_blocks = (n_tiles + (unsigned)SWR_SCAN_BLOCK - 1u) / (unsigned)SWR_SCAN_BLOCK;
        unsigned long long* sums = d_total + 32;      // room for 4096 block sums (2^20 tiles)
        hipLaunchKernelGGL(k_scan_sums, dim3(scan_blocks), dim3(SWR_SCAN_BLOCK), 0, F, (const uint32_t*)ba.tile_count, n_tiles, sums);
        // async: the device decides whether the batch fits; sync: the host does (capacity "infinite" here)
        const unsigned long long cap = mode == MODE_ASYNC ? (unsigned long long)ba.list_capacity : ~0ull;
        hipLaunchKernelGGL(k_scan_apply, dim3(scan_blocks), dim3(SWR_SCAN_BLOCK), 0, F, ba.tile_count,
                           S.d_tile_start.as<uint32_t>(), n_tiles, (const unsigned long long*)sums, d_total,
                           cap, b.seq, c->d_ctrl.as<Ctrl>(), c->d_counters.as<Counters>() + 64,
                           mode == MODE_ASYNC ? 1 : 0, (const uint32_t*)ov.tile_work, ov.hist, ov.tile_bucket);
        SWR_HIP(c, hipGetLastError());
    }
    uint32_t cover_items = ba.list_capacity;          // async: grid covers the whole capacity, lanes beyond the total exit
    if (mode == MODE_SYNC) {
        unsigned long long total = 0;
        SWR_HIP(c, hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, F));      // (MODE_SYNC: F is the context's stream)
        SWR_HIP(c, hipStreamSynchronize(F));
        if (total > kMaxPairs && hi - lo > 2) {
            // too many (triangle, tile) pairs for one round: split the slot range.  Order is preserved
            // because the framebuffer carries the state from one round to the next.
            uint32_t mid = lo + (((hi - lo) / 2u) & ~1u);
            if (mid == lo) mid = lo + 2;
            if ((rc = bin_and_raster(c, P, lo, mid))) return rc;
            return bin_and_raster(c, P, mid, hi);
        }
        if (total == 0) return run_clear(c, b, P.cc, P.cd);
        if (total > 0xffffffffull) return fail(c, SWR_ERR_UNSUPPORTED, "a single triangle covers more tile pairs than one round can hold");
        c->host_tile_pairs += total;                  // tile_pairs of a round that really runs
        // a little headroom so that the next, similar frame can run without reading the total back
        if ((rc = ensure_pairs(c, (size_t)std::min<unsigned long long>(total + total / 4 + 4096, std::max(total, kMaxPairs))))) return rc;
        ba.tile_list = c->d_tile_list.as<uint32_t>();
        ba.list_capacity = (uint32_t)std::min<size_t>(pair_capacity(c), 0xffffffffu);
        cover_items = (uint32_t)total;
    }
    {
        ScopedSpan sp(c, ST_BIN, F);
        BinArgs bf = ba;
        // test hook: a FILL capacity below what COUNT was checked against forces the list-overflow path (bin_overflow)
        if (mode == MODE_ASYNC && c->debug_fill_capacity) bf.list_capacity = std::min(bf.list_capacity, c->debug_fill_capacity);
        // the grid's last blocks place the tiles in the raster kernel's dispatch order (tile_place_block)
        bf.bin_blocks = bin_blocks;
        bf.order_tiles_y = c->band_tile_rows;
        bf.tile_bucket = ov.tile_bucket; bf.order_hist = ov.hist; bf.order_cursor = ov.cursor; bf.tile_order = ov.tile_order;
        hipLaunchKernelGGL(k_bin<true>, dim3(bin_blocks + order_blocks(c->tiles_x, c->band_tile_rows)), dim3(256), 0, F, bf);   // cursors were zeroed by k_scan_apply
        SWR_HIP(c, hipGetLastError());
    }
    {
        ScopedSpan sp(c, ST_SORT, F);
        hipLaunchKernelGGL(k_sort_tiles, dim3((n_tiles + SWR_SORT_TPB * SWR_SORT_TPW - 1u) / (SWR_SORT_TPB * SWR_SORT_TPW)), dim3(64 * SWR_SORT_TPB), 0, F, S.d_tile_start.as<uint32_t>(),
                           S.d_tile_count.as<uint32_t>(), c->d_tile_list.as<uint32_t>(), n_tiles, c->d_pair_tile.as<uint32_t>(), ctrl, b.seq,
                           (const uint4*)ov.tile_order);
        SWR_HIP(c, hipGetLastError());
    }
    if (cover_items) {
        ScopedSpan sp(c, ST_COVER, F);
        CoverArgs ca;
        ca.recs = S.d_recs.as<TriRec>();
        ca.odd_base = P.odd_base;
        ca.tile_list = c->d_tile_list.as<uint32_t>();
        ca.pair_tile = c->d_pair_tile.as<uint32_t>();
        ca.masks = S.d_masks.as<uint4>();
        ca.info = S.d_pcounts.as<uint2>();
        ca.refs = S.d_pair_refs.as<uint4>();
        ca.n_pairs = d_total;
        ca.ctrl = ctrl; ca.seq = b.seq;
        ca.fp = frame_params(c, b.near_clip);
        ca.dbg = d_total + 8;
        // (a multiple of 8 blocks: the kernel hands XCD x the x-th contiguous eighth of the blocks that hold pairs)
        const dim3 cg((unsigned)((((cover_items + (uint32_t)SWR_COVER_BLOCK - 1u) / (uint32_t)SWR_COVER_BLOCK) + 7u) & ~7u)), cb(SWR_COVER_BLOCK);
        with_flag(b.wireframe, [&](auto wire) { hipLaunchKernelGGL(k_cover<decltype(wire)::value>, cg, cb, 0, F, ca); });
        SWR_HIP(c, hipGetLastError());
    }
    if (F != c->stream) {
        // hand-over: the raster kernel (context's stream) starts when this batch's front end is complete
        SWR_HIP(c, hipEventRecord(S.front_done, F));
        SWR_HIP(c, hipStreamWaitEvent(c->stream, S.front_done, 0));
    } else if (c->pipelining && mode == MODE_ASYNC) {
        // a batch that is NOT pipelined (too big to gain, see execute_batch) while others are: the next pipelined front end shares
        // slot_tb / want / the lists with this one and may not start on the front stream before this point of the raster stream
        SWR_HIP(c, hipEventRecord(c->r_front_ev, c->stream));
        c->r_front_pending = true;
    }
    if ((rc = launch_raster(c, P, n_tiles))) return rc;
    if (c->pipelining && S.raster_done) {
        // ... and the front end that reuses this set (two flushes from now) starts when this raster kernel is complete
        SWR_HIP(c, hipEventRecord(S.raster_done, c->stream));
        S.raster_pending = true;
    }
    return SWR_OK;
}

// The raster kernel of one round, on the context's stream: one wave per tile over what the round's front end left in the set.
int launch_raster(swr_context* c, Pass& P, uint32_t n_tiles) {
    const Batch& b = P.b; RasterSet& S = P.S;
    const OrderView ov = order_view(S, n_tiles);
    ScopedSpan sp(c, ST_RASTER);
    RasterArgs ra;
    ra.fp = frame_params(c, b.near_clip);
    ra.recs = S.d_recs.as<TriRec>();
    ra.vout = S.d_vout.as<VOut>();
    ra.vout_bytes = (uint32_t)std::min<size_t>(S.d_vout.cap, 0xfffffff0u);
    ra.vnorm = b_needs_vnorm(b) ? S.d_vnorm.as<float4>() : nullptr;
    ra.user_consts = b_has_user_program(b) ? at<const float>(S.d_upload.p, P.up.off_consts) : nullptr;
    ra.draws = at<const DrawParams>(S.d_upload.p, 0);
    ra.tile_start = S.d_tile_start.as<uint32_t>();
    ra.tile_count = S.d_tile_count.as<uint32_t>();
    ra.pair_refs = S.d_pair_refs.as<uint4>();
    ra.color = b.color; ra.depth = b.depth;
    ra.tile_stats = c->d_tile_stats.as<uint32_t>();
    memcpy(ra.clear_rgba, b.clear_rgba, 16);
    ra.clear_color_on = P.cc ? 1 : 0;
    ra.clear_depth_on = P.cd ? 1 : 0;
    ra.tile_order = ov.tile_order;
    ra.tile_work = ov.tile_work;
    ra.n_tiles = n_tiles;
    ra.dbg = c->d_total.as<unsigned long long>() + 8;     // zero unless a SWR_DEBUG_COUNTERS build bumps it
    ra.ctrl = c->d_ctrl.as<Ctrl>(); ra.seq = b.seq;
    RasterTraits traits;
    traits.wireframe = b.wireframe;
    for (auto& d : b.draws) traits.add(d.p.program, d.p.blend, d.p.depth_test);
    ra.depth_only_grows = traits.depth_only_grows ? 1 : 0;
    const RasterKernel kernel = select_raster_kernel(traits);
    // every instantiation the library carries, by RasterKernel (a user program brings its own pair: UserProg::fn)
    using RasterFn = void (*)(RasterArgs, const uint4*, const uint2*);
    static const RasterFn table[] = {
        k_raster_c<false, true, SWR_PROG_DEBUG_VARYINGS, -1, -1, true>,                                  // debug_varyings_none
        k_raster_c<false, true, SWR_PROG_DEBUG_VARYINGS>,                                                // debug_varyings
        k_raster_c<true, true>,                                                                          // wireframe
        k_raster_c<false, true, -1, -1, -1, true>,                                                       // generic_none
        k_raster_c<false, true, SWR_PROG_PHONG_4POINT, SWR_BLEND_ALPHA, SWR_DEPTH_LESSEQUAL>,            // phong_default
        k_raster_c<false, true>,                                                                         // generic_phong
        k_raster_c<false, false, SWR_PROG_DUST2_LAMBERT_FOG, SWR_BLEND_ALPHA, SWR_DEPTH_LESSEQUAL>,      // dust2_default
        k_raster_c<false, false, SWR_PROG_GOURAUD, SWR_BLEND_ALPHA, SWR_DEPTH_LESSEQUAL>,                // gouraud_default
        k_raster_c<false, false>,                                                                        // generic
    };
    static_assert(sizeof table / sizeof table[0] == (size_t)RasterKernel::user, "one kernel per built-in RasterKernel, in its order");
    const dim3 g((n_tiles + 511u) & ~511u), t(64);       // one wave per tile (grid in whole 8 x 64 XCD segments)
    const uint4* mk = (const uint4*)S.d_masks.as<uint4>();
    const uint2* pc = (const uint2*)S.d_pcounts.as<uint2>();
    if (kernel == RasterKernel::user || kernel == RasterKernel::user_none) {
        void* args[] = { &ra, &mk, &pc };
        hipFunction_t fn = b.draws[0].prog->fn[kernel == RasterKernel::user_none ? 1 : 0];
        SWR_HIP(c, hipModuleLaunchKernel(fn, g.x, 1, 1, t.x, 1, 1, 0, c->stream, args, nullptr));
    } else {
        hipLaunchKernelGGL(table[(int)kernel], g, t, 0, c->stream, ra, mk, pc);
    }
    SWR_HIP(c, hipGetLastError());
    P.cc = P.cd = false;
    return SWR_OK;
}

// the host's half of a batch's upload block: the draws as the kernels index them and the block maps of the two geometry kernels
struct BatchGeometry {
    std::vector<DrawParams> hp;
    std::vector<BlockMap> vblocks, tblocks;
    uint64_t V = 0, T = 0; bool any_cull = false;       // vertices, triangles of the whole batch; some draw is frustum-culled
};
static BatchGeometry batch_geometry(const Batch& b) {
    BatchGeometry g;
    const size_t nd = b.draws.size();
    g.hp.resize(nd);
    std::vector<uint32_t> frag_reps;
    for (size_t i = 0; i < nd; ++i) {
        DrawParams p = b.draws[i].p;
        p.vert_base = (uint32_t)g.V; p.tri_base = (uint32_t)g.T;
        for (uint32_t f = 0; f < p.n_verts; f += SWR_GEOM_BLOCK) g.vblocks.push_back({ (uint32_t)i, f });
        for (uint32_t f = 0; f < p.n_tris; f += SWR_GEOM_BLOCK) g.tblocks.push_back({ (uint32_t)i, f });
        g.V += p.n_verts; g.T += p.n_tris;
        g.any_cull = g.any_cull || b.draws[i].frustum_cull;
        // fragment-stage identity: draws that differ only in geometry / matrices / cull mode share one set of fragment constants.
        // A user draw's captured block is compared bit for bit: as float VALUES, constants (or the words of a slot's pointer) that
        // differ only as +0 / -0 do would be merged, and a NaN constant would never match itself
        p.frag_draw = (uint32_t)i;
        for (uint32_t j : frag_reps) {
            const DrawParams& q = g.hp[j];
            if (q.program == p.program && q.blend == p.blend && q.depth_test == p.depth_test && q.tex == p.tex && q.tex_w == p.tex_w &&
                q.tex_h == p.tex_h && memcmp(&q.u, &p.u, sizeof p.u) == 0 &&
                (p.program < SWR_PROG_USER_BASE || memcmp(b.draws[j].ublock.get(), b.draws[i].ublock.get(), sizeof(UserBlock)) == 0)) { p.frag_draw = j; break; }
        }
        // a representative must have its k_vertex block 0 run (it writes fog_r1 / fog_den): it has vertices and is not subject to the
        // device-side frustum test; the list is bounded so that a batch of thousands of distinct materials stays linear
        if (p.frag_draw == (uint32_t)i && p.n_verts > 0 && !b.draws[i].frustum_cull && frag_reps.size() < 64) frag_reps.push_back((uint32_t)i);
        g.hp[i] = p;
    }
    return g;
}

// [k_frustum_cull ->] k_vertex -> k_setup on the front end's stream.  A user program with a vertex half brings its own k_vertex_user
// (k_vertex's parameters plus the constants) and k_setup (whose clipper also lerps data4.w): same grids, same argument values.
int launch_geometry(swr_context* c, const Pass& P, const BatchGeometry& g, uint32_t n_tiles, int count_stats) {
    const Batch& b = P.b; RasterSet& S = P.S; const hipStream_t F = P.F;
    const UserProg* vprog = b_has_user_vertex(b) ? b.draws[0].prog.get() : nullptr;
    const auto launch = [&](hipFunction_t user_fn, const void* builtin, size_t blocks, void** args) {
        return user_fn ? hipModuleLaunchKernel(user_fn, (unsigned)blocks, 1, 1, SWR_GEOM_BLOCK, 1, 1, 0, F, args, nullptr)
                       : hipLaunchKernel(builtin, dim3((unsigned)blocks), dim3(SWR_GEOM_BLOCK), args, 0, F);
    };
    const uint32_t nd = (uint32_t)b.draws.size();
    const DrawParams* d_draws = at<const DrawParams>(S.d_upload.p, 0);
    const BlockMap* d_vblocks = at<const BlockMap>(S.d_upload.p, P.up.off_vb);
    const BlockMap* d_tblocks = at<const BlockMap>(S.d_upload.p, P.up.off_tb);
    const uint32_t* d_visible = nullptr;
    if (g.any_cull) {
        ScopedSpan sp(c, ST_VERTEX, F);
        uint32_t* vis = at<uint32_t>(S.d_upload.p, P.up.off_vis);
        hipLaunchKernelGGL(k_frustum_cull, dim3((nd + 63) / 64), dim3(64), 0, F, d_draws,
                           at<const float4* const>(S.d_upload.p, P.up.off_bp), nd, vis);
        SWR_HIP(c, hipGetLastError());
        d_visible = vis;
    }
    float4* a_vnorm = b_needs_vnorm(b) ? S.d_vnorm.as<float4>() : (float4*)nullptr;
    if (!g.vblocks.empty()) {
        ScopedSpan sp(c, ST_VERTEX, F);
        VOut* a_vout = S.d_vout.as<VOut>();
        float* a_fog = at<float>(S.d_upload.p, offsetof(DrawParams, fog_r1));
        uint32_t* a_zero = S.d_tile_count.as<uint32_t>();
        uint32_t a_n_zero = n_tiles;
        uint32_t* a_hist = order_view(S, n_tiles).hist;
        const float* a_consts = at<const float>(S.d_upload.p, P.up.off_consts);     // (k_vertex_user only)
        void* args[] = { &d_draws, &d_vblocks, &a_vout, &d_visible, &a_fog, &a_vnorm, &a_zero, &a_n_zero, &a_hist, &a_consts };
        SWR_HIP(c, launch(vprog ? vprog->vertex_fn : nullptr, (const void*)k_vertex, g.vblocks.size(), args));
    }
    {
        ScopedSpan sp(c, ST_SETUP, F);
        FrameParams fp = frame_params(c, b.near_clip);
        const VOut* a_vout = S.d_vout.as<VOut>();
        VOut* a_pool = S.d_vout.as<VOut>() + g.V;
        uint32_t a_pool_base = (uint32_t)g.V;
        TriRec* a_recs = S.d_recs.as<TriRec>();
        uint32_t a_odd_base = P.odd_base;
        unsigned long long* a_tb = c->d_slot_tb.as<unsigned long long>();
        uint8_t* a_want = c->d_want.as<uint8_t>();
        Counters* a_counters = c->d_counters.as<Counters>();
        const Ctrl* a_ctrl = c->d_ctrl.as<Ctrl>();
        uint32_t a_seq = b.seq;
        int a_count = count_stats, a_wire = b.wireframe ? 1 : 0;
        void* args[] = { &d_draws, &d_tblocks, &a_vout, &a_pool, &a_pool_base, &a_recs, &a_odd_base, &a_tb, &a_want, &fp, &a_counters, &a_ctrl, &a_seq,
                         &a_count, &a_wire, &d_visible, &a_vnorm };
        SWR_HIP(c, launch(vprog ? vprog->setup_fn : nullptr, (const void*)k_setup, g.tblocks.size(), args));
    }
    return SWR_OK;
}

// launches one batch (clears + draws) on the stream
int execute_batch(swr_context* c, const Batch& b, int mode, int count_stats) {
    bool cc = b.clear_color, cd = b.clear_depth;
    if (b.draws.empty()) return run_clear(c, b, cc, cd);
    int rc;
    // pipelined flushes alternate between the two RasterSets and run their front end on the front stream; a synchronous batch (the
    // first frame, a replay, SWR_SYNC_FLUSH) reads the pair total back half way and runs on the context's stream alone
    if ((rc = ensure_front_stream(c))) return rc;
    // (what that buys and what it costs a short burst of frames: DESIGN.md section 8, profiles/r04_frames_in_flight.md; mode 2 keeps
    // big frames on one stream for callers whose bursts are that short, frames of at most 2^15 tiles or batches of at most 2^17
    // triangles are pipelined regardless)
    const BatchGeometry g = batch_geometry(b);
    const uint64_t V = g.V, T = g.T;
    const uint32_t n_tiles = (uint32_t)c->tiles_x * (uint32_t)c->band_tile_rows;
    const bool piped = mode == MODE_ASYNC && (c->pipelining == 1 || (c->pipelining == 2 && (T <= c->pipeline_max_tris ||
                                                                                            n_tiles <= c->pipeline_max_tiles)));
    Pass P{ b, c->sets[c->pipelining ? (b.seq & 1u) : 0u], piped ? c->front_stream : c->stream, mode, cc, cd };
    RasterSet& S = P.S; const hipStream_t F = P.F;
    if (c->pipelining && mode != MODE_ASYNC) SWR_HIP(c, hipStreamSynchronize(c->front_stream));     // earlier front ends and mesh uploads
    if (c->pipelining && mode == MODE_ASYNC) {
        // stream-level ordering between the two places a front end can run (no host wait)
        if (!piped && c->f_tail_pending) {
            SWR_HIP(c, hipEventRecord(c->f_tail_ev, c->front_stream));
            SWR_HIP(c, hipStreamWaitEvent(c->stream, c->f_tail_ev, 0));
            c->f_tail_pending = false;
        }
        if (piped && c->r_front_pending) {
            SWR_HIP(c, hipStreamWaitEvent(c->front_stream, c->r_front_ev, 0));
            c->r_front_pending = false;
        }
        if (piped) c->f_tail_pending = true;
    }
    const uint64_t spt = b.wireframe ? 6 : 2;        // primitive slots per submitted triangle
    // (V + 4 T vertex records of 64 B: k_raster_c addresses them with 32-bit byte offsets)
    if (V + 4 * T >= (1ull << 26) || spt * T >= 0xffffffffull)
        return fail(c, SWR_ERR_UNSUPPORTED, "internal error: a batch beyond 2^26 vertex-stage records reached execute_batch (record_draw flushes before)");
    if (T == 0) return run_clear(c, b, cc, cd);
    // the per-tile scan (k_scan_sums / k_scan_apply) holds 4096 block sums of SWR_SCAN_BLOCK = 256 tiles each
    if (n_tiles > (1u << 20))
        return fail(c, SWR_ERR_UNSUPPORTED, "more than 2^20 tiles in one band (a target beyond 16384 x 16384): render it in tile-row bands (swr_set_band)");

    P.up = upload_layout(b.draws.size(), g.vblocks.size(), g.tblocks.size(), g.any_cull, b_has_user_program(b));
    if ((rc = ensure(c, S.d_upload, P.up.bytes))) return rc;
    if ((rc = ensure(c, S.d_vout, (size_t)(V + 4 * T) * sizeof(VOut)))) return rc;
    if (b_needs_vnorm(b) && (rc = ensure(c, S.d_vnorm, S.d_vout.cap / 4))) return rc;        // one float4 per VOut entry
    // filled batches keep their records densely (rec_index, swr_device.h): T even-slot records, then from a whole line on the T records of
    // the odd slots (second fan triangles of near-clipped quads: almost never touched); wireframe batches one record per slot
    P.odd_base = (b.wireframe || !SWR_DENSE_RECORDS) ? 0u : record_odd_base(T);
    if ((rc = ensure(c, S.d_recs, (size_t)(spt * T + 2) * sizeof(TriRec)))) return rc;
    if ((rc = ensure(c, c->d_slot_tb, (size_t)(spt * T) * 8))) return rc;
    if ((rc = ensure(c, c->d_want, (size_t)(spt * T) + 64))) return rc;
    if ((rc = ensure(c, S.d_tile_count, (size_t)n_tiles * 4))) return rc;
    if ((rc = ensure(c, S.d_tile_start, (size_t)n_tiles * 4))) return rc;
    if ((rc = ensure(c, S.d_order, order_bytes(n_tiles)))) return rc;
    if (c->tile_stats_tiles != n_tiles) {
        // another tile count (resize / band change): the fragment counters gathered so far move into the carry words of d_total
        // (swr_get_stats adds them), in stream order, so totals survive a change of geometry
        if (c->tile_stats_tiles) {
            hipLaunchKernelGGL(k_reduce_tile_stats, dim3(1), dim3(1024), 0, c->stream, c->d_tile_stats.as<uint32_t>(),
                               (uint32_t)c->tile_stats_tiles, c->d_total.as<unsigned long long>() + 4, 1);
            SWR_HIP(c, hipGetLastError());
        }
        if ((rc = ensure(c, c->d_tile_stats, (size_t)n_tiles * 12))) return rc;
        SWR_HIP(c, hipMemsetAsync(c->d_tile_stats.p, 0, (size_t)n_tiles * 12, c->stream));
        c->tile_stats_tiles = n_tiles;
    }
    // the set's buffers were last read by the raster kernel of two flushes ago
    if (piped && S.raster_pending) SWR_HIP(c, hipStreamWaitEvent(F, S.raster_done, 0));
    if (S.hist_tiles != n_tiles) {
        SWR_HIP(c, hipMemsetAsync(order_view(S, n_tiles).tile_work, 0, (size_t)n_tiles * 4, F));      // no fragment history for this tiling in this set
        S.hist_tiles = n_tiles;
    }
    const size_t nd = b.draws.size();
    char* stage = (char*)slot_acquire(c, P.up.bytes);
    if (!stage) return fail(c, SWR_ERR_OOM, "hipHostMalloc failed for the upload staging block");
    memcpy(stage, g.hp.data(), nd * sizeof(DrawParams));
    if (!g.vblocks.empty()) memcpy(stage + P.up.off_vb, g.vblocks.data(), g.vblocks.size() * sizeof(BlockMap));
    memcpy(stage + P.up.off_tb, g.tblocks.data(), g.tblocks.size() * sizeof(BlockMap));
    if (g.any_cull) {
        const float4** bp = at<const float4*>(stage, P.up.off_bp);
        for (size_t i = 0; i < nd; ++i) bp[i] = b.draws[i].frustum_cull ? b.draws[i].mesh->d_bounds : nullptr;
    }
    if (b_has_user_program(b)) {                  // each draw's captured block (k_raster_c reads that of the draw's frag_draw)
        UserBlock* ub = at<UserBlock>(stage, P.up.off_consts);
        for (size_t i = 0; i < nd; ++i) ub[i] = *b.draws[i].ublock;
    }
    SWR_HIP(c, hipMemcpyAsync(S.d_upload.p, stage, P.up.bytes, hipMemcpyHostToDevice, F));
    if ((rc = launch_geometry(c, P, g, n_tiles, count_stats))) return rc;
    const bool counts_clear = !g.vblocks.empty() && n_tiles != 0;      // k_vertex cleared the per-tile counters and the order histogram
    rc = bin_and_raster(c, P, 0, (uint32_t)(spt * T), counts_clear);
    slot_submit(c);
    if (rc) return rc;
    // a synchronous batch ran its front end on the context's stream: the next pipelined front end shares slot_tb / want / the lists
    // with it, so it may not start before this one is over (rare path: the first frame and replays)
    if (c->pipelining && mode != MODE_ASYNC) SWR_HIP(c, hipStreamSynchronize(c->stream));
    if (P.cc || P.cd) return run_clear(c, b, P.cc, P.cd);   // nothing was binned
    return SWR_OK;
}

// complete = the batch's kernels are known to have finished (the stream was drained, or an event behind them has been waited for)
void retire_batch(swr_context* c, Batch& b, bool complete = false) {
    for (auto& d : b.draws) {
        if (d.mesh && d.mesh->transient) { if (complete) pool_mesh(c, d.mesh); else c->garbage.push_back(d.mesh); }
        if (d.prog && !complete) c->prog_garbage.push_back(std::move(d.prog));      // (its module stays loaded until the streams are idle)
    }
    b.draws.clear();
}

// Counters::overflow (mirrored in the pinned word host_poison[1]): a list position beyond the capacity in a batch that
// could not poison itself (synchronous flush: the lists were sized from the COUNT pass, so COUNT and FILL disagreed).
// The dropped pair cannot be recovered there: report it instead of returning a silently wrong image.
int check_list_overflow(swr_context* c) {
    if (!c->host_poison || !((volatile uint32_t*)c->host_poison)[1]) return SWR_OK;
    c->host_poison[1] = 0;
    return fail(c, SWR_ERR_HIP, "internal error: a (triangle, tile) pair did not fit its tile list and was dropped (Counters::overflow)");
}

// a fresh control block on the device: no batch poisoned (a blocking copy: at creation, or with the streams idle)
int reset_ctrl(swr_context* c) {
    Ctrl fresh; fresh.poison = 0; fresh.first_bad = 0xffffffffu; fresh.need = 0; fresh.host_flag = c->host_poison;
    SWR_HIP(c, hipMemcpy(c->d_ctrl.p, &fresh, sizeof fresh, hipMemcpyHostToDevice));
    return SWR_OK;
}

// stream must be idle: looks at the control block, replays what did not fit, retires the in-flight batches
int validate_locked(swr_context* c) {
    if (c->inflight.empty()) return check_list_overflow(c);
    int rc = SWR_OK;
    if (*(volatile uint32_t*)c->host_poison) {          // set by k_scan_apply / bin_overflow together with Ctrl::poison (stream is idle here)
        Ctrl h;
        SWR_HIP(c, hipMemcpy(&h, c->d_ctrl.p, sizeof h, hipMemcpyDeviceToHost));
        *c->host_poison = 0;
        c->host_poison[1] = 0;                              // an overflow inside an optimistic batch is cured by the replay below
        if ((rc = reset_ctrl(c))) return rc;
        std::vector<Batch> todo;
        todo.swap(c->inflight);
        c->replays++;
        for (auto& b : todo) {
            if (!rc && b.seq >= h.first_bad) {
                rc = execute_batch(c, b, MODE_SYNC, b.seq != h.first_bad);   // the first bad batch already counted its triangles
                retire_batch(c, b);                                         // (replayed: its kernels are in flight again)
            } else {
                retire_batch(c, b, true);
            }
        }
        if (!rc) rc = drain_streams(c);
        if (!rc) rc = check_list_overflow(c);
        return rc;
    }
    for (auto& b : c->inflight) retire_batch(c, b, true);
    c->inflight.clear();
    return check_list_overflow(c);
}

int flush_locked(swr_context* c) {
    if (c->W <= 0 || c->H <= 0 || band_pixels(c) == 0) {          // Rasterizer.cs:176: silently skip
        for (auto& d : c->draws) if (d.mesh && d.mesh->transient) c->garbage.push_back(d.mesh);
        c->draws.clear(); c->pend_verts = c->pend_tris = 0;
        c->pend_clear_color = c->pend_clear_depth = false;
        return SWR_OK;
    }
    if (c->draws.empty() && !c->pend_clear_color && !c->pend_clear_depth) return SWR_OK;
    Batch b;
    b.draws.swap(c->draws);
    b.clear_color = c->pend_clear_color; b.clear_depth = c->pend_clear_depth;
    memcpy(b.clear_rgba, c->clear_rgba, 16);
    b.near_clip = c->near_clip;
    b.wireframe = c->debug_mode == SWR_DEBUG_WIREFRAME;
    if (b.wireframe && b_needs_vnorm(b)) {
        // DrawLine hands Interpolate the TRIANGLE's outputs[0..1] for all three edges (Rasterizer.cs:421-423); a line record keeps the
        // edge's end points, not those two vertices' screen positions, so the program's ScreenCoords term is not available there
        for (auto& d : b.draws) if (d.mesh && d.mesh->transient) c->garbage.push_back(d.mesh);
        c->pend_verts = c->pend_tris = 0;
        return fail(c, SWR_ERR_UNSUPPORTED, b_has_user_program(b) ? "user programs are not available in DebugMode.Wireframe"
                                                                   : "SWR_PROG_DEBUG_VARYINGS is not available in DebugMode.Wireframe");
    }
    b.seq = c->next_seq++;
    b.color = c->color; b.depth = c->depth;
    c->pend_clear_color = c->pend_clear_depth = false;
    c->pend_verts = c->pend_tris = 0;
    if (!b.draws.empty()) c->totals.flushes++;
    // optimistic once an earlier (synchronous) batch has sized the pair buffers
    const bool optimistic = !c->sync_flush && pair_capacity(c) > 0;
    int rc = execute_batch(c, b, optimistic ? MODE_ASYNC : MODE_SYNC, 1);
    if (optimistic && !rc) {
        c->inflight.push_back(std::move(b));
        if (c->inflight.size() >= 64) {                            // bound the replay log
            if ((rc = drain_streams(c))) return rc;
            rc = validate_locked(c);
        }
    } else {
        retire_batch(c, b);
    }
    return rc;
}

// the shape of most entry points that observe or change state the GPU uses: launch what is recorded, then wait for it (one host sync)
int flush_and_sync_locked(swr_context* c) {
    int rc = flush_locked(c);
    return rc ? rc : sync_locked(c);
}

int ensure_bounds(swr_context* c, swr_mesh* m) {
    if (m->bounds_ready) return SWR_OK;
    if (!m->d_bounds) SWR_HIP(c, hipMalloc((void**)&m->d_bounds, sizeof(float4)));
    // (on the stream the mesh was uploaded on and k_frustum_cull will read the result on)
    hipLaunchKernelGGL(k_bounding_sphere, dim3(1), dim3(1024), 0, use_front_stream(c), (const swr_vertex*)m->d_verts, (uint32_t)m->n_verts, m->d_bounds);
    SWR_HIP(c, hipGetLastError());
    m->bounds_ready = true;
    return SWR_OK;
}

// Multi-GPU bands: a mesh whose exact bounding box projects entirely above or below this context's band of tile
// rows produces no fragment here, so the draw is not recorded at all (every rank would otherwise run the vertex, setup
// and count stages for all triangles).  Conservative: the corners are projected in double arithmetic and must all be in
// front of the camera plane (w > 0: then every point of the box projects inside the hull of the projected corners); the
// margin covers what the DEVICE's float32 evaluation of a vertex can differ from that: the three chained row-vector
// products of k_vertex (Renderer.cs:832-834) round 4 products + 3 sums per component and stage, so
// |fl(clip_k) - clip_k| <= 16 * 2^-24 * (|p| |model| |view| |proj|)_k (the running-error bound with absolute values,
// maximal at a corner of the box), which moves the screen row by at most H/2 * (E_y + |ndc_y| E_w) / (w - E_w); plus
// two pixels for the viewport arithmetic and the floor / ceil of the pixel bbox.  With large cancelling translations
// that bound exceeds any fixed margin -- then the draw is simply kept.
static bool band_rejects(const swr_context* c, const swr_mesh* m, const float* model, const float* view, const float* proj) {
    if (!m->has_box || c->il_k > 0 || (c->band_ty0 <= 0 && c->band_ty1 >= c->tiles_y)) return false;    // stripes: every rank sees the whole frame
    double mv[16], M[16], amv[16], A[16];
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k) {
            double a = 0, b = 0;
            for (int j = 0; j < 4; ++j) { a += (double)model[r * 4 + j] * (double)view[j * 4 + k]; b += std::fabs((double)model[r * 4 + j]) * std::fabs((double)view[j * 4 + k]); }
            mv[r * 4 + k] = a; amv[r * 4 + k] = b;
        }
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k) {
            double a = 0, b = 0;
            for (int j = 0; j < 4; ++j) { a += mv[r * 4 + j] * (double)proj[j * 4 + k]; b += amv[r * 4 + j] * std::fabs((double)proj[j * 4 + k]); }
            M[r * 4 + k] = a; A[r * 4 + k] = b;
        }
    const double u16 = 16.0 / 16777216.0;
    double smin = 1e300, smax = -1e300, ey = 0, ew = 0, wmin = 1e300, ndc_abs = 0;
    for (int corner = 0; corner < 8; ++corner) {
        const double x = (corner & 1) ? m->box_hi[0] : m->box_lo[0];
        const double y = (corner & 2) ? m->box_hi[1] : m->box_lo[1];
        const double z = (corner & 4) ? m->box_hi[2] : m->box_lo[2];
        const double cy = x * M[1] + y * M[5] + z * M[9] + M[13];
        const double cw = x * M[3] + y * M[7] + z * M[11] + M[15];
        const double sy_abs = std::fabs(x) * A[1] + std::fabs(y) * A[5] + std::fabs(z) * A[9] + A[13];
        const double sw_abs = std::fabs(x) * A[3] + std::fabs(y) * A[7] + std::fabs(z) * A[11] + A[15];
        if (!std::isfinite(cy) || !std::isfinite(cw) || !std::isfinite(sy_abs) || !std::isfinite(sw_abs)) return false;
        ey = std::max(ey, u16 * sy_abs); ew = std::max(ew, u16 * sw_abs);
        if (!(cw > 0)) return false;                                                             // not in front: keep
        wmin = std::min(wmin, cw);
        const double ndc = cy / cw;
        ndc_abs = std::max(ndc_abs, std::fabs(ndc));
        const double sy = (1.0 - (ndc * 0.5 + 0.5)) * (double)c->H;                              // Rasterizer.cs:385-386
        if (!std::isfinite(sy)) return false;
        smin = std::min(smin, sy); smax = std::max(smax, sy);
    }
    if (!(wmin - ew > 1e-6 * wmin)) return false;                       // the float32 w of some vertex may not be safely positive: keep
    const double margin = 2.0 + 0.5 * (double)c->H * (ey + ndc_abs * ew) / (wmin - ew);
    if (!std::isfinite(margin)) return false;
    const double y0 = (double)band_y0(c), y1 = (double)std::min(c->H, c->band_ty1 * SWR_TILE);   // band = pixel rows [y0, y1)
    return smax + margin < y0 || smin - margin > y1;
}

int record_draw(swr_context* c, swr_mesh* mesh, const float* model, const float* view, const float* proj,
                int program, const swr_uniforms* u, const swr_texture* tex, int cull, int depth_test, int blend, bool frustum_cull = false) {
    if (!mesh || !model || !view || !proj) return fail(c, SWR_ERR_INVALID_ARG, "null argument to render_mesh");
    std::shared_ptr<UserProg> uprog;
    if (program >= SWR_PROG_USER_BASE) {
        auto it = c->progs.find(program);
        if (it == c->progs.end()) return fail(c, SWR_ERR_INVALID_ARG, "unknown or destroyed user program id");
        if (c->debug_mode == SWR_DEBUG_WIREFRAME)
            return fail(c, SWR_ERR_UNSUPPORTED, "user programs are not available in DebugMode.Wireframe");
        uprog = it->second;
    } else if (program < SWR_PROG_FLAT_COLOR || program > SWR_PROG_DEBUG_VARYINGS) {
        return fail(c, SWR_ERR_INVALID_ARG, "unknown program id");
    }
    if ((program == SWR_PROG_DUST2_LAMBERT_FOG || program == SWR_PROG_PHONG_4POINT) && !u)
        return fail(c, SWR_ERR_INVALID_ARG, "this program needs a uniform block");
    if (cull < 0 || cull > 2 || depth_test < 0 || depth_test > 7 || blend < 0 || blend > 3)
        return fail(c, SWR_ERR_INVALID_ARG, "enum value out of range");
    if (c->W <= 0 || c->H <= 0) return SWR_OK;                      // Rasterizer.cs:176
    const int n_tris = mesh->n_idx / 3;                             // Rasterizer.cs:180
    if (n_tris == 0) return SWR_OK;
    // (nothing of it can land in this band -- unless a vertex program moves the vertices: the box says nothing then, the draw is kept)
    if (!(uprog && uprog->vertex_fn) && band_rejects(c, mesh, model, view, proj)) return SWR_OK;
    // one batch holds fewer than 2^26 vertex-stage records (one per vertex + four per triangle for the clipper: k_raster_c addresses
    // them with 32-bit byte offsets); a batch of several draws is flushed in time below, a SINGLE draw beyond it cannot be helped
    if ((uint64_t)mesh->n_verts + 4 * (uint64_t)n_tris >= (1ull << 26))
        return fail(c, SWR_ERR_UNSUPPORTED, "mesh exceeds 2^26 vertex-stage records (vertices + 4 x triangles: about 16.7 M triangles): split it");
    // keep a batch within the 32-bit slot / vertex numbering
    // (and the vertex-stage output -- one record per vertex plus four per triangle for the clipper -- below 4 GiB)
    if (c->pend_verts + (uint64_t)mesh->n_verts + 4 * (c->pend_tris + (uint64_t)n_tris) >= (1ull << 26)) {
        int rc = flush_locked(c); if (rc) return rc;
    }
    // SWR_PROG_DEBUG_VARYINGS and each user program have kernels of their own: a batch holds either only such draws or none
    // (submission order is kept)
    if (!c->draws.empty() && kernel_class(c->draws.back().p.program) != kernel_class(program)) {
        int rc = flush_locked(c); if (rc) return rc;
    }
    DrawCmd d;
    memset(&d.p, 0, sizeof d.p);
    memcpy(d.p.model, model, 64); memcpy(d.p.view, view, 64); memcpy(d.p.proj, proj, 64);
    if (u) d.p.u = *u;
    d.p.verts = mesh->d_verts; d.p.idx = mesh->d_idx;
    d.p.tex = tex ? tex->d_rgba : nullptr;
    d.p.tex_w = tex ? tex->w : 0; d.p.tex_h = tex ? (tex->bilinear ? -tex->h : tex->h) : 0;
    if (tex && tex->bilinear && tex->d_blocked) { d.p.tex = tex->d_blocked; d.p.tex_w = -tex->w; }      // (texture_fetch in swr_device.h)
    d.p.tex_wf = tex ? (float)tex->w : 0.0f; d.p.tex_hf = tex ? (float)tex->h : 0.0f;
    d.p.program = program; d.p.cull = cull; d.p.depth_test = depth_test; d.p.blend = blend;
    d.p.n_verts = (uint32_t)mesh->n_verts; d.p.n_tris = (uint32_t)n_tris;
    d.p.nm_flags = c->nm_flags;
    d.mesh = mesh;
    d.frustum_cull = frustum_cull;
    if (uprog) {       // the constants and the slots' textures as they are NOW (a C# closure's captured fields): later set_constants,
                       // set_texture and set_filter calls leave this draw alone
        auto ub = std::make_shared<UserBlock>();
        memcpy(ub->constants, uprog->constants, sizeof ub->constants);
        for (int s = 0; s < SWR_PROGRAM_TEXTURES - 1; ++s) ub->tex[s] = texture_slot_of(uprog->tex[s]);
        d.ublock = std::move(ub);
        d.prog = std::move(uprog);
    }
    if (frustum_cull) { int rc = ensure_bounds(c, mesh); if (rc) return rc; }
    c->draws.push_back(d);
    c->pend_verts += mesh->n_verts; c->pend_tris += n_tris;
    return SWR_OK;
}

int make_mesh(swr_context* c, const swr_vertex* v, int nv, const uint16_t* idx, int ni, bool transient, swr_mesh** out) {
    if (nv < 0 || ni < 0 || (nv > 0 && !v) || (ni > 0 && !idx) || !out) return fail(c, SWR_ERR_INVALID_ARG, "bad mesh arguments");
    const int used = (ni / 3) * 3;
    for (int i = 0; i < used; ++i)
        if ((int)idx[i] >= nv) return fail(c, SWR_ERR_INVALID_ARG, "index out of range (C#: IndexOutOfRangeException)");
    swr_mesh* m = nullptr;
    if (transient) {                               // smallest pooled mesh whose buffers hold these arrays
        size_t best = (size_t)-1;
        for (size_t i = 0; i < c->mesh_pool.size(); ++i) {
            swr_mesh* q = c->mesh_pool[i];
            if (q->cap_verts >= (size_t)nv * sizeof(swr_vertex) && q->cap_idx >= (size_t)ni * 2 + 8 &&
                (best == (size_t)-1 || q->cap_verts + q->cap_idx < c->mesh_pool[best]->cap_verts + c->mesh_pool[best]->cap_idx)) best = i;
        }
        if (best != (size_t)-1) {
            m = c->mesh_pool[best];
            c->mesh_pool.erase(c->mesh_pool.begin() + (std::ptrdiff_t)best);
            c->mesh_pool_bytes -= m->cap_verts + m->cap_idx;
            m->bounds_ready = false; m->has_box = false;
        }
    }
    if (!m) m = new swr_mesh();
    m->n_verts = nv; m->n_idx = ni; m->transient = transient; m->owner = c;
    if (nv > 0) {                                  // exact AABB (min / max only): input to band_rejects
        bool ok = true;
        for (int k = 0; k < 3; ++k) { m->box_lo[k] = v[0].position[k]; m->box_hi[k] = v[0].position[k]; }
        for (int i = 0; i < nv; ++i)
            for (int k = 0; k < 3; ++k) {
                const float p = v[i].position[k];
                if (!(p == p)) ok = false;
                m->box_lo[k] = std::min(m->box_lo[k], p); m->box_hi[k] = std::max(m->box_hi[k], p);
            }
        m->has_box = ok;
    }
    hipError_t e = hipSuccess;
    if (nv && m->cap_verts < (size_t)nv * sizeof(swr_vertex)) {
        e = hipMalloc((void**)&m->d_verts, (size_t)nv * sizeof(swr_vertex));
        if (e == hipSuccess) m->cap_verts = (size_t)nv * sizeof(swr_vertex);
    }
    if (e == hipSuccess && ni && m->cap_idx < (size_t)ni * 2 + 8) {
        e = hipMalloc((void**)&m->d_idx, (size_t)ni * 2 + 8);
        if (e == hipSuccess) m->cap_idx = (size_t)ni * 2 + 8;
    }
    // (only front-end kernels read a mesh: the upload goes to their stream, so a pipelined frame does not wait for the raster stream)
    if (e == hipSuccess && nv) e = hipMemcpyAsync(m->d_verts, v, (size_t)nv * sizeof(swr_vertex), hipMemcpyHostToDevice, use_front_stream(c));
    if (e == hipSuccess && ni) e = hipMemcpyAsync(m->d_idx, idx, (size_t)ni * 2, hipMemcpyHostToDevice, use_front_stream(c));
    // (a retained mesh may be read from the ray stream: an event behind its upload orders that reader without a wait on this stream)
    if (e == hipSuccess && !transient) e = hipEventCreateWithFlags(&m->uploaded, hipEventDisableTiming);
    if (e == hipSuccess && !transient) e = hipEventRecord(m->uploaded, use_front_stream(c));
    if (e != hipSuccess) {
        destroy_mesh(m);
        return fail_hip(c, "mesh upload failed: ", e);
    }
    *out = m;
    return SWR_OK;
}

// Were the pixels of present slot `slot` rendered by a batch that has to be replayed?  Only if a batch flushed at or before that
// present poisoned itself: Ctrl::first_bad (one small blocking copy, and only when the pinned poison word is up at all).
int present_is_stale(swr_context* c, int slot, bool& stale) {
    stale = false;
    if (!*(volatile uint32_t*)c->host_poison) return SWR_OK;
    Ctrl h;
    SWR_HIP(c, hipMemcpy(&h, c->d_ctrl.p, sizeof h, hipMemcpyDeviceToHost));
    stale = h.first_bad <= c->present_seq[slot];
    return SWR_OK;
}
}  // namespace
