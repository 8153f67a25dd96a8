// swr_deform.h -- host side of deforming meshes (swr_mesh_create_like / _readback / _blend / _set_skin / _skin / _skin_batch, DESIGN.md
// section 28) and of skeletal animation (swr_skeleton_*, swr_pose_set_*): the bracket around a kernel that writes
// retained meshes, the staged uploads of palettes, requests and job tables, and the skeleton's blobs as swr_animation_layout.h lays
// them out.  Included by swr_api.hip only, after swr_flush.h and swr_query.h.  The entry points in swr_api.hip are a call each.
#pragma once
#include "swr_animation_layout.h"

namespace {
// a retained mesh of this context, or the message why not
int deform_mesh_check(swr_context* c, const swr_mesh* m, const char* null_msg) {
    if (!m) return fail(c, SWR_ERR_INVALID_ARG, null_msg);
    if (m->transient) return fail(c, SWR_ERR_INVALID_ARG, "a transient mesh (swr_render_mesh_arrays) cannot be deformed, copied or read back");
    if (m->owner != c) return fail(c, SWR_ERR_INVALID_ARG, "the mesh belongs to another context");
    return SWR_OK;
}

// does a draw of the list read one of the n destinations `dsts` (sorted by address)?
bool batch_reads(const std::vector<DrawCmd>& draws, const swr_mesh* const* dsts, size_t n) {
    for (const DrawCmd& d : draws) if (std::binary_search(dsts, dsts + n, (const swr_mesh*)d.mesh)) return true;
    return false;
}

// Everything that must happen before a kernel may WRITE the vertices of the destinations (n of them, sorted by address: one mesh for
// swr_mesh_blend and swr_mesh_skin, a batch's for swr_mesh_skin_batch); returns the stream it runs on.
//   A. immediate-mode semantics: draws recorded so far that reference a destination are launched first (they see the old vertices) --
//      and only then: a loop that deforms sixteen players and draws them stays one batch;
//   B. an optimistic batch in flight that references a destination may be replayed later (validate_locked), and a replay runs the front end
//      again: it must read the vertices the batch saw, so the streams are drained and the batches validated before the first write
//      (transient meshes solve the same problem through c->garbage: their buffers are not reused before the streams were idle).
//      A loop that presents every frame has retired those batches in swr_present_wait: nothing to wait for there.
// The deform runs where make_mesh uploads (use_front_stream): only front-end kernels read a mesh, and every front end issued later
// is behind it -- on the front stream by stream order, on the context's stream through f_tail_pending (execute_batch).
int deform_begin(swr_context* c, const swr_mesh* const* dsts, size_t n, hipStream_t* stream) {
    int rc;
    if (batch_reads(c->draws, dsts, n) && (rc = flush_locked(c))) return rc;
    bool in_flight = false;
    for (const Batch& b : c->inflight) in_flight = in_flight || batch_reads(b.draws, dsts, n);
    if (in_flight && (rc = sync_locked(c))) return rc;
    if ((rc = ensure_front_stream(c))) return rc;
    *stream = use_front_stream(c);
    return SWR_OK;
}

// ... and after it, for the destinations that have vertices (in any order): what the host knows about their old vertices is void.
//   C. readers on the ray stream (swr_raycast, swr_character_update, swr_mesh_readback) are ordered behind swr_mesh::uploaded: it is
//      recorded again behind the deform -- or, for a batch, ONE event of c->pose_events that its destinations share stands in for it
//      (swr_mesh::posed; an event record per mesh was most of a small batch's stream time).  The query entry points return only after
//      their kernels finished (they wait for their own result under the context mutex), so no ray-stream reader of a destination is in
//      flight when a deform is issued;
//   D. the bounding sphere is computed again on first use (swr_mesh_bounds, swr_render_mesh_culled follow the pose);
//   E. the host-side box is gone: band_rejects keeps the draw on every rank (conservative and correct).
int deform_end(swr_context* c, swr_mesh* const* dst, int n, hipStream_t stream, bool batch) {
    std::shared_ptr<SharedEvent> ev;
    if (batch) {
        for (auto& e : c->pose_events) if (e.use_count() == 1) { ev = e; break; }          // no mesh holds it: its waits were issued long ago
        if (!ev) {
            ev = std::make_shared<SharedEvent>();
            SWR_HIP(c, hipEventCreateWithFlags(&ev->ev, hipEventDisableTiming));
            c->pose_events.push_back(ev);
        }
    }
    SWR_HIP(c, hipEventRecord(batch ? ev->ev : dst[0]->uploaded, stream));
    for (int k = 0; k < n; ++k) {
        if (dst[k]->n_verts == 0) continue;
        dst[k]->posed = ev;
        dst[k]->upload_seen = false;
        dst[k]->bounds_ready = false;
        dst[k]->has_box = false;
    }
    return SWR_OK;
}

// A staged upload (F): bytes on their way to the device without a wait -- a palette, a request list, a job table.  palette_slot hands
// out the first slot whose last reader is over, else a new one; the caller fills host.p, copies it up and launches the reader on one
// stream, and ends with palette_submit on that stream.
int palette_slot(swr_context* c, size_t bytes, PaletteSlot** out, bool device_copy = true) {
    PaletteSlot* s = nullptr;
    const size_t n = c->palettes.size();
    for (size_t k = 0; k < n && !s; ++k) {
        PaletteSlot& q = c->palettes[(c->palette_next + k) % n];
        if (q.busy && hipEventQuery(q.done) == hipSuccess) q.busy = false;
        if (!q.busy) { s = &q; c->palette_next = (c->palette_next + k + 1) % n; }
    }
    if (!s && n < SWR_PALETTE_SLOTS_MAX) {
        c->palettes.emplace_back();
        s = &c->palettes.back();
        SWR_HIP(c, hipEventCreateWithFlags(&s->done, hipEventDisableTiming));
    }
    if (!s) {       // back-pressure: SWR_PALETTE_SLOTS_MAX palettes queued and none read yet
        s = &c->palettes[c->palette_next % n];
        c->palette_next = (c->palette_next + 1) % n;
        SWR_HIP(c, hipEventSynchronize(s->done));
        s->busy = false;
    }
    // (a free slot's buffers are idle: growing them frees nothing a kernel reads)
    if (s->host.cap < bytes) SWR_HIP(c, ensure_pinned(s->host, std::max<size_t>(bytes, 4096)));
    // (device_copy = false: staging for a copy that goes elsewhere, swr_pose_set_upload)
    if (device_copy) { int rc = ensure(c, s->dev, std::max<size_t>(bytes, 4096)); if (rc) return rc; }
    *out = s;
    return SWR_OK;
}
// ... behind the last launch that reads the slot: the slot is taken until this point of stream s has passed.  The one place a slot
// becomes busy -- a slot that was handed out and not submitted would be reused under a running kernel.
int palette_submit(swr_context* c, PaletteSlot* slot, hipStream_t s) {
    SWR_HIP(c, hipEventRecord(slot->done, s));
    slot->busy = true;
    return SWR_OK;
}

int mesh_create_like(swr_context* c, const swr_mesh* src, swr_mesh** out) {
    if (!out) return fail(c, SWR_ERR_INVALID_ARG, "out is null");
    int rc = deform_mesh_check(c, src, "the source mesh is null"); if (rc) return rc;
    if ((rc = ensure_front_stream(c))) return rc;
    swr_mesh* m = new swr_mesh();
    m->n_verts = src->n_verts; m->n_idx = src->n_idx; m->owner = c;
    memcpy(m->box_lo, src->box_lo, sizeof m->box_lo); memcpy(m->box_hi, src->box_hi, sizeof m->box_hi);
    m->has_box = src->has_box;
    const size_t vbytes = (size_t)src->n_verts * sizeof(swr_vertex), ibytes = (size_t)src->n_idx * 2;
    // behind src's upload or its last deform, on their stream: the arrays do not cross PCIe again
    const hipStream_t s = use_front_stream(c);
    hipError_t e = hipSuccess;
    if (vbytes) { e = hipMalloc((void**)&m->d_verts, vbytes); if (e == hipSuccess) m->cap_verts = vbytes; }
    if (e == hipSuccess && ibytes) { e = hipMalloc((void**)&m->d_idx, ibytes + 8); if (e == hipSuccess) m->cap_idx = ibytes + 8; }
    if (e == hipSuccess && vbytes) e = hipMemcpyAsync(m->d_verts, src->d_verts, vbytes, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && ibytes) e = hipMemcpyAsync(m->d_idx, src->d_idx, ibytes, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&m->uploaded, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(m->uploaded, s);
    if (e != hipSuccess) {
        destroy_mesh(m);
        return fail_hip(c, "mesh copy failed: ", e);
    }
    *out = m;
    return SWR_OK;
}

int mesh_readback(swr_context* c, const swr_mesh* mesh, swr_vertex* out) {
    int rc = deform_mesh_check(c, mesh, "the mesh is null"); if (rc) return rc;
    if (!out) return fail(c, SWR_ERR_INVALID_ARG, "the destination is null");
    if (mesh->n_verts == 0) return SWR_OK;
    // a reader on the ray stream: behind the upload or the last deform (swr_mesh::uploaded) and behind nothing else -- recorded draws
    // are not flushed, a frame in flight is not waited for
    if ((rc = ensure_ray_stream(c))) return rc;
    swr_mesh* m = const_cast<swr_mesh*>(mesh);
    if (!m->upload_seen) { SWR_HIP(c, hipStreamWaitEvent(c->ray_stream, m->posed ? m->posed->ev : m->uploaded, 0)); m->upload_seen = true; }
    SWR_HIP(c, hipMemcpyAsync(out, m->d_verts, (size_t)m->n_verts * sizeof(swr_vertex), hipMemcpyDeviceToHost, c->ray_stream));
    SWR_HIP(c, hipStreamSynchronize(c->ray_stream));
    return SWR_OK;
}

int mesh_blend(swr_context* c, swr_mesh* dst, const swr_mesh* a, const swr_mesh* b, float t) {
    int rc;
    if ((rc = deform_mesh_check(c, dst, "the destination mesh is null"))) return rc;
    if ((rc = deform_mesh_check(c, a, "key frame a is null"))) return rc;
    if ((rc = deform_mesh_check(c, b, "key frame b is null"))) return rc;
    if (dst == a || dst == b) return fail(c, SWR_ERR_INVALID_ARG, "the destination mesh is one of the key frames (make a target with swr_mesh_create_like)");
    if (a->n_verts != dst->n_verts || b->n_verts != dst->n_verts) return fail(c, SWR_ERR_INVALID_ARG, "the key frames and the destination must have equal vertex counts");
    if (dst->n_verts == 0) return SWR_OK;
    hipStream_t s = nullptr;
    if ((rc = deform_begin(c, &dst, 1, &s))) return rc;
    const uint32_t n_words = 3u * (uint32_t)dst->n_verts;
    hipLaunchKernelGGL(k_mesh_blend, dim3((n_words + SWR_DEFORM_BLOCK - 1u) / SWR_DEFORM_BLOCK), dim3(SWR_DEFORM_BLOCK), 0, s,
                       reinterpret_cast<const float4*>(a->d_verts), reinterpret_cast<const float4*>(b->d_verts),
                       reinterpret_cast<float4*>(dst->d_verts), n_words, t);
    SWR_HIP(c, hipGetLastError());
    return deform_end(c, &dst, 1, s, false);
}

int mesh_set_skin(swr_context* c, swr_mesh* m, const uint16_t* joints4, const float* weights4) {
    int rc = deform_mesh_check(c, m, "the mesh is null"); if (rc) return rc;
    if ((joints4 == nullptr) != (weights4 == nullptr)) return fail(c, SWR_ERR_INVALID_ARG, "pass both joints4 and weights4, or NULL for both (which removes the attributes)");
    if (!joints4) {
        // (hipFree waits for the device: a queued k_mesh_skin has read them by then)
        if (m->d_joints) SWR_HIP(c, hipFree(m->d_joints));
        m->d_joints = nullptr;
        if (m->d_weights) SWR_HIP(c, hipFree(m->d_weights));
        m->d_weights = nullptr;
        m->max_joint = -1; m->has_skin = false;
        return SWR_OK;
    }
    const size_t nv = (size_t)m->n_verts;
    int max_joint = -1;
    for (size_t i = 0; i < 4 * nv; ++i) max_joint = std::max(max_joint, (int)joints4[i]);
    if ((rc = ensure_front_stream(c))) return rc;
    if (nv) {
        // a second call replaces the attributes in place, on the stream the skinning kernels run on (behind those queued so far)
        if (!m->d_joints) SWR_HIP(c, hipMalloc((void**)&m->d_joints, nv * sizeof(ushort4)));
        if (!m->d_weights) SWR_HIP(c, hipMalloc((void**)&m->d_weights, nv * sizeof(float4)));
        const hipStream_t s = use_front_stream(c);
        SWR_HIP(c, hipMemcpyAsync(m->d_joints, joints4, nv * sizeof(ushort4), hipMemcpyHostToDevice, s));
        SWR_HIP(c, hipMemcpyAsync(m->d_weights, weights4, nv * sizeof(float4), hipMemcpyHostToDevice, s));
    }
    m->max_joint = max_joint; m->has_skin = true;
    return SWR_OK;
}

int mesh_skin(swr_context* c, swr_mesh* dst, const swr_mesh* src, const float* palette, int n_joints) {
    int rc;
    if ((rc = deform_mesh_check(c, dst, "the destination mesh is null"))) return rc;
    if ((rc = deform_mesh_check(c, src, "the source mesh is null"))) return rc;
    if (!palette) return fail(c, SWR_ERR_INVALID_ARG, "the palette is null");
    if (dst == src) return fail(c, SWR_ERR_INVALID_ARG, "the destination mesh is the source (make a target with swr_mesh_create_like)");
    if (src->n_verts != dst->n_verts) return fail(c, SWR_ERR_INVALID_ARG, "the source and the destination must have equal vertex counts");
    if (!src->has_skin) return fail(c, SWR_ERR_INVALID_ARG, "the source mesh has no skin attributes (swr_mesh_set_skin)");
    if (n_joints > 65535) return fail(c, SWR_ERR_UNSUPPORTED, "a palette holds at most 65535 joints (16-bit joint indices)");
    if (n_joints <= src->max_joint) return fail(c, SWR_ERR_INVALID_ARG, "n_joints must exceed the largest joint index the source's skin attributes use");
    if (dst->n_verts == 0) return SWR_OK;
    hipStream_t s = nullptr;
    if ((rc = deform_begin(c, &dst, 1, &s))) return rc;
    const size_t bytes = (size_t)n_joints * 64;
    PaletteSlot* slot = nullptr;
    if ((rc = palette_slot(c, bytes, &slot))) return rc;
    memcpy(slot->host.p, palette, bytes);
    SWR_HIP(c, hipMemcpyAsync(slot->dev.p, slot->host.p, bytes, hipMemcpyHostToDevice, s));
    const dim3 grid(((uint32_t)dst->n_verts + SWR_DEFORM_BLOCK - 1u) / SWR_DEFORM_BLOCK), block(SWR_DEFORM_BLOCK);
    hipLaunchKernelGGL(k_mesh_skin, grid, block, 0, s, (const swr_vertex*)src->d_verts, (const ushort4*)src->d_joints,
                       (const float4*)src->d_weights, (const float*)slot->dev.p, dst->d_verts, (uint32_t)dst->n_verts, c->nm_flags);
    SWR_HIP(c, hipGetLastError());
    if ((rc = palette_submit(c, slot, s))) return rc;
    return deform_end(c, &dst, 1, s, false);
}

// ---- skeletal animation: clips to palettes on the GPU, one skin launch for a crowd
int skeleton_check(swr_context* c, const swr_skeleton* k) {
    if (!k) return fail(c, SWR_ERR_INVALID_ARG, "the skeleton is null");
    if (k->owner != c) return fail(c, SWR_ERR_INVALID_ARG, "the skeleton belongs to another context");
    return SWR_OK;
}
int pose_set_check(swr_context* c, const swr_pose_set* p) {
    if (!p) return fail(c, SWR_ERR_INVALID_ARG, "the pose set is null");
    if (p->owner != c) return fail(c, SWR_ERR_INVALID_ARG, "the pose set belongs to another context");
    return SWR_OK;
}
// behind a write of the set on stream s: what swr_pose_set_readback orders itself by
int pose_set_written(swr_context* c, swr_pose_set* p, hipStream_t s) {
    SWR_HIP(c, hipEventRecord(p->written, s));
    p->written_seen = false;
    return SWR_OK;
}
void destroy_skeleton(swr_skeleton* k) {
    if (k->d_static) (void)hipFree(k->d_static);
    if (k->d_clips) (void)hipFree(k->d_clips);
    delete k;
}
void destroy_pose_set(swr_pose_set* p) {
    if (p->d_palettes) (void)hipFree(p->d_palettes);
    if (p->d_worlds) (void)hipFree(p->d_worlds);
    if (p->written) (void)hipEventDestroy(p->written);
    delete p;
}
// the arrays of k's blob as k_pose_sample reads them
SkeletonDev skeleton_dev(const swr_skeleton* k) {
    const SkeletonLayout l = skeleton_layout((size_t)k->n_nodes, (size_t)k->n_joints, (size_t)k->n_levels);
    const float* f = static_cast<const float*>(k->d_static);
    const int32_t* w = static_cast<const int32_t*>(k->d_static);
    SkeletonDev sk{};
    sk.rest_local = f + l.rest_local; sk.inverse_bind = f + l.inverse_bind; sk.rest_t = f + l.rest_t; sk.rest_r = f + l.rest_r; sk.rest_s = f + l.rest_s;
    sk.parent = w + l.parent; sk.order = w + l.order; sk.level_start = w + l.level_start; sk.joint_node = w + l.joint_node;
    sk.n_nodes = (uint32_t)k->n_nodes; sk.n_joints = (uint32_t)k->n_joints; sk.n_levels = (uint32_t)k->n_levels;
    return sk;
}

int skeleton_create(swr_context* c, int n_nodes, const int32_t* parent, const float* rest_local, const float* rest_t,
                        const float* rest_r, const float* rest_s, int n_joints, const int32_t* joint_node, const float* inverse_bind,
                        swr_skeleton** out) {
    if (!out || !parent || !rest_local || !rest_t || !rest_r || !rest_s) return fail(c, SWR_ERR_INVALID_ARG, "a skeleton array is null");
    if (n_nodes < 1 || n_joints < 0) return fail(c, SWR_ERR_INVALID_ARG, "a skeleton has at least one node and no negative joint count");
    if (n_joints > 0 && (!joint_node || !inverse_bind)) return fail(c, SWR_ERR_INVALID_ARG, "joint_node or inverse_bind is null");
    if (n_nodes > SWR_SKELETON_MAX_NODES || n_joints > 65535) return fail(c, SWR_ERR_UNSUPPORTED, "a skeleton holds at most 65535 nodes and 65535 joints");
    const size_t nn = (size_t)n_nodes, nj = (size_t)n_joints;
    std::vector<int32_t> depth(nn), order(nn);
    int n_levels = 0;
    for (size_t i = 0; i < nn; ++i) {
        if (parent[i] < -1 || parent[i] >= (int32_t)i) return fail(c, SWR_ERR_INVALID_ARG, "nodes must be in topological order: parent[i] < i, or -1 for a root");
        depth[i] = parent[i] < 0 ? 0 : depth[(size_t)parent[i]] + 1;
        n_levels = std::max(n_levels, depth[i] + 1);
    }
    for (size_t j = 0; j < nj; ++j)
        if (joint_node[j] < 0 || joint_node[j] >= n_nodes) return fail(c, SWR_ERR_INVALID_ARG, "a joint's node index is out of range");
    // the level table: nodes by depth, in index order within a level (a counting sort)
    std::vector<int32_t> level_start((size_t)n_levels + 1, 0);
    for (size_t i = 0; i < nn; ++i) ++level_start[(size_t)depth[i] + 1];
    for (int l = 0; l < n_levels; ++l) level_start[(size_t)l + 1] += level_start[(size_t)l];
    { std::vector<int32_t> at(level_start.begin(), level_start.end() - 1); for (size_t i = 0; i < nn; ++i) order[(size_t)at[(size_t)depth[i]]++] = (int32_t)i; }
    const SkeletonLayout l = skeleton_layout(nn, nj, (size_t)n_levels);
    const size_t words = l.words;
    std::vector<uint32_t> blob(words);
    memcpy(&blob[l.rest_local], rest_local, 64 * nn); memcpy(&blob[l.rest_t], rest_t, 12 * nn); memcpy(&blob[l.rest_r], rest_r, 16 * nn);
    memcpy(&blob[l.rest_s], rest_s, 12 * nn); memcpy(&blob[l.parent], parent, 4 * nn); memcpy(&blob[l.order], order.data(), 4 * nn);
    memcpy(&blob[l.level_start], level_start.data(), 4 * ((size_t)n_levels + 1));
    if (nj) { memcpy(&blob[l.inverse_bind], inverse_bind, 64 * nj); memcpy(&blob[l.joint_node], joint_node, 4 * nj); }
    swr_skeleton* k = new swr_skeleton();
    k->owner = c; k->n_nodes = n_nodes; k->n_joints = n_joints; k->n_levels = n_levels;
    k->clips.assign(1, 0u);
    hipError_t e = hipMalloc(&k->d_static, words * 4);
    if (e == hipSuccess) e = hipMemcpy(k->d_static, blob.data(), words * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        destroy_skeleton(k);
        return fail_hip(c, "skeleton upload failed: ", e);
    }
    *out = k;
    return SWR_OK;
}

int skeleton_destroy(swr_context* c, swr_skeleton* k) {
    if (!k) return SWR_OK;
    int rc = skeleton_check(c, k); if (rc) return rc;
    destroy_skeleton(k);                       // (hipFree waits for the device: a queued k_pose_sample has read it by then)
    return SWR_OK;
}

int skeleton_add_clip(swr_context* c, swr_skeleton* k, const swr_anim_channel* channels, int n_channels, int* clip_index) {
    int rc = skeleton_check(c, k); if (rc) return rc;
    if (!clip_index || n_channels < 0 || (n_channels > 0 && !channels)) return fail(c, SWR_ERR_INVALID_ARG, "channels or clip_index is null, or n_channels is negative");
    const size_t nn = (size_t)k->n_nodes;
    size_t words = k->clips.size() + clip_table_words(nn);
    std::vector<uint8_t> taken(3 * nn, 0);
    for (int i = 0; i < n_channels; ++i) {
        const swr_anim_channel& ch = channels[i];
        if (ch.interpolation == SWR_ANIM_CUBICSPLINE) return fail(c, SWR_ERR_UNSUPPORTED, "CUBICSPLINE interpolation is not supported (STEP and LINEAR are)");
        if (ch.interpolation != SWR_ANIM_STEP && ch.interpolation != SWR_ANIM_LINEAR) return fail(c, SWR_ERR_INVALID_ARG, "unknown interpolation");
        if (ch.node < 0 || ch.node >= k->n_nodes) return fail(c, SWR_ERR_INVALID_ARG, "a channel's node index is out of range");
        if (ch.path < SWR_ANIM_PATH_TRANSLATION || ch.path > SWR_ANIM_PATH_SCALE) return fail(c, SWR_ERR_INVALID_ARG, "a channel's path is none of translation, rotation, scale");
        if (ch.n_keys < 1) return fail(c, SWR_ERR_INVALID_ARG, "a channel needs at least one key");
        if (!ch.times || !ch.values) return fail(c, SWR_ERR_INVALID_ARG, "a channel's times or values are null");
        uint8_t& t = taken[3 * (size_t)ch.node + (size_t)ch.path];
        if (t) return fail(c, SWR_ERR_INVALID_ARG, "two channels target the same node and path");
        t = 1;
        for (int q = 0; q + 1 < ch.n_keys; ++q)
            if (!(ch.times[q + 1] >= ch.times[q])) return fail(c, SWR_ERR_INVALID_ARG, "key times must not decrease (or be NaN)");
        words += clip_channel_words(ch.path, (size_t)ch.n_keys);
    }
    if (words >= ((size_t)1 << 30)) return fail(c, SWR_ERR_UNSUPPORTED, "the skeleton's clips exceed 2^30 words");
    // the new blob on the host, then in a new allocation; the old one is freed once the device is idle (a queued k_pose_sample may
    // read it) -- a load-time call
    std::vector<uint32_t> blob = k->clips;
    const uint32_t base = (uint32_t)blob.size();
    blob.resize(words, 0u);
    size_t at = base + clip_table_words(nn);
    for (int i = 0; i < n_channels; ++i) {
        const swr_anim_channel& ch = channels[i];
        const size_t comps = clip_channel_comps(ch.path), nk = (size_t)ch.n_keys;
        blob[base + 3 * (size_t)ch.node + (size_t)ch.path] = (uint32_t)at;
        blob[at] = (uint32_t)ch.interpolation; blob[at + 1] = (uint32_t)ch.n_keys;
        memcpy(&blob[at + 2], ch.times, 4 * nk);
        memcpy(&blob[at + 2 + nk], ch.values, 4 * nk * comps);
        at += clip_channel_words(ch.path, nk);
    }
    uint32_t* d_new = nullptr;
    SWR_HIP(c, hipMalloc((void**)&d_new, words * 4));
    hipError_t e = hipMemcpy(d_new, blob.data(), words * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && k->d_clips) { e = hipDeviceSynchronize(); ++c->host_syncs; }
    if (e != hipSuccess) { (void)hipFree(d_new); SWR_HIP(c, e); }
    if (k->d_clips) (void)hipFree(k->d_clips);
    k->d_clips = d_new;
    k->clips.swap(blob);
    *clip_index = (int)k->clip_base.size();
    k->clip_base.push_back(base);
    return SWR_OK;
}

int pose_set_create(swr_context* c, int n_instances, int n_joints, swr_pose_set** out) {
    if (!out) return fail(c, SWR_ERR_INVALID_ARG, "out is null");
    if (n_instances < 1 || n_joints < 1) return fail(c, SWR_ERR_INVALID_ARG, "a pose set has at least one instance and one joint");
    if (n_joints > 65535 || (size_t)n_instances * (size_t)n_joints > ((size_t)1 << 24))
        return fail(c, SWR_ERR_UNSUPPORTED, "a pose set holds at most 65535 joints per instance and 2^24 matrices");
    swr_pose_set* p = new swr_pose_set();
    p->owner = c; p->n_instances = n_instances; p->n_joints = n_joints;
    const size_t bytes = (size_t)n_instances * (size_t)n_joints * 64;
    hipError_t e = hipMalloc((void**)&p->d_palettes, bytes);
    if (e == hipSuccess) e = hipMemset(p->d_palettes, 0, bytes);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);          // (the streams of a context do not wait for the null stream)
    if (e == hipSuccess) e = hipEventCreateWithFlags(&p->written, hipEventDisableTiming);
    if (e != hipSuccess) {
        destroy_pose_set(p);
        return fail_hip(c, "pose set allocation failed: ", e);
    }
    *out = p;
    return SWR_OK;
}

int pose_set_destroy(swr_context* c, swr_pose_set* p) {
    if (!p) return SWR_OK;
    int rc = pose_set_check(c, p); if (rc) return rc;
    destroy_pose_set(p);                       // (hipFree waits for the device: the kernels queued on the set are over by then)
    return SWR_OK;
}

int pose_set_sample(swr_context* c, swr_pose_set* p, const swr_skeleton* k, const swr_pose_request* requests, int n) {
    int rc;
    if ((rc = pose_set_check(c, p)) || (rc = skeleton_check(c, k))) return rc;
    if (n < 0 || n > p->n_instances) return fail(c, SWR_ERR_INVALID_ARG, "n must be within 0 .. n_instances");
    if (n > 0 && !requests) return fail(c, SWR_ERR_INVALID_ARG, "requests is null");
    if (k->n_joints != p->n_joints) return fail(c, SWR_ERR_INVALID_ARG, "the pose set's joint count is not the skeleton's");
    const int n_clips = (int)k->clip_base.size();
    for (int i = 0; i < n; ++i)
        if (requests[i].clip_a < 0 || requests[i].clip_a >= n_clips || requests[i].clip_b >= n_clips)
            return fail(c, SWR_ERR_INVALID_ARG, "a request names a clip the skeleton does not have");
    if (n == 0) return SWR_OK;
    if ((rc = ensure_front_stream(c))) return rc;
    if (p->world_nodes < k->n_nodes) {
        // the node matrices grow to the largest skeleton the set was sampled with (hipFree waits for the device: the first sample, once)
        if (p->d_worlds) { SWR_HIP(c, hipFree(p->d_worlds)); p->d_worlds = nullptr; p->world_nodes = 0; }
        SWR_HIP(c, hipMalloc((void**)&p->d_worlds, (size_t)p->n_instances * (size_t)k->n_nodes * 64));
        p->world_nodes = k->n_nodes;
    }
    const hipStream_t s = use_front_stream(c);
    const size_t bytes = (size_t)n * sizeof(PoseRequestDev);
    PaletteSlot* slot = nullptr;
    if ((rc = palette_slot(c, bytes, &slot))) return rc;
    PoseRequestDev* rq = static_cast<PoseRequestDev*>(slot->host.p);
    for (int i = 0; i < n; ++i) {
        const swr_pose_request& r = requests[i];
        rq[i] = PoseRequestDev{ k->clip_base[(size_t)r.clip_a], r.time_a, r.clip_b < 0 ? SWR_ANIM_NO_CLIP : k->clip_base[(size_t)r.clip_b], r.time_b, r.weight };
    }
    SWR_HIP(c, hipMemcpyAsync(slot->dev.p, slot->host.p, bytes, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_pose_sample, dim3((uint32_t)n), dim3(SWR_POSE_BLOCK), 0, s, skeleton_dev(k), (const uint32_t*)k->d_clips,
                       (const PoseRequestDev*)slot->dev.p, reinterpret_cast<float4*>(p->d_worlds), reinterpret_cast<float4*>(p->d_palettes),
                       (uint32_t)p->n_joints * 16u);
    SWR_HIP(c, hipGetLastError());
    if ((rc = palette_submit(c, slot, s))) return rc;
    return pose_set_written(c, p, s);
}

int pose_set_upload(swr_context* c, swr_pose_set* p, int first, int n, const float* palettes) {
    int rc = pose_set_check(c, p); if (rc) return rc;
    if (first < 0 || n < 0 || first > p->n_instances || n > p->n_instances - first) return fail(c, SWR_ERR_INVALID_ARG, "first .. first + n - 1 must be instances of the set");
    if (n > 0 && !palettes) return fail(c, SWR_ERR_INVALID_ARG, "palettes is null");
    if (n == 0) return SWR_OK;
    if ((rc = ensure_front_stream(c))) return rc;
    const hipStream_t s = use_front_stream(c);
    const size_t stride = (size_t)p->n_joints * 16, bytes = (size_t)n * stride * 4;
    PaletteSlot* slot = nullptr;
    if ((rc = palette_slot(c, bytes, &slot, false))) return rc;
    memcpy(slot->host.p, palettes, bytes);
    SWR_HIP(c, hipMemcpyAsync(p->d_palettes + (size_t)first * stride, slot->host.p, bytes, hipMemcpyHostToDevice, s));
    if ((rc = palette_submit(c, slot, s))) return rc;
    return pose_set_written(c, p, s);
}

int pose_set_readback(swr_context* c, const swr_pose_set* set, float* out) {
    int rc = pose_set_check(c, set); if (rc) return rc;
    if (!out) return fail(c, SWR_ERR_INVALID_ARG, "the destination is null");
    // a reader on the ray stream, as swr_mesh_readback: behind the set's last write and behind nothing else
    if ((rc = ensure_ray_stream(c))) return rc;
    swr_pose_set* p = const_cast<swr_pose_set*>(set);
    if (!p->written_seen) { SWR_HIP(c, hipStreamWaitEvent(c->ray_stream, p->written, 0)); p->written_seen = true; }
    SWR_HIP(c, hipMemcpyAsync(out, p->d_palettes, (size_t)p->n_instances * (size_t)p->n_joints * 64, hipMemcpyDeviceToHost, c->ray_stream));
    SWR_HIP(c, hipStreamSynchronize(c->ray_stream));
    return SWR_OK;
}

int mesh_skin_batch(swr_context* c, int n, swr_mesh* const* dst, const swr_mesh* const* src, const swr_pose_set* set, const int32_t* instance) {
    int rc = pose_set_check(c, set); if (rc) return rc;
    if (n < 0) return fail(c, SWR_ERR_INVALID_ARG, "n is negative");
    if (n == 0) return SWR_OK;
    if (!dst || !src || !instance) return fail(c, SWR_ERR_INVALID_ARG, "dst, src or instance is null");
    std::vector<const swr_mesh*> dsts((size_t)n);
    uint64_t blocks = 0;
    for (int k = 0; k < n; ++k) {
        if ((rc = deform_mesh_check(c, dst[k], "a destination mesh is null"))) return rc;
        if ((rc = deform_mesh_check(c, src[k], "a source mesh is null"))) return rc;
        if (src[k]->n_verts != dst[k]->n_verts) return fail(c, SWR_ERR_INVALID_ARG, "a job's source and destination must have equal vertex counts");
        if (!src[k]->has_skin) return fail(c, SWR_ERR_INVALID_ARG, "a source mesh has no skin attributes (swr_mesh_set_skin)");
        if (instance[k] < 0 || instance[k] >= set->n_instances) return fail(c, SWR_ERR_INVALID_ARG, "an instance is not one of the pose set's");
        if (set->n_joints <= src[k]->max_joint) return fail(c, SWR_ERR_INVALID_ARG, "the pose set's n_joints must exceed the largest joint index a source's skin attributes use");
        dsts[(size_t)k] = dst[k];
        blocks += ((uint64_t)dst[k]->n_verts + SWR_DEFORM_BLOCK - 1u) / SWR_DEFORM_BLOCK;
    }
    std::sort(dsts.begin(), dsts.end());
    if (std::adjacent_find(dsts.begin(), dsts.end()) != dsts.end()) return fail(c, SWR_ERR_INVALID_ARG, "a destination mesh appears twice in the batch");
    for (int k = 0; k < n; ++k)
        if (std::binary_search(dsts.begin(), dsts.end(), src[k])) return fail(c, SWR_ERR_INVALID_ARG, "a destination mesh is a job's source (make a target with swr_mesh_create_like)");
    if (blocks == 0) return SWR_OK;
    if (blocks > 0x7fffffffull) return fail(c, SWR_ERR_UNSUPPORTED, "the batch exceeds 2^31 blocks of vertices");
    hipStream_t s = nullptr;
    if ((rc = deform_begin(c, dsts.data(), dsts.size(), &s))) return rc;
    // the job table: jobs with vertices, by first block
    PaletteSlot* slot = nullptr;
    if ((rc = palette_slot(c, (size_t)n * sizeof(SkinJob), &slot))) return rc;
    SkinJob* jobs = static_cast<SkinJob*>(slot->host.p);
    uint32_t n_jobs = 0, first_block = 0;
    for (int k = 0; k < n; ++k) {
        if (dst[k]->n_verts == 0) continue;
        jobs[n_jobs++] = SkinJob{ src[k]->d_verts, src[k]->d_joints, src[k]->d_weights, dst[k]->d_verts, (uint32_t)dst[k]->n_verts, first_block,
                                  (uint32_t)instance[k] * (uint32_t)set->n_joints * 16u, 0u };
        first_block += ((uint32_t)dst[k]->n_verts + SWR_DEFORM_BLOCK - 1u) / SWR_DEFORM_BLOCK;
    }
    SWR_HIP(c, hipMemcpyAsync(slot->dev.p, slot->host.p, (size_t)n_jobs * sizeof(SkinJob), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_mesh_skin_batch, dim3(first_block), dim3(SWR_DEFORM_BLOCK), 0, s, (const SkinJob*)slot->dev.p, n_jobs,
                       (const float*)set->d_palettes, c->nm_flags);
    SWR_HIP(c, hipGetLastError());
    if ((rc = palette_submit(c, slot, s))) return rc;
    return deform_end(c, dst, n, s, true);
}
}  // namespace
