// swr_animation_layout.h -- where the arrays of a skeleton lie in its device blob (swr_skeleton::d_static) and how many words the
// pieces of a clip blob take (swr_skeleton::d_clips, read by swr_animation.hip.h), in 32-bit words.  No HIP types: pure functions of
// counts (tests/test_animation_layout_host.py builds them with the host compiler).  swr_deform.h fills and reads the blobs by these.
#pragma once
#include <cstddef>
#include "swr.h"

namespace swr {
// d_static: rest_local | inverse_bind | rest_t | rest_r | rest_s | parent | order | level_start | joint_node -- the matrices first
// (16-byte loads: their offsets are multiples of 4 words whatever the counts)
struct SkeletonLayout { size_t rest_local, inverse_bind, rest_t, rest_r, rest_s, parent, order, level_start, joint_node, words; };
inline SkeletonLayout skeleton_layout(size_t n_nodes, size_t n_joints, size_t n_levels) {
    SkeletonLayout l;
    l.rest_local = 0; l.inverse_bind = l.rest_local + 16 * n_nodes; l.rest_t = l.inverse_bind + 16 * n_joints;
    l.rest_r = l.rest_t + 3 * n_nodes; l.rest_s = l.rest_r + 4 * n_nodes; l.parent = l.rest_s + 3 * n_nodes;
    l.order = l.parent + n_nodes; l.level_start = l.order + n_nodes; l.joint_node = l.level_start + n_levels + 1;
    l.words = l.joint_node + n_joints;
    return l;
}
// a clip: its node table (one word per node and path: where the channel lies, 0 for none), then its channels
constexpr size_t clip_table_words(size_t n_nodes) { return 3 * n_nodes; }
// a channel: interpolation | n_keys | times | values, a rotation key of 4 components and any other of 3
constexpr size_t clip_channel_comps(int path) { return path == SWR_ANIM_PATH_ROTATION ? 4 : 3; }
constexpr size_t clip_channel_words(int path, size_t n_keys) { return 2 + n_keys * (1 + clip_channel_comps(path)); }
}  // namespace swr
