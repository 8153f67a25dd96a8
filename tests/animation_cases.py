"""Cases and the numpy float32 restatement of skeletal animation (test helper; not part of the package).

csrc/swr_animation.hip.h samples clips and evaluates joint hierarchies on the GPU (k_pose_sample) and skins a crowd in one launch
(k_mesh_skin_batch).  The definitions are build-defined and have ONE form for every numerics build and either Transform flag
(include/swr.h "SKELETAL ANIMATION"): plain float32, no fused multiply-add, sums left to right.  They are
restated here operation by operation on numpy float32 scalars and arrays (one rounding per operation, as -ffp-contract=off gives):

  find_key          the key search: !(t > T[0]) -> key 0; t >= T[n-1] -> key n-1; else the largest k with T[k] <= t and u
  lerp / quaternion_lerp   a*(1-u) + b*u per scalar; Quaternion.Lerp's scalar form (the normalised lerp)
  compose           S x Matrix4x4.CreateFromQuaternion(R) x T
  mul               Matrix4x4.Multiply: ((a_i1 b_1j + a_i2 b_2j) + a_i3 b_3j) + a_i4 b_4j
  worlds            level by level, world[i] = local[i] x world[parent[i]] with the parent's world finished first
  palettes          inverse_bind[j] x world[node(j)]

Results are compared as mesh_deform_cases.same_words compares vertices: uint32 words, a NaN against a NaN by NaN-ness only."""
from __future__ import annotations

import json
import os

import numpy as np

F32 = np.float32
T, R, S = 0, 1, 2                             # SWR_ANIM_PATH_*
STEP, LINEAR, CUBICSPLINE = 0, 1, 2           # SWR_ANIM_*
PATH_NAMES = ("translation", "rotation", "scale")
INTERP_NAMES = ("STEP", "LINEAR", "CUBICSPLINE")

# node counts of the GPU cases: k_pose_sample strides 256 threads (four waves of 64) over the nodes, so 1, 65 and 257 leave a live
# lane alone in a wave, 63 / 64 sit at a wave's edge
NODE_COUNTS = (1, 2, 63, 64, 65, 257)
KEY_COUNTS = (1, 2, 3, 64, 65, 1000)
WEIGHTS = (0.0, 1.0, 0.5, -0.25, 1.5, float("nan"))


def same_words(got, want):
    """Word for word, NaN against NaN by NaN-ness.  Returns the indices that differ."""
    g, w = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    assert g.shape == w.shape, (g.shape, w.shape)
    ok = (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))
    return np.argwhere(~ok)


# ============================================================================ restatement
MUTANTS = ("first_lt", "last_gt", "search_lt", "key_at_u0", "norm_stored", "dot_gt", "dot_signbit", "rsqrt_flush", "targeted_by_a_only",
           "left_nested")
"""One-token departures from the definition that the restatement can take on request (`mut`, a tuple of these names; () is the
definition): tests/test_animation_edges_host.py shows which cases of tests/animation_edge_cases.py each one turns red.
  first_lt            t < T[0] in place of !(t > T[0])            last_gt     t > T[n-1] in place of t >= T[n-1]
  search_lt           T[mid] < t in the binary search             key_at_u0   an interior key hit exactly returns the stored key
  norm_stored         stored keys are normalised too              dot_gt      dot > 0 adds
  dot_signbit         the arm is chosen by dot's sign bit         rsqrt_flush a subnormal ls is taken as 0
  targeted_by_a_only  the untargeted test ignores clip b          left_nested ((l_i x l_p) x l_pp) x ... up the chain
A `probe`, where given, is called as probe(kind, **facts):
  "channel"  once per sampled channel: node, path, interpolation, t, arm ("first" | "last" | "between"), k, u (None unless between),
             dup_before (T[k-1] == T[k]), dup_after (T[k] == T[k+1]), and dot, ls, inv of the key interpolation (None where no
             Quaternion.Lerp ran); times and key (the channel's key times and the stored key k)
  "blend"    once per two-clip Quaternion.Lerp: node, dot, ls, inv
  "node"     once per node and request: node, targeted ("none" | "a" | "b" | "both"; "a" also for a single clip)"""


def find_key(times, t, mut=(), probe=None):
    """(k, u): key k as stored when u is None, else keys k and k + 1 at u = (t - T[k]) / (T[k+1] - T[k]) (the interpolation decides).
    probe, where given, is called with (arm, k, u)."""
    tm = np.asarray(times, dtype=F32)
    t = F32(t)
    n = tm.shape[0]
    if (t < tm[0]) if "first_lt" in mut else (not (t > tm[0])):       # (a NaN t lands here)
        if probe is not None:
            probe("first", 0, None)
        return 0, None
    if (t > tm[n - 1]) if "last_gt" in mut else (t >= tm[n - 1]):
        if probe is not None:
            probe("last", n - 1, None)
        return n - 1, None
    lo, hi = 0, n - 1                         # T[lo] <= t < T[hi]
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if (tm[mid] < t) if "search_lt" in mut else (tm[mid] <= t):
            lo = mid
        else:
            hi = mid
    if "key_at_u0" in mut and lo > 0 and t == tm[lo]:
        if probe is not None:
            probe("between", lo, None)
        return lo, None
    with np.errstate(all="ignore"):
        u = F32(F32(t - tm[lo]) / F32(tm[lo + 1] - tm[lo]))
    if probe is not None:
        probe("between", lo, u)
    return lo, u


def lerp(a, b, u):
    a, b, u = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32), F32(u)
    with np.errstate(all="ignore"):
        u1 = F32(F32(1.0) - u)
        return (a * u1 + b * u).astype(F32)


def _normalised(r, mut=(), probe=None):
    with np.errstate(all="ignore"):
        ls = ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3]
        if "rsqrt_flush" in mut and F32(0.0) < ls < np.finfo(F32).tiny:
            ls = F32(0.0)
        inv = F32(1.0) / np.sqrt(ls)
        if probe is not None:
            probe(ls, inv)
        return (r * inv).astype(F32)


def quaternion_lerp(a, b, u, mut=(), probe=None):
    """probe, where given, is called with (dot, ls, inv)."""
    a, b, u = np.asarray(a, dtype=F32).reshape(4), np.asarray(b, dtype=F32).reshape(4), F32(u)
    with np.errstate(all="ignore"):
        u1 = F32(F32(1.0) - u)
        dot = ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]
        if "dot_gt" in mut:
            adds = dot > F32(0.0)
        elif "dot_signbit" in mut:
            adds = not np.signbit(dot)
        else:
            adds = dot >= F32(0.0)
        r = (u1 * a + u * b) if adds else (u1 * a - u * b)
        r = r.astype(F32)
        return _normalised(r, mut, None if probe is None else (lambda ls, inv: probe(dot, ls, inv)))


def blend_values(path, a, b, u, mut=(), probe=None):
    return quaternion_lerp(a, b, u, mut, probe) if path == R else lerp(a, b, u)


def sample_channel(ch, t, mut=(), probe=None):
    """One channel (node, path, interpolation, times, values) at time t."""
    node, path, interp, times, values = ch
    values = np.asarray(values, dtype=F32).reshape(len(times), -1)
    seen = {}
    if probe is None:
        k, u = find_key(times, t, mut)
    else:
        k, u = find_key(times, t, mut, lambda arm, k, u: seen.update(arm=arm, k=k, u=u))
    if u is None or interp == STEP:
        out = values[k].copy()
        if "norm_stored" in mut and path == R:
            out = _normalised(out, mut)
    else:
        out = blend_values(path, values[k], values[k + 1], u, mut,
                           None if probe is None else (lambda dot, ls, inv: seen.update(dot=dot, ls=ls, inv=inv)))
    if probe is not None:
        tm = np.asarray(times, dtype=F32)
        kk = seen["k"]
        probe("channel", node=int(node), path=int(path), interpolation=int(interp), t=F32(t), arm=seen["arm"], k=kk, u=seen["u"],
              dup_before=bool(kk > 0 and tm[kk - 1] == tm[kk]), dup_after=bool(kk + 1 < len(tm) and tm[kk] == tm[kk + 1]),
              dot=seen.get("dot"), ls=seen.get("ls"), inv=seen.get("inv"), times=tm, key=values[kk])
    return out


def create_from_quaternion(q):
    x, y, z, w = (F32(v) for v in np.asarray(q, dtype=F32).reshape(4))
    one, two = F32(1.0), F32(2.0)
    with np.errstate(all="ignore"):
        xx, yy, zz = x * x, y * y, z * z
        xy, wz, xz, wy, yz, wx = x * y, z * w, z * x, y * w, y * z, x * w
        m = np.eye(4, dtype=F32)
        m[0, :3] = one - two * (yy + zz), two * (xy + wz), two * (xz - wy)
        m[1, :3] = two * (xy - wz), one - two * (zz + xx), two * (yz + wx)
        m[2, :3] = two * (xz + wy), two * (yz - wx), one - two * (yy + xx)
    return m


def compose(t, q, s):
    m = create_from_quaternion(q)
    s = np.asarray(s, dtype=F32).reshape(3)
    with np.errstate(all="ignore"):
        for i in range(3):
            m[i, :3] = m[i, :3] * s[i]
    m[3, :3] = np.asarray(t, dtype=F32).reshape(3)
    return m


def mul(a, b):
    """Matrix4x4.Multiply; a may be a stack (..., 4, 4) against one b or a stack of the same length."""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    with np.errstate(all="ignore"):
        r = a[..., :, 0:1] * b[..., 0:1, :] + a[..., :, 1:2] * b[..., 1:2, :]
        r = r + a[..., :, 2:3] * b[..., 2:3, :]
        return (r + a[..., :, 3:4] * b[..., 3:4, :]).astype(F32)


def mul_left_nested(chain):
    """((m0 x m1) x m2) x ...: what a thread that multiplies its way UP its ancestors computes -- NOT the definition."""
    r = chain[0]
    for m in chain[1:]:
        r = mul(r, m)
    return r


class Skeleton:
    def __init__(self, parent, rest_local, rest_t, rest_r, rest_s, joint_node, inverse_bind):
        self.parent = np.asarray(parent, dtype=np.int32)
        n = self.parent.shape[0]
        self.rest_local = np.ascontiguousarray(rest_local, dtype=F32).reshape(n, 4, 4)
        self.rest_t = np.ascontiguousarray(rest_t, dtype=F32).reshape(n, 3)
        self.rest_r = np.ascontiguousarray(rest_r, dtype=F32).reshape(n, 4)
        self.rest_s = np.ascontiguousarray(rest_s, dtype=F32).reshape(n, 3)
        self.joint_node = np.asarray(joint_node, dtype=np.int32)
        self.inverse_bind = np.ascontiguousarray(inverse_bind, dtype=F32).reshape(self.joint_node.shape[0], 4, 4)
        self.n_nodes, self.n_joints = n, int(self.joint_node.shape[0])

    def args(self):
        return (self.parent, self.rest_local, self.rest_t, self.rest_r, self.rest_s, self.joint_node, self.inverse_bind)

    def depth(self):
        d = np.zeros(self.n_nodes, dtype=np.int64)
        for i in range(self.n_nodes):
            d[i] = 0 if self.parent[i] < 0 else d[self.parent[i]] + 1
        return d


def locals_of(sk, clips, req, mut=(), probe=None):
    """Every node's local matrix under a request (clip_a, time_a, clip_b, time_b, weight); clips: a list of channel lists."""
    clip_a, time_a, clip_b, time_b, weight = req
    two = clip_b >= 0
    tables = []
    for c in (clip_a, clip_b) if two else (clip_a,):
        tab = {}
        for ch in clips[c]:
            tab[(int(ch[0]), int(ch[1]))] = ch
        tables.append(tab)
    rest = (sk.rest_t, sk.rest_r, sk.rest_s)
    out = sk.rest_local.copy()
    times = (time_a, time_b)
    deciding = tables[:1] if "targeted_by_a_only" in mut else tables
    for i in range(sk.n_nodes):
        if probe is not None:
            by = [any((i, p) in tab for p in (T, R, S)) for tab in tables] + [False]
            probe("node", node=i, targeted="both" if by[0] and by[1] else "a" if by[0] else "b" if by[1] else "none")
        if not any((i, p) in tab for tab in deciding for p in (T, R, S)):
            continue                                  # untargeted: the rest matrix's words
        trs = []
        for p in (T, R, S):
            vals = [sample_channel(tab[(i, p)], times[k], mut, probe) if (i, p) in tab else rest[p][i].copy() for k, tab in enumerate(tables)]
            if two:
                blend_probe = None if probe is None or p != R else (lambda dot, ls, inv, i=i: probe("blend", node=i, dot=dot, ls=ls, inv=inv))
                trs.append(blend_values(p, vals[0], vals[1], weight, mut, blend_probe))
            else:
                trs.append(vals[0])
        out[i] = compose(*trs)
    return out


def worlds_of(sk, local, mut=(), probe=None):
    world = np.array(local, dtype=F32, copy=True)
    if "left_nested" in mut:
        for i in range(sk.n_nodes):
            chain, p = [world[i]], sk.parent[i]
            while p >= 0:
                chain.append(local[p])
                p = sk.parent[p]
            world[i] = mul_left_nested(chain)
        return world
    d = sk.depth()
    for level in range(1, int(d.max()) + 1 if sk.n_nodes else 0):
        nodes = np.nonzero(d == level)[0]
        world[nodes] = mul(world[nodes], world[sk.parent[nodes]])      # the parents (level - 1) are finished
    return world


def palette_of(sk, clips, req, mut=(), probe=None):
    world = worlds_of(sk, locals_of(sk, clips, req, mut, probe), mut, probe)
    if sk.n_joints == 0:
        return np.zeros((0, 4, 4), dtype=F32)
    return mul(sk.inverse_bind, world[sk.joint_node])


def palettes_of(sk, clips, requests, mut=(), probe=None):
    return np.stack([palette_of(sk, clips, tuple(r), mut, probe) for r in requests])


# ============================================================================ generators
def _unit_quaternions(rng, n):
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F32)


def _affine(rng, n):
    m = np.zeros((n, 4, 4), dtype=F32)
    for k in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        m[k, :3, :3] = (q * rng.uniform(0.8, 1.25)).astype(F32)
        m[k, 3, :3] = rng.uniform(-1.0, 1.0, 3).astype(F32)
        m[k, 3, 3] = 1.0
    return m


def skeleton(kind, n_nodes, seed=0, n_joints=None, matrix_nodes=True):
    """kind: "chain" (depth n_nodes), "star" (one root, n_nodes - 1 children), "tree" (random parents), "forest" (two roots or more,
    random parents below them).  Rest T, R, S are random; a fifth of the nodes (with matrix_nodes) carry a rest MATRIX that is not
    the compose of their T, R, S -- a glTF node given as a matrix -- so that "an untargeted node keeps its rest words" is visible.
    Joints: n_joints nodes (default: all) in a shuffled order, with random inverse bind matrices."""
    rng = np.random.default_rng(4000 + 31 * n_nodes + seed)
    if kind == "chain":
        parent = np.arange(-1, n_nodes - 1)
    elif kind == "star":
        parent = np.concatenate([[-1], np.zeros(n_nodes - 1, dtype=np.int64)])
    elif kind == "tree":
        parent = np.array([-1] + [int(rng.integers(0, i)) for i in range(1, n_nodes)])
    elif kind == "forest":
        roots = min(n_nodes, 2 + seed % 2)
        parent = np.array([-1] * roots + [int(rng.integers(0, i)) for i in range(roots, n_nodes)])
    else:
        raise ValueError(kind)
    t = rng.uniform(-1.0, 1.0, (n_nodes, 3)).astype(F32)
    r = _unit_quaternions(rng, n_nodes)
    s = rng.uniform(0.75, 1.25, (n_nodes, 3)).astype(F32)
    local = np.stack([compose(t[i], r[i], s[i]) for i in range(n_nodes)])
    if matrix_nodes:
        as_matrix = rng.random(n_nodes) < 0.2
        local[as_matrix] = _affine(rng, int(as_matrix.sum()))
    nj = n_nodes if n_joints is None else n_joints
    joint_node = rng.permutation(n_nodes)[:nj] if nj <= n_nodes else rng.integers(0, n_nodes, nj)
    return Skeleton(parent, local, t, r, s, joint_node, _affine(rng, nj))


def key_times(rng, n_keys, duplicates=True):
    """non-decreasing key times from 0.25 on, about 0.1 apart, some of them repeated"""
    step = rng.uniform(0.05, 0.15, n_keys)
    if duplicates and n_keys > 2:
        step[rng.random(n_keys) < 0.15] = 0.0
    step[0] = 0.25
    return np.cumsum(step).astype(F32)


def channel(rng, node, path, interp, n_keys, duplicates=True):
    times = key_times(rng, n_keys, duplicates)
    if path == R:
        values = _unit_quaternions(rng, n_keys)
    elif path == S:
        values = rng.uniform(0.5, 1.5, (n_keys, 3)).astype(F32)
    else:
        values = rng.uniform(-2.0, 2.0, (n_keys, 3)).astype(F32)
    return (int(node), int(path), int(interp), times, values)


def clip(sk, seed, n_keys=5, cover=0.7, interp=None):
    """Channels on a random subset of the (node, path) pairs (every pair with cover = 1); interp None mixes STEP and LINEAR."""
    rng = np.random.default_rng(9000 + seed)
    out = []
    for i in range(sk.n_nodes):
        for p in (T, R, S):
            if rng.random() < cover:
                nk = n_keys if isinstance(n_keys, int) else int(n_keys[rng.integers(0, len(n_keys))])
                out.append(channel(rng, i, p, int(rng.integers(0, 2)) if interp is None else interp, nk))
    return out


def subset_sheet():
    """Eight root nodes and eight children, node k of each group with channels on the subset k of {T, R, S} (bit p = path p): every
    subset, on roots and below a parent."""
    sk = skeleton("forest", 16, seed=5)
    sk.parent[:] = [-1] * 8 + list(range(8))
    rng = np.random.default_rng(77)
    chans = []
    for i in range(16):
        for p in (T, R, S):
            if (i % 8) >> p & 1:
                chans.append(channel(rng, i, p, LINEAR, 4, duplicates=False))
    return sk, chans


def edge_times(times):
    """The key search's edges for one channel's key times: before, on and past the first and last key, on an interior key, between
    keys, on either side of a duplicate, NaN and the infinities."""
    tm = np.asarray(times, dtype=F32)
    out = [np.nextafter(tm[0], F32(-np.inf)), tm[0], np.nextafter(tm[0], F32(np.inf)), tm[-1], np.nextafter(tm[-1], F32(-np.inf)),
           np.nextafter(tm[-1], F32(np.inf)), F32(tm[-1] + F32(10.0)), F32(-1.0), F32(0.0), F32(np.nan), F32(np.inf), F32(-np.inf)]
    for k in range(1, len(tm) - 1):
        out += [tm[k], np.nextafter(tm[k], F32(-np.inf)), np.nextafter(tm[k], F32(np.inf)), F32((tm[k] + tm[k + 1]) * F32(0.5))]
    return np.unique(np.asarray(out, dtype=F32).view(np.uint32)).view(F32)       # (unique by words: NaN stays)


def requests(n, n_clips, seed, t_lo=0.0, t_hi=1.5, two=False):
    """n requests with a different time (and clip, where there are several) per instance."""
    rng = np.random.default_rng(12000 + seed)
    out = []
    for i in range(n):
        ca = int(rng.integers(0, n_clips))
        cb = int(rng.integers(0, n_clips)) if two else -1
        out.append((ca, F32(rng.uniform(t_lo, t_hi)), cb, F32(rng.uniform(t_lo, t_hi)), F32(rng.uniform(0.0, 1.0)) if two else F32(0.0)))
    return out


def nlerp_slerp_angle(spacing_deg, steps=2001):
    """The largest angle (degrees, float64) between the normalised lerp and the spherical lerp of two unit quaternions `spacing_deg`
    of ROTATION apart (half that on the quaternion sphere), over u in [0, 1]."""
    half = np.radians(spacing_deg) / 2.0                   # angle between the quaternions
    u = np.linspace(0.0, 1.0, steps)
    a = np.array([0.0, 0.0, 0.0, 1.0])
    b = np.array([0.0, 0.0, np.sin(half), np.cos(half)])
    n = (1.0 - u)[:, None] * a + u[:, None] * b
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    sl = (np.sin((1.0 - u) * half) / np.sin(half))[:, None] * a + (np.sin(u * half) / np.sin(half))[:, None] * b
    # the rotation between the two results: twice the angle between the quaternions
    d = np.clip(np.abs((n * sl).sum(axis=1)), 0.0, 1.0)
    return float(np.degrees(2.0 * np.arccos(d)).max())


# ============================================================================ a skinned, animated glTF file
def write_gltf(directory, name="animated", cubic=False):
    """A small skinned, animated .gltf + .bin: five nodes
         0 "rig" (no joint, TRS) -> 1 "hip" (joint) -> 2 "spine" (joint, given as a MATRIX);  1 -> 3 "pad" (no joint) -> 4 "hand" (joint)
       the mesh on node 5 with skin 0 whose joints are listed child-first [4, 2, 1]; two animations (the second with a STEP channel
       and a channel on the non-joint parent).  Returns (path, expected) where expected holds the arrays that were written."""
    rng = np.random.default_rng(321)
    blob = bytearray()
    views, accessors = [], []

    def add(arr, ctype, atype):
        arr = np.ascontiguousarray(arr)
        while len(blob) % 4:
            blob.append(0)
        views.append({"buffer": 0, "byteOffset": len(blob), "byteLength": arr.nbytes})
        blob.extend(arr.tobytes())
        acc = {"bufferView": len(views) - 1, "componentType": ctype, "count": int(arr.shape[0]), "type": atype}
        if atype == "VEC3" and ctype == 5126:
            acc["min"], acc["max"] = arr.min(axis=0).tolist(), arr.max(axis=0).tolist()
        accessors.append(acc)
        return len(accessors) - 1

    pos = rng.uniform(-1, 1, (6, 3)).astype(F32)
    nrm = np.tile(np.array([0, 0, 1], dtype=F32), (6, 1))
    joints = rng.integers(0, 3, (6, 4)).astype(np.uint16)
    w = rng.uniform(0.1, 1.0, (6, 4))
    weights = (w / w.sum(axis=1, keepdims=True)).astype(F32)
    idx = np.array([0, 1, 2, 3, 4, 5], dtype=np.uint16)
    ibm = _affine(rng, 3)
    a_pos, a_nrm = add(pos, 5126, "VEC3"), add(nrm, 5126, "VEC3")
    a_j, a_w, a_i = add(joints, 5123, "VEC4"), add(weights, 5126, "VEC4"), add(idx, 5123, "SCALAR")
    a_ibm = add(ibm.reshape(3, 16), 5126, "MAT4")
    q = _unit_quaternions(rng, 3)
    spine = _affine(rng, 1)[0]
    nodes = [
        {"name": "rig", "children": [1], "translation": [0.5, 0.0, -0.25], "scale": [1.0, 2.0, 1.0]},
        {"name": "hip", "children": [2, 3], "rotation": q[0].tolist(), "translation": [0.0, 1.0, 0.0]},
        {"name": "spine", "matrix": spine.reshape(-1).tolist()},
        {"name": "pad", "children": [4], "rotation": q[1].tolist()},
        {"name": "hand", "translation": [0.25, 0.5, 0.75], "rotation": q[2].tolist(), "scale": [0.5, 0.5, 0.5]},
        {"name": "body", "mesh": 0, "skin": 0},
    ]
    clips = []
    animations = []
    for c, spec in enumerate(([(1, R, LINEAR, 4), (4, T, LINEAR, 3), (4, S, LINEAR, 2)],
                              [(3, R, STEP, 3), (1, T, LINEAR, 5), (0, T, LINEAR, 2)])):
        chans, samplers, channels = [], [], []
        for node, path, interp, nk in spec:
            ch = channel(rng, node, path, CUBICSPLINE if cubic and c == 1 and path == T and node == 1 else interp, nk, duplicates=False)
            chans.append(ch)
            vals = ch[4] if ch[2] != CUBICSPLINE else np.repeat(ch[4], 3, axis=0)
            samplers.append({"input": add(ch[3], 5126, "SCALAR"), "output": add(vals, 5126, "VEC4" if path == R else "VEC3"),
                             "interpolation": INTERP_NAMES[ch[2]]})
            channels.append({"sampler": len(samplers) - 1, "target": {"node": node, "path": PATH_NAMES[path]}})
        animations.append({"name": f"clip{c}", "samplers": samplers, "channels": channels})
        clips.append(chans)
    doc = {"asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": [0, 5]}], "nodes": nodes,
           "meshes": [{"primitives": [{"attributes": {"POSITION": a_pos, "NORMAL": a_nrm, "JOINTS_0": a_j, "WEIGHTS_0": a_w}, "indices": a_i}]}],
           "skins": [{"name": "skin", "joints": [4, 2, 1], "inverseBindMatrices": a_ibm}],
           "animations": animations, "accessors": accessors, "bufferViews": views,
           "buffers": [{"uri": name + ".bin", "byteLength": len(blob)}]}
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, name + ".bin"), "wb") as f:
        f.write(bytes(blob))
    path = os.path.join(directory, name + ".gltf")
    with open(path, "w") as f:
        json.dump(doc, f)
    # the skeleton a loader must find: nodes 0, 1, 2, 3, 4 (all of them: 0 and 3 are ancestors), in pre-order 0, 1, 2, 3, 4
    rest_t = np.array([[0.5, 0.0, -0.25], [0.0, 1.0, 0.0], [0, 0, 0], [0, 0, 0], [0.25, 0.5, 0.75]], dtype=F32)
    rest_r = np.array([[0, 0, 0, 1], q[0], [0, 0, 0, 1], q[1], q[2]], dtype=F32)
    rest_s = np.array([[1, 2, 1], [1, 1, 1], [1, 1, 1], [1, 1, 1], [0.5, 0.5, 0.5]], dtype=F32)
    rest_local = np.stack([compose(rest_t[i], rest_r[i], rest_s[i]) for i in range(5)])
    rest_local[2] = spine
    expected = {"nodes": [0, 1, 2, 3, 4], "skeleton": Skeleton([-1, 0, 1, 1, 3], rest_local, rest_t, rest_r, rest_s, [4, 2, 1], ibm),
                "clips": clips, "joints": joints, "weights": weights, "positions": pos}
    return path, expected
