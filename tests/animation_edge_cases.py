"""Named cases at the branches and numeric edges of skeletal animation (test helper on top of tests/animation_cases.py; not part of
the package).  tests/test_animation_edges_host.py holds each case to the branch it is named for in the restatement;
tests/test_gpu_animation_edges.py runs them on the device, word for word.

  K1  key times with duplicates at the ENDS ([.5, .5, .75, 1, 1] and [.5, .5, .5]): on, beside, before and past them
  K2  rotation keys of length 2 and 0.5: an interior key hit exactly is NORMALISED (the lerp arm at u = 0), an end key is returned as stored
  K3  the divisor T[k+1] - T[k]: subnormal, +Inf, +Inf by overflow, and Inf / Inf
  Q1  Quaternion.Lerp at dot == 0 and dot == -0.0, between two keys and between two clips
  Q2  1 / sqrt(ls) with ls subnormal, underflowed to 0, large and overflowed to +Inf
  Q3  a rest rotation of length 2 on a node that one clip targets and the other does not
  H1  levels of 256, 257 and 513 nodes, every node a joint, a child's thread and its parent's in different waves
  H2 - H5  the host's sequencing: one set sampled with skeletons of 3, 514, 3 nodes; AddClip between samples; more samples than pinned
      request slots; n = 5, 2, 0 on one set
  B1  the batched skin's block table: (0, 128, 128, 256, 1, 0) vertices, and 300 jobs of one vertex

A Case is one call of swr_pose_set_sample on a set of its own.  `nan` states, as a literal, the (instance, joint) pairs of the palette
that hold a NaN -- same_words equates any NaN with any NaN, so the tests assert this set separately -- and `on` states, per instance,
the (arm, k, u word) the LINEAR rotation channel of node 1 takes (K families) or other branch facts the host file asserts.
The sheet skeleton of the K and Q families: node 0 a root without channels, nodes 1 and 2 its children; joint j is node j."""
from __future__ import annotations

import collections

import numpy as np

import animation_cases as A
from animation_cases import F32, LINEAR, R, S, STEP, T

Case = collections.namedtuple("Case", "name sk clips requests nan on")
PALETTE_SLOTS = 256                            # SWR_PALETTE_SLOTS_MAX of csrc/swr_host.h: palette_slot hands out that many at most


def word_of(x):
    return int(np.asarray(x, dtype=F32).reshape(1).view(np.uint32)[0])


def up(x):
    return np.nextafter(F32(x), F32(np.inf))


def down(x):
    return np.nextafter(F32(x), F32(-np.inf))


def one(t, clip=0):
    return (clip, F32(t), -1, F32(0.0), F32(0.0))


def sheet_skeleton(seed=0, rest_r=None, bare_node_1=False):
    """Three nodes (0 <- 1, 0 <- 2) with random rest T, R, S and inverse binds; joint j is node j.  bare_node_1: node 1 is a root with
    an identity inverse bind, so that palette 1 is its local matrix word for word (x + 0 = x) and shows elements of any magnitude."""
    sk = A.skeleton("star", 3, seed=seed, matrix_nodes=False)
    t, r, s, local = sk.rest_t.copy(), sk.rest_r.copy(), sk.rest_s.copy(), sk.rest_local.copy()
    if rest_r is not None:
        for i, q in rest_r.items():
            r[i] = q
            local[i] = A.compose(t[i], r[i], s[i])
    parent, ib = sk.parent.copy(), sk.inverse_bind.copy()
    if bare_node_1:
        parent[1], ib[1] = -1, np.eye(4, dtype=F32)
    return A.Skeleton(parent, local, t, r, s, [0, 1, 2], ib)


def distinct_keys(n, seed, scale_r=None):
    """n pairwise different keys per path: the key index shows in the words."""
    rng = np.random.default_rng(700 + seed)
    q = A._unit_quaternions(rng, n)
    if scale_r is not None:
        q = (q * np.asarray(scale_r, dtype=F32).reshape(n, 1)).astype(F32)
    tv = np.array([[k + 1, -0.5 * (k + 1), 0.25 * (k + 1)] for k in range(n)], dtype=F32)
    sv = np.array([[1 + 0.125 * k, 1 - 0.0625 * k, 0.75 + 0.25 * k] for k in range(n)], dtype=F32)
    return {T: tv, R: q, S: sv}


def sheet_clip(times, keys, paths=(T, R, S)):
    """Node 1: LINEAR channels on `paths`; node 2: the same keys as STEP."""
    tm = np.asarray(times, dtype=F32)
    return [(node, p, interp, tm, keys[p]) for node, interp in ((1, LINEAR), (2, STEP)) for p in paths]


# ============================================================================ K1
K1_TIMES_A = (0.5, 0.5, 0.75, 1.0, 1.0)
K1_TIMES_B = (0.5, 0.5, 0.5)
K1_A = (  # t, arm, k, u word
    (0.25, "first", 0, None), (0.5, "first", 0, None), (up(0.5), "between", 1, 0x34800000), (0.75, "between", 2, 0x00000000),
    (down(1.0), "between", 2, 0x3f7ffffc), (1.0, "last", 4, None), (1.5, "last", 4, None))
K1_B = ((0.25, "first", 0, None), (0.5, "first", 0, None), (0.75, "last", 2, None))


def k1_cases():
    out = []
    for name, times, rows in (("k1_duplicates_at_both_ends", K1_TIMES_A, K1_A), ("k1_all_keys_at_one_time", K1_TIMES_B, K1_B)):
        out.append(Case(name, sheet_skeleton(1), [sheet_clip(times, distinct_keys(len(times), 1))], [one(r[0]) for r in rows], frozenset(),
                        [r[1:] for r in rows]))
    return out


# ============================================================================ K2
K2_TIMES = (0.25, 0.5, 0.75, 1.0)
K2_LENGTHS = (2.0, 0.5, 2.0, 0.5)
K2 = ((0.125, "first", 0, None), (0.25, "first", 0, None), (down(0.5), "between", 0, 0x3f7ffffe), (0.5, "between", 1, 0x00000000),
      (up(0.5), "between", 1, 0x34800000), (down(0.75), "between", 1, 0x3f7ffffc), (0.75, "between", 2, 0x00000000),
      (up(0.75), "between", 2, 0x34800000), (1.0, "last", 3, None), (2.0, "last", 3, None))


def k2_cases():
    keys = distinct_keys(4, 2, scale_r=K2_LENGTHS)
    return [Case("k2_rotation_keys_of_length_2_and_half", sheet_skeleton(2), [sheet_clip(K2_TIMES, keys, paths=(R,))], [one(r[0]) for r in K2],
                 frozenset(), [r[1:] for r in K2])]


# ============================================================================ K3
K3_SUB = (F32(1e-40), F32(2e-40), F32(4e-40))        # words 0x000116c2, 0x00022d85, 0x00045b0a
INF = F32(np.inf)


def k3_cases():
    """(the u words of the subnormal case are those of subnormal differences divided exactly; a device that flushed them would
    divide 0 by 0)"""
    sub = [(F32(1.5e-40), "between", 0, 0x3f000076), (F32(3e-40), "between", 1, 0x3effff8a), (down(K3_SUB[1]), "between", 0, 0x3f7fff15)]
    mk = lambda name, times, rows, nan: Case(name, sheet_skeleton(3), [sheet_clip(times, distinct_keys(len(times), 3))],      # noqa: E731
                                             [one(r[0]) for r in rows], frozenset(nan), [r[1:] for r in rows])
    return [
        mk("k3_subnormal_divisor", K3_SUB, sub, ()),
        mk("k3_divisor_plus_inf", (0.0, INF), [(1.0, "between", 0, 0x00000000), (3e38, "between", 0, 0x00000000), (INF, "last", 1, None)], ()),
        # u = Inf / Inf: every LINEAR path of node 1 is NaN; node 2 (STEP) keeps key 0
        mk("k3_inf_over_inf", (-INF, 0.0), [(-1.0, "between", 0, "nan")], [(0, 1)]),
        mk("k3_divisor_overflows", (-3e38, 3e38), [(0.0, "between", 0, 0x00000000)], ()),
    ]


# ============================================================================ Q1
Q1_PAIRS = {
    "plus_zero": ((1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), 0x00000000, (0x3f72dce8, 0x3ea1e89b, 0x00000000, 0x00000000)),
    "minus_zero": ((1e-23, 1.0, 1.0, 1.0), (-1e-23, -0.0, -0.0, -0.0), 0x80000000, (0x1894e6ac, 0x3f13cd3a, 0x3f13cd3a, 0x3f13cd3a)),
    "minus_zero_w0": ((1e-23, 1.0, 1.0, 0.0), (-1e-23, -0.0, -0.0, -0.0), 0x80000000, (0x18b65da6, 0x3f3504f4, 0x3f3504f4, 0x00000000)),
}
"""a, b, the word of dot, the words of Quaternion.Lerp(a, b, 0.25): (0.94868326, 0.31622776, 0, 0) and
(3.849e-24, 0.57735026, 0.57735026, 0.57735026) -- all ADD.  In a rotation matrix the x of the second pair (3.8e-24 added, 7.7e-24
subtracted) only ever meets sums of order one, so no palette shows which arm ran; the third pair has w = 0 as well, which leaves
2 x y, 2 x z alone in four elements, and its cases put node 1 at a root under an identity inverse bind."""


def q1_cases():
    out = []
    for name, (a, b, _, _) in Q1_PAIRS.items():
        keys = {R: np.array([a, b], dtype=F32)}
        out.append(Case(f"q1_keys_dot_{name}", sheet_skeleton(4, bare_node_1=True), [sheet_clip((0.0, 1.0), keys, paths=(R,))], [one(0.25)], frozenset(), name))
        ca = [(1, R, STEP, np.array([0.0], F32), np.array([a], F32))]
        cb = [(1, R, STEP, np.array([0.0], F32), np.array([b], F32))]
        out.append(Case(f"q1_blend_dot_{name}", sheet_skeleton(4, bare_node_1=True), [ca, cb], [(0, F32(0.0), 1, F32(0.0), F32(0.25))], frozenset(), name))
    return out


# ============================================================================ Q2
Q2_A, Q2_B = (0.0, 0.0, 0.0, 1.0), (0.0, 0.6, 0.0, 0.8)
Q2 = (  # m, the word of ls at u = 0.5, the kind of result, NaN in joint 1
    (7.7e-20, 0x003a1ae1, "finite", False), (1e-19, 0x00620056, "finite", False), (1e-23, 0x00000000, "nan", True), (1e-30, 0x00000000, "nan", True),
    (1.2e19, 0x7ec30019, "finite", False), (2e19, 0x7f800000, "zero", False))
"""|0.5 a + 0.5 b|^2 = 0.9: m = 2e19 has finite squares (0.81 m^2 = 3.24e38) whose SUM is +Inf"""


def q2_keys(m):
    return np.array([np.asarray(Q2_A, dtype=F32) * F32(m), np.asarray(Q2_B, dtype=F32) * F32(m)], dtype=F32)


def q2_cases():
    return [Case(f"q2_length_{m:g}", sheet_skeleton(5), [sheet_clip((0.0, 1.0), {R: q2_keys(m)}, paths=(R,))], [one(0.5)],
                 frozenset([(0, 1)] if nan else []), (word, kind)) for m, word, kind, nan in Q2]


# ============================================================================ Q3
Q3_WEIGHTS = (0.0, 1.0, 0.5)


def q3_cases():
    """Nodes 1 and 2 have rest rotations of length 2 and rest MATRICES that are not their compose.  Clip a: R on node 1 (a unit key), T
    on node 2.  Clip b: S on node 1 only.  Node 1's R blends clip a's key with rest_r; node 2's R blends rest_r with rest_r: length 1."""
    q = A._unit_quaternions(np.random.default_rng(41), 3)
    sk = sheet_skeleton(6, rest_r={1: q[0] * F32(2.0), 2: q[1] * F32(2.0)})
    sk.rest_local[1:] = A._affine(np.random.default_rng(42), 2)
    ca = [(1, R, STEP, np.array([0.0], F32), q[2:3]), (2, T, STEP, np.array([0.0], F32), np.array([[1, 2, 3]], F32))]
    cb = [(1, S, STEP, np.array([0.0], F32), np.array([[1.5, 0.5, 2.0]], F32))]
    reqs = [(0, F32(0.0), 1, F32(0.0), F32(w)) for w in Q3_WEIGHTS]
    return [Case("q3_rest_rotation_of_length_2", sk, [ca, cb], reqs, frozenset(), None)]


def numerics_cases():
    """K1 - Q3: what also runs under the library variants and the Transform flags."""
    return k1_cases() + k2_cases() + k3_cases() + q1_cases() + q2_cases() + q3_cases()


# ============================================================================ H1
H1_SHAPES = {"h1_two_levels_of_256": (256, 2), "h1_two_levels_of_257": (257, 2), "h1_three_levels_of_257": (257, 3), "h1_513_below_one_root": (513, 0)}


def h1_case(name):
    """Levels of `width` nodes: the node at position i of a level has the node at position width - 1 - i of the level above as its
    parent (k_pose_sample gives position i to thread i % 256: wave i / 64 against wave (width - 1 - i) / 64).  Every node is a joint."""
    width, levels = H1_SHAPES[name]
    if levels == 0:
        sk = A.skeleton("star", width + 1, seed=21)
    else:
        sk = A.skeleton("tree", width * levels, seed=20 + levels)
        for l in range(levels):
            for i in range(width):
                sk.parent[l * width + i] = -1 if l == 0 else (l - 1) * width + (width - 1 - i)
    assert sk.n_joints == sk.n_nodes and sorted(sk.joint_node.tolist()) == list(range(sk.n_nodes))
    clips = [A.clip(sk, 300 + width + levels), A.clip(sk, 310 + width + levels)]
    reqs = [(0, F32(0.45), -1, F32(0.0), F32(0.0)), (1, F32(0.7), 0, F32(0.3), F32(0.375))]
    return Case(name, sk, clips, reqs, frozenset(), (width, levels))


# ============================================================================ H2 - H5: scripts
class Script:
    """Host calls in order.  ops: ("sample", set, skeleton, requests) | ("add_clip", skeleton, channels) | ("read", set).
    skeletons: name -> (Skeleton, [clips present from the start]); sets: name -> n_instances (n_joints is the skeletons')."""

    def __init__(self, name, skeletons, sets, ops):
        self.name, self.skeletons, self.sets, self.ops = name, skeletons, sets, ops

    def expected_reads(self, mut=()):
        """What each "read" returns, in order: a set holds zeros until sampled; a sample of n requests writes instances 0 .. n - 1."""
        clips = {k: list(v[1]) for k, v in self.skeletons.items()}
        n_joints = next(iter(self.skeletons.values()))[0].n_joints
        state = {k: np.zeros((n, n_joints, 4, 4), dtype=F32) for k, n in self.sets.items()}
        out = []
        for op in self.ops:
            if op[0] == "sample" and len(op[3]):
                state[op[1]][:len(op[3])] = A.palettes_of(self.skeletons[op[2]][0], clips[op[2]], op[3], mut)
            elif op[0] == "add_clip":
                clips[op[1]].append(op[2])
            elif op[0] == "read":
                out.append(state[op[1]].copy())
        return out


def _sk3(seed):
    sk = A.skeleton("tree", 3, seed=seed)
    return sk, [A.clip(sk, 400 + seed, cover=1.0)]


def h2_scripts():
    a, c = _sk3(1), _sk3(2)
    big = A.skeleton("tree", 514, seed=3, n_joints=3)
    b = (big, [A.clip(big, 403)])
    sks = {"a": a, "b": b, "c": c}
    ra, rb, rc = A.requests(2, 1, 401), A.requests(2, 1, 402), A.requests(2, 1, 403)
    return [
        Script("h2_3_514_3_read_each", sks, {"s": 2}, [("sample", "s", "a", ra), ("read", "s"), ("sample", "s", "b", rb), ("read", "s"),
                                                      ("sample", "s", "c", rc), ("read", "s")]),
        Script("h2_3_514_3_read_last", sks, {"s": 2}, [("sample", "s", "a", ra), ("sample", "s", "b", rb), ("sample", "s", "c", rc), ("read", "s")]),
        Script("h2_one_skeleton_twice_read_last", sks, {"s": 2}, [("sample", "s", "b", rb), ("sample", "s", "b", A.requests(2, 1, 404)), ("read", "s")]),
    ]


def h3_script():
    sk = A.skeleton("tree", 9, seed=4)
    c0, c1 = A.clip(sk, 410), A.clip(sk, 411)
    two = [(0, F32(0.4), 1, F32(0.9), F32(0.25)), (1, F32(0.6), 0, F32(0.35), F32(0.75))]
    return Script("h3_add_clip_between_samples", {"k": (sk, [c0])}, {"first": 2, "second": 2},
                  [("sample", "first", "k", A.requests(2, 1, 410)), ("add_clip", "k", c1), ("sample", "second", "k", two), ("read", "first"), ("read", "second")])


def h4_script():
    """One more sample than palette_slot has slots, back to back on as many one-instance sets, each at a time of its own."""
    sk, clips = _sk3(5)
    n = PALETTE_SLOTS + 1
    # the root's translation runs over all the request times, so that no two palettes are the same
    ramp = (0, T, LINEAR, np.array([0.0, 2.0], F32), np.array([[0, 0, 0], [512, -256, 128]], F32))
    clips = [[ch for ch in clips[0] if (ch[0], ch[1]) != (0, T)] + [ramp]]
    times = (np.arange(n) / F32(128.0)).astype(F32)
    sets = {f"s{k}": 1 for k in range(n)}
    return Script("h4_one_more_sample_than_slots", {"k": (sk, clips)}, sets,
                  [("sample", f"s{k}", "k", [one(times[k])]) for k in range(n)] + [("read", f"s{k}") for k in range(n)])


def h5_script():
    sk = A.skeleton("tree", 7, seed=6)
    clips = [A.clip(sk, 430), A.clip(sk, 431)]
    return Script("h5_n_5_then_2_then_0", {"k": (sk, clips)}, {"s": 5},
                  [("sample", "s", "k", A.requests(5, 2, 430)), ("sample", "s", "k", A.requests(2, 2, 431, two=True)), ("sample", "s", "k", []), ("read", "s")])


def scripts():
    return h2_scripts() + [h3_script(), h4_script(), h5_script()]


# ============================================================================ B1
B1_COUNTS = (0, 128, 128, 256, 1, 0)           # whole blocks of SWR_DEFORM_BLOCK = 128 vertices, then a block of one
B1_JOBS = 300                                   # 300 blocks of one vertex: nine steps of k_mesh_skin_batch's search (2^8 < 300 <= 2^9)
