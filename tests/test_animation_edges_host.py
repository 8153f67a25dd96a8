"""The cases of tests/animation_edge_cases.py on the CPU, against the restatement alone (no GPU here; tests/test_gpu_animation_edges.py
runs them on the device):

  - each case is on the branch it is named for: arm, k and u as words, dot, ls and inv through the restatement's probe;
  - each case's palette holds NaN in exactly the (instance, joint) pairs it states;
  - each host mutant of animation_cases.MUTANTS turns exactly the cases named in RED red;
  - REACH: a replay, through the probed restatement, of every input tests/test_gpu_animation.py sends to swr_pose_set_sample, and of the
    new cases: which branches each set reaches (`python tests/test_animation_edges_host.py` prints both columns;
    profiles/r26_animation_edges.md keeps them)."""
import collections

import numpy as np
import pytest

import animation_cases as A
import animation_edge_cases as E

F32 = np.float32
TINY = np.finfo(F32).tiny


def words(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def nan_set(pal):
    return {(i, j) for i in range(pal.shape[0]) for j in range(pal.shape[1]) if np.isnan(pal[i, j]).any()}


def probed(case, mut=()):
    """(palettes, [(instance, kind, facts)]) of a case."""
    seen, pals = [], []
    for i, rq in enumerate(case.requests):
        pals.append(A.palette_of(case.sk, case.clips, tuple(rq), mut, lambda kind, i=i, **kw: seen.append((i, kind, kw))))
    return np.stack(pals), seen


def channel_facts(seen, node, path, instance=None):
    return [kw for i, kind, kw in seen if kind == "channel" and kw["node"] == node and kw["path"] == path and instance in (None, i)]


# ------------------------------------------------------------------------------------------------ the cases are where they claim to be
@pytest.mark.parametrize("case", E.k1_cases() + E.k2_cases() + E.k3_cases(), ids=lambda c: c.name)
def test_k_cases_take_the_stated_arm_key_and_u(case):
    pal, seen = probed(case)
    assert nan_set(pal) == set(case.nan)
    for i, (arm, k, u) in enumerate(case.on):
        lin, step = channel_facts(seen, 1, A.R, i)[0], channel_facts(seen, 2, A.R, i)[0]
        for f in (lin, step):                                         # the STEP channel searches the same keys
            assert (f["arm"], f["k"]) == (arm, k), (case.name, i, f)
            if u is None:
                assert f["u"] is None
            elif u == "nan":
                assert np.isnan(f["u"])
            else:
                assert E.word_of(f["u"]) == u, (case.name, i, hex(E.word_of(f["u"])))
        # LINEAR interpolates only between keys; STEP never does
        assert (lin["ls"] is not None) == (arm == "between") and step["ls"] is None


def test_k1_values():
    a, b = E.k1_cases()
    _, seen = probed(a)
    f = channel_facts(seen, 1, A.T)
    assert [x["dup_after"] for x in f[:2]] == [True, True] and [x["dup_before"] for x in f[5:]] == [True, True]      # T[0] == T[1], T[3] == T[4]
    assert f[2]["dup_before"] and f[2]["u"] == F32(2.3841858e-07) and f[4]["u"] == F32(0.99999976)
    keys = E.distinct_keys(5, 1)
    loc = [A.locals_of(a.sk, a.clips, rq) for rq in a.requests]
    # node 2 (STEP): t = .5 is key 0, just past it key 1 (the LAST of the duplicates), 1.0 is key 4; the translation is row 4
    assert [int(np.flatnonzero((keys[A.T] == l[2][3, :3]).all(axis=1))[0]) for l in loc] == [0, 0, 1, 2, 2, 4, 4]
    assert np.array_equal(loc[1][1][3, :3], keys[A.T][0]) and np.array_equal(loc[5][1][3, :3], keys[A.T][4])          # LINEAR: stored
    loc = [A.locals_of(b.sk, b.clips, rq) for rq in b.requests]
    keys = E.distinct_keys(3, 1)
    assert [int(np.flatnonzero((keys[A.T] == l[n][3, :3]).all(axis=1))[0]) for l in loc for n in (1, 2)] == [0, 0, 0, 0, 2, 2]


def test_k2_interior_keys_are_normalised_and_end_keys_are_not():
    (c,) = E.k2_cases()
    keys = c.clips[0][0][4]
    assert np.allclose(np.linalg.norm(keys, axis=1), E.K2_LENGTHS, rtol=1e-6)
    _, seen = probed(c)
    for i, (arm, k, u) in enumerate(c.on):
        lin = A.sample_channel(c.clips[0][0], c.requests[i][1])
        step = A.sample_channel(c.clips[0][1], c.requests[i][1])
        assert np.array_equal(words(step), words(keys[k]))
        if arm == "between":
            assert abs(float(np.linalg.norm(lin)) - 1.0) < 1e-6 and not np.array_equal(words(lin), words(keys[k]))
            f = channel_facts(seen, 1, A.R, i)[0]
            assert abs(float(f["inv"]) * E.K2_LENGTHS[k if u != 0x3f7ffffe and u != 0x3f7ffffc else k + 1] - 1.0) < 1e-5
        else:
            assert np.array_equal(words(lin), words(keys[k]))


def test_k3_divisors():
    sub, inf, nan, over = E.k3_cases()
    tm = np.asarray(E.K3_SUB, dtype=F32)
    assert [E.word_of(x) for x in tm] == [0x000116c2, 0x00022d85, 0x00045b0a]
    assert all(0 < F32(tm[k + 1] - tm[k]) < TINY for k in range(2))                                  # subnormal divisors
    assert [A.find_key(tm, rq[1])[1] for rq in sub.requests] == [F32(0.50000703), F32(0.49999648), F32(0.999986)]
    with np.errstate(all="ignore"):
        assert F32(F32(3e38) - F32(-3e38)) == F32(np.inf) and np.isnan(F32(np.inf) / F32(np.inf))
    pal, _ = probed(nan)
    assert np.isnan(pal[0, 1]).any() and np.isfinite(pal[0, 2]).all() and np.isfinite(pal[0, 0]).all()
    for c in (sub, inf, over):
        assert np.isfinite(probed(c)[0]).all(), c.name


def test_q1_dot_is_zero_and_the_lerp_adds():
    assert np.array_equal(A.quaternion_lerp(*E.Q1_PAIRS["plus_zero"][:2], 0.25)[:2], [F32(0.94868326), F32(0.31622776)])
    assert np.array_equal(A.quaternion_lerp(*E.Q1_PAIRS["minus_zero"][:2], 0.25)[1:], [F32(0.57735026)] * 3)
    for name, (a, b, dot_word, want) in E.Q1_PAIRS.items():
        r = A.quaternion_lerp(a, b, 0.25)
        assert [E.word_of(x) for x in r] == list(want), name
        u1, u = F32(0.75), F32(0.25)
        added = (u1 * np.asarray(a, F32) + u * np.asarray(b, F32)).astype(F32)
        assert not np.array_equal(words(r), words(A.quaternion_lerp(a, b, 0.25, ("dot_gt",)))), "subtracting gives other words"
        assert np.allclose(r, added / np.linalg.norm(added))
    for c in E.q1_cases():
        pal, seen = probed(c)
        assert nan_set(pal) == set()
        kind = "blend" if "blend" in c.name else "channel"
        f = [kw for _, k, kw in seen if k == kind and kw["node"] == 1 and kw.get("dot") is not None]
        assert len(f) == 1 and E.word_of(f[0]["dot"]) == E.Q1_PAIRS[c.on][2], c.name
        # the result is in the local matrix: node 1 composes rest T, the lerp, rest S
        q = A.quaternion_lerp(*E.Q1_PAIRS[c.on][:2], 0.25)
        local = A.locals_of(c.sk, c.clips, c.requests[0])
        assert np.array_equal(words(local[1]), words(A.compose(c.sk.rest_t[1], q, c.sk.rest_s[1])))


def test_q2_ls_words_and_the_three_kinds_of_result():
    for c, (m, word, kind, nan) in zip(E.q2_cases(), E.Q2):
        pal, seen = probed(c)
        f = channel_facts(seen, 1, A.R)[0]
        assert f["arm"] == "between" and f["u"] == F32(0.5) and E.word_of(f["ls"]) == word, (c.name, hex(E.word_of(f["ls"])))
        q = A.sample_channel(c.clips[0][0], 0.5)
        assert nan_set(pal) == set(c.nan) == ({(0, 1)} if nan else set())
        if kind == "finite":
            assert abs(float(np.linalg.norm(q.astype(np.float64))) - 1.0) < 1e-6
        elif kind == "nan":                                            # 0 x Inf and tiny x Inf
            assert f["inv"] == F32(np.inf) and np.isnan(q).any() and np.isinf(q).any()
        else:                                                          # inv = 1 / Inf = 0: the ZERO quaternion, no NaN
            assert f["inv"] == F32(0.0) and np.array_equal(q, np.zeros(4, F32))
            local = A.locals_of(c.sk, c.clips, c.requests[0])[1]
            assert np.array_equal(local[:3, :3], np.diag(c.sk.rest_s[1]))
    subnormal = [w for _, w, _, _ in E.Q2 if 0 < w < 0x00800000]
    assert len(subnormal) == 2 and [w for _, w, _, _ in E.Q2].count(0) == 2 and E.Q2[-1][1] == 0x7f800000
    with np.errstate(all="ignore"):                                   # every square of the last case is finite: the SUM overflows
        r = (F32(0.5) * E.q2_keys(2e19)[0] + F32(0.5) * E.q2_keys(2e19)[1]).astype(F32)
        assert np.isfinite(r * r).all() and np.isinf((r * r).sum(dtype=F32))


def test_q3_the_blend_reads_the_rest_rotation_not_the_matrix():
    (c,) = E.q3_cases()
    sk = c.sk
    assert all(abs(float(np.linalg.norm(sk.rest_r[i])) - 2.0) < 1e-6 for i in (1, 2))
    for rq, w in zip(c.requests, E.Q3_WEIGHTS):
        local = A.locals_of(sk, c.clips, rq)
        unit = sk.rest_r[2] * F32(0.5)                                  # Quaternion.Lerp(r, r, w) = r / |r|: dot = 4, ls = 4, exactly
        t2 = A.lerp(np.array([1, 2, 3], F32), sk.rest_t[2], w)
        assert np.array_equal(words(local[2]), words(A.compose(t2, A.quaternion_lerp(sk.rest_r[2], sk.rest_r[2], w), sk.rest_s[2])))
        assert np.allclose(A.quaternion_lerp(sk.rest_r[2], sk.rest_r[2], w), unit, rtol=1e-6)
        assert not np.array_equal(words(local[2]), words(sk.rest_local[2]))
        q1 = A.quaternion_lerp(c.clips[0][0][4][0], sk.rest_r[1], w)  # node 1: clip a's key against the REST rotation of clip b
        assert np.array_equal(words(local[1][:3, :3]), words(A.compose((0, 0, 0), q1, A.lerp(sk.rest_s[1], [1.5, 0.5, 2.0], w))[:3, :3]))
    pal, seen = probed(c)
    assert nan_set(pal) == set()
    assert {kw["targeted"] for _, k, kw in seen if k == "node" and kw["node"] in (1, 2)} == {"both", "a"}


def level_facts(sk):
    """(widths, all_joints, crossings): per level its width and whether every node of it is a joint; the number of nodes whose thread
    (position in the level mod 256) is in another wave than its parent's."""
    d = sk.depth()
    pos = np.zeros(sk.n_nodes, dtype=np.int64)
    widths, all_joints = [], []
    joints = set(sk.joint_node.tolist())
    for l in range(int(d.max()) + 1):
        nodes = np.nonzero(d == l)[0]
        pos[nodes] = np.arange(nodes.shape[0])
        widths.append(int(nodes.shape[0]))
        all_joints.append(all(int(n) in joints for n in nodes))
    crossings = sum(1 for i in range(sk.n_nodes) if sk.parent[i] >= 0 and d[i] >= 1 and widths[d[i]] > 64 and widths[d[i] - 1] > 64
                    and (pos[i] % 256) // 64 != (pos[sk.parent[i]] % 256) // 64)
    return widths, all_joints, crossings


def test_h1_shapes():
    for name, (width, levels) in E.H1_SHAPES.items():
        c = E.h1_case(name)
        widths, all_joints, crossings = level_facts(c.sk)
        assert widths == ([width] * levels if levels else [1, width]) and all(all_joints), name
        assert c.sk.n_nodes <= 771
        assert (crossings > width // 2) if levels else crossings == 0
        pal, seen = probed(c)
        assert nan_set(pal) == set() and np.isfinite(pal).all()
        assert not np.array_equal(c.sk.joint_node, np.arange(c.sk.n_nodes))                         # shuffled
        kinds = collections.Counter(kw["targeted"] for _, k, kw in seen if k == "node")
        assert kinds["none"] > 0 and kinds["a"] > 0 and kinds["b"] > 0 and kinds["both"] > 0
        matrix_nodes = sum(not np.array_equal(c.sk.rest_local[i], A.compose(c.sk.rest_t[i], c.sk.rest_r[i], c.sk.rest_s[i])) for i in range(c.sk.n_nodes))
        assert 0.1 < matrix_nodes / c.sk.n_nodes < 0.3


def test_the_scripts_read_what_they_say():
    by = {s.name: s for s in E.scripts()}
    for s in by.values():
        for r in s.expected_reads():
            assert nan_set(r) == set() and np.isfinite(r).all(), s.name
        assert len({sk.n_joints for sk, _ in s.skeletons.values()}) == 1
    s = by["h2_3_514_3_read_each"]
    assert [s.skeletons[op[2]][0].n_nodes for op in s.ops if op[0] == "sample"] == [3, 514, 3]
    each, last = s.expected_reads(), by["h2_3_514_3_read_last"].expected_reads()
    assert len(each) == 3 and len(last) == 1 and np.array_equal(words(each[2]), words(last[0]))
    assert not np.array_equal(words(each[0]), words(each[1])) and not np.array_equal(words(each[1]), words(each[2]))
    s = by["h2_one_skeleton_twice_read_last"]
    first = A.palettes_of(s.skeletons["b"][0], s.skeletons["b"][1], s.ops[0][3])
    assert not np.array_equal(words(first), words(s.expected_reads()[0]))                           # the stale pose is finite and different
    s = by["h3_add_clip_between_samples"]
    assert [op[0] for op in s.ops] == ["sample", "add_clip", "sample", "read", "read"] and all(rq[2] >= 0 for rq in s.ops[2][3])
    s = by["h4_one_more_sample_than_slots"]
    assert len(s.sets) == E.PALETTE_SLOTS + 1 and [op[0] for op in s.ops] == ["sample"] * 257 + ["read"] * 257
    reads = s.expected_reads()
    assert len({r.tobytes() for r in reads}) == 257                                                 # distinct requests, distinct palettes
    s = by["h5_n_5_then_2_then_0"]
    assert [len(op[3]) for op in s.ops if op[0] == "sample"] == [5, 2, 0]
    (r,) = s.expected_reads()
    first = A.palettes_of(s.skeletons["k"][0], s.skeletons["k"][1], s.ops[0][3])
    assert np.array_equal(words(r[2:]), words(first[2:])) and not np.array_equal(words(r[0]), words(first[0])) \
        and not np.array_equal(words(r[1]), words(first[1]))


def test_b1_counts():
    assert sum(E.B1_COUNTS) == 513 and [(n + 127) // 128 for n in E.B1_COUNTS] == [0, 1, 1, 2, 1, 0]
    assert 2 ** 8 < E.B1_JOBS <= 2 ** 9


# ------------------------------------------------------------------------------------------------ host mutants
def all_cases():
    return E.numerics_cases() + [E.h1_case(n) for n in ("h1_two_levels_of_257", "h1_three_levels_of_257")]


RED = {
    "first_lt": {"k1_duplicates_at_both_ends", "k1_all_keys_at_one_time", "k2_rotation_keys_of_length_2_and_half"},
    "last_gt": {"k1_duplicates_at_both_ends", "k2_rotation_keys_of_length_2_and_half", "k3_divisor_plus_inf"},
    "search_lt": {"k1_duplicates_at_both_ends", "k2_rotation_keys_of_length_2_and_half"},
    "key_at_u0": {"k2_rotation_keys_of_length_2_and_half"},
    # (every stored rotation key that is not of unit length to the last bit, and whose departure shows in a matrix: Q2's STEP keys
    # (0, 0, 0, m) do not, w enters a rotation matrix only in products with x, y, z; the NaN cases get NaN in joint 2 as well)
    "norm_stored": {"k1_duplicates_at_both_ends", "k2_rotation_keys_of_length_2_and_half", "q1_keys_dot_minus_zero", "q1_blend_dot_minus_zero",
                    "q1_keys_dot_minus_zero_w0", "q1_blend_dot_minus_zero_w0", "q2_length_1e-23", "q2_length_1e-30", "h1_two_levels_of_257",
                    "h1_three_levels_of_257"},
    # (the issue's pair (1e-23, 1, 1, 1) is NOT red under the two dot mutants: see animation_edge_cases.Q1_PAIRS)
    "dot_gt": {"q1_keys_dot_plus_zero", "q1_blend_dot_plus_zero", "q1_keys_dot_minus_zero_w0", "q1_blend_dot_minus_zero_w0"},
    "dot_signbit": {"q1_keys_dot_minus_zero_w0", "q1_blend_dot_minus_zero_w0"},
    "rsqrt_flush": {"q2_length_7.7e-20", "q2_length_1e-19"},
    "targeted_by_a_only": {"h1_two_levels_of_257", "h1_three_levels_of_257"},
    "left_nested": {"h1_three_levels_of_257"},
}


@pytest.fixture(scope="module")
def definition():
    return {c.name: (c, A.palettes_of(c.sk, c.clips, c.requests)) for c in all_cases()}


@pytest.mark.parametrize("mutant", A.MUTANTS)
def test_each_host_mutant_turns_the_named_cases_red(definition, mutant):
    red = set()
    for name, (c, want) in definition.items():
        got = A.palettes_of(c.sk, c.clips, c.requests, (mutant,))
        if A.same_words(got, want).size or nan_set(got) != set(c.nan):
            red.add(name)
    assert red == RED[mutant], (mutant, sorted(red ^ RED[mutant]))


def test_the_definition_is_green_and_every_case_states_its_nan_set(definition):
    assert set(RED) == set(A.MUTANTS)
    for name, (c, want) in definition.items():
        assert nan_set(want) == set(c.nan), name
        assert not A.same_words(A.palettes_of(c.sk, c.clips, c.requests, ()), want).size


def test_the_scripts_see_the_mutants_too():
    """targeted_by_a_only through H3 and H5 (a node only clip b targets), left_nested through every tree deeper than two."""
    by = {s.name: s for s in E.scripts()}
    for name, mutant in (("h3_add_clip_between_samples", "targeted_by_a_only"), ("h5_n_5_then_2_then_0", "targeted_by_a_only"),
                         ("h2_3_514_3_read_each", "left_nested")):
        want, got = by[name].expected_reads(), by[name].expected_reads((mutant,))
        assert any(A.same_words(g, w).size for g, w in zip(got, want)), (name, mutant)


# ------------------------------------------------------------------------------------------------ reach
def old_inputs():
    """Every (skeleton, clips, requests) tests/test_gpu_animation.py sends to swr_pose_set_sample, as that file builds them."""
    out = []
    one = lambda t: (0, F32(t), -1, F32(0.0), F32(0.0))                                               # noqa: E731
    for n in A.NODE_COUNTS:
        sk = A.skeleton("tree", n, seed=1)
        out.append((f"tree{n}", sk, [A.clip(sk, 10 + n), A.clip(sk, 20 + n)], A.requests(2, 2, n)))
    for kind, n in (("chain", 33), ("star", 200), ("forest", 40), ("forest", 2)):
        sk = A.skeleton(kind, n, seed=0)
        out.append((f"{kind}{n}", sk, [A.clip(sk, 30 + n)], A.requests(2, 1, 7)))
    for n in (1, 2, 17):
        sk = A.skeleton("tree", 65, seed=2, n_joints=40)
        out.append((f"instances{n}", sk, [A.clip(sk, 40 + k) for k in range(3)], A.requests(n, 3, n)))
    for nk in A.KEY_COUNTS:
        sk = A.skeleton("chain", 3, seed=3)
        clips = [A.clip(sk, 50 + nk, n_keys=nk, cover=1.0)]
        out.append((f"keys{nk}", sk, clips, A.requests(9, 1, nk, t_hi=float(max(c[3][-1] for c in clips[0])) + 0.1)))
    sk = A.skeleton("tree", 20, seed=4)
    out.append(("step_linear", sk, [A.clip(sk, 60, n_keys=(2, 3, 7), cover=1.0)], A.requests(5, 1, 60)))
    sk = A.skeleton("chain", 3, seed=5)
    times = np.array([0.25, 0.5, 0.5, 0.5, 0.75, 1.25], dtype=F32)
    rng = np.random.default_rng(70)
    clip = []
    for i in range(3):
        for p in (A.T, A.R, A.S):
            ch = A.channel(rng, i, p, A.LINEAR if (i + p) % 3 else A.STEP, len(times))
            clip.append((ch[0], ch[1], ch[2], times, ch[4]))
    out.append(("edge_times", sk, [clip], [one(t) for t in A.edge_times(times)]))
    sk = A.skeleton("chain", 2, seed=6, matrix_nodes=False)
    out.append(("zero_quaternion", sk, [[(1, A.R, A.LINEAR, np.array([0.0, 1.0], F32), np.zeros((2, 4), F32))]], [one(0.5)]))
    sk = A.skeleton("tree", 24, seed=7)
    clips = [A.clip(sk, 80, cover=0.5), A.clip(sk, 81, cover=0.5)]
    for w in A.WEIGHTS:
        out.append((f"weight{w}", sk, clips, [(0, F32(0.45), 1, F32(0.8), F32(w)), (1, F32(0.3), 0, F32(0.6), F32(w)), (0, F32(0.45), 0, F32(0.45), F32(w))]))
    out.append(("clip_b_minus_one", sk, clips, [(0, F32(0.45), -1, F32(0.8), F32(0.5)), (0, F32(0.45), -1, F32(np.nan), F32(np.nan)),
                                                (0, F32(0.45), -7, F32(3.0), F32(-2.0))]))
    sk, chans = A.subset_sheet()
    out.append(("subset_sheet", sk, [chans], [one(0.4)]))
    out.append(("subset_sheet_empty_clip", sk, [chans, []], [(1, F32(0.4), -1, F32(0.0), F32(0.0)), (0, F32(0.4), 1, F32(0.0), F32(0.25))]))
    sk = A.skeleton("tree", 65, seed=8)
    out.append(("one_definition", sk, [A.clip(sk, 90), A.clip(sk, 91)], A.requests(3, 2, 90) + A.requests(2, 2, 91, two=True)))
    sk = A.skeleton("tree", 9, seed=9)
    out.append(("pose_set", sk, [A.clip(sk, 95)], A.requests(3, 1, 95)))
    sk = A.skeleton("tree", 8, seed=10, n_joints=5)
    out.append(("crowd", sk, [A.clip(sk, 100), A.clip(sk, 101)], A.requests(7, 2, 100)))
    sk = A.skeleton("tree", 6, seed=11)
    out.append(("refusals", sk, [A.clip(sk, 110)], A.requests(2, 1, 110)))
    for kind in ("star", "chain"):
        sk = A.skeleton(kind, 1100, seed=12, n_joints=8, matrix_nodes=False)
        sk.rest_s[:] = 1.0
        sk.rest_local[:] = np.stack([A.compose(sk.rest_t[i], sk.rest_r[i], sk.rest_s[i]) for i in range(sk.n_nodes)])
        out.append((f"{kind}1100", sk, [[A.channel(np.random.default_rng(5), n, A.R, A.LINEAR, 3) for n in (0, 500, 1099)]], [one(0.4)]))
    ident = np.eye(4, dtype=F32)
    sk = A.Skeleton([-1, 0, 1], [ident] * 3, np.zeros((3, 3)), [[0, 0, 0, 1]] * 3, np.ones((3, 3)), [0, 1, 2], [ident] * 3)
    q = np.array([0.0, 0.0, np.sin(0.15), np.cos(0.15)], dtype=F32)
    tm = np.array([0.0, 1.0], F32)
    stage = [(0, A.T, A.LINEAR, tm, np.array([[0, 0, 0], [0.3, 0.0, 0.0]], F32)), (1, A.R, A.LINEAR, tm, np.array([[0, 0, 0, 1], q], F32)),
             (2, A.S, A.STEP, tm, np.array([[1, 1, 1], [1, 0.5, 1]], F32))]
    out.append(("stage", sk, [stage], [one(0.0), one(1.0)]))
    sk = A.Skeleton([-1], [ident], [[0, 0, 0]], [[0, 0, 0, 1]], [[1, 1, 1]], [0], [ident])
    out.append(("ray", sk, [[(0, A.T, A.LINEAR, tm, np.array([[0, 0, 0], [20, 0, 0]], F32))]], [one(0.5), one(0.0)]))
    steps = [(0, A.T, A.STEP, np.arange(6, dtype=F32), np.array([[10.0 * k, 0, 0] for k in range(6)], F32))]
    out.append(("ray_batches", sk, [steps], [one(float(s)) for s in range(6)]))
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        _, want = A.write_gltf(d)
    out.append(("gltf", want["skeleton"], want["clips"], [(0, F32(0.45), -1, F32(0.0), F32(0.0)), (1, F32(0.5), 0, F32(0.4), F32(0.25))]))
    return out


def new_inputs():
    out = [(c.name, c.sk, c.clips, c.requests) for c in E.numerics_cases() + [E.h1_case(n) for n in E.H1_SHAPES]]
    for s in E.scripts():
        clips = {k: list(v[1]) for k, v in s.skeletons.items()}
        for op in s.ops:
            if op[0] == "add_clip":
                clips[op[1]].append(op[2])
            elif op[0] == "sample" and len(op[3]):
                out.append((s.name, s.skeletons[op[2]][0], list(clips[op[2]]), op[3]))
    return out


ROWS = ("t == T[0] == T[1] (first arm)", "t == T[n-1] == T[n-2] (last arm)", "channels whose keys are all one time (n > 1)",
        "LINEAR rotation on an interior key (u == 0)", "... whose key is not of unit length", "dot == 0 with ls > 0, between keys",
        "dot == 0 with ls > 0, between clips", "... dot == -0.0", "ls subnormal", "ls == 0", "ls == +Inf", "divisor subnormal",
        "divisor +Inf", "u NaN (Inf / Inf)", "levels of 256 or more, every node a joint", "nodes in another wave than their parent",
        "nodes only clip b targets")


def reach(inputs):
    n = collections.Counter({r: 0 for r in ROWS})
    seen_sk = set()
    for _, sk, clips, reqs in inputs:
        for c in {id(c): c for clip in clips for c in clip}.values():
            tm = np.asarray(c[3], dtype=F32)
            n[ROWS[2]] += int(tm.shape[0] > 1 and tm[0] == tm[-1])

        def probe(kind, **f):
            if kind == "node":
                n[ROWS[16]] += f["targeted"] == "b"
                return
            if kind == "blend":
                if f["dot"] == 0 and f["ls"] > 0:
                    n[ROWS[6]] += 1
                    n[ROWS[7]] += bool(np.signbit(f["dot"]))
            else:
                tm = f["times"]
                n[ROWS[0]] += f["arm"] == "first" and f["t"] == tm[0] and f["dup_after"]
                n[ROWS[1]] += f["arm"] == "last" and f["t"] == tm[-1] and f["dup_before"]
                if f["arm"] == "between":
                    with np.errstate(all="ignore"):
                        div = F32(tm[f["k"] + 1] - tm[f["k"]])
                    n[ROWS[11]] += bool(0 < div < TINY)
                    n[ROWS[12]] += bool(np.isinf(div))
                    n[ROWS[13]] += bool(np.isnan(f["u"]))
                if f["ls"] is not None:
                    if f["u"] == 0 and f["t"] == tm[f["k"]]:
                        n[ROWS[3]] += 1
                        key = f["key"].astype(np.float64)
                        n[ROWS[4]] += abs(float(key @ key) - 1.0) > 1e-3
                    if f["dot"] == 0 and f["ls"] > 0:
                        n[ROWS[5]] += 1
                        n[ROWS[7]] += bool(np.signbit(f["dot"]))
            if f.get("ls") is not None:
                n[ROWS[8]] += bool(0 < f["ls"] < TINY)
                n[ROWS[9]] += bool(f["ls"] == 0)
                n[ROWS[10]] += bool(np.isposinf(f["ls"]))

        for rq in reqs:
            A.locals_of(sk, clips, tuple(rq), (), probe)
        if id(sk) not in seen_sk:
            seen_sk.add(id(sk))
            widths, all_joints, crossings = level_facts(sk)
            n[ROWS[14]] += sum(w >= 256 and a for w, a in zip(widths, all_joints))
            n[ROWS[15]] += crossings
    return n


# the host's sequencing, by reading tests/test_gpu_animation.py: every set there is sampled with ONE skeleton and ONE n; the only
# AddClip calls after a sample are the refused ones (the blob is not rebuilt); the longest run of samples without a readback of a
# sampled set is the 11 frames of the sample-skin-draw-present loop (11 request slots and 11 job tables on one context)
OLD_SEQUENCING = {"sets sampled with a larger skeleton than before": 0, "accepted AddClip after a sample": 0, "sets sampled with two different n": 0,
                  "most samples on one context before a palette is read": 11}


def new_sequencing():
    n = collections.Counter()
    most = 0
    for s in E.scripts():
        nodes, counts, sampled, run = {}, collections.defaultdict(set), False, 0
        for op in s.ops:
            if op[0] == "sample":
                if not len(op[3]):
                    counts[op[1]].add(0)
                    continue
                k = s.skeletons[op[2]][0].n_nodes
                n["sets sampled with a larger skeleton than before"] += op[1] in nodes and k > nodes[op[1]]
                nodes[op[1]] = max(k, nodes.get(op[1], 0))
                counts[op[1]].add(len(op[3]))
                sampled, run = True, run + 1
                most = max(most, run)
            elif op[0] == "add_clip":
                n["accepted AddClip after a sample"] += sampled
            else:
                run = 0
        n["sets sampled with two different n"] += sum(len(v) > 1 for v in counts.values())
    n["most samples on one context before a palette is read"] = most
    return n


def test_reach_before_and_after():
    old, new = reach(old_inputs()), reach(new_inputs())
    zero_before = [ROWS[k] for k in (0, 1, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15)]
    for r in zero_before:
        assert old[r] == 0, (r, old[r])
    for r in ROWS:
        assert new[r] > 0, r
    # reached before, but only where both sides of the branch give the same words, or nearly: interior keys of unit length, and the
    # all-zero quaternion (ls == 0, NaN on either arm)
    assert old[ROWS[3]] > 0 and old[ROWS[9]] == 1
    # one random three-key channel of the old inputs has all its keys at one time, but no request time falls on it (rows 0 and 1)
    assert old[ROWS[2]] == 1
    # ... and this the old inputs did reach (the hand-worked node of tests/test_animation_host.py is one such, too)
    assert old[ROWS[16]] > 0
    seq = new_sequencing()
    assert seq["sets sampled with a larger skeleton than before"] == 2 and seq["accepted AddClip after a sample"] == 1
    assert seq["sets sampled with two different n"] == 1 and seq["most samples on one context before a palette is read"] == E.PALETTE_SLOTS + 1
    assert OLD_SEQUENCING["most samples on one context before a palette is read"] < E.PALETTE_SLOTS


if __name__ == "__main__":
    old, new = reach(old_inputs()), reach(new_inputs())
    print(f"{'':64s} {'old':>6s} {'new':>6s}")
    for r in ROWS:
        print(f"{r:64s} {old[r]:6d} {new[r]:6d}")
    seq = new_sequencing()
    for r, v in OLD_SEQUENCING.items():
        print(f"{r:64s} {v:6d} {seq[r]:6d}")
