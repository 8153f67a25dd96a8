"""The cases of tests/raycast_edge_cases.py on the CPU, against the restatement and the oracle library alone (no GPU here;
tests/test_gpu_raycast_edges.py runs them on the device):

  - each case is on the branch it is named for: det, distance and key words as words, in the three dot orders and both cross models;
  - each host mutant of raycast_cases.MUTANTS turns exactly the cases named in RED red, old cases included;
  - REACH: a replay, through the restatement with a probe, of every input tests/test_gpu_raycast.py sends to the device, and of the new
    cases: which of the branches each set reaches (`python tests/test_raycast_edges_host.py` prints both columns;
    profiles/r25_raycast_edges.md keeps them)."""
import collections

import numpy as np
import pytest

import raycast_cases as R
import raycast_edge_cases as E
from oracle import binding as ob

F32 = np.float32
MODELS = [(order, fused) for order in (0, 1, 2) for fused in (False, True)]


@pytest.fixture(scope="module")
def ref(oracle_lib):
    return lambda case, **kw: R.reference(oracle_lib, "", case, **kw)


def parts(case, order, fused, ray=0, target=0, probe=None):
    tg = case.targets[target]
    return R.intersect(case.origins[ray], case.directions[ray], np.asarray(tg.vertices["position"], dtype=F32), tg.indices, case.mask, order, fused,
                       probe=probe)


# ------------------------------------------------------------------------------------------------ the cases are where they claim to be
def test_identity_matrices_everywhere():
    seq = [c for c, _ in E.e6_sequence()]
    for c in E.single_call_cases() + seq + list(E.e8_case()) + [E.e5_chunk_case(n) for n in E.E5_RAYS]:
        for t in c.targets:
            assert np.array_equal(t.model, np.eye(4, dtype=F32)) and np.array_equal(t.normal_matrix, np.eye(4, dtype=F32)), c.name


def test_e1_det_is_the_threshold_word():
    assert E.word_of(R.EPS) == E.EPS_WORD == 0x322bcc77
    for c in E.e1_cases():
        word = E.EPS_WORD + {"at": 0, "above": 1, "below": -1}[c.name.rsplit("_", 1)[1]]
        sign = 0x80000000 if "front_mask" in c.name else 0
        for order, fused in MODELS:
            seen = []
            alive, *_ = parts(c, order, fused, probe=lambda det, before, alive, dist: seen.append(det[0]))
            assert E.word_of(seen[0]) == (word | sign), (c.name, order, fused, hex(E.word_of(seen[0])))
            assert bool(alive[0]) == c.expect[0], (c.name, order, fused)


def test_e2_distance_words():
    for c in E.e2_cases():
        for order, fused in MODELS:
            alive, dist, *_ = parts(c, order, fused)
            assert alive[0], c.name                                   # RayIntersectsTriangle says yes in all four; the key decides
            if c.name in E.E2_WORDS:
                assert E.word_of(dist[0]) == E.E2_WORDS[c.name], (c.name, order, fused, hex(E.word_of(dist[0])))
            else:
                assert np.isfinite(dist[0]) and dist[0] > F32(9e29)
            assert (R.winner(alive, dist) is not None) == c.expect[0], c.name
    # the geometric distance of the overflow case is finite: 1e33 is a float, the product 1000 x (1e33 x 1000) is not
    with np.errstate(over="ignore"):
        assert np.isfinite(F32(1e33)) and np.isfinite(F32(1e33) * F32(1000)) and np.isinf(F32(1000) * (F32(1e33) * F32(1000)))


def test_e3_subnormal_words(ref):
    assert E.word_of(E.DENORM_MIN) == 1
    by = {c.name: c for c in E.e3_cases()}
    for order, fused in MODELS:
        alive, dist, *_ = parts(by["e3_distance_minus_denorm_min"], order, fused)
        assert not alive[0] and E.word_of(dist[0]) == 0x80000001
        alive, dist, *_ = parts(by["e3_distance_plus_denorm_min"], order, fused)
        assert alive[0] and E.word_of(dist[0]) == 0x00000001
        for name, words in (("e3_subnormal_twins_near_first", [1, 2]), ("e3_subnormal_twins_far_first", [2, 1])):
            alive, dist, *_ = parts(by[name], order, fused)
            assert alive.all() and [E.word_of(x) for x in dist] == words, name
    for name, tri in E.E3_WINNER.items():
        r = ref(by[name])[0, 0]
        assert int(r["triangle"]) == tri and E.word_of(r["distance"]) == 1 and r["normal"].tolist() == [0.0, 0.0, 1.0], name
    # a device that flushed subnormals would see the origin of the first case ON the plane, from where the ray hits, at a zero
    flushed = R.Case("flushed", [(.25, .25, -0.0)], [R.DOWN], [R.kat_target()], 1)
    r = ref(flushed)[0, 0]
    assert int(r["found"]) == 1 and float(r["distance"]) == 0.0


@pytest.mark.parametrize("fused", [False, True], ids=["cross_rounded", "cross_fused"])
@pytest.mark.parametrize("variant", list(R.DOT_ORDER))
def test_every_case_has_its_stated_outcome(variant, fused):
    lib = ob.load(variant=variant)
    seq = [c for c, _ in E.e6_sequence()]
    for c in E.single_call_cases() + seq + [E.e8_case()[1]]:
        got = R.reference(lib, variant, c, fused=fused)
        assert [bool(x) for x in got["found"].reshape(-1)] == list(c.expect), (c.name, variant, fused)


def test_e4_every_hit_is_the_last_triangle(ref):
    for reverse in (False, True):
        c, order = E.e4_case(reverse)
        assert [t.indices.shape[0] // 3 for t in c.targets] == [E.E4_COUNTS[k] for k in order]
        got = ref(c)
        for r in range(got.shape[0]):
            for t in range(got.shape[1]):
                T = E.E4_COUNTS[order[t]]
                assert int(got[r, t]["triangle"]) == (T - 1 if c.expect[r * got.shape[1] + t] else -1), (c.name, r, t)
        first_blocks = (E.E4_COUNTS[order[0]] + 255) // 256
        assert sum(int(x) >= 256 * first_blocks for x in got["triangle"].reshape(-1)) == 2       # 257 and 513: beyond target 0's blocks
        assert max(E.E4_COUNTS) != E.E4_COUNTS[order[0]]                                           # the first is not the largest


def test_e5_directions_differ_and_hits_and_misses_mix(ref):
    for n in E.E5_RAYS:
        c = E.e5_chunk_case(n)
        d = R.normalize3v(c.directions, 0)
        assert c.origins.shape[0] == n and np.unique(d, axis=0).shape[0] == n
        hits = int(ref(c)["found"].sum())
        assert n // 2 < hits < n, (n, hits)
    c = E.e5_only_31_and_32_case()
    assert np.unique(R.normalize3v(c.directions, 0), axis=0).shape[0] == 63            # 31 and 32 share (0, 0, -1), from different origins
    assert not np.array_equal(c.origins[31], c.origins[32])
    assert np.flatnonzero(ref(c)["found"].reshape(-1)).tolist() == [31, 32]


def test_e6_sequence_moves_every_key_word(ref):
    seq = E.e6_sequence()
    assert [(c.origins.shape[0], len(c.targets), nearest) for c, nearest in seq] == [(5, 3, False), (5, 3, False), (3, 5, False), (5, 3, True), (5, 3, True)]
    a, b, c3 = (ref(c) for c, _ in seq[:3])
    assert a["found"].all() and not b["found"].any()
    # (c) differs from (a) as a list of 15 key words in both directions: words that were hits are misses and the triangle-0 keys differ
    assert (c3["found"].reshape(-1) != a["found"].reshape(-1)).any() and (c3["distance"].reshape(-1) != a["distance"].reshape(-1)).all()
    fold = [R.fold_nearest(row) for row in ref(seq[3][0])]
    assert [int(f["target"]) for f in fold] == [0] * 5
    assert [int(R.fold_nearest(row)["target"]) for row in ref(seq[4][0])] == [-1] * 5


def test_e7_fold_winners(ref):
    for c, winners, word in E.e7_cases():
        got = ref(c)
        fold = [R.fold_nearest(row) for row in got]
        assert [int(f["target"]) for f in fold] == winners, c.name
        assert E.word_of(fold[0]["distance"]) == word, c.name
        le = [int(R.fold_nearest(row, mut=("fold_le",))["target"]) for row in got]
        assert le != winners, c.name                                  # every E7 case holds a tie the `<=` fold decides the other way
    plus, minus = (ref(c)[0] for c, _, _ in E.e7_cases()[:2])
    assert plus[0]["distance"] == plus[1]["distance"] and E.word_of(plus[0]["distance"]) != E.word_of(plus[1]["distance"])


def test_e8_uses_the_last_index(ref):
    full, small = E.e8_case()
    assert full.targets[0].vertices.shape[0] == 65536 and full.targets[0].indices.tolist() == [65535, 65534, 65533]
    v, s = full.targets[0].vertices, small.targets[0].vertices
    assert all(np.array_equal(v[name][[65535, 65534, 65533]], s[name][[2, 1, 0]]) for name in ("position", "normal"))
    r = ref(small)[0, 0]
    assert int(r["found"]) == 1 and float(r["distance"]) == 1.0
    # an index that lost bit 15 or was read as signed names a filler vertex: no hit there
    low = R.Case("low", full.origins, full.directions, [R.Target(v[:32768], [32767, 32766, 32765])], 1)
    assert int(ref(low)[0, 0]["found"]) == 0


# ------------------------------------------------------------------------------------------------ host mutants
RED = {
    "det_back_le": ["e1_back_mask_at"],
    "det_front_ge": ["e1_front_mask_at"],
    "absdet_le": ["e1_back_mask_at", "e1_no_mask_at", "e1_front_mask_at"],
    "uv_sum_ge": ["edges_inclusive"],                                                       # (.5, .5): u + v == 1, an old case
    "dist_le": ["origin_on_plane_front", "origin_on_plane_behind_mask0", "zero_twins_plus_first", "zero_twins_minus_first",
                "e7_minus_zero_then_plus_zero", "e7_plus_zero_then_minus_zero"],           # +-0.0: old cases see it
    "key_le_max": ["e2_distance_is_maxvalue"],
    "key_unchecked": ["zero_direction", "nan_origin", "inf_direction", "e2_distance_is_maxvalue", "e2_distance_overflows_to_inf"],
    "key_flush": ["e3_subnormal_twins_far_first"],
    "fold_le": ["nearest_ties", "e7_minus_zero_then_plus_zero", "e7_plus_zero_then_minus_zero", "e7_miss_then_two_that_tie", "e7_winners_first_and_last"],
}
NEW_ONLY = ("det_back_le", "det_front_ge", "absdet_le", "key_le_max", "key_flush")         # no old case turns red: the gap


def all_cases():
    seq = [c for c, _ in E.e6_sequence()]
    return R.host_cases() + R.tie_cases() + [R.nearest_tie_case()] + E.single_call_cases() + seq + [E.e8_case()[1]] + [E.e5_chunk_case(n) for n in E.E5_RAYS]


def test_host_mutants_turn_exactly_the_named_cases_red(ref):
    assert sorted(RED) == sorted(R.MUTANTS)
    cases = all_cases()
    clean = {c.name: ref(c) for c in cases}
    red = {}
    for m in R.MUTANTS:
        red[m] = []
        for c in cases:
            got = ref(c, mut=(m,))
            pairs = R.same_records(got, clean[c.name])
            fold = all(R.same_records(R.fold_nearest(a, mut=(m,)), R.fold_nearest(b)) for a, b in zip(got, clean[c.name]))
            if not (pairs and fold):
                red[m].append(c.name)
    print(red)
    assert red == RED
    old = {c.name for c in R.host_cases() + R.tie_cases() + [R.nearest_tie_case()]}
    assert sorted(m for m in RED if not old & set(RED[m])) == sorted(NEW_ONLY)


def test_mut_empty_is_the_reference(ref):
    for c in R.host_cases() + R.tie_cases():
        assert R.same_records(ref(c, mut=()), ref(c))
        assert R.same_records(ref(c, mut=(), rule="le"), ref(c, rule="le"))


# ------------------------------------------------------------------------------------------------ reach
class Reach:
    """Counts, over every (ray, target) of the cases given to it, the boundary values of the kernels' comparisons and launch shapes."""

    def __init__(self):
        self.n = collections.Counter()
        self.ray_counts = collections.Counter()
        self.max_index = 0

    def probe(self, det, before, alive, dist):
        w = np.ascontiguousarray(det).view(np.uint32)
        self.n["det == +eps"] += int((w == E.EPS_WORD).sum())
        self.n["det == -eps"] += int((w == (E.EPS_WORD | 0x80000000)).sum())
        d = np.ascontiguousarray(dist).view(np.uint32)
        self.n["distance == MaxValue, alive"] += int((alive & (d == 0x7f7fffff)).sum())
        self.n["distance one ULP below MaxValue, alive"] += int((alive & (d == 0x7f7ffffe)).sum())
        self.n["distance +Inf, alive"] += int((alive & (d == 0x7f800000)).sum())
        self.n["distance NaN, alive"] += int((alive & np.isnan(dist)).sum())
        self.n["distance a negative subnormal, at the distance test"] += int((before & (d > 0x80000000) & (d < 0x80800000)).sum())
        self.n["distance a positive subnormal, alive"] += int((alive & (d > 0) & (d < 0x00800000)).sum())
        self.n["distance +-0, alive"] += int((alive & ((d == 0) | (d == 0x80000000))).sum())

    def add(self, lib, case, fused=False):
        got = R.reference(lib, "", case, fused=fused, probe=self.probe)
        n_rays, n_targets = got.shape
        self.ray_counts[n_rays] += 1
        tris = [t.indices.shape[0] // 3 for t in case.targets]
        self.max_index = max([self.max_index] + [int(t.indices.max()) for t in case.targets if t.indices.size])
        if len(set(tris)) > 1:
            self.n["calls whose targets differ in size"] += 1
            if tris[0] != max(tris):
                self.n["... and the first target is not the largest"] += 1
            self.n["... hits beyond the first target's blocks"] += int((got["triangle"] >= 256 * ((tris[0] + 255) // 256)).sum())
        for row in got:
            hit = np.flatnonzero(row["found"])
            if hit.size > 1:
                d = row["distance"][hit]
                best = np.flatnonzero(d == d.min())
                if best.size > 1:
                    self.n["fold ties"] += 1
                    if len({E.word_of(x) for x in d[best]}) > 1:
                        self.n["fold ties between +0.0 and -0.0"] += 1
            if hit.size and hit[0] > 0:
                self.n["rays whose first target misses and a later one hits"] += 1
        return got


def old_inputs():
    """every (case, fused) tests/test_gpu_raycast.py sends to the device, in its order (the numerics tests repeat three of them with
    both cross models, the renderer tests two, test_arguments the KAT)"""
    cs = [(c, False) for c in R.host_cases()]
    cs += [(R.count_case(T, where)[0], False) for where in ("last", "first") for T in R.COUNTS]
    cs += [(c, False) for c in R.tie_cases()]
    cs += [(R.shape_case(n_rays, n_targets), False) for n_targets in (1, 3) for n_rays in (1, 2, 65)]
    cs += [(R.nearest_tie_case(), False), (R.dust2_case(), False)]
    cs += [(R.shape_case(n, 3), False) for n in (7278, 7280)]
    dust2 = R.dust2_case()
    big = max(range(len(dust2.targets)), key=lambda t: dust2.targets[t].vertices.shape[0])
    cs += [(c, True) for c in (R.count_case(65, "last")[0], R.Case("dust2_largest_mesh", dust2.origins, dust2.directions, [dust2.targets[big]], 1), R.shape_case(65, 1))]
    return cs


def new_inputs():
    seq = [c for c, _ in E.e6_sequence()]
    return [(c, False) for c in E.single_call_cases() + seq + [E.e8_case()[1]] + [E.e5_chunk_case(n) for n in E.E5_RAYS]] + [(c, True) for c in E.numerics_cases()]


def reach_of(lib, inputs):
    r = Reach()
    for c, fused in inputs:
        r.add(lib, c, fused)
    return r


NEVER_BEFORE = ("det == +eps", "det == -eps", "distance == MaxValue, alive", "distance one ULP below MaxValue, alive", "distance +Inf, alive",
                "distance a negative subnormal, at the distance test", "distance a positive subnormal, alive", "fold ties between +0.0 and -0.0")


def test_reach_before_and_after(oracle_lib):
    old, new = reach_of(oracle_lib, old_inputs()), reach_of(oracle_lib, new_inputs())
    new.max_index = 65535                                               # (E8's full mesh; the reference case carries its three vertices)
    print(report(old, new))
    for k in NEVER_BEFORE:
        assert old.n[k] == 0 and new.n[k] > 0, (k, old.n[k], new.n[k])
    assert sorted(old.ray_counts) == [1, 2, 3, 6, 42, 65, 7278, 7280]
    assert all(n in new.ray_counts for n in E.E5_RAYS) and not any(n in old.ray_counts for n in E.E5_RAYS)
    # dust2 is the one old call with targets of different sizes; its first mesh is not its largest and 7 of its hits lie beyond it
    assert old.n["calls whose targets differ in size"] == 1 and old.n["... hits beyond the first target's blocks"] == 7
    assert old.n["distance NaN, alive"] > 0 and old.n["fold ties"] > 0
    assert old.max_index < 65535
    assert new.n["... hits beyond the first target's blocks"] >= 3 and new.n["rays whose first target misses and a later one hits"] >= 3


def report(old, new):
    keys = list(dict.fromkeys(list(old.n) + list(new.n)))
    lines = ["| | old cases | new cases |", "|---|---|---|"]
    lines += [f"| {k} | {old.n[k]} | {new.n[k]} |" for k in keys]
    lines.append(f"| ray counts per call | {', '.join(map(str, sorted(old.ray_counts)))} | {', '.join(map(str, sorted(new.ray_counts)))} |")
    lines.append(f"| largest index | {old.max_index} | {new.max_index} |")
    return "\n".join(lines)


if __name__ == "__main__":
    ob.build()
    lib = ob.load()
    a, b = reach_of(lib, old_inputs()), reach_of(lib, new_inputs())
    b.max_index = 65535
    print(report(a, b))
