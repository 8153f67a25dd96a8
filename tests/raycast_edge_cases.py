"""Named cases at the branches of the ray queries (test helper on top of tests/raycast_cases.py; not part of the package).

Every case keeps identity model and normal matrices, so the world vertices are the stored words under every build and both Transform
flags, and states its expected `found` per (ray, target) as a literal.  tests/test_raycast_edges_host.py holds each to the branch it
is named for in the restatement; tests/test_gpu_raycast_edges.py runs them on the device.

  E1  det == +-float32(1e-8) and its two neighbours, under `det < eps` (mask 1), `fabsf(det) < eps` alone (mask 0), `det > -eps` (mask 2)
  E2  distance float.MaxValue (no key), one ULP below (the largest key), +Inf by overflow of a finite geometric distance, 1e30
  E3  distance -denorm_min (a miss), +denorm_min (word 1), and twins at words 1 and 2 in both index orders
  E4  targets of 1, 0, 256, 257, 513 and 64 triangles in one call, forwards and backwards: the only hit is each one's LAST triangle
  E5  31 / 32 / 33 / 63 / 64 rays of different directions; 64 rays of which only 31 and 32 hit
  E6  the sequence of queries over one key buffer (all hit; all miss; another n_targets; nearest all hit, nearest all miss)
  E7  the fold over targets: -0.0 then +0.0 and the reverse, a miss followed by two that tie, winners first and last in one call
  E8  a mesh of 65536 vertices (swr_mesh_create accepts every count a 16-bit index can name) whose triangle is (65535, 65534, 65533)"""
from __future__ import annotations

import numpy as np

import raycast_cases as R
from raycast_cases import DOWN, F32, KAT_POS, UP, Case, Target, make_vertices

EPS_WORD = 0x322bcc77                          # float32(1e-8)
DENORM_MIN = np.nextafter(F32(0), F32(1))      # word 0x00000001
MAX_BELOW = np.nextafter(R.FLT_MAX, F32(0))    # word 0x7f7ffffe
E4_COUNTS = (1, 0, 256, 257, 513, 64)
E5_RAYS = (31, 32, 33, 63, 64)


def f32_of(word):
    return np.array([word], dtype=np.uint32).view(F32)[0]


def word_of(x):
    return int(np.asarray(x, dtype=F32).reshape(1).view(np.uint32)[0])


# ============================================================================ E1
def e1_cases():
    """(0,0,0), (a,0,0), (0,1,0) from (a/4, .25, 1) straight down: pvec = (1, 0, 0) (reversed winding: (0, -a, 0)), det = +-a in every
    dot order and both cross models, u = v = .25 up to the rounding of 1 / a, distance about 1."""
    cs = []
    for name, word, hit in (("at", EPS_WORD, True), ("above", EPS_WORD + 1, True), ("below", EPS_WORD - 1, False)):
        a = f32_of(word)
        pos = [(0, 0, 0), (a, 0, 0), (0, 1, 0)]
        o = [(a / F32(4), .25, 1)]
        cs.append(Case(f"e1_back_mask_{name}", o, [DOWN], [Target(make_vertices(pos), [0, 1, 2])], 1, [hit]))
        cs.append(Case(f"e1_no_mask_{name}", o, [DOWN], [Target(make_vertices(pos), [0, 1, 2])], 0, [hit]))
        cs.append(Case(f"e1_front_mask_{name}", o, [DOWN], [Target(make_vertices(pos), [0, 2, 1])], 2, [hit]))
    return cs


# ============================================================================ E2
def e2_cases():
    big = [(0, 0, 0), (1000, 0, 0), (0, 1000, 0)]
    return [Case("e2_distance_is_maxvalue", [(.25, .25, R.FLT_MAX)], [DOWN], [R.kat_target()], 1, [False]),
            Case("e2_distance_one_ulp_below_maxvalue", [(.25, .25, MAX_BELOW)], [DOWN], [R.kat_target()], 1, [True]),
            Case("e2_distance_1e30", [(250, 250, 1e30)], [DOWN], [Target(make_vertices(big), [0, 1, 2])], 1, [True]),
            Case("e2_distance_overflows_to_inf", [(250, 250, 1e33)], [DOWN], [Target(make_vertices(big), [0, 1, 2])], 1, [False])]


E2_WORDS = {"e2_distance_is_maxvalue": 0x7f7fffff, "e2_distance_one_ulp_below_maxvalue": 0x7f7ffffe, "e2_distance_overflows_to_inf": 0x7f800000}


# ============================================================================ E3
def subnormal_twin_case(near_first):
    """Triangle A in z = 0, triangle B in z = -denorm_min, the ray from z = +denorm_min: distances 0x00000001 and 0x00000002.  The
    normals differ, so the record names its triangle twice."""
    kat = np.asarray(KAT_POS, dtype=F32)
    far = kat + np.array([0, 0, -DENORM_MIN], dtype=F32)
    pos = np.concatenate([kat, far]) if near_first else np.concatenate([far, kat])
    nrm = [(0, 0, 1)] * 3 + [(0, 1, 0)] * 3 if near_first else [(0, 1, 0)] * 3 + [(0, 0, 1)] * 3
    return Case("e3_subnormal_twins_near_first" if near_first else "e3_subnormal_twins_far_first", [(.25, .25, DENORM_MIN)], [DOWN],
                [Target(make_vertices(pos, nrm), np.arange(6))], 1, [True])


def e3_cases():
    return [Case("e3_distance_minus_denorm_min", [(.25, .25, -DENORM_MIN)], [DOWN], [R.kat_target()], 1, [False]),
            Case("e3_distance_plus_denorm_min", [(.25, .25, DENORM_MIN)], [DOWN], [R.kat_target()], 1, [True]),
            subnormal_twin_case(True), subnormal_twin_case(False)]


E3_WINNER = {"e3_distance_plus_denorm_min": 0, "e3_subnormal_twins_near_first": 0, "e3_subnormal_twins_far_first": 1}


# ============================================================================ E4
def e4_case(reverse=False):
    """Targets of E4_COUNTS triangles, each built as count_case(T, "last") builds it, the KAT triangle of target k moved to y + 10 k.
    Ray k runs down x = .25, y = 10 k + .25 and meets that triangle alone (the other triangles lie in x >= 3.8); ray 6 runs down
    y = -9.75 and meets nothing.  Target 1 has no triangle, so ray 1 misses everything too."""
    targets = []
    for k, T in enumerate(E4_COUNTS):
        tg = R.count_case(T, "last")[0].targets[0]
        if T:
            tg.vertices["position"][-3:] += np.array([0, 10 * k, 0], dtype=F32)
        targets.append(tg)
    o = [(.25, 10 * k + .25, 1) for k in range(len(E4_COUNTS))] + [(.25, -9.75, 1)]
    order = list(range(len(E4_COUNTS)))
    if reverse:
        order.reverse()
    expect = [r < len(E4_COUNTS) and order[t] == r and E4_COUNTS[r] > 0 for r in range(len(o)) for t in range(len(order))]
    return Case("e4_mixed_sizes_reversed" if reverse else "e4_mixed_sizes", o, [DOWN] * len(o), [targets[k] for k in order], 1, expect), order


# ============================================================================ E5
def e5_target(seed=41):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.5, 1.5, size=(70, 1, 3))
    p = (c + rng.uniform(-0.5, 0.5, size=(70, 3, 3))).astype(F32).reshape(-1, 3)
    return Target(make_vertices(p, rng.normal(size=(210, 3))), np.arange(210, dtype=np.uint16)), p.reshape(70, 3, 3).mean(axis=1)


def e5_chunk_case(n_rays):
    """n_rays rays from around one mesh of 70 random triangles at triangle centres chosen at random: every direction differs (asserted on
    the host), a good part hits.  expect is not stated ray by ray: the restatement decides, the host test bounds the hit count."""
    tg, centres = e5_target()
    rng = np.random.default_rng(43 + n_rays)
    o = rng.uniform(-6, 6, size=(n_rays, 3)).astype(F32)
    d = (centres[rng.integers(0, 70, n_rays)] - o + rng.normal(scale=0.02, size=(n_rays, 3))).astype(F32)
    return Case(f"e5_{n_rays}_rays", o, d, [tg], 0)


def e5_only_31_and_32_case():
    """64 rays against the KAT triangle: ray r starts at (.25, .25, 1) and points up and away in a direction of its own, but rays 31 and
    32 -- the last of the first chunk, the first of the second -- which point at the triangle from two different origins."""
    a = 2 * np.pi * np.arange(64) / 64
    o = np.tile(F32([.25, .25, 1]), (64, 1))
    d = np.stack([np.cos(a), np.sin(a), np.full(64, 0.5)], axis=1).astype(F32)
    o[31], d[31] = (.125, .5, 2), (0, 0, -1)
    o[32], d[32] = (.5, .125, 3), (0, 0, -3)
    return Case("e5_only_rays_31_and_32_hit", o, d, [R.kat_target()], 1, [r in (31, 32) for r in range(64)])


# ============================================================================ E6
def _stack(n, dz=-0.5):
    """n KAT triangles, target k in z = k dz"""
    return [Target(make_vertices(np.asarray(KAT_POS, dtype=F32) + F32([0, 0, k * dz])), [0, 1, 2]) for k in range(n)]


def e6_sequence():
    """[(case, nearest)] to be run IN THIS ORDER on a context of its own.  (a) 5 rays x 3 targets, all 15 pairs hit; (b) the same rays
    pointing up: 15 misses over the 15 key words (a) used; (c) 3 x 5 over the same 15 words, where pair (r, t) hits iff t <= r + 1
    -- key word r * 5 + t was pair (r', t') = divmod(., 3) of (a); (d) nearest over 5 x 3, all hit, then all miss."""
    xy = [(.1, .1), (.2, .1), (.1, .2), (.3, .3), (.25, .25)]
    o = [(x, y, 1) for x, y in xy]
    three, five = _stack(3), _stack(5)
    # (c): ray r starts between target r + 1 and target r + 2, looking UP with mask 0: it sees targets 0 .. r + 1
    oc = [(x, y, -0.5 * (r + 1) - 0.25) for r, (x, y) in enumerate(xy[:3])]
    return [(Case("e6a_all_pairs_hit", o, [DOWN] * 5, three, 1, [True] * 15), False),
            (Case("e6b_all_pairs_miss", o, [UP] * 5, three, 1, [False] * 15), False),
            (Case("e6c_other_n_targets", oc, [UP] * 3, five, 0, [t <= r + 1 for r in range(3) for t in range(5)]), False),
            (Case("e6d_nearest_all_hit", o, [DOWN] * 5, three, 1, [True] * 15), True),
            (Case("e6d_nearest_all_miss", o, [UP] * 5, three, 1, [False] * 15), True)]


# ============================================================================ E7
def e7_cases():
    """[(case, winning target per ray, distance word of ray 0's winner)]; mask 0 where a reversed winding must be seen."""
    plus, minus = R.kat_target(), R.kat_target(True)            # from (.25, .25, 0) downwards: +0.0 and -0.0
    away = Target(make_vertices(np.asarray(KAT_POS, dtype=F32) + F32([5, 0, 0])), [0, 1, 2])
    on = [(.25, .25, 0)]
    near = Target(make_vertices(np.asarray(KAT_POS, dtype=F32) + F32([2, 0, .5])), [0, 1, 2])
    return [(Case("e7_minus_zero_then_plus_zero", on, [DOWN], [minus, plus], 0, [True, True]), [0], 0x80000000),
            (Case("e7_plus_zero_then_minus_zero", on, [DOWN], [plus, minus], 0, [True, True]), [0], 0x00000000),
            (Case("e7_miss_then_two_that_tie", [(.25, .25, 1)], [DOWN], [away, R.kat_target(), R.kat_target()], 1, [False, True, True]), [1], 0x3f800000),
            # ray 0 meets targets 0 and 1 at distance 1 (target 0 wins, first of equals); ray 1 meets target 0 at 1 and target 2 at 0.5
            (Case("e7_winners_first_and_last", [(.25, .25, 1), (2.25, .25, 1)], [DOWN] * 2,
                  [Target(make_vertices(np.concatenate([np.asarray(KAT_POS, dtype=F32), np.asarray(KAT_POS, dtype=F32) + F32([2, 0, 0])])), np.arange(6)),
                   R.kat_target(), near], 1, [True, True, False, True, False, True]), [0, 2], 0x3f800000)]


# ============================================================================ E8
E8_VERTICES = 65536


def e8_case():
    """(the case on the full mesh, the same case on the mesh of the triangle's three vertices alone -- indices (2, 1, 0) -- for the
    reference, whose per-vertex transforms the other 65533 vertices do not enter).  The filler vertices are random triangles in
    x >= 3.8, so an index that lost its high bits names a triangle the ray misses."""
    rng = np.random.default_rng(47)
    pos = (rng.uniform([4, -3, -3], [9, 3, 3], size=(E8_VERTICES, 3))).astype(F32)
    nrm = rng.normal(size=(E8_VERTICES, 3)).astype(F32)
    pos[65535], pos[65534], pos[65533] = KAT_POS[0], KAT_POS[1], KAT_POS[2]
    o, d = [(.25, .25, 1)], [DOWN]
    full = Case("e8_indices_65535_65534_65533", o, d, [Target(make_vertices(pos, nrm), [65535, 65534, 65533])], 1, [True])
    small = Case("e8_reference", o, d, [Target(make_vertices(pos[65533:], nrm[65533:]), [2, 1, 0])], 1, [True])
    return full, small


# ============================================================================ lists
def numerics_cases():
    """E1 - E3: what runs under SWR_RAY_CROSS_FUSED and on the sensitivity builds as well"""
    return e1_cases() + e2_cases() + e3_cases()


def single_call_cases():
    """every case that is one call with a stated outcome per pair (E6 is a sequence, E8 has a reference case of its own)"""
    return numerics_cases() + [e4_case(False)[0], e4_case(True)[0], e5_only_31_and_32_case()] + [c for c, _, _ in e7_cases()]
