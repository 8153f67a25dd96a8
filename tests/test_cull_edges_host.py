"""The frustum-culler edge cases of tests/cull_edge_cases.py on the CPU: proof, with the oracle alone, that the families contain
what they are for.  These are conditions on the cases, not measurements of the backend (tests/test_gpu_cull_edges.py runs them).

  - the float32 restatement of CalculateBoundingSphere (cull_edge_cases.sphere_trace) equals the oracle bit for bit on every mesh
    in all six oracle builds; only then is it asked WHICH vertex each pass chose;
  - B1: every pass's choice sits at both ends of the index range, for every size;
  - B2: the tied candidates are distinct points at bit-equal squared distance, in the stated thread / wave / stride relation
    (thread of index i = (i - 1) % 1024 in pass 1, i % 1024 in passes 2 and 3), and swapping them changes the sphere's bits;
  - B3: the last outsider is the highest planted index, the on-radius vertices have dist == r, the 1-ULP vertex has dist = r + 1 ULP;
  - B4: the squared distances really are subnormal / +Inf in float32, the centre really carries -0.0;
  - B6: >= 8 meshes differ in bits between the default and the dotpw oracle, >= 2 of them by another chosen vertex; none under dpps;
  - F1 / F2: every case is outside exactly its plane, every scale row is the maximum somewhere and two rows tie exactly; every
    threshold flips between nextafter(r*, 0) and r* and stays put for 8 ULP either side, per oracle build and Transform flag;
    >= 10 % of the thresholds move under the Transform flag and >= 10 % between the default and the dotpw oracle, none under dpps;
  - batch: every threshold translation flips in the same way, both patterns keep and cull draws in all three blocks, and
    thresholds that differ between the flags (0,0) and (1,1) exist for the per-draw flag test."""
import numpy as np
import pytest

import cull_edge_cases as K
from oracle import binding as ob

F32 = np.float32


@pytest.fixture(scope="module")
def libs():
    ob.build()
    return {v: ob.load(variant=v) for v in K.VARIANTS}


ALL_SPHERE_CASES = [(f, c) for f, make in K.SPHERE_FAMILIES.items() for c in make()]


def test_oracle_builds_are_what_their_names_say(libs):
    for v, lib in libs.items():
        assert lib.oswr_dot_pairwise() == K.DOT_ORDER[v] and lib.oswr_numerics_fma() == int(v.startswith("fma"))


def test_restatement_equals_the_oracle_bit_for_bit_in_every_build(libs):
    names = [c.name for _, c in ALL_SPHERE_CASES]
    assert len(set(names)) == len(names)
    for _, c in ALL_SPHERE_CASES:
        for v, lib in libs.items():
            got, want = K.sphere_trace(c.vertices, K.DOT_ORDER[v])["sphere"], K.oracle_sphere(lib, c.vertices)
            assert K.same_words(got, want), (c.name, v, K.words(got), K.words(want))


def test_b1_sizes_put_every_choice_at_both_ends():
    cases = K.b1_sizes()
    assert {c.vertices.shape[0] for c in cases} == set(K.SIZES)
    for n in K.SIZES[3:]:
        traces = [K.sphere_trace(c.vertices) for c in cases if c.vertices.shape[0] == n]
        for c, t in zip([c for c in cases if c.vertices.shape[0] == n], traces):
            assert (t["i1"], t["i2"], t["last"]) == (c.note["i1"], c.note["i2"], c.note["last"]), c.name
            assert int((t["dist"] > t["r0"]).sum()) >= 1
        assert any(t["i1"] >= n - 2 for t in traces) and any(t["i1"] == 1 for t in traces)
        assert any(t["i2"] >= n - 2 for t in traces) and any(t["i2"] == 0 for t in traces)
        assert any(t["last"] >= n - 2 for t in traces) and any(t["last"] == 1 for t in traces)
        # a later outsider must beat earlier ones somewhere, or "first outsider" would pass too
        assert any(int((t["dist"] > t["r0"]).sum()) >= 2 for t in traces)


def _swapped(vertices, i, j):
    v = vertices.copy()
    v[[i, j]] = v[[j, i]]
    return v


def test_b2_ties_are_exact_distinct_and_placed_as_stated(libs):
    lib = libs[""]
    seen = set()
    for c in K.b2_ties():
        t = K.sphere_trace(c.vertices)
        for pass_no, tied in ((c.note["pass_no"], c.note["tied"]),) + (((1, c.note["also_pass1"]),) if "also_pass1" in c.note else ()):
            d = t["d1"] if pass_no == 1 else t["d2"]
            assert len(tied) >= 2 and len({K.bits(d[i]) for i in tied}) == 1, c.name                 # bit-equal distances
            assert len({tuple(c.vertices["position"][i]) for i in tied}) == len(tied), c.name         # distinct points
            assert d[tied[0]] == np.nanmax(d) and int((d == d[tied[0]]).sum()) == len(tied), c.name   # they are the maxima, and no other
            assert (t["i1"] if pass_no == 1 else t["i2"]) == min(tied), c.name                        # the lowest index wins
            lo, hi = sorted(tied)[:2]
            a, b = K.thread_of(lo, pass_no), K.thread_of(hi, pass_no)
            seen.add((pass_no, "higher_thread" if a > b else "same_thread" if a == b else "one_wave" if a // 64 == b // 64 else "two_waves"))
            # the winner's coordinates matter: with the two candidates exchanged the sphere has other bits
            assert not K.same_words(K.oracle_sphere(lib, c.vertices), K.oracle_sphere(lib, _swapped(c.vertices, lo, hi))), c.name
    assert seen == {(p, k) for p in (1, 2) for k in ("higher_thread", "same_thread", "one_wave", "two_waves")}
    for tag, (lo, hi) in K.TIE_PLACES.items():
        assert lo < hi < K.TIE_N
    lo, hi = K.TIE_PLACES["a_lower_index_in_higher_thread"]
    assert (K.thread_of(lo, 1), K.thread_of(hi, 1), K.thread_of(lo, 2), K.thread_of(hi, 2)) == (699, 5, 700, 6)
    lo, hi = K.TIE_PLACES["b_same_thread"]
    assert hi == lo + 1024


def test_b3_last_outsider_on_the_radius_and_one_ulp_outside(libs):
    kinds = set()
    for c in K.b3_last_outsider():
        t = K.sphere_trace(c.vertices)
        assert t["r0"] == F32(8.0), c.name
        outside = [int(i) for i in np.nonzero(t["dist"] > t["r0"])[0]]
        assert outside == c.note["outsiders"], c.name
        assert t["last"] == (max(outside) if outside else None), c.name
        if len(outside) >= 2:
            # over waves and strides, each with a distance of its own (so the sphere tells which one was taken), the last not in
            # the highest thread
            assert len({i // 64 for i in outside}) >= 3 and len({i // K.BLOCK for i in outside}) >= 2 or "one_ulp" in c.note, c.name
            assert len({K.bits(t["dist"][i]) for i in outside}) == len(outside), c.name
            if "one_ulp" not in c.note:
                assert max(outside) % K.BLOCK < max(i % K.BLOCK for i in outside), c.name
        for i in c.note.get("on_radius", ()):
            assert t["dist"][i] == t["r0"] and i > max(outside, default=-1), c.name
            kinds.add("on_radius")
        if "one_ulp" in c.note:
            assert K.bits(t["dist"][c.note["one_ulp"]]) == K.bits(t["r0"]) + 1 and t["last"] == c.note["one_ulp"], c.name
            kinds.add("one_ulp")
        kinds.add("nothing" if not outside else "some")
    assert kinds == {"on_radius", "one_ulp", "nothing", "some"}


def test_b4_reaches_subnormal_inf_and_negative_zero(libs):
    sub = inf = negz = ident = 0
    for c in K.b4_range():
        p = c.vertices["position"]
        t = K.sphere_trace(c.vertices)
        o = K.oracle_sphere(libs[""], c.vertices)
        if c.note.get("subnormal"):
            with np.errstate(under="ignore"):
                d = p[1] - p[0]; sq = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]          # the three-line float32 computation
            tiny = np.finfo(F32).tiny
            assert sq.dtype == F32 and 0 < sq < tiny, c.name
            assert 0 < t["d2"][t["i2"]] < tiny and o[3] > 0 and np.isfinite(o[3]), c.name     # the winning distance too; r survives
            sub += 1
        if c.note.get("inf"):
            with np.errstate(over="ignore"):
                d1 = t["d1"]
            assert int(np.isposinf(d1).sum()) >= 2 and np.isfinite(p).all(), c.name          # several candidates, finite coordinates
            assert (t["i1"], t["i2"]) == (c.note["i1"], c.note["i2"]), c.name
            assert t["i1"] == int(np.nonzero(np.isposinf(d1))[0][0]), c.name                  # the lowest index among them
            assert np.isposinf(o[3]), c.name
            inf += 1
        if "neg_zero" in c.note:
            for k in c.note["neg_zero"]:
                assert K.bits(o[k]) == 0x80000000, c.name
            negz += 1
        if c.note.get("identical"):
            assert len({tuple(q) for q in p}) == 1 and o[3] == 0 and K.same_words(o[:3], p[0]), c.name
            ident += 1
    assert sub >= 2 and inf >= 2 and negz >= 1 and ident >= 2


def test_b5_non_finite_vertices_are_where_they_should_be(libs):
    for c in K.b5_non_finite():
        p = c.vertices["position"]
        assert not np.isfinite(p).all(), c.name
        o = K.oracle_sphere(libs[""], c.vertices)
        if "nan_in_the_middle" in c.name:
            assert np.isfinite(p[0]).all() and np.isfinite(o).all() and o[3] > 0, c.name       # all three passes ignore it
        if "nan_at_vertex_0" in c.name:
            assert np.isnan(p[0][0]) and np.isnan(o[0]) and o[3] == 0, c.name
        if "inf_coordinate" in c.name:
            assert np.isinf(p).any() and not np.isnan(p).any() and np.isposinf(o[3]), c.name


def test_b6_is_sensitive_to_the_dot_order(libs):
    cases = K.b6_dot_order()
    assert cases[0].name == K.B6_NAMED and cases[0].vertices.shape[0] == 77
    differ = other = 0
    for c in cases:
        d, pw, dp = (K.oracle_sphere(libs[v], c.vertices) for v in ("", "dotpw", "dpps"))
        assert K.same_words(d, dp), c.name                       # the dpps order moves only the sign of a zero
        differ += not K.same_words(d, pw)
        a, b = K.sphere_trace(c.vertices, 0), K.sphere_trace(c.vertices, 2)
        moved = (a["i1"], a["i2"]) != (b["i1"], b["i2"])
        assert moved == bool(c.note.get("other_vertex", False)) or c.name == K.B6_NAMED, c.name
        other += moved
    assert differ == len(cases) >= 8 and other >= 2
    assert any(c.vertices.shape[0] > K.BLOCK for c in cases)      # the strided loop too


# ------------------------------------------------------------------------------------------------ frustum thresholds
def _flips(lib, case, r, flag):
    """Rejected for the 8 radii below r, accepted at r and the 8 above."""
    with K.oracle_flags(lib, flag):
        for k in range(-8, 9):
            if K.oracle_inside(lib, case.sphere(K.ulp_step(r, k)), case.model, case.view, case.proj) != (k >= 0):
                return False
    return True


def test_f1_cases_are_outside_exactly_their_plane_with_every_scale_row(libs):
    cases = K.f1_cases()
    assert 36 <= len(cases) <= 48
    per_plane = {p: 0 for p in K.PLANES}
    rows = set()
    for c in cases:
        assert K.outside_planes(c) == [c.plane], c.name
        per_plane[c.plane] += 1
        rs = K.row_scales(c.model)
        assert c.max_row == tuple(int(i) for i in np.nonzero(rs == rs.max())[0]), c.name
        rows.add(c.max_row)
        m = c.model.reshape(4, 4)
        assert np.count_nonzero(np.abs(m[:3, :3]) > 1e-3) >= 5 and np.abs(m[3, :3]).min() > 0, c.name      # rotated, translated
        assert len({round(float(s), 3) for s in rs}) >= 2, c.name                                           # non-uniform scale
    assert all(v >= 1 for v in per_plane.values()), per_plane
    assert {(0,), (1,), (2,)} <= rows and any(len(r) == 2 for r in rows), rows


def test_every_threshold_flips_and_stays_put(libs):
    """Per oracle build x Transform flag: the family's one number per case is a threshold of THAT configuration."""
    for v, lib in libs.items():
        for flag in (0, 1):
            for c in K.f1_cases():
                r = K.threshold_radius(lib, c, flag)
                assert r is not None and 0 < r < 1e3, (c.name, v, flag)
                assert _flips(lib, c, r, flag), (c.name, v, flag, r)
        assert tuple(x.value for x in _get_flags(lib)) == (lib.oswr_numerics_fma(),) * 2           # the default is back


def _get_flags(lib):
    import ctypes as C
    a, b = C.c_int(-1), C.c_int(-1)
    lib.oswr_get_transform_fma(C.byref(a), C.byref(b))
    return a, b


def test_thresholds_move_under_the_flag_and_the_dot_order_but_not_under_dpps(libs):
    cases = K.f1_cases()
    base = [K.threshold_radius(libs[""], c, 0) for c in cases]
    fused = [K.threshold_radius(libs[""], c, 1) for c in cases]
    dotpw = [K.threshold_radius(libs["dotpw"], c, 0) for c in cases]
    dpps = [K.threshold_radius(libs["dpps"], c, 0) for c in cases]
    flag_moved = sum(a != b for a, b in zip(base, fused))
    dot_moved = sum(a != b for a, b in zip(base, dotpw))
    print(f"thresholds moved: {flag_moved} of {len(cases)} under the Transform flag, {dot_moved} under dotpw")
    assert 10 * flag_moved >= len(cases) and 10 * dot_moved >= len(cases)
    assert base == dpps
    # the compile-time default of the fma build is the flag set: its default threshold is the product's (1, 1) threshold
    assert [K.threshold_radius(libs["fma"], c, None) for c in cases] == fused


def test_f3_degenerate_cases_decide_as_built(libs):
    cases = K.f3_degenerate()
    for c in cases:
        got = {K.oracle_inside(lib, c.sphere, c.model, c.view, c.proj) for lib in libs.values()}
        assert len(got) == 1, c.name
        if c.expect is not None:
            assert got == {c.expect}, c.name
    by = {c.name: c for c in cases}
    assert not by["f3_zero_model_origin_inside"].model.any() and not by["f3_zero_projection_nan_planes"].proj.any()
    assert np.isposinf(by["f3_inf_radius_far_outside"].sphere[3])
    # the same far-away centre with a large finite radius is rejected: it is the Inf that accepts
    c = by["f3_inf_radius_far_outside"]
    assert not K.oracle_inside(libs[""], np.array([*c.sphere[:3], 1.0], dtype=F32), c.model, c.view, c.proj)


# ------------------------------------------------------------------------------------------------ batch
def test_batch_thresholds_flip_and_both_patterns_fill_three_blocks(libs):
    lib = libs[""]
    meshes = K.batch_meshes()
    assert [i.size // 3 for _, i in meshes] == [1, 2, 3, 4, 5]
    spheres = [K.oracle_sphere(lib, v) for v, _ in meshes]
    assert len({K.words(s) for s in spheres}) == 5
    for complement in (False, True):
        draws = K.batch_pattern(lib, complement)
        assert len(draws) == K.BATCH_DRAWS == 2 * 64 + 2
        for d in draws:
            m = d.model.reshape(4, 4)
            for k in range(-8, 9):          # weakly monotone in the translation: accepted below t*, rejected from t* on
                t = K.ulp_step(m[3, 0], k - d.step)
                assert K.oracle_inside(lib, spheres[d.mesh], K.with_translation(m, t), K.BATCH_VIEW, K.BATCH_PROJ) == (k < 0)
        keep = [(not d.cull_request) or d.step < 0 for d in draws]
        for block in (slice(0, 64), slice(64, 128), slice(128, 130)):
            assert True in keep[block] and (False in keep[block] or block.start == 128)
        # requested-and-kept, requested-and-culled, not requested with a sphere outside, not requested with a sphere inside
        assert {(d.cull_request, d.step < 0) for d in draws} == {(True, True), (True, False), (False, True), (False, False)}
        kept_counts = {d.mesh + 1 for d in draws if d.step < 0}
        culled_counts = {d.mesh + 1 for d in draws if d.step >= 0}
        assert not kept_counts & culled_counts and kept_counts | culled_counts == {1, 2, 3, 4, 5}


def test_batch_has_thresholds_that_differ_between_the_flags(libs):
    assert len(K.flag_sensitive_batch_draws()) >= 2
