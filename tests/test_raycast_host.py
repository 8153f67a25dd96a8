"""The ray-query cases of tests/raycast_cases.py on the CPU: the restatement is what it claims, the cases are what they claim, and the
bindings agree with the header (no GPU here; tests/test_gpu_raycast.py runs the same cases on the device).

Host mutants of the restatement (test_host_mutants_turn_named_cases_red):
  `<=` for `<` in the tie            -> twins_T513_0_512, twins_T513_64_257, twins_T2_0_1 and both zero-twin cases name the HIGHER index
  `u >= 1` for `u > 1`               -> edges_inclusive loses the ray through the vertex (1, 0) (u = 1, v = 0)
  unsigned distance words, unmapped  -> zero_twins_minus_first: -0.0 (0x80000000) loses to +0.0 although it is first"""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

import raycast_cases as R
from oracle import binding as ob
from softwarerenderer_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def ref(oracle_lib):
    return lambda case, **kw: R.reference(oracle_lib, "", case, **kw)


def bits(x):
    return int(np.asarray(x, dtype=F32).reshape(1).view(np.uint32)[0])


def test_the_hand_kat(ref):
    r = ref(R.host_cases()[0])[0, 0]
    tg = R.kat_target()
    alive, dist, u, v, d, _ = R.intersect((.25, .25, 1), (0, 0, -2), tg.vertices["position"], tg.indices, 1, 0, False)
    assert alive[0] and (float(u[0]), float(v[0]), float(dist[0])) == (0.25, 0.25, 1.0) and d.tolist() == [0.0, 0.0, -1.0]
    assert (int(r["found"]), int(r["target"]), int(r["triangle"]), float(r["distance"])) == (1, 0, 0, 1.0)
    assert r["point"].tolist() == [0.25, 0.25, 0.0] and r["normal"].tolist() == [0.0, 0.0, 1.0]


@pytest.mark.parametrize("fused", [False, True], ids=["cross_rounded", "cross_fused"])
def test_every_host_case_has_its_stated_outcome(ref, fused):
    for c in R.host_cases():
        got = ref(c, fused=fused)
        assert [bool(x) for x in got["found"].reshape(-1)] == list(c.expect), c.name
        miss = got[got["found"] == 0]
        assert (miss["distance"] == R.FLT_MAX).all() and (miss["triangle"] == -1).all() and not miss["point"].any() and not miss["normal"].any()


def test_signed_zero_distances_on_the_plane(ref):
    by = {c.name: c for c in R.host_cases()}
    assert bits(ref(by["origin_on_plane_front"])[0, 0]["distance"]) == 0x00000000
    assert bits(ref(by["origin_on_plane_behind_mask0"])[0, 0]["distance"]) == 0x80000000


def test_counts_and_ties_name_the_triangle_they_claim(ref):
    for T in R.COUNTS:
        for where in ("last", "first"):
            c, hit = R.count_case(T, where)
            r = ref(c)[0, 0]
            assert bool(r["found"]) == (T > 0) and int(r["triangle"]) == (hit if T else -1), c.name
    want = {"twins_T513_0_512": 0, "twins_T513_64_257": 64, "twins_T2_0_1": 0, "zero_twins_plus_first": 0, "zero_twins_minus_first": 0}
    for c in R.tie_cases():
        r = ref(c)[0, 0]
        assert int(r["triangle"]) == want[c.name], c.name
    # the winner's own word: +0.0 when the front winding is first, -0.0 when the reversed one is
    assert bits(ref(R.zero_twin_case(False))[0, 0]["distance"]) == 0 and bits(ref(R.zero_twin_case(True))[0, 0]["distance"]) == 0x80000000
    # the twins differ in their normals, so the index decides the answer
    assert ref(R.twin_case(513, 0, 512))[0, 0]["normal"].tolist() == [0.0, 0.0, 1.0]


def test_host_mutants_turn_named_cases_red(ref):
    red = {}
    for mutant, kw in (("tie_le", {"rule": "le"}), ("u_ge_1", {"u_sense": ">="}), ("rawbits", {"rule": "rawbits"})):
        red[mutant] = [c.name for c in R.host_cases() + R.tie_cases() if not R.same_records(ref(c, **kw), ref(c))]
    print(red)
    assert red["tie_le"] == ["twins_T513_0_512", "twins_T513_64_257", "twins_T2_0_1", "zero_twins_plus_first", "zero_twins_minus_first"]
    assert red["u_ge_1"] == ["edges_inclusive"]
    assert red["rawbits"] == ["zero_twins_minus_first"]


def test_shape_nearest_and_dust2_cases_are_not_vacuous(ref):
    for n_rays in (1, 2, 65):
        for n_targets in (1, 3):
            got = ref(R.shape_case(n_rays, n_targets))
            assert got.shape == (n_rays, n_targets)
            if n_rays == 65:
                assert 0 < int(got["found"].sum()) < got.size
                if n_targets == 3:
                    assert got[:, 1]["found"].any() and np.isnan(got[:, 1]["normal"][got[:, 1]["found"] == 1]).all()    # the zero normal matrix
    got = ref(R.nearest_tie_case())
    fold = [R.fold_nearest(row) for row in got]
    assert [int(f["target"]) for f in fold] == [0, 2, -1] and [int(f["found"]) for f in fold] == [1, 1, 0]
    assert got[0, 0]["distance"] == got[0, 1]["distance"] and got[1, 2]["distance"] < got[1, 0]["distance"]


def test_dust2_rays_hit_the_map(ref):
    c = R.dust2_case()
    assert len(c.targets) == 11 and sum(t.indices.shape[0] // 3 for t in c.targets) == 9061 and c.origins.shape[0] == 42
    got = ref(c)
    hits, rays = int(got["found"].sum()), int(got["found"].any(axis=1).sum())
    print(f"dust2: {hits} of {got.size} pairs hit, {rays} of 42 rays hit something")
    assert hits >= 10 and rays >= 10


@pytest.mark.parametrize("variant", list(R.DOT_ORDER))
def test_vectorised_dot3_equals_the_oracle_library(variant):
    lib = ob.load(variant=variant)
    rng = np.random.default_rng(3)
    a = rng.normal(size=(3000, 3)).astype(F32) * F32(10) ** rng.integers(-3, 4, size=(3000, 1)).astype(F32)
    b = rng.normal(size=(3000, 3)).astype(F32)
    a[:8] = F32(-0.0); b[:8] = F32(1.0)                                       # the dpps order differs from the sequential one only here
    got = R.dot3v(a, b, R.DOT_ORDER[variant])
    want = np.array([R.oracle_dot3(lib, a[i], b[i]) for i in range(a.shape[0])], dtype=F32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_fma32_is_one_rounding():
    rng = np.random.default_rng(4)
    a, b = rng.normal(size=4000).astype(F32), rng.normal(size=4000).astype(F32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.normal(scale=1e-7, size=4000))).astype(F32)    # heavy cancellation
    c[:1000] = rng.normal(size=1000).astype(F32)
    # sums that sit next to a float32 midpoint in float64: where double rounding would show
    a[1000:1200] = F32(1.0) + F32(2.0) ** -23; b[1000:1200] = F32(1.0) + F32(2.0) ** -23
    c[1000:1200] = (F32(2.0) ** rng.integers(-30, 2, size=200).astype(F32)).astype(F32)
    got = R.fma32(a, b, c)

    def exact(x, y, z):
        want = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        g = F32(float(want))
        cands = sorted({float(g), float(np.nextafter(g, F32(np.inf))), float(np.nextafter(g, F32(-np.inf)))}, key=lambda k: abs(Fraction(k) - want))
        if abs(Fraction(cands[0]) - want) == abs(Fraction(cands[1]) - want):                      # a tie: to even
            return [k for k in cands[:2] if (bits(k) & 1) == 0][0]
        return cands[0]
    for i in range(a.shape[0]):
        assert float(got[i]) == exact(a[i], b[i], c[i]), (i, a[i], b[i], c[i])
    x, y = rng.normal(size=(500, 3)).astype(F32), rng.normal(size=(500, 3)).astype(F32)
    assert (R.cross3v(x, y, True) != R.cross3v(x, y, False)).any()           # the two Cross models are distinguishable


def test_bindings_match_the_header():
    """Fails without the feature: the structs, the two exports and the built library's symbols."""
    assert (ctypes.sizeof(_native.Ray), ctypes.sizeof(_native.RayTarget), ctypes.sizeof(_native.RayHit)) == (24, 136, 40)
    hdr = open(os.path.join(ROOT, "include", "swr.h")).read()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ("swr_raycast", "swr_raycast_nearest"):
        assert name in _native.EXPORTS and f" {name}(" in hdr and hasattr(lib, name)
    assert _native.SWR_RAY_CROSS_FUSED == 0x100 and "SWR_RAY_CROSS_FUSED = 0x100" in hdr
    from softwarerenderer_amd import Physics, RaycastFaceMask
    assert int(RaycastFaceMask.IgnoreBackfaces) == 1 and int(RaycastFaceMask.IgnoreFrontfaces) == 2 and callable(Physics.Raycast)


def test_invert_for_the_normal_matrix():
    from softwarerenderer_amd import hostmath as hm
    m = R._model(np.random.default_rng(1))
    inv = hm.invert(m)
    assert inv.dtype == F32 and np.allclose(m.astype(np.float64) @ inv.astype(np.float64), np.eye(4), atol=1e-5)
    assert np.array_equal(hm.normal_matrix(m), inv.T)
    assert hm.invert(np.zeros((4, 4))) is None and hm.invert(np.full((4, 4), np.nan)) is None
    s = hm.identity(); s[1, 1] = 0
    assert hm.invert(s) is None
