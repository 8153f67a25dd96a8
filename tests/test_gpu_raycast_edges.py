"""swr_raycast / swr_raycast_nearest at their branches: the cases of tests/raycast_edge_cases.py (E1 - E8) on the device against the
restatement of tests/raycast_cases.py, every pair of every case, with no tolerance -- integers as integers, floats as 32-bit words
(test_gpu_raycast.check / raycast_cases.same_records); where a case has several targets, swr_raycast_nearest against fold_nearest.
tests/test_raycast_edges_host.py shows on the CPU that each case is on the branch it is named for; profiles/r25_raycast_edges.md
holds the device mutants these cases were run against and what each turned red.

E1 - E3 (det at +-1e-8f, distances at float.MaxValue / +Inf / +-denorm_min) also run under SWR_RAY_CROSS_FUSED, under both
Transform flags and on the five sensitivity builds."""
import numpy as np
import pytest

import raycast_cases as R
import raycast_edge_cases as E
from softwarerenderer_amd import Device
from softwarerenderer_amd.rasterizer import Physics
from test_gpu_raycast import MODES, Uploaded, check, mode  # noqa: F401  (mode: the module-scoped fixture of the sensitivity builds)

pytestmark = pytest.mark.gpu


def found_of(got):
    return [bool(x) for x in got["found"].reshape(-1)]


def run(dev, olib, variant, case, **kw):
    got, want = check(dev, olib, variant, case, **kw)
    assert found_of(got) == list(case.expect), f"{case.name}: found {found_of(got)}"
    return got


# ------------------------------------------------------------------------------------------------ E1 - E3
@pytest.mark.parametrize("case", E.e1_cases(), ids=lambda c: c.name)
def test_e1_det_at_the_threshold(device, oracle_lib, case):
    run(device, oracle_lib, "", case)


@pytest.mark.parametrize("case", E.e2_cases(), ids=lambda c: c.name)
def test_e2_the_upper_limit_of_the_key(device, oracle_lib, case):
    got = run(device, oracle_lib, "", case)
    if case.name == "e2_distance_one_ulp_below_maxvalue":
        assert E.word_of(got[0, 0]["distance"]) == 0x7f7ffffe
    elif not case.expect[0]:
        assert E.word_of(got[0, 0]["distance"]) == 0x7f7fffff and int(got[0, 0]["triangle"]) == -1      # the miss record, not +Inf


@pytest.mark.parametrize("case", E.e3_cases(), ids=lambda c: c.name)
def test_e3_subnormal_distances(device, oracle_lib, case):
    got = run(device, oracle_lib, "", case)
    if case.expect[0]:
        assert E.word_of(got[0, 0]["distance"]) == 0x00000001 and int(got[0, 0]["triangle"]) == E.E3_WINNER[case.name]


@pytest.mark.parametrize("fused", [False, True], ids=["cross_rounded", "cross_fused"])
@pytest.mark.parametrize("flags", [(0, 0), (1, 1)], ids=["t0n0", "t1n1"])
def test_e1_to_e3_on_the_product_build(device, oracle_lib, flags, fused):
    default = device.transform_fma()
    try:
        device.set_transform_fma(*flags)
        for case in E.numerics_cases():
            run(device, oracle_lib, "", case, fused=fused, flag=flags[0], what=f"product, flags {flags}, fused {fused}")
    finally:
        device.set_transform_fma(*default)


@pytest.mark.parametrize("fused", [False, True], ids=["cross_rounded", "cross_fused"])
def test_e1_to_e3_on_a_sensitivity_build(mode, fused):
    dev, olib, variant = mode
    for case in E.numerics_cases():
        run(dev, olib, variant, case, fused=fused, what=variant)


# ------------------------------------------------------------------------------------------------ E4, E5
@pytest.mark.parametrize("reverse", [False, True], ids=["as_listed", "reversed"])
def test_e4_targets_of_mixed_sizes(device, oracle_lib, reverse):
    case, order = E.e4_case(reverse)
    got = run(device, oracle_lib, "", case)
    for r in range(got.shape[0]):
        for t in range(got.shape[1]):
            want = E.E4_COUNTS[order[t]] - 1 if case.expect[r * got.shape[1] + t] else -1
            assert int(got[r, t]["triangle"]) == want, (r, t)


@pytest.mark.parametrize("n_rays", E.E5_RAYS)
def test_e5_ray_chunks(device, oracle_lib, n_rays):
    got, want = check(device, oracle_lib, "", E.e5_chunk_case(n_rays))
    assert got.shape == (n_rays, 1) and 0 < int(got["found"].sum()) < n_rays


def test_e5_only_the_rays_either_side_of_a_chunk_border_hit(device, oracle_lib):
    got = run(device, oracle_lib, "", E.e5_only_31_and_32_case())
    assert np.flatnonzero(got["found"].reshape(-1)).tolist() == [31, 32]


# ------------------------------------------------------------------------------------------------ E6
def test_e6_the_keys_between_calls(oracle_lib):
    """One context of its own, the calls in sequence over the same key words: every call against the reference.  A key that
    k_ray_finish did not put back shows in the next call as a hit nobody made (b), in another pair (c), or in the fold (d)."""
    dev = Device(0)
    try:
        for case, nearest in E.e6_sequence():
            want = R.reference(oracle_lib, "", case)
            assert found_of(want) == list(case.expect), case.name
            with Uploaded(dev, case) as targets:
                if nearest:
                    got = Physics.RaycastNearest(case.origins, case.directions, targets, case.mask)
                    fold = [R.fold_nearest(row) for row in want]
                    bad = [f"ray {r}: got {R.show(got[r])} want {R.show(fold[r])}" for r in range(len(fold)) if not R.same_records(got[r], fold[r])]
                else:
                    got = Physics.RaycastBatch(case.origins, case.directions, targets, case.mask)
                    assert got.shape == want.shape, case.name
                    bad = [f"ray {r} target {t}: got {R.show(got[r, t])} want {R.show(want[r, t])}"
                           for r in range(want.shape[0]) for t in range(want.shape[1]) if not R.same_records(got[r, t], want[r, t])]
            assert not bad, f"{case.name}: {len(bad)} records differ:\n" + "\n".join(bad[:8])
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ E7
@pytest.mark.parametrize("entry", E.e7_cases(), ids=lambda e: e[0].name)
def test_e7_the_fold_over_targets(device, oracle_lib, entry):
    case, winners, word = entry
    run(device, oracle_lib, "", case)                                   # (pairs and nearest against the reference and its fold)
    with Uploaded(device, case) as targets:
        near = Physics.RaycastNearest(case.origins, case.directions, targets, case.mask)
    assert [int(x) for x in near["target"]] == winners and E.word_of(near[0]["distance"]) == word


# ------------------------------------------------------------------------------------------------ E8
def test_e8_the_last_index_of_a_full_mesh(device, oracle_lib):
    """swr_mesh_create takes 65536 vertices: the triangle (65535, 65534, 65533) of such a mesh against the reference of the same
    three vertices (no other vertex enters it)."""
    full, small = E.e8_case()
    want = R.reference(oracle_lib, "", small)
    with Uploaded(device, full) as targets:
        got = Physics.RaycastBatch(full.origins, full.directions, targets, full.mask)
        near = Physics.RaycastNearest(full.origins, full.directions, targets, full.mask)
    assert int(want[0, 0]["found"]) == 1
    assert R.same_records(got, want), f"got {R.show(got[0, 0])}\nwant {R.show(want[0, 0])}"
    assert R.same_records(near, want[0])
