"""swr_pose_set_sample / swr_mesh_skin_batch at their branches and numeric edges: the cases of tests/animation_edge_cases.py on the
device against the numpy float32 restatement of tests/animation_cases.py, every word of every palette, with no tolerance
(animation_cases.same_words).  same_words equates any NaN with any NaN, so every case also states, as a literal, which
(instance, joint) pairs hold a NaN, and the device's set must be that one.  tests/test_animation_edges_host.py shows on the CPU that
each case is on the branch it is named for; profiles/r26_animation_edges.md holds the device mutants these cases were run against.

K1 - Q3 (the key search, the divisor, dot at zero, quaternion lengths at the ends of float32) also run under the six library variants
and under all four Transform flags."""
import os

import numpy as np
import pytest

import animation_cases as A
import animation_edge_cases as E
from softwarerenderer_amd import Device, PoseSet
from test_gpu_animation import (PKG, VARIANTS, _assert_palettes, _batch_against_single_calls, _gpu_palettes, _requests, _sampled_set, _upload,
                                crowd_palettes)  # noqa: F401  (crowd_palettes: the module-scoped fixture of the batched skin)

pytestmark = pytest.mark.gpu
F32 = np.float32


def nan_set(pal):
    return {(i, j) for i in range(pal.shape[0]) for j in range(pal.shape[1]) if np.isnan(pal[i, j]).any()}


def held(got, want, nan, what):
    """Word for word, and NaN in exactly the stated (instance, joint) pairs."""
    _assert_palettes(got, want, what)
    assert nan_set(got) == set(nan), f"{what}: NaN in {sorted(nan_set(got))}, stated {sorted(nan)}"


@pytest.fixture(scope="module")
def numerics():
    """K1 - Q3 with the restatement's palettes, computed once."""
    return [(c, A.palettes_of(c.sk, c.clips, c.requests)) for c in E.numerics_cases()]


def run(dev, case, want, what=""):
    got = _gpu_palettes(dev, case.sk, case.clips, case.requests)
    held(got, want, case.nan, f"{case.name} {what}")
    return got


# ------------------------------------------------------------------------------------------------ K1 - Q3
@pytest.mark.parametrize("k", range(len(E.numerics_cases())), ids=[c.name for c in E.numerics_cases()])
def test_k1_to_q3(device, numerics, k):
    case, want = numerics[k]
    got = run(device, case, want)
    if case.name.startswith("q2_") and case.on[1] == "zero":
        # ls = +Inf: inv = 0, the quaternion is (0, 0, 0, 0) and not NaN; the node's rotation block is exactly diag(s)
        sk = case.sk
        local = np.diag(np.append(sk.rest_s[1], F32(1.0))).astype(F32)
        local[3, :3] = sk.rest_t[1]
        by_hand = A.mul(sk.inverse_bind[1], A.mul(local, sk.rest_local[0]))
        assert not A.same_words(got[0, 1], by_hand).size
    if case.name.startswith("q2_") and case.on[1] == "nan":
        assert np.isnan(got[0, 1][:3, :3]).all()


@pytest.mark.parametrize("lib", VARIANTS)
def test_k1_to_q3_under_every_library_variant(numerics, lib):
    if not os.path.exists(os.path.join(PKG, lib)):
        pytest.fail(f"{lib} is missing: __graft_entry__.build() makes it (make -C softwarerenderer_amd/csrc variants)")
    dev = Device(0, lib=lib)
    try:
        for case, want in numerics:
            run(dev, case, want, lib)
    finally:
        dev.close()


@pytest.mark.parametrize("fused_t,fused_tn", [(False, False), (True, False), (False, True), (True, True)])
def test_k1_to_q3_under_all_four_transform_flags(device, numerics, fused_t, fused_tn):
    was = device.transform_fma()
    try:
        device.set_transform_fma(fused_t, fused_tn)
        for case, want in numerics:
            run(device, case, want, f"flags {fused_t} {fused_tn}")
    finally:
        device.set_transform_fma(*was)


# ------------------------------------------------------------------------------------------------ H1
@pytest.mark.parametrize("name", list(E.H1_SHAPES))
def test_h1_wide_levels_with_every_node_a_joint(device, name):
    case = E.h1_case(name)
    run(device, case, A.palettes_of(case.sk, case.clips, case.requests))


# ------------------------------------------------------------------------------------------------ H2 - H5
def play(dev, script):
    """The script's host calls in order; every read against the restatement's state of that set at that point."""
    want = script.expected_reads()
    n_joints = next(iter(script.skeletons.values()))[0].n_joints
    sks = {k: _upload(dev, sk, clips) for k, (sk, clips) in script.skeletons.items()}
    sets = {k: PoseSet(dev, n, n_joints) for k, n in script.sets.items()}
    reads = 0
    try:
        for op in script.ops:
            if op[0] == "sample":
                sets[op[1]].Sample(sks[op[2]], _requests(op[3]))
            elif op[0] == "add_clip":
                sks[op[1]].AddClip(op[2])
            else:
                held(sets[op[1]].Read(), want[reads], (), f"{script.name}: read {reads} (set {op[1]})")
                reads += 1
        assert reads == len(want) > 0
    finally:
        for s in sets.values():
            s.Dispose()
        for g in sks.values():
            g.Dispose()


@pytest.mark.parametrize("script", E.scripts(), ids=lambda s: s.name)
def test_h2_to_h5_the_host_sequencing(script):
    """On a context of its own, so that the palette slots start from none."""
    dev = Device(0)
    try:
        play(dev, script)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ B1
def test_b1_whole_blocks_and_empty_jobs_in_one_table(device, crowd_palettes):
    g, ps = _sampled_set(device, crowd_palettes)
    try:
        _batch_against_single_calls(device, ps, E.B1_COUNTS, (0, 1, 2, 3, 4, 5))
    finally:
        ps.Dispose(); g.Dispose()


def test_b1_three_hundred_jobs_of_one_vertex(device, crowd_palettes):
    g, ps = _sampled_set(device, crowd_palettes)
    try:
        _batch_against_single_calls(device, ps, (1,) * E.B1_JOBS, [k % 7 for k in range(E.B1_JOBS)])
    finally:
        ps.Dispose(); g.Dispose()
