"""The user vertex contract on the GPU, field by field (swr_vs_in, swr_vs_env, swr_vs_out of csrc/swr_program.hip.h), and the
64-vertex LDS slabs of k_vertex / k_vertex_user.

Every test compiles a vertex probe of tests/vertex_probe_cases.py with a fragment probe of tests/program_probe_cases.py, lets the
pair write contract scalars, raw, into the frame and compares 32-bit words with fs_in_reference fed by the vertex probe's numpy
restatement -- which tests/test_vertex_probe_host.py holds to the oracle.  No tolerance; a NaN word is matched by any NaN.

What tests/test_gpu_vertex_program.py cannot see and this file does: a different value in every one of the sixteen output scalars
(the o2 / o3 / vnorm packing, the clipper's own lerp of normal and data4.w), every scalar of swr_vs_env by index, the per-draw
constants of the vertex stage beside the per-identity constants of the fragment stage past the 64-identity cap, vertex counts one
below, at and one above the wave and the block size in both vertex kernels, and the helpers at a zero, a huge and a denormal
vector."""
import os

import numpy as np
import pytest

import program_probe_cases as PC
import vertex_probe_cases as VC
from softwarerenderer_amd import Device, _native
from softwarerenderer_amd.rasterizer import Program
from test_gpu_program_probe import assert_words, render
from util import assert_frame_parity, render_oracle

pytestmark = pytest.mark.gpu
F32 = np.float32


def fragment_text(name):
    return PC.PROBE_ALL if name == "all" else PC.CONSTANTS3 if name == "constants3" else PC.NARROW[int(name[6:])]


class Compiled(dict):
    """(vertex probe, fragment probe) -> program id: every pair of texts is compiled once, when a test first asks for it."""

    def __init__(self, dev):
        super().__init__()
        self.dev = dev

    def __missing__(self, key):
        self[key] = self.dev.compile_program(fragment_text(key[1]), vertex_source=VC.VERTEX_TEXTS[key[0]])
        return self[key]

    def destroy(self):
        for pid in self.values():
            self.dev.destroy_program(pid)


@pytest.fixture(scope="module")
def programs(device):
    ids = Compiled(device)
    yield ids
    ids.destroy()


_expected = {}


def expected(scene, stage, flags=0, fused=False):
    """(planes, count) of a scene under a vertex probe, computed once."""
    key = (id(scene), stage, flags, fused)
    if key not in _expected:
        _expected[key] = (scene, *VC.expected(scene, stage, flags, fused))
    return _expected[key][1:]


def check(dev, programs, scene, stage, groups, what, flags=0, fused=False, form="wide", after_recording=None):
    """Render `scene` under (vertex probe `stage`, fragment group g) for every g of `groups`; each frame equals the reference.
    A scene whose draws carry constants of their own keeps them but for PROBE_ALL's selector (the reference reads the draws as
    they are rendered: constants[63] is itself an env scalar)."""
    own = hasattr(scene.draws[0], "constants")
    for g in groups:
        names = PC.group_names(g)
        s = VC.with_selectors(scene, None, g) if own else PC.with_constants(scene, PC.selector_constants(g))
        planes, count = expected(s if own else scene, stage, flags, fused)
        covered = int((count > 0).sum())
        assert count.max() == 1 and covered > 0
        c, _, st = render(dev, s, programs[(stage, "all" if form == "wide" else f"narrow{g}")], after_recording=after_recording)
        assert_words(c, PC.expected_colour(s, names, planes, count), f"{what}/{form}/{'+'.join(names)}")
        assert st["fragments_written"] == covered, (what, form, names, st["fragments_written"], covered)


def flags_of(dev):
    return VC.nm_flags(*dev.transform_fma())


NARROW_GROUPS = [g for g in PC.FS_IN_GROUPS if set(PC.group_names(g)) & {"data4.x", "data4.w", "normal.x", "normal.z"}]


# ---- 1. ROUTE: a different value in every output scalar, every swr_fs_in scalar read back
@pytest.mark.parametrize("name", ["cells", "clipped"])
def test_route_every_fs_in_scalar_equals_the_reference_word_for_word(device, programs, name):
    scene = {"cells": VC.cells, "clipped": VC.clipped}[name]()
    check(device, programs, scene, "route", PC.FS_IN_GROUPS, f"route/{name}", flags_of(device))
    check(device, programs, scene, "route", NARROW_GROUPS, f"route/{name}", flags_of(device), form="narrow")


def test_route_on_the_fma_build_with_the_clippers_lerp_fused():
    lib = "libswr_hip_fma.so"
    if not os.path.exists(os.path.join(os.path.dirname(_native.LIB_PATH), lib)):
        pytest.fail(f"{lib} is missing: __graft_entry__.build() makes it")
    dev = Device(0, lib=lib)
    ids = Compiled(dev)
    try:
        assert dev.numerics_mode()[0] == 1
        check(dev, ids, VC.clipped(), "route", PC.FS_IN_GROUPS, "route/fma/clipped", flags_of(dev), fused=True)
    finally:
        ids.destroy()
        dev.close()


# ---- 2. ENV_ALL: every scalar of swr_vs_env
@pytest.mark.parametrize("tr,tn", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_every_env_scalar_is_what_the_draw_was_recorded_with(device, programs, tr, tn):
    default = device.transform_fma()
    device.set_transform_fma(tr, tn)
    try:
        flags = VC.nm_flags(tr, tn)
        assert flags_of(device) == flags
        pid = programs[("env_all", "all")]
        for k in range(VC.N_ENV_SELECTORS):
            s = VC.with_selectors(VC.env_scene(), k, 0)
            # constants set after the draws were recorded change nothing
            check(device, programs, s, "env_all", VC.ENV_FRAGMENT_GROUPS, f"env/t{tr}n{tn}/selector {k}", flags,
                  after_recording=lambda: device.set_program_constants(pid, np.full(64, -7.0, dtype=F32)))
        # the reference's planes ARE the recorded values where a vertex is a sample (weights exactly 1, 0, 0): draw 0 lies on the lattice
        s = VC.with_selectors(VC.env_scene(), VC.N_ENV_SELECTORS - 1, 0)
        planes, count = expected(s, "env_all", flags)
        slot, e = VC.env_entries(VC.N_ENV_SELECTORS - 1)[-1]
        assert VC.ENV_TABLE[e][0] == "nm_flags" and F32(flags) in planes[slot][count > 0]
    finally:
        device.set_transform_fma(*default)


def test_an_unknown_env_selector_leaves_the_outputs_zero(device, programs):
    s = VC.with_selectors(VC.env_scene(), VC.N_ENV_SELECTORS, 0)
    planes, count = expected(s, "env_all", flags_of(device))
    assert all((planes[n][count > 0] == 0).all() for n in VC.ENV_SLOTS)
    check(device, programs, s, "env_all", VC.ENV_FRAGMENT_GROUPS, "env/unknown selector", flags_of(device))


@pytest.mark.parametrize("block", list(VC.ENV_NARROW_SELECTORS))
def test_narrow_env_texts_give_the_words_of_env_all(device, programs, block):
    """A text that reads one block of the env and nothing else: the kernel loads only that."""
    s = VC.with_selectors(VC.env_scene(), VC.ENV_NARROW_SELECTORS[block], 0)
    check(device, programs, s, f"env_narrow_{block}", VC.ENV_FRAGMENT_GROUPS, f"env/narrow/{block}", flags_of(device))


# ---- 3. many_draws: per-draw constants in the vertex stage, per-identity constants in the fragment stage, past the cap
@pytest.mark.parametrize("mode", [0, 1])
def test_seventy_draws_each_see_their_own_constants_matrix_and_uniforms(device, programs, mode):
    s = VC.many_draws()
    want, count = PC.expected_flat(s, lambda t: s.draws[t.draw].constants[:3], tris=PC.probe_tris(s, VC.stage_of("many")))
    device.set_pipelining(mode)
    try:
        check(device, programs, s, "many", VC.MANY_FRAGMENT_GROUPS, f"many/pipelining {mode}", flags_of(device), form="narrow")
        # ... and the fragment half of the same batch reads the constants of its fragment identity
        c, _, st = render(device, s, programs[("many", "constants3")])
        assert_words(c, want, f"many/constants3/pipelining {mode}")
        assert st["fragments_written"] == int(count.sum())
    finally:
        device.set_pipelining(1)


# ---- 4. slabs: vertex counts around the wave and the block size, in both vertex kernels
def test_slabs_through_the_user_vertex_kernel(device, programs):
    check(device, programs, VC.slabs(), "route", PC.FS_IN_GROUPS, "slabs", flags_of(device))


@pytest.mark.parametrize("program", [Program.DebugVaryings, Program.Gouraud])
def test_slabs_through_the_builtin_vertex_kernel_equal_the_oracle(device, program):
    s = VC.with_program(VC.slabs(), program)
    c, z, st = render(device, s)
    _, count = expected(VC.slabs(), "route", 0)
    assert st["fragments_written"] == int((count > 0).sum())
    rc, rd, _ = render_oracle(s)
    assert_frame_parity(c, z, rc, rd, color_ulp=1, what=f"slabs/{program.name}")


# ---- 5. ZEROS and HELPERS
def test_a_vertex_program_that_writes_the_clip_position_only_leaves_zeros(device, programs):
    scene = VC.cells()
    planes, count = expected(scene, "zeros", flags_of(device))
    for name, _ in PC.FS_IN[4:13] + PC.FS_IN[18:25]:
        assert (planes[name][count > 0] == 0).all(), name                # (a zero of either sign: 0 times a weight of -0)
    check(device, programs, scene, "zeros", PC.FS_IN_GROUPS, "zeros", flags_of(device))


@pytest.mark.parametrize("tr,tn", [(0, 0), (1, 1)])
def test_helpers_at_zero_huge_and_denormal_vectors(device, programs, tr, tn):
    default = device.transform_fma()
    device.set_transform_fma(tr, tn)
    try:
        scene = VC.helpers_scene()
        planes, count = expected(scene, "helpers", VC.nm_flags(tr, tn))
        cov = planes["data4.x"][count > 0]
        assert np.isnan(cov).any() and (cov == 0).any() and np.isfinite(cov).any()
        check(device, programs, scene, "helpers", PC.FS_IN_GROUPS, f"helpers/t{tr}n{tn}", VC.nm_flags(tr, tn))
    finally:
        device.set_transform_fma(*default)
