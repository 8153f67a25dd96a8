"""swr_character_update at its branches: the cases of tests/character_edge_cases.py against the restatement of
tests/character_cases.py, with the bar of tests/test_gpu_character.py -- after EVERY step every field of the state and of the trace,
integers as integers, floats as 32-bit words, a NaN word of the reference a NaN word here; no tolerance anywhere.
tests/test_character_edges_host.py asserts on the CPU that every case is on the branch it is named for.

  C1  dead CheckPlane rays: plane_ray's `!(dot < 0.0001f)`, k_char_begin's mask, the MASKED skip of k_char_cast, the `!act` return of a
      controller whose 18 rays are dead but which is not done; the two neighbours of the threshold and rd . rd == 0.0001f itself; a
      batch of five
  C2  2 x 4 = 8 rays (stride 18 > slide_rays), 32 and 64 (n_here == 32 in the last chunk), 80 (Lerp at 1/4 .. 3/4), 4096 (the maximum),
      each with 1 and 3 controllers (4096: 1); 4160 refused with the states untouched; swr_character_ray_counts for all six
  C3  cs_max returning its 0 and meeting equal operands, cs_min returning addSpeed and meeting equal operands
  C4  NaN velocity, NaN input on the ground and in the air, +Inf and NaN position; NaN velocity in the air under a finite wish
      and a NaN GroundFriction (where fminf / fmaxf differ from MathF.Min / MathF.Max in a finite word): alone, and (but the last)
      between two ordinary controllers; the key buffer is clean afterwards
  C5  chain_attempts [3, 3] and [2, 3]: the sixth k_char_slide launch decides; beside a controller that is done after the first
  C6  a slide hit at exactly moveDistance, one ULP nearer, one ULP farther
  C7  the jump gate
  numerics: C1, C2 (8 and 80 rays) and C5 on the five sensitivity builds and under SWR_RAY_CROSS_FUSED.

The device mutants this file and tests/test_gpu_character.py were run against: profiles/r21_character_edges.md."""
import numpy as np
import pytest

import character_cases as K
import character_edge_cases as E
import raycast_cases as R
from softwarerenderer_amd import CharacterController, _native
from softwarerenderer_amd.rasterizer import Physics
from test_gpu_character import Uploaded, check_batch, check_case, mode  # noqa: F401  (mode: the fixture of the five builds)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def w_of(oracle_lib):
    return lambda targets: K.World(oracle_lib, "", targets)


def run_batch(dev, olib, variant, b, fused=False, what=""):
    return check_batch(dev, olib, variant, b.targets, b.p, b.states, b.inputs, b.dt, b.ring, b.steps, fused=fused, what=what or b.name)


def device_steps(dev, b):
    """[(states, traces)] of a batch on the device alone"""
    out, cur = [], b.states.copy()
    with Uploaded(dev, b.targets) as up:
        for _ in range(b.steps):
            tr = CharacterController.UpdateRaw(dev, b.p, cur, b.inputs, b.dt, b.ring, up)
            out.append((cur.copy(), tr))
    return out


def assert_neighbours_unmoved(dev, b, drop):
    """on the device: every controller but `drop` has the bytes it has when the batch runs without them"""
    fewer, keep = b.without(drop)
    full, short = device_steps(dev, b), device_steps(dev, fewer)
    for k in range(b.steps):
        assert full[k][0][keep].tobytes() == short[k][0].tobytes() and full[k][1][keep].tobytes() == short[k][1].tobytes(), (b.name, k)


# ------------------------------------------------------------------------------------------------ single controllers
def test_c1_dead_plane_rays(device, oracle_lib, w_of):
    for case in E.plane_ray_cases(w_of):
        want = check_case(device, oracle_lib, "", case)
        if case.name in E.DEAD_MASKS or case.name == "c1_threshold_dead":
            assert (int(want[0][1]["ground_found"]), int(want[0][1]["ceiling_found"])) == \
                {"c1_ceiling_rays_dead": (1, 0)}.get(case.name, (0, 0))      # what a cast of the dead rays would have found is not


def test_c1_a_dead_ray_controller_in_a_batch(device, oracle_lib):
    b = E.dead_ray_batch()
    run_batch(device, oracle_lib, "", b)
    assert_neighbours_unmoved(device, b, drop=(2, 4))


@pytest.mark.parametrize("case", [c for c, _, _ in E.math_arm_cases()], ids=lambda c: c.name)
def test_c3_math_arms(device, oracle_lib, case):
    check_case(device, oracle_lib, "", case)


@pytest.mark.parametrize("case", E.nonfinite_cases(), ids=lambda c: c.name)
def test_c4_non_finite_alone(device, oracle_lib, case):
    check_case(device, oracle_lib, "", case)


def test_c4_non_finite_in_a_batch_and_the_key_buffer_after_it(device, oracle_lib):
    rays = R.shape_case(65, 3)
    b = E.nonfinite_batch()
    with Uploaded(device, rays.targets) as ray_targets:
        before = Physics.RaycastNearest(rays.origins, rays.directions, ray_targets, rays.mask)
        want = run_batch(device, oracle_lib, "", b)
        after = Physics.RaycastNearest(rays.origins, rays.directions, ray_targets, rays.mask)
    assert R.same_records(after, before) and int(before["found"].sum()) > 0
    assert any(not np.isfinite(s["position"]).all() for s, _ in want)
    assert_neighbours_unmoved(device, b, drop=tuple(range(1, b.states.shape[0] - 1)))


def test_c5_all_six_rounds(device, oracle_lib):
    for case in E.six_round_cases():
        want = check_case(device, oracle_lib, "", case)
        assert want[0][1]["chain_attempts"].tolist() == ([3, 3] if case.name == "c5_three_and_three" else [2, 3])
    want = run_batch(device, oracle_lib, "", E.six_round_batch())
    assert want[0][1]["chain_attempts"].tolist() == [[0, 1], [3, 3], [2, 3]]


def test_c6_the_slide_limit_is_strict(device, oracle_lib, w_of):
    stops = [int(check_case(device, oracle_lib, "", case)[0][1]["chain_stop"][1]) for case in E.slide_limit_cases(w_of)]
    assert stops == [1, 2, 1]                                               # the tie, one ULP nearer, one ULP farther


@pytest.mark.parametrize("case", E.jump_gate_cases(), ids=lambda c: c.name)
def test_c7_the_jump_gate(device, oracle_lib, case):
    check_case(device, oracle_lib, "", case)


# ------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("b", E.layout_batches(), ids=lambda b: b.name)
def test_c2_ray_layouts(device, oracle_lib, b):
    want = run_batch(device, oracle_lib, "", b)
    assert 2 in {int(x) for _, t in want for x in t["chain_stop"].reshape(-1)}


def test_c2_ray_counts_and_the_refused_layout(device):
    for height, radius, counts, rays in E.LAYOUTS + [E.REFUSED_LAYOUT]:
        p = K.params(height=height, radius=radius)
        assert CharacterController.RayCounts(p) == counts == K.ray_counts(p), (height, radius)
    height, radius, counts, rays = E.REFUSED_LAYOUT
    b = E.layout_batch(height, radius, 1)
    assert rays == 4160 and b.ring.shape[0] == 64
    cur = b.states.copy()
    with Uploaded(device, b.targets) as up:
        with pytest.raises(_native.SwrError) as err:
            CharacterController.UpdateRaw(device, b.p, cur, b.inputs, b.dt, b.ring, up)
    assert err.value.code == _native.SWR_ERR_UNSUPPORTED and cur.tobytes() == b.states.tobytes()


# ------------------------------------------------------------------------------------------------ numerics
def run_numerics(dev, olib, variant, fused, what):
    cases, batches = E.numerics_cases(lambda targets: K.World(olib, variant, targets, fused))
    for case in cases:
        check_case(dev, olib, variant, case, fused=fused, what=what)
    for b in batches:
        run_batch(dev, olib, variant, b, fused=fused, what=f"{what} {b.name}")


def test_numerics_cross_fused_on_the_product_build(device, oracle_lib):
    run_numerics(device, oracle_lib, "", True, "product, cross fused")


@pytest.mark.parametrize("fused", [False, True], ids=["cross_rounded", "cross_fused"])
def test_numerics_on_a_sensitivity_build(mode, fused):
    dev, olib, variant = mode
    run_numerics(dev, olib, variant, fused, variant)
