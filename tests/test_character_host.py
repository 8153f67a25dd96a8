"""The restatement of CharacterController.Update in tests/character_cases.py, pinned on the CPU with hand-derived cases on tiny meshes;
the Python class's defaults and swr_character_ray_counts (host code of the library) against the reference's formulas.

Every GPU test of tests/test_gpu_character.py compares the device with this restatement word for word, so what is asserted here is
what the device is held to.  The coverage test states what the cases reach together; the mutant test shows that each serial-schedule
or ordering rule of the restatement is visible in a named case."""
import numpy as np
import pytest

import character_cases as K
import raycast_cases as R
from oracle import binding as ob
from softwarerenderer_amd import CharacterController

F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    return ob.load()


@pytest.fixture(scope="module")
def runs(lib):
    """name -> (case, [(state, trace)] per step) for every host case and the three special ones"""
    cases = K.host_cases() + [K.slide_tie_case(), K.plane_tie_case(), K.max_distance_case(lambda t: K.World(lib, "", t))]
    return {c.name: (c, K.run_case(K.World(lib, "", c.targets), c)) for c in cases}


def close(a, b, tol=2e-6):
    return np.allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rtol=0, atol=tol)


def test_cast_many_is_raycast_for_every_ray(lib):
    case = R.shape_case(65, 1)
    tg = case.targets[0]
    P, N = R.world_arrays(lib, tg.vertices, tg.model, tg.normal_matrix)
    for fused in (False, True):
        found, dist, point, normal = K.cast_many(case.origins, case.directions, P, N, tg.indices, 0, fused)
        for r in range(case.origins.shape[0]):
            want = R.raycast(case.origins[r], case.directions[r], P, N, tg.indices, 1, 0, fused)
            got = R.miss_record(0)
            got["found"], got["distance"], got["point"], got["normal"], got["triangle"] = found[r], dist[r], point[r], normal[r], want["triangle"]
            assert R.same_records(got, want), (fused, r)
        assert found.any() and not found.all()


# ------------------------------------------------------------------------------------------------ hand-derived cases
def test_resting_on_a_floor_snaps_to_half_the_height_and_stops_the_fall(runs):
    _, steps = runs["rest_on_floor"]
    for s, t in steps:
        assert int(t["ground_found"]) == 1 and float(s["position"][1]) == 0.25 and float(s["velocity"][1]) == 0.0 and int(s["grounded"]) == 1
        assert t["chain_stop"].tolist() == [1, 1]
    assert float(steps[0][0]["actual_step_size"]) == float(F32(0.3))


def test_free_fall_over_nothing(runs):
    _, steps = runs["free_fall"]
    vy, y = 0.0, 5.0
    for s, t in steps:
        vy -= 14.0 / 60.0
        y += vy / 60.0
        assert int(t["ground_found"]) == 0 and t["chain_attempts"].tolist() == [0, 1] and t["chain_stop"].tolist() == [0, 1]
        assert close(s["velocity"][1], vy) and close(s["position"][1], y, 1e-5) and float(s["actual_step_size"]) == 0.0
        assert np.isneginf(t["ground_point"]).all() and t["ground_normal"].tolist() == [0, 1, 0]
    assert close(steps[0][0]["velocity"][0], 0.35 * 5 / 60)              # AirAccelerate: AirAcceleration * wishSpeed * dt


def test_a_jump_and_its_cooldown(runs):
    _, steps = runs["jump_and_cooldown"]
    s, t = steps[0]
    assert float(s["velocity"][1]) == 4.0 and float(s["jump_cooldown"]) == 0.25 and close(s["position"][1], 0.65)
    assert int(t["ground_found"]) == 1 and t["chain_attempts"].tolist() == [0, 1]          # the floor is seen, the cooldown forbids the snap
    assert [round(float(x[0]["jump_cooldown"]), 4) for x in steps] == [0.25, 0.15, 0.05, -0.05]
    assert all(float(x[0]["velocity"][1]) != 4.0 for x in steps[1:])                       # no second jump: not grounded any more


def test_a_ceiling_stops_a_rise_and_clears_the_cooldown(runs):
    _, steps = runs["ceiling_stops_a_rise"]
    s, t = steps[0]
    assert int(t["ceiling_found"]) == 1 and int(s["ceiling"]) == 1 and float(s["velocity"][1]) == 0.0 and float(s["jump_cooldown"]) == 0.0
    assert float(s["position"][1]) == float(F32(0.72))
    assert int(steps[1][1]["ceiling_found"]) == 0


def test_noclip(runs):
    _, steps = runs["noclip"]
    s, t = steps[0]                                                       # |(3, 4, 0)| = 5 > 1: normalised, times MoveSpeed 5
    assert close(s["velocity"], (3, 4, 0)) and close(s["position"], (0.05, 0.1 + 4 / 60, 0)) and not t.tobytes().strip(b"\0")
    assert close(steps[1][0]["velocity"], (1.5, 2.0, 0))                  # |(0.3, 0.4, 0)| = 0.5: taken as it is; Y is kept
    assert float(s["actual_step_size"]) == float(F32(0.03)) and int(s["noclip"]) == 1


def test_walking_square_into_a_wall_stops_a_skin_width_before_it(runs):
    _, steps = runs["wall_square_on"]
    s, t = steps[0]                                                       # the ring reaches 0.83 + 0.151; the wall is 0.019 away
    assert t["chain_stop"].tolist() == [1, 2] and t["chain_attempts"].tolist() == [1, 1]
    assert close(s["position"], (0.83 + (1 - 0.83 - 0.151) - 0.001, 0.25, 0), 1e-6)
    assert all(close(x[0]["position"][0], 0.848, 1e-6) for x in steps[1:])


def test_walking_at_45_degrees_into_a_wall_slides_along_it(runs):
    _, steps = runs["wall_at_45_degrees"]
    for s, t in steps:
        assert t["chain_attempts"].tolist() == [1, 2] and t["chain_stop"].tolist() == [1, 1]
    assert close(steps[0][0]["position"][0], 0.848 + 0.001 * (1 - np.sqrt(0.5)), 2e-5)     # stopped a skin width back ALONG the move
    z = [float(s["position"][2]) for s, _ in steps]
    assert all(b > a + 0.03 for a, b in zip([0.0] + z, z)) and all(close(s["position"][0], steps[0][0]["position"][0], 1e-6) for s, _ in steps)


def test_a_corner_reaches_the_third_attempt(runs):
    _, steps = runs["corner"]
    assert steps[0][1]["chain_attempts"].tolist() == [1, 3] and steps[0][1]["chain_stop"].tolist() == [1, 4]
    assert float(steps[0][0]["position"][0]) < 0.85 and float(steps[0][0]["position"][2]) < 0.95


def test_the_vertical_snap_slides_under_a_slope(lib, runs):
    _, steps = runs["snap_slides_under_a_slope"]                          # chain 1: up into the slope, along it, up the wall: depth limit
    for s, t in steps:
        assert t["chain_attempts"].tolist() == [3, 1] and t["chain_stop"].tolist() == [4, 1] and int(t["ceiling_found"]) == 1
        assert 0.1 < float(s["position"][1]) < 0.25 and 0 < float(s["position"][0]) < 0.05      # stopped under the slope, pushed toward +x
    targets, states, inputs = K.chain1_batch()
    out = K.run_batch(K.World(lib, "", targets), K.params(), states, inputs, 1 / 60, CharacterController.Ring(18), 3)
    assert {1, 2, 3} <= {int(x) for _, t in out for x in t["chain_attempts"][:, 0]}


def test_a_zero_move_gives_the_position_back(runs):
    _, steps = runs["zero_move_in_the_air"]
    for s, t in steps:                                                    # Normalize(0) = NaN directions: nothing is hit, desiredPos returns
        assert s["position"].tolist() == [0, 5, 0] and s["velocity"].tolist() == [0, 0, 0] and t["chain_stop"].tolist() == [0, 1]


def test_a_slide_swallowed_by_rounding_ends_with_a_zero_direction(runs):
    _, steps = runs["slide_swallowed_by_rounding"]                        # at 2^24 the safe stop position rounds onto the desired one
    assert steps[0][1]["chain_stop"].tolist() == [0, 3] and float(steps[0][0]["position"][0]) == 16777218.0


def test_project_on_plane(lib):
    w = K.World(lib, "", [])
    v = K.v3(1, 2, 3)
    assert K.project_on_plane(w, v, K.v3(0, 0.0009, 0)).tolist() == v.tolist()             # |n|^2 = 8.1e-7 < 1e-6: the vector itself
    assert K.project_on_plane(w, v, K.v3(0, 0.0011, 0)).tolist() == [1, 0, 3]              # a SHORT normal still projects: / |n|^2
    assert K.project_on_plane(w, v, K.v3(0, 2, 0)).tolist() == [1, 0, 3]
    got = K.project_on_plane(w, K.v3(1, 0, 0), K.v3(F32(0.6), F32(0.8), 0))
    assert close(got, (1 - 0.36, -0.48, 0))


def test_friction_below_a_tenth_stops_the_controller(runs):
    _, steps = runs["friction_below_a_tenth"]
    assert steps[0][0]["velocity"].tolist() == [0, 0, 0] and close(steps[0][0]["position"], (0.05 / 60, 0.25, 0.02 / 60))


def test_the_air_speed_clamp(runs):
    _, steps = runs["air_speed_clamp"]
    for s, _ in steps:
        assert close(np.hypot(s["velocity"][0], s["velocity"][2]), 6.0, 1e-5)
    assert close(steps[0][0]["position"][0], 10 / 60)                     # the step itself still moved with the unclamped velocity


def test_the_tilted_ground_normal_bends_the_move(runs):
    _, steps = runs["tilted_ground_normal"]
    gn = steps[0][1]["ground_normal"]
    assert close(gn, np.array([0.18, 0.9, 0.4]) / np.linalg.norm([0.18, 0.9, 0.4]), 1e-6)
    assert float(steps[0][0]["position"][1]) < 0.25                       # MoveXZ has a Y component: down the slope of the NORMAL


# ------------------------------------------------------------------------------------------------ ties and mutants
def differs(a, b):
    return [not (K.same_state(x[0], y[0]) and K.same_trace(x[1], y[1])) for x, y in zip(a, b)]


def test_the_slide_tie_goes_to_the_first_target(lib, runs):
    case, steps = runs["slide_tie"]
    assert steps[0][1]["chain_stop"].tolist() == [0, 4] and float(steps[0][0]["position"][2]) < 0      # the z < 0 half: the move slid
    w = K.World(lib, "", case.targets)
    ray_major = K.run_case(w, case, ("slide_ray_major",))
    assert ray_major[0][1]["chain_stop"].tolist() == [0, 2] and float(ray_major[0][0]["position"][2]) == 0
    assert not close(ray_major[-1][0]["position"], steps[-1][0]["position"], 1e-5)
    ring = case.ring                                                      # (the table is exactly symmetric)
    assert (ring[:9, 0] == ring[::-1][:9, 0]).all() and (ring[:9, 1] == -ring[::-1][:9, 1]).all()


def test_the_plane_tie_goes_to_the_first_ray(lib, runs):
    case, steps = runs["plane_tie"]
    left = np.array([-0.2, 0.9, 0.3]) / np.linalg.norm([-0.2, 0.9, 0.3])
    assert close(steps[0][1]["ground_normal"], left, 1e-6)                # offset 1 (-x) reaches only the SECOND target
    target_major = K.run_case(K.World(lib, "", case.targets), case, ("plane_target_major",))
    assert float(target_major[0][1]["ground_normal"][0]) > 0 and not close(target_major[-1][0]["position"], steps[-1][0]["position"], 1e-4)


MUTANTS = [("plane_target_major", "", ["plane_tie"]), ("slide_ray_major", "", ["slide_tie"]), ("plane_lt", "", ["hit_at_max_distance"]),
           ("chain1_new_step", "", ["sunk_below_a_ledge"]), ("project_dot3v", "dotpw", ["tilted_ground_normal"])]


@pytest.mark.parametrize("mutant,variant,red", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_host_mutants_turn_named_cases_red(runs, mutant, variant, red):
    olib = ob.load(variant=variant) if variant else ob.load()
    for name in red:
        case = runs[name][0]
        w = K.World(olib, variant, case.targets)
        assert any(differs(K.run_case(w, case), K.run_case(w, case, (mutant,)))), (mutant, name)
    if mutant == "project_dot3v":                                         # ... and under the sequential order the mutant is invisible
        case = runs[red[0]][0]
        w = K.World(ob.load(), "", case.targets)
        assert not any(differs(K.run_case(w, case), K.run_case(w, case, (mutant,))))
    if mutant == "chain1_new_step":
        assert runs["sunk_below_a_ledge"][1][0][1]["chain_stop"].tolist() == [1, 1]            # 0.03 keeps the low rays under the ledge


def test_coverage_of_the_cases(runs):
    traces = [t for _, steps in runs.values() for _, t in steps]
    states = [s for _, steps in runs.values() for s, _ in steps]
    assert {int(t["ground_found"]) for t in traces} == {0, 1} and {int(t["ceiling_found"]) for t in traces} == {0, 1}
    assert {int(x) for t in traces for x in t["chain_stop"]} == {0, 1, 2, 3, 4}
    assert {int(x) for t in traces for x in t["chain_attempts"]} == {0, 1, 2, 3}
    steps_in = {float(c.start["actual_step_size"]) for c, _ in runs.values()} | {float(s["actual_step_size"]) for s in states}
    assert steps_in == {float(F32(0.03)), float(F32(0.3)), 0.0}


def test_the_numerics_switches_are_visible_in_the_numerics_cases(lib):
    """The GPU numerics tests distinguish something: the Cross model, the Transform flag, the fused Lerp and the shuffle-add dot order
    each change a word of the restatement on the 45-degree wall / corner cases of character_cases.numerics_cases.  The dpps order
    differs from the sequential one only in the sign of a zero sum ((z + 0) turns -0.0 into +0.0) and changes no word there; the
    dpps builds are still compared in full."""
    cases = K.numerics_cases()
    assert [c.name for c in cases] == ["wall_at_45_degrees_leaning", "corner_leaning"] and K.ray_counts(cases[0].p) == (3, 18)

    def words(variant="", fused=False, flag=None):
        olib = ob.load(variant=variant) if variant else lib
        return b"".join(s.tobytes() + t.tobytes() for c in cases for s, t in K.run_case(K.World(olib, variant, c.targets, fused, flag), c))
    base = words()
    assert words(fused=True) != base, "Cross model"
    assert words(flag=1) != base, "Transform flag"
    assert words("dotpw") != base, "dot order"
    assert words("fma") != base, "Lerp"
    attempts = [int(t["chain_attempts"][1]) for c in cases for _, t in K.run_case(K.World(lib, "", c.targets), c)]
    assert {1, 2, 3} <= set(attempts)


def test_the_dust2_batch_lands_and_collides(lib):
    targets, states, inputs, dt = K.dust2_batch()
    out = K.run_batch(K.World(lib, "", targets), K.params(), states, inputs, dt, CharacterController.Ring(18), 6)
    assert len(targets) == 11
    assert any(int(t["ground_found"].max()) for _, t in out) and any(int(s["grounded"].max()) for s, _ in out)
    assert any(int(t["chain_stop"].max()) >= 2 for _, t in out)           # a collision ended a chain


# ------------------------------------------------------------------------------------------------ the package's host side
def test_the_python_class_has_the_reference_defaults():
    c = CharacterController((1, 2, 3), [], [])
    assert c.Position.tolist() == [1, 2, 3] and c.Velocity.tolist() == [0, 0, 0] and not (c.IsGrounded or c.IsCeiling or c.IsNoClipEnabled)
    assert (c.Gravity.tolist(), c.Height, c.Radius, c.StepSize, float(c.ActualStepSize)) == ([0, -14, 0], 0.5, 0.15, 0.3, float(F32(0.03)))
    assert (c.MoveSpeed, c.JumpForce, c.GroundAcceleration, c.AirAcceleration, c.MaxAirSpeed, c.GroundFriction, c.AirControl) == \
        (5.0, 4.0, 3.5, 0.35, 6.0, 6.0, 0.2)
    assert c.CamOffset.tolist() == [0, F32(0.15), 0] and float(c.JumpCooldownTimer) == 0 and c.JumpCooldownDuration == 0.25
    assert c.Params().tobytes() == K.params().tobytes()
    s = c.State()
    assert float(s["actual_step_size"]) == float(F32(0.03)) and s["position"].tolist() == [1, 2, 3]


def test_update_batch_takes_controllers_built_from_the_same_meshes_and_equal_matrices():
    mesh_a, mesh_b = object(), object()                                   # (the check looks at identity and matrices only)
    one = CharacterController((0, 0, 0), [[mesh_a, mesh_b]], [np.eye(4)])
    two = CharacterController((1, 0, 0), [[mesh_a, mesh_b]], [np.eye(4, dtype=np.float32)])
    moved = CharacterController((1, 0, 0), [[mesh_a, mesh_b]], [np.eye(4) * 2])
    fewer = CharacterController((1, 0, 0), [[mesh_a]], [np.eye(4)])
    assert CharacterController._same_targets(one, two) and not CharacterController._same_targets(one, moved)
    assert not CharacterController._same_targets(one, fewer)
    two.Height = 1.0
    with pytest.raises(ValueError):                                       # other properties: refused before any device call
        CharacterController.UpdateBatch([one, two], 1 / 60, [(0, 0, 0)] * 2, [False] * 2)


def test_ray_counts_follow_the_formulas():
    assert CharacterController.RayCounts(K.params()) == (1, 18) == K.ray_counts(K.params())
    tall = K.params(height=1.0, radius=0.3)
    assert CharacterController.RayCounts(tall) == (1, 37) == K.ray_counts(tall)
    for h, r in ((2.0, 0.15), (0.5, 0.01), (1.8, 0.25), (3.0, 0.499)):
        p = K.params(height=h, radius=r)
        assert CharacterController.RayCounts(p) == K.ray_counts(p), (h, r)
    assert CharacterController.RayCounts(K.params(height=2.0, radius=0.15))[0] == 6 and CharacterController.RayCounts(K.params(radius=0.01))[1] == 4


def test_the_ring_is_the_float32_angle_through_the_c_runtime():
    import math
    ring = CharacterController.Ring(18)
    assert ring.shape == (18, 2) and ring.dtype == np.float32 and ring[0].tolist() == [1, 0]
    angle = F32(F32(F32(2) * F32(math.pi)) * F32(5)) / F32(18)
    assert ring[5].tolist() == [float(F32(math.cos(float(angle)))), float(F32(math.sin(float(angle))))]
