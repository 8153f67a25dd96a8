"""The cases of tests/character_edge_cases.py on the restatement alone (CPU): for every family the condition that makes it mean
something -- the mask, the layout, the arm of MathF.Max / MathF.Min, the attempt pair, the tie -- is asserted here, so a case that
drifts off its branch fails on the CPU instead of passing silently on the GPU.  tests/test_gpu_character_edges.py compares the device
with the same restatement word for word.

`PYTHONPATH=. python tests/test_character_edges_host.py` prints the reach counts of the old cases and of the new ones
(profiles/r21_character_edges.md)."""
import collections

import numpy as np
import pytest

import character_cases as K
import character_edge_cases as E
from oracle import binding as ob

F32 = np.float32
VARIANTS = ["fma", "dotpw", "fma_dotpw", "dpps", "fma_dpps"]


@pytest.fixture(scope="module")
def lib():
    return ob.load()


@pytest.fixture(scope="module")
def w_of(lib):
    return lambda targets: K.World(lib, "", targets)


def run_reaching(w, case, mut=()):
    with E.reaching() as reach:
        return K.run_case(w, case, mut), reach


@pytest.fixture(scope="module")
def runs(w_of):
    """name -> (case, [(state, trace)], Reach) for every single-controller case"""
    return {c.name: (c,) + run_reaching(w_of(c.targets), c) for c in E.single_cases(w_of)}


@pytest.fixture(scope="module")
def batch_runs(w_of):
    """name -> (batch, [(states, traces)], Reach)"""
    out = {}
    for b in E.batches():
        with E.reaching() as reach:
            out[b.name] = (b, b.run(w_of(b.targets)), reach)
    return out


def differs(a, b):
    return [not (K.same_state(x[0], y[0]) and K.same_trace(x[1], y[1])) for x, y in zip(a, b)]


def alone(w_of, batch, i):
    """controller i of a batch stepped on its own"""
    w = w_of(batch.targets)
    s, out = batch.states[i], []
    for _ in range(batch.steps):
        s, t = K.update(w, batch.p, s, batch.inputs[i], batch.dt, batch.ring)
        out.append((s, t))
    return out


def assert_neighbours_unmoved(w_of, batch, steps, drop):
    """every controller but `drop` has the words it has when the batch runs without them, and when it runs alone"""
    fewer, keep = batch.without(drop)
    short = fewer.run(w_of(batch.targets))
    for j, i in enumerate(keep):
        solo = alone(w_of, batch, i)
        for k in range(batch.steps):
            assert K.same_state(steps[k][0][i], short[k][0][j]) and K.same_trace(steps[k][1][i], short[k][1][j]), (i, k)
            assert K.same_state(steps[k][0][i], solo[k][0]) and K.same_trace(steps[k][1][i], solo[k][1]), (i, k)


# ------------------------------------------------------------------------------------------------ C1
@pytest.mark.parametrize("name", sorted(E.DEAD_MASKS))
def test_c1_dead_rays_would_have_hit(w_of, runs, name):
    case, steps, reach = runs[name]
    assert reach.masks[0] == E.DEAD_MASKS[name] and set(reach.live_counts) <= {0, 9}
    cast = K.run_case(w_of(case.targets), case, ("plane_cast_dead",))
    ground = (int(steps[0][1]["ground_found"]), int(cast[0][1]["ground_found"]))
    ceiling = (int(steps[0][1]["ceiling_found"]), int(cast[0][1]["ceiling_found"]))
    want_ground = (0, 1) if not E.DEAD_MASKS[name] & 0x1ff else (ground[0], ground[0])
    want_ceiling = (0, 1) if not E.DEAD_MASKS[name] & 0x3fe00 else (ceiling[0], ceiling[0])
    assert ground == want_ground and ceiling == want_ceiling, (ground, ceiling)      # only the dead direction finds something new


def test_c1_the_live_rays_of_the_ceiling_case_still_find_the_floor(runs):
    _, steps, _ = runs["c1_ceiling_rays_dead"]
    assert int(steps[0][1]["ground_found"]) == 1 and steps[0][1]["chain_attempts"].tolist() == [1, 1]
    assert float(steps[0][0]["position"][1]) == 0.75                        # snapped onto the floor at 0.5


def test_c1_the_threshold_lies_between_two_neighbours(w_of, runs):
    (dead, dead_steps, dead_reach), (live, live_steps, live_reach) = runs["c1_threshold_dead"], runs["c1_threshold_live"]
    a, b = dead.start["velocity"][1], live.start["velocity"][1]
    assert np.nextafter(a, F32(0)) == b                                     # the longer ray is the slower rise
    assert dead_reach.masks[0] == 0x3fe00 and live_reach.masks[0] == 0x3ffff
    h = F32(0.5) / F32(2) - F32(0.01)
    rd = lambda vy: ((F32(0.26) + vy * F32(0.1)) - h) - (F32(0.26) + h)     # noqa: E731  :257, :264-268, y alone
    assert rd(a) * rd(a) < F32(0.0001) <= rd(b) * rd(b)
    assert (int(dead_steps[0][1]["ground_found"]), int(live_steps[0][1]["ground_found"])) == (0, 1)
    cast = K.run_case(w_of(dead.targets), dead, ("plane_cast_dead",))
    assert int(cast[0][1]["ground_found"]) == 1
    assert not any(differs(live_steps, K.run_case(w_of(live.targets), live, ("plane_cast_dead",))))


def test_c1_a_ray_of_exactly_the_threshold_takes_part(w_of, runs):
    case, steps, reach = runs["c1_threshold_exact"]
    rd = (F32(0) + case.start["velocity"][1] * F32(case.dt)) - F32(0)
    assert rd * rd == F32(0.0001) and reach.masks[0] == 0x3ffff
    assert (int(steps[0][1]["ground_found"]), int(steps[0][1]["ceiling_found"])) == (1, 1)
    with E.reaching() as le:
        mutant = K.run_case(w_of(case.targets), case, ("plane_dead_le",))
    assert le.masks[0] == 0 and (int(mutant[0][1]["ground_found"]), int(mutant[0][1]["ceiling_found"])) == (0, 0)


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_walks_find_their_pairs_under_every_build(variant):
    olib = ob.load(variant=variant)
    w_of = lambda targets: K.World(olib, variant, targets)                  # noqa: E731
    assert [c.name for c in E.plane_threshold_cases(w_of)] == ["c1_threshold_dead", "c1_threshold_live"]
    assert len(E.slide_limit_cases(w_of)) == 3


def test_c1_a_dead_ray_controller_leaves_its_neighbours_alone(w_of, batch_runs):
    batch, steps, reach = batch_runs["c1_batch"]
    n = batch.states.shape[0]
    assert n == 5 and int(batch.states[1]["noclip"]) == 1
    first = reach.masks[:n - 1]                                             # (the noclip controller casts no plane ray: four masks a step)
    assert first == [0x3ffff, 0x3fe00, 0x3ffff, 0x1ff]
    assert_neighbours_unmoved(w_of, batch, steps, drop=(2, 4))


# ------------------------------------------------------------------------------------------------ C2
def test_c2_the_layouts(w_of, batch_runs):
    for height, radius, counts, rays in E.LAYOUTS + [E.REFUSED_LAYOUT]:
        assert K.ray_counts(K.params(height=height, radius=radius)) == counts and (counts[0] + 1) * counts[1] == rays
    seen = collections.Counter()
    for name, (batch, steps, _) in batch_runs.items():
        if not name.startswith("c2_"):
            continue
        v, h = K.ray_counts(batch.p)
        seen[(v + 1) * h] += 1
        stops = {int(x) for _, t in steps for x in t["chain_stop"].reshape(-1)}
        attempts = {int(x) for _, t in steps for x in t["chain_attempts"][:, 1]}
        assert 2 in stops and 2 in attempts, (name, stops, attempts)         # the chain-2 fold stopped a move and let one slide
    assert seen == {8: 2, 32: 2, 64: 2, 80: 2, 4096: 1}
    big = batch_runs["c2_4096_rays_x1"][0]
    assert big.states.shape[0] == 1 and len(big.targets) == 2


# ------------------------------------------------------------------------------------------------ C3
@pytest.mark.parametrize("case,which,arm", E.math_arm_cases(), ids=[c.name for c, _, _ in E.math_arm_cases()])
def test_c3_the_arm_named_is_taken(runs, case, which, arm):
    _, steps, reach = runs[case.name]
    assert (reach.max_arms if which == "max" else reach.min_arms)[0] == arm
    assert int(steps[0][1]["ground_found"]) == 1


def test_c3_results_of_the_arms(runs):
    _, steps, _ = runs["c3_drop_exceeds_speed"]
    assert steps[0][0]["velocity"].tolist() == [3.5, 0, 0]                  # stopped dead by friction, then 3.5 * 5 * 0.2 of acceleration
    assert int(steps[0][1]["ceiling_found"]) == 1 and int(steps[0][0]["ceiling"]) == 1      # the floor's front face, from above
    _, steps, _ = runs["c3_drop_equals_speed"]
    assert steps[0][0]["velocity"].tolist() == [4.375, 0, 0]
    _, steps, _ = runs["c3_add_speed_is_smaller"]
    assert steps[0][0]["velocity"].tolist() == [5, 0, 0]
    _, steps, _ = runs["c3_min_of_equals"]
    assert steps[0][0]["velocity"].tolist() == [4, 0, 2]


# ------------------------------------------------------------------------------------------------ C4
def test_c4_the_nan_arms_are_taken(runs):
    assert runs["c4_nan_velocity_x"][2].max_arms[0] == "nan_left" and runs["c4_nan_velocity_x"][2].min_arms[0] == "nan_right"
    assert runs["c4_nan_move_x_on_the_ground"][2].min_arms[0] == "nan_left"     # past !(addSpeed <= 0) with addSpeed = NaN
    assert runs["c4_nan_move_x_in_the_air"][2].min_arms[0] == "nan_left"
    _, steps, _ = runs["c4_nan_velocity_x"]
    assert np.isnan(steps[0][0]["position"]).all()                          # through ProjectOnPlane into all of MoveXZ
    _, steps, _ = runs["c4_inf_position_x"]
    assert np.isposinf(steps[-1][0]["position"][0]) and np.isfinite(steps[-1][0]["position"][1:]).all()
    assert int(steps[0][1]["ground_found"]) == 0                            # Inf - Inf: every ray direction is NaN
    _, steps, _ = runs["c4_nan_position_y"]
    assert np.isnan(steps[-1][0]["position"][1]) and np.isfinite(steps[-1][0]["position"][[0, 2]]).all()


def test_c4_fmax_and_fmin_are_not_the_reference(w_of, runs, monkeypatch):
    """MathF.Max / MathF.Min hand a NaN operand back, fmaxf / fminf drop it: each difference reaches a finite word of a named case."""
    def changed(name):
        case, steps, _ = runs[name]
        return any(differs(steps, K.run_case(w_of(case.targets), case)))
    with monkeypatch.context() as m:
        m.setattr(K, "cs_max", lambda a, b: np.fmax(a, b))
        assert changed("c4_nan_ground_friction") and not changed("c4_nan_velocity_x")
    with monkeypatch.context() as m:
        m.setattr(K, "cs_min", lambda a, b: np.fmin(a, b))
        assert changed("c4_nan_velocity_x_in_the_air") and not changed("c4_nan_move_x_in_the_air")
    _, steps, reach = runs["c4_nan_ground_friction"]
    assert reach.max_arms[0] == "nan_left" and np.isnan(steps[0][0]["velocity"][[0, 2]]).all() and np.isfinite(steps[0][0]["position"]).all()
    _, steps, reach = runs["c4_nan_velocity_x_in_the_air"]
    assert reach.min_arms[0] == "nan_right" and np.isnan(steps[0][0]["velocity"][2])


def test_c4_the_ordinary_neighbours_are_unmoved(w_of, batch_runs, runs):
    batch, steps, _ = batch_runs["c4_batch"]
    n = len(E.nonfinite_rows())
    assert n == 6 and batch.states.shape[0] == n + 2
    assert_neighbours_unmoved(w_of, batch, steps, drop=tuple(range(1, n + 1)))
    assert np.isfinite(steps[-1][0]["position"][[0, n + 1]]).all() and 2 in steps[0][1]["chain_stop"][0].tolist()
    for i, (name, _, _) in enumerate(E.nonfinite_rows()):                   # ... and the five are the five single cases
        for k in range(batch.steps):
            assert K.same_state(steps[k][0][1 + i], runs[name][1][k][0]) and K.same_trace(steps[k][1][1 + i], runs[name][1][k][1])


# ------------------------------------------------------------------------------------------------ C5
def test_c5_all_six_rounds(runs, batch_runs):
    _, steps, _ = runs["c5_three_and_three"]
    for _, t in steps:
        assert t["chain_attempts"].tolist() == [3, 3] and t["chain_stop"].tolist() == [4, 4]
    _, steps, _ = runs["c5_two_and_three"]
    assert [t["chain_attempts"].tolist() for _, t in steps] == [[2, 3], [2, 3]]
    assert [t["chain_stop"].tolist() for _, t in steps] == [[1, 1], [1, 4]]
    _, steps, _ = batch_runs["c5_batch"]
    for _, t in steps:
        assert t["chain_attempts"].tolist() == [[0, 1], [3, 3], [2, 3]]     # controller 0 is done after the first round


# ------------------------------------------------------------------------------------------------ C6
def test_c6_a_hit_at_exactly_move_distance_does_not_stop_the_move(w_of, runs):
    tie, nearer, farther = (runs[n] for n in ("c6_hit_at_move_distance", "c6_one_ulp_nearer", "c6_one_ulp_farther"))
    x = tie[0].start["position"][0]
    assert nearer[0].start["position"][0] == np.nextafter(x, F32(2)) and farther[0].start["position"][0] == np.nextafter(x, F32(0))
    w = w_of(tie[0].targets)
    stop = lambda run, mut=(): int((K.run_case(w, run[0], mut) if mut else run[1])[0][1]["chain_stop"][1])      # noqa: E731
    assert (stop(tie), stop(tie, ("slide_le",))) == (1, 2)
    assert (stop(nearer), stop(nearer, ("slide_le",))) == (2, 2)
    assert (stop(farther), stop(farther, ("slide_le",))) == (1, 1)
    # the tie is ray 0's own: cast_many's distance for it IS moveDistance
    case = tie[0]
    P, N = w.arrays(0)
    radius = F32(case.p["radius"]) + F32(0.001)
    move = (case.start["velocity"] * F32(case.dt)).astype(F32)
    half = F32(case.p["height"]) * F32(0.5)
    lowest = w.lerp(-half + F32(0), half, F32(0))                           # (in the air: ActualStepSize is 0)
    origin = case.start["position"] + K.v3(0, lowest, 0) + K.v3(radius * case.ring[0][0], 0, radius * case.ring[0][1])
    found, dist, _, _ = K.cast_many([origin], [K.R.normalize3v(move, w.order)], P, N, case.targets[0].indices, w.order, False)
    assert case.ring[0].tolist() == [1, 0] and bool(found[0]) and dist[0] == K.length(w, move) == F32(0.125)


# ------------------------------------------------------------------------------------------------ C7
def test_c7_the_jump_gate(runs):
    _, steps, _ = runs["c7_jump_under_cooldown"]
    assert all(float(s["velocity"][1]) < 0 and 0 < float(s["jump_cooldown"]) < 0.2 for s, _ in steps)
    _, steps, _ = runs["c7_cooldown_equals_dt"]
    assert float(steps[0][0]["velocity"][1]) == 4.0 and float(steps[0][0]["jump_cooldown"]) == 0.25 and int(steps[0][0]["grounded"]) == 1
    assert steps[0][1]["chain_attempts"].tolist() == [0, 1]                 # the fresh cooldown forbids the snap
    _, steps, _ = runs["c7_jump_in_the_air"]
    assert all(float(s["velocity"][1]) < 0 and float(s["jump_cooldown"]) == 0 and not int(s["grounded"]) for s, _ in steps)


# ------------------------------------------------------------------------------------------------ coverage
def reach_of(single, batched):
    """masks, layouts, arms and attempt pairs over ([(case, steps, Reach)], [(p, steps, Reach)])"""
    masks, layouts, pairs = collections.Counter(), collections.Counter(), collections.Counter()
    arms = {"max": collections.Counter(), "min": collections.Counter()}
    for p, steps, reach, traces in [(c.p, s, r, [t for _, t in s]) for c, s, r in single] + \
                                   [(p, s, r, [t for _, ts in s for t in ts]) for p, s, r in batched]:
        v, h = K.ray_counts(p)
        layouts[(v + 1) * h] += 1
        masks.update(reach.masks)
        arms["max"].update(reach.max_arms); arms["min"].update(reach.min_arms)
        pairs.update(tuple(t["chain_attempts"].tolist()) for t in traces)
    return masks, layouts, arms, pairs


def test_coverage_of_the_new_cases(lib, w_of, runs, batch_runs):
    masks, layouts, arms, pairs = reach_of(list(runs.values()), [(b.p, s, r) for b, s, r in batch_runs.values()])
    assert {0, 0x1ff, 0x3fe00, 0x3ffff} == set(masks)
    assert {8, 32, 64, 80, 4096} <= set(layouts)
    assert set(arms["max"]) == {"left", "right", "equal", "nan_left"}       # (its right operand is the constant 0: never NaN)
    assert set(arms["min"]) == {"left", "right", "equal", "nan_left", "nan_right"}
    assert (3, 3) in pairs and (2, 3) in pairs
    assert any(not np.isfinite(s[f]).all() for _, steps, _ in runs.values() for s, _ in steps for f in K.STATE_FLOATS)
    old = K.host_cases() + [K.slide_tie_case(), K.plane_tie_case(), K.max_distance_case(w_of)]
    for mutant, red in (("plane_cast_dead", ["c1_ground_rays_dead", "c1_ceiling_rays_dead", "c1_all_rays_dead", "c1_threshold_dead"]),
                        ("plane_dead_le", ["c1_threshold_exact"]), ("slide_le", ["c6_hit_at_move_distance"])):
        for name in red:
            case, steps, _ = runs[name]
            assert any(differs(steps, K.run_case(w_of(case.targets), case, (mutant,)))), (mutant, name)
        for case in old:
            w = w_of(case.targets)
            assert not any(differs(K.run_case(w, case), K.run_case(w, case, (mutant,)))), (mutant, case.name)


def old_reach(lib):
    """what the inputs of tests/test_gpu_character.py reach, replayed through the restatement"""
    from softwarerenderer_amd import CharacterController
    w_of = lambda targets: K.World(lib, "", targets)                        # noqa: E731
    single = [(c,) + run_reaching(w_of(c.targets), c) for c in
              K.host_cases() + [K.slide_tie_case(), K.plane_tie_case(), K.max_distance_case(w_of)] + K.numerics_cases()]
    batched = []

    def batch(targets, p, states, inputs, dt, ring, steps):
        with E.reaching() as reach:
            batched.append((p, K.run_batch(w_of(targets), p, states, inputs, dt, ring, steps), reach))
    for n in (1, 2, 65):
        for n_targets in (0, 1, 3, 4):
            targets, states, inputs = K.batch_case(n, n_targets)
            batch(targets[:n_targets], K.params(), states, inputs, 0.05, CharacterController.Ring(18), 3)
    targets, states, inputs = K.chain1_batch()
    batch(targets, K.params(), states, inputs, 1 / 60, CharacterController.Ring(18), 3)
    targets, states, inputs = K.batch_case(3, 4)
    states["position"][:, 1] += 0.25
    states["position"][:, 0] -= 0.15
    batch(targets, K.params(height=1.0, radius=0.3), states, inputs, 0.05, CharacterController.Ring(37), 3)
    targets, states, inputs, dt = K.dust2_batch()
    batch(targets, K.params(), states, inputs, dt, CharacterController.Ring(18), 6)
    return reach_of(single, batched)


if __name__ == "__main__":
    the_lib = ob.load()
    the_w_of = lambda targets: K.World(the_lib, "", targets)                # noqa: E731
    new_single = [(c,) + run_reaching(the_w_of(c.targets), c) for c in E.single_cases(the_w_of)]
    new_batched = []
    for b_ in E.batches():
        with E.reaching() as reach_:
            new_batched.append((b_.p, b_.run(the_w_of(b_.targets)), reach_))
    for title, (masks_, layouts_, arms_, pairs_) in (("old", old_reach(the_lib)), ("new", reach_of(new_single, new_batched))):
        print(title)
        print("  masks   ", {hex(k): v for k, v in sorted(masks_.items())})
        print("  layouts ", dict(sorted(layouts_.items())))
        print("  max arms", dict(sorted(arms_["max"].items())), " min arms", dict(sorted(arms_["min"].items())))
        print("  attempts", dict(sorted(pairs_.items())))
