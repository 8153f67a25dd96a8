"""Cases that put swr_character_update on the branches the cases of character_cases.py never reach (test helper; not part of the
package).  Built on character_cases.py: its Case, World, update, run_case, run_batch and scene builders; the restatement there is the
reference for every one of them.  tests/test_character_edges_host.py asserts, on the restatement alone, the condition that makes each
family mean something; tests/test_gpu_character_edges.py holds the device to the restatement word for word.

  C1  dead CheckPlane rays (:270): ground rays dead, ceiling rays dead, all 18 dead, the two neighbours of the 0.0001 threshold and
      the threshold itself
  C2  ray layouts: 8 rays (stride 18), 32, 64 (full last chunk), 80 (5 vertical steps), 4096 (the maximum), 4160 (refused)
  C3  the arms of MathF.Max / MathF.Min in ApplyFriction and GroundAccelerate; a ceiling ray that points down
  C4  non-finite velocity, input and position
  C5  controllers that use all six slide rounds
  C6  a slide hit at exactly moveDistance (:362, strict) and its two neighbours
  C7  the jump gate (:75)

The constants of C5 are the result of a seeded search (profiles/r21_character_edges.md); the searches of C1 and C6 are short bounded
walks that run here, under the World they are asked for, and raise AssertionError if they do not find what they look for."""
from __future__ import annotations

import contextlib
import dataclasses

import numpy as np

import character_cases as K
from character_cases import Case, STILL, ceiling_quad, floor, params, state, wall
from softwarerenderer_amd.rasterizer import CHARACTER_DTYPE, CHARACTER_INPUT_DTYPE, CharacterController

F32 = np.float32
NAN, INF = float("nan"), float("inf")


@dataclasses.dataclass
class Batch:
    """Several controllers in one call: they share the parameters, the ring and the targets."""
    name: str
    targets: list
    states: np.ndarray                   # CHARACTER_DTYPE
    inputs: np.ndarray                   # CHARACTER_INPUT_DTYPE, the same at every step
    dt: float = 1.0 / 60.0
    steps: int = 2
    p: np.ndarray = dataclasses.field(default_factory=params)
    ring: np.ndarray = None

    def __post_init__(self):
        if self.ring is None:
            self.ring = CharacterController.Ring(K.ray_counts(self.p)[1])

    def run(self, w):
        return K.run_batch(w, self.p, self.states, self.inputs, self.dt, self.ring, self.steps)

    def without(self, drop):
        keep = [i for i in range(self.states.shape[0]) if i not in drop]
        fewer = dataclasses.replace(self, name=self.name + "_without", states=self.states[keep].copy(), inputs=self.inputs[keep].copy())
        return fewer, keep


def batch_of(name, targets, rows, **kw):
    """rows: (state, move, jump) per controller"""
    states = np.array([r[0] for r in rows], dtype=CHARACTER_DTYPE)
    inputs = np.zeros(len(rows), dtype=CHARACTER_INPUT_DTYPE)
    for i, r in enumerate(rows):
        inputs[i]["move"], inputs[i]["jump"] = r[1], int(r[2])
    return Batch(name, targets, states, inputs, **kw)


# ============================================================================ what the restatement reaches
class Reach:
    """What character_cases.probe is told while cases run: the live mask of every Update (bit r: ray r of CheckPlane takes part, ground
    rays first) and the arm every MathF.Max / MathF.Min call takes."""

    def __init__(self):
        self.masks, self.live_counts, self.max_arms, self.min_arms = [], [], [], []
        self._half = None

    @staticmethod
    def arm(a, b):
        if np.isnan(a):
            return "nan_left"
        if np.isnan(b):
            return "nan_right"
        return "equal" if a == b else None

    def __call__(self, kind, *v):
        if kind == "plane":
            direction, live = v
            bits = sum(1 << r for r in range(9) if live[r])
            self.live_counts.append(sum(live))
            if direction == -1:
                self._half = bits
            else:
                self.masks.append(self._half | bits << 9)
        elif kind == "max":
            a, b = v
            self.max_arms.append(self.arm(a, b) or ("left" if b < a else "right"))
        else:
            a, b = v
            self.min_arms.append(self.arm(a, b) or ("left" if a < b else "right"))


@contextlib.contextmanager
def reaching():
    reach, was = Reach(), K.probe
    K.probe = reach
    try:
        yield reach
    finally:
        K.probe = was


# ============================================================================ C1: dead plane rays
# rd of a CheckPlane ray is (0, vel_y * dt -+ 2 (Height / 2 - 0.01), 0): the offsets have no y and frameEnd.x/z == pos.x/z.  At the
# defaults 2 (Height / 2 - 0.01) = 0.48, so vel_y * dt = 0.475 leaves the ground rays 0.005 long, pointing DOWN at the floor, and
# -0.475 leaves the ceiling rays 0.005 long, pointing UP at the ceiling: a cast that ignored the mask would find both.
def dead_ray_cases():
    cs = []
    cs.append(Case("c1_ground_rays_dead", [floor()], state((0, 0.26, 0), (1.0, 6.15, 0.5)), [STILL] * 2, dt=0.1))
    cs.append(Case("c1_ceiling_rays_dead", [floor(0.5), ceiling_quad(1.2)], state((0, 0.9, 0), (0.5, -3.35, 1.0)), [STILL] * 2, dt=0.1))
    # Height 0.02: Height / 2 - 0.01 is +0, both directions' rays are (0, vel_y * dt, 0) = 0.005 down, 0.01 above the floor
    cs.append(Case("c1_all_rays_dead", [floor()], state((0, 0.01, 0), (0.3, -0.05, 0.2)), [STILL] * 2, dt=0.1,
                   p=params(height=0.02, gravity=(0, 0, 0))))
    return cs


def plane_threshold_exact_case():
    """rd . rd == 0.0001f itself: float32(0.01) squares to float32(0.0001) exactly.  Height 0.02 (no half-height offset), dt = 1, the
    position 0 and vel_y = -0.01f make every rd exactly (0, -0.01f, 0); `<` keeps all 18 rays, and they find the floor 0.005 below."""
    return Case("c1_threshold_exact", [floor(-0.005)], state((0, 0, 0), (0, -0.01, 0)), [STILL] * 2, dt=1.0,
                p=params(height=0.02, gravity=(0, 0, 0)))


DEAD_MASKS = {"c1_ground_rays_dead": 0x3fe00, "c1_ceiling_rays_dead": 0x1ff, "c1_all_rays_dead": 0}      # at the first step


def first_mask(w, case):
    with reaching() as reach:
        K.update(w, case.p, case.start, case.input(0), case.dt, case.ring)
    return reach.masks[0]


def plane_threshold_cases(w_of):
    """Two neighbouring vel_y around 4.7 (dt = 0.1, no gravity: rd.y = vel_y * dt - 0.48 crosses -0.01): under the first the ground
    rays have rd . rd < 0.0001f and take no part, under the second they do.  -> [dead, live]"""
    p = params(gravity=(0, 0, 0))
    targets = [floor()]
    w = w_of(targets)
    case_of = lambda vy, name: Case(name, targets, state((0, 0.26, 0), (0.5, vy, 0)), [STILL] * 2, dt=0.1, p=p)      # noqa: E731
    vy = F32(4.7)
    was = first_mask(w, case_of(vy, ""))
    assert was in (0x3fe00, 0x3ffff), hex(was)
    toward = F32(0) if was == 0x3fe00 else F32(8)                           # a dead ray grows as vel_y falls
    for _ in range(64):
        nxt = np.nextafter(vy, toward)
        now = first_mask(w, case_of(nxt, ""))
        if now != was:
            dead, live = (vy, nxt) if was == 0x3fe00 else (nxt, vy)
            return [case_of(dead, "c1_threshold_dead"), case_of(live, "c1_threshold_live")]
        vy = nxt
    raise AssertionError("no two neighbouring velocities put rd . rd on either side of 0.0001f")


def dead_ray_batch():
    """Controller 2 has its ground rays dead and controller 4 its ceiling rays, between ordinary ones and a noclip one."""
    rows = [(state((-2, 0.25, 0), (1, 0, 0), grounded=1, step=0.3), (1, 0, 0), False),
            (state((3, 0.5, 3), noclip=1), (0.3, 0.4, 0), False),
            (state((0, 0.26, 0), (1.0, 6.15, 0.5)), (0, 0, 0), False),
            (state((2, 0.6, 1), (0, 0, 1)), (0, 0, 1), False),
            (state((1, 0.9, -2), (0.5, -3.35, 1.0)), (0, 0, 0), False)]
    return batch_of("c1_batch", [floor(), ceiling_quad(1.2)], rows, dt=0.1)


# ============================================================================ C2: ray layouts
LAYOUTS = [(0.05, 0.02, (1, 4), 8), (0.5, 0.1265, (1, 16), 32), (0.6, 0.2537, (1, 32), 64), (1.1, 0.1265, (4, 16), 80),
           (64.5, 0.5095, (63, 64), 4096)]                                  # Height, Radius, (verticalSteps, horizontalRays), rays
REFUSED_LAYOUT = (65.5, 0.5105, (64, 64), 4160)


def layout_batch(height, radius, n):
    """One floor and the wall x = 1; n controllers (1 or 3) a skin width and 0.019 from the wall: 0 runs into it almost square on (stop
    2) and is then turned along it by its input, 1 runs into it at 45 degrees and slides, 2 square on."""
    p = params(height=height, radius=radius)
    gap = float(F32(1) - (F32(radius) + F32(0.001)) - F32(0.019))
    rows = [(state((gap, height / 2, 0.0), (3, 0, 1.2), grounded=1, step=0.3), (0, 0, 1), False),
            (state((gap, height / 2, 0.5), (2, 0, 2), grounded=1, step=0.03), (1, 0, 1), False),
            (state((gap, height / 2, -0.5), (3, 0, 0), grounded=1, step=0.3), (1, 0, 0), False)][:n]
    rays = (K.ray_counts(p)[0] + 1) * K.ray_counts(p)[1]
    return batch_of(f"c2_{rays}_rays_x{n}", [floor(), wall((1, 0, 0), (-1, 0, 0), y1=height + 4.0)], rows, p=p, steps=2 if rays > 1000 else 3)


def layout_batches(only=None):
    out = []
    for height, radius, _, rays in LAYOUTS:
        if only is None or rays in only:
            out += [layout_batch(height, radius, n) for n in ((1,) if rays == 4096 else (1, 3))]
    return out


# ============================================================================ C3: MathF.Max / MathF.Min and friction
def math_arm_cases():
    on_floor = lambda vel: state((0, 0.25, 0), vel, grounded=1, step=0.3)    # noqa: E731
    run = [((1, 0, 0), False)] * 2
    return [
        # GroundFriction * dt = 1.2: the drop exceeds the speed, MathF.Max returns its 0.  vel_y * dt = -0.56: the "ceiling" ray runs
        # from 0.01 above the floor DOWN through it, and the floor's front face is reported as a ceiling
        (Case("c3_drop_exceeds_speed", [floor()], on_floor((2, 0, 1)), run, dt=0.2), "max", "right"),
        # 4 * 0.25 = 1 and |(3, 0, 4)| = 5 exactly: speed - drop = +0 == 0
        (Case("c3_drop_equals_speed", [floor()], on_floor((3, 0, 4)), run, dt=0.25, p=params(ground_friction=4.0)), "max", "equal"),
        # no friction, 4.9 of the 5 wished for already there: addSpeed 0.1 < 3.5 * 5 / 60
        (Case("c3_add_speed_is_smaller", [floor()], on_floor((4.9, 0, 0)), run, p=params(ground_friction=0.0)), "min", "right"),
        # powers of two: 4 * (1 * 4) * 0.25 = 4 = 4 - 0, the velocity being square to the wish
        (Case("c3_min_of_equals", [floor()], on_floor((0, 0, 2)), run, dt=0.25,
              p=params(ground_friction=0.0, ground_acceleration=4.0, move_speed=4.0)), "min", "equal"),
    ]


# ============================================================================ C4: non-finite controllers
def nonfinite_rows():
    """(name, state, move): ordinary data -- no index or address is derived from any of it"""
    return [("c4_nan_velocity_x", state((0, 0.25, 0), (NAN, 0, 1), grounded=1, step=0.3), (1, 0, 0)),
            ("c4_nan_move_x_on_the_ground", state((0, 0.25, 0.5), (1, 0, 0), grounded=1, step=0.3), (NAN, 0, 1)),
            ("c4_nan_move_x_in_the_air", state((0, 2.0, -0.5), (1, 0, 0)), (NAN, 0, 1)),
            ("c4_inf_position_x", state((INF, 0.25, 0), (1, 0, 0.5)), (1, 0, 0)),
            ("c4_nan_position_y", state((0, NAN, 0), (1, 0, 0.5)), (1, 0, 0)),
            # one in which the NaN does NOT swallow everything (the device mutant fminf passed the five above): wish = (0, 0, 1) is
            # finite, currentSpeed = NaN * 0 + ... is not: MathF.Min(finite, NaN) is NaN and reaches z; fminf gives the finite
            # operand, and `addSpeed > 0` would skip the block
            ("c4_nan_velocity_x_in_the_air", state((0, 2.0, 0.5), (NAN, 0, 1)), (0, 0, 1))]


def nonfinite_targets():
    return [floor(), K.X_WALL()]


def nonfinite_cases():
    targets = nonfinite_targets()
    cases = [Case(name, targets, s, [(move, False)] * 3) for name, s, move in nonfinite_rows()]
    # ... and the same for MathF.Max (the device mutant fmaxf passed them too): a NaN GroundFriction makes the drop NaN beside a finite
    # speed; MathF.Max(NaN, 0) is NaN and so is the velocity, fmaxf gives 0 and the controller stops and accelerates again
    cases.append(Case("c4_nan_ground_friction", targets, state((0, 0.25, 0), (2, 0, 1), grounded=1, step=0.3), [((1, 0, 0), False)] * 2,
                      p=params(ground_friction=NAN)))
    return cases


def nonfinite_batch():
    """All of them between two ordinary controllers: the first walks into the wall, the last falls."""
    rows = [(state((0.83, 0.25, 0), (3, 0, 0), grounded=1, step=0.3), (1, 0, 0), False)]
    rows += [(s, move, False) for _, s, move in nonfinite_rows()]
    rows += [(state((-2, 0.6, 1), (0, 0, 1)), (0, 0, 1), False)]
    return batch_of("c4_batch", nonfinite_targets(), rows, steps=3)


# ============================================================================ C5: all six rounds
def six_round_targets():
    """snap_slides_under_a_slope (chain 1: three attempts) with a wall looking at -z and an oblique wall beside it: the first try of the
    seeded search that gave chain_attempts [3, 3]."""
    base = {c.name: c for c in K.host_cases()}["snap_slides_under_a_slope"]
    return base.targets + [wall((0, 0, 0.201), (0, 0, -1)), wall((-0.216, 0.0, 0.018), (0.748, 0.0, -0.664), length=3.0)]


SIX_ROUNDS = state((0, 0.1, 0), (-4.19, 0.0, 4.57))                         # [3, 3], stops [4, 4], at both steps
TWO_THEN_THREE = state((-0.119, 0.1, -0.305), (-3.29, 0.0, 4.82))           # [2, 3] at both steps (stops [1, 1], then [1, 4])
ONE_ROUND = state((-3.0, 0.6, -3.0), cooldown=0.2)                          # in the air, clear of everything: [0, 1], done in the first round


def six_round_cases():
    targets = six_round_targets()
    return [Case("c5_three_and_three", targets, SIX_ROUNDS, [STILL] * 2, dt=0.05),
            Case("c5_two_and_three", targets, TWO_THEN_THREE, [STILL] * 2, dt=0.05)]


def six_round_batch():
    rows = [(ONE_ROUND, (0, 0, 0), False), (SIX_ROUNDS, (0, 0, 0), False), (TWO_THEN_THREE, (0, 0, 0), False)]
    return batch_of("c5_batch", six_round_targets(), rows, dt=0.05)


# ============================================================================ C6: the slide fold's strict limit
def slide_limit_cases(w_of):
    """The wall x = 1, no gravity, a controller in the air moving 2 * 2^-4 along +x: ray 0 of the ring, (1, 0), starts Radius + 0.001
    ahead of the position, and from pos.x = 1 - 0.151f - 0.125 (or a neighbour within 4 ULP) its hit distance IS moveDistance: `<`
    lets the move through (stop 1), `<=` would stop it.  -> [tie, one ULP nearer the wall, one ULP farther]"""
    p = params(gravity=(0, 0, 0))
    targets = [K.X_WALL()]
    w = w_of(targets)
    vx, dt = F32(2.0), F32(0.0625)
    case_of = lambda x, name: Case(name, targets, state((x, 0.25, 0), (vx, 0, 0)), [STILL] * 2, dt=float(dt), p=p)      # noqa: E731
    x0 = (F32(1) - (F32(0.15) + F32(0.001))) - vx * dt
    tries = [x0]
    for toward in (F32(0), F32(2)):
        x = x0
        for _ in range(4):
            x = np.nextafter(x, toward)
            tries.append(x)
    for x in tries:
        c = case_of(x, "c6_hit_at_move_distance")
        strict = int(K.run_case(w, c)[0][1]["chain_stop"][1])
        loose = int(K.run_case(w, c, ("slide_le",))[0][1]["chain_stop"][1])
        if strict == 1 and loose == 2:
            return [c, case_of(np.nextafter(x, F32(2)), "c6_one_ulp_nearer"), case_of(np.nextafter(x, F32(0)), "c6_one_ulp_farther")]
    raise AssertionError("no position puts ray 0's hit at exactly moveDistance")


# ============================================================================ C7: the jump gate
def jump_gate_cases():
    on_floor = lambda cd: state((0, 0.25, 0), grounded=1, cooldown=cd, step=0.3)      # noqa: E731
    jump = [((0, 0, 0), True)] * 3
    return [Case("c7_jump_under_cooldown", [floor()], on_floor(0.2), jump),
            Case("c7_cooldown_equals_dt", [floor()], on_floor(0.0625), jump, dt=0.0625),      # 0.0625 - 0.0625 = +0, and +0 <= 0
            Case("c7_jump_in_the_air", [floor()], state((0, 1.0, 0)), jump)]


# ============================================================================ everything
def plane_ray_cases(w_of):
    """C1's single controllers"""
    return dead_ray_cases() + plane_threshold_cases(w_of) + [plane_threshold_exact_case()]


def single_cases(w_of):
    return (plane_ray_cases(w_of) + [c for c, _, _ in math_arm_cases()] + nonfinite_cases() + six_round_cases() + slide_limit_cases(w_of) +
            jump_gate_cases())


def batches():
    return [dead_ray_batch()] + layout_batches() + [nonfinite_batch(), six_round_batch()]


def numerics_cases(w_of):
    """what runs on the sensitivity builds and under SWR_RAY_CROSS_FUSED: C1, the layouts of 8 and 80 rays, C5"""
    return plane_ray_cases(w_of) + six_round_cases(), [dead_ray_batch()] + layout_batches((8, 80)) + [six_round_batch()]
