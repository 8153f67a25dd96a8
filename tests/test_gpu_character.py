"""swr_character_update (csrc/swr_character.hip.h) against the restatement of tests/character_cases.py, with no tolerance anywhere:
after EVERY step every field of the state and of the trace is compared -- integers as integers, floats as 32-bit words
(cull_edge_cases.same_words: a NaN word of the reference must be a NaN word here).

  - every host case of tests/test_character_host.py stepped 3-4 times, so that actual_step_size, the cooldown and grounded carry;
  - batch shapes: 1 / 2 / 65 controllers in one call with positions and inputs of their own (some end chain 2 at its first attempt,
    others go on to the third; controller 1 is noclip), against 1, 3 and 4 targets under models of their own, and no target at all;
  - ray counts: the default (2 x 18 = 36 rays) and Height 1.0, Radius 0.3 (2 x 37 = 74 rays: past the 32-ray chunk and 64);
  - both tie cases, whose winners tests/test_character_host.py names;
  - dust2: 2 controllers x 6 steps over the 11 meshes;
  - numerics: the product build under the Transform flags (0,0) and (1,1), with and without SWR_RAY_CROSS_FUSED, and the five
    sensitivity builds against the oracle built alike, on the 45-degree wall and the corner with leaning walls and a taller capsule
    (character_cases.numerics_cases: the host test shows which switch changes which words there) and the tilted ground normal;
  - beside the renderer: an update between two recorded draws leaves them one batch; an update beside a frame in flight makes no
    host wait on the frame's stream; both frames are the oracle's;
  - swr_raycast_nearest right after an update returns what it returned before (the key buffer is left clean);
  - the staging threshold: 7000 controllers in one call (pageable host block) against the same in two calls of 3500 (pinned block),
    byte for byte, with and without the trace, on a context of its own whose key buffer grows under the call;
  - arguments: the INVALID_ARG / UNSUPPORTED cases and the empty calls; the Python class against the restatement.

Device mutants (one change in a scratch copy of csrc/, built as a library of its own, this file and
tests/test_gpu_character_edges.py run once on it): the table in profiles/r21_character_edges.md says which tests each turns red.  Of
this file's, test_ties catches TARGET_MAJOR swapped in either fold and test_a_hit_at_exactly_max_distance `<` for `<=` under
INCLUSIVE; `w.step_now = w.step_in` dropped from k_char_planes changes nothing (k_char_begin stores the same value)."""
import ctypes as C
import os

import numpy as np
import pytest

import character_cases as K
import raycast_cases as R
from oracle import binding as ob
from softwarerenderer_amd import CharacterController, Device, _native, scenes
from softwarerenderer_amd.rasterizer import (CHARACTER_DTYPE, CHARACTER_INPUT_DTYPE, CHARACTER_TRACE_DTYPE, BlendMode, CullMode, DepthTest,
                                              MainWindow, Mesh, Physics, Program, Rasterizer, ShaderProgram)
from util import assert_frame_parity

pytestmark = pytest.mark.gpu

MODES = [("libswr_hip_fma.so", "fma"), ("libswr_hip_dotpw.so", "dotpw"), ("libswr_hip_fma_dotpw.so", "fma_dotpw"),
         ("libswr_hip_dpps.so", "dpps"), ("libswr_hip_fma_dpps.so", "fma_dpps")]


@pytest.fixture(scope="module", params=MODES, ids=[m[1] for m in MODES])
def mode(request):
    lib, variant = request.param
    if not os.path.exists(os.path.join(os.path.dirname(_native.LIB_PATH), lib)):
        pytest.fail(f"{lib} is missing: __graft_entry__.build() makes it (make -C softwarerenderer_amd/csrc variants)")
    olib = ob.load(variant=variant)
    dev = Device(0, lib=lib)
    assert dev.numerics_mode() == (olib.oswr_numerics_fma(), olib.oswr_dot_pairwise())
    yield dev, olib, variant
    dev.close()


class Uploaded:
    """raycast_cases.Targets as retained meshes on `dev`: [(Mesh, model, normal_matrix)]."""

    def __init__(self, dev, targets):
        self.meshes = [Mesh(dev, t.vertices, t.indices) for t in targets]
        self.targets = [(m, t.model, t.normal_matrix) for m, t in zip(self.meshes, targets)]

    def __enter__(self):
        return self.targets

    def __exit__(self, *exc):
        for m in self.meshes:
            m.Dispose()


def compare(got_s, got_t, want_s, want_t, what):
    bad = [f"controller {i}: got  {K.show(got_s[i], got_t[i])}\n{' ' * 14}want {K.show(want_s[i], want_t[i])}"
           for i in range(want_s.shape[0]) if not (K.same_state(got_s[i], want_s[i]) and K.same_trace(got_t[i], want_t[i]))]
    assert not bad, f"{what}: {len(bad)} of {want_s.shape[0]} controllers differ:\n" + "\n".join(bad[:6])


def check_batch(dev, olib, variant, targets, p, states, inputs, dt, ring, steps, fused=False, flag=None, what=""):
    """`steps` calls for the whole batch on `dev`, each compared with the restatement stepped controller by controller."""
    w = K.World(olib, variant, targets, fused, flag)
    want = K.run_batch(w, p, states, inputs, dt, ring, steps)
    cur = states.copy()
    with Uploaded(dev, targets) as up:
        for k in range(steps):
            tr = CharacterController.UpdateRaw(dev, p, cur, inputs, dt, ring, up, fused)
            compare(cur, tr, want[k][0], want[k][1], f"{what} step {k}")
    return want


def check_case(dev, olib, variant, case, fused=False, flag=None, what=""):
    w = K.World(olib, variant, case.targets, fused, flag)
    want = K.run_case(w, case)
    cur = np.array([case.start], dtype=CHARACTER_DTYPE)
    with Uploaded(dev, case.targets) as up:
        for k in range(len(case.inputs)):
            tr = CharacterController.UpdateRaw(dev, case.p, cur, np.array([case.input(k)], dtype=CHARACTER_INPUT_DTYPE), case.dt, case.ring, up, fused)
            compare(cur, tr, np.array([want[k][0]]), np.array([want[k][1]]), f"{what} {case.name} step {k}")
    return want


# ------------------------------------------------------------------------------------------------ cases
@pytest.mark.parametrize("case", K.host_cases(), ids=lambda c: c.name)
def test_the_host_cases(device, oracle_lib, case):
    check_case(device, oracle_lib, "", case)


def test_a_hit_at_exactly_max_distance(device, oracle_lib):
    want = check_case(device, oracle_lib, "", K.max_distance_case(lambda t: K.World(oracle_lib, "", t)))
    assert int(want[0][1]["ground_found"]) == 1


def test_ties(device, oracle_lib):
    slide = check_case(device, oracle_lib, "", K.slide_tie_case())
    assert int(slide[0][1]["chain_stop"][1]) == 4                      # the first TARGET won: the move slid (rays outer: stop 2)
    plane = check_case(device, oracle_lib, "", K.plane_tie_case())
    assert float(plane[0][1]["ground_normal"][0]) < 0                  # offset 1 came first: the SECOND target's normal


@pytest.mark.parametrize("n_targets", [0, 1, 3, 4])
@pytest.mark.parametrize("n", [1, 2, 65])
def test_batch_shapes(device, oracle_lib, n, n_targets):
    targets, states, inputs = K.batch_case(n, n_targets)
    targets = targets[:n_targets]
    p = K.params()
    want = check_batch(device, oracle_lib, "", targets, p, states, inputs, 0.05, CharacterController.Ring(18), 3, what=f"{n} x {n_targets}")
    if n == 65 and n_targets == 4:
        attempts = np.concatenate([t["chain_attempts"][:, 1] for _, t in want])
        assert {1, 3} <= set(attempts.tolist()) and int(states[1]["noclip"]) == 1


def test_a_batch_whose_first_chain_ends_at_different_attempts(device, oracle_lib):
    targets, states, inputs = K.chain1_batch()
    want = check_batch(device, oracle_lib, "", targets, K.params(), states, inputs, 1 / 60, CharacterController.Ring(18), 3, what="chain 1")
    assert {0, 1, 2, 3} <= {int(x) for _, t in want for x in t["chain_attempts"][:, 0]}      # (0: the noclip controller)


def test_ray_counts_past_the_chunk_and_the_wave(device, oracle_lib):
    p = K.params(height=1.0, radius=0.3)
    assert K.ray_counts(p) == (1, 37) == CharacterController.RayCounts(p)
    targets, states, inputs = K.batch_case(3, 4)
    states["position"][:, 1] += 0.25                                   # (the taller capsule stands at Height / 2 = 0.5)
    states["position"][:, 0] -= 0.15
    want = check_batch(device, oracle_lib, "", targets, p, states, inputs, 0.05, CharacterController.Ring(37), 3, what="74 rays")
    assert max(int(t["chain_attempts"][:, 1].max()) for _, t in want) >= 2


def test_dust2(device, oracle_lib):
    targets, states, inputs, dt = K.dust2_batch()
    want = check_batch(device, oracle_lib, "", targets, K.params(), states, inputs, dt, CharacterController.Ring(18), 6, what="dust2")
    assert any(int(t["ground_found"].max()) for _, t in want) and any(int(t["chain_stop"].max()) >= 2 for _, t in want)


def test_the_python_class(device, oracle_lib):
    case = {c.name: c for c in K.host_cases()}["wall_at_45_degrees"]
    want = K.run_case(K.World(oracle_lib, "", case.targets), case)
    meshes = [Mesh(device, t.vertices, t.indices) for t in case.targets]
    try:
        cc = CharacterController(case.start["position"], [meshes], [np.eye(4, dtype=np.float32)])
        cc.Velocity, cc.IsGrounded, cc.ActualStepSize = case.start["velocity"].copy(), True, np.float32(0.3)
        for k in range(len(case.inputs)):
            cc.Update(case.dt, case.inputs[k][0], case.inputs[k][1])
            assert K.same_state(cc.State(), want[k][0]) and K.same_trace(cc.LastTrace, want[k][1]), k
    finally:
        for m in meshes:
            m.Dispose()


def test_update_batch_steps_several_controllers_in_one_call(device, oracle_lib):
    """CharacterController.UpdateBatch: three objects built from the same meshes and matrices, states of their own."""
    targets, states, inputs = K.chain1_batch()
    pick = [0, 2, 4]
    want = K.run_batch(K.World(oracle_lib, "", targets), K.params(), states[pick], inputs[pick], 1 / 60, CharacterController.Ring(18), 3)
    meshes = [Mesh(device, t.vertices, t.indices) for t in targets]
    try:
        ccs = []
        for i in pick:
            cc = CharacterController(states[i]["position"], [meshes], [np.eye(4, dtype=np.float32)])
            cc.Velocity = states[i]["velocity"].copy()
            ccs.append(cc)
        for k in range(3):
            CharacterController.UpdateBatch(ccs, 1 / 60, [inputs[i]["move"] for i in pick], [bool(inputs[i]["jump"]) for i in pick])
            for j, cc in enumerate(ccs):
                assert K.same_state(cc.State(), want[k][0][j]) and K.same_trace(cc.LastTrace, want[k][1][j]), (k, j)
        other = CharacterController((0, 1, 0), [meshes[:1]], [np.eye(4, dtype=np.float32)])
        with pytest.raises(ValueError):
            CharacterController.UpdateBatch([ccs[0], other], 1 / 60, [(0, 0, 0)] * 2, [False] * 2)
    finally:
        for m in meshes:
            m.Dispose()


# ------------------------------------------------------------------------------------------------ numerics
def numerics_cases():
    by = {c.name: c for c in K.host_cases()}
    return K.numerics_cases() + [by["tilted_ground_normal"]]


@pytest.mark.parametrize("fused", [False, True], ids=["cross_rounded", "cross_fused"])
@pytest.mark.parametrize("flags", [(0, 0), (1, 1)], ids=["t0n0", "t1n1"])
def test_numerics_on_the_product_build(device, oracle_lib, flags, fused):
    default = device.transform_fma()
    try:
        device.set_transform_fma(*flags)
        for case in numerics_cases():
            check_case(device, oracle_lib, "", case, fused=fused, flag=flags[0], what=f"product, flags {flags}, fused {fused}")
    finally:
        device.set_transform_fma(*default)


@pytest.mark.parametrize("fused", [False, True], ids=["cross_rounded", "cross_fused"])
def test_numerics_on_a_sensitivity_build(mode, fused):
    dev, olib, variant = mode
    for case in numerics_cases():
        check_case(dev, olib, variant, case, fused=fused, what=variant)


# ------------------------------------------------------------------------------------------------ beside the renderer
CLEAR = (0.125, 0.25, 0.5, 1.0)


def test_an_update_between_two_draws_leaves_them_one_batch(device, oracle_lib):
    s = scenes.cfg1()
    d = s.draws[0]
    shifted = d.model.copy(); shifted[3, 0] = np.float32(0.25)
    targets, states, inputs = K.batch_case(2, 4)
    w = K.World(oracle_lib, "", targets)
    ring = CharacterController.Ring(18)
    want = K.run_batch(w, K.params(), states, inputs, 0.05, ring, 1)[0]
    Rasterizer.NearClip, Rasterizer.FarClip = 0.1, 1000.0
    win = MainWindow(device, s.width, s.height)
    prog = ShaderProgram(Program.Gouraud)
    mesh = Mesh(device, d.vertices, d.indices)
    try:
        with Uploaded(device, targets) as up:
            device.reset_stats()
            win.ClearDepthBuffer(); win.ClearColorBuffer(CLEAR)
            Rasterizer.RenderMesh(win, mesh, None, d.model, d.view, d.projection, prog.VertexShader, prog.FragmentShader, CullMode.None_, DepthTest.LessEqual, BlendMode.Alpha)
            cur = states.copy()
            tr = CharacterController.UpdateRaw(device, K.params(), cur, inputs, 0.05, ring, up)
            Rasterizer.RenderMesh(win, mesh, None, shifted, d.view, d.projection, prog.VertexShader, prog.FragmentShader, CullMode.None_, DepthTest.LessEqual, BlendMode.Alpha)
            c, z = win._read()
            assert device.stats()["flushes"] == 1
        compare(cur, tr, want[0], want[1], "between two draws")
    finally:
        mesh.Dispose()
    o = ob.OracleRenderer(s.width, s.height)
    o.set_state(0.1, 1000.0, 0)
    o.clear_depth(); o.clear_color(CLEAR)
    for m in (d.model, shifted):
        assert o.render_mesh(d.vertices, d.indices, m, d.view, d.projection, int(Program.Gouraud), None, None, int(CullMode.None_), int(DepthTest.LessEqual), int(BlendMode.Alpha)) == 0
    assert_frame_parity(c, z, o.color.copy(), o.depth.copy(), 1, "two draws around a character update")
    o.close()


def test_an_update_beside_a_frame_in_flight(device, oracle_lib):
    s = scenes.cfg1()
    targets, states, inputs = K.batch_case(65, 4)
    ring = CharacterController.Ring(18)
    want = K.run_batch(K.World(oracle_lib, "", targets), K.params(), states, inputs, 0.05, ring, 1)[0]
    was = device.pipelining()
    r = scenes.SceneRenderer(device, s)
    try:
        device.set_pipelining(1)
        with Uploaded(device, targets) as up:
            r.submit_frame()
            device.flush()
            syncs = device.sync_count()
            cur = states.copy()
            tr = CharacterController.UpdateRaw(device, K.params(), cur, inputs, 0.05, ring, up)
            assert device.sync_count() == syncs                       # no wait on the frame's stream
            c, z = r.window._read()
        compare(cur, tr, want[0], want[1], "beside a frame in flight")
    finally:
        device.set_pipelining(was)
        r.close()
    o = ob.OracleRenderer(s.width, s.height)
    rc, rz = o.render_scene(s)
    o.close()
    assert_frame_parity(c, z, rc, rz, 1, "cfg1 with a character update in flight")


def test_the_key_buffer_is_left_clean(device, oracle_lib):
    case = R.shape_case(65, 3)
    targets, states, inputs = K.batch_case(65, 4)
    with Uploaded(device, case.targets) as ray_targets, Uploaded(device, targets) as up:
        before = Physics.RaycastNearest(case.origins, case.directions, ray_targets, case.mask)
        pairs = Physics.RaycastBatch(case.origins, case.directions, ray_targets, case.mask)
        cur = states.copy()
        for _ in range(2):
            CharacterController.UpdateRaw(device, K.params(), cur, inputs, 0.05, CharacterController.Ring(18), up)
        after = Physics.RaycastNearest(case.origins, case.directions, ray_targets, case.mask)
        assert R.same_records(after, before) and int(before["found"].sum()) > 0
        assert R.same_records(Physics.RaycastBatch(case.origins, case.directions, ray_targets, case.mask), pairs)


# ------------------------------------------------------------------------------------------------ the staging threshold
RAY_TARGET_BYTES = 152                  # sizeof(RayTarget), csrc/swr_raycast.hip.h
STAGED_BYTES = 1 << 20                  # a call of up to this many bytes, up and down together, goes through the pinned block


def update_bytes(n, n_ring, n_targets):
    """what swr_character_update moves with the trace on: controllers | inputs | ring | targets up, states | traces down"""
    al = lambda b: (b + 15) & ~15
    up = al(n * CHARACTER_DTYPE.itemsize) + al(n * CHARACTER_INPUT_DTYPE.itemsize) + al(n_ring * 8) + al(n_targets * RAY_TARGET_BYTES)
    return up + al(n * CHARACTER_DTYPE.itemsize) + n * CHARACTER_TRACE_DTYPE.itemsize


def test_across_the_staging_threshold():
    """7000 controllers in one call are staged in pageable memory, the same controllers in two calls of 3500 in the pinned block: three
    steps from the same states, byte for byte the same states and traces after each; once more without the trace (the shorter
    download).  On a context of its own, so that the key buffer grows under this call: the 65-ray queries of
    test_the_key_buffer_is_left_clean return afterwards what they returned before.

    Two targets, the floor and the x wall: over the floor alone no slide ray can decide anything at any start height (chain 1 moves
    straight down onto it and its lowest ray starts ActualStepSize above the capsule's foot, chain 2 runs parallel to it), and every
    chain of the restatement stops with 1; with the wall the controllers near the corner stop with 2 from the second step on."""
    assert update_bytes(7000, 18, 1) == 1064304 and update_bytes(3500, 18, 1) == 532304       # (one target: 144 bytes fewer)
    assert update_bytes(7000, 18, 2) == 1064448 > STAGED_BYTES >= 532448 == update_bytes(3500, 18, 2)
    targets, states, inputs = K.batch_case(7000, 2)
    p, ring, half = K.params(), CharacterController.Ring(18), 3500
    case = R.shape_case(65, 3)
    dev = Device(0)
    try:
        with Uploaded(dev, case.targets) as ray_targets, Uploaded(dev, targets[:2]) as up:
            before = Physics.RaycastNearest(case.origins, case.directions, ray_targets, case.mask)
            pairs = Physics.RaycastBatch(case.origins, case.directions, ray_targets, case.mask)
            assert int(before["found"].sum()) > 0
            one, two, first = states.copy(), states.copy(), None
            grounded = stopped = 0
            for k in range(3):
                tr = CharacterController.UpdateRaw(dev, p, one, inputs, 0.05, ring, up)
                halves = [CharacterController.UpdateRaw(dev, p, two[a:a + half], inputs[a:a + half], 0.05, ring, up) for a in (0, half)]
                assert one.tobytes() == two.tobytes(), f"states differ after step {k}"
                assert tr.tobytes() == np.concatenate(halves).tobytes(), f"traces differ after step {k}"
                grounded += int(tr["ground_found"].sum())
                stopped += int((tr["chain_stop"] >= 2).any(axis=1).sum())
                if first is None:
                    first = one.copy()
            assert grounded > 0 and stopped > 0, (grounded, stopped)         # rays were cast, and some of them decided something
            bare = states.copy()
            assert CharacterController.UpdateRaw(dev, p, bare, inputs, 0.05, ring, up, trace=False) is None
            assert bare.tobytes() == first.tobytes()
            assert R.same_records(Physics.RaycastNearest(case.origins, case.directions, ray_targets, case.mask), before)
            assert R.same_records(Physics.RaycastBatch(case.origins, case.directions, ray_targets, case.mask), pairs)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ arguments
def test_arguments(device):
    lib, ctx = device._lib, device._ctx
    fn = lib.swr_character_update
    targets, states, inputs = K.batch_case(2, 1)
    p = K.params().reshape(1)
    ring = CharacterController.Ring(18)
    trace = np.zeros(2, dtype=CHARACTER_TRACE_DTYPE)
    with Uploaded(device, targets) as up:
        arr, kept, _ = Physics._targets(up)
        T, Pp, S, I_, Rg, Tr = C.addressof(arr), p.ctypes.data, states.ctypes.data, inputs.ctypes.data, ring.ctypes.data, trace.ctypes.data
        keep = states.copy()
        assert fn(ctx, Pp, S, I_, 0, 0.05, Rg, 18, T, 1, 0, Tr) == _native.SWR_OK
        assert fn(ctx, None, None, None, 0, 0.05, None, 0, None, 0, 0, None) == _native.SWR_OK
        assert states.tobytes() == keep.tobytes() and not trace.view(np.uint8).any()          # the empty calls write nothing
        for args in ((None, S, I_, 2, 0.05, Rg, 18, T, 1, 0, Tr), (Pp, None, I_, 2, 0.05, Rg, 18, T, 1, 0, Tr), (Pp, S, None, 2, 0.05, Rg, 18, T, 1, 0, Tr),
                     (Pp, S, I_, 2, 0.05, None, 18, T, 1, 0, Tr), (Pp, S, I_, 2, 0.05, Rg, 18, None, 1, 0, Tr), (Pp, S, I_, -1, 0.05, Rg, 18, T, 1, 0, Tr),
                     (Pp, S, I_, 2, 0.05, Rg, 18, T, -1, 0, Tr), (Pp, S, I_, 2, 0.05, Rg, -1, T, 1, 0, Tr), (Pp, S, I_, 2, 0.05, Rg, 17, T, 1, 0, Tr),
                     (Pp, S, I_, 2, 0.05, Rg, 18, T, 1, 1, Tr), (Pp, S, I_, 2, 0.05, Rg, 18, T, 1, 0x200, Tr), (Pp, S, I_, 2, 0.05, Rg, 18, T, 1, -1, Tr)):
            assert fn(ctx, *args) == _native.SWR_ERR_INVALID_ARG, args
        assert fn(None, Pp, S, I_, 2, 0.05, Rg, 18, T, 1, 0, Tr) == _native.SWR_ERR_INVALID_ARG
        assert states.tobytes() == keep.tobytes()
        for n, n_targets in ((65537, 1), (2, 65536), (65536, 64)):                          # refused before anything is read
            assert fn(ctx, Pp, S, I_, n, 0.05, Rg, 18, T, n_targets, 0, Tr) == _native.SWR_ERR_UNSUPPORTED
        assert b"2^24" in lib.swr_last_error(ctx) and b"65536 controllers" in lib.swr_last_error(ctx)
        huge = K.params(radius=40.0).reshape(1)                                              # 4 pi r / 0.1 = 5026 rays a ring
        assert fn(ctx, huge.ctypes.data, S, I_, 2, 0.05, Rg, 18, T, 1, 0, Tr) == _native.SWR_ERR_UNSUPPORTED
        wide = K.params(radius=15.0).reshape(1)                                              # 2 x 1885 rays an attempt
        wide_ring = np.zeros((CharacterController.RayCounts(wide)[1], 2), dtype=np.float32)
        assert wide_ring.shape[0] == 1885                                                    # n x rays > 2^22 with NO target: still refused
        assert fn(ctx, wide.ctypes.data, S, I_, 65536, 0.05, wide_ring.ctypes.data, 1885, None, 0, 0, Tr) == _native.SWR_ERR_UNSUPPORTED
        assert b"2^22 rays" in lib.swr_last_error(ctx)
        no_mesh = (_native.RayTarget * 1)()
        no_mesh[0].model[:] = arr[0].model[:]
        assert fn(ctx, Pp, S, I_, 2, 0.05, Rg, 18, C.addressof(no_mesh), 1, 0, Tr) == _native.SWR_ERR_INVALID_ARG
        assert fn(ctx, Pp, S, I_, 2, 0.05, Rg, 18, T, 1, 0, None) == _native.SWR_OK          # the trace is optional
    many = np.zeros(4096, dtype=CHARACTER_DTYPE)
    many["position"][:, 1] = 5.0
    CharacterController.UpdateRaw(device, K.params(), many, np.zeros(4096, dtype=CHARACTER_INPUT_DTYPE), 0.05, ring, [], trace=False)
    assert (many["position"][:, 1] < 5.0).all() and (many["actual_step_size"] == 0).all()      # 4096 controllers, no target: free fall
