"""swr_raycast / swr_raycast_nearest (csrc/swr_raycast.hip.h) against the restatement of tests/raycast_cases.py, with no tolerance
anywhere: every record of every (ray, target) pair is compared -- found, target, triangle as integers, distance / point / normal as
32-bit words (cull_edge_cases.same_words: a NaN word of the reference must be a NaN word here).

  - the host cases of tests/test_raycast_host.py (KAT, face masks, inclusive edges, degenerate rays, +-0.0 on the plane), through
    swr_raycast and through Physics.Raycast;
  - triangle counts 0 .. 513 around the wave (64) and the block (256), the only hit in the last / the first triangle;
  - ties: coplanar twins with different normals at (0, 512), (64, 257) of 513 and (0, 1) of 2, +0.0 / -0.0 twins in both orders: the
    lower index wins and the record says so;
  - shape: 1 / 2 / 65 rays x 1 / 3 targets under models of their own, one with a zero normal matrix (NaN normals);
  - swr_raycast_nearest = the fold of the pairs in target order (a cross-target tie, a ray that misses everything, dust2);
  - dust2: 42 rays shaped like MoveWithSlide's against the 11 meshes (55 of the 462 pairs hit, every ray hits something);
  - numerics: the product build under the Transform flags (0,0) and (1,1), with and without SWR_RAY_CROSS_FUSED, and the five
    sensitivity builds against the oracle built alike, on the T = 65 case and the dust2 mesh with the most vertices;
  - the renderer is not disturbed: a query between two recorded draws leaves them one batch; a query beside a frame in flight
    (pipelining 1, flushed, not synchronised) returns the same hits, makes no host wait on the frame's stream, and the frame is
    still the oracle's;
  - the staging threshold: 7278 rays x 3 targets (1 048 496 bytes up and down: the largest such query staged in the pinned block) and
    7280 (1 048 784: pageable) against the reference, swr_raycast_nearest on the 7280, and a 65-ray query repeated after the key buffer
    has grown under it, on a context of its own;
  - arguments: the INVALID_ARG / UNSUPPORTED cases and the empty calls.

Device mutants (one change in a scratch copy of csrc/, built as a library of its own, this file and tests/test_gpu_raycast_edges.py
run once on it): profiles/r25_raycast_edges.md lists them, with the tests each turned red."""
import ctypes as C
import os

import numpy as np
import pytest

import raycast_cases as R
from oracle import binding as ob
from softwarerenderer_amd import Device, _native, scenes
from softwarerenderer_amd.rasterizer import (RAY_DTYPE, RAY_HIT_DTYPE, BlendMode, CullMode, DepthTest, MainWindow, Mesh, Physics, Program,
                                              Rasterizer, RaycastFaceMask, ShaderProgram)
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
    """The targets of a case as retained meshes on `dev`."""

    def __init__(self, dev, case):
        self.meshes = [Mesh(dev, t.vertices, t.indices) for t in case.targets]
        self.targets = [(m, t.model, t.normal_matrix) for m, t in zip(self.meshes, case.targets)]

    def __enter__(self):
        return self.targets

    def __exit__(self, *exc):
        for m in self.meshes:
            m.Dispose()


def check(dev, olib, variant, case, fused=False, flag=None, nearest=True, what=""):
    """Every pair of `case` on `dev` against the reference; with `nearest`, swr_raycast_nearest against the fold of the reference."""
    want = R.reference(olib, variant, case, fused=fused, flag=flag)
    with Uploaded(dev, case) as targets:
        got = Physics.RaycastBatch(case.origins, case.directions, targets, case.mask, fused)
        near = Physics.RaycastNearest(case.origins, case.directions, targets, case.mask, fused) if nearest else None
    assert got.shape == want.shape, (what, case.name)
    bad = [f"ray {r} target {t}: got {R.show(got[r, t])}\n{' ' * 18}want {R.show(want[r, t])}"
           for r in range(want.shape[0]) for t in range(want.shape[1]) if not R.same_records(got[r, t], want[r, t])]
    assert not bad, f"{what} {case.name}: {len(bad)} of {want.size} pairs differ:\n" + "\n".join(bad[:8])
    if nearest:
        fold = [R.fold_nearest(row) for row in want]
        badn = [f"ray {r}: got {R.show(near[r])}\n{' ' * 8}want {R.show(fold[r])}" for r in range(len(fold)) if not R.same_records(near[r], fold[r])]
        assert not badn, f"{what} {case.name}: nearest differs from the fold for {len(badn)} rays:\n" + "\n".join(badn[:8])
    return got, want


# ------------------------------------------------------------------------------------------------ cases
def test_the_host_cases(device, oracle_lib):
    for case in R.host_cases():
        got, want = check(device, oracle_lib, "", case)
        assert [bool(x) for x in got["found"].reshape(-1)] == list(case.expect), case.name
        with Uploaded(device, case) as targets:                       # ... and one by one through the reference's own signature
            for r in range(case.origins.shape[0]):
                hit, dist, point, normal = Physics.Raycast(case.origins[r], case.directions[r], targets[0][0], targets[0][1], RaycastFaceMask(case.mask))
                one = R.miss_record(0)
                one["found"], one["distance"], one["point"], one["normal"] = hit, dist, point, normal
                one["triangle"] = want[r, 0]["triangle"]              # (not part of Physics.Raycast's result)
                assert R.same_records(one, want[r, 0]), (case.name, r)


def test_physics_raycast_defaults_to_ignore_backfaces_and_refuses_a_singular_model(device):
    case = R.host_cases()[2]                                           # mask0_reversed_winding: hit with mask 0, missed by the default mask
    with Uploaded(device, case) as targets:
        mesh, model, _ = targets[0]
        assert Physics.Raycast(case.origins[0], case.directions[0], mesh, model, RaycastFaceMask.None_)[0] is True
        assert Physics.Raycast(case.origins[0], case.directions[0], mesh, model)[0] is False
        hit, dist, point, normal = Physics.Raycast(case.origins[0], case.directions[0], mesh, np.zeros((4, 4), np.float32), RaycastFaceMask.None_)
        assert (hit, dist) == (False, float(R.FLT_MAX)) and not point.any() and not normal.any()       # Physics.cs:30-36


@pytest.mark.parametrize("where", ["last", "first"])
@pytest.mark.parametrize("T", R.COUNTS)
def test_triangle_counts(device, oracle_lib, T, where):
    case, hit = R.count_case(T, where)
    got, _ = check(device, oracle_lib, "", case)
    assert int(got[0, 0]["found"]) == (1 if T else 0) and int(got[0, 0]["triangle"]) == (hit if T else -1)


def test_ties(device, oracle_lib):
    want_tri = {"twins_T513_0_512": 0, "twins_T513_64_257": 64, "twins_T2_0_1": 0, "zero_twins_plus_first": 0, "zero_twins_minus_first": 0}
    words = {}
    for case in R.tie_cases():
        got, _ = check(device, oracle_lib, "", case)
        assert int(got[0, 0]["triangle"]) == want_tri[case.name], case.name
        words[case.name] = int(got[0, 0]["distance"].reshape(1).view(np.uint32)[0])
    assert words["zero_twins_plus_first"] == 0x00000000 and words["zero_twins_minus_first"] == 0x80000000     # the winner's own word


@pytest.mark.parametrize("n_targets", [1, 3])
@pytest.mark.parametrize("n_rays", [1, 2, 65])
def test_shapes(device, oracle_lib, n_rays, n_targets):
    got, _ = check(device, oracle_lib, "", R.shape_case(n_rays, n_targets))
    if n_rays == 65 and n_targets == 3:
        hit = got[:, 1][got[:, 1]["found"] == 1]
        assert hit.size and np.isnan(hit["normal"]).all()              # the zero normal matrix: NaN words came back


def test_nearest_over_targets(device, oracle_lib):
    case = R.nearest_tie_case()
    check(device, oracle_lib, "", case)
    with Uploaded(device, case) as targets:
        near = Physics.RaycastNearest(case.origins, case.directions, targets, case.mask)
    assert [int(x) for x in near["target"]] == [0, 2, -1] and [int(x) for x in near["found"]] == [1, 1, 0]
    assert float(near[2]["distance"]) == float(R.FLT_MAX) and int(near[2]["triangle"]) == -1


def test_dust2(device, oracle_lib):
    got, _ = check(device, oracle_lib, "", R.dust2_case())
    assert got.shape == (42, 11) and int(got["found"].sum()) == 55 and bool(got["found"].any(axis=1).all())


# ------------------------------------------------------------------------------------------------ the staging threshold
RAY_TARGET_BYTES = 152                  # sizeof(RayTarget), csrc/swr_raycast.hip.h
STAGED_BYTES = 1 << 20                  # a query of up to this many bytes, up and down together, goes through the pinned block


def query_bytes(n_rays, n_targets, n_out):
    """what swr_raycast / swr_raycast_nearest move: align16(rays) + align16(targets) up, the records down"""
    al = lambda b: (b + 15) & ~15
    return al(n_rays * RAY_DTYPE.itemsize) + al(n_targets * RAY_TARGET_BYTES) + n_out * RAY_HIT_DTYPE.itemsize


@pytest.fixture(scope="module")
def own_device():
    """A context whose key buffer and staging blocks no earlier test has grown."""
    dev = Device(0)
    yield dev
    dev.close()


@pytest.fixture(scope="module")
def small_query(own_device, oracle_lib):
    """The 65-ray query of test_gpu_character.py::test_the_key_buffer_is_left_clean on the fresh context, taken BEFORE anything large."""
    case = R.shape_case(65, 3)
    with Uploaded(own_device, case) as targets:
        near = Physics.RaycastNearest(case.origins, case.directions, targets, case.mask)
        pairs = Physics.RaycastBatch(case.origins, case.directions, targets, case.mask)
    assert R.same_records(pairs, R.reference(oracle_lib, "", case)) and int(near["found"].sum()) > 0
    return case, near, pairs


@pytest.mark.parametrize("n_rays,pinned", [(7278, True), (7280, False)], ids=["largest_pinned", "pageable"])
def test_across_the_staging_threshold(own_device, oracle_lib, small_query, n_rays, pinned):
    """7278 rays x 3 targets per pair is the largest query of that shape that is staged in the pinned block; 7280 goes through the
    caller's memory.  Both against the reference, pair by pair; the small query taken before still returns the same records after the
    key buffer has grown under it."""
    assert RAY_DTYPE.itemsize == 24 and RAY_HIT_DTYPE.itemsize == 40
    total = query_bytes(n_rays, 3, 3 * n_rays)
    assert total == (1048496 if pinned else 1048784) and (total <= STAGED_BYTES) == pinned
    case = R.shape_case(n_rays, 3)
    want = R.reference(oracle_lib, "", case)
    assert int(want["found"].sum()) > 1000
    with Uploaded(own_device, case) as targets:
        got = Physics.RaycastBatch(case.origins, case.directions, targets, case.mask)
        near = Physics.RaycastNearest(case.origins, case.directions, targets, case.mask) if not pinned else None
    assert got.shape == want.shape
    bad = [(r, t) for r in range(want.shape[0]) for t in range(3) if not R.same_records(got[r, t], want[r, t])]
    assert not bad, f"{case.name}: {len(bad)} of {want.size} pairs differ, first {bad[:8]}"
    if near is not None:
        assert query_bytes(n_rays, 3, n_rays) <= STAGED_BYTES                    # (the same rays, 40 n bytes down: pinned)
        badn = [r for r in range(n_rays) if not R.same_records(near[r], R.fold_nearest(got[r]))]
        assert not badn, f"{case.name}: nearest is not the nearest of the pairs for {len(badn)} rays, first {badn[:8]}"
    small, near65, pairs65 = small_query
    with Uploaded(own_device, small) as targets:
        assert R.same_records(Physics.RaycastNearest(small.origins, small.directions, targets, small.mask), near65)
        assert R.same_records(Physics.RaycastBatch(small.origins, small.directions, targets, small.mask), pairs65)


# ------------------------------------------------------------------------------------------------ numerics
def numerics_cases():
    dust2 = R.dust2_case()
    big = max(range(len(dust2.targets)), key=lambda t: dust2.targets[t].vertices.shape[0])
    return [R.count_case(65, "last")[0], R.Case("dust2_largest_mesh", dust2.origins, dust2.directions, [dust2.targets[big]], 1),
            R.shape_case(65, 1)]


@pytest.mark.parametrize("fused", [False, True], ids=["cross_rounded", "cross_fused"])
@pytest.mark.parametrize("flags", [(0, 0), (1, 1)], ids=["t0n0", "t1n1"])
def test_numerics_on_the_product_build(device, oracle_lib, flags, fused):
    default = device.transform_fma()
    try:
        device.set_transform_fma(*flags)
        for case in numerics_cases():
            check(device, oracle_lib, "", case, fused=fused, flag=flags[0], what=f"product, flags {flags}, fused {fused}")
    finally:
        device.set_transform_fma(*default)


def test_the_two_cross_models_and_the_transform_flag_are_visible(oracle_lib):
    """(the numerics tests above distinguish something: each switch changes words of the reference on these cases)"""
    case = R.shape_case(65, 1)
    base = R.reference(oracle_lib, "", case)
    assert not R.same_records(R.reference(oracle_lib, "", case, fused=True), base)
    assert not R.same_records(R.reference(oracle_lib, "", case, flag=1), base)


@pytest.mark.parametrize("fused", [False, True], ids=["cross_rounded", "cross_fused"])
def test_numerics_on_a_sensitivity_build(mode, fused):
    dev, olib, variant = mode
    for case in numerics_cases():
        check(dev, olib, variant, case, fused=fused, what=variant)


# ------------------------------------------------------------------------------------------------ beside the renderer
CLEAR = (0.125, 0.25, 0.5, 1.0)


def test_a_query_between_two_draws_leaves_them_one_batch(device, oracle_lib):
    s = scenes.cfg1()
    d = s.draws[0]
    shifted = d.model.copy(); shifted[3, 0] = np.float32(0.25)
    case = R.count_case(65, "last")[0]
    want = R.reference(oracle_lib, "", case)
    Rasterizer.NearClip, Rasterizer.FarClip = 0.1, 1000.0
    win = MainWindow(device, s.width, s.height)
    prog = ShaderProgram(Program.Gouraud)
    mesh = Mesh(device, d.vertices, d.indices)
    try:
        with Uploaded(device, case) as targets:
            device.reset_stats()
            win.ClearDepthBuffer(); win.ClearColorBuffer(CLEAR)
            Rasterizer.RenderMesh(win, mesh, None, d.model, d.view, d.projection, prog.VertexShader, prog.FragmentShader, CullMode.None_, DepthTest.LessEqual, BlendMode.Alpha)
            got = Physics.RaycastBatch(case.origins, case.directions, targets, case.mask)
            Rasterizer.RenderMesh(win, mesh, None, shifted, d.view, d.projection, prog.VertexShader, prog.FragmentShader, CullMode.None_, DepthTest.LessEqual, BlendMode.Alpha)
            c, z = win._read()
            assert device.stats()["flushes"] == 1
        assert R.same_records(got, want)
    finally:
        mesh.Dispose()
    o = ob.OracleRenderer(s.width, s.height)
    o.set_state(0.1, 1000.0, 0)
    o.clear_depth(); o.clear_color(CLEAR)
    for m in (d.model, shifted):
        assert o.render_mesh(d.vertices, d.indices, m, d.view, d.projection, int(Program.Gouraud), None, None, int(CullMode.None_), int(DepthTest.LessEqual), int(BlendMode.Alpha)) == 0
    assert_frame_parity(c, z, o.color.copy(), o.depth.copy(), 1, "two draws around a ray query")
    o.close()


def test_a_query_beside_a_frame_in_flight(device, oracle_lib):
    s = scenes.cfg1()
    case = R.shape_case(65, 3)
    want = R.reference(oracle_lib, "", case)
    was = device.pipelining()
    r = scenes.SceneRenderer(device, s)
    try:
        device.set_pipelining(1)
        with Uploaded(device, case) as targets:
            r.submit_frame()
            device.flush()
            syncs = device.sync_count()
            got = Physics.RaycastBatch(case.origins, case.directions, targets, case.mask)
            assert device.sync_count() == syncs                       # no wait on the frame's stream
            c, z = r.window._read()
        assert R.same_records(got, want)
    finally:
        device.set_pipelining(was)
        r.close()
    o = ob.OracleRenderer(s.width, s.height)
    rc, rz = o.render_scene(s)
    o.close()
    assert_frame_parity(c, z, rc, rz, 1, "cfg1 with a ray query in flight")


# ------------------------------------------------------------------------------------------------ arguments
def test_arguments(device):
    lib, ctx = device._lib, device._ctx
    case = R.host_cases()[0]
    rays = np.zeros(1, dtype=RAY_DTYPE)
    rays["origin"], rays["direction"] = case.origins[0], case.directions[0]
    out = np.zeros(4, dtype=RAY_HIT_DTYPE)
    with Uploaded(device, case) as targets:
        arr, kept, _ = Physics._targets(targets)
        T, Rp, O = C.addressof(arr), rays.ctypes.data, out.ctypes.data
        for fn in (lib.swr_raycast, lib.swr_raycast_nearest):
            out[:] = 0
            out["found"] = 7
            assert fn(ctx, Rp, 0, T, 1, 1, O) == _native.SWR_OK and fn(ctx, Rp, 1, T, 0, 1, O) == _native.SWR_OK
            assert fn(ctx, None, 0, None, 0, 0, None) == _native.SWR_OK
            assert (out["found"] == 7).all()                           # the empty calls write nothing
            assert fn(ctx, Rp, 1, T, 1, 1, O) == _native.SWR_OK and int(out[0]["found"]) == 1 and int(out[1]["found"]) == 7
            for args in ((None, 1, T, 1, 1, O), (Rp, 1, None, 1, 1, O), (Rp, 1, T, 1, 1, None), (Rp, -1, T, 1, 1, O), (Rp, 1, T, -1, 1, O),
                         (Rp, 1, T, 1, 4, O), (Rp, 1, T, 1, 0x200, O), (Rp, 1, T, 1, -1, O)):
                assert fn(ctx, *args) == _native.SWR_ERR_INVALID_ARG, args
            assert fn(None, Rp, 1, T, 1, 1, O) == _native.SWR_ERR_INVALID_ARG
            for n_rays, n_targets in (((1 << 20) + 1, 1), (1, 65536), (1 << 20, 17)):      # refused before anything is read
                assert fn(ctx, Rp, n_rays, T, n_targets, 1, O) == _native.SWR_ERR_UNSUPPORTED
            assert b"2^24" in lib.swr_last_error(ctx)
        no_mesh = (_native.RayTarget * 1)()
        no_mesh[0].model[:] = arr[0].model[:]
        assert lib.swr_raycast(ctx, Rp, 1, C.addressof(no_mesh), 1, 1, O) == _native.SWR_ERR_INVALID_ARG
