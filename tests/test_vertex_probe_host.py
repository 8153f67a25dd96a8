"""The vertex probes, their reference and their scenes (tests/vertex_probe_cases.py) on the CPU.

tests/test_gpu_vertex_probe.py holds k_vertex_user, the program's k_setup and shade_user to fs_in_reference fed with the numpy
restatement of a vertex text.  Here that reference is held to the oracle: the restated helpers to oswr_nm_transform4 /
oswr_nm_transform_normal3 under all four oswr_set_transform_fma settings, the restated Renderer.VertexShader to oswr_vertex_shader
word for word (the NaN of a zero normal included), and data4 -- through the clipper and the interpolator -- to the oracle's own
Vector4 key (world_pos), on every covered sample of `clipped` and `cells`.  The scenes' conditions are asserted, not assumed, and
four deliberately wrong restatements must each turn their named planes red and no others."""
import ctypes as C

import numpy as np
import pytest

import program_probe_cases as PC
import vertex_probe_cases as VC
from cull_edge_cases import same_words
from oracle import binding as ob

F32 = np.float32
SETTINGS = [(0, 0), (1, 0), (0, 1), (1, 1)]


@pytest.fixture(scope="module")
def lib():
    ob.build()
    lib = ob.load(variant="")
    fp = C.POINTER(C.c_float)
    lib.oswr_nm_transform4.restype = None; lib.oswr_nm_transform4.argtypes = [fp, fp, fp]
    lib.oswr_nm_transform_normal3.restype = None; lib.oswr_nm_transform_normal3.argtypes = [fp, fp, fp]
    yield lib
    lib.oswr_set_transform_fma(0, 0)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


SPECIAL = [(0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (2.0 ** 70, -2.0 ** 70, 2.0 ** 70), (1e-40, 2e-40, -3e-40), (1e-20, 2e-20, -1e-20),
           (3e38, 3e38, 3e38), (float("nan"), 1.0, 0.0), (float("inf"), 1.0, -1.0)]


@pytest.mark.parametrize("tr,tn", SETTINGS)
def test_restated_helpers_equal_the_oracles_under_every_setting(lib, tr, tn):
    lib.oswr_set_transform_fma(tr, tn)
    rng = np.random.default_rng(11)
    vecs = [rng.normal(size=3) * 10.0 ** rng.uniform(-3, 3) for _ in range(40)] + SPECIAL
    n = 0
    for v in vecs:
        v4 = np.array([*v, rng.uniform(-2, 2)], dtype=F32)
        for m in (rng.uniform(-2, 2, 16).astype(F32), (rng.normal(size=16) * 1e3).astype(F32), np.eye(4, dtype=F32).reshape(-1)):
            want4, want3 = np.zeros(4, F32), np.zeros(3, F32)
            lib.oswr_nm_transform4(_fp(v4), _fp(m), _fp(want4))
            lib.oswr_nm_transform_normal3(_fp(v4), _fp(m), _fp(want3))
            assert same_words(VC.transform4(v4, m, bool(tr)), want4), (tr, tn, v4, m)
            assert same_words(VC.transform_normal3(v4[:3], m, bool(tn)), want3), (tr, tn, v4, m)
            # the fused and the unfused model differ somewhere: the flags are not decoration
            n += int(not same_words(VC.transform4(v4, m, True), VC.transform4(v4, m, False)))
    assert n > 10


def _oracle_vertex(lib, d, i):
    v = np.ascontiguousarray(d.vertices)
    m, vw, p = (np.ascontiguousarray(a, dtype=F32).reshape(-1) for a in (d.model, d.view, d.projection))
    o = ob.OVertexOutput()
    lib.oswr_vertex_shader(v.ctypes.data + i * v.dtype.itemsize, m.ctypes.data, vw.ctypes.data, p.ctypes.data, int(d.program), C.byref(o))
    return o


@pytest.mark.parametrize("name,settings", [("cells", SETTINGS), ("helpers", SETTINGS), ("slabs", [(0, 0), (1, 1)])])
def test_restated_renderer_vertex_shader_equals_the_oracles_word_for_word(lib, name, settings):
    scene = {"cells": VC.cells, "helpers": VC.helpers_scene, "slabs": VC.slabs}[name]()
    for tr, tn in settings:
        lib.oswr_set_transform_fma(tr, tn)
        nan = n = 0
        for d in scene.draws:
            mine = VC.renderer_stage(d, VC.nm_flags(tr, tn))
            for i in range(d.vertices.shape[0]):
                o = _oracle_vertex(lib, d, i)
                for theirs, key in (("clip", "clip"), ("color", "color"), ("texcoord", "uv"), ("normal", "normal"), ("world_normal", "wn")):
                    want = np.array(list(getattr(o, theirs)), dtype=F32)
                    assert same_words(mine[key][i], want), (name, tr, tn, i, key, mine[key][i], want)
                nan += int(np.isnan(mine["wn"][i]).all())
                n += 1
        if name == "helpers":
            assert nan == 3, "the zero normal's world normal is NaN in all three components, at its three vertices"
    assert n == sum(d.vertices.shape[0] for d in scene.draws)


def _as_oracle(stage, v):
    o = ob.OVertexOutput()
    for field, key in (("clip", "clip"), ("color", "color"), ("texcoord", "uv"), ("normal", "normal"), ("world_normal", "wn"),
                       ("world_pos", "data4")):
        getattr(o, field)[:] = [float(x) for x in stage[key][v]]
    o.has_data, o.interpolate = 1, 1
    return o


ORACLE_FIELDS = (("clip", PC.FS_IN[0:4]), ("color", PC.FS_IN[4:8]), ("texcoord", PC.FS_IN[8:10]), ("normal", PC.FS_IN[10:13]),
                 ("barycentric", PC.FS_IN[15:18]), ("world_normal", PC.FS_IN[18:21]), ("world_pos", PC.FS_IN[21:25]))


@pytest.mark.parametrize("name", ["clipped", "cells"])
def test_data4_through_clipper_and_interpolator_equals_the_oracles_vector4_key(lib, name):
    """ROUTE's sixteen outputs as the oracle's own VertexOutput (data4 as Data["WorldPos"], the reference's Vector4 key) through
    oswr_clip_triangle and oswr_interpolate, against probe_tris / fs_in_reference on every covered sample."""
    lib.oswr_set_transform_fma(0, 0)
    scene = {"clipped": VC.clipped, "cells": VC.cells}[name]()
    stages = [VC.route_stage(d) for d in scene.draws]
    n = differs = 0
    for t in PC.probe_tris(scene, VC.stage_of("route")):
        vin = (ob.OVertexOutput * 3)(*[_as_oracle(stages[t.draw], v) for v in t.vid])
        poly, idx = vin, (0, 1, 2)
        if t.fan is not None:
            poly = (ob.OVertexOutput * 4)()
            assert lib.oswr_clip_triangle(F32(scene.near_clip), vin, poly) == t.n_poly
            idx = t.fan
        a, b, c = poly[idx[2]], poly[idx[1]], poly[idx[0]]
        for o, key in ((a, 0), (b, 1), (c, 2)):
            assert same_words(np.array(list(o.world_pos), dtype=F32), t.out["data4"][key]), (name, t.draw, t.fan, "data4 at the outputs")
        for rect in t.rects():
            r = PC.fs_in_reference(scene, t.draw, t, rect)
            w = r["weights"]
            for i in range(w.shape[1]):
                o = ob.OVertexOutput()
                lib.oswr_interpolate(C.byref(a), C.byref(b), C.byref(c), float(w[0, i]), float(w[1, i]), float(w[2, i]), 1, C.byref(o))
                for field, names in ORACLE_FIELDS:
                    want = np.array(list(getattr(o, field)), dtype=F32)
                    got = np.array([r[nm][i] for nm, _ in names], dtype=F32)
                    assert same_words(got, want), (name, t.draw, t.index, t.fan, field, i, got, want)
                n += 1
            differs += int((r["data4.w"] != r["data4.z"]).sum())
    print(f"{name}: {n} covered samples equal the oracle in 21 words each, data4 included")
    assert n >= (200 if name == "cells" else 50) and differs == n


def test_the_tables_and_the_texts():
    outs = [o for o, _, _, _ in VC.ROUTE_TABLE]
    assert sorted(outs) == sorted(VC.VS_OUT) and len(outs) == 16
    assert {i for _, i, _, _ in VC.ROUTE_TABLE} == set(VC.VS_IN), "every input scalar is used"
    pairs = [(i, f) for _, i, f, _ in VC.ROUTE_TABLE]
    assert len(set(pairs)) == 16, "distinct (input scalar, factor) pairs"
    assert all(np.log2(f) == int(np.log2(f)) for _, _, f, _ in VC.ROUTE_TABLE), "power-of-two factors"
    assert len({c for _, _, _, c in VC.ROUTE_TABLE}) == 16
    for o, i, f, c in VC.ROUTE_TABLE:
        assert f"out.{o} = in.{i} * " in VC.ROUTE
    # ENV_ALL: every one of the table's scalars sits in exactly one case, in the slot env_entries names
    seen = []
    for k in range(VC.N_ENV_SELECTORS):
        for s, e in VC.env_entries(k):
            assert f"out.{s} = {VC.ENV_TABLE[e][1]};" in VC.ENV_ALL.split(f"case {k}:")[1].split("break;")[0]
            seen.append(e)
    assert seen == list(range(len(VC.ENV_TABLE))) and len(seen) == 48 + 49 + 64 + 1
    assert "world_normal" not in VC.ENV_ALL
    for block, k in VC.ENV_NARROW_SELECTORS.items():
        text = VC.env_narrow(k)
        assert "switch" not in text and all(VC.ENV_TABLE[e][1] in text for _, e in VC.env_entries(k))
        other = {"model": ("env.uniforms", "env.constants"), "uniforms": ("env.model", "env.constants"), "constants": ("env.model", "env.uniforms")}[block]
        assert not any(o in text for o in other) and "env.view" not in text and "env.projection" not in text
    # between them the fragment groups read every slot
    for groups, slots in ((VC.ENV_FRAGMENT_GROUPS, VC.ENV_SLOTS), (VC.MANY_FRAGMENT_GROUPS, [s for s, _ in VC.MANY_TABLE])):
        assert set(slots) <= {n for g in groups for n in PC.group_names(g)}
    assert VC.ZEROS.count("out.") == 1 and "out.clip_position" in VC.ZEROS


def test_scene_conditions():
    # ---- nothing is covered twice; ROUTE's outputs differ pairwise at every vertex
    for scene, stage in ((VC.cells(), "route"), (VC.clipped(), "route"), (VC.slabs(), "route"), (VC.helpers_scene(), "helpers"),
                         (VC.many_draws(), "many")):
        _, count = VC.expected(scene, stage)
        assert count.max() == 1 and count.sum() > 0, f"{scene.name}: a sample is covered by two triangles"
    s = VC.with_selectors(VC.env_scene(), 0, 1)
    assert VC.expected(s, "env_all")[1].max() == 1
    for scene in (VC.cells(), VC.clipped(), VC.slabs()):
        assert VC.route_outputs_differ(scene), scene.name
        # ... and is not the same at the three vertices of any triangle: a copy in the place of the clipper's lerp shows
        # (but in the cell whose normals are u, -u, -u)
        assert VC.outputs_differ_across_each_triangle(scene, but=(PC.CANCEL_CELL,) if scene is VC.cells() else ()), scene.name
    tris = PC.probe_tris(VC.clipped(), VC.stage_of("route"))
    assert sorted({t.n_poly for t in tris}) == [3, 4]
    assert {t.fan for t in tris if t.n_poly == 4} == {(0, 1, 2), (0, 2, 3)}

    # ---- slabs
    s = VC.slabs()
    assert [d.vertices.shape[0] for d in s.draws] == list(VC.SLAB_COUNTS) == [3, 63, 64, 65, 127, 128, 129, 193]
    bases = np.concatenate([[0], np.cumsum(VC.SLAB_COUNTS)[:-1]])
    assert all(b % 64 for b in bases[1:]), bases                        # vert_base = the running sum of n_verts (batch_geometry)
    tris = PC.probe_tris(s, VC.stage_of("route"))
    drawn = {(t.draw, t.vid) for t in tris}
    assert drawn == {(j, tri) for j, n in enumerate(VC.SLAB_COUNTS) for tri in VC.SLAB_TRIPLES[n]}, "a triangle of slabs is not drawn"
    covered = [sum(int(t.tri.cover(r)[0].sum()) for r in t.rects()) for t in tris]
    print(f"slabs: {len(tris)} triangles, covered samples per triangle {min(covered)} .. {max(covered)}")
    assert min(covered) >= 24
    phases = {64: set(), 128: set(), 192: set()}
    for n in VC.SLAB_COUNTS:
        triples = VC.SLAB_TRIPLES[n]
        flat = [v for t in triples for v in t]
        assert len(set(flat)) == len(flat) and max(flat) == n - 1 and min(flat) == 0, n
        for b in phases:
            phases[b] |= {p for p, t in (("a", (b - 2, b - 1, b)), ("b", (b - 1, b, b + 1))) if t in triples}
    assert phases == {64: {"a", "b"}, 128: {"a", "b"}, 192: {"a"}}, phases          # (191, 192, 193) needs a 194th vertex
    # every vertex, indexed or not, differs from every other of its draw in every position-independent attribute
    for d in s.draws:
        for member in ("uv", "normal", "color"):
            a = d.vertices[member]
            for c in range(a.shape[1]):
                assert len(np.unique(a[:, c])) == a.shape[0], (member, c)

    # ---- many_draws
    s = VC.many_draws()
    assert len(s.draws) == 70 and len({t.draw for t in PC.probe_tris(s, VC.stage_of("many"))}) == 70
    ident = [(bytes(d.uniforms), d.constants.tobytes()) for d in s.draws]
    assert len(set(ident)) == 69 and ident[69] == ident[64] and ident.index(ident[64]) == 64
    assert len({np.asarray(d.model).tobytes() for d in s.draws}) == 70
    consts = np.stack([d.constants for d in s.draws])
    assert not (consts == 0)[:, :3].any(), "no constant that could differ from another only in the sign of a zero"
    # ---- env_scene: 2 x 161 probe values, all different (the selectors' two places apart)
    vals = [VC.ENV_TABLE[e][2](d, 0) for d in VC.env_scene().draws for e in range(len(VC.ENV_TABLE) - 1)]
    assert len(set(float(v) for v in vals)) == 2 * 161
    # ---- helpers_scene: what the special normals give
    st = VC.helpers_stage(VC.helpers_scene().draws[0])
    kinds = list(VC.HELPER_NORMALS)
    u = {k: st["data4"][3 * i:3 * i + 3, :3] for i, k in enumerate(kinds)}
    assert np.isnan(u["zero"]).all()
    assert (u["huge"] == 0).all()
    assert not np.isfinite(u["denormal"]).any()
    assert np.allclose(np.linalg.norm(u["ordinary"].astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert np.allclose(np.linalg.norm(u["denormal_length"].astype(np.float64), axis=1), 1.0, atol=1e-3)


HOST_MUTANTS = {            # mutant -> (scene, the planes it must change)
    "data4_w_from_z": ("cells", ["data4.w"]),
    "normal_world_normal_swapped": ("cells", ["normal.x", "normal.y", "normal.z", "world_normal.x", "world_normal.y", "world_normal.z"]),
    "tex_y_from_wn_x": ("clipped", ["tex_coord.y"]),
    "data4_renormalised": ("clipped", ["data4.x", "data4.y", "data4.z"]),
}


@pytest.mark.parametrize("mutant", PC.VERTEX_MUTANTS)
def test_host_mutants_turn_named_planes_red_and_no_others(mutant):
    name, members = HOST_MUTANTS[mutant]
    scene = {"cells": VC.cells, "clipped": VC.clipped}[name]()
    good, _ = VC.expected(scene, "route")
    bad, _ = VC.expected(scene, "route", mutant=mutant)
    changed = {nm for nm, _ in PC.TABLE if not same_words(good[nm], bad[nm])}
    print(mutant, sorted(changed))
    assert changed == set(members), changed
    groups = {g for g in range(len(PC.GROUPS)) if set(PC.group_names(g)) & changed}
    assert groups and groups <= set(PC.FS_IN_GROUPS)


def test_default_probe_tris_is_unchanged_by_the_vertex_stage_argument():
    """probe_tris with the restated Renderer.VertexShader as its vertex stage gives the words of the default path (data4 = 0)."""
    for scene in (PC.cells(), PC.clipped()):
        a, ca = PC.expected_planes(scene)
        b, cb = VC.expected(scene, "renderer")
        assert np.array_equal(ca, cb)
        for nm, _ in PC.TABLE:
            assert same_words(a[nm], b[nm]), (scene.name, nm)
