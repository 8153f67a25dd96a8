"""The probe scenes and the reference of tests/program_probe_cases.py on the CPU.

fs_in_reference is what tests/test_gpu_program_probe.py holds the GPU to, word for word.  Here it is held, word for word, to the
oracle's oswr_interpolate of the same three outputs (from oswr_vertex_shader and, for clipped triangles, oswr_clip_triangle) and the
same weights, on every covered sample of `cells` and `clipped`: the GPU test's reference is then the oracle's arithmetic, not a
second opinion.  The scenes' conditions are asserted, not assumed; and five deliberately wrong restatements must each change a word,
or the probe table could not see that mistake in the kernel either.  NaN words are matched by any NaN (cull_edge_cases.same_words)."""
import ctypes as C

import numpy as np
import pytest

import program_probe_cases as PC
import shade_edge_scenes as S
from cull_edge_cases import same_words
from oracle import binding as ob

F32 = np.float32
ORACLE_FIELDS = (("clip", PC.FS_IN[0:4]), ("color", PC.FS_IN[4:8]), ("texcoord", PC.FS_IN[8:10]), ("normal", PC.FS_IN[10:13]),
                 ("screen", PC.FS_IN[13:15]), ("barycentric", PC.FS_IN[15:18]), ("world_normal", PC.FS_IN[18:21]))


@pytest.fixture(scope="module")
def lib():
    ob.build()
    return ob.load(variant="")


@pytest.fixture(scope="module")
def refs():
    """scene name -> (scene, [(ProbeTri, rect, fs_in_reference)])"""
    out = {}
    for s in (PC.cells(), PC.clipped()):
        out[s.name.split("_")[1]] = (s, [(t, r, PC.fs_in_reference(s, t.draw, t, r)) for t in PC.probe_tris(s) for r in t.rects()])
    return out


def oracle_outputs(lib, scene, t):
    """outputs[0..2] of one ProbeTri from the oracle's own vertex shader and clipper, ScreenCoords set as DrawTriangle sets them."""
    d = scene.draws[t.draw]
    v = np.ascontiguousarray(d.vertices)
    m, vw, p = (np.ascontiguousarray(a, dtype=F32).reshape(-1) for a in (d.model, d.view, d.projection))
    vin = (ob.OVertexOutput * 3)()
    for i, vi in enumerate(t.vid):
        lib.oswr_vertex_shader(v.ctypes.data + vi * v.dtype.itemsize, m.ctypes.data, vw.ctypes.data, p.ctypes.data, int(d.program), C.byref(vin[i]))
    poly, idx = vin, (0, 1, 2)
    if t.fan is not None:
        poly = (ob.OVertexOutput * 4)()
        assert lib.oswr_clip_triangle(F32(scene.near_clip), vin, poly) == t.n_poly
        idx = t.fan
    outs = [poly[idx[2]], poly[idx[1]], poly[idx[0]]]                     # outputs = { v2, v1, v0 }, Rasterizer.cs:367
    inv_w, inv_h = F32(1.0) / F32(scene.width - 1), F32(1.0) / F32(scene.height - 1)
    for i, o in enumerate(outs):
        o.screen[0], o.screen[1] = float(F32(t.tri.sx[i] * inv_w)), float(F32(t.tri.sy[i] * inv_h))
    return outs


@pytest.mark.parametrize("name", ["cells", "clipped"])
def test_reference_equals_the_oracle_word_for_word_on_every_covered_sample(lib, refs, name):
    lib.oswr_set_transform_fma(0, 0)
    scene, items = refs[name]
    n = 0
    for t, rect, r in items:
        a, b, c = oracle_outputs(lib, scene, t)
        for name_, mine in (("clip", "clip"), ("color", "color"), ("texcoord", "uv"), ("normal", "normal"), ("world_normal", "wn")):
            theirs = np.array([list(getattr(o, name_)) for o in (a, b, c)], dtype=F32)
            assert same_words(theirs, t.out[mine]), (scene.name, t.draw, t.index, t.fan, name_, "the three outputs differ")
        w = r["weights"]
        for i in range(w.shape[1]):
            o = ob.OVertexOutput()
            lib.oswr_interpolate(C.byref(a), C.byref(b), C.byref(c), float(w[0, i]), float(w[1, i]), float(w[2, i]), 1, C.byref(o))
            for field, names in ORACLE_FIELDS:
                want = np.array(list(getattr(o, field)), dtype=F32)
                got = np.array([r[nm][i] for nm, _ in names], dtype=F32)
                assert same_words(got, want), (scene.name, t.draw, t.index, t.fan, field, i, got, want)
            n += 1
    print(f"{name}: {n} covered samples equal the oracle in 21 words each")
    assert n >= (200 if name == "cells" else 50)


def test_sampling_restatement_equals_the_oracle_at_the_probes_uv(lib, refs):
    """texture_nearest / texture_bilinear of shade_edge_scenes at the uv the SAMPLE probes compute, against the oracle's two samplers."""
    scene, _ = refs["cells"]
    for _, tex, bilinear in PC.TEXTURE_SETTINGS[1:]:
        s = PC.with_texture(scene, tex, bilinear)
        fn = lib.oswr_texture_sample_bilinear if bilinear else lib.oswr_texture_sample
        t8 = np.ascontiguousarray(tex)
        n = 0
        for t in PC.probe_tris(s):
            for rect in t.rects():
                r = PC.fs_in_reference(s, t.draw, t, rect)
                uv = np.ascontiguousarray(r["sample_uv"])
                for i in range(uv.shape[0]):
                    want = np.zeros(4, dtype=F32)
                    fn(t8.ctypes.data, tex.shape[1], tex.shape[0], uv[i].ctypes.data, want.ctypes.data)
                    got = np.array([r["sample." + c][i] for c in "xyzw"], dtype=F32)
                    assert same_words(got, want), (bilinear, tex.shape, uv[i], got, want)
                    n += 1
        assert n >= 200


def test_scene_conditions(refs):
    for name, floor in (("cells", 200), ("clipped", 50)):
        scene, items = refs[name]
        _, count = PC.expected_planes(scene)
        assert count.max() == 1, f"{name}: a sample is covered by two triangles"
        # every probe group renders the same scene: its covered samples are the scene's
        covered = int((count > 0).sum())
        assert covered == sum(r["weights"].shape[1] for _, _, r in items)
        for g in PC.FS_IN_GROUPS:
            assert covered >= floor, (name, PC.group_names(g), covered)
        print(f"{name}: {covered} covered samples, {len(items)} (triangle, tile) pairs")
    scene, items = refs["cells"]
    zero = sum(int((r["weights"] == 0).any(axis=0).sum()) for _, _, r in items)
    assert zero >= 1, "no sample with a weight of exactly 0"
    short = {t.index for t, _, r in items if (r["len_sq"] <= F32(1e-6)).any()}
    assert PC.CANCEL_CELL in short, "no triangle whose world normal cancels (len_sq <= 1e-6)"
    assert any(np.isnan(r["normal.x"]).all() and not np.isnan(r["normal.y"]).any() for t, _, r in items if t.index == PC.NAN_CELL)
    assert len({tuple(t.out["clip"][:, 3]) for t, _, _ in items}) == 6 and all(len(set(t.out["clip"][:, 3])) == 3 for t, _, _ in items)
    assert all(len(set(t.out["clip"][:, 2])) == 3 for t, _, _ in items), "clip.z does not differ per vertex"
    # no two vertices of a triangle can change places unseen: three different screen x and y (but for the cancelling cell)
    assert all(len(set(t.tri.sx)) == 3 and len(set(t.tri.sy)) == 3 for t, _, _ in items if t.index != PC.CANCEL_CELL)
    assert all(len(set(t.tri.sx)) == 3 and len(set(t.tri.sy)) == 3 for t, _, _ in refs["clipped"][1])
    persp = np.concatenate([r["tex_coord.x"] for _, _, r in items])
    aff = np.concatenate([r["affine_tex_coord.x"] for _, _, r in items]).astype(F32)
    differ = int((persp.view(np.uint32) != aff.view(np.uint32)).sum())
    assert differ > persp.size // 2, (differ, persp.size)
    print(f"cells: {zero} samples with a zero weight, cells {sorted(short)} with len_sq <= 1e-6, perspective != affine in {differ} of {persp.size}")
    scene, items = refs["clipped"]
    sizes = sorted({t.n_poly for t, _, _ in items})
    assert sizes == [3, 4], sizes
    assert {t.fan for t, _, _ in items if t.n_poly == 4} == {(0, 1, 2), (0, 2, 3)}, "a 4-vertex polygon must draw both fan triangles"
    w = PC.wide()
    _, count = PC.expected_planes(w)
    assert count.max() == 1
    tiles = count.reshape(w.height // 16, 16, w.width // 16, 16).sum(axis=(1, 3))
    assert tiles.shape == (5, 9) and tiles.min() > 128, tiles.min()        # most of EVERY tile


def test_the_table_and_the_texts():
    assert [n for n, _ in PC.TABLE[:25]] == [n for n, _ in PC.FS_IN] and len(PC.GROUPS) == 10
    for g, grp in enumerate(PC.GROUPS):
        for _, expr in grp:
            assert expr in PC.NARROW[g] and expr in PC.PROBE_ALL
        assert f"case {g}:" in PC.PROBE_ALL
    seen = set()
    for g in range(PC.N_CONSTANT_GROUPS):
        seen |= set(PC.constants3_indices(g))
    assert seen == set(range(64))


HOST_MUTANTS = {            # mutant -> (scene, the words it must change)
    "clip_w_affine": ("cells", ["clip_position.w"]),
    "barycentric_z_from_sum": ("cells", ["barycentric.z"]),
    "screen_y_from_x": ("cells", ["screen_coords.y"]),
    "normal_from_world_normal": ("cells", ["normal.x", "normal.y", "normal.z"]),
    "world_normal_always_renormalised": ("cells", ["world_normal.x", "world_normal.y", "world_normal.z"]),
}


@pytest.mark.parametrize("mutant", PC.MUTANTS)
def test_host_mutants_turn_named_cases_red(refs, mutant):
    """A wrong restatement must change an expected word of its own member on the named scene, and of no other member."""
    name, members = HOST_MUTANTS[mutant]
    scene, items = refs[name]
    changed = {}
    for t, rect, r in items:
        m = PC.fs_in_reference(scene, t.draw, t, rect, mutant)
        for nm, _ in PC.TABLE:
            if not same_words(m[nm], r[nm]):
                changed[nm] = changed.get(nm, 0) + int(((m[nm].view(np.uint32) != r[nm].view(np.uint32)) & ~(np.isnan(m[nm]) & np.isnan(r[nm]))).sum())
    print(mutant, changed)
    assert changed and set(changed) <= set(members), changed
    assert all(nm in changed for nm in members) or mutant == "world_normal_always_renormalised", changed
    # the probe groups that hold those members are the ones a GPU frame would differ in
    groups = {g for g in range(len(PC.GROUPS)) if set(PC.group_names(g)) & set(changed)}
    assert groups and groups <= set(PC.FS_IN_GROUPS)


def test_shaded_still_shares_its_head_with_the_reference(refs):
    """Shaded (shade_edge_scenes) and fs_in_reference run the same Weights: clip.z and len_sq agree on `cells`."""
    scene, items = refs["cells"]
    d = scene.draws[0]
    stage = S.vertex_stage(d)
    for t, rect, r in items:
        sh = S.Shaded(d, stage, np.array(t.vid), t.tri, rect, None, False)
        assert same_words(sh.clip_z, r["clip_position.z"]) and same_words(sh.len_sq, r["len_sq"])
