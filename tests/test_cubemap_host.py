"""Cube maps without a GPU (include/swr.h): the numpy restatement of tests/cubemap_cases.py against hand-written
known answers and an independent float64 formulation through the face cameras, the degenerate directions, four wrong twins that each
fail a named case, the program texts through the run-time compile step, the new names in every binding, and the Python wrappers'
argument checks against a fake library."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import cubemap_cases as K
from softwarerenderer_amd import Texture, _native as N, hostmath as hm
from test_post_host import ROOT, validate

F32 = np.float32
AXES = np.array(hm.CUBE_FACE_AXIS, dtype=F32)


# ---- known answers ---------------------------------------------------------------------------------------------------------------
# per face: the direction of (s, t) = (1, 0.5) -- the middle of its right edge -- and of (0.5, 0) -- the middle of its top edge
RIGHT = [(1, 0, 1), (-1, 0, -1), (1, 1, 0), (1, -1, 0), (-1, 0, 1), (1, 0, -1)]
TOP = [(1, 1, 0), (-1, 1, 0), (0, 1, 1), (0, -1, -1), (0, 1, 1), (0, 1, -1)]
# ... which a tie hands to the earlier axis: the face that wins, where it differs from the face the edge was written for
TIE_WINNER = {(2, "right"): 0, (3, "right"): 0, (4, "right"): 1, (5, "right"): 0, (4, "top"): 2, (5, "top"): 2}


def test_centres_edges_and_corners_by_hand():
    face, st = K.cube_face(AXES)
    assert face.tolist() == [0, 1, 2, 3, 4, 5] and (st == 0.5).all()
    # just inside each edge's middle, so that the face is not in question: s (or t) is within 1e-6 of the edge
    for f in range(6):
        for name, table, want in (("right", RIGHT, (1.0, 0.5)), ("top", TOP, (0.5, 0.0))):
            d = AXES[f] + (np.array(table[f], dtype=F32) - AXES[f]) * F32(0.999999)
            face, st = K.cube_face(d)
            assert face == f and np.allclose(st, want, rtol=0, atol=1e-6), (f, name, face, st)
            # ON the edge the tie goes to the earlier axis, and the coordinate is exactly 0 or 1 in whichever face wins
            face, st = K.cube_face(np.array(table[f], dtype=F32))
            assert face == TIE_WINNER.get((f, name), f), (f, name, face)
            assert ((st == 0) | (st == 1) | (st == 0.5)).all() and ((st == 0) | (st == 1)).any(), (f, name, st)
    # the other two edges and the four corners of every face, from the two hand-written tables: left = the centre mirrored through
    # right, bottom through top, a corner the sum of two steps; approached from inside the face
    for f in range(6):
        right, top = np.array(RIGHT[f], dtype=F32) - AXES[f], np.array(TOP[f], dtype=F32) - AXES[f]
        for a, b in ((-1, 0), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1)):
            d = AXES[f] + (a * right + b * top) * F32(0.999999)
            face, st = K.cube_face(d)
            assert face == f and np.allclose(st, ((1 + a) / 2, (1 - b) / 2), rtol=0, atol=1e-6), (f, a, b, face, st)
    # the eight corners of the cube themselves all belong to an X face, at a corner of it
    for x in (-1, 1):
        for y in (-1, 1):
            for z in (-1, 1):
                face, st = K.cube_face(np.array([x, y, z], dtype=F32))
                assert face == (1 if x < 0 else 0)
                assert st.tolist() == [(z * x + 1) / 2, (1 - y) / 2], (x, y, z, st)
    # the face's left, right, top and bottom in the world: +X shows -Z .. +Z left to right and +Y at the top
    assert K.cube_face(np.array([1, 0.5, -0.25], dtype=F32))[1].tolist() == [0.375, 0.25]
    assert K.cube_face(np.array([0.5, 2, -1], dtype=F32))[1].tolist() == [0.625, 0.75]          # +Y: +X right, -Z... +Z at the top
    assert K.cube_face(np.array([0.5, -2, -1], dtype=F32))[1].tolist() == [0.625, 0.25]
    assert K.cube_face(np.array([0.5, 0.25, 4], dtype=F32)) [1].tolist() == [0.4375, 0.46875]   # +Z: -X to the right
    assert K.cube_face(np.array([0.5, 0.25, -4], dtype=F32))[1].tolist() == [0.5625, 0.46875]
    # the length does not matter, down to subnormals and up to 2^120
    for scale in (2.0 ** -140, 2.0 ** 120, 3.0):
        face, st = K.cube_face((K.lattice() * F32(scale)).astype(F32))
        f0, st0 = K.cube_face(K.lattice())
        assert np.array_equal(face, f0) and (np.array_equal(st, st0) or scale == 3.0)
        assert np.allclose(st, st0, rtol=0, atol=1e-6)


def test_a_cube_of_one_texel_and_the_nearest_texel():
    faces = K.colour_faces(1)
    a = K.atlas(faces)
    for filtered in (False, True):
        got = K.sample_cube(a, filtered, K.directions())
        face, _ = K.cube_face(K.directions())
        want = (faces[face, 0, 0].astype(F32) * K.INV255).astype(F32)
        # (under the bilinear filter the four taps are the one texel: c (1 - f) + c f is c to an ulp, and exactly c where f is 0 or 0.5)
        assert np.allclose(got, want, rtol=0, atol=2e-7) and (filtered or np.array_equal(got, want))
    # n = 4: s = 1 lands in the last texel, s = 0.5 in texel 2, a boundary 2 k / n - 1 in texel k
    st = np.array([(0.0, 0.0), (1.0, 1.0), (0.5, 0.25), (0.75, 0.999)], dtype=F32)
    x, y = K.nearest_xy(4, st)
    assert x.tolist() == [0, 3, 2, 3] and y.tolist() == [0, 3, 1, 3]


def test_the_clamped_footprint_at_a_face_edge():
    n = 4
    st = np.array([(0.0, 0.5), (1.0, 0.5), (0.125, 0.125), (0.5, 1.0)], dtype=F32)
    x0, x1, y0, y1, fx, fy = K.footprint(n, st)
    assert x0.tolist() == [0, 3, 0, 1] and x1.tolist() == [0, 3, 1, 2]
    assert y0.tolist() == [1, 1, 0, 3] and y1.tolist() == [2, 2, 1, 3]
    assert fx.tolist() == [0.5, 0.5, 0.0, 0.5] and fy.tolist() == [0.5, 0.5, 0.0, 0.5]
    # at s = 0 both taps are column 0 of THIS face: the colour of the neighbouring face never enters
    faces = np.zeros((6, n, n, 4), dtype=np.uint8)
    faces[0, :, 0] = 255                                  # +X's left column; its neighbour there is +Z's right column, left black
    got = K.sample_cube(K.atlas(faces), True, np.array([1.0, 0.0, -1.0 + 1e-7], dtype=F32))
    assert K.cube_face(np.array([1.0, 0.0, -1.0 + 1e-7], dtype=F32))[0] == 0 and np.allclose(got, 1.0, rtol=0, atol=2e-7)
    got = K.sample_cube(K.atlas(faces), True, np.array([1.0 - 1e-6, 0.0, -1.0], dtype=F32))      # across the edge: -Z's right column
    assert K.cube_face(np.array([1.0 - 1e-6, 0.0, -1.0], dtype=F32))[0] == 5 and (got == 0.0).all(), "the seam is the defined result"


def test_every_degenerate_direction_is_the_centre_of_face_0():
    face, st = K.cube_face(K.degenerate())
    assert (face == 0).all() and (st == 0.5).all()
    a = K.atlas(K.colour_faces(3))
    want = (a[1, 1].astype(F32) * K.INV255).astype(F32)
    assert (K.sample_cube(a, False, K.degenerate()) == want).all()
    words = K.atlas(K.depth_faces(3, finite=True))
    assert (K.depth_sample(words, K.degenerate()) == words[1, 1]).all()


def test_the_restatement_meets_the_face_cameras_in_float64():
    rng = np.random.default_rng(27)
    worst, n = 0.0, 0
    for v in rng.normal(size=(2000, 3)).astype(F32):
        a = np.sort(np.abs(v))
        if a[2] - a[1] < 1e-3 * a[2]:
            continue                                      # (a tie: the float64 side may pick the neighbouring face)
        face, st = K.cube_face(v)
        x, y, w = K.texel_of_direction_f64(int(face), v, 1)
        assert w > 0, (v, face, w)
        worst = max(worst, abs(x - st[0]), abs(y - st[1]))
        n += 1
    print(f"{n} directions, restatement against the cameras {worst:.3e}")
    assert n > 1900 and worst <= 1e-5
    # cube_face_view is create_look_at for an eye where eye + axis - eye is the axis, and translates by the eye
    for f in range(6):
        eye = np.array([0.5, -2.0, 4.0], dtype=F32)
        want = hm.create_look_at(eye, eye + AXES[f], np.array(hm.CUBE_FACE_UP[f], dtype=F32))
        assert np.array_equal(hm.cube_face_view(f, eye), want), f
        view = np.zeros(16, dtype=F32)
        assert ctypes.CDLL(N.LIB_PATH).swr_cube_face_view(f, eye.ctypes.data_as(ctypes.c_void_p), view.ctypes.data_as(ctypes.c_void_p)) == 0
        assert np.array_equal(view.reshape(4, 4), want), f
    with pytest.raises(ValueError):
        hm.cube_face_view(6, (0, 0, 0))
    assert ctypes.CDLL(N.LIB_PATH).swr_cube_face_view(-1, None, None) == N.SWR_ERR_INVALID_ARG


# ---- the wrong twins -------------------------------------------------------------------------------------------------------------
def test_each_wrong_twin_fails_a_named_case():
    right = lambda d: K.cube_face(np.array(d, dtype=F32))
    # GL's mirrored table: +X at z = 0.5 is right of the centre here, left of it there
    assert right((1, 0, 0.5))[1].tolist() == [0.75, 0.5] and K.cube_face(np.array((1, 0, 0.5), dtype=F32), mirrored=True)[1].tolist() == [0.25, 0.5]
    # `>` for `>=`: the tie x == y must go to X, the strict form sends it on (to Y, and x == y == z to Z)
    assert right((1, 1, 0))[0] == 0 and K.cube_face(np.array((1, 1, 0), dtype=F32), strict=True)[0] == 2
    assert right((1, 1, 1))[0] == 0 and K.cube_face(np.array((1, 1, 1), dtype=F32), strict=True)[0] == 4
    # -0 to the negative face: a major component cannot be -0 (then all three are zero), so the case that tells is the origin
    # written with negative zeros, which is face 0 like every degenerate direction
    zeros = np.array((-0.0, -0.0, -0.0), dtype=F32)
    assert np.signbit(zeros).all() and right(zeros)[0] == 0 and K.cube_face(zeros, negative_zero=True)[0] == 1
    d = np.array((1.0, 0.5, -0.0), dtype=F32)
    assert np.array_equal(K.cube_face(d)[1], K.cube_face(d, negative_zero=True)[1])          # (off the origin the twin is harmless)
    # wrap instead of clamp: at s = 0 the second tap must stay in column 0; wrapped it would be column n - 1
    faces = np.zeros((6, 4, 4, 4), dtype=np.uint8)
    faces[0, :, 3] = 255
    d = np.array([1.0, 0.0, -1.0], dtype=F32)
    assert (K.level_sample(K.atlas(faces), True, d) == 0).all() and (K.level_sample(K.atlas(faces), True, d, wrap=True) == F32(0.5)).all()


# ---- programs, bindings ----------------------------------------------------------------------------------------------------------
def test_every_program_text_compiles_and_the_contracts_stay_apart():
    lib = N.load()
    log = ctypes.create_string_buffer(1 << 14)
    for name, (vertex, fragment) in K.FRAGMENT_TEXTS.items():
        if vertex is None:
            rc = lib.swr_program_validate(fragment.encode(), log, len(log))
        else:
            rc = lib.swr_program_validate_vf(vertex.encode(), fragment.encode(), log, len(log))
        assert rc == N.SWR_OK, (name, log.value.decode())
    for name, text in K.POST_TEXTS.items():
        rc, msg = validate(lib, text)
        assert rc == N.SWR_OK, (name, msg)
    # the fragment contract does not gain the swr_post_* names, nor the post contract the bare ones
    assert lib.swr_program_validate(K.FRAGMENT_PROBE.replace("swr_sample_cube(", "swr_post_sample_cube(").encode(), log, len(log)) == N.SWR_ERR_INVALID_ARG
    assert validate(lib, K.POST_PROBE.replace("swr_post_shadow_cube(", "swr_shadow_cube("))[0] == N.SWR_ERR_INVALID_ARG


def test_the_new_names_are_in_every_binding():
    lib, raw = N.load(), ctypes.CDLL(N.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "swr.h")).read()
    cs = open(os.path.join(ROOT, "csharp", "RasterizerNative.cs")).read()
    hpp = open(os.path.join(ROOT, "softwarerenderer_amd", "cpp", "Rasterizer.hpp")).read()
    smoke = open(os.path.join(ROOT, "tests", "c", "cubemap_smoke.c")).read()
    for name in K.NEW_EXPORTS:
        assert name in N.EXPORTS and hasattr(raw, name) and getattr(lib, name).argtypes is not None, name
        assert re.search(r"\bint\s+%s\(" % name, header), name
        assert re.search(r"extern int %s\(" % name, cs), name
        assert name + "(" in hpp, name
    assert "#define SWR_ABI_VERSION 3" in header
    for method in ("Cube", "CubeTarget", "CubeDepth", "IsCube", "UpdateFaceFrom", "UpdateFaceFromDepth", "UpdateFaceFromPost", "ReadFace",
                   "SampleCube", "SampleCubeDepth", "CubeFace"):
        assert hasattr(Texture, method), method
        assert re.search(r"\b%s\(" % method, hpp), method
    assert hasattr(hm, "cube_face_view")
    tex = cs[cs.index("class TextureNative"):]
    for method in ("public static TextureNative CreateCube(", "public static TextureNative CreateCubeDepth(", "public void UpdateFaceFrom(",
                   "public void UpdateFaceFromDepth(", "public static Matrix4x4 CubeFaceView("):
        assert method in tex, method
    for helper in ("swr_cube_face", "swr_sample_cube", "swr_sample_cube_level", "swr_sample_cube_lod", "swr_cube_texel", "swr_cube_size",
                   "swr_sample_cube_depth", "swr_shadow_cube"):
        assert helper in header and "swr_post_" + helper[4:] in header, helper
        for unit in ("swr_program.hip.h", "swr_post.hip.h"):
            text = open(os.path.join(ROOT, "softwarerenderer_amd", "csrc", unit)).read()
            assert (helper if unit == "swr_program.hip.h" else "swr_post_" + helper[4:]) + "(" in text, (unit, helper)
    for name in ("swr_texture_create_cube", "swr_texture_sample_cube", "swr_texture_sample_cube_depth", "swr_cube_face_view", "swr_texture_readback_face"):
        assert name in smoke, name
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "cubemap_smoke.mk" in entry and "tests/c/cubemap_smoke" in open(os.path.join(ROOT, ".gitignore")).read()
    # the pins the layout answers to: the slot and the header did not grow
    device = open(os.path.join(ROOT, "softwarerenderer_amd", "csrc", "swr_device.h")).read()
    assert "struct TextureSlot { const uint8_t* texels; int w, h; };" in device and "sizeof(TextureHeader) == 144" in device


class _FakeDevice:
    """records the calls of the new entry points; every one answers SWR_OK"""

    def __init__(self):
        self.calls = []

        def rec(name):
            def f(*a):
                self.calls.append((name, a))
                return 0
            return f
        self._ctx = 1234
        self._lib = types.SimpleNamespace(**{n: rec(n) for n in K.NEW_EXPORTS + ("swr_texture_format",)})

    def _ck(self, rc):
        assert rc == 0


def test_the_python_wrappers_check_their_arguments_before_the_library_is_called():
    dev = _FakeDevice()
    for bad in (np.zeros((5, 4, 4, 4)), np.zeros((6, 4, 3, 4)), np.zeros((6, 4, 4, 3)), np.zeros((6, 4, 4)), np.zeros((6, 0, 0, 4))):
        with pytest.raises(ValueError):
            Texture.Cube(dev, bad)
    with pytest.raises(ValueError):
        Texture.CubeDepth(dev, 4, np.zeros((6, 4, 3)))
    assert dev.calls == []
    cube = Texture.Cube(dev, np.zeros((6, 4, 4, 4), dtype=np.uint8))
    assert (cube.Width, cube.Height) == (4, 24) and dev.calls[-1][0] == "swr_texture_create_cube" and dev.calls[-1][1][2] == 4
    target, depth = Texture.CubeTarget(dev, 8), Texture.CubeDepth(dev, 2)
    assert dev.calls[-2][1][1] is None and (target.Width, target.Height) == (8, 48)
    assert dev.calls[-1][0] == "swr_texture_create_cube_depth" and dev.calls[-1][1][1] is None and depth.Height == 12
    made = len(dev.calls)
    for face in (-1, 6, 99):
        for call in (lambda: cube.UpdateFaceFrom(face, None), lambda: cube.UpdateFaceFromDepth(face, None), lambda: cube.UpdateFaceFromPost(face, None, None),
                     lambda: cube.ReadFace(face)):
            with pytest.raises(ValueError):
                call()
    for level in (-1, 3, 40):
        with pytest.raises(ValueError):
            cube.ReadFace(0, level)
    for bad in (np.zeros((5, 2)), np.zeros(()), np.zeros((3, 4))):
        with pytest.raises(ValueError):
            cube.SampleCube(bad)
        with pytest.raises(ValueError):
            depth.SampleCubeDepth(bad, 0.0)
        with pytest.raises(ValueError):
            Texture.CubeFace(dev, bad)
    assert len(dev.calls) == made, "a refused wrapper call reached the library"
    # what does go through: n x (x, y, z, lod) records, the lod broadcast
    cube.SampleCube(np.ones((7, 2, 3)), 1.5)
    name, args = dev.calls[-1]
    assert name == "swr_texture_sample_cube" and args[3] == 14
    face, st = Texture.CubeFace(dev, np.ones((5, 3)))
    assert face.shape == (5,) and face.dtype == np.int32 and st.shape == (5, 2) and dev.calls[-1][1][2] == 5
