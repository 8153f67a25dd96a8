"""The seven batched texture probes (swr_texture_sample, _sample_depth, _sample_lod, swr_texture_lod, swr_texture_cube_face,
_sample_cube, _sample_cube_depth; csrc/swr_texture.h) share one path through the context's scratch block: n records up, one kernel, one
or two arrays down, one host wait.  Here they run back to back on ONE context of its own, interleaved, with n = 1, 3 and 257 -- an input
block whose end is no multiple of 16, more than one block of threads, a scratch block that grows between calls and is then reused by a
smaller call with another layout -- and every result is compared word for word with the restatements the per-feature tests already
use (mipmap_cases, depth_texture_cases, cubemap_cases).  swr_sync_count rises by exactly one per call, and by none for n = 0."""
import numpy as np
import pytest

import cubemap_cases as K
import depth_texture_cases as D
import mipmap_cases as M
from softwarerenderer_amd import Device, Texture

pytestmark = pytest.mark.gpu
F32 = np.float32
COUNTS = (1, 3, 257, 3, 1)           # grows to 257, then the smaller calls reuse the grown block


def same_words(got, want, what):
    """32-bit words, NaN payloads included"""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype and g.itemsize == 4, (what, g.shape, w.shape, g.dtype, w.dtype)
    bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
    assert bad.size == 0, (what, f"{len(bad)} words differ, first at {tuple(bad[0])}: got {g[tuple(bad[0])]!r} want {w[tuple(bad[0])]!r}")


def first(pool, n, shift):
    """n records of a pool, cyclically, from record `shift` on"""
    return np.ascontiguousarray(np.roll(pool, -shift, axis=0)[np.arange(n) % len(pool)])


def test_the_seven_probes_interleaved_on_one_context():
    dev = Device(0)
    texels, plane = M.texture((4, 4)), D.depth_pool_plane(4, 4, 7)
    faces, words = K.colour_faces(2), K.depth_faces(2)
    tex, depth = Texture(dev, texels), Texture.Depth(dev, 4, 4, plane)
    cube, dcube = Texture.Cube(dev, faces), Texture.CubeDepth(dev, 2, words)
    try:
        tex.GenerateMipmaps()
        levels, L = M.chain(texels), M.full_levels(4, 4)
        assert tex.Levels == L == 3
        atlas, watlas, slots = K.atlas(faces), K.atlas(words), ((plane, False), None, None, None)
        uv_pool, dir_pool = D.lookup_uvs(4, 4), K.directions(2)
        lod_pool, grad_pool = M.lods_for(L), np.asarray(M.gradient_ladder(4, 4, L), dtype=F32)

        def sample(n, k):
            uv = first(uv_pool, n, k)
            same_words(tex.Sample(uv), M.sample_level(levels, False, 0, uv), ("sample", n))

        def sample_depth(n, k):
            uv, ref = first(uv_pool, n, k), D.lookup_refs(n, seed=k)
            got_d, got_s = depth.SampleDepth(uv, ref)
            same_words(got_d, D.depth_sample(slots, 0, uv), ("sample_depth, depth", n))
            same_words(got_s, D.shadow(slots, 0, uv, ref), ("sample_depth, shadow", n))

        def sample_lod(n, k):
            uv, lods = first(uv_pool, n, k), first(lod_pool, n, k)
            same_words(tex.SampleLod(uv, lods), M.sample_lod(levels, False, uv, lods), ("sample_lod", n))

        def lod(n, k):
            g = first(grad_pool, n, k)
            same_words(tex.Lod(g), M.lod(4, 4, g, L), ("lod", n))

        def cube_face(n, k):
            d = first(dir_pool, n, k)
            face, st = Texture.CubeFace(dev, d)
            want_face, want_st = K.cube_face(d)
            assert face.dtype == np.int32 and np.array_equal(face, want_face), ("cube_face, face", n)
            same_words(st, want_st, ("cube_face, st", n))

        def sample_cube(n, k):
            d = first(dir_pool, n, k)
            same_words(cube.SampleCube(d), K.sample_cube(atlas, False, d), ("sample_cube", n))

        def sample_cube_depth(n, k):
            d = first(dir_pool, n, k)
            ref = K.refs_for(watlas, d, seed=k)
            got_d, got_s = dcube.SampleCubeDepth(d, ref)
            same_words(got_d, K.depth_sample(watlas, d), ("sample_cube_depth, depth", n))
            same_words(got_s, K.shadow_cube(watlas, False, d, ref), ("sample_cube_depth, shadow", n))

        # neighbours in this order differ in their input record (8, 12 or 16 bytes) and in their outputs (one or two, 4 to 16 bytes)
        probes = [sample, cube_face, lod, sample_depth, sample_cube, sample_lod, sample_cube_depth]
        dev.sync()
        for round_no, n in enumerate(COUNTS):
            for j in range(len(probes)):
                probe = probes[(j + 3 * round_no) % len(probes)]          # another neighbour order in every round
                before = dev.sync_count()
                probe(n, 5 * round_no + j)
                assert dev.sync_count() - before == 1, (probe.__name__, n, "host waits of one probe")
        before = dev.sync_count()
        for probe in probes:
            probe(0, 0)                                                  # SWR_OK without touching the device
        assert dev.sync_count() == before, "an empty probe waited for the device"
        sample(3, 1)                                                     # ... and the context is as it was
    finally:
        for t in (tex, depth, cube, dcube):
            t.Dispose()
        dev.close()
