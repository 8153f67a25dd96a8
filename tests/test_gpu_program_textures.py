"""User programs with four texture slots on the GPU (swr_program_set_texture).

Every test lets a run-time compiled program write what it read of its slots, raw, into the frame (the texts of
tests/program_texture_cases.py: BlendMode.None, no sample covered twice) and compares 32-bit words with the numpy twin, whose sampler
is the oracle's.  No tolerance: swr_sample(env, slot, uv) is swr::texture_fetch, the function swr_sample(env, uv) calls.  A NaN word
is matched by any NaN.  Every frame's fragments_written equals the twin's count, which is positive: an empty frame cannot pass."""
import dataclasses

import numpy as np
import pytest

import program_probe_cases as PC
import program_texture_cases as T
import render_to_texture_cases as RT
from softwarerenderer_amd import _native as N
from softwarerenderer_amd.rasterizer import MainWindow, Rasterizer, ShaderProgram, Texture
from test_gpu_program_probe import assert_words
from test_gpu_program_probe import render as probe_render

pytestmark = pytest.mark.gpu
F32 = np.float32
TEXTURES = dict(T.TEXTURES, **{"5x7": PC.TEX_5x7})


@pytest.fixture(scope="module")
def programs(device):
    """name -> program id: every text is compiled once per module, when a test first asks for it."""
    class Compiled(dict):
        def __missing__(self, name):
            self[name] = (device.compile_program(PC.PROBE_ALL, vertex_source=T.VERTEX) if name == "VERTEX"
                          else device.compile_program(T.TEXTS[name]))
            return self[name]
    ids = Compiled()
    yield ids
    for pid in ids.values():
        device.destroy_program(pid)


@pytest.fixture(scope="module")
def live(device):
    """(name, bilinear) -> a Texture of the device with those texels under that filter, made on first use."""
    class Live(dict):
        def __missing__(self, key):
            t = Texture(device, TEXTURES[key[0]])
            t.SetBilinear(key[1])
            self[key] = t
            return t
    made = Live()
    yield made
    for t in made.values():
        t.Dispose()


def bind(live, spec, bilinear=False):
    """spec: four entries, None, a texture's name or (name, bilinear) -> (the live Textures, the twin's slots)."""
    keys = [None if s is None else (s, bilinear) if isinstance(s, str) else tuple(s) for s in spec]
    return tuple(None if k is None else live[k] for k in keys), tuple(None if k is None else (TEXTURES[k[0]], k[1]) for k in keys)


def render(dev, scene, pid, per_draw, before=None, after_recording=None):
    """One frame of `scene` as ONE batch under user program `pid`; draw j is recorded after a set_program_constants of per_draw[j][0]
    and, for slots 1 .. 3, a set_program_texture of per_draw[j][1][slot]; per_draw[j][1][0] is its `texture` argument.
    before(j) runs ahead of that.  Returns (colour, stats)."""
    w = MainWindow(dev, scene.width, scene.height)
    Rasterizer.NearClip, Rasterizer.FarClip = scene.near_clip, scene.far_clip
    w.ClearDepthBuffer(); w.ClearColorBuffer(scene.clear_color)
    dev.reset_stats()
    for j, d in enumerate(scene.draws):
        if before is not None:
            before(j, w)
        k, tex = per_draw[j]
        dev.set_program_constants(pid, k)
        for s in (1, 2, 3):
            dev.set_program_texture(pid, s, tex[s])
        prog = ShaderProgram(pid, d.uniforms, tex[0])
        Rasterizer.RenderMesh(w, d.vertices, d.indices, d.model, d.view, d.projection, prog.VertexShader, prog.FragmentShader,
                              d.cull, d.depth_test, d.blend)
    if after_recording is not None:
        after_recording()
    c, _ = w._read(True, False)
    return c, dev.stats()


def check(dev, pid, scene, name, draws, what, **kw):
    """draws[j] = (constants, live Textures, twin slots) of draw j.  The frame equals the twin's; returns it."""
    want, n = T.twin_frame(scene, name, [(k, slots) for k, _, slots in draws])
    c, st = render(dev, scene, pid, [(k, tex) for k, tex, _ in draws], **kw)
    assert_words(c, want, what)
    assert st["fragments_written"] == n > 0, (what, st["fragments_written"], n)
    return c


# ---- 1. four slots, four different answers
FOUR_SPEC = ("12x20", "8x8", "5x3", "1x1")


@pytest.mark.parametrize("bilinear", [False, True], ids=["nearest", "bilinear"])
def test_four_slots_give_four_different_answers(device, programs, live, bilinear):
    s = PC.wide()
    tex, slots = bind(live, FOUR_SPEC, bilinear)
    swapped_tex, swapped_slots = (tex[0], tex[2], tex[1], tex[3]), (slots[0], slots[2], slots[1], slots[3])
    for group in (0, 1):
        k = T.constants(s.width, s.height, group=group)
        first = check(device, programs["FOUR"], s, "FOUR", [(k, tex, slots)], f"four/{bilinear}/group{group}")
        # "every slot reads slot 0" is another frame
        wrong, _ = T.twin_frame(s, "FOUR", [(k, slots)], twin=T.four_all_slot0)
        assert (wrong.view(np.uint32) != first.view(np.uint32)).any()
        second = check(device, programs["FOUR"], s, "FOUR", [(k, swapped_tex, swapped_slots)], f"four/{bilinear}/group{group}/swapped")
        assert (first.view(np.uint32) != second.view(np.uint32)).any(), "slots 1 and 2 exchanged: the same frame"


# ---- 2. unbound and out of range
@pytest.mark.parametrize("slot", [1, 3, -1, 4, 1000])
def test_an_unbound_or_out_of_range_slot_has_no_texture(device, programs, live, slot):
    s = T.tiles(2, 64, 32)
    tex, slots = bind(live, ("12x20", None, "5x3", None))
    for mode, value in ((T.SAMPLE, 1.0), (T.TEXEL, 1.0), (T.SIZE, 0.0)):
        for group in (0, 1):
            k = T.constants(s.width, s.height, group=group, mode=mode, slot=slot)
            c = check(device, programs["PROBE"], s, "PROBE", [(k, tex, slots)] * 2, f"unbound/slot{slot}/mode{mode}/group{group}")
            covered = T.coverage(s)[1] > 0
            assert (c[covered][:, :3] == value).all()          # ones; size (0, 0), has_texture false


@pytest.mark.parametrize("mode", [T.SAMPLE, T.TEXEL, T.SIZE], ids=["sample", "texel", "size"])
def test_a_slot_computed_per_pixel(device, programs, live, mode):
    s = PC.wide()
    tex, slots = bind(live, ("12x20", None, ("5x3", True), None))
    for group in (0, 1):
        k = T.constants(s.width, s.height, group=group, mode=mode, slot=T.PER_PIXEL)
        check(device, programs["PROBE"], s, "PROBE", [(k, tex, slots)], f"per_pixel/mode{mode}/group{group}")


# ---- 3. swr_texel and swr_texture_size
@pytest.mark.parametrize("slot", [0, 2])
@pytest.mark.parametrize("setting", [n for n, _, _ in PC.TEXTURE_SETTINGS])
def test_texel_and_size_under_every_texture_setting(device, programs, live, setting, slot):
    """The texel walk runs x over -2 .. w + 1 and y over -2 .. h + 1; the size is positive whatever the filter and the layout (the
    raw words env.tex_w / env.tex_h are not: tests/test_gpu_program_probe.py pins them)."""
    name = {"none": None, "nearest12x20": ("12x20", False), "bilinear12x20": ("12x20", True), "bilinear5x7": ("5x7", True)}[setting]
    spec = [None] * 4
    spec[slot] = name
    tex, slots = bind(live, spec)
    s = PC.wide()
    w, h = (0, 0) if name is None else TEXTURES[name[0]].shape[1::-1]
    for mode in (T.TEXEL, T.SIZE):
        for group in (0, 1):
            k = T.constants(s.width, s.height, group=group, mode=mode, slot=slot, texel_span=(max(w, 1) + 4, max(h, 1) + 4))
            c = check(device, programs["PROBE"], s, "PROBE", [(k, tex, slots)], f"texel_size/{setting}/slot{slot}/mode{mode}/group{group}")
            if mode == T.SIZE and group == 0:
                covered = T.coverage(s)[1] > 0
                assert (c[covered][:, 0] == w).all() and (c[covered][:, 1] == h).all() and (c[covered][:, 2] == (name is not None)).all()


# ---- 4. captured per draw
def test_three_draws_in_one_batch_each_read_their_own_slots(device, programs, live):
    s = T.tiles(3, 64, 32)
    draws = []
    for j, spec in enumerate(((None, "8x8", "5x3", "1x1"), (None, "5x3", "8x8b", None), ("12x20", None, "1x1", "8x8"))):
        tex, slots = bind(live, spec, bilinear=j == 1)
        draws.append((T.constants(s.width, s.height, slot=T.PER_PIXEL), tex, slots))
    # a set_program_texture after recording changes nothing
    pid = programs["PROBE"]
    check(device, pid, s, "PROBE", draws, "captured/three", after_recording=lambda: device.set_program_texture(pid, 2, live[("12x20", False)]))


def test_a_recorded_draw_keeps_the_filter_it_captured(device, programs):
    s = T.tiles(2, 64, 32)
    t = Texture(device, TEXTURES["8x8"])
    try:
        k = T.constants(s.width, s.height, slot=2)
        tex = (None, None, t, None)
        draws = [(k, tex, (None, None, (TEXTURES["8x8"], False), None)), (k, tex, (None, None, (TEXTURES["8x8"], True), None))]
        nearest, _ = T.twin_frame(s, "PROBE", [(k, draws[0][2])] * 2)
        # draw 0 is recorded under nearest; the filter is switched before draw 1 is recorded, and once more before the flush
        c = check(device, programs["PROBE"], s, "PROBE", draws, "captured/filter",
                  before=lambda j, w: t.SetBilinear(j == 1), after_recording=lambda: t.SetBilinear(False))
        assert (c.view(np.uint32) != nearest.view(np.uint32)).any(), "the two filters give the same frame: the test shows nothing"
    finally:
        t.Dispose()


def test_seventy_draws_alternate_two_bindings_of_slot_2(device, programs, live):
    """Past the 64-entry list of fragment representatives (batch_geometry): two identities, 35 draws each."""
    s = T.tiles(70, 160, 112)
    k = T.constants(s.width, s.height, slot=2)
    pair = [bind(live, (None, None, n, None)) for n in ("8x8", "8x8b")]
    draws = [(k, *pair[j & 1]) for j in range(70)]
    c = check(device, programs["PROBE"], s, "PROBE", draws, "captured/seventy")
    one, _ = T.twin_frame(s, "PROBE", [(k, pair[0][1])] * 70)
    assert (c.view(np.uint32) != one.view(np.uint32)).any()


# ---- 5. identity
@pytest.mark.parametrize("order", ["ab", "ba"])
def test_draws_that_differ_only_in_slot_3_do_not_share_fragment_state(device, programs, live, order):
    s = T.tiles(2, 64, 32)
    k = T.constants(s.width, s.height, slot=3)
    a, b = (bind(live, ("12x20", "5x3", "1x1", n)) for n in (("8x8", "8x8b") if order == "ab" else ("8x8b", "8x8")))
    c = check(device, programs["PROBE"], s, "PROBE", [(k, *a), (k, *b)], f"identity/slot3/{order}")
    same, _ = T.twin_frame(s, "PROBE", [(k, a[1])] * 2)
    assert (c.view(np.uint32) != same.view(np.uint32)).any()


@pytest.mark.parametrize("order", ["ab", "ba"])
def test_fragment_identity_tells_the_sign_of_a_zero_constant(device, programs, order):
    """The case test_fragment_identity_of_constants_is_bitwise leaves out: constants[0] = +0.0 against -0.0, everything else
    equal.  Each draw reads its own 1 / constants[0]."""
    blocks = []
    for v in ((0.0, -0.0) if order == "ab" else (-0.0, 0.0)):
        k = np.array([4.0, 0.5, 1.0] + [0.125 * j for j in range(61)], dtype=F32)
        k[0] = v
        blocks.append(k)
    assert blocks[0].tobytes() != blocks[1].tobytes() and (blocks[0] == blocks[1]).all()
    s = PC.tile_scene(f"ptex_identity_zero_{order}", 64, 32, [0, 0], constants=blocks)
    with np.errstate(all="ignore"):
        want, count = PC.expected_flat(s, lambda t: np.array([F32(1.0) / blocks[t.draw][0], blocks[t.draw][1], blocks[t.draw][2]], dtype=F32))
    assert (want[..., 0] == -np.inf).any() and (want[..., 0] == np.inf).any()
    c, _, st = probe_render(device, s, programs["IDENTITY"])
    assert_words(c, want, f"identity/zero_sign/{order}", exact_nan=True)
    assert st["fragments_written"] == int(count.sum()) > 0


# ---- 6. the vertex half
@pytest.mark.parametrize("bilinear", [False, True], ids=["nearest", "bilinear"])
def test_the_vertex_half_reads_the_same_slots(device, programs, live, bilinear):
    """swr_sample(env, 1, in.uv) into data4, swr_texel(env, 0, ..) into color, a size and a has_texture into tex_coord; PROBE_ALL
    returns them.  One draw of 3 vertices and one of 65, under different slot-1 textures, in one batch."""
    from vertex_probe_cases import nm_flags
    scene = T.vertex_scene()
    flags = nm_flags(*device.transform_fma())
    bound = [bind(live, ("12x20", "8x8", "5x3", None), bilinear), bind(live, ("12x20", "5x3", "8x8b", "1x1"), bilinear)]
    stages = [T.vertex_stage(d, flags, bound[j][1]) for j, d in enumerate(scene.draws)]
    used = [np.unique(d.indices) for d in scene.draws]
    tx = np.concatenate([st[1][0][u] for st, u in zip(stages, used)]); ty = np.concatenate([st[1][1][u] for st, u in zip(stages, used)])
    assert (tx.min(), tx.max(), ty.min(), ty.max()) == (-2, 13, -2, 21)          # 12 x 20: both sides of the clamp, at drawn vertices
    assert not np.array_equal(stages[0][0]["data4"][:3], stages[1][0]["data4"][:3])
    planes, count = PC.expected_planes(scene, tris=PC.probe_tris(scene, lambda j, d: stages[j][0]))
    covered = int((count > 0).sum())
    assert count.max() == 1 and covered > 0
    for g in T.VERTEX_GROUPS:
        k = PC.selector_constants(g)
        c, st = render(device, scene, programs["VERTEX"], [(k, bound[j][0]) for j in range(2)])
        assert_words(c, PC.expected_colour(scene, PC.group_names(g), planes, count), f"vertex/{bilinear}/{'+'.join(PC.group_names(g))}")
        assert st["fragments_written"] == covered


# ---- 7. render to texture through a slot
@pytest.mark.parametrize("pipelining", [1, 0], ids=["in_flight", "one_stream"])
def test_a_texture_update_between_two_draws_orders_as_recorded(device, programs, pipelining):
    """Draw A samples T in slot 2; T.UpdateFrom(the frame, which holds A by then); draw B samples T; one read-back.  A holds the old
    texels, B the new ones."""
    s = T.tiles(2, 64, 32)
    old = np.random.default_rng(77).integers(0, 256, (s.height, s.width, 4), dtype=np.uint8)
    k = T.constants(s.width, s.height, slot=2, lo=0.0, hi=1.0)          # u = (x + 0.5) / 64 + constants[2]: draw A, in tile 0, looks 32
    kb = k.copy()                                                        # texels to the right (what it writes is not what T held there),
    k[2], kb[2] = 0.5, -0.25                                             # draw B, in tile 1, 16 texels to the left: at A's tile
    one = dataclasses.replace(s, draws=s.draws[:1])
    frame_a, _ = T.twin_frame(one, "PROBE", [(k, (None, None, (old, False), None))])
    new = RT.texels(frame_a, 1, 1)
    assert (new != old).any()
    want, n = T.twin_frame(s, "PROBE", [(k, (None, None, (old, False), None)), (kb, (None, None, (new, False), None))])
    stale, _ = T.twin_frame(s, "PROBE", [(k, (None, None, (old, False), None)), (kb, (None, None, (old, False), None))])
    assert (want.view(np.uint32) != stale.view(np.uint32)).any()
    before = device.pipelining()
    t = Texture(device, old)
    try:
        device.set_pipelining(pipelining)
        tex = (None, None, t, None)
        c, st = render(device, s, programs["PROBE"], [(k, tex), (kb, tex)], before=lambda j, w: t.UpdateFrom(w) if j == 1 else None)
        assert_words(c, want, f"rtt/{pipelining}")
        assert st["fragments_written"] == n > 0
        assert np.array_equal(t.Read(), new)
    finally:
        device.set_pipelining(before)
        t.Dispose()


# ---- 8. lifetimes and errors
def test_bad_ids_and_slots_are_refused_and_leave_the_bindings(device, programs, live):
    pid = programs["PROBE"]
    s = T.tiles(1, 64, 32)
    tex, slots = bind(live, (None, "8x8", "5x3", "1x1"))
    other = live[("12x20", False)]

    def refused():
        for bad_pid, slot in ((pid, 0), (pid, 4), (pid, -1), (pid + 100000, 1), (int(N.SWR_PROG_USER_BASE) - 1, 1), (2, 1)):
            with pytest.raises(N.SwrError) as e:
                device.set_program_texture(bad_pid, slot, other)
            assert e.value.code == N.SWR_ERR_INVALID_ARG, (bad_pid, slot)
    k = T.constants(s.width, s.height, slot=T.PER_PIXEL)
    # the refused calls come after the three good ones of `render` and before the draw is recorded
    w = MainWindow(device, s.width, s.height)
    Rasterizer.NearClip, Rasterizer.FarClip = s.near_clip, s.far_clip
    w.ClearDepthBuffer(); w.ClearColorBuffer(s.clear_color)
    device.reset_stats()
    device.set_program_constants(pid, k)
    for slot in (1, 2, 3):
        device.set_program_texture(pid, slot, tex[slot])
    refused()
    d = s.draws[0]
    prog = ShaderProgram(pid, d.uniforms, None)
    Rasterizer.RenderMesh(w, d.vertices, d.indices, d.model, d.view, d.projection, prog.VertexShader, prog.FragmentShader, d.cull, d.depth_test, d.blend)
    c, _ = w._read(True, False)
    want, n = T.twin_frame(s, "PROBE", [(k, slots)])
    assert_words(c, want, "errors/bindings stay")
    assert device.stats()["fragments_written"] == n > 0


def test_destroying_a_bound_texture_unbinds_it(device, programs, live):
    pid = programs["PROBE"]
    s = T.tiles(2, 64, 32)
    t = Texture(device, TEXTURES["8x8"])
    k = T.constants(s.width, s.height, slot=2)
    with_t = (None, None, (TEXTURES["8x8"], False), None)
    c = check(device, pid, s, "PROBE", [(k, (None, None, t, None), with_t)] * 2, "destroy/before")
    device.set_program_texture(pid, 2, t)
    t.Dispose()                                     # clears slot 2 of every live program
    # draws recorded now, without another set_program_texture, read ones there
    w = MainWindow(device, s.width, s.height)
    w.ClearDepthBuffer(); w.ClearColorBuffer(s.clear_color)
    device.reset_stats()
    device.set_program_constants(pid, k)
    for d in s.draws:
        prog = ShaderProgram(pid, d.uniforms, None)
        Rasterizer.RenderMesh(w, d.vertices, d.indices, d.model, d.view, d.projection, prog.VertexShader, prog.FragmentShader, d.cull, d.depth_test, d.blend)
    after, _ = w._read(True, False)
    want, n = T.twin_frame(s, "PROBE", [(k, T.NO_SLOTS)] * 2)
    assert_words(after, want, "destroy/after")
    assert device.stats()["fragments_written"] == n > 0
    assert (after.view(np.uint32) != c.view(np.uint32)).any()


def test_a_destroyed_program_still_renders_its_recorded_draws(device, live):
    pid = device.compile_program(T.PROBE)
    s = T.tiles(2, 64, 32)
    tex, slots = bind(live, ("12x20", "8x8", None, "5x3"))
    k = T.constants(s.width, s.height, slot=T.PER_PIXEL)
    check(device, pid, s, "PROBE", [(k, tex, slots)] * 2, "destroy/program", after_recording=lambda: device.destroy_program(pid))
    with pytest.raises(N.SwrError):
        device.set_program_texture(pid, 1, None)


# ---- 9. nothing else moved
def test_a_program_without_slot_helpers_does_not_see_the_slots(device, programs, live):
    s = PC.wide()
    for bilinear in (False, True):
        tex0, slots0 = bind(live, ("12x20", None, None, None), bilinear)
        tex1, slots1 = bind(live, ("12x20", "8x8", "5x3", "1x1"), bilinear)
        for group in (0, 1):
            k = T.constants(s.width, s.height, group=group)
            a = check(device, programs["PLAIN"], s, "PLAIN", [(k, tex0, slots0)], f"plain/{bilinear}/{group}/unbound")
            b = check(device, programs["PLAIN"], s, "PLAIN", [(k, tex1, slots1)], f"plain/{bilinear}/{group}/bound")
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_python_custom_program_sets_its_textures_before_every_draw(device, live):
    """Shaders.Custom(..., textures=...): the slots are set beside the constants before every draw, so a change of the field between
    two draws of one batch reaches the second draw alone."""
    from softwarerenderer_amd.rasterizer import Shaders
    s = T.tiles(2, 64, 32)
    k = T.constants(s.width, s.height, slot=1)
    binds = [bind(live, (None, n, None, None)) for n in ("8x8", "5x3")]
    w = MainWindow(device, s.width, s.height)
    Rasterizer.NearClip, Rasterizer.FarClip = s.near_clip, s.far_clip
    w.ClearDepthBuffer(); w.ClearColorBuffer(s.clear_color)
    device.reset_stats()
    p = Shaders.Custom(T.PROBE, uniforms=s.draws[0].uniforms, constants=k)
    for d, b in zip(s.draws, binds):
        p.textures = b[0][1:]
        Rasterizer.RenderMesh(w, d.vertices, d.indices, d.model, d.view, d.projection, p.VertexShader, p.FragmentShader, d.cull, d.depth_test, d.blend)
    c, _ = w._read(True, False)
    want, n = T.twin_frame(s, "PROBE", [(k, b[1]) for b in binds])
    assert_words(c, want, "python mirror")
    assert device.stats()["fragments_written"] == n > 0
    for dev_, pid in p._ids.values():
        dev_.destroy_program(pid)
