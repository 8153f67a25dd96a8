"""User programs with texture slots (swr_program_set_texture, include/swr.h), restated in numpy float32: the
program texts handed to swr_program_create / _create_vf, their twins, and the frames they leave.  Not a test module:
tests/test_program_textures_host.py and tests/test_gpu_program_textures.py import it.

Built on program_probe_cases (scenes in which no sample is covered twice, drawn with BlendMode.None: the colour plane holds the
program's raw words), vertex_probe_cases (the restated vertex stage and its slab scene) and post_texture_cases (the samplers:
oracle_sample is the oracle's own pair, texel and size the restatement a host test holds to it).

A fragment text computes its uv from the PIXEL, `((float)env.x + 0.5f) * constants[0] + constants[2]` -- a rounded product and a
rounded sum, the operations of post_texture_cases.pixel_uv -- so that a twin needs the coverage of a scene and nothing of the
interpolator.  It returns three words and w = 1 (the raster stage writes only results with w > 0); constants[63] picks the channel
group, (x, y, z) or (w, x, y).  `slots` is a sequence of four entries, None or (texels (h, w, 4) uint8, bilinear): slot 0 the
draw's texture, slots 1 .. 3 what the draw captured when it was recorded."""
import functools

import numpy as np

import post_texture_cases as X
import program_probe_cases as PC
import vertex_probe_cases as VC

F32 = np.float32
SLOTS = 4
NO_SLOTS = (None, None, None, None)
GROUP, MODE, SLOT = 63, 62, 61            # constants[63]: channel group; PROBE: constants[62] the helper, constants[61] the slot
PER_PIXEL = 9999.0                        # PROBE: constants[61] == PER_PIXEL asks for slot (env.x + env.y) % 5
SAMPLE, TEXEL, SIZE = 0, 1, 2             # PROBE's modes

HEAD = PC.HEAD
UV = """    const float u = ((float)env.x + 0.5f) * env.constants[0] + env.constants[2];
    const float v = ((float)env.y + 0.5f) * env.constants[1] + env.constants[3];
"""
PICK = f"    return env.constants[{GROUP}] != 0.0f ? make_float4(r.w, r.x, r.y, 1.0f) : make_float4(r.x, r.y, r.z, 1.0f);\n}}\n"

# the four slots at once, weights 1/2, 1/4, 1/8, 1/16 (exact products), summed left to right
FOUR = """__device__ float mix4(float a, float b, float c, float d) { return ((a * 0.5f + b * 0.25f) + c * 0.125f) + d * 0.0625f; }
""" + HEAD + UV + """    const float2 uv = make_float2(u, v);
    const float4 a = swr_sample(env, 0, uv), b = swr_sample(env, 1, uv), c = swr_sample(env, 2, uv), d = swr_sample(env, 3, uv);
    const float4 r = make_float4(mix4(a.x, b.x, c.x, d.x), mix4(a.y, b.y, c.y, d.y), mix4(a.z, b.z, c.z, d.z), mix4(a.w, b.w, c.w, d.w));
""" + PICK

# one helper of one slot, both chosen by constants: the slot may be any int, or vary by pixel.  The texel read walks x over
# -2 .. constants[4] - 3 and y over -2 .. constants[5] - 3 (constants[4] = w + 4: from two before the texture to one past its end)
PROBE = HEAD + UV + f"""    const int slot = env.constants[{SLOT}] == {PER_PIXEL!r}f ? (env.x + env.y) % 5 : (int)env.constants[{SLOT}];
    float4 r;
    switch ((int)env.constants[{MODE}]) {{
    case {SAMPLE}: r = swr_sample(env, slot, make_float2(u, v)); break;
    case {TEXEL}: r = swr_texel(env, slot, env.x % (int)env.constants[4] - 2, env.y % (int)env.constants[5] - 2); break;
    case {SIZE}: {{
        const int2 s = swr_texture_size(env, slot);
        r = make_float4((float)s.x, (float)s.y, swr_has_texture(env, slot) ? 1.0f : 0.0f, (float)(s.x * 256 + s.y));
    }} break;
    default: return swr_discard();
    }}
""" + PICK

# no slot helper at all: the contract as it was before the slots
PLAIN = HEAD + UV + "    const float4 r = swr_sample(env, make_float2(u, v));\n" + PICK

# the porting guide's example: diffuse times lightmap
LIGHTMAP = HEAD + """    const float4 d = swr_sample(env, in.tex_coord), l = swr_sample(env, 1, in.tex_coord);
    return make_float4(in.color.x * d.x * l.x, in.color.y * d.y * l.y, in.color.z * d.z * l.z, in.color.w * d.w);
}
"""

# the vertex half: slot 1 sampled at in.uv into data4, a texel of slot 0 (the draw's texture) into color, from two before the
# texture to one past its end for uv in [0, 1) and a 12 x 20 texture; the fragment half is PROBE_ALL of program_probe_cases, which
# returns color and data4 as they arrive
VERTEX = (VC.VS_HEAD + VC.CLIP_RENDERER +
          "    out.data4 = swr_sample(env, 1, in.uv);\n"
          "    out.color = swr_texel(env, 0, (int)(in.uv.x * 16.0f) - 2, (int)(in.uv.y * 24.0f) - 2);\n"
          "    const int2 s = swr_texture_size(env, 2);\n"
          "    out.tex_coord = make_float2((float)(s.x * 256 + s.y), swr_has_texture(env, 3) ? 1.0f : 0.0f);\n}\n")
VERTEX_GROUPS = [g for g in PC.FS_IN_GROUPS if any(n.split(".")[0] in ("color", "data4", "tex_coord") for n in PC.group_names(g))]

# every helper of each half, for the compile-only tests: (vertex text or None, fragment text)
ONE_HELPER = {
    "fragment/has": (None, HEAD + "    return swr_has_texture(env, 1) ? in.color : swr_discard();\n}\n"),
    "fragment/sample": (None, HEAD + "    return swr_sample(env, 1, in.tex_coord);\n}\n"),
    "fragment/texel": (None, HEAD + "    return swr_texel(env, 2, env.x, env.y);\n}\n"),
    "fragment/size": (None, HEAD + "    const int2 s = swr_texture_size(env, 3);\n    return make_float4((float)s.x, (float)s.y, 0.0f, 1.0f);\n}\n"),
    "vertex/has": (VC.VS_HEAD + VC.CLIP_RENDERER + "    out.color.x = swr_has_texture(env, 1) ? 1.0f : 0.0f;\n}\n", PC.NARROW[1]),
    "vertex/sample": (VC.VS_HEAD + VC.CLIP_RENDERER + "    out.data4 = swr_sample(env, 1, in.uv);\n}\n", PC.NARROW[1]),
    "vertex/texel": (VC.VS_HEAD + VC.CLIP_RENDERER + "    out.color = swr_texel(env, 0, 1, 2);\n}\n", PC.NARROW[1]),
    "vertex/size": (VC.VS_HEAD + VC.CLIP_RENDERER + "    const int2 s = swr_texture_size(env, 2);\n    out.color.x = (float)(s.x + s.y);\n}\n", PC.NARROW[1]),
}

# ---- the textures ---------------------------------------------------------------------------------------------------------------
# (w, h): 12 x 20 and 8 x 8 get a block-linear copy under the filter; 5 x 3 and 1 x 1 (not multiples of 4) never do
TEXTURES = {"12x20": PC.TEX_12x20, "8x8": X.texture((8, 8)), "5x3": X.texture((5, 3)), "1x1": X.texture((1, 1)),
            "8x8b": X.texture((8, 8), seed=1)}


def slots_of(names, bilinear=False):
    """('12x20', None, '5x3', ..) -> the `slots` of a twin."""
    return tuple(None if n is None else (TEXTURES[n], bilinear) for n in names)


def constants(W, H, group=0, mode=SAMPLE, slot=0, texel_span=(16, 24), lo=-2.0, hi=3.0):
    """64 constants: the uv scale and shift that spread the pixels' centres over about [lo, hi], the texel walk's periods, the slot,
    the mode and the channel group."""
    k = X.uv_constants((W, H), lo, hi).copy()
    k[4], k[5] = texel_span
    k[SLOT], k[MODE], k[GROUP] = slot, mode, group
    return k


# ---- the twins: (constants, slots, xs, ys) -> (n, 4) float32 at the pixels (xs, ys) ------------------------------------------------
def pixel_uv(k, xs, ys):
    u = ((xs.astype(F32) + F32(0.5)) * k[0]).astype(F32) + k[2]
    v = ((ys.astype(F32) + F32(0.5)) * k[1]).astype(F32) + k[3]
    return np.stack([u.astype(F32), v.astype(F32)], axis=-1)


def pick(r, k):
    r = np.asarray(r, dtype=F32)
    return np.ascontiguousarray(r[:, [3, 0, 1]] if k[GROUP] != 0 else r[:, :3])


def four_twin(k, slots, xs, ys, order=(0, 1, 2, 3)):
    uv = pixel_uv(k, xs, ys)
    return X._mix4(*[X.sample(slots, s, uv) for s in order])


def four_all_slot0(k, slots, xs, ys):
    """WRONG TWIN: every slot reads slot 0."""
    return four_twin(k, slots, xs, ys, order=(0, 0, 0, 0))


def plain_twin(k, slots, xs, ys):
    return X.sample(slots, 0, pixel_uv(k, xs, ys))


def _one_slot(k, slots, slot, xs, ys):
    mode = int(k[MODE])
    if mode == SAMPLE:
        return X.sample(slots, slot, pixel_uv(k, xs, ys))
    if mode == TEXEL:
        return X.texel(slots, slot, xs % int(k[4]) - 2, ys % int(k[5]) - 2)
    assert mode == SIZE
    w, h = X.size(slots, slot)
    bound = 0 <= slot < SLOTS and slots[slot] is not None
    return np.broadcast_to(np.array([w, h, 1.0 if bound else 0.0, w * 256 + h], dtype=F32), (len(xs), 4)).copy()


def probe_twin(k, slots, xs, ys):
    if k[SLOT] != F32(PER_PIXEL):
        return _one_slot(k, slots, int(k[SLOT]), xs, ys)
    out = np.zeros((len(xs), 4), dtype=F32)
    for s in range(5):
        m = (xs + ys) % 5 == s
        if m.any():
            out[m] = _one_slot(k, slots, s, xs[m], ys[m])
    return out


TWINS = {"FOUR": four_twin, "PROBE": probe_twin, "PLAIN": plain_twin}
TEXTS = {"FOUR": FOUR, "PROBE": PROBE, "PLAIN": PLAIN, "IDENTITY": PC.IDENTITY_CONSTANTS, "LIGHTMAP": LIGHTMAP}


# ---- frames -----------------------------------------------------------------------------------------------------------------------
_coverage = {}


def coverage(scene):
    """(draw, count): per pixel the draw that covers it (-1: none) and how many triangles do; computed once per scene."""
    if id(scene) not in _coverage:
        draw = np.full((scene.height, scene.width), -1, dtype=np.int32)
        count = np.zeros((scene.height, scene.width), dtype=np.int32)
        for t in PC.probe_tris(scene):
            for sX, eX, sY, eY in t.rects():
                with np.errstate(all="ignore"):
                    inside = t.tri.cover((sX, eX, sY, eY))[0]
                draw[sY:eY + 1, sX:eX + 1][inside] = t.draw
                count[sY:eY + 1, sX:eX + 1] += inside
        _coverage[id(scene)] = (scene, draw, count)
    return _coverage[id(scene)][1:]


def expected_frame(scene, words_of):
    """(colour, fragments): every pixel draw j covers shows the three words words_of(j, xs, ys)[i] and w = 1, every other pixel
    the clear colour.  No sample of the scene may be covered twice."""
    draw, count = coverage(scene)
    assert count.max() == 1
    out = np.empty((scene.height, scene.width, 4), dtype=F32)
    out[...] = np.asarray(scene.clear_color, dtype=F32)
    for j in range(len(scene.draws)):
        ys, xs = np.nonzero(draw == j)
        if len(xs):
            out[ys, xs, :3] = np.asarray(words_of(j, xs, ys), dtype=F32).reshape(len(xs), 3)
            out[ys, xs, 3] = 1.0
    return out, int(count.sum())


def twin_frame(scene, name, per_draw, twin=None):
    """per_draw[j] = (constants, slots) of draw j as it was recorded."""
    fn = twin or TWINS[name]
    return expected_frame(scene, lambda j, xs, ys: pick(fn(per_draw[j][0], per_draw[j][1], xs, ys), per_draw[j][0]))


@functools.lru_cache(maxsize=None)
def tiles(n, W, H):
    """n one-triangle draws in one batch, draw i in tile i of a W x H frame (program_probe_cases.tile_scene)."""
    return PC.tile_scene(f"ptex_tiles_{n}", W, H, [0] * n)


# ---- the vertex half --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vertex_scene():
    """Two draws of vertex_probe_cases.slabs in one batch: the one of 3 vertices and the one of 65 (one past the 64-vertex slab),
    every vertex under a uv of its own; those of the nine drawn vertices are VERTEX_UVS, which send VERTEX's texel read to both sides
    of the clamp of a 12 x 20 texture in x and in y."""
    import copy
    import dataclasses
    s = VC.slabs()
    draws, n = [], 0
    for d in s.draws:
        if d.vertices.shape[0] not in (3, 65):
            continue
        d = copy.copy(d)
        d.vertices = d.vertices.copy()
        for v in np.unique(d.indices):
            d.vertices["uv"][v] = VERTEX_UVS[n]
            n += 1
        draws.append(d)
    assert [d.vertices.shape[0] for d in draws] == [3, 65] and n == len(VERTEX_UVS)
    return dataclasses.replace(s, name="ptex_vertex", draws=draws)


VERTEX_UVS = [(0.01, 0.01), (0.99, 0.99), (0.5, 0.3), (0.07, 0.95), (0.93, 0.05), (0.3, 0.6), (0.6, 0.9), (0.2, 0.2), (0.8, 0.45)]


def vertex_stage(d, flags, slots):
    """VERTEX restated per vertex: the outputs probe_tris(scene, vertex_stage=...) takes."""
    V, n = d.vertices, d.vertices.shape[0]
    o = VC._empty(n)
    for i in range(n):
        o["clip"][i] = VC.renderer_clip(d, i, flags)
    uv = V["uv"].astype(F32)
    o["data4"] = X.sample(slots, 1, uv)
    tx = np.trunc((uv[:, 0] * F32(16.0)).astype(F32)).astype(np.int64) - 2
    ty = np.trunc((uv[:, 1] * F32(24.0)).astype(F32)).astype(np.int64) - 2
    o["color"] = X.texel(slots, 0, tx, ty)
    w, h = X.size(slots, 2)
    o["uv"][:, 0] = w * 256 + h
    o["uv"][:, 1] = 1.0 if slots[3] is not None else 0.0
    return o, (tx, ty)
