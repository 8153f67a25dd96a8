"""Probes of the user vertex contract, field by field (test helper; not part of the package).

A run-time compiled vertex program (swr_vertex, csrc/swr_program.hip.h) runs in k_vertex_user (csrc/swr_geometry.hip.h), which packs
its twenty output scalars into four VOut rows and the Normal side array -- tex_coord beside world_normal.xy, world_normal.z beside
data4.xyz, normal beside data4.w -- and hands them to the program's own k_setup (the clipper lerps normal and data4.w apart from the
rest) and to shade_user, which unpacks them again.  A VERTEX PROBE is a vertex text plus its numpy float32 restatement, both
generated from one table so that the two cannot drift apart (the discipline of TABLE in program_probe_cases.py).  What it writes is
read back, word for word, by the fragment probes of program_probe_cases.py, unchanged (PROBE_ALL / NARROW), against
fs_in_reference fed with the restatement's per-vertex outputs (probe_tris(scene, vertex_stage=...)).

  ROUTE    the clip position of Renderer.VertexShader; each of the sixteen other output scalars = one input scalar times a power of
           two plus a constant of its own: every output differs from every other at every vertex, every input scalar is used.
           (The product with a power of two is exact, so `a * f + c` has the same bits whether or not the compiler fuses it.  The
           constants are there because `clipped` places its vertices at the unit vectors: products alone would give 0 in several
           outputs at once.)
  ENV_ALL  clip = (in.position.xyz, 1): the matrices are free and carry probe values.  `switch ((int)env.constants[62])` picks
           which thirteen scalars of ENV_TABLE leave in color, tex_coord, normal and data4 (world_normal is renormalised by the
           raster stage and carries nothing); an unknown selector leaves the outputs zero.  env_narrow(k) is case k alone: nothing
           else of the env is read.
  ZEROS    writes clip_position only.
  HELPERS  swr_normalize, swr_transform_normal and swr_transform of the vertex's own inputs, at a zero normal (0 / 0 = NaN), one
           of magnitude 2^70 (|n|^2 = Inf, n / Inf = 0), a denormal one (|n|^2 = 0, n / 0 = Inf or NaN), one whose |n|^2 is a
           denormal, and ordinary ones.
  MANY     two scalars each of the draw's constants, model matrix and uniform block (scene `many_draws`).

Scenes: `cells` and `clipped` of program_probe_cases.py, each vertex under an alpha of its own, for ROUTE and ZEROS; `slabs` (one draw per vertex count around the 64-vertex
LDS slab and the 128-vertex block of k_vertex / k_vertex_user), `env_scene`, `helpers_scene` and `many_draws` (70 draws, one more
than the list of fragment identities holds, one of them a repeat of the 65th's identity)."""
from __future__ import annotations

import copy
import dataclasses
import functools

import numpy as np

import geometry_edge_scenes as G
import program_probe_cases as PC
import shade_edge_scenes as S
from edge_scenes import F32, TILE, clip_pos
from softwarerenderer_amd import _native as N
from softwarerenderer_amd import hostmath as hm
from softwarerenderer_amd import scenes
from softwarerenderer_amd.rasterizer import Program

NM_TRANSFORM_FMA, NM_TRANSFORM_NORMAL_FMA = 1, 2          # SWR_NM_* (csrc/swr_device.h): swr_vs_env::nm_flags


def nm_flags(transform_fused, transform_normal_fused):
    return (NM_TRANSFORM_FMA if transform_fused else 0) | (NM_TRANSFORM_NORMAL_FMA if transform_normal_fused else 0)


# ============================================================================ the restated helpers
def _madd(a, b, c, fused):
    return G.fma32(a, b, c) if fused else F32(F32(a * b) + c)


def transform4(v, m, fused):
    """swr::vec4_transform: Vector4.Transform(v, M), ((x row1 + y row2) + z row3) + w row4, each madd fused or not."""
    m = np.asarray(m, dtype=F32).reshape(4, 4)
    out = np.empty(4, dtype=F32)
    with np.errstate(all="ignore"):
        for j in range(4):
            r = F32(m[0, j] * v[0])
            for i in (1, 2, 3):
                r = _madd(m[i, j], v[i], r, fused)
            out[j] = r
    return out


def transform_normal3(n, m, fused):
    """swr::vec3_transform_normal: Vector3.TransformNormal(n, M)."""
    m = np.asarray(m, dtype=F32).reshape(4, 4)
    out = np.empty(3, dtype=F32)
    with np.errstate(all="ignore"):
        for j in range(3):
            r = F32(m[0, j] * n[0])
            for i in (1, 2):
                r = _madd(m[i, j], n[i], r, fused)
            out[j] = r
    return out


def dot3(a, b):
    """swr::dot3 of the product build (SWR_DOT_PAIRWISE = 0): (ax bx + ay by) + az bz."""
    with np.errstate(all="ignore"):
        return F32(F32(F32(a[0] * b[0]) + F32(a[1] * b[1])) + F32(a[2] * b[2]))


def normalize3(v):
    """swr_normalize: v / v.Length(), Length = sqrt(dot3(v, v)): no guard (NaN at zero, 0 where |v|^2 overflows)."""
    v = np.asarray(v, dtype=F32)
    with np.errstate(all="ignore"):
        return (v / np.sqrt(dot3(v, v))).astype(F32)


def _pos1(V, i):
    return np.array([*V["position"][i], 1.0], dtype=F32)


def renderer_clip(d, i, flags):
    ft = bool(flags & NM_TRANSFORM_FMA)
    return transform4(transform4(transform4(_pos1(d.vertices, i), d.model, ft), d.view, ft), d.projection, ft)


def _empty(n):
    return {"clip": np.zeros((n, 4), F32), "color": np.zeros((n, 4), F32), "uv": np.zeros((n, 2), F32),
            "normal": np.zeros((n, 3), F32), "wn": np.zeros((n, 3), F32), "data4": np.zeros((n, 4), F32)}


def renderer_stage(d, flags=0):
    """RENDERER_VS (tests/vertex_program_texts.py) = Renderer.VertexShader, per vertex, under the draw's nm_flags."""
    V, n = d.vertices, d.vertices.shape[0]
    o = _empty(n)
    for i in range(n):
        o["clip"][i] = renderer_clip(d, i, flags)
        o["wn"][i] = normalize3(transform_normal3(V["normal"][i].astype(F32), d.model, bool(flags & NM_TRANSFORM_NORMAL_FMA)))
    o["color"], o["uv"], o["normal"] = V["color"].astype(F32), V["uv"].astype(F32), V["normal"].astype(F32)
    return o


# ============================================================================ texts
VS_HEAD = "__device__ void swr_vertex(const swr_vs_in& in, const swr_vs_env& env, swr_vs_out& out) {\n"
CLIP_RENDERER = ("    const float4 world = swr_transform(make_float4(in.position.x, in.position.y, in.position.z, 1.0f), env.model, env);\n"
                 "    const float4 viewp = swr_transform(world, env.view, env);\n"
                 "    out.clip_position = swr_transform(viewp, env.projection, env);\n")
CLIP_POSITION = "    out.clip_position = make_float4(in.position.x, in.position.y, in.position.z, 1.0f);\n"

# the twelve scalars of swr_vs_in: name -> (member of VERTEX_DTYPE, component)
VS_IN = {f"{m}.{c}": (m, i) for m, comps in (("position", "xyz"), ("uv", "xy"), ("normal", "xyz"), ("color", "xyzw"))
         for i, c in enumerate(comps)}
assert len(VS_IN) == 12
# the sixteen scalars of swr_vs_out beside clip_position: name -> (member of the stage's dict, component)
VS_OUT = {f"{m}.{c}": (k, i) for m, k, comps in (("color", "color", "xyzw"), ("tex_coord", "uv", "xy"), ("normal", "normal", "xyz"),
                                                   ("world_normal", "wn", "xyz"), ("data4", "data4", "xyzw"))
          for i, c in enumerate(comps)}
assert len(VS_OUT) == 16


def _c(v):
    return f"{float(F32(v))!r}f"


# ---- ROUTE: (output scalar, input scalar, power-of-two factor, constant)
ROUTE_TABLE = (
    ("color.x", "position.y", 0.5, 3.1), ("color.y", "uv.x", 2.0, -1.3), ("color.z", "normal.z", 0.25, 5.7),
    ("color.w", "color.y", 4.0, -2.9), ("tex_coord.x", "color.w", 0.5, 7.3), ("tex_coord.y", "position.x", 2.0, -30.1),
    ("normal.x", "uv.y", 4.0, 9.9), ("normal.y", "color.x", 0.125, -4.7), ("normal.z", "normal.x", 2.0, 11.3),
    ("world_normal.x", "color.z", 0.5, -5.9), ("world_normal.y", "position.z", 0.25, 43.7), ("world_normal.z", "normal.y", 4.0, -16.3),
    ("data4.x", "uv.x", 0.5, 15.1), ("data4.y", "color.y", 0.25, -7.7), ("data4.z", "position.y", 2.0, 77.3),
    ("data4.w", "color.w", 8.0, -8.9),
)
ROUTE = VS_HEAD + CLIP_RENDERER + "".join(f"    out.{o} = in.{i} * {_c(f)} + {_c(c)};\n" for o, i, f, c in ROUTE_TABLE) + "}\n"


def route_stage(d, flags=0, table=ROUTE_TABLE):
    V, n = d.vertices, d.vertices.shape[0]
    o = _empty(n)
    for i in range(n):
        o["clip"][i] = renderer_clip(d, i, flags)
    with np.errstate(all="ignore"):
        for out, inp, f, c in table:
            (k, j), (m, a) = VS_OUT[out], VS_IN[inp]
            o[k][:, j] = (V[m][:, a].astype(F32) * F32(f)).astype(F32) + F32(c)
    return o


# ---- ENV_ALL: every scalar a vertex program can read of its env
def _uniform_paths():
    out = []
    for name, ctype in N.Uniforms._fields_:
        if name.startswith("_pad"):
            continue
        if name == "lights":
            for l in range(4):
                for lname, lt in N.PointLight._fields_:
                    n = getattr(lt, "_length_", 0)
                    out += [(f"lights[{l}].{lname}" + (f"[{i}]" if n else ""), ("lights", l, lname, i if n else None)) for i in range(max(n, 1))]
        else:
            n = getattr(ctype, "_length_", 0)
            out += [(name + (f"[{i}]" if n else ""), (name, None, None, i if n else None)) for i in range(max(n, 1))]
    return out


UNIFORM_PATHS = _uniform_paths()
assert len(UNIFORM_PATHS) == 3 + 4 + 4 + 2 + 1 + 3 + 4 * 8 == 49          # the named scalars of swr_uniforms (include/swr.h), no pads


def uniform_value(u, path):
    name, l, lname, i = path
    v = getattr(u, name)
    if l is not None:
        v = getattr(v[l], lname)
    return F32(v[i] if i is not None else v)


def set_uniform(u, path, value):
    name, l, lname, i = path
    if l is None:
        if i is None:
            setattr(u, name, float(value))
        else:
            getattr(u, name)[i] = float(value)
    elif i is None:
        setattr(getattr(u, name)[l], lname, float(value))
    else:
        getattr(getattr(u, name)[l], lname)[i] = float(value)


def _env_table():
    """(name, C++ expression, getter(draw, flags))"""
    t = []
    for m in ("model", "view", "projection"):
        t += [(f"{m}[{i}]", f"env.{m}[{i}]", lambda d, fl, m=m, i=i: F32(np.asarray(getattr(d, m), dtype=F32).reshape(-1)[i])) for i in range(16)]
    t += [(f"uniforms.{n}", f"env.uniforms.{n}", lambda d, fl, p=p: uniform_value(d.uniforms, p)) for n, p in UNIFORM_PATHS]
    t += [(f"constants[{i}]", f"env.constants[{i}]", lambda d, fl, i=i: F32(d.constants[i])) for i in range(64)]
    t += [("nm_flags", "(float)env.nm_flags", lambda d, fl: F32(fl))]
    return t


ENV_TABLE = _env_table()
assert len(ENV_TABLE) == 48 + 49 + 64 + 1 == 162 and len({n for n, _, _ in ENV_TABLE}) == 162
ENV_INDEX = {n: i for i, (n, _, _) in enumerate(ENV_TABLE)}
ENV_SLOTS = ("color.x", "color.y", "color.z", "color.w", "tex_coord.x", "tex_coord.y", "normal.x", "normal.y", "normal.z",
             "data4.x", "data4.y", "data4.z", "data4.w")
ENV_SELECTOR = 62                     # ENV_ALL reads its selector from env.constants[62] (PROBE_ALL reads its own from [63])
N_ENV_SELECTORS = -(-len(ENV_TABLE) // len(ENV_SLOTS))
assert N_ENV_SELECTORS == 13
# the fragment groups (program_probe_cases.GROUPS) that between them hold every slot
ENV_FRAGMENT_GROUPS = [g for g in PC.FS_IN_GROUPS if set(PC.group_names(g)) & set(ENV_SLOTS)]


def env_entries(k):
    """[(slot, index into ENV_TABLE)] of selector k."""
    return [(s, 13 * k + i) for i, s in enumerate(ENV_SLOTS) if 13 * k + i < len(ENV_TABLE)]


def _env_case(k):
    return "".join(f" out.{s} = {ENV_TABLE[e][1]};" for s, e in env_entries(k))


ENV_ALL = (VS_HEAD + CLIP_POSITION + f"    switch ((int)env.constants[{ENV_SELECTOR}]) {{\n" +
           "".join(f"    case {k}:{_env_case(k)} break;\n" for k in range(N_ENV_SELECTORS)) + "    }\n}\n")


def env_narrow(k):
    return VS_HEAD + CLIP_POSITION + "   " + _env_case(k) + "\n}\n"


def _block(prefix):
    """The selector whose thirteen scalars all belong to one block of the table."""
    return next(k for k in range(N_ENV_SELECTORS) if all(ENV_TABLE[e][0].startswith(prefix) for _, e in env_entries(k)) and len(env_entries(k)) == 13)


ENV_NARROW_SELECTORS = {"model": _block("model["), "uniforms": _block("uniforms."), "constants": _block("constants[")}


def position_clip(d):
    V = d.vertices
    return np.concatenate([V["position"].astype(F32), np.ones((V.shape[0], 1), F32)], axis=1)


def slots_stage(d, flags, entries):
    """clip = (position, 1); the slots of `entries` = [(output scalar, ENV_TABLE index)] carry that env scalar at every vertex."""
    o = _empty(d.vertices.shape[0])
    o["clip"] = position_clip(d)
    for s, e in entries:
        k, j = VS_OUT[s]
        o[k][:, j] = ENV_TABLE[e][2](d, flags)
    return o


def env_stage(d, flags=0):
    """ENV_ALL under the draw's own selector (an unknown one leaves the outputs zero)."""
    k = int(d.constants[ENV_SELECTOR])
    return slots_stage(d, flags, env_entries(k) if 0 <= k < N_ENV_SELECTORS else [])


# ---- ZEROS
ZEROS = VS_HEAD + CLIP_RENDERER + "}\n"


def zeros_stage(d, flags=0):
    o = _empty(d.vertices.shape[0])
    for i in range(d.vertices.shape[0]):
        o["clip"][i] = renderer_clip(d, i, flags)
    return o


# ---- HELPERS
HELPERS = (VS_HEAD + CLIP_POSITION +
           "    const float3 tn = swr_transform_normal(in.normal, env.model, env);\n"
           "    const float3 u = swr_normalize(in.normal);\n"
           "    const float3 un = swr_normalize(tn);\n"
           "    out.color = swr_transform(make_float4(in.position.x, in.position.y, in.position.z, 1.0f), env.view, env);\n"
           "    out.data4 = make_float4(u.x, u.y, u.z, un.z);\n"
           "    out.normal = tn;\n"
           "    out.tex_coord = make_float2(un.x, un.y);\n}\n")


def helpers_stage(d, flags=0):
    V, n = d.vertices, d.vertices.shape[0]
    o = _empty(n)
    o["clip"] = position_clip(d)
    for i in range(n):
        nrm = V["normal"][i].astype(F32)
        tn = transform_normal3(nrm, d.model, bool(flags & NM_TRANSFORM_NORMAL_FMA))
        u, un = normalize3(nrm), normalize3(tn)
        o["color"][i] = transform4(_pos1(V, i), d.view, bool(flags & NM_TRANSFORM_FMA))
        o["data4"][i] = (u[0], u[1], u[2], un[2])
        o["normal"][i] = tn
        o["uv"][i] = un[:2]
    return o


# ---- MANY: two scalars each of the constants, the model matrix and the uniform block, in two fragment groups (color.x stays 0:
# CONSTANTS3 reads its group number there)
MANY_TABLE = (("color.z", "constants[0]"), ("color.w", "model[13]"), ("tex_coord.x", "uniforms.fog_end"),
              ("data4.x", "constants[61]"), ("data4.y", "model[0]"), ("data4.z", "uniforms.lights[2].range"))
MANY = VS_HEAD + CLIP_POSITION + "".join(f"    out.{s} = {ENV_TABLE[ENV_INDEX[n]][1]};\n" for s, n in MANY_TABLE) + "}\n"
MANY_FRAGMENT_GROUPS = [g for g in PC.FS_IN_GROUPS if set(PC.group_names(g)) & {s for s, _ in MANY_TABLE}]


def many_stage(d, flags=0):
    return slots_stage(d, flags, [(s, ENV_INDEX[n]) for s, n in MANY_TABLE])


VERTEX_TEXTS = {"route": ROUTE, "env_all": ENV_ALL, "zeros": ZEROS, "helpers": HELPERS, "many": MANY,
                **{f"env_narrow_{b}": env_narrow(k) for b, k in ENV_NARROW_SELECTORS.items()}}
STAGES = {"route": route_stage, "env_all": env_stage, "zeros": zeros_stage, "helpers": helpers_stage, "many": many_stage,
          "renderer": renderer_stage, **{f"env_narrow_{b}": env_stage for b in ENV_NARROW_SELECTORS}}


def stage_of(name, flags=0):
    """The vertex_stage callable probe_tris takes."""
    return lambda j, d: STAGES[name](d, flags)


def expected(scene, name, flags=0, fused=False, mutant=None):
    """(planes, count) of `scene` under vertex probe `name`."""
    return PC.expected_planes(scene, mutant, tris=PC.probe_tris(scene, stage_of(name, flags), fused))


# ============================================================================ scenes
def _with_alphas(scene, seed):
    """A copy of `scene` whose vertices each have an alpha of their own (the scenes of program_probe_cases.py give every vertex
    0.7: an output fed by in.color.w would be the same at the three vertices of a triangle, and a clipper that copied it instead
    of lerping it could not be told from one that lerps)."""
    rng = np.random.default_rng(seed)
    draws = []
    for d in scene.draws:
        d = copy.copy(d)
        d.vertices = d.vertices.copy()
        d.vertices["color"][:, 3] = rng.uniform(0.3, 1.0, d.vertices.shape[0]).astype(F32)
        draws.append(d)
    return dataclasses.replace(scene, name=scene.name + "_alphas", draws=draws)


@functools.lru_cache(maxsize=None)
def cells():
    return _with_alphas(PC.cells(), 800)


@functools.lru_cache(maxsize=None)
def clipped():
    return _with_alphas(PC.clipped(), 801)


def outputs_differ_across_each_triangle(scene, stage="route", flags=0, but=()):
    """No one of the sixteen output scalars is the same at all three vertices of a triangle (triangle numbers in `but` apart): of
    any two edges the clipper cuts, one then has ends that differ, and a copy in the place of the lerp shows.  (Three different
    values cannot be had everywhere: `clipped` places its vertices at the unit vectors.)"""
    for j, d in enumerate(scene.draws):
        o = STAGES[stage](d, flags)
        for i, vid in enumerate(d.indices.reshape(-1, 3)):
            if i in but:
                continue
            for k, c in VS_OUT.values():
                v = o[k][[int(x) for x in vid], c]
                if len(set(v.view(np.uint32).tolist())) < 2 and not np.isnan(v).any():
                    return False
    return True


SLAB_COUNTS = (3, 63, 64, 65, 127, 128, 129, 193)
# per vertex count, disjoint index triples: from vertex 0, to vertex N - 1, and across every multiple b of 64 below N in one of the
# two phases (b - 2, b - 1, b) and (b - 1, b, b + 1); between them the draws hold both phases of 64 and of 128 (192 + 1 = N is no
# vertex of the largest draw: only the first phase exists there)
SLAB_TRIPLES = {
    3: [(0, 1, 2)],
    63: [(0, 1, 2), (60, 61, 62)],
    64: [(0, 1, 2), (61, 62, 63)],
    65: [(0, 1, 2), (62, 63, 64)],
    127: [(0, 1, 2), (63, 64, 65), (124, 125, 126)],
    128: [(0, 1, 2), (62, 63, 64), (125, 126, 127)],
    129: [(0, 1, 2), (63, 64, 65), (126, 127, 128)],
    193: [(0, 1, 2), (63, 64, 65), (127, 128, 129), (190, 191, 192)],
}
SLAB_W, SLAB_H = 128, 64


@functools.lru_cache(maxsize=None)
def slabs(seed=0):
    """One batch, one draw per vertex count of SLAB_COUNTS, in that order (vert_base = 0, 3, 66, 130, 195, 322, 450, 579: none but
    the first a multiple of 64).  Every vertex, indexed or not, has random attributes of its own; the indexed ones form skewed
    one-tile triangles as in `cells` (clip.w a permutation of (1, 2, 4), clip.z tilted), one per tile of a 128 x 64 frame."""
    rng = np.random.default_rng(500 + seed)
    nx = SLAB_W // TILE
    draws, cell = [], 0
    for n in SLAB_COUNTS:
        w = rng.choice([1.0, 2.0, 4.0], n)
        pos = np.stack([rng.uniform(-0.9, 0.9, n) * w, rng.uniform(-0.9, 0.9, n) * w, w], axis=1).astype(F32)
        col = rng.uniform(0.1, 1.0, (n, 4))
        uv = rng.uniform(0.05, 0.95, (n, 2))
        nrm = rng.normal(size=(n, 3)) * 0.3 + np.array([0.2, 0.3, 1.0])
        idx = []
        for tri in SLAB_TRIPLES[n]:
            q = 0.25 if (cell + cell // nx) & 1 else 0.0
            x0, y0 = TILE * (cell % nx) + 4 + q, TILE * (cell // nx) + 4 + q
            for v, (X, Y), cw in zip(tri, [(x0, y0 + 1), (x0 + 8, y0), (x0 + 2, y0 + 8)], PC.CELL_W[cell % 6]):
                px, py = clip_pos(X, Y, SLAB_W, SLAB_H)
                pos[v] = (F32(F32(px) * F32(cw)), F32(F32(py) * F32(cw)), cw)
            idx += list(tri)
            cell += 1
        I = hm.identity()
        d = scenes.Draw(scenes.make_vertices(pos, uv=uv, normal=nrm, color=col), np.array(idx, dtype=np.uint16), I, I, I,
                        program=Program.Dust2LambertFog, uniforms=scenes.default_uniforms())
        draws.append(PC._tilted(PC._probe_state(d), 2.0))
    assert cell <= nx * (SLAB_H // TILE)
    return scenes.Scene(f"vprobe_slabs_{seed}", SLAB_W, SLAB_H, draws, clear_color=PC.CLEAR, near_clip=PC.NEAR)


def with_program(scene, program):
    """A copy of `scene` whose every draw runs the built-in `program`."""
    draws = []
    for d in scene.draws:
        d = copy.copy(d)
        d.program = program
        draws.append(d)
    return dataclasses.replace(scene, draws=draws)


def _probe_values(j):
    """162 distinct probe values for draw j, in ENV_TABLE's order (quarters: exact in float32)."""
    return (np.arange(len(ENV_TABLE), dtype=F32) * F32(0.25) + F32(1000.0 * (j + 1) + 0.125)).astype(F32)


def _apply_probe_values(d, vals):
    for m in ("model", "view", "projection"):
        setattr(d, m, np.array([vals[ENV_INDEX[f"{m}[{i}]"]] for i in range(16)], dtype=F32).reshape(4, 4))
    u = N.Uniforms()
    for n, p in UNIFORM_PATHS:
        set_uniform(u, p, vals[ENV_INDEX["uniforms." + n]])
    d.uniforms = u
    d.constants = np.array([vals[ENV_INDEX[f"constants[{i}]"]] for i in range(64)], dtype=F32)
    return d


@functools.lru_cache(maxsize=None)
def env_scene():
    """Two one-triangle draws (tiles 0 and 2 of a 64 x 16 frame, on and off the lattice) whose model, view, projection, uniform
    block and constants hold 161 probe values each, every one different from every other in the scene."""
    rng = np.random.default_rng(600)
    draws = []
    for j, k in enumerate((0, 2)):
        c = S.Cells(64, 16, rng)
        c.cell(k, half=bool(j), z=float(rng.uniform(-0.5, 0.5)))
        draws.append(_apply_probe_values(PC._probe_state(c.draw(S.DUST2)), _probe_values(j)))
    return scenes.Scene("vprobe_env", 64, 16, draws, clear_color=PC.CLEAR, near_clip=PC.NEAR)


def with_selectors(scene, vertex_selector, fragment_group):
    """A copy whose draws carry the two selectors in constants[62] (None: left as it is) and constants[63]."""
    draws = []
    for d in scene.draws:
        d = copy.copy(d)
        d.constants = d.constants.copy()
        d.constants[PC.SELECTOR] = fragment_group
        if vertex_selector is not None:
            d.constants[ENV_SELECTOR] = vertex_selector
        draws.append(d)
    return dataclasses.replace(scene, draws=draws)


HELPER_NORMALS = {
    "zero": [(0.0, 0.0, 0.0)] * 3,
    "huge": [(2.0 ** 70, 0.0, 0.0), (0.0, -2.0 ** 70, 2.0 ** 70), (2.0 ** 70, 2.0 ** 70, -2.0 ** 70)],
    "denormal": [(1e-40, 0.0, 0.0), (0.0, 2e-40, -1e-40), (1e-41, 1e-40, 3e-40)],
    "ordinary": [(0.3, -0.2, 0.9), (-0.1, 0.4, 0.7), (0.5, 0.5, -0.6)],
    "denormal_length": [(1e-20, 0.0, 0.0), (0.0, 2e-20, -1e-20), (1e-21, 1e-20, 3e-20)],
    "huge_among_ordinary": [(2.0 ** 70, 1.0, 0.0), (0.3, -0.2, 0.9), (-0.1, 0.4, 0.7)],
}


@functools.lru_cache(maxsize=None)
def helpers_scene():
    """One draw of six one-tile triangles (128 x 16), the three normals of each of one kind of HELPER_NORMALS; a general model and
    view matrix (HELPERS takes the clip position from the input position as it is)."""
    rng = np.random.default_rng(700)
    c = S.Cells(128, 16, rng)
    for k, kind in enumerate(HELPER_NORMALS):
        c.cell(k, half=bool(k & 1), nrm=HELPER_NORMALS[kind], z=float(rng.uniform(-0.5, 0.5)))
    d = PC._probe_state(c.draw(S.DUST2))
    d.model = rng.uniform(-1.5, 1.5, (4, 4)).astype(F32)
    d.view = rng.uniform(-1.5, 1.5, (4, 4)).astype(F32)
    d.constants = np.zeros(64, dtype=F32)
    return scenes.Scene("vprobe_helpers", 128, 16, [d], clear_color=PC.CLEAR, near_clip=PC.NEAR)


N_MANY, MANY_REPEAT = 70, (69, 64)          # draw 69 repeats the fragment identity of draw 64, the 65th


@functools.lru_cache(maxsize=None)
def many_draws():
    """70 one-triangle draws in one batch (tile_scene), each under constants, a model matrix and a uniform block of its own: 69
    fragment identities where the list of representatives holds 64; the last draw has the constants and the uniform block of
    the 65th (the first identity the list has no room for) and a model matrix of its own."""
    blocks, us = [], []
    for i in range(N_MANY):
        j = MANY_REPEAT[1] if i == MANY_REPEAT[0] else i
        k = np.zeros(64, dtype=F32)
        k[:3] = (j + 1, j + 1.5, -(j + 1))
        k[3:] = np.arange(61) * 0.25 + 200.0 * (j + 1)
        k[PC.SELECTOR] = 0.0
        u = scenes.default_uniforms()
        u.fog_end, u.shininess, u.lights[2].range = 100.0 + j, 8.0 + 0.5 * j, 7.0 + 0.25 * j
        blocks.append(k); us.append(u)
    s = PC.tile_scene("vprobe_many", 160, 112, [0] * N_MANY, constants=blocks, uniforms=us)
    for i, d in enumerate(s.draws):
        d.model = (np.arange(16, dtype=F32) * F32(0.5) + F32(3000.0 + 10.0 * i)).astype(F32).reshape(4, 4)
    return s


def route_outputs_differ(scene, flags=0):
    """At every vertex of every draw the sixteen ROUTE outputs are pairwise different words (a NaN equals no other output)."""
    for d in scene.draws:
        o = route_stage(d, flags)
        rows = np.stack([o[k][:, j] for k, j in VS_OUT.values()], axis=1)
        for r in rows:
            vals = r[~np.isnan(r)]
            if len(set(vals.view(np.uint32).tolist())) != len(vals) or np.isnan(r).sum() > 1:
                return False
    return True
