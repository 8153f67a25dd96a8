"""Cases and the reference restatement for the GPU ray queries (test helper; not part of the package).

csrc/swr_raycast.hip.h answers Physics.Raycast (Physics.cs:19-179) for every (ray, mesh) pair: k_ray_cast, one lane per triangle and a
64-bit atomicMin per hit on the key (distance bits with +-0 mapped to 0) << 32 | triangle; k_ray_finish, which recomputes the winner and
-- for swr_raycast_nearest -- folds a ray's targets in order.  `raycast` below restates the reference in numpy float32, vectorised over
the triangles, in its serial schedule: the nearest hit under float `<` among distances below float.MaxValue, the lowest triangle index
on ties.  It is the reference of every GPU test:

  * world vertices and normals come from the ORACLE library, vertex by vertex (oswr_nm_transform4, oswr_nm_dot3), so they follow the
    oracle build (Lerp / dot order) and its run-time Transform flag;
  * dot3 is restated in its three summation orders for the vectorised part (tests/test_raycast_host.py holds it to oswr_nm_dot3);
  * cross3 is restated in both forms; the fused form needs a float32 fma, which numpy does not have: fma32 computes the exact float64
    product, adds with the rounding error recovered (TwoSum), rounds to odd and then to float32 -- one rounding, as the hardware fma
    (held to exact rational arithmetic in the host test).

`rule` and `u_sense` make the three host mutants of the restatement (test_raycast_host.py::test_host_mutants_turn_named_cases_red);
the `mut` tuple names the further ones of MUTANTS (tests/test_raycast_edges_host.py); with mut=() the arithmetic is untouched.

The case lists: HOST_CASES (KAT, face masks, inclusive edges, degenerate rays, +-0 on the plane), count_case (T triangles, the only hit
in the last / first), tie cases (coplanar twins, +0.0 / -0.0 twins), shape_case (rays x targets with models of their own and one zero
normal matrix), nearest cases, dust2_case (42 rays shaped like CharacterController.MoveWithSlide's against the 11 meshes of
tests/golden/models/dust2)."""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools
import os

import numpy as np

from softwarerenderer_amd import hostmath as hm
from softwarerenderer_amd.rasterizer import RAY_HIT_DTYPE, VERTEX_DTYPE

F32 = np.float32
FLT_MAX = np.finfo(F32).max
EPS = F32(1e-8)                                # Physics.cs:147
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOT_ORDER = {"": 0, "fma": 0, "dotpw": 2, "fma_dotpw": 2, "dpps": 1, "fma_dpps": 1}      # oracle variant -> SWR_DOT_PAIRWISE
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 513)
CROSS_FUSED = 0x100


# ============================================================================ float32 helpers
def dot3v(a, b, order):
    """Vector3.Dot over the last axis in the three summation orders of SWR_DOT_PAIRWISE (0 sequential, 1 dpps, 2 shuffle-adds)."""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    with np.errstate(all="ignore"):
        x, y, z = a[..., 0] * b[..., 0], a[..., 1] * b[..., 1], a[..., 2] * b[..., 2]
        if order == 0:
            return (x + y) + z
        if order == 1:
            return (x + y) + (z + F32(0.0))
        return (x + z) + (y + F32(0.0))


def fma32(a, b, c):
    """float32 fma(a, b, c), one rounding: exact product in float64, TwoSum, round to odd, round to float32."""
    a, b, c = (np.asarray(t, dtype=F32).astype(np.float64) for t in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b                                  # 24 x 24 bits: exact
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)            # s + err == p + c exactly
        odd = (np.ascontiguousarray(s).view(np.int64) & 1) != 0
        toward = np.where(err > 0, np.nextafter(s, np.inf), np.where(err < 0, np.nextafter(s, -np.inf), s))
        s = np.where((err != 0) & ~odd, toward, s)
        return s.astype(F32)


def cross3v(a, b, fused):
    """Vector3.Cross: x = a.y*b.z - a.z*b.y etc.; fused = fma(-a.z, b.y, round(a.y*b.z))."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=F32), np.asarray(b, dtype=F32))
    out = np.empty(a.shape, dtype=F32)
    with np.errstate(all="ignore"):
        for k in range(3):
            i, j = (k + 1) % 3, (k + 2) % 3
            p = a[..., i] * b[..., j]
            out[..., k] = fma32(-a[..., j], b[..., i], p) if fused else p - a[..., j] * b[..., i]
    return out


def normalize3v(v, order):
    """Vector3.Normalize = v / v.Length()."""
    v = np.asarray(v, dtype=F32)
    with np.errstate(all="ignore"):
        return v / np.sqrt(dot3v(v, v, order))[..., None]


# ============================================================================ the oracle's transforms
def _oracle_fns(lib):
    fp = C.POINTER(C.c_float)
    lib.oswr_nm_transform4.restype = None; lib.oswr_nm_transform4.argtypes = [fp, fp, fp]
    lib.oswr_nm_dot3.restype = C.c_float; lib.oswr_nm_dot3.argtypes = [fp, fp]
    return lib.oswr_nm_transform4, lib.oswr_nm_dot3


def oracle_dot3(lib, a, b) -> np.float32:
    _, dot = _oracle_fns(lib)
    fa, fb = (C.c_float * 3)(*[float(x) for x in a]), (C.c_float * 3)(*[float(x) for x in b])
    return F32(dot(fa, fb))


def world_arrays(lib, vertices, model, normal_matrix):
    """Physics.cs:43-49 through the oracle library, under its CURRENT Transform flag: (world positions, world normals), (n, 3) each."""
    tr, dot = _oracle_fns(lib)
    v = np.ascontiguousarray(vertices)
    m = (C.c_float * 16)(*np.asarray(model, dtype=F32).reshape(-1).tolist())
    nm = (C.c_float * 16)(*np.asarray(normal_matrix, dtype=F32).reshape(-1).tolist())
    P, N = np.empty((v.shape[0], 3), dtype=F32), np.empty((v.shape[0], 3), dtype=F32)
    vin, out = (C.c_float * 4)(), (C.c_float * 4)()
    for i in range(v.shape[0]):
        vin[0], vin[1], vin[2], vin[3] = *[float(x) for x in v["position"][i]], 1.0
        tr(vin, m, out)
        P[i] = out[0], out[1], out[2]
        vin[0], vin[1], vin[2], vin[3] = *[float(x) for x in v["normal"][i]], 0.0
        tr(vin, nm, out)
        n = np.array([out[0], out[1], out[2]], dtype=F32)
        n3 = (C.c_float * 3)(*n.tolist())
        with np.errstate(all="ignore"):
            N[i] = n / np.sqrt(F32(dot(n3, n3)))
    return P, N


# ============================================================================ the restatement
def miss_record(target):
    r = np.zeros((), dtype=RAY_HIT_DTYPE)
    r["target"], r["triangle"], r["distance"] = target, -1, FLT_MAX
    return r


MUTANTS = ("det_back_le", "det_front_ge", "absdet_le", "uv_sum_ge", "dist_le", "key_le_max", "key_unchecked", "key_flush", "fold_le")


def intersect(origin, direction, P, idx, mask, order, fused, u_sense=">", mut=(), probe=None):
    """RayIntersectsTriangle + `if (distance < 0)` over all triangles: (alive, distance, u, v, normalised direction).  `mut` names
    host mutants (MUTANTS; () = the reference); `probe`, if given, is called with (det, alive before the distance test, alive, dist) and changes nothing."""
    o = np.asarray(origin, dtype=F32)
    d = normalize3v(np.asarray(direction, dtype=F32), order)                 # :69
    tri = np.asarray(idx, dtype=np.int64).reshape(-1)
    tri = tri[:(tri.shape[0] // 3) * 3].reshape(-1, 3)
    with np.errstate(all="ignore"):
        v0, v1, v2 = P[tri[:, 0]], P[tri[:, 1]], P[tri[:, 2]]
        e1, e2 = v1 - v0, v2 - v0
        pvec = cross3v(d, e2, fused)
        det = dot3v(e1, pvec, order)
        alive = np.ones(tri.shape[0], dtype=bool)
        if mask & 1:
            alive &= ~((det <= EPS) if "det_back_le" in mut else (det < EPS))
        if mask & 2:
            alive &= ~((det >= -EPS) if "det_front_ge" in mut else (det > -EPS))
        alive &= ~((np.abs(det) <= EPS) if "absdet_le" in mut else (np.abs(det) < EPS))
        inv = F32(1.0) / det
        tvec = o - v0
        u = dot3v(tvec, pvec, order) * inv
        alive &= ~((u < 0) | ((u >= 1) if u_sense == ">=" else (u > 1)))
        qvec = cross3v(tvec, e1, fused)
        v = dot3v(d, qvec, order) * inv
        alive &= ~((v < 0) | ((u + v >= 1) if "uv_sum_ge" in mut else (u + v > 1)))
        dist = dot3v(e2, qvec, order) * inv
        before = alive.copy()
        alive &= ~((dist <= 0) if "dist_le" in mut else (dist < 0))
    if probe is not None:
        probe(det, before, alive, dist)
    return alive, dist, u, v, d, tri


def winner(alive, dist, rule="serial", mut=()):
    """Index of the triangle RaycastInternal keeps, or None.  rule: 'serial' = the reference (strict `<` from float.MaxValue over
    0, 1, 2, ...); 'le' = the mutant `<=` (the LAST of equals); 'rawbits' = the mutant that orders the unsigned distance words
    without mapping -0.0 to +0.0.  mut: 'key_le_max' lets float.MaxValue itself win, 'key_unchecked' lets every surviving distance
    win, NaN and +Inf included, in the order of their words (-0.0 as +0.0), 'key_flush' orders subnormal distances as zero."""
    with np.errstate(all="ignore"):
        cand = alive & ((dist <= FLT_MAX) if "key_le_max" in mut else (dist < FLT_MAX))
    if "key_unchecked" in mut:
        cand = alive.copy()
    if not cand.any():
        return None
    if "key_unchecked" in mut or "key_flush" in mut:
        w = np.ascontiguousarray(dist).view(np.uint32).astype(np.uint64)
        w = np.where(w == 0x80000000, np.uint64(0), w)
        if "key_flush" in mut:
            w = np.where(w < 0x00800000, np.uint64(0), w)
        key = (w << np.uint64(32)) | np.arange(dist.shape[0], dtype=np.uint64)
        return int(np.argmin(np.where(cand, key, np.uint64(0xffffffffffffffff))))
    if rule == "rawbits":
        key = (np.ascontiguousarray(dist).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(dist.shape[0], dtype=np.uint64)
        return int(np.argmin(np.where(cand, key, np.uint64(0xffffffffffffffff))))
    d = np.where(cand, dist, F32(np.inf))
    if rule == "le":
        return int(d.shape[0] - 1 - np.argmin(d[::-1]))
    return int(np.argmin(d))                                                 # first occurrence of the minimum; -0.0 == +0.0


def raycast(origin, direction, P, N, idx, mask, order, fused, target=0, rule="serial", u_sense=">", mut=(), probe=None):
    """Physics.Raycast for one ray and one mesh whose world arrays are P, N: one RAY_HIT_DTYPE record."""
    alive, dist, u, v, d, tri = intersect(origin, direction, P, idx, mask, order, fused, u_sense, mut, probe)
    w = winner(alive, dist, rule, mut)
    r = miss_record(target)
    if w is None:
        return r
    with np.errstate(all="ignore"):
        b = (F32(1.0) - u[w]) - v[w], u[w], v[w]                             # :177
        n0, n1, n2 = N[tri[w, 0]], N[tri[w, 1]], N[tri[w, 2]]
        n = (n0 * b[0] + n1 * b[1]) + n2 * b[2]                              # :99
        r["found"], r["triangle"], r["distance"] = 1, w, dist[w]
        r["normal"] = normalize3v(n, order)
        r["point"] = np.asarray(origin, dtype=F32) + d * dist[w]             # :100
    return r


def fold_nearest(row, mut=()):
    """The callers' `if (hit && distance < best)` over one ray's records in target order, from "not found" (mut 'fold_le': `<=`)."""
    best = miss_record(-1)
    for r in row:
        if r["found"] and (not best["found"] or (r["distance"] <= best["distance"] if "fold_le" in mut else r["distance"] < best["distance"])):
            best = r.copy()
    return best


def same_records(got, want):
    """Integer fields equal; float fields the same 32-bit words, a NaN word of the reference matched by any NaN (cull_edge_cases)."""
    from cull_edge_cases import same_words
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    if got.shape != want.shape:
        return False
    return all(np.array_equal(got[f], want[f]) for f in ("found", "target", "triangle")) and \
        all(same_words(got[f], want[f]) for f in ("distance", "point", "normal"))


def show(r):
    from cull_edge_cases import words
    return f"found {int(r['found'])} target {int(r['target'])} tri {int(r['triangle'])} d {words(r['distance'])} p {words(r['point'])} n {words(r['normal'])}"


# ============================================================================ cases
def make_vertices(positions, normals=None):
    p = np.asarray(positions, dtype=F32).reshape(-1, 3)
    v = np.zeros(p.shape[0], dtype=VERTEX_DTYPE)
    v["position"] = p
    v["normal"] = np.asarray(normals, dtype=F32).reshape(-1, 3) if normals is not None else np.tile(F32([0, 0, 1]), (p.shape[0], 1))
    v["color"] = 1.0
    return v


@dataclasses.dataclass
class Target:
    vertices: np.ndarray
    indices: np.ndarray
    model: np.ndarray = dataclasses.field(default_factory=hm.identity)
    normal_matrix: np.ndarray = None
    world: dict = dataclasses.field(default_factory=dict)      # (oracle variant, Transform flag) -> world positions, normals

    def __post_init__(self):
        self.indices = np.ascontiguousarray(self.indices, dtype=np.uint16).reshape(-1)
        if self.normal_matrix is None:
            self.normal_matrix = hm.normal_matrix(self.model)
            assert self.normal_matrix is not None


@dataclasses.dataclass
class Case:
    name: str
    origins: np.ndarray
    directions: np.ndarray
    targets: list
    mask: int = 1
    expect: object = None              # per (ray, target): True / False = found, or None = not stated; a list over rays x targets

    def __post_init__(self):
        self.origins = np.asarray(self.origins, dtype=F32).reshape(-1, 3)
        self.directions = np.asarray(self.directions, dtype=F32).reshape(-1, 3)


KAT_POS = [(0, 0, 0), (1, 0, 0), (0, 1, 0)]
DOWN, UP = (0, 0, -1), (0, 0, 1)


def kat_target(reverse=False):
    return Target(make_vertices(KAT_POS), [0, 2, 1] if reverse else [0, 1, 2])


def host_cases():
    """Named single-mesh cases with their stated outcome (expect = found, per ray)."""
    front, back = kat_target(), kat_target(True)
    sub = np.nextafter(F32(0), F32(-1))                                     # one ULP below u = 0
    cs = [Case("kat", [(.25, .25, 1)], [(0, 0, -2)], [front], 1, [True])]
    for mask, f, b in ((0, True, True), (1, True, False), (2, False, True), (3, False, False)):
        cs.append(Case(f"mask{mask}_front_winding", [(.25, .25, 1)], [DOWN], [front], mask, [f]))
        cs.append(Case(f"mask{mask}_reversed_winding", [(.25, .25, 1)], [DOWN], [back], mask, [b]))
    cs.append(Case("edges_inclusive", [(0, .25, 1), (.25, 0, 1), (.5, .5, 1), (0, 0, 1), (1, 0, 1), (0, 1, 1)], [DOWN] * 6, [front], 1, [True] * 6))
    cs.append(Case("one_ulp_outside_u0", [(sub, .25, 1), (-1e-7, .25, 1)], [DOWN] * 2, [front], 1, [False, False]))
    cs.append(Case("zero_direction", [(.25, .25, 1)], [(0, 0, 0)], [front], 0, [False]))
    cs.append(Case("triangle_behind_origin", [(.25, .25, -1)], [DOWN], [front], 0, [False]))
    cs.append(Case("origin_on_plane_front", [(.25, .25, 0)], [DOWN], [front], 1, [True]))           # distance +0.0
    cs.append(Case("origin_on_plane_behind_mask0", [(.25, .25, 0)], [UP], [front], 0, [True]))      # distance -0.0
    cs.append(Case("nan_origin", [(np.nan, .25, 1)], [DOWN], [front], 0, [False]))
    cs.append(Case("inf_direction", [(.25, .25, 1)], [(0, 0, -np.inf)], [front], 0, [False]))
    return cs


def _small_triangles(rng, n):
    """n small triangles well away from the line x = y = .25 the count / tie rays run along (x in [4, 9])."""
    c = rng.uniform([4, -3, -3], [9, 3, 3], size=(n, 1, 3))
    p = (c + rng.uniform(-0.2, 0.2, size=(n, 3, 3))).astype(F32).reshape(-1, 3)
    nrm = rng.normal(size=(3 * n, 3)).astype(F32)
    return p, nrm


def count_case(T, where, seed=11):
    """One target of T triangles whose only hit is the KAT triangle, placed last or first."""
    rng = np.random.default_rng(seed + T)
    n_other = max(T - 1, 0)
    p, nrm = _small_triangles(rng, n_other)
    if T == 0:
        pos, normals, idx = np.zeros((0, 3), F32), np.zeros((0, 3), F32), np.zeros(0, np.uint16)
    else:
        kat = np.asarray(KAT_POS, dtype=F32)
        katn = rng.normal(size=(3, 3)).astype(F32)
        pos = np.concatenate([p, kat]) if where == "last" else np.concatenate([kat, p])
        normals = np.concatenate([nrm, katn]) if where == "last" else np.concatenate([katn, nrm])
        idx = np.arange(3 * T, dtype=np.uint16)
    hit = T - 1 if where == "last" else 0
    return Case(f"count_T{T}_{where}", [(.25, .25, 1)], [DOWN], [Target(make_vertices(pos, normals), idx)], 1, [T > 0]), hit


def twin_case(T, ia, ib, seed=23):
    """Coplanar twins at triangle indices ia < ib: the same positions, different normals; the lower index wins."""
    rng = np.random.default_rng(seed + T + ia)
    p, nrm = _small_triangles(rng, T)
    p = p.reshape(T, 3, 3); nrm = nrm.reshape(T, 3, 3)
    kat = np.asarray(KAT_POS, dtype=F32) + F32([0, 0, -.5])
    p[ia] = kat; p[ib] = kat
    nrm[ia] = F32([0, 0, 1]); nrm[ib] = F32([1, 0, 0])
    t = Target(make_vertices(p.reshape(-1, 3), nrm.reshape(-1, 3)), np.arange(3 * T, dtype=np.uint16))
    return Case(f"twins_T{T}_{ia}_{ib}", [(.25, .25, 1)], [DOWN], [t], 1, [True])


def zero_twin_case(minus_first):
    """Mask 0, origin on the plane: the front winding gives +0.0, the reversed one -0.0; they tie, the lower index wins and its
    OWN word comes back."""
    pos = np.concatenate([np.asarray(KAT_POS, dtype=F32)] * 2)
    plus, minus = [0, 1, 2], [3, 5, 4]
    idx = minus + plus if minus_first else plus + minus
    t = Target(make_vertices(pos, [(0, 0, 1)] * 3 + [(0, 1, 0)] * 3), idx)
    return Case("zero_twins_minus_first" if minus_first else "zero_twins_plus_first", [(.25, .25, 0)], [DOWN], [t], 0, [True])


def tie_cases():
    return [twin_case(513, 0, 512), twin_case(513, 64, 257), twin_case(2, 0, 1), zero_twin_case(False), zero_twin_case(True)]


def _model(rng):
    """rotation x non-uniform scale x translation"""
    s = np.eye(4, dtype=F32)
    s[0, 0], s[1, 1], s[2, 2] = rng.uniform(0.5, 2.0, 3).astype(F32)
    r = hm.multiply(hm.create_rotation_y(rng.uniform(0, 6.28)), hm.create_rotation_x(rng.uniform(0, 6.28)))
    return hm.multiply(hm.multiply(r, s), hm.create_translation(*rng.uniform(-2, 2, 3))).astype(F32)


def shape_case(n_rays, n_targets, seed=31):
    """n_targets meshes of 70 random triangles under models of their own; with three targets the middle one carries an all-zero
    normal matrix (NaN normals).  Rays start around the scene and aim at world-space triangle centres, so a good part of them hit."""
    rng = np.random.default_rng(seed + 7 * n_rays + n_targets)
    targets, centres = [], []
    for t in range(n_targets):
        c = rng.uniform(-1.5, 1.5, size=(70, 1, 3))
        p = (c + rng.uniform(-0.5, 0.5, size=(70, 3, 3))).astype(F32).reshape(-1, 3)
        m = _model(rng)
        nm = np.zeros((4, 4), dtype=F32) if (n_targets == 3 and t == 1) else None
        targets.append(Target(make_vertices(p, rng.normal(size=(210, 3))), np.arange(210, dtype=np.uint16), m, nm))
        world = np.concatenate([p.astype(np.float64), np.ones((210, 1))], axis=1) @ m.astype(np.float64)
        centres.append(world[:, :3].reshape(70, 3, 3).mean(axis=1))
    centres = np.concatenate(centres)
    o = rng.uniform(-6, 6, size=(n_rays, 3)).astype(F32)
    aim = centres[rng.integers(0, centres.shape[0], n_rays)]
    d = (aim - o + rng.normal(scale=0.02, size=(n_rays, 3))).astype(F32)
    return Case(f"shape_{n_rays}x{n_targets}", o, d, targets, 0)


def nearest_tie_case():
    """Three targets: the same mesh under the same model twice (equal distances: the FIRST wins), and one nearer for ray 1 only;
    ray 2 misses everything."""
    a, b = kat_target(), kat_target()
    near = Target(make_vertices(np.asarray(KAT_POS, dtype=F32) + F32([2, 0, .5])), [0, 1, 2])
    return Case("nearest_ties", [(.25, .25, 1), (2.25, .25, 1), (-5, -5, 1)], [DOWN] * 3, [a, b, near], 1)


@functools.lru_cache(maxsize=None)
def dust2_meshes():
    from softwarerenderer_amd.modelloader import Model
    model = Model().LoadModel(os.path.join(ROOT, "tests", "golden", "models", "dust2", "scene.gltf"))
    return tuple((np.ascontiguousarray(m.Vertices), np.ascontiguousarray(m.Indices, dtype=np.uint16).reshape(-1)) for m in model.Meshes)


def dust2_case():
    """42 rays shaped like MoveWithSlide's (CharacterController.cs:340-357): 6 capsule positions at the median vertex +- 0.3 x extent
    (default_rng(5)), 7 of the 37 ring rays of radius 0.3 each, at height +0.5, all of a position along its move direction; the 11
    meshes under identity matrices."""
    meshes = dust2_meshes()
    allp = np.concatenate([v["position"] for v, _ in meshes]).astype(np.float64)
    med, ext = np.median(allp, axis=0), allp.max(axis=0) - allp.min(axis=0)
    rng = np.random.default_rng(5)
    o, d = [], []
    for _ in range(6):
        pos = med + rng.uniform(-0.3, 0.3, 3) * ext
        ang = rng.uniform(0, 2 * np.pi)
        move = np.array([np.cos(ang), rng.uniform(-0.2, 0.2), np.sin(ang)])
        for h in range(0, 35, 5):
            a = 2 * np.pi * h / 37
            o.append(pos + np.array([0.3 * np.cos(a), 0.5, 0.3 * np.sin(a)])); d.append(move)
    I = hm.identity()
    return Case("dust2_42_rays", np.asarray(o), np.asarray(d), [Target(v, i, I, I.copy()) for v, i in meshes], 1)


# ============================================================================ a case on the reference
def reference(lib, variant, case, fused=False, rule="serial", u_sense=">", flag=None, mut=(), probe=None):
    """(n_rays, n_targets) records of `case` under the oracle build `lib`, its run-time Transform flag `flag` (None = the build's
    default) and the given Cross model.  The world arrays are kept on the Target per (variant, flag).  `mut` / `probe`: see intersect."""
    from cull_edge_cases import oracle_flags
    order = DOT_ORDER[variant]
    out = np.zeros((case.origins.shape[0], len(case.targets)), dtype=RAY_HIT_DTYPE)
    for t, tg in enumerate(case.targets):
        key = (variant, flag)
        if key not in tg.world:
            with oracle_flags(lib, flag):
                tg.world[key] = world_arrays(lib, tg.vertices, tg.model, tg.normal_matrix)
        P, N = tg.world[key]
        for r in range(case.origins.shape[0]):
            out[r, t] = raycast(case.origins[r], case.directions[r], P, N, tg.indices, case.mask, order, fused, t, rule, u_sense, mut, probe)
    return out
