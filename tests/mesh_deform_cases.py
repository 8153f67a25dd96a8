"""Cases and the numpy float32 restatement of the mesh deforms (test helper; not part of the package).

csrc/swr_mesh_deform.hip.h rewrites a retained mesh's vertices on the GPU: swr_mesh_blend (every scalar of a record =
nm_lerp(a, b, t), the clipper's Lerp) and swr_mesh_skin (linear-blend skinning by a joint palette in the System.Numerics model).
`blend` and `skin` below restate them from helpers the test tree already has, so the arithmetic has one definition here too:

  * geometry_edge_scenes.shaders_lerp / fma32              Shaders.Lerp in both models of SWR_NUMERICS_FMA
  * vertex_probe_cases.transform4 / transform_normal3 / _madd   Vector4.Transform, Vector3.TransformNormal and the madd, fused or not
  * raycast_cases.normalize3v                              Vector3.Normalize in the three dot orders of SWR_DOT_PAIRWISE
    (vertex_probe_cases.normalize3 is the same expression in the product build's order: held equal in test_mesh_deform_host.py)

Results are compared word for word (uint32 views); a NaN is compared as NaN-ness only (its payload is the hardware's)."""
from __future__ import annotations

import functools

import numpy as np

import geometry_edge_scenes as G
import raycast_cases as RC
import vertex_probe_cases as VP
from softwarerenderer_amd.rasterizer import VERTEX_DTYPE

F32 = np.float32
NM_TRANSFORM_FMA, NM_TRANSFORM_NORMAL_FMA = VP.NM_TRANSFORM_FMA, VP.NM_TRANSFORM_NORMAL_FMA
DOT_ORDER = RC.DOT_ORDER                      # library / oracle variant name -> SWR_DOT_PAIRWISE

# k_mesh_blend: 128 threads, one 16-byte word each (42 2/3 vertices a block); k_mesh_skin: 128 vertices a block in two slabs of 64.
# 1000 is a multiple of neither; 65 and 257 leave a slab with one live lane
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1000)
T_VALUES = (0.0, 1.0, 0.5, 1.0 / 3.0, -0.25, 1.5, 1e-45, float("nan"))
SPECIALS = (-0.0, 1e-40, 3.4e38, float("inf"))            # -0, a subnormal, near float.MaxValue, Inf


def as_floats(v):
    """(n, 12) float32 view of a vertex array: position 0:3, uv 3:5, normal 5:8, color 8:12."""
    return np.ascontiguousarray(v).view(F32).reshape(-1, 12)


def same_words(got, want):
    """Word for word, NaN against NaN by NaN-ness.  Returns the indices (vertex, scalar) that differ."""
    g, w = as_floats(got), as_floats(want)
    ok = (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))
    return np.argwhere(~ok)


# ============================================================================ restatement
def blend(a, b, t, fused):
    """swr_mesh_blend: dst = nm_lerp(a, b, t) for all twelve scalars; the normal is not renormalised."""
    out = np.zeros(np.asarray(a).shape[0], dtype=VERTEX_DTYPE)
    if out.shape[0]:
        as_floats(out)[:] = G.shaders_lerp(as_floats(a), as_floats(b), t, fused)
    return out


def skin_vertex(pos, nrm, joints, weights, palette, flags, order):
    ft, ftn = bool(flags & NM_TRANSFORM_FMA), bool(flags & NM_TRANSFORM_NORMAL_FMA)
    p4 = np.array([pos[0], pos[1], pos[2], 1.0], dtype=F32)
    rp, rn = np.zeros(3, F32), np.zeros(3, F32)
    with np.errstate(all="ignore"):
        for k in range(4):
            m, w = palette[int(joints[k])], F32(weights[k])
            pk = VP.transform4(p4, m, ft)[:3]                        # Vector3.Transform: x, y, z of Vector4.Transform((p, 1), M)
            nk = VP.transform_normal3(np.asarray(nrm, dtype=F32), m, ftn)
            for c in range(3):
                rp[c] = F32(w * pk[c]) if k == 0 else VP._madd(w, pk[c], rp[c], ft)
                rn[c] = F32(w * nk[c]) if k == 0 else VP._madd(w, nk[c], rn[c], ftn)
    return rp, RC.normalize3v(rn, order)


def skin(v, joints, weights, palette, flags=0, order=0):
    """swr_mesh_skin: all four influences, weights as given, the normal normalised, uv and colour copied."""
    v = np.ascontiguousarray(v)
    out = v.copy()
    pal = np.asarray(palette, dtype=F32).reshape(-1, 4, 4)
    j, w = np.asarray(joints).reshape(-1, 4), np.asarray(weights, dtype=F32).reshape(-1, 4)
    for i in range(v.shape[0]):
        out["position"][i], out["normal"][i] = skin_vertex(v["position"][i], v["normal"][i], j[i], w[i], pal, flags, order)
    return out


# ============================================================================ cases
def key_frame(n, seed):
    """n vertices, each of the twelve scalars different at every vertex (and from every other scalar of the vertex)."""
    rng = np.random.default_rng(seed)
    v = np.zeros(n, dtype=VERTEX_DTYPE)
    f = as_floats(v)
    f[:] = rng.uniform(-4.0, 4.0, size=(n, 12)).astype(F32) + np.arange(12, dtype=F32)[None, :] * F32(8.0)
    return v


def key_frames_special(n=65):
    """Two key frames whose scalars walk through SPECIALS against ordinary values, in both roles (a and b), in every column."""
    a, b = key_frame(n, 901), key_frame(n, 902)
    fa, fb = as_floats(a), as_floats(b)
    k = 0
    for i in range(n):
        for s in range(12):
            if (i + s) % 3 == 0:
                (fa if (k // len(SPECIALS)) % 2 == 0 else fb)[i, s] = F32(SPECIALS[k % len(SPECIALS)])
                k += 1
    return a, b


def indices_for(n):
    """a triangle list over n vertices (retained meshes need indices below n; zero vertices: none)."""
    if n == 0:
        return np.zeros(0, dtype=np.uint16)
    i = np.arange(max(n - 2, 1), dtype=np.int64)
    return np.stack([i, (i + 1) % n, (i + 2) % n], axis=1).astype(np.uint16).reshape(-1)


def rigid_palette(n_joints, seed):
    """n_joints rotations with a translation each (row-vector convention: translation in the fourth row), float32."""
    rng = np.random.default_rng(seed)
    pal = np.zeros((n_joints, 4, 4), dtype=F32)
    for k in range(n_joints):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        pal[k, :3, :3] = q.astype(F32)
        pal[k, 3, :3] = rng.uniform(-2.0, 2.0, 3).astype(F32)
        pal[k, 3, 3] = 1.0
    return pal


@functools.lru_cache(maxsize=None)
def skin_case(n, n_joints, seed=0):
    """(vertices, joints, weights, palette): every vertex has four non-zero weights summing to about one; vertex 0 (if any) uses joint 0
    and vertex n - 1 joint n_joints - 1, in different influence slots."""
    rng = np.random.default_rng(1000 + 7 * n + n_joints + seed)
    v = key_frame(n, 500 + n)
    joints = rng.integers(0, n_joints, size=(n, 4)).astype(np.uint16)
    w = rng.uniform(0.05, 1.0, size=(n, 4))
    weights = (w / w.sum(axis=1, keepdims=True)).astype(F32)
    if n:
        joints[0, 2] = 0
        joints[n - 1, 1] = n_joints - 1
    return v, joints, weights, rigid_palette(n_joints, 77 + n_joints)


def models_differ_case():
    """One vertex whose weighted sum rounds differently under the two Transform models, by hand (identity palette, so
    p_k = position exactly): x = 3, w = (2^-25, 1 - 2^-24, 0, 0).  r0 = 3 * 2^-25 (exact).  Unfused: w1 * 3 = 3 - 0.75 ulp rounds to
    3 - ulp (ulp = 2^-22), plus 0.375 ulp = 3 - 0.625 ulp -> 3 - ulp = 0x403FFFFF.  Fused: 3 - 0.75 ulp + 0.375 ulp = 3 - 0.375 ulp ->
    3 = 0x40400000.  The zero weights then add 0 * 3 and change nothing.  The normal (0, 0, 1): 2^-25 + (1 - 2^-24) = 1 - 2^-25, a tie
    between 1 - 2^-24 and 1, to even: 1, in both models (the product w1 * 1 is exact)."""
    v = np.zeros(1, dtype=VERTEX_DTYPE)
    v["position"][0] = (3.0, 0.0, 0.0)
    v["normal"][0] = (0.0, 0.0, 1.0)
    v["uv"][0] = (0.25, 0.75)
    v["color"][0] = (0.1, 0.2, 0.3, 0.4)
    joints = np.array([[0, 1, 0, 1]], dtype=np.uint16)
    weights = np.array([[2.0 ** -25, 1.0 - 2.0 ** -24, 0.0, 0.0]], dtype=F32)
    palette = np.tile(np.eye(4, dtype=F32), (2, 1, 1))
    return v, joints, weights, palette, {"unfused": 0x403FFFFF, "fused": 0x40400000}
