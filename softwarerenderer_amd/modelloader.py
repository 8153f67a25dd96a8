"""Asset ingestion without Assimp (row N4): glTF 2.0 (+ .bin / data: URIs) and Wavefront OBJ -> the reference's
`Mesh` shape (Shaders.VertexInput[] + ushort[] indices), mirroring `Model` / `Mesh` of ModelLoader.cs.

Host-side: it only PRODUCES inputs of the hot path.  What is reproduced from ModelLoader.cs (file:line):
  * node walk with globalTransform = nodeTransform * parentTransform, row-vector convention   :159-162,296-299
  * positions through Vector3.Transform(pos, global); normals through Normalize(TransformNormal(n, upper 3x3))   :188-191
  * vertex de-duplication on (position, normal, uv) in first-seen order, 16-bit indices        :165-218
  * PostProcessSteps.FlipUVs (v -> 1 - v), white default vertex colour, diffuse texture path  :145-150,184-186,240-270
  * a directory of model files = animation frames sorted by name                              :79-115
Beyond the reference (build-defined): a glTF primitive's JOINTS_0 / WEIGHTS_0 and a skin's inverseBindMatrices are
read and kept beside the vertices they belong to (Mesh.joints, Mesh.weights, Model.Skins), the inputs of Mesh.SkinFrom.
Model.FramePair names the two key frames around a time.  Skeletal animation (build-defined): `animations`
(samplers, channels, STEP / LINEAR) and every node's TRS or matrix are read into Model.Skeletons -- per skin, its joints plus the
ancestors they need, renumbered topologically -- and Model.Clips; Model.UploadSkeleton hands both to the GPU, where the channels are
sampled (softwarerenderer_amd.Skeleton / PoseSet).  CUBICSPLINE raises a ValueError.
Where Assimp's own numerics matter (normal generation when a mesh has none, TRS composition) this loader is
build-defined -- AssimpNet 5.0.0-beta1 is not available, so those results are unpinned.
One deliberate difference: the reference wraps its ushort index silently past 65,535 unique vertices
(ModelLoader.cs:206 `(ushort)vertices.Count`); this loader starts a new Mesh instead, so every mesh is valid.
"""
from __future__ import annotations

import base64
import json
import os
from typing import Dict, List, Optional

import numpy as np

from .rasterizer import VERTEX_DTYPE

F = np.float32
MAX_VERTS = 65535


class Mesh:
    """public class Mesh (ModelLoader.cs:43-60)."""

    def __init__(self, vertices: np.ndarray, indices: np.ndarray, material: Optional[dict] = None, root: str = "",
                 joints: Optional[np.ndarray] = None, weights: Optional[np.ndarray] = None, skin: Optional[int] = None):
        self.Vertices = vertices
        self.BaseVertices = vertices.copy()
        self.Indices = indices
        self.Material = material or {}
        self.ModelRootPath = root
        self.joints = joints               # (n, 4) uint16 indices into the skin's joint list, or None: JOINTS_0
        self.weights = weights             # (n, 4) float32, as stored (not renormalised), or None: WEIGHTS_0
        self.Skin = skin                   # index into Model.Skins, or None
        self._gpu = None

    def Upload(self, device):
        """Retained GPU mesh (softwarerenderer_amd.Mesh); its SphereBounds is FrustumCuller.CalculateBoundingSphere on the GPU."""
        from .rasterizer import Mesh as GpuMesh
        if self._gpu is None:
            self._gpu = GpuMesh(device, self.Vertices, self.Indices)
            if self.joints is not None and self.weights is not None:
                self._gpu.SetSkin(self.joints, self.weights)
        return self._gpu


def _transform_points(p: np.ndarray, m: np.ndarray) -> np.ndarray:
    """Vector3.Transform(p, M): ((x*row1 + y*row2) + z*row3) + row4, float32, row-vector convention."""
    x, y, z = p[:, 0:1], p[:, 1:2], p[:, 2:3]
    r = x * m[0:1, :3]
    r = r + y * m[1:2, :3]
    r = r + z * m[2:3, :3]
    return (r + m[3:4, :3]).astype(F)


def _transform_normals(n: np.ndarray, m: np.ndarray) -> np.ndarray:
    """Vector3.Normalize(Vector3.TransformNormal(n, rotationOnly)) (ModelLoader.cs:189-191)."""
    x, y, z = n[:, 0:1], n[:, 1:2], n[:, 2:3]
    r = x * m[0:1, :3]
    r = r + y * m[1:2, :3]
    r = (r + z * m[2:3, :3]).astype(F)
    ln = np.sqrt(((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]).astype(F)).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (r / ln[:, None]).astype(F)


def _quat_to_matrix(q) -> np.ndarray:
    """Matrix4x4.CreateFromQuaternion (row-vector convention), q = (x, y, z, w)."""
    x, y, z, w = (F(v) for v in q)
    xx, yy, zz = x * x, y * y, z * z
    xy, wz, xz, wy, yz, wx = x * y, z * w, z * x, y * w, y * z, x * w
    m = np.eye(4, dtype=F)
    m[0, 0] = F(1) - F(2) * (yy + zz); m[0, 1] = F(2) * (xy + wz); m[0, 2] = F(2) * (xz - wy)
    m[1, 0] = F(2) * (xy - wz); m[1, 1] = F(1) - F(2) * (zz + xx); m[1, 2] = F(2) * (yz + wx)
    m[2, 0] = F(2) * (xz + wy); m[2, 1] = F(2) * (yz - wx); m[2, 2] = F(1) - F(2) * (yy + xx)
    return m


def _node_matrix(node: dict) -> np.ndarray:
    if "matrix" in node:
        # glTF stores column-major for column vectors; read row-major it IS the row-vector matrix
        return np.asarray(node["matrix"], dtype=F).reshape(4, 4)
    s = np.eye(4, dtype=F)
    if "scale" in node:
        s[0, 0], s[1, 1], s[2, 2] = (F(v) for v in node["scale"])
    r = _quat_to_matrix(node["rotation"]) if "rotation" in node else np.eye(4, dtype=F)
    t = np.eye(4, dtype=F)
    if "translation" in node:
        t[3, 0], t[3, 1], t[3, 2] = (F(v) for v in node["translation"])
    return ((s @ r).astype(F) @ t).astype(F)          # row vectors: scale, then rotate, then translate


def _face_normals(pos: np.ndarray, tris: np.ndarray) -> np.ndarray:
    """Stand-in for Assimp's GenerateNormals when a mesh has none: area-weighted vertex normals (build-defined)."""
    n = np.zeros_like(pos, dtype=np.float64)
    a, b, c = pos[tris[:, 0]], pos[tris[:, 1]], pos[tris[:, 2]]
    fn = np.cross(b - a, c - a)
    for k in range(3):
        np.add.at(n, tris[:, k], fn)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    ln[ln == 0] = 1.0
    return (n / ln).astype(F)


def _build_meshes(pos, nrm, uv, col, tri_idx, material, root, joints=None, weights=None, skin=None) -> List[Mesh]:
    """De-duplicate on (position, normal, uv) in first-seen order (ModelLoader.cs:165-218); split at 65,535 vertices.  Skin
    attributes (joints, weights: four per source vertex) follow the vertex they belong to: they join the key, so two corners that agree
    in position, normal and uv and differ in their influences stay two vertices; without them the key is the reference's."""
    meshes: List[Mesh] = []
    keys = np.concatenate([pos, nrm, uv], axis=1).astype(F)
    key_bytes = keys.view(np.uint8).reshape(keys.shape[0], -1)
    skinned = joints is not None and weights is not None
    if skinned:
        key_bytes = np.concatenate([key_bytes, np.ascontiguousarray(joints, dtype=np.uint16).view(np.uint8).reshape(keys.shape[0], -1),
                                    np.ascontiguousarray(weights, dtype=F).view(np.uint8).reshape(keys.shape[0], -1)], axis=1)
    table: Dict[bytes, int] = {}
    verts: List[int] = []
    idx: List[int] = []

    def emit():
        if not idx:
            return
        v = np.zeros(len(verts), dtype=VERTEX_DTYPE)
        sel = np.asarray(verts, dtype=np.int64)
        v["position"], v["uv"], v["normal"], v["color"] = pos[sel], uv[sel], nrm[sel], col[sel]
        if skinned:
            meshes.append(Mesh(v, np.asarray(idx, dtype=np.uint16), material, root, np.ascontiguousarray(joints[sel], dtype=np.uint16),
                               np.ascontiguousarray(weights[sel], dtype=F), skin))
        else:
            meshes.append(Mesh(v, np.asarray(idx, dtype=np.uint16), material, root))

    for tri in tri_idx.reshape(-1, 3):
        new = sum(1 for vi in tri if key_bytes[vi].tobytes() not in table)
        if len(verts) + new > MAX_VERTS:               # the reference would wrap here; start a fresh mesh instead
            emit()
            table, verts, idx = {}, [], []
        for vi in tri:
            kb = key_bytes[vi].tobytes()
            j = table.get(kb)
            if j is None:
                j = len(verts)
                table[kb] = j
                verts.append(int(vi))
            idx.append(j)
    emit()
    return meshes


# ------------------------------------------------------------------------------------------ glTF
_COMP = {5120: np.int8, 5121: np.uint8, 5122: np.int16, 5123: np.uint16, 5125: np.uint32, 5126: np.float32}
_NCOMP = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT4": 16}


class _Gltf:
    def __init__(self, path: str):
        self.root = os.path.dirname(os.path.abspath(path))
        self.doc = json.load(open(path, "r"))
        self.buffers = []
        for b in self.doc.get("buffers", []):
            uri = b.get("uri", "")
            if uri.startswith("data:"):
                self.buffers.append(base64.b64decode(uri.split(",", 1)[1]))
            else:
                self.buffers.append(open(os.path.join(self.root, uri), "rb").read())

    def accessor(self, i: int) -> np.ndarray:
        a = self.doc["accessors"][i]
        dt, nc = np.dtype(_COMP[a["componentType"]]), _NCOMP[a["type"]]
        bv = self.doc["bufferViews"][a["bufferView"]]
        off = bv.get("byteOffset", 0) + a.get("byteOffset", 0)
        stride = bv.get("byteStride", 0) or dt.itemsize * nc
        buf = self.buffers[bv["buffer"]]
        raw = np.frombuffer(buf, dtype=np.uint8, count=(a["count"] - 1) * stride + dt.itemsize * nc, offset=off)
        rows = np.lib.stride_tricks.as_strided(raw, shape=(a["count"], dt.itemsize * nc), strides=(stride, 1))
        out = np.ascontiguousarray(rows).view(dt).reshape(a["count"], nc)
        if a.get("normalized") and dt.kind in "iu":
            out = out.astype(np.float32) / float(np.iinfo(dt).max)
        return out

    def material(self, i: Optional[int]) -> dict:
        if i is None:
            return {}
        m = self.doc.get("materials", [])[i]
        pbr = m.get("pbrMetallicRoughness", {})
        out = {"Name": m.get("name", ""), "BaseColor": tuple(pbr.get("baseColorFactor", (1, 1, 1, 1))),
               "Metallic": pbr.get("metallicFactor", 0.0), "Roughness": pbr.get("roughnessFactor", 0.5), "TexturePaths": {}}
        tex = pbr.get("baseColorTexture")
        if tex is not None:
            src = self.doc["textures"][tex["index"]].get("source")
            if src is not None and "uri" in self.doc["images"][src]:
                out["TexturePaths"]["Diffuse"] = os.path.join(self.root, self.doc["images"][src]["uri"])   # ModelLoader.cs:266-268
        return out


def _gltf_skins(g: "_Gltf") -> List[dict]:
    """The document's skins: {"Name", "Joints": node indices, "InverseBindMatrices": (n, 4, 4) float32}.  glTF stores the matrices
    column-major for column vectors; read row-major they ARE the row-vector matrices (as _node_matrix reads a node's).  A skin
    without the accessor has identities."""
    out = []
    for s in g.doc.get("skins", []):
        joints = [int(j) for j in s.get("joints", [])]
        if "inverseBindMatrices" in s:
            ibm = g.accessor(s["inverseBindMatrices"]).astype(F).reshape(-1, 4, 4)
        else:
            ibm = np.tile(np.eye(4, dtype=F), (len(joints), 1, 1))
        out.append({"Name": s.get("name", ""), "Joints": joints, "InverseBindMatrices": np.ascontiguousarray(ibm)})
    return out


def compose_trs(t, r, s) -> np.ndarray:
    """A node's local matrix from T, R (xyzw) and S, as the GPU composes it (include/swr.h "SKELETAL ANIMATION"): row i of
    Matrix4x4.CreateFromQuaternion(R) times s_i, one rounding each; row 4 = (t, 1); column 4 = (0, 0, 0, 1)."""
    from .hostmath import create_from_quaternion
    m = create_from_quaternion(r)
    sc = np.asarray(s, dtype=F).reshape(3)
    with np.errstate(all="ignore"):
        for i in range(3):
            m[i, :3] = m[i, :3] * sc[i]
    m[3, :3] = np.asarray(t, dtype=F).reshape(3)
    return m


def _gltf_skeletons(g: "_Gltf", skins: List[dict]) -> List[dict]:
    """One skeleton per skin: the skin's joints plus every ancestor they need, renumbered so that parent < child (a pre-order walk
    from the document's roots; a skin may list its joints child-first, and a joint may hang under a node that is no joint).
      "Nodes"  glTF node index of each skeleton node        "Parent"  skeleton index of its parent, -1 for a root
      "RestLocal" (n, 4, 4), "RestT" (n, 3), "RestR" (n, 4) xyzw, "RestS" (n, 3): a TRS node's matrix is compose_trs of its
               values (defaults 0, identity, 1); a node given as a matrix keeps it, with T, R, S at their defaults (glTF animates
               TRS nodes only)
      "JointNode" skeleton index of each joint, in the skin's order        "InverseBind" (n_joints, 4, 4)"""
    nodes = g.doc.get("nodes", [])
    parent_of = {}
    for i, n in enumerate(nodes):
        for ch in n.get("children", []):
            parent_of[int(ch)] = i
    out = []
    for skin in skins:
        need = set()
        for j in skin["Joints"]:
            k = j
            while k is not None and k not in need:
                need.add(k)
                k = parent_of.get(k)
        order: List[int] = []
        stack = sorted((k for k in need if parent_of.get(k) is None), reverse=True)
        while stack:                                   # pre-order: a parent is numbered before its children
            k = stack.pop()
            order.append(k)
            stack.extend(sorted((int(ch) for ch in nodes[k].get("children", []) if int(ch) in need), reverse=True))
        index = {k: i for i, k in enumerate(order)}
        n = len(order)
        sk = {"Name": skin["Name"], "Nodes": order, "Parent": np.array([index.get(parent_of.get(k), -1) for k in order], dtype=np.int32),
              "RestLocal": np.zeros((n, 4, 4), dtype=F), "RestT": np.zeros((n, 3), dtype=F), "RestR": np.zeros((n, 4), dtype=F),
              "RestS": np.ones((n, 3), dtype=F), "JointNode": np.array([index[j] for j in skin["Joints"]], dtype=np.int32),
              "InverseBind": skin["InverseBindMatrices"]}
        sk["RestR"][:, 3] = 1.0
        for i, k in enumerate(order):
            node = nodes[k]
            if "matrix" in node:
                sk["RestLocal"][i] = np.asarray(node["matrix"], dtype=F).reshape(4, 4)
                continue
            if "translation" in node:
                sk["RestT"][i] = node["translation"]
            if "rotation" in node:
                sk["RestR"][i] = node["rotation"]
            if "scale" in node:
                sk["RestS"][i] = node["scale"]
            sk["RestLocal"][i] = compose_trs(sk["RestT"][i], sk["RestR"][i], sk["RestS"][i])
        out.append(sk)
    return out


def _gltf_clips(g: "_Gltf") -> List[dict]:
    """The document's animations: {"Name", "Channels": [{"Node": glTF node index, "Path": "translation" | "rotation" | "scale",
    "Interpolation": "STEP" | "LINEAR", "Times": (n,) float32, "Values": (n, 3 | 4) float32}]}.  Channels without a target node and
    morph-target weights are skipped (not built); CUBICSPLINE raises."""
    out = []
    for a in g.doc.get("animations", []):
        chans = []
        for ch in a.get("channels", []):
            tgt = ch.get("target", {})
            if "node" not in tgt or tgt.get("path") not in ("translation", "rotation", "scale"):
                continue
            smp = a["samplers"][ch["sampler"]]
            interp = smp.get("interpolation", "LINEAR")
            if interp == "CUBICSPLINE":
                raise ValueError(f"animation {a.get('name', len(out))!r}: CUBICSPLINE interpolation is not supported (STEP and LINEAR are)")
            if interp not in ("STEP", "LINEAR"):
                raise ValueError(f"animation {a.get('name', len(out))!r}: unknown interpolation {interp!r}")
            chans.append({"Node": int(tgt["node"]), "Path": tgt["path"], "Interpolation": interp,
                          "Times": np.ascontiguousarray(g.accessor(smp["input"]).astype(F).reshape(-1)),
                          "Values": np.ascontiguousarray(g.accessor(smp["output"]).astype(F))})
        out.append({"Name": a.get("name", ""), "Channels": chans})
    return out


def _load_gltf(path: str, skins_out: Optional[list] = None, skeletons_out: Optional[list] = None, clips_out: Optional[list] = None) -> List[Mesh]:
    g = _Gltf(path)
    doc = g.doc
    meshes: List[Mesh] = []
    skins = _gltf_skins(g)
    if skins_out is not None:
        skins_out.extend(skins)
    if skeletons_out is not None:
        skeletons_out.extend(_gltf_skeletons(g, skins))
    if clips_out is not None:
        clips_out.extend(_gltf_clips(g))

    def process(node_i: int, parent: np.ndarray):
        node = doc["nodes"][node_i]
        glob = (_node_matrix(node) @ parent).astype(F)                         # ModelLoader.cs:162
        rot = np.eye(4, dtype=F)
        rot[:3, :3] = glob[:3, :3]                                             # :164-168
        if "mesh" in node:
            for prim in doc["meshes"][node["mesh"]]["primitives"]:
                if prim.get("mode", 4) != 4:
                    continue                                                   # only triangle lists (face.IndexCount != 3 -> skipped, :178)
                att = prim["attributes"]
                pos = g.accessor(att["POSITION"]).astype(F)
                n = pos.shape[0]
                tri = g.accessor(prim["indices"]).reshape(-1).astype(np.int64) if "indices" in prim else np.arange(n, dtype=np.int64)
                tri = tri[: (tri.size // 3) * 3]
                nrm = g.accessor(att["NORMAL"]).astype(F) if "NORMAL" in att else _face_normals(pos, tri.reshape(-1, 3))
                uv = g.accessor(att["TEXCOORD_0"]).astype(F)[:, :2] if "TEXCOORD_0" in att else np.zeros((n, 2), dtype=F)
                uv = uv.copy()
                if "TEXCOORD_0" in att:
                    uv[:, 1] = F(1.0) - uv[:, 1]                               # PostProcessSteps.FlipUVs, :148
                col = np.ones((n, 4), dtype=F)
                if "COLOR_0" in att:
                    c = g.accessor(att["COLOR_0"]).astype(F)
                    col[:, :c.shape[1]] = c
                joints = weights = None
                if "JOINTS_0" in att and "WEIGHTS_0" in att:
                    joints = g.accessor(att["JOINTS_0"]).astype(np.uint16)[:, :4]        # u8 or u16 indices into the skin's joint list
                    weights = g.accessor(att["WEIGHTS_0"]).astype(F)[:, :4]               # float, or normalised u8 / u16 (accessor)
                meshes.extend(_build_meshes(_transform_points(pos, glob), _transform_normals(nrm, rot), uv, col, tri,
                                            g.material(prim.get("material")), g.root, joints, weights, node.get("skin")))
        for ch in node.get("children", []):
            process(ch, glob)                                                  # :296-299

    scene = doc["scenes"][doc.get("scene", 0)]
    for ni in scene["nodes"]:
        process(ni, np.eye(4, dtype=F))
    return meshes


# ------------------------------------------------------------------------------------------ OBJ
def _load_obj(path: str) -> List[Mesh]:
    root = os.path.dirname(os.path.abspath(path))
    v, vt, vn = [], [], []
    groups: Dict[str, List[tuple]] = {}
    cur = "default"
    for line in open(path, "r"):
        p = line.split()
        if not p or p[0].startswith("#"):
            continue
        if p[0] == "v":
            v.append([float(x) for x in p[1:4]])
        elif p[0] == "vt":
            vt.append([float(p[1]), float(p[2]) if len(p) > 2 else 0.0])
        elif p[0] == "vn":
            vn.append([float(x) for x in p[1:4]])
        elif p[0] == "usemtl":
            cur = p[1] if len(p) > 1 else "default"
        elif p[0] == "f":
            corners = []
            for tok in p[1:]:
                a = (tok.split("/") + ["", ""])[:3]
                vi = int(a[0]); ti = int(a[1]) if a[1] else 0; ni = int(a[2]) if a[2] else 0
                corners.append((vi - 1 if vi > 0 else len(v) + vi, (ti - 1 if ti > 0 else len(vt) + ti) if ti else -1,
                                (ni - 1 if ni > 0 else len(vn) + ni) if ni else -1))
            for k in range(1, len(corners) - 1):                               # Triangulate: fan
                groups.setdefault(cur, []).extend([corners[0], corners[k], corners[k + 1]])
    V = np.asarray(v, dtype=F).reshape(-1, 3)
    VT = np.asarray(vt, dtype=F).reshape(-1, 2)
    VN = np.asarray(vn, dtype=F).reshape(-1, 3)
    meshes: List[Mesh] = []
    ident = np.eye(4, dtype=F)
    for name, corners in groups.items():
        c = np.asarray(corners, dtype=np.int64)
        pos = V[c[:, 0]]
        tri = np.arange(c.shape[0], dtype=np.int64)
        uv = np.zeros((c.shape[0], 2), dtype=F)
        has_t = c[:, 1] >= 0
        if has_t.any():
            uv[has_t] = VT[c[has_t, 1]]
            uv[has_t, 1] = F(1.0) - uv[has_t, 1]                               # FlipUVs
        if (c[:, 2] >= 0).all() and VN.size:
            nrm = VN[c[:, 2]]
        else:
            nrm = _face_normals(pos, tri.reshape(-1, 3))
        col = np.ones((c.shape[0], 4), dtype=F)
        meshes.extend(_build_meshes(_transform_points(pos, ident), _transform_normals(nrm, ident), uv, col, tri,
                                    {"Name": name, "TexturePaths": {}}, root))
    return meshes


# ------------------------------------------------------------------------------------------ Model
class Model:
    """public class Model (ModelLoader.cs:62-349): Meshes, Lights, AnimationFrames, LoadModel."""

    _model_cache: Dict[str, "Model"] = {}
    SUPPORTED = {".gltf", ".obj"}          # the reference lists .fbx .obj .dae .3ds .blend .gltf .glb (Assimp); here: no Assimp

    def __init__(self):
        self.Meshes: List[Mesh] = []
        self.Lights: list = []             # Light.cs is dead data for the renderer
        self.AnimationFrames: List["Model"] = []
        self.Skins: List[dict] = []        # glTF skins (build-defined): joint node indices and inverse bind matrices, see _gltf_skins
        self.Skeletons: List[dict] = []    # one per skin: its joints and their ancestors in topological order, see _gltf_skeletons
        self.Clips: List[dict] = []        # glTF animations: channels with key times and values, see _gltf_clips

    def ClipChannels(self, skeleton: int, clip: int) -> list:
        """Clips[clip]'s channels on nodes of Skeletons[skeleton], as Skeleton.AddClip takes them: (skeleton node, path,
        interpolation, times, values).  Channels on other nodes are not the skeleton's."""
        index = {k: i for i, k in enumerate(self.Skeletons[skeleton]["Nodes"])}
        return [(index[c["Node"]], c["Path"], c["Interpolation"], c["Times"], c["Values"])
                for c in self.Clips[clip]["Channels"] if c["Node"] in index]

    def UploadSkeleton(self, device, skeleton: int = 0):
        """softwarerenderer_amd.Skeleton of Skeletons[skeleton] with every clip of the model added: clip i of the result is Clips[i]."""
        from .rasterizer import Skeleton
        sk = self.Skeletons[skeleton]
        out = Skeleton(device, sk["Parent"], sk["RestLocal"], sk["RestT"], sk["RestR"], sk["RestS"], sk["JointNode"], sk["InverseBind"])
        for c in range(len(self.Clips)):
            out.AddClip(self.ClipChannels(skeleton, c))
        return out

    def FramePair(self, time: float, fps: float = 30.0):
        """(i, j, t): the key frames AnimationFrames[i] and [j] around `time` seconds at `fps` frames a second, and the blend
        factor t in [0, 1) as a float32 (a fraction that would round up to 1.0 is the float32 just below it) -- Mesh.BlendFrom's
        caller-side helper.  Frame k = floor(time * fps) is where PlayAnimation
        (ModelLoader.cs:331-348) stands after `time`; it wraps as the reference's index does, so the last frame blends into the first."""
        n = len(self.AnimationFrames)
        if n == 0:
            raise ValueError("the model has no animation frames")
        f = float(time) * float(fps)
        k = int(np.floor(f))
        return k % n, (k + 1) % n, min(F(f - k), np.nextafter(F(1.0), F(0.0)))

    def LoadModel(self, file_path: str) -> "Model":
        path = os.path.abspath(file_path)
        cached = Model._model_cache.get(path)
        if cached is not None:                                                  # ModelLoader.cs:80-86,118-124
            self.Meshes, self.Lights, self.AnimationFrames, self.Skins = cached.Meshes, cached.Lights, cached.AnimationFrames, cached.Skins
            self.Skeletons, self.Clips = cached.Skeletons, cached.Clips
            return self
        if os.path.isdir(path):                                                 # a directory = animation frames, :79-115
            files = sorted(f for f in os.listdir(path) if os.path.splitext(f)[1].lower() in Model.SUPPORTED)
            self.AnimationFrames = [Model()._load_single(os.path.join(path, f)) for f in files]
            if self.AnimationFrames:
                self.Meshes, self.Lights, self.Skins = self.AnimationFrames[0].Meshes, self.AnimationFrames[0].Lights, self.AnimationFrames[0].Skins
                self.Skeletons, self.Clips = self.AnimationFrames[0].Skeletons, self.AnimationFrames[0].Clips
        elif os.path.isfile(path):
            self._load_single(path)
        else:
            raise FileNotFoundError(f"Model path not found: {path}")            # :131-134
        Model._model_cache[path] = self
        return self

    def _load_single(self, path: str) -> "Model":
        ext = os.path.splitext(path)[1].lower()
        if ext == ".gltf":
            self.Skins, self.Skeletons, self.Clips = [], [], []
            self.Meshes = _load_gltf(path, self.Skins, self.Skeletons, self.Clips)
        elif ext == ".obj":
            self.Meshes = _load_obj(path)
        else:
            raise ValueError(f"unsupported model format {ext} (this loader reads .gltf and .obj)")
        return self
