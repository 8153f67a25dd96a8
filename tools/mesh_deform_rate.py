#!/usr/bin/env python3
"""Cost of deforming meshes on the GPU, one JSON file (default profiles/r23_mesh_deform.json).  Needs a GPU.
One process on one MI355X, every variant warmed, the variants of a group alternated over --rounds rounds, medians.
  (a) large: swr_mesh_blend and swr_mesh_skin at 65,535 vertices, PER CALL (device events around --launches back-to-back calls on one
      stream, so a call includes the boundary to the next: a launch-bound figure, not the kernel's).  The same arrays every call: they
      stay in the caches;
  (b) hbm: the same calls cycling through --sets (40) distinct sets of 65,535-vertex meshes, 300 to 380 MB in all, more than the 256 MB
      Infinity Cache holds: every call streams from HBM.  Bytes per vertex: blend 96 read + 48 written, skin 48 + 8 + 16 read + 48 written;
  (c) small: the calls on the two meshes of tests/golden/models/gordon_freeman (118 and 477 vertices, 639 triangles), where the launch
      dominates; 16 players x 2 meshes per frame against the frame's front end (0.195 ms alone);
  (d) frames: sixteen skinned players at 1920 x 1080 with an 8-bit asynchronous present, per frame (host clock around --frames frames
      that end in a wait for the last present): swr_mesh_skin into retained targets, beside the path there was before -- the same
      skinning in numpy and every mesh created again with swr_mesh_create (and the old one destroyed).
KERNEL times come from a kernel trace, a run of its own per group:
    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/mesh_deform_rate.py --only GROUP --out FILE
and --trace GROUP=DIR/run_kernel_stats.csv (repeatable) folds them into the JSON as "kernel_trace", with the bandwidth the
algorithm's bytes make of the average kernel time where the group has one vertex count (large, hbm).
usage: python tools/mesh_deform_rate.py [--out FILE] [--rounds N] [--launches N] [--frames N] [--sets N] [--only GROUP] [--trace GROUP=CSV ...]"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from softwarerenderer_amd import Device, MainWindow, Mesh, Rasterizer, Texture, hostmath as hm, scenes   # noqa: E402
from softwarerenderer_amd.modelloader import Model                                                       # noqa: E402
from softwarerenderer_amd.rasterizer import ShaderProgram, VERTEX_DTYPE                                 # noqa: E402
from tools.resolve_rate import COPY_PEAK_GBS, Hip                                                       # noqa: E402

F32 = np.float32
BLEND_BYTES, SKIN_BYTES = 96 + 48, 48 + 8 + 16 + 48           # per vertex, as the algorithm needs them (the palette is cache-resident)
FRONT_END_MS = 0.195                                          # cfg3's front end alone
N_JOINTS = 24


def stats_us(ms):
    v = [x * 1e3 for x in ms]
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "runs": [round(x, 3) for x in v]}


def synthetic_vertices(n, seed):
    rng = np.random.default_rng(seed)
    v = np.zeros(n, dtype=VERTEX_DTYPE)
    v["position"] = rng.uniform(-1, 1, (n, 3)); v["uv"] = rng.uniform(0, 1, (n, 2))
    nr = rng.normal(size=(n, 3)); v["normal"] = nr / np.linalg.norm(nr, axis=1, keepdims=True)
    v["color"] = rng.uniform(0, 1, (n, 4))
    return v


def skin_attributes(v, seed):
    """joints by height band (four neighbouring bands per vertex), weights normalised: what a rigged character looks like to the kernel"""
    rng = np.random.default_rng(seed)
    y = v["position"][:, 1].astype(np.float64)
    band = np.clip(((y - y.min()) / max(float(np.ptp(y)), 1e-9) * (N_JOINTS - 4)).astype(np.int64), 0, N_JOINTS - 4)
    joints = (band[:, None] + np.arange(4)[None, :]).astype(np.uint16)
    w = rng.uniform(0.05, 1.0, (v.shape[0], 4))
    return joints, (w / w.sum(axis=1, keepdims=True)).astype(F32)


def palette(frame, player=0):
    """N_JOINTS rigid joint matrices that sway with the frame number (row-vector convention)"""
    pal = np.zeros((N_JOINTS, 4, 4), dtype=F32)
    for k in range(N_JOINTS):
        a = 0.15 * np.sin(0.21 * frame + 0.5 * k + player)
        c, s = np.cos(a), np.sin(a)
        pal[k] = np.array([[c, 0, -s, 0], [0, 1, 0, 0], [s, 0, c, 0], [0.02 * np.sin(0.13 * frame + k), 0, 0, 1]], dtype=F32)
    return pal


def numpy_skin(v, joints, weights, pal):
    """the same deform on the host, vectorised (float32; the work a user does today before swr_mesh_create)"""
    out = v.copy()
    p = np.concatenate([v["position"], np.ones((v.shape[0], 1), F32)], axis=1)
    m = pal[joints.astype(np.int64)]                                        # (n, 4, 4, 4)
    pk = np.einsum("ni,nkij->nkj", p, m)[..., :3]
    nk = np.einsum("ni,nkij->nkj", v["normal"], m[:, :, :3, :3])
    rp, rn = (weights[..., None] * pk).sum(axis=1), (weights[..., None] * nk).sum(axis=1)
    out["position"] = rp
    out["normal"] = rn / np.linalg.norm(rn, axis=1, keepdims=True)
    return out


def kernel_group(hip, dev, meshes_v, rounds, launches, warmup, label, sets=1):
    """per-call time of blend and skin on every vertex array of meshes_v; `sets` distinct sets of device arrays are used in turn"""
    out = []
    stream = dev._rate_stream
    for n_label, v in meshes_v:
        n = v.shape[0]
        idx = np.array([0, 1, 2], dtype=np.uint16)
        other, attrs, pal = synthetic_vertices(n, 9), skin_attributes(v, 3), palette(1)
        groups = []
        for _ in range(sets):
            a, b = Mesh(dev, v, idx), Mesh(dev, other, idx)
            a.SetSkin(*attrs)
            groups.append((a, b, a.Like()))
        turn = {"blend": 0, "skin": 0}

        def blend():
            a, b, dst = groups[turn["blend"] % sets]
            turn["blend"] += 1
            dst.BlendFrom(a, b, 0.37)

        def skin():
            a, _, dst = groups[turn["skin"] % sets]
            turn["skin"] += 1
            dst.SkinFrom(a, pal)
        variants = {"swr_mesh_blend": blend, "swr_mesh_skin": skin}
        runs = {name: [] for name in variants}
        for r in range(rounds + 1):                                     # round 0 is the warm-up of every variant
            for name, fn in variants.items():
                ms = hip.timed(stream, fn, launches, warmup)
                if r:
                    runs[name].append(ms)
        dev.sync()
        for name, ms in runs.items():
            out.append({"group": label, "case": name, "mesh": n_label, "vertices": n, "sets": sets, "us_per_call": stats_us(ms)})
        for g in groups:
            for m in g:
                m.Dispose()
    return out


def kernel_trace(group, path):
    """the k_mesh_* rows of a rocprofv3 kernel-stats csv; large / hbm: one vertex count, so the algorithm's bytes over the average time"""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            kind = "blend" if "k_mesh_blend" in r["Name"] else "skin" if "k_mesh_skin" in r["Name"] else None
            if kind is None:
                continue
            rec = {"group": group, "kernel": "k_mesh_" + kind, "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 3),
                   "min_us": round(float(r["MinNs"]) / 1e3, 3), "max_us": round(float(r["MaxNs"]) / 1e3, 3), "std_us": round(float(r["StdDev"]) / 1e3, 3)}
            if group in ("large", "hbm"):
                by = (BLEND_BYTES if kind == "blend" else SKIN_BYTES) * 65535
                gbs = by / (float(r["AverageNs"]) * 1e-9) / 1e9
                rec.update({"algorithmic_bytes": by, "kernel_gb_per_s": round(gbs, 1), "kernel_share_of_copy_peak": round(gbs / COPY_PEAK_GBS, 4)})
            rows.append(rec)
    return rows


def frame_loops(dev, model, rounds, frames):
    """(c): sixteen players, two meshes each, skinned every frame; Present8Async, the wait one frame behind"""
    w, h = 1920, 1080
    win = MainWindow(dev, w, h)
    scene = scenes.from_model(model, w, h, tex_size=64)
    view, proj = scene.draws[0].view, scene.draws[0].projection
    texs = [Texture(dev, t) for t in scene.textures]
    progs = [ShaderProgram(d.program, d.uniforms, texs[d.texture]) for d in scene.draws]
    base = [np.ascontiguousarray(d.vertices) for d in scene.draws]
    idx = [d.indices for d in scene.draws]
    attrs = [skin_attributes(v, 11 + i) for i, v in enumerate(base)]
    span = float(np.ptp(np.concatenate([v["position"] for v in base])[:, 0])) * 0.5
    models = [hm.multiply(hm.create_scale(0.5 * 0.3), hm.create_translation((px - 1.5) * span * 0.45, (py - 1.5) * span * 0.45, 0.0))
              for py in range(4) for px in range(4)]
    out = [np.zeros((h, w, 3), np.uint8) for _ in range(2)]
    for o in out:
        dev.pin(o)
    src = [Mesh(dev, v, i).SetSkin(*a) for v, i, a in zip(base, idx, attrs)]
    # two targets per player and mesh, alternating by frame: the deform of frame f never meets the batch of frame f - 1 in flight
    targets = [[[s.Like() for s in src] for _ in models] for _ in range(2)]

    def draw(mesh, k, pl):
        d = scene.draws[k]
        Rasterizer.RenderMesh(win, mesh, None, models[pl], view, proj, progs[k].VertexShader, progs[k].FragmentShader, d.cull, d.depth_test, d.blend)

    state = {"f": 0, "pending": [], "old": []}

    def begin():
        win.ClearDepthBuffer(); win.ClearColorBuffer((0.1, 0.1, 0.1, 1.0))

    def end():
        f = state["f"]
        state["pending"].append(win.Present8Async(out[f % 2]))
        while len(state["pending"]) > 1:
            win.PresentWait(state["pending"].pop(0))
        state["f"] = f + 1

    def gpu_frame():
        f = state["f"]
        begin()
        for pl in range(len(models)):
            pal = palette(f, pl)
            for k in range(len(src)):
                draw(targets[f % 2][pl][k].SkinFrom(src[k], pal), k, pl)
        end()

    def host_frame():
        f = state["f"]
        begin()
        fresh = []
        for pl in range(len(models)):
            pal = palette(f, pl)
            for k in range(len(src)):
                m = Mesh(dev, numpy_skin(base[k], attrs[k][0], attrs[k][1], pal), idx[k])
                fresh.append(m)
                draw(m, k, pl)
        end()
        for m in state["old"]:                       # last frame's meshes: swr_mesh_destroy (flushes and waits)
            m.Dispose()
        state["old"] = fresh

    def host_deform_only():
        f = state["f"]
        for pl in range(len(models)):
            pal = palette(f, pl)
            for k in range(len(src)):
                numpy_skin(base[k], attrs[k][0], attrs[k][1], pal)
        state["f"] = f + 1

    def run(fn, n):
        for _ in range(5):
            fn()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        for t in state["pending"]:
            win.PresentWait(t)
        state["pending"] = []
        return (time.perf_counter() - t0) / n * 1e3

    variants = {"swr_mesh_skin into retained targets": gpu_frame, "numpy skin + swr_mesh_create per frame": host_frame,
                "(numpy skin alone, no GPU call)": host_deform_only}
    runs = {name: [] for name in variants}
    syncs = {}
    for r in range(rounds + 1):
        for name, fn in variants.items():
            s0 = dev.sync_count()
            ms = run(fn, frames)
            syncs[name] = (dev.sync_count() - s0) / (frames + 5)
            if r:
                runs[name].append(ms)
    dev.sync()
    st = dev.stats()
    res = [{"group": "frames", "case": name, "frame": [w, h], "players": len(models), "meshes_per_player": len(src),
            "ms_per_frame": {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "runs": [round(x, 4) for x in ms]},
            "host_syncs_per_frame": round(syncs[name], 3)} for name, ms in runs.items()]
    res.append({"group": "frames", "case": "sanity", "fragments_written_total": int(st["fragments_written"]), "triangles_in_total": int(st["triangles_in"])})
    for m in state["old"] + src + [t for two in targets for pl in two for t in pl]:
        m.Dispose()
    for o in out:
        dev.unpin(o)
    for t in texs:
        t.Dispose()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_mesh_deform.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--sets", type=int, default=40, help="distinct mesh sets of the hbm group")
    ap.add_argument("--only", choices=["large", "hbm", "small", "frames"], default=None)
    ap.add_argument("--trace", action="append", default=[], metavar="GROUP=CSV", help="a kernel-stats csv of a traced --only GROUP run")
    a = ap.parse_args()
    model = Model().LoadModel(os.path.join(ROOT, "tests", "golden", "models", "gordon_freeman", "scene.gltf"))
    hip = Hip()
    dev = Device(0)
    res = {"device": dev.name, "build": dev.build_info(), "rounds": a.rounds, "launches": a.launches, "frames": a.frames,
           "copy_peak_gb_per_s": COPY_PEAK_GBS, "bytes_per_vertex": {"blend": BLEND_BYTES, "skin": SKIN_BYTES}, "records": [], "kernel_trace": []}
    dev.set_pipelining(0)                         # the deform runs where mesh uploads run: with pipelining off, on the context's stream
    dev._rate_stream = hip.stream()
    dev.set_stream(dev._rate_stream.value)
    big = [("65,535 vertices", synthetic_vertices(65535, 1))]
    if a.only in (None, "large"):
        res["records"] += kernel_group(hip, dev, big, a.rounds, a.launches, a.warmup, "large")
    if a.only in (None, "hbm"):
        res["records"] += kernel_group(hip, dev, big, a.rounds, a.launches, a.warmup, "hbm", sets=a.sets)
    if a.only in (None, "small"):
        small = [(f"gordon_freeman mesh {i}", np.ascontiguousarray(m.Vertices)) for i, m in enumerate(model.Meshes)]
        recs = kernel_group(hip, dev, small, a.rounds, a.launches, a.warmup, "small")
        res["records"] += recs
        per_player = {c: sum(r["us_per_call"]["median"] for r in recs if r["case"] == c) for c in ("swr_mesh_blend", "swr_mesh_skin")}
        res["sixteen_players"] = {c: {"us_per_frame": round(16 * us, 2), "share_of_front_end": round(16 * us / (FRONT_END_MS * 1e3), 3)} for c, us in per_player.items()}
    dev.set_stream(0)
    dev.set_pipelining(1)
    if a.only in (None, "frames"):
        res["records"] += frame_loops(dev, model, a.rounds, a.frames)
    dev.close()
    for t in a.trace:
        group, path = t.split("=", 1)
        res["kernel_trace"] += kernel_trace(group, path)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    for r in res["records"]:
        print(r["group"], "|", r["case"], "|", r.get("mesh", ""), "|", r.get("us_per_call", r.get("ms_per_frame", {})).get("median", ""),
              "us/call" if "us_per_call" in r else "ms/frame", "| syncs/frame", r.get("host_syncs_per_frame", ""))
    for r in res["kernel_trace"]:
        print("trace", r["group"], "|", r["kernel"], "|", r["avg_us"], "us avg", r["min_us"], "min |", r.get("kernel_gb_per_s", ""), "GB/s", r.get("kernel_share_of_copy_peak", ""))
    if "sixteen_players" in res:
        print("sixteen players x 2 meshes:", res["sixteen_players"])


if __name__ == "__main__":
    main()
