#!/usr/bin/env python3
"""Cost of skeletal animation on the GPU, one JSON file (default profiles/r24_animation.json).  Needs a GPU.
One process on one MI355X, every variant warmed, the variants of a group alternated over --rounds rounds, medians.  The yardstick is
the parent commit's path measured BESIDE the new one in the same process: poses made in numpy on the host and one swr_mesh_skin per
mesh, against one swr_pose_set_sample and one swr_mesh_skin_batch.
  (a) crowd: sixteen players of the two meshes of tests/golden/models/gordon_freeman (118 and 477 vertices) on a 64-joint skeleton.
      STREAM time per frame (device events around --launches frames issued back to back, the old way's palettes made beforehand so
      that the stream, not numpy, is what is timed) and HOST time per frame (wall clock of issuing one frame's calls, the old way's
      numpy poses included), both ways;
  (b) large: one job of 65,535 vertices through swr_mesh_skin_batch beside swr_mesh_skin, per call; swr_pose_set_sample at 16 x 64
      and 256 x 64 joints, per call;
  (c) frames: the r23 end-to-end loop both ways -- sixteen skinned players at 1920 x 1080, 8-bit asynchronous present, the wait one
      frame behind -- per frame on the host clock, with the host syncs per frame.
KERNEL times come from a kernel trace, a run of its own per group (a kernel name is one row of the trace's statistics, so the two
sizes of each kernel are traced apart):
    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/animation_rate.py --only crowd --out FILE
    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/animation_rate.py --only large --out FILE
(--only crowd launches k_pose_sample at 16 x 64 and k_mesh_skin_batch at 32 jobs only; --only large launches them at 256 x 64 and at
one job of 65,535 vertices, and k_mesh_skin.)  --trace GROUP=DIR/run_kernel_stats.csv (repeatable) folds them into the JSON.
usage: python tools/animation_rate.py [--out FILE] [--rounds N] [--launches N] [--frames N] [--only GROUP] [--trace GROUP=CSV ...]"""
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

from softwarerenderer_amd import Device, MainWindow, Mesh, PoseSet, Rasterizer, Skeleton, Texture, hostmath as hm, scenes   # noqa: E402
from softwarerenderer_amd.modelloader import Model, compose_trs                                                          # noqa: E402
from softwarerenderer_amd.rasterizer import ShaderProgram                                                                # noqa: E402
from tools.mesh_deform_rate import skin_attributes, stats_us, synthetic_vertices                                         # noqa: E402
from tools.resolve_rate import Hip                                                                                       # noqa: E402

F32 = np.float32
N_JOINTS, N_KEYS, PLAYERS = 64, 32, 16


class Rig:
    """A 64-joint tree (every node a joint) with one clip of LINEAR channels on every (node, path), and its evaluation in numpy --
    what a caller of the parent commit does on the host every frame."""

    def __init__(self, seed=1):
        rng = np.random.default_rng(seed)
        n = N_JOINTS
        self.parent = np.array([-1] + [int(rng.integers(max(0, i - 6), i)) for i in range(1, n)], dtype=np.int32)
        self.rest_t = rng.uniform(-0.05, 0.05, (n, 3)).astype(F32)
        self.rest_r = np.tile(np.array([0, 0, 0, 1], dtype=F32), (n, 1))
        self.rest_s = np.ones((n, 3), dtype=F32)
        self.rest_local = np.stack([compose_trs(self.rest_t[i], self.rest_r[i], self.rest_s[i]) for i in range(n)])
        self.joint_node = np.arange(n, dtype=np.int32)
        self.inverse_bind = np.tile(np.eye(4, dtype=F32), (n, 1, 1))
        self.times = np.linspace(0.0, 2.0, N_KEYS).astype(F32)
        ang = rng.uniform(-0.1, 0.1, (n, N_KEYS))
        self.key_r = np.zeros((n, N_KEYS, 4), dtype=F32)
        self.key_r[..., 1], self.key_r[..., 3] = np.sin(ang), np.cos(ang)
        self.key_t = (self.rest_t[:, None, :] + rng.uniform(-0.01, 0.01, (n, N_KEYS, 3))).astype(F32)
        self.key_s = np.ones((n, N_KEYS, 3), dtype=F32)
        depth = np.zeros(n, dtype=np.int64)
        for i in range(1, n):
            depth[i] = depth[self.parent[i]] + 1
        self.levels = [np.nonzero(depth == d)[0] for d in range(1, int(depth.max()) + 1)]

    def upload(self, dev):
        g = Skeleton(dev, self.parent, self.rest_local, self.rest_t, self.rest_r, self.rest_s, self.joint_node, self.inverse_bind)
        chans = []
        for i in range(N_JOINTS):
            chans += [(i, "translation", "LINEAR", self.times, self.key_t[i]), (i, "rotation", "LINEAR", self.times, self.key_r[i]),
                      (i, "scale", "LINEAR", self.times, self.key_s[i])]
        g.AddClip(chans)
        return g

    def palette(self, t):
        """numpy, vectorised over the nodes and float32: key search, lerp / normalised lerp, compose, the hierarchy level by level"""
        k = int(np.clip(np.searchsorted(self.times, t, side="right") - 1, 0, N_KEYS - 2))
        u = F32(np.clip((t - self.times[k]) / (self.times[k + 1] - self.times[k]), 0.0, 1.0))
        tr = self.key_t[:, k] * (1 - u) + self.key_t[:, k + 1] * u
        sc = self.key_s[:, k] * (1 - u) + self.key_s[:, k + 1] * u
        q = self.key_r[:, k] * (1 - u) + self.key_r[:, k + 1] * u
        q = q / np.linalg.norm(q, axis=1, keepdims=True)
        x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        m = np.zeros((N_JOINTS, 4, 4), dtype=F32)
        m[:, 0, 0], m[:, 0, 1], m[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z - w * y)
        m[:, 1, 0], m[:, 1, 1], m[:, 1, 2] = 2 * (x * y - w * z), 1 - 2 * (z * z + x * x), 2 * (y * z + w * x)
        m[:, 2, 0], m[:, 2, 1], m[:, 2, 2] = 2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (y * y + x * x)
        m[:, :3, :3] *= sc[:, :, None]
        m[:, 3, :3], m[:, 3, 3] = tr, 1.0
        for nodes in self.levels:
            m[nodes] = np.matmul(m[nodes], m[self.parent[nodes]])
        return np.matmul(self.inverse_bind, m[self.joint_node])


def player_time(frame, player):
    return F32((0.031 * frame + 0.11 * player) % 2.0)


def crowd_group(hip, dev, model, rig, rounds, launches, warmup, only_new=False):
    """(a): stream and host time per frame of posing and skinning sixteen players of two meshes, the old way and the new"""
    stream = dev._rate_stream
    base = [np.ascontiguousarray(m.Vertices) for m in model.Meshes]
    src = [Mesh(dev, v, np.ascontiguousarray(m.Indices)).SetSkin(*skin_attributes(v, 11 + i)) for i, (v, m) in enumerate(zip(base, model.Meshes))]
    dsts = [[s.Like() for s in src] for _ in range(PLAYERS)]
    g, ps = rig.upload(dev), PoseSet(dev, PLAYERS, N_JOINTS)
    flat_dst = [d for pl in dsts for d in pl]
    flat_src = [s for _ in dsts for s in src]
    inst = [pl for pl in range(PLAYERS) for _ in src]
    pals = [[rig.palette(player_time(f, pl)) for pl in range(PLAYERS)] for f in range(8)]
    state = {"f": 0}

    def old_stream():                                  # the palettes were made beforehand: 32 copies, 32 launches
        f = state["f"] = state["f"] + 1
        for pl in range(PLAYERS):
            for k, s in enumerate(src):
                dsts[pl][k].SkinFrom(s, pals[f % 8][pl])

    def old_host():                                    # ... and with the poses made in numpy, as a frame has to
        f = state["f"] = state["f"] + 1
        for pl in range(PLAYERS):
            pal = rig.palette(player_time(f, pl))
            for k, s in enumerate(src):
                dsts[pl][k].SkinFrom(s, pal)

    def new():                                         # at most two small copies, two launches
        f = state["f"] = state["f"] + 1
        ps.Sample(g, PoseSet.Requests([0] * PLAYERS, [player_time(f, pl) for pl in range(PLAYERS)]))
        dev.SkinBatch(flat_dst, flat_src, ps, inst)

    variants = {"one Sample + one SkinBatch": new} if only_new else \
        {"32 x swr_mesh_skin, palettes made beforehand": old_stream, "one Sample + one SkinBatch": new}
    runs = {name: [] for name in variants}
    for r in range(rounds + 1):                        # round 0 is the warm-up of every variant
        for name, fn in variants.items():
            ms = hip.timed(stream, fn, launches, warmup)
            if r:
                runs[name].append(ms)
    dev.sync()
    out = [{"group": "crowd", "case": name, "players": PLAYERS, "meshes_per_player": len(src), "joints": N_JOINTS,
            "stream_us_per_frame": stats_us(ms)} for name, ms in runs.items()]
    if not only_new:
        host = {"numpy poses + 32 x swr_mesh_skin": old_host, "one Sample + one SkinBatch": new}
        hruns = {name: [] for name in host}
        for r in range(rounds + 1):
            for name, fn in host.items():
                dev.sync()
                t0 = time.perf_counter()
                for _ in range(launches):
                    fn()
                ms = (time.perf_counter() - t0) / launches * 1e3
                dev.sync()
                if r:
                    hruns[name].append(ms)
        out += [{"group": "crowd", "case": name, "players": PLAYERS, "meshes_per_player": len(src), "joints": N_JOINTS,
                 "host_us_per_frame": stats_us(ms)} for name, ms in hruns.items()]
    for m in flat_dst + src:
        m.Dispose()
    ps.Dispose(); g.Dispose()
    return out


def large_group(hip, dev, rig, rounds, launches, warmup, only_large=False):
    """(b): one 65,535-vertex job batched beside swr_mesh_skin; the sampler at 16 and 256 instances (--only large: 256 alone)"""
    stream = dev._rate_stream
    v = synthetic_vertices(65535, 1)
    src = Mesh(dev, v, np.array([0, 1, 2], dtype=np.uint16)).SetSkin(*skin_attributes(v, 3))
    dst = src.Like()
    g = rig.upload(dev)
    sets = {n: PoseSet(dev, n, N_JOINTS) for n in ((256,) if only_large else (16, 256))}
    reqs = {n: PoseSet.Requests([0] * n, [player_time(3, pl) for pl in range(n)]) for n in sets}
    for n, ps in sets.items():
        ps.Sample(g, reqs[n])
    pal = sets[256].Read()[0]
    variants = {"swr_mesh_skin, 65,535 vertices": lambda: dst.SkinFrom(src, pal),
                "swr_mesh_skin_batch, one job of 65,535 vertices": lambda: dev.SkinBatch([dst], [src], sets[256], [0]),
                "swr_pose_set_sample, 256 x 64 joints": lambda: sets[256].Sample(g, reqs[256])}
    if not only_large:
        variants["swr_pose_set_sample, 16 x 64 joints"] = lambda: sets[16].Sample(g, reqs[16])
    runs = {name: [] for name in variants}
    for r in range(rounds + 1):
        for name, fn in variants.items():
            ms = hip.timed(stream, fn, launches, warmup)
            if r:
                runs[name].append(ms)
    dev.sync()
    for m in (dst, src):
        m.Dispose()
    for ps in sets.values():
        ps.Dispose()
    g.Dispose()
    return [{"group": "large", "case": name, "us_per_call": stats_us(ms)} for name, ms in runs.items()]


def kernel_trace(group, path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            n = r["Name"]
            name = "k_pose_sample" if "k_pose_sample" in n else "k_mesh_skin_batch" if "k_mesh_skin_batch" in n else "k_mesh_skin" if "k_mesh_skin" in n else None
            if name is None:
                continue
            rows.append({"group": group, "kernel": name, "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 3),
                         "min_us": round(float(r["MinNs"]) / 1e3, 3), "max_us": round(float(r["MaxNs"]) / 1e3, 3), "std_us": round(float(r["StdDev"]) / 1e3, 3)})
    return rows


def frame_loops(dev, model, rig, rounds, frames):
    """(c): sixteen players, two meshes each, posed and skinned every frame; Present8Async, the wait one frame behind"""
    w, h = 1920, 1080
    win = MainWindow(dev, w, h)
    scene = scenes.from_model(model, w, h, tex_size=64)
    view, proj = scene.draws[0].view, scene.draws[0].projection
    texs = [Texture(dev, t) for t in scene.textures]
    progs = [ShaderProgram(d.program, d.uniforms, texs[d.texture]) for d in scene.draws]
    base = [np.ascontiguousarray(d.vertices) for d in scene.draws]
    idx = [d.indices for d in scene.draws]
    span = float(np.ptp(np.concatenate([v["position"] for v in base])[:, 0])) * 0.5
    models = [hm.multiply(hm.create_scale(0.5 * 0.3), hm.create_translation((px - 1.5) * span * 0.45, (py - 1.5) * span * 0.45, 0.0))
              for py in range(4) for px in range(4)]
    out = [np.zeros((h, w, 3), np.uint8) for _ in range(2)]
    for o in out:
        dev.pin(o)
    src = [Mesh(dev, v, i).SetSkin(*skin_attributes(v, 11 + k)) for k, (v, i) in enumerate(zip(base, idx))]
    # two targets per player and mesh, alternating by frame: the deform of frame f never meets the batch of frame f - 1 in flight
    targets = [[[s.Like() for s in src] for _ in models] for _ in range(2)]
    flat = [[t for pl in two for t in pl] for two in targets]
    flat_src = [s for _ in models for s in src]
    inst = [pl for pl in range(len(models)) for _ in src]
    g, ps = rig.upload(dev), [PoseSet(dev, len(models), N_JOINTS) for _ in range(2)]
    state = {"f": 0, "pending": []}

    def draw_all(two):
        for pl in range(len(models)):
            for k in range(len(src)):
                d = scene.draws[k]
                Rasterizer.RenderMesh(win, two[pl][k], None, models[pl], view, proj, progs[k].VertexShader, progs[k].FragmentShader, d.cull, d.depth_test, d.blend)

    def end():
        f = state["f"]
        state["pending"].append(win.Present8Async(out[f % 2]))
        while len(state["pending"]) > 1:
            win.PresentWait(state["pending"].pop(0))
        state["f"] = f + 1

    def old_frame():
        f = state["f"]
        win.ClearDepthBuffer(); win.ClearColorBuffer((0.1, 0.1, 0.1, 1.0))
        for pl in range(len(models)):
            pal = rig.palette(player_time(f, pl))
            for k in range(len(src)):
                targets[f % 2][pl][k].SkinFrom(src[k], pal)
        draw_all(targets[f % 2])
        end()

    def new_frame():
        f = state["f"]
        win.ClearDepthBuffer(); win.ClearColorBuffer((0.1, 0.1, 0.1, 1.0))
        ps[f % 2].Sample(g, PoseSet.Requests([0] * len(models), [player_time(f, pl) for pl in range(len(models))]))
        dev.SkinBatch(flat[f % 2], flat_src, ps[f % 2], inst)
        draw_all(targets[f % 2])
        end()

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

    variants = {"numpy poses + 32 x swr_mesh_skin (the parent's way)": old_frame, "one Sample + one SkinBatch": new_frame}
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
    for m in src + [t for two in flat for t in two]:
        m.Dispose()
    for p in ps:
        p.Dispose()
    g.Dispose()
    for o in out:
        dev.unpin(o)
    for t in texs:
        t.Dispose()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_animation.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--only", choices=["crowd", "large", "frames"], default=None)
    ap.add_argument("--trace", action="append", default=[], metavar="GROUP=CSV", help="a kernel-stats csv of a traced --only GROUP run")
    a = ap.parse_args()
    model = Model().LoadModel(os.path.join(ROOT, "tests", "golden", "models", "gordon_freeman", "scene.gltf"))
    rig = Rig()
    hip = Hip()
    dev = Device(0)
    res = {"device": dev.name, "build": dev.build_info(), "rounds": a.rounds, "launches": a.launches, "frames": a.frames, "records": [], "kernel_trace": []}
    dev.set_pipelining(0)                         # the deform calls run where mesh uploads run: with pipelining off, on the context's stream
    dev._rate_stream = hip.stream()
    dev.set_stream(dev._rate_stream.value)
    if a.only in (None, "crowd"):
        res["records"] += crowd_group(hip, dev, model, rig, a.rounds, a.launches, a.warmup, only_new=a.only == "crowd")
    if a.only in (None, "large"):
        res["records"] += large_group(hip, dev, rig, a.rounds, a.launches, a.warmup, only_large=a.only == "large")
    dev.set_stream(0)
    dev.set_pipelining(1)
    if a.only in (None, "frames"):
        res["records"] += frame_loops(dev, model, rig, a.rounds, a.frames)
    dev.close()
    for t in a.trace:
        group, path = t.split("=", 1)
        res["kernel_trace"] += kernel_trace(group, path)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    for r in res["records"]:
        fig = r.get("stream_us_per_frame") or r.get("host_us_per_frame") or r.get("us_per_call") or r.get("ms_per_frame") or {}
        unit = "us/frame (stream)" if "stream_us_per_frame" in r else "us/frame (host)" if "host_us_per_frame" in r else "us/call" if "us_per_call" in r else "ms/frame"
        print(r["group"], "|", r["case"], "|", fig.get("median", ""), unit, "| syncs/frame", r.get("host_syncs_per_frame", ""))
    for r in res["kernel_trace"]:
        print("trace", r["group"], "|", r["kernel"], "|", r["calls"], "calls |", r["avg_us"], "us avg", r["min_us"], "min", r["std_us"], "std")


if __name__ == "__main__":
    main()
