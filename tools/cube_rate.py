#!/usr/bin/env python3
"""Cost of cube maps, one JSON file (default profiles/r22_cubemaps.json).  Needs a GPU.  One process on one
MI355X, every variant warmed, the variants of a group alternated over --rounds rounds, medians.
  (a) one face update of a 512^2 cube from a frame at (1, 1) and at (2, 2), beside swr_texture_update_from_frame into a 512^2 texture:
      the same kernel, launched with a face's offset;
  (b) six face updates of a cube that has its chain (each regenerates it), beside six without a chain;
  (c) a 1920 x 1080 frame of one curved mirror: REFLECT of tests/cubemap_cases.py samples a 512^2 cube by the reflected view vector,
      under the nearest filter and under the bilinear one, beside the same frame through a program that samples one 512^2 texture by
      uv (swr_sample) -- whose raster kernel is, instruction for instruction, the parent commit's (profiles/r22_cubemaps.md); with
      --parent-tree DIR (a built checkout of the parent commit) that program is also timed under the parent's package and library,
      in a child process.
usage: python tools/cube_rate.py [--out FILE] [--rounds N] [--launches N] [--parent-tree DIR]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE_ROOT = os.environ.get("SWR_CUBE_RATE_TREE") or ROOT              # (the child of --parent-tree imports the parent's package)
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, PACKAGE_ROOT)

from softwarerenderer_amd import BlendMode, CullMode, DepthTest, Device, MainWindow, Rasterizer, Texture, hostmath as hm, scenes   # noqa: E402
from softwarerenderer_amd.rasterizer import ShaderProgram                                            # noqa: E402
from tools.resolve_rate import Hip                                                                  # noqa: E402

HEAD = "__device__ float4 swr_fragment(const swr_fs_in& in, const swr_fs_env& env) {\n"
SINGLE = HEAD + "    const float4 t = swr_sample(env, 0, in.tex_coord);\n    return make_float4(t.x, t.y, t.z, 1.0f);\n}\n"


def stats_us(ms):
    v = [x * 1e3 for x in ms]
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "runs": [round(x, 3) for x in v]}


def alternate(hip, stream, variants, rounds, launches, warmup):
    runs = {name: [] for name in variants}
    for r in range(rounds + 1):                                         # round 0 is the warm-up of every variant
        for name, fn in variants.items():
            ms = hip.timed(stream, fn, launches, warmup)
            if r:
                runs[name].append(ms)
    return runs


def updates(hip, dev, rounds, launches, warmup):
    stream = hip.stream()
    dev.set_stream(stream.value)
    out, n = [], 512
    for k in (1, 2):
        win = MainWindow(dev, n * k, n * k)
        win.Upload(color=np.random.default_rng(k).random((n * k, n * k, 4), dtype=np.float32))
        cube, chained, flat = Texture.CubeTarget(dev, n), Texture.CubeTarget(dev, n), Texture.Target(dev, n, n)
        chained.GenerateMipmaps()

        def six(t):
            for f in range(6):
                t.UpdateFaceFrom(f, win, k, k)
        variants = {"swr_texture_update_from_frame, 512^2 texture": lambda: flat.UpdateFrom(win, k, k),
                    "swr_texture_update_face_from_frame, one face": lambda: cube.UpdateFaceFrom(3, win, k, k),
                    "six face updates, no chain": lambda: six(cube),
                    "six face updates, each regenerating the chain": lambda: six(chained)}
        runs = alternate(hip, stream, variants, rounds, launches, warmup)
        dev.sync()
        out += [{"case": name, "factors": [k, k], "cube": n, "us": stats_us(ms)} for name, ms in runs.items()]
        for t in (cube, chained, flat):
            t.Dispose()
    dev.set_stream(0)
    return out


def mirror_mesh(cells=48):
    """a bulging sheet in front of the camera: positions, normals that fan out, uv over the sheet"""
    g = np.linspace(-1.0, 1.0, cells + 1)
    x, y = np.meshgrid(g, g)
    z = -2.0 - 0.4 * (x * x + y * y)
    pos = np.stack([1.9 * x, 1.1 * y, z], axis=-1).reshape(-1, 3)
    nrm = np.stack([0.8 * x, 0.8 * y, np.ones_like(x)], axis=-1).reshape(-1, 3)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    uv = np.stack([(x + 1) / 2, (y + 1) / 2], axis=-1).reshape(-1, 2)
    idx = []
    for j in range(cells):
        for i in range(cells):
            a = j * (cells + 1) + i
            idx += [a, a + 1, a + cells + 2, a, a + cells + 2, a + cells + 1]
    v = scenes.make_vertices([tuple(p) for p in pos], uv=[tuple(t) for t in uv], normal=[tuple(t) for t in nrm])
    return v, np.array(idx, dtype=np.uint16)


def frames(hip, dev, rounds, launches, warmup, which=("reflect", "single")):
    stream = hip.stream()
    dev.set_stream(stream.value)
    was = dev.pipelining()
    dev.set_pipelining(0)
    w, h, n = 1920, 1080, 512
    win = MainWindow(dev, w, h)
    v, idx = mirror_mesh()
    I, proj = hm.identity(), hm.create_perspective_fov(np.pi / 3, w / h, 0.1, 100.0)
    rng = np.random.default_rng(5)
    variants, made, pids = {}, [], []

    def frame(pid, tex):
        def go():
            prog = ShaderProgram(pid, None, tex)
            win.ClearDepthBuffer(); win.ClearColorBuffer((0.1, 0.2, 0.3, 1.0))
            Rasterizer.RenderMesh(win, v, idx, I, I, proj, prog.VertexShader, prog.FragmentShader, CullMode.None_, DepthTest.LessEqual, BlendMode.None_)
            dev.flush()
        return go
    for filt in (False, True):
        name = "bilinear" if filt else "nearest"
        if "reflect" in which:
            import cubemap_cases as K
            cube = Texture.Cube(dev, rng.integers(0, 256, (6, n, n, 4), dtype=np.uint8))
            cube.SetBilinear(filt)
            pid = dev.compile_program(K.REFLECT_FRAGMENT, vertex_source=K.REFLECT_VERTEX)
            dev.set_program_constants(pid, np.zeros(64, dtype=np.float32))
            dev.set_program_texture(pid, 1, cube)
            variants[f"REFLECT (swr_sample_cube), {name}"] = frame(pid, None)
            made.append(cube); pids.append(pid)
        if "single" in which:
            flat = Texture(dev, rng.integers(0, 256, (n, n, 4), dtype=np.uint8))
            flat.SetBilinear(filt)
            pid = dev.compile_program(SINGLE)
            variants[f"SINGLE (swr_sample), {name}"] = frame(pid, flat)
            made.append(flat); pids.append(pid)
    runs = alternate(hip, stream, variants, rounds, launches, warmup)
    dev.sync()
    out = [{"case": name, "frame": [w, h], "texture": n, "us": stats_us(ms)} for name, ms in runs.items()]
    for t in made:
        t.Dispose()
    for pid in pids:
        dev.destroy_program(pid)
    dev.set_pipelining(was)
    dev.set_stream(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_cubemaps.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: SINGLE is timed under its package and library in a child process")
    ap.add_argument("--single-only", action="store_true", help="(the child's mode) time SINGLE alone and print the records as JSON")
    a = ap.parse_args()
    if a.single_only:
        hip, dev = Hip(), Device(0)
        print("RECORDS " + json.dumps({"build": dev.build_info(), "frames": frames(hip, dev, a.rounds, a.launches, a.warmup, which=("single",))}))
        dev.close()
        return
    parent = None
    if a.parent_tree:                                                    # first, while this process has not opened the GPU
        env = dict(os.environ, SWR_CUBE_RATE_TREE=os.path.abspath(a.parent_tree))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--single-only", "--rounds", str(a.rounds), "--launches", str(a.launches),
                            "--warmup", str(a.warmup)], env=env, capture_output=True, text=True, timeout=300)
        line = [l for l in r.stdout.splitlines() if l.startswith("RECORDS ")]
        parent = json.loads(line[0][8:]) if r.returncode == 0 and line else {"error": (r.stdout + r.stderr)[-2000:]}
    hip, dev = Hip(), Device(0)
    res = {"device": dev.name, "build": dev.build_info(), "rounds": a.rounds, "launches": a.launches,
           "face_updates": updates(hip, dev, a.rounds, a.launches, a.warmup), "mirror_frame": frames(hip, dev, a.rounds, a.launches, a.warmup),
           "mirror_frame_parent_library": parent}
    dev.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    for group in ("face_updates", "mirror_frame"):
        for rec in res[group]:
            print(group, rec["case"], rec.get("factors", ""), rec["us"]["median"], "us")
    if parent and "frames" in parent:
        for rec in parent["frames"]:
            print("parent library", rec["case"], rec["us"]["median"], "us")


if __name__ == "__main__":
    main()
