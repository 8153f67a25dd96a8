#!/usr/bin/env python3
"""Cost of mip chains, one JSON file (default profiles/r20_mipmaps.json).  Needs a GPU.  One process on one
MI355X, every variant warmed, the variants of a group alternated over --rounds rounds, medians.
  (a) swr_texture_generate_mipmaps of a 512^2, 1024^2 and 2048^2 texture -- the header is in place after the first call, so a call is
      the downsample launches alone --, device events around --launches back-to-back calls; beside it swr_texture_update_from_frame
      (1, 1) into the same texture without and with the chain: what an update pays for keeping the chain.
  (b) a ground plane that recedes to the horizon, 1920 x 1080, one 2048^2 texture repeating over it, pipelining off, device events
      around clear + draw + flush: the PLAIN program (swr_sample) against the RECIPE (swr_sample_grad), both of tests/mipmap_cases.py,
      under the nearest filter and under the bilinear one.
usage: python tools/mipmap_rate.py [--out FILE] [--rounds N] [--launches N]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

from softwarerenderer_amd import BlendMode, CullMode, DepthTest, Device, MainWindow, Rasterizer, Texture, hostmath as hm, scenes   # noqa: E402
from softwarerenderer_amd.rasterizer import ShaderProgram                                            # noqa: E402
from tools.resolve_rate import Hip                                                                  # noqa: E402
import mipmap_cases as M                                                                            # noqa: E402


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


def generate(hip, dev, rounds, launches, warmup):
    stream = hip.stream()
    dev.set_stream(stream.value)
    out = []
    for n in (512, 1024, 2048):
        win = MainWindow(dev, n, n)
        win.Upload(color=np.random.default_rng(n).random((n, n, 4), dtype=np.float32))
        chained, plain = Texture.Target(dev, n, n), Texture.Target(dev, n, n)
        chained.GenerateMipmaps()
        variants = {"swr_texture_generate_mipmaps": chained.GenerateMipmaps,
                    "swr_texture_update_from_frame, no chain": lambda: plain.UpdateFrom(win),
                    "swr_texture_update_from_frame, chain regenerated": lambda: chained.UpdateFrom(win)}
        runs = alternate(hip, stream, variants, rounds, launches, warmup)
        dev.sync()
        levels = M.full_levels(n, n)
        moved = n * n * 4 + 2 * sum((n >> l) ** 2 * 4 for l in range(1, levels))       # level 0 read; every other level written, most read
        for name, ms in runs.items():
            rec = {"case": name, "texture": [n, n], "levels": levels, "us": stats_us(ms)}
            if name == "swr_texture_generate_mipmaps":
                rec["bytes_moved"] = moved
                rec["GB_per_s"] = round(moved / (rec["us"]["median"] * 1e-6) / 1e9, 1)
            out.append(rec)
        chained.Dispose(); plain.Dispose()
    dev.set_stream(0)
    return out


def ground(hip, dev, rounds, launches, warmup):
    stream = hip.stream()
    dev.set_stream(stream.value)
    was = dev.pipelining()
    dev.set_pipelining(0)
    w, h, n = 1920, 1080, 2048
    win = MainWindow(dev, w, h)
    texels = np.random.default_rng(3).integers(0, 256, (n, n, 4), dtype=np.uint8)
    v = scenes.make_vertices([(-40.0, -1.0, -1.2), (40.0, -1.0, -1.2), (40.0, -1.0, -200.0), (-40.0, -1.0, -200.0)],
                             uv=[(-10.0, 0.3), (10.0, 0.3), (10.0, 50.0), (-10.0, 50.0)])
    idx = np.array([0, 1, 2, 0, 2, 3], dtype=np.uint16)
    I, proj = hm.identity(), hm.create_perspective_fov(np.pi / 3, w / h, 0.1, 1000.0)
    pids = {"PLAIN (swr_sample)": dev.compile_program(M.PLAIN), "RECIPE (swr_sample_grad)": dev.compile_program(M.RECIPE)}
    textures, variants = [], {}
    for filt in (False, True):
        tex = Texture(dev, texels)
        tex.SetBilinear(filt)
        tex.GenerateMipmaps()
        textures.append(tex)
        for name, pid in pids.items():
            def go(pid=pid, tex=tex):
                prog = ShaderProgram(pid, None, tex)
                win.ClearDepthBuffer(); win.ClearColorBuffer((0.1, 0.2, 0.3, 1.0))
                Rasterizer.RenderMesh(win, v, idx, I, I, proj, prog.VertexShader, prog.FragmentShader, CullMode.None_, DepthTest.LessEqual, BlendMode.None_)
                dev.flush()
            variants[f"{name}, {'bilinear' if filt else 'nearest'}"] = go
    runs = alternate(hip, stream, variants, rounds, launches, warmup)
    dev.sync()
    out = [{"case": name, "frame": [w, h], "texture": [n, n], "us": stats_us(ms)} for name, ms in runs.items()]
    for tex in textures:
        tex.Dispose()
    for pid in pids.values():
        dev.destroy_program(pid)
    dev.set_pipelining(was)
    dev.set_stream(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_mipmaps.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    hip, dev = Hip(), Device(0)
    res = {"device": dev.name, "build": dev.build_info() if hasattr(dev, "build_info") else None, "rounds": a.rounds, "launches": a.launches,
           "generate": generate(hip, dev, a.rounds, a.launches, a.warmup), "ground_plane": ground(hip, dev, a.rounds, a.launches, a.warmup)}
    dev.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    for group in ("generate", "ground_plane"):
        for rec in res[group]:
            print(group, rec["case"], rec.get("texture"), rec["us"]["median"], "us", rec.get("GB_per_s", ""))


if __name__ == "__main__":
    main()
