#!/usr/bin/env python3
"""Cost of depth textures, one JSON file (default profiles/r18_depth_texture.json).  Needs a GPU.  The method of
tools/render_to_texture_rate.py: one process, every variant warmed by a dropped round, the variants alternated over --rounds rounds (at
least 7), medians and max - min.
  (a) the kernel alone, device events around --launches back-to-back launches: k_depth_to_texture (MAX; MIN and FIRST beside it) beside
      k_frame_to_texture (opaque) at the same texture shape and factors -- a 1024^2 texture from a 1024^2 frame at (1, 1) and from a
      2048^2 frame at (2, 2) -- with and without the block-linear copy.  The planes stay in the Infinity Cache: comparisons, not HBM rates.
  (b) end to end, host wall clock ending in a synchronise: a light context renders a 2048^2 frame, its depth is resolved (2, 2) MAX
      into a 1024^2 depth texture with the 2 x 2 filter, a screen context renders a 1920x1080 cfg3-style frame under the shadow recipe
      (tests/depth_texture_cases.py) that looks every fragment up in it.  With swr_texture_update_from_depth, and with the
      host route in the same process: swr_readback's depth, the reduction in numpy, swr_texture_create_depth, swr_texture_set_filter,
      swr_texture_destroy of the previous one.
  (c) --bench-before / --bench-after FILE: the `bench.py --gpus 1 --steps 50 --warmup 5` lines of the parent's library and of this one.
usage: python tools/depth_texture_rate.py [--out FILE] [--rounds N] [--bench-before FILE] [--bench-after FILE]"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import depth_texture_cases as D                                                     # noqa: E402
from softwarerenderer_amd import DepthReduce, Device, Texture, scenes               # noqa: E402
from tools.render_to_texture_rate import SHAPES, TEX, bench_lines, camera_scene, summary      # noqa: E402
from tools.resolve_rate import Hip                                                  # noqa: E402


def kernel_alone(hip, dev, rounds, launches, warmup):
    out = []
    stream = hip.stream()
    dev.set_stream(stream.value)
    lib, ctx = dev._lib, dev._ctx
    for size, (kx, ky) in SHAPES:
        cam = scenes.SceneRenderer(dev, camera_scene(size))
        cam.render()                                                    # the planes the kernels read: cfg3-style content
        colour = {False: Texture.Target(dev, TEX, TEX), True: Texture.Target(dev, TEX, TEX)}
        depth = {False: Texture.Depth(dev, TEX, TEX), True: Texture.Depth(dev, TEX, TEX)}
        colour[True].SetBilinear(True); depth[True].SetBilinear(True)

        def call(fn, tex, mode):
            def go():
                rc = fn(ctx, tex._h, None, kx, ky, mode)
                if rc:
                    dev._ck(rc)
            return go
        variants, base_of = {}, {}
        for blocked in (False, True):
            b = "true" if blocked else "false"
            base = f"k_frame_to_texture<{kx}, {ky}, false, {b}>"
            variants[base] = call(lib.swr_texture_update_from_frame, colour[blocked], 0)
            for mode in (DepthReduce.Max, DepthReduce.Min, DepthReduce.First):
                name = f"k_depth_to_texture<{kx}, {ky}, {b}> {mode.name.upper()}"
                variants[name] = call(lib.swr_texture_update_from_depth, depth[blocked], int(mode))
                base_of[name] = base
        runs = {name: [] for name in variants}
        for r in range(rounds + 1):                                     # round 0 is the warm-up of every variant
            for name, fn in variants.items():
                ms = hip.timed(stream, fn, launches, warmup)
                if r:
                    runs[name].append(ms)
        dev.sync()
        us = {name: [x * 1e3 for x in ms] for name, ms in runs.items()}      # microseconds per launch, one figure per round
        for name, v in us.items():
            med = statistics.median(v)
            rec = {"kernel": name, "frame": list(size), "texture": [TEX, TEX],
                   "us": {"median": round(med, 3), "min": round(min(v), 3), "max": round(max(v), 3), "spread": round(max(v) - min(v), 3),
                          "runs": [round(x, 3) for x in v]}}
            if name in base_of:
                b = us[base_of[name]]
                rec["minus_k_frame_to_texture_us"] = round(med - statistics.median(b), 3)
                rec["k_frame_to_texture_spread_us"] = round(max(b) - min(b), 3)
                rec["at_or_below_k_frame_to_texture_plus_its_spread"] = med <= statistics.median(b) + (max(b) - min(b))
            out.append(rec)
        for t in list(colour.values()) + list(depth.values()):
            t.Dispose()
        cam.close()
    dev.set_stream(0)
    return out


def end_to_end(light_dev, scr_dev, rounds, frames, warmup):
    size, (kx, ky) = SHAPES[0]
    light_scene = camera_scene(size)
    light = scenes.SceneRenderer(light_dev, light_scene)
    d0 = light_scene.draws[0]
    pid = scr_dev.compile_program(D.SHADOW_FRAGMENT, vertex_source=D.SHADOW_VERTEX)
    k = np.zeros(64, dtype=np.float32)
    k[:16] = (np.asarray(d0.view, dtype=np.float64) @ np.asarray(d0.projection, dtype=np.float64)).astype(np.float32).reshape(-1)
    k[16] = 1.0 / 256.0
    k[17:20], k[20:23] = (1.0, 0.75, 0.5), (0.25, 0.25, 0.5)
    scr_dev.set_program_constants(pid, k)
    s = scenes.cfg3(1920, 1080, (2, 2), (96, 48), tex_size=8, seed=4)
    screen = scenes.SceneRenderer(scr_dev, dataclasses.replace(s, draws=[dataclasses.replace(d, program=pid) for d in s.draws]))
    target = Texture.Depth(scr_dev, TEX, TEX)
    target.SetBilinear(True)
    host = np.empty((size[1], size[0]), dtype=np.float32)
    light_dev.pin(host)
    lib, lctx = light_dev._lib, light_dev._ctx
    state = {"tex": None}

    def frame_new():
        light.submit_frame()
        target.UpdateFromDepth(light.window, kx, ky, DepthReduce.Max)
        screen.submit_frame()

    def frame_host():
        light.submit_frame()
        light_dev._ck(lib.swr_readback(lctx, None, host.ctypes.data))
        old, state["tex"] = state["tex"], Texture.Depth(scr_dev, TEX, TEX, D.reduce(host, kx, ky, D.MAX))
        state["tex"].SetBilinear(True)
        scr_dev.set_program_texture(pid, 1, state["tex"])
        screen.submit_frame()
        if old is not None:
            old.Dispose()

    variants = {"update_from_depth": frame_new, "host_route": frame_host}
    times = {name: [] for name in variants}
    for r in range(rounds + 1):                                         # round 0 warms both variants and is dropped
        for name, fn in variants.items():
            if name != "host_route":
                scr_dev.set_program_texture(pid, 1, target)
            for i in range(warmup + frames):
                if i == warmup:
                    light_dev.sync(); scr_dev.sync(); t0 = time.perf_counter()
                fn()
            light_dev.sync(); scr_dev.sync()
            if r:
                times[name].append((time.perf_counter() - t0) * 1e3 / frames)
    base = summary(times["host_route"])
    out = []
    for name, ms in times.items():
        rec = {"light_frame": list(size), "factors": [kx, ky], "texture": [TEX, TEX], "screen": [1920, 1080], "variant": name,
               "frames": frames, "ms_per_frame": summary(ms)}
        if name != "host_route":
            rec["host_route_over_this"] = round(base["median_ms"] / rec["ms_per_frame"]["median_ms"], 3)
            rec["host_route_spread_ms"] = base["spread_ms"]
        out.append(rec)
    scr_dev.set_program_texture(pid, 1, None)
    if state["tex"] is not None:
        state["tex"].Dispose()
    light_dev.unpin(host)
    target.Dispose(); screen.close(); light.close()
    scr_dev.destroy_program(pid)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_depth_texture.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--frame-warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--bench-before", default=None, help="file holding the bench.py lines of the parent commit's library")
    ap.add_argument("--bench-after", default=None, help="file holding the bench.py lines of this library")
    a = ap.parse_args()
    if a.rounds < 7:
        ap.error("--rounds must be at least 7")
    hip = Hip()
    light_dev, scr_dev = Device(0), Device(0)                           # raises without a GPU: there is nothing to measure then
    res = {"what": "depth textures (tools/depth_texture_rate.py): (a) k_depth_to_texture beside k_frame_to_texture (opaque), device events; "
                   "(b) end to end, light context -> depth texture -> shadowed screen context, host wall clock per frame, "
                   "swr_texture_update_from_depth beside the host route; one process, variants alternated, medians over the rounds, one MI355X",
           "device": light_dev.name, "swr_build_info": light_dev.build_info(), "rounds": a.rounds, "frames": a.frames,
           "frame_warmup": a.frame_warmup, "launches": a.launches, "warmup": a.warmup}
    res["kernel_alone"] = kernel_alone(hip, scr_dev, a.rounds, a.launches, a.warmup)
    res["end_to_end"] = end_to_end(light_dev, scr_dev, a.rounds, a.frames, a.frame_warmup)
    res["bench_cfg3"] = {"cmd": "python bench.py --gpus 1 --steps 50 --warmup 5", "parent_library": bench_lines(a.bench_before),
                         "this_library": bench_lines(a.bench_after)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1); f.write("\n")
    print(json.dumps(res))
    light_dev.close(); scr_dev.close()


if __name__ == "__main__":
    main()
