#!/usr/bin/env python3
"""Cost of render to texture, one JSON file (default profiles/r14_render_to_texture.json).  Needs a GPU.
One process, every shape warmed, the variants alternated over --rounds rounds (at least 7), medians, and the baseline's own
max - min spread beside every difference.  Shapes: a 1024^2 texture from a 2048^2 frame at (2, 2) and from a 1024^2 frame at (1, 1),
cfg3-style content, both alpha modes, with and without the block-linear copy of the bilinear filter.
  (a) end to end, host wall clock ending in a synchronise, frames in flight on: a camera context renders its frame, the frame becomes
      the texture, a screen context renders a 1920x1080 cfg3-style frame that samples it.  With swr_texture_update_from_frame, and
      with the host route of the parent commit in the same process: swr_readback_rgb8 (4 bytes per pixel), swr_texture_create from
      those bytes (swr_texture_set_filter with the bilinear filter), swr_texture_destroy of the previous one.  The host route has no
      alpha to keep: it is the baseline of both alpha modes.
  (b) the kernel alone, device events around --launches back-to-back launches: k_frame_to_texture beside k_present8 of the same
      factors at 4 bytes per pixel into a device buffer.  k_present8 is launched through swr_resolve_rgb8_device_async -- the launch
      of swr_resolve_rgb8_device without its validating wait, which would put a host round trip between the timed launches.
  (c) --bench-before / --bench-after FILE: the `bench.py --gpus 1 --steps 50 --warmup 5` lines of the parent's library and of this one (every
      line of each file: the two are run alternately).
usage: python tools/render_to_texture_rate.py [--out FILE] [--rounds N] [--bench-before FILE] [--bench-after FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from softwarerenderer_amd import Device, Texture, scenes          # noqa: E402
from tools.resolve_rate import Hip                                  # noqa: E402

TEX = 1024
SHAPES = [((2048, 2048), (2, 2)), ((1024, 1024), (1, 1))]


def camera_scene(size):
    return scenes.cfg3(size[0], size[1], (4, 4), (64, 32), tex_size=512, seed=2)


def screen_scene(bilinear):
    return scenes.cfg3(1920, 1080, (2, 2), (96, 48), tex_size=8, seed=4, bilinear=bilinear)


def summary(ms):
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "spread_ms": round(max(ms) - min(ms), 4),
            "runs_ms": [round(x, 4) for x in ms]}


def end_to_end(cam_dev, scr_dev, rounds, frames, warmup):
    out = []
    for size, (kx, ky) in SHAPES:
        cam = scenes.SceneRenderer(cam_dev, camera_scene(size))
        for blocked in (False, True):
            screen = scenes.SceneRenderer(scr_dev, screen_scene(blocked))
            target = Texture.Target(scr_dev, TEX, TEX)
            if blocked:
                target.SetBilinear(True)
            lib, cctx = cam_dev._lib, cam_dev._ctx
            host = np.empty((TEX, TEX, 4), dtype=np.uint8)
            cam_dev.pin(host)
            state = {"tex": None}

            def use(tex):
                for p in screen.programs:
                    p.texture = tex
                screen._calls = None                                   # (the prepared calls hold the texture's handle)

            def frame_new(keep):
                cam.submit_frame()
                target.UpdateFrom(cam.window, kx, ky, keep_alpha=keep)
                screen.submit_frame()

            def frame_host():
                cam.submit_frame()
                cam_dev._ck(lib.swr_readback_rgb8(cctx, kx, ky, 4, host.ctypes.data))
                old, state["tex"] = state["tex"], Texture(scr_dev, host)
                if blocked:
                    state["tex"].SetBilinear(True)
                use(state["tex"])
                screen.submit_frame()
                if old is not None:
                    old.Dispose()

            variants = {"update_from_frame_opaque": lambda: frame_new(False), "update_from_frame_keep_alpha": lambda: frame_new(True),
                        "host_route": frame_host}
            times = {name: [] for name in variants}
            for r in range(rounds + 1):                                 # round 0 warms every variant of this shape and is dropped
                for name, fn in variants.items():
                    if name != "host_route":
                        use(target)
                    for i in range(warmup + frames):
                        if i == warmup:
                            cam_dev.sync(); scr_dev.sync(); t0 = time.perf_counter()
                        fn()
                    cam_dev.sync(); scr_dev.sync()
                    if r:
                        times[name].append((time.perf_counter() - t0) * 1e3 / frames)
            base = summary(times["host_route"])
            for name, ms in times.items():
                rec = {"frame": list(size), "factors": [kx, ky], "texture": [TEX, TEX], "block_linear_copy": blocked, "variant": name,
                       "frames": frames, "ms_per_frame": summary(ms)}
                if name != "host_route":
                    rec["host_route_over_this"] = round(base["median_ms"] / rec["ms_per_frame"]["median_ms"], 3)
                    rec["host_route_spread_ms"] = base["spread_ms"]
                out.append(rec)
            use(None)
            if state["tex"] is not None:
                state["tex"].Dispose()
            cam_dev.unpin(host)
            target.Dispose(); screen.close()
        cam.close()
    return out


def kernel_alone(hip, dev, rounds, launches, warmup):
    out = []
    stream = hip.stream()
    dev.set_stream(stream.value)
    lib, ctx = dev._lib, dev._ctx
    for size, (kx, ky) in SHAPES:
        cam = scenes.SceneRenderer(dev, camera_scene(size))
        cam.render()                                                    # the frame the kernels read: cfg3-style content
        d_out = hip.malloc(TEX * TEX * 4)
        plain, blocked = Texture.Target(dev, TEX, TEX), Texture.Target(dev, TEX, TEX)
        blocked.SetBilinear(True)

        def present8():
            rc = lib.swr_resolve_rgb8_device_async(ctx, kx, ky, 4, d_out)
            if rc:
                dev._ck(rc)

        def update(tex, mode):
            def go():
                rc = lib.swr_texture_update_from_frame(ctx, tex._h, None, kx, ky, mode)
                if rc:
                    dev._ck(rc)
            return go
        variants = {f"k_present8<{kx}, {ky}, 4>": present8,
                    f"k_frame_to_texture<{kx}, {ky}, false, false>": update(plain, 0),
                    f"k_frame_to_texture<{kx}, {ky}, true, false>": update(plain, 1),
                    f"k_frame_to_texture<{kx}, {ky}, false, true>": update(blocked, 0),
                    f"k_frame_to_texture<{kx}, {ky}, true, true>": update(blocked, 1)}
        runs = {name: [] for name in variants}
        for r in range(rounds + 1):                                     # round 0 is the warm-up of every variant
            for name, fn in variants.items():
                ms = hip.timed(stream, fn, launches, warmup)
                if r:
                    runs[name].append(ms)
        dev.sync()
        base_name = f"k_present8<{kx}, {ky}, 4>"
        us = {name: [x * 1e3 for x in ms] for name, ms in runs.items()}      # microseconds per launch, one figure per round
        base_med, base_spread = statistics.median(us[base_name]), max(us[base_name]) - min(us[base_name])
        for name, v in us.items():
            med = statistics.median(v)
            texels = TEX * TEX
            by = texels * kx * ky * 16 + texels * 4 * (2 if name.endswith("true>") else 1)
            rec = {"kernel": name, "frame": list(size), "texture": [TEX, TEX],
                   "us": {"median": round(med, 3), "min": round(min(v), 3), "max": round(max(v), 3), "spread": round(max(v) - min(v), 3),
                          "runs": [round(x, 3) for x in v]},
                   "algorithmic_bytes": by, "gb_per_s": round(by / (med * 1e-6) / 1e9, 1)}
            if name != base_name:
                rec["minus_k_present8_us"] = round(med - base_med, 3)
                rec["k_present8_spread_us"] = round(base_spread, 3)
                rec["inside_k_present8_spread"] = abs(med - base_med) <= base_spread
            out.append(rec)
        hip.lib.hipFree(d_out)
        plain.Dispose(); blocked.Dispose(); cam.close()
    dev.set_stream(0)
    return out


def bench_lines(path):
    """Every JSON line of the file (the runs of one library, in the order they were made)."""
    if not path or not os.path.exists(path):
        return None
    runs = [json.loads(ln) for ln in open(path).read().splitlines() if ln.startswith("{")]
    return [{"ms_per_step": b.get("ms_per_step"), "value": b.get("value"), "unit": b.get("unit")} for b in runs] or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_render_to_texture.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--frame-warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--bench-before", default=None, help="file holding the bench.py lines of the parent commit's library")
    ap.add_argument("--bench-after", default=None, help="file holding the bench.py lines of this library")
    a = ap.parse_args()
    if a.rounds < 7:
        ap.error("--rounds must be at least 7")
    hip = Hip()
    cam_dev, scr_dev = Device(0), Device(0)                             # raises without a GPU: there is nothing to measure then
    res = {"what": "render to texture (tools/render_to_texture_rate.py): (a) end to end, camera context -> texture -> screen context, host wall "
                   "clock per frame, swr_texture_update_from_frame beside the parent commit's host route; (b) k_frame_to_texture beside k_present8 "
                   "(4 bytes per pixel), device events; one process, variants alternated, medians over the rounds, one MI355X",
           "device": cam_dev.name, "swr_build_info": cam_dev.build_info(), "rounds": a.rounds, "frames": a.frames, "frame_warmup": a.frame_warmup,
           "launches": a.launches, "warmup": a.warmup}
    res["end_to_end"] = end_to_end(cam_dev, scr_dev, a.rounds, a.frames, a.frame_warmup)
    res["kernel_alone"] = kernel_alone(hip, scr_dev, a.rounds, a.launches, a.warmup)
    res["bench_cfg3"] = {"cmd": "python bench.py --gpus 1 --steps 50 --warmup 5", "parent_library": bench_lines(a.bench_before),
                         "this_library": bench_lines(a.bench_after)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1); f.write("\n")
    print(json.dumps(res))
    cam_dev.close(); scr_dev.close()


if __name__ == "__main__":
    main()
