#!/usr/bin/env python3
"""Cost of the supersampled present, one JSON file (default profiles/r10_resolve.json):
  (a) kernel time, device events around --launches launches after --warmup: k_resolve_rgb (2, 2) at 3840x2160, (4, 4) and (1, 1) at
      4096^2, and k_flatten_rgb on the same planes in the same call, alternated three times; algorithmic bytes (source x 16 +
      output x 12), GB/s, share of the 6.29 TB/s measured copy peak, the A/A spread of the flatten.  --ab-lib FILE times another
      in-tree build of the library (make EXTRA=...) in the same process.
  (b) frame loop with pinned buffers, --frames frames after --frame-warmup, alternated three times: render 3840x2160 and present
      resolved (2, 2); render 3840x2160 and PresentAsync; render 1920x1080 and PresentAsync.
  (c) --bench-json FILE: a `bench.py --gpus 1 --steps 50 --warmup 5` line recorded beside it, with the parent's recorded figure.
With --present8 the same two measurements are made for the 8-bit present (default profiles/r13_present8.json):
  (a) k_present8 at (1, 1) and (2, 2), 3 and 4 bytes per pixel, at 3840x2160 and 4096^2, beside k_flatten_rgb and k_resolve_rgb of
      the same factors on the same plane; --ab-lib as above.
  (b) render 1920x1080 and Present8Async (1, 1), render 3840x2160 and Present8Async (2, 2), 3 bytes per pixel, each beside the same
      loop with today's float present (PresentAsync, PresentResolvedAsync (2, 2)) in the same process.
usage: python tools/resolve_rate.py [--present8] [--out FILE] [--ab-lib libNAME.so] [--bench-json FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from softwarerenderer_amd import Device, MainWindow, scenes          # noqa: E402

COPY_PEAK_GBS = 6290.0            # measured float4 copy peak of one MI355X
PARENT_CFG3_MS = 0.555            # README, "Performance": bench.py cfg3 on the parent, frames in flight
# the three cases the feature is quoted on, then the extremes of the factor range (the widest lane stride, the most rows per thread)
KERNEL_CASES = [((3840, 2160), [(2, 2)]), ((4096, 4096), [(4, 4), (1, 1), (8, 8), (8, 1), (1, 8)])]
PRESENT8_CASES = [((3840, 2160), [(1, 1), (2, 2)]), ((4096, 4096), [(1, 1), (2, 2), (8, 8)])]      # (8, 8): the most registers


class Hip:
    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so")

    def ck(self, rc):
        if rc:
            raise RuntimeError(f"HIP error {rc}")

    def malloc(self, nbytes):
        p = C.c_void_p()
        self.ck(self.lib.hipMalloc(C.byref(p), C.c_size_t(nbytes)))
        return p

    def stream(self):
        s = C.c_void_p()
        self.ck(self.lib.hipStreamCreate(C.byref(s)))
        return s

    def event(self):
        e = C.c_void_p()
        self.ck(self.lib.hipEventCreate(C.byref(e)))
        return e

    def timed(self, stream, fn, launches, warmup):
        """ms per launch of fn(), device events around `launches` back-to-back calls on `stream`."""
        e0, e1 = self.event(), self.event()
        for _ in range(warmup):
            fn()
        self.ck(self.lib.hipEventRecord(e0, stream))
        for _ in range(launches):
            fn()
        self.ck(self.lib.hipEventRecord(e1, stream))
        self.ck(self.lib.hipEventSynchronize(e1))
        ms = C.c_float(0)
        self.ck(self.lib.hipEventElapsedTime(C.byref(ms), e0, e1))
        self.lib.hipEventDestroy(e0); self.lib.hipEventDestroy(e1)
        return ms.value / launches


def rate(ms, src_px, out_px, out_bpp=12):
    by = src_px * 16 + out_px * out_bpp
    gbs = by / (ms * 1e-3) / 1e9
    return {"us": round(ms * 1e3, 2), "algorithmic_bytes": by, "gb_per_s": round(gbs, 1), "share_of_copy_peak": round(gbs / COPY_PEAK_GBS, 3)}


def kernel_times(hip, devs, launches, warmup, cases=KERNEL_CASES, present8=False):
    """devs: {label: Device}.  Per plane size: flatten and each resolve case (with present8, k_present8 of the same factors at 3 and
    4 bytes per pixel as well) on every build, the round repeated three times."""
    out = []
    stream = hip.stream()
    for dev in devs.values():
        dev.set_stream(stream.value)
    rng = np.random.default_rng(1)
    for (w, h), pairs in cases:
        d_rgb = hip.malloc(w * h * 12)
        wins = {}
        for label, dev in devs.items():
            wins[label] = MainWindow(dev, w, h)
            wins[label].Upload(color=rng.random((h, w, 4), dtype=np.float32))
        runs = {}
        for _ in range(3):
            for label, dev in devs.items():
                lib, ctx = dev._lib, dev._ctx
                wins[label]._activate()

                def flatten():
                    rc = lib.swr_flatten_rgb_device_async(ctx, d_rgb)
                    if rc:
                        dev._ck(rc)
                runs.setdefault((label, "k_flatten_rgb"), []).append(hip.timed(stream, flatten, launches, warmup))
                for kx, ky in pairs:
                    def resolve():
                        rc = lib.swr_resolve_rgb_device_async(ctx, kx, ky, d_rgb)
                        if rc:
                            dev._ck(rc)
                    runs.setdefault((label, f"k_resolve_rgb<{kx}, {ky}>"), []).append(hip.timed(stream, resolve, launches, warmup))
                    for bpp in (3, 4) if present8 else ():
                        def quantise():
                            rc = lib.swr_resolve_rgb8_device_async(ctx, kx, ky, bpp, d_rgb)
                            if rc:
                                dev._ck(rc)
                        runs.setdefault((label, f"k_present8<{kx}, {ky}, {bpp}>"), []).append(hip.timed(stream, quantise, launches, warmup))
        for dev in devs.values():
            dev.sync()
        hip.lib.hipFree(d_rgb)
        for (label, kernel), ms in runs.items():
            k = [int(x) for x in kernel[kernel.index("<") + 1:-1].split(",")] if "<" in kernel else (1, 1)
            med = statistics.median(ms)
            rec = {"build": label, "kernel": kernel, "source": [w, h], "runs_us": [round(x * 1e3, 2) for x in ms]}
            rec.update(rate(med, w * h, (w // k[0]) * (h // k[1]), k[2] if len(k) == 3 else 12))
            rec["spread"] = round((max(ms) - min(ms)) / med, 4)          # of three alternated runs: for the flatten, the A/A spread
            out.append(rec)
    for dev in devs.values():
        dev.set_stream(0)
    return out


def frame_loops(dev, frames, warmup, present8=False):
    """ms per frame (host wall clock over `frames` frames, present i / wait i - 2) of the loops, alternated three times.  A loop is
    (renderer, resolve factors or None for PresentAsync, payload shape, payload type): a uint8 payload goes through Present8Async, and
    a loop without a payload only renders (one sync at the end) -- what the loop costs when nothing is copied."""
    big = scenes.cfg3(3840, 2160, tex_size=1024)
    small = scenes.cfg3(1920, 1080, tex_size=1024)
    rb = scenes.SceneRenderer(dev, big)
    rs = scenes.SceneRenderer(dev, small)
    if present8:
        loops = {"render_1920x1080_present8_1x1_rgb8": (rs, (1, 1), (1080, 1920, 3), np.uint8),
                 "render_1920x1080_present_plain": (rs, None, (1080, 1920, 3), np.float32),
                 "render_3840x2160_present8_2x2_rgb8": (rb, (2, 2), (1080, 1920, 3), np.uint8),
                 "render_3840x2160_present_resolved_2x2": (rb, (2, 2), (1080, 1920, 3), np.float32),
                 "render_1920x1080_no_present": (rs, None, (0,), None),
                 "render_3840x2160_no_present": (rb, None, (0,), None)}
    else:
        loops = {"render_3840x2160_present_resolved_2x2": (rb, (2, 2), (1080, 1920, 3), np.float32),
                 "render_3840x2160_present_plain": (rb, None, (2160, 3840, 3), np.float32),
                 "render_1920x1080_present_plain": (rs, None, (1080, 1920, 3), np.float32)}
    bufs = {name: [np.zeros(shape, dtype=dtype) for _ in range(2)] for name, (_, _, shape, dtype) in loops.items() if dtype}
    for pair in bufs.values():
        for b in pair:
            dev.pin(b)
    for r in (rb, rs):
        r.render(); r.render()                                         # sizes the pair buffers of both raster sets
    times = {name: [] for name in loops}
    for _ in range(3):
        for name, (r, k, _, dtype) in loops.items():
            win, tickets, t0 = r.window, [None, None], 0.0
            for i in range(warmup + frames):
                if i == warmup:
                    dev.sync(); t0 = time.perf_counter()
                r.submit_frame()
                if dtype is None:
                    continue
                j = i & 1
                if tickets[j] is not None:
                    win.PresentWait(tickets[j])
                if dtype == np.uint8:
                    tickets[j] = win.Present8Async(bufs[name][j], *k)
                else:
                    tickets[j] = win.PresentResolvedAsync(bufs[name][j], *k) if k else win.PresentAsync(bufs[name][j])
            for t in tickets:
                if t is not None:
                    win.PresentWait(t)
            dev.sync()
            times[name].append((time.perf_counter() - t0) * 1e3 / frames)
    for pair in bufs.values():
        for b in pair:
            dev.unpin(b)
    rb.close(); rs.close()
    return {name: {"ms_per_frame": round(statistics.median(v), 4), "runs_ms": [round(x, 4) for x in v],
                   "bytes_to_host_per_frame": int(np.prod(loops[name][2])) * np.dtype(loops[name][3] or np.uint8).itemsize} for name, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--present8", action="store_true", help="measure the 8-bit present instead (default output profiles/r13_present8.json)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--frame-warmup", type=int, default=5)
    ap.add_argument("--ab-lib", default=None, help="another in-tree build of the library to time beside the product (file name)")
    ap.add_argument("--bench-json", default=None, help="file holding the JSON line of bench.py --gpus 1 --steps 50 --warmup 5")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "r13_present8.json" if a.present8 else "r10_resolve.json")
    hip = Hip()
    dev = Device(0)
    devs = {"product": dev}
    if a.ab_lib:
        devs[a.ab_lib] = Device(0, lib=a.ab_lib)
    what = ("8-bit present (tools/resolve_rate.py --present8): (a) kernel time of k_present8 beside k_flatten_rgb and k_resolve_rgb of the "
            "same factors on the same planes" if a.present8 else
            "supersampled present (tools/resolve_rate.py): (a) kernel time of k_resolve_rgb beside k_flatten_rgb on the same planes")
    res = {"what": what + ", device events, three alternated runs, median; (b) frame loops with pinned buffers, host wall clock; one MI355X",
           "device": dev.name, "swr_build_info": dev.build_info(),
           "builds": {label: d.build_info() for label, d in devs.items()},
           "launches": a.launches, "warmup": a.warmup, "copy_peak_gb_per_s": COPY_PEAK_GBS,
           "kernel_time": kernel_times(hip, devs, a.launches, a.warmup, PRESENT8_CASES if a.present8 else KERNEL_CASES, a.present8)}
    for label, d in devs.items():
        if d is not dev:
            d.close()
    res["frames"], res["frame_warmup"] = a.frames, a.frame_warmup
    res["frame_loop"] = frame_loops(dev, a.frames, a.frame_warmup, a.present8)
    if a.bench_json and os.path.exists(a.bench_json):
        lines = [ln for ln in open(a.bench_json).read().splitlines() if ln.startswith("{")]
        b = json.loads(lines[-1])
        res["bench_cfg3"] = {"cmd": "python bench.py --gpus 1 --steps 50 --warmup 5", "ms_per_step": b.get("ms_per_step"), "value": b.get("value"),
                             "unit": b.get("unit"), "parent_recorded_ms_per_step": PARENT_CFG3_MS}
    else:
        res["bench_cfg3"] = None
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1); f.write("\n")
    print(json.dumps(res))
    dev.close()


if __name__ == "__main__":
    main()
