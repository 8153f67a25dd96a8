#!/usr/bin/env python3
"""Cost of post-process programs, one JSON file (default profiles/r15_post.json), on one MI355X:
  (a) kernel time, device events around --launches launches after --warmup, the candidates of a case alternated three times in one
      process: at 1920x1080 (1, 1) RGBX8 the IDENTITY program's k_post beside k_present8<1, 1, 4> (both move the same bytes), then
      TINT and BOX3; at 3840x2160 (2, 2) k_resolve_rgba + k_post beside k_present8<2, 2, 4>: the intermediate RGBA plane costs one
      more write and read of 16 B per window pixel, and this is where that is measured.
  (b) frame loop with pinned buffers and 1 M triangles (scenes.cfg3), host wall clock, alternated three times: render 1920x1080,
      swr_present_post_async (TINT, RGB8), wait for the previous ticket; the same loop with swr_present_rgb8_async; and the host
      route the feature replaces -- swr_readback, TINT in numpy, quantise in numpy.
  (c) --bench-json FILE [--parent-bench-json FILE]: `bench.py --gpus 1 --steps 50 --warmup 5` lines of this commit and its parent
      from the same session, recorded beside the rest.
usage: python tools/post_rate.py [--out FILE] [--bench-json FILE] [--parent-bench-json FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

from softwarerenderer_amd import Device, MainWindow, PostProgram, _native, scenes          # noqa: E402
from tools.resolve_rate import COPY_PEAK_GBS, Hip                                           # noqa: E402
import post_cases as P                                                                      # noqa: E402

IDENTITY, TINT, BOX3, TINT_K = P.IDENTITY, P.TINT, P.BOX3, P.TINT_CONSTANTS       # the programs the tests hold, with their twins
CASES = [((1920, 1080), (1, 1)), ((3840, 2160), (2, 2))]


def timed(hip, stream, fn, launches, warmup):
    """(ms per launch between two device events around `launches` back-to-back calls, ms per call the host took to enqueue them):
    where the second is not well below the first, the first measures the enqueue rate, not the kernel."""
    e0, e1 = hip.event(), hip.event()
    for _ in range(warmup):
        fn()
    hip.ck(hip.lib.hipEventRecord(e0, stream))
    t0 = time.perf_counter()
    for _ in range(launches):
        fn()
    host_ms = (time.perf_counter() - t0) * 1e3 / launches
    hip.ck(hip.lib.hipEventRecord(e1, stream))
    hip.ck(hip.lib.hipEventSynchronize(e1))
    ms = C.c_float(0)
    hip.ck(hip.lib.hipEventElapsedTime(C.byref(ms), e0, e1))
    hip.lib.hipEventDestroy(e0); hip.lib.hipEventDestroy(e1)
    return ms.value / launches, host_ms


def kernel_times(hip, dev, launches, warmup):
    out = []
    stream = hip.stream()
    dev.set_stream(stream.value)
    posts = {"IDENTITY": PostProgram(dev, IDENTITY), "TINT": PostProgram(dev, TINT, constants=TINT_K), "BOX3": PostProgram(dev, BOX3)}
    rng = np.random.default_rng(1)
    lib, ctx = dev._lib, dev._ctx
    for (w, h), (kx, ky) in CASES:
        ow, oh = w // kx, h // ky
        d_out = hip.malloc(ow * oh * 4)
        win = MainWindow(dev, w, h)
        win.Upload(color=rng.random((h, w, 4), dtype=np.float32), depth=rng.random((h, w), dtype=np.float32))

        def present8():
            rc = lib.swr_resolve_rgb8_device_async(ctx, kx, ky, 4, d_out)
            if rc:
                dev._ck(rc)

        def post(name):
            pid = posts[name]._id

            def run():
                rc = lib.swr_post_device_async(ctx, pid, kx, ky, _native.SWR_POST_RGBX8, d_out)
                if rc:
                    dev._ck(rc)
            return run

        resolve_too = "k_resolve_rgba<%d, %d> + " % (kx, ky) if (kx, ky) != (1, 1) else ""
        cands = {f"k_present8<{kx}, {ky}, 4>": present8, f"k_present8<{kx}, {ky}, 4> again": present8}
        cands.update({f"{resolve_too}k_post<RGBX8> {name}": post(name) for name in posts})
        runs, enqueue = {}, {}
        for _ in range(3):
            for label, fn in cands.items():
                ms, host_ms = timed(hip, stream, fn, launches, warmup)
                runs.setdefault(label, []).append(ms)
                enqueue.setdefault(label, []).append(host_ms)
        dev.sync()
        hip.lib.hipFree(d_out)
        base = statistics.median(runs[f"k_present8<{kx}, {ky}, 4>"])
        for label, ms in runs.items():
            med = statistics.median(ms)
            by = w * h * 16 + ow * oh * 4 + (0 if "k_post" not in label or (kx, ky) == (1, 1) else 2 * ow * oh * 16)
            out.append({"case": label, "source": [w, h], "factors": [kx, ky], "runs_us": [round(x * 1e3, 2) for x in ms], "us": round(med * 1e3, 2),
                        "host_enqueue_us_per_launch": round(statistics.median(enqueue[label]) * 1e3, 2),
                        "ratio_to_k_present8": round(med / base, 3), "spread": round((max(ms) - min(ms)) / med, 4),
                        "bytes_moved_frame_plus_plane_plus_output": by, "gb_per_s": round(by / (med * 1e-3) / 1e9, 1),
                        "share_of_copy_peak": round(by / (med * 1e-3) / 1e9 / COPY_PEAK_GBS, 3)})
    for p in posts.values():
        p.close()
    dev.set_stream(0)
    return out


def host_tint_rgb8(color, k):
    """The host route's arithmetic: TINT and the 8-bit quantiser in numpy float32."""
    c = color[..., :3] * k[0:3] + k[3:6]
    with np.errstate(invalid="ignore"):
        q = np.rint(np.clip(np.nan_to_num(c, nan=0.0), 0.0, 1.0) * np.float32(255.0))
    return q.astype(np.uint8)


def frame_loops(dev, frames, warmup, host_frames):
    r = scenes.SceneRenderer(dev, scenes.cfg3(1920, 1080, tex_size=1024))
    win = r.window
    tint = PostProgram(dev, TINT, constants=TINT_K)
    bufs = [np.zeros((1080, 1920, 3), dtype=np.uint8) for _ in range(2)]
    color = np.zeros((1080, 1920, 4), dtype=np.float32)
    for b in bufs + [color]:
        dev.pin(b)
    r.render(); r.render()                                             # sizes the pair buffers of both raster sets
    loops = ["render_present_post_tint_rgb8", "render_present8_rgb8", "render_readback_numpy_tint_quantise"]
    times = {name: [] for name in loops}
    for _ in range(3):
        for name in loops:
            host = name.startswith("render_readback")
            n = host_frames if host else frames
            tickets, t0 = [None, None], 0.0
            for i in range(warmup + n):
                if i == warmup:
                    dev.sync(); t0 = time.perf_counter()
                r.submit_frame()
                if host:
                    dev._ck(dev._lib.swr_readback(dev._ctx, color.ctypes.data, None))
                    host_tint_rgb8(color, TINT_K)
                    continue
                j = i & 1
                if tickets[j] is not None:
                    win.PresentWait(tickets[j])
                tickets[j] = win.PresentPostAsync(tint, bufs[j], 1, 1) if "post" in name else win.Present8Async(bufs[j], 1, 1)
            for t in tickets:
                if t is not None:
                    win.PresentWait(t)
            dev.sync()
            times[name].append((time.perf_counter() - t0) * 1e3 / n)
    for b in bufs + [color]:
        dev.unpin(b)
    tint.close(); r.close()
    return {name: {"ms_per_frame": round(statistics.median(v), 4), "runs_ms": [round(x, 4) for x in v]} for name, v in times.items()}


def bench_line(path):
    if not path or not os.path.exists(path):
        return None
    lines = [json.loads(ln) for ln in open(path).read().splitlines() if ln.startswith("{")]
    return {"cmd": "python bench.py --gpus 1 --steps 50 --warmup 5", "ms_per_step": [b.get("ms_per_step") for b in lines],
            "value": [b.get("value") for b in lines], "unit": lines[-1].get("unit") if lines else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_post.json"))
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--host-frames", type=int, default=10)
    ap.add_argument("--frame-warmup", type=int, default=5)
    ap.add_argument("--bench-json", default=None, help="file of JSON lines of bench.py --gpus 1 --steps 50 --warmup 5 on this commit")
    ap.add_argument("--parent-bench-json", default=None, help="... and on the parent commit, same session")
    a = ap.parse_args()
    hip = Hip()
    dev = Device(0)
    res = {"what": "post-process programs (tools/post_rate.py): (a) kernel time of k_post (and k_resolve_rgba in front of it) beside k_present8 on "
                   "the same planes into RGBX8, device events, three alternated runs, median; (b) frame loops at 1920x1080 with 1 M triangles and "
                   "pinned buffers, host wall clock; one MI355X",
           "device": dev.name, "swr_build_info": dev.build_info(), "launches": a.launches, "warmup": a.warmup, "copy_peak_gb_per_s": COPY_PEAK_GBS,
           "kernel_time": kernel_times(hip, dev, a.launches, a.warmup),
           "frames": a.frames, "host_frames": a.host_frames, "frame_warmup": a.frame_warmup,
           "frame_loop": frame_loops(dev, a.frames, a.frame_warmup, a.host_frames),
           "bench_cfg3": bench_line(a.bench_json), "bench_cfg3_parent": bench_line(a.parent_bench_json)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1); f.write("\n")
    print(json.dumps(res))
    dev.close()


if __name__ == "__main__":
    main()
