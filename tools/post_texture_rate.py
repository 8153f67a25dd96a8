#!/usr/bin/env python3
"""Cost of textures in post programs and of a pass into a texture, one JSON file (default
profiles/r16_post_texture.json).  Needs a GPU.  One process on one MI355X, every variant warmed, the variants of a group alternated
over --rounds rounds, medians; the reference points (the identity program's k_post, k_frame_to_texture, the host route) are
measured in the same process, not taken from older files.
  (a), (b) kernel time at 1920x1080, (1, 1), RGBX8 into a device buffer, device events around --launches back-to-back launches: the
      IDENTITY program's k_post; SAMPLE (tests/post_texture_cases.py) with one 1024^2 texture, uv one to one over the window, under
      the nearest filter and under the bilinear filter (block-linear copy); SAMPLE with the slot unbound; OVERLAY, which reads the
      frame as well (SAMPLE's result does not depend on in.color, so the compiler drops the frame's load from its k_post).
  (c) swr_texture_update_from_post of the IDENTITY program into a 1024^2 target from a 1024^2 frame, with and without the target's
      block-linear copy and in both alpha modes, beside swr_texture_update_from_frame (k_frame_to_texture) on the same shapes.  The
      two-pass alternative (RGBX8 into the texels, then k_block_texture) was not built: there is no figure for it.
  (d) the blur chain as frame time, host wall clock ending in a synchronise: a camera context renders 2048^2, BLUR_H at (2, 2) into
      a 1024^2 texture A, BLUR_V of A into T, a screen context renders a 1920x1080 frame that samples T -- beside the host route in
      the same loop: swr_readback_post of each pass and swr_texture_create of its bytes.
  (e) --bench-before / --bench-after FILE: the `bench.py --gpus 1 --steps 50 --warmup 5` lines of the parent commit's tree and of this
      one, run alternately in the same session, recorded beside the rest.
usage: python tools/post_texture_rate.py [--out FILE] [--rounds N] [--bench-before FILE] [--bench-after FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

from softwarerenderer_amd import Device, MainWindow, PostProgram, Texture, _native, scenes          # noqa: E402
from tools.resolve_rate import Hip                                                                  # noqa: E402
import post_cases as P                                                                              # noqa: E402
import post_texture_cases as X                                                                      # noqa: E402

TEX = 1024


def stats_us(ms):
    v = [x * 1e3 for x in ms]
    med = statistics.median(v)
    return {"median": round(med, 3), "min": round(min(v), 3), "max": round(max(v), 3), "spread": round(max(v) - min(v), 3),
            "runs": [round(x, 3) for x in v]}


def alternate(hip, stream, variants, rounds, launches, warmup):
    runs = {name: [] for name in variants}
    for r in range(rounds + 1):                                         # round 0 is the warm-up of every variant
        for name, fn in variants.items():
            ms = hip.timed(stream, fn, launches, warmup)
            if r:
                runs[name].append(ms)
    return runs


def sampling_kernels(hip, dev, rounds, launches, warmup):
    stream = hip.stream()
    dev.set_stream(stream.value)
    lib, ctx = dev._lib, dev._ctx
    w, h = 1920, 1080
    rng = np.random.default_rng(1)
    win = MainWindow(dev, w, h)
    win.Upload(color=rng.random((h, w, 4), dtype=np.float32), depth=rng.random((h, w), dtype=np.float32))
    texels = rng.integers(0, 256, (TEX, TEX, 4), dtype=np.uint8)
    nearest, bilinear = Texture(dev, texels), Texture(dev, texels)
    bilinear.SetBilinear(True)
    d_out = hip.malloc(w * h * 4)
    k = P.constants64([1.0 / w, 1.0 / h, 0.0, 0.0, 0.0])                # uv one to one over the window
    # the programs without textures of DESIGN.md section 20, re-measured: their k_post now carries the slots in its argument
    progs = {"IDENTITY": PostProgram(dev, P.IDENTITY), "TINT": PostProgram(dev, P.TINT, constants=P.TINT_CONSTANTS), "BOX3": PostProgram(dev, P.BOX3)}
    for name, tex in (("SAMPLE nearest", nearest), ("SAMPLE bilinear, block-linear copy", bilinear), ("SAMPLE, slot unbound", None)):
        progs[name] = PostProgram(dev, X.SAMPLE, constants=k)
        progs[name].SetTexture(0, tex)
    # SAMPLE never reads in.color, so its k_post does not load the frame; OVERLAY reads both the frame and the texture
    for name, tex in (("OVERLAY nearest", nearest), ("OVERLAY bilinear, block-linear copy", bilinear)):
        progs[name] = PostProgram(dev, X.OVERLAY, constants=k)
        progs[name].SetTexture(0, tex)

    def post(pid):
        def go():
            rc = lib.swr_post_device_async(ctx, pid, 1, 1, _native.SWR_POST_RGBX8, d_out)
            if rc:
                dev._ck(rc)
        return go
    variants = {"k_post<RGBX8> " + name: post(p._id) for name, p in progs.items()}
    runs = alternate(hip, stream, variants, rounds, launches, warmup)
    dev.sync()
    base = statistics.median(runs["k_post<RGBX8> IDENTITY"]) * 1e3
    out = []
    for name, ms in runs.items():
        rec = {"case": name, "source": [w, h], "factors": [1, 1], "texture": [TEX, TEX], "us": stats_us(ms)}
        rec["minus_identity_us"] = round(rec["us"]["median"] - base, 3)
        out.append(rec)
    for p in progs.values():
        p.close()
    hip.lib.hipFree(d_out)
    nearest.Dispose(); bilinear.Dispose()
    dev.set_stream(0)
    return out


def pass_into_texture(hip, dev, rounds, launches, warmup):
    stream = hip.stream()
    dev.set_stream(stream.value)
    lib, ctx = dev._lib, dev._ctx
    win = MainWindow(dev, TEX, TEX)
    win.Upload(color=np.random.default_rng(2).random((TEX, TEX, 4), dtype=np.float32))
    plain, blocked = Texture.Target(dev, TEX, TEX), Texture.Target(dev, TEX, TEX)
    blocked.SetBilinear(True)
    identity = PostProgram(dev, P.IDENTITY)

    def from_post(tex, mode):
        def go():
            rc = lib.swr_texture_update_from_post(ctx, tex._h, None, identity._id, 1, 1, mode)
            if rc:
                dev._ck(rc)
        return go

    def from_frame(tex, mode):
        def go():
            rc = lib.swr_texture_update_from_frame(ctx, tex._h, None, 1, 1, mode)
            if rc:
                dev._ck(rc)
        return go
    variants = {}
    for label, tex in (("row-major only", plain), ("with block-linear copy", blocked)):
        for mode, alpha in ((0, "opaque"), (1, "keep alpha")):
            variants[f"k_frame_to_texture<1, 1>, {alpha}, {label}"] = from_frame(tex, mode)
            variants[f"k_post<texels> IDENTITY, {alpha}, {label}"] = from_post(tex, mode)
    runs = alternate(hip, stream, variants, rounds, launches, warmup)
    dev.sync()
    out = [{"case": name, "frame": [TEX, TEX], "factors": [1, 1], "texture": [TEX, TEX], "us": stats_us(ms)} for name, ms in runs.items()]
    identity.close(); plain.Dispose(); blocked.Dispose()
    dev.set_stream(0)
    return out


def blur_chain(cam_dev, scr_dev, rounds, frames, warmup):
    cam = scenes.SceneRenderer(cam_dev, scenes.cfg3(2048, 2048, (4, 4), (64, 32), tex_size=512, seed=2))
    screen = scenes.SceneRenderer(scr_dev, scenes.cfg3(1920, 1080, (2, 2), (96, 48), tex_size=8, seed=4))
    blur_h, blur_v = PostProgram(cam_dev, X.BLUR_H), PostProgram(cam_dev, X.BLUR_V)
    a, t = Texture.Target(cam_dev, TEX, TEX), Texture.Target(scr_dev, TEX, TEX)
    lib, cctx = cam_dev._lib, cam_dev._ctx
    host_a, host_t = np.empty((TEX, TEX, 4), dtype=np.uint8), np.empty((TEX, TEX, 4), dtype=np.uint8)
    cam_dev.pin(host_a); cam_dev.pin(host_t)
    state = {"a": None, "t": None}

    def use(tex):
        for p in screen.programs:
            p.texture = tex
        screen._calls = None                                            # (the prepared calls hold the texture's handle)

    def frame_device():
        cam.submit_frame()
        a.UpdateFromPost(cam.window, blur_h, 2, 2, keep_alpha=True)     # on the camera's stream
        t.UpdateFromPost(cam.window, blur_v, 2, 2)                      # on the screen's stream, behind the camera's
        screen.submit_frame()

    def frame_host():
        cam.submit_frame()
        cam_dev._ck(lib.swr_readback_post(cctx, blur_h._id, 2, 2, _native.SWR_POST_RGBX8, host_a.ctypes.data))
        old_a, state["a"] = state["a"], Texture(cam_dev, host_a)
        blur_v.SetTexture(0, state["a"])
        cam_dev._ck(lib.swr_readback_post(cctx, blur_v._id, 2, 2, _native.SWR_POST_RGBX8, host_t.ctypes.data))
        old_t, state["t"] = state["t"], Texture(scr_dev, host_t)
        use(state["t"])
        screen.submit_frame()
        for old in (old_a, old_t):                                      # (each waits for its context: the copies out of the host buffers are over)
            if old is not None:
                old.Dispose()

    variants = {"update_from_post_twice": frame_device, "host_route_readback_post_and_texture_create": frame_host}
    times = {name: [] for name in variants}
    for r in range(rounds + 1):                                         # round 0 warms both variants and is dropped
        for name, fn in variants.items():
            if name == "update_from_post_twice":
                blur_v.SetTexture(0, a)
                use(t)
            for i in range(warmup + frames):
                if i == warmup:
                    cam_dev.sync(); scr_dev.sync(); t0 = time.perf_counter()
                fn()
            cam_dev.sync(); scr_dev.sync()
            if r:
                times[name].append((time.perf_counter() - t0) * 1e3 / frames)
    out = {name: {"ms_per_frame": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                  "runs_ms": [round(x, 4) for x in v]} for name, v in times.items()}
    out["host_route_over_update_from_post"] = round(out["host_route_readback_post_and_texture_create"]["ms_per_frame"] /
                                                    out["update_from_post_twice"]["ms_per_frame"], 3)
    use(None)
    blur_v.SetTexture(0, None)
    for tex in (state["a"], state["t"], a, t):
        if tex is not None:
            tex.Dispose()
    cam_dev.sync(); scr_dev.sync()
    cam_dev.unpin(host_a); cam_dev.unpin(host_t)
    blur_h.close(); blur_v.close(); screen.close(); cam.close()
    return out


def bench_lines(path):
    """Every JSON line of the file (the runs of one tree, in the order they were made)."""
    if not path or not os.path.exists(path):
        return None
    runs = [json.loads(ln) for ln in open(path).read().splitlines() if ln.startswith("{")]
    return [{"ms_per_step": b.get("ms_per_step"), "value": b.get("value"), "unit": b.get("unit")} for b in runs] or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_post_texture.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--frame-warmup", type=int, default=5)
    ap.add_argument("--bench-before", default=None, help="file holding the bench.py lines of the parent commit's tree")
    ap.add_argument("--bench-after", default=None, help="file holding the bench.py lines of this tree")
    a = ap.parse_args()
    hip = Hip()
    cam_dev, scr_dev = Device(0), Device(0)                             # raises without a GPU: there is nothing to measure then
    res = {"what": "textures in post programs and a pass into a texture (tools/post_texture_rate.py): (a), (b) k_post sampling one 1024^2 texture "
                   "beside the identity program at 1920x1080 into RGBX8; (c) swr_texture_update_from_post beside swr_texture_update_from_frame "
                   "into a 1024^2 target; device events, per launch; (d) the two-pass blur of a 2048^2 camera frame onto a 1920x1080 screen frame "
                   "beside the host route, host wall clock per frame; one process, variants alternated, medians over the rounds, one MI355X",
           "device": cam_dev.name, "swr_build_info": cam_dev.build_info(), "rounds": a.rounds, "launches": a.launches, "warmup": a.warmup,
           "frames": a.frames, "frame_warmup": a.frame_warmup}
    res["sampling_kernels"] = sampling_kernels(hip, scr_dev, a.rounds, a.launches, a.warmup)
    res["pass_into_texture"] = pass_into_texture(hip, scr_dev, a.rounds, a.launches, a.warmup)
    res["blur_chain"] = blur_chain(cam_dev, scr_dev, a.rounds, a.frames, a.frame_warmup)
    res["bench_cfg3"] = {"cmd": "python bench.py --gpus 1 --steps 50 --warmup 5", "parent_tree": bench_lines(a.bench_before),
                         "this_tree": bench_lines(a.bench_after)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1); f.write("\n")
    print(json.dumps(res))
    cam_dev.close(); scr_dev.close()


if __name__ == "__main__":
    main()
