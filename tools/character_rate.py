#!/usr/bin/env python3
"""Wall time of swr_character_update on dust2 for n = 1, 64, 1024 controllers: median, min and p90 of `--calls`
calls after `--warmup` warm-ups, every call from the same input state (grounded controllers 0.25 above the floor around one spot of
the map, 6 m/s in directions of their own, default properties: 18 + 36 rays per cast).

In the same process it measures what the call replaces at the interface the library had before it: one swr_raycast_nearest per
executed phase.  The phases are read from the trace of the timed call -- the two CheckPlanes (18 rays a controller, one query), then
attempt a of chain c for the controllers whose trace says they ran it (36 rays each) -- and for each phase the median time of
swr_raycast_nearest with that many rays against the same 11 meshes is taken; `replaced_sum_us` is their sum.  The host arithmetic
between the queries, which the one call also moves to the device, is not counted on either side.
Prints one JSON line.  usage: python tools/character_rate.py [--calls 200] [--warmup 20]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from softwarerenderer_amd import CharacterController, Device, hostmath as hm          # noqa: E402
from softwarerenderer_amd.modelloader import Model                                     # noqa: E402
from softwarerenderer_amd.rasterizer import CHARACTER_DTYPE, CHARACTER_INPUT_DTYPE, CHARACTER_TRACE_DTYPE, Physics     # noqa: E402
from raycast_rate import slide_rays, timed                                              # noqa: E402


def start_states(n, meshes, seed=9):
    allp = np.concatenate([m.Vertices["position"] for m in meshes]).astype(np.float64)
    med, ext = np.median(allp, axis=0), allp.max(axis=0) - allp.min(axis=0)
    rng = np.random.default_rng(5)
    spots = []
    for _ in range(3):
        spots.append(med + rng.uniform(-0.3, 0.3, 3) * ext)
        rng.uniform(0, 2 * np.pi); rng.uniform(-0.2, 0.2)
    spot = spots[2]                                  # a spot with a floor at y = 0 under it and walls 1.5 to 3.5 away
    rng = np.random.default_rng(seed)
    s = np.zeros(n, dtype=CHARACTER_DTYPE)
    i = np.zeros(n, dtype=CHARACTER_INPUT_DTYPE)
    ang = rng.uniform(0, 2 * np.pi, n)
    d = np.stack([np.cos(ang), np.zeros(n), np.sin(ang)], axis=1)
    s["position"] = np.array([spot[0], 0.25, spot[2]]) + d * rng.uniform(0.0, 1.4, n)[:, None]
    s["velocity"], s["grounded"], s["actual_step_size"] = 6.0 * d, 1, 0.3
    i["move"] = d
    return s, i


def measure(dev, model, targets, n, calls, warmup, dt=1.0 / 60.0):
    cc = CharacterController((0, 0, 0), [], [])
    params = cc.Params()
    v_steps, h_rays = CharacterController.RayCounts(params)
    ring = CharacterController.Ring(h_rays)
    states, inputs = start_states(n, model.Meshes)
    arr, kept, _ = Physics._targets(targets)
    p = params.reshape(1)
    cur, trace, ts = states.copy(), np.zeros(n, dtype=CHARACTER_TRACE_DTYPE), []
    fn = dev._lib.swr_character_update
    args = (dev._ctx, p.ctypes.data, cur.ctypes.data, inputs.ctypes.data, n, dt, ring.ctypes.data, int(ring.shape[0]), C.addressof(arr), len(kept), 0,
            trace.ctypes.data)
    for k in range(warmup + calls):
        np.copyto(cur, states)
        t0 = time.perf_counter()
        rc = fn(*args)
        t1 = time.perf_counter()
        if rc:
            dev._ck(rc)
        if k >= warmup:
            ts.append((t1 - t0) * 1e6)
    per = (v_steps + 1) * h_rays
    phases = [("check_planes", 18 * n)]
    for c in (0, 1):
        for a in range(3):
            ran = int((trace["chain_attempts"][:, c] > a).sum())
            if ran:
                phases.append((f"chain{c + 1}_attempt{a}", per * ran))
    replaced = []
    for name, rays in phases:
        r = timed(dev, slide_rays(rays, model.Meshes), targets, calls, warmup)
        replaced.append({"phase": name, "rays": rays, "median_us": r["median_us"]})
    return {"controllers": n, "rays_per_slide_attempt": per,
            "update": {"median_us": round(statistics.median(ts), 2), "min_us": round(min(ts), 2), "p90_us": round(sorted(ts)[int(0.9 * len(ts))], 2)},
            "grounded": int(trace["ground_found"].sum()), "chain2_attempts": np.bincount(trace["chain_attempts"][:, 1], minlength=4).tolist(),
            "replaced": replaced, "replaced_sum_us": round(sum(r["median_us"] for r in replaced), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    dev = Device(0)
    model = Model().LoadModel(os.path.join(ROOT, "tests", "golden", "models", "dust2", "scene.gltf"))
    I = hm.identity()
    targets = [(m.Upload(dev), I, I) for m in model.Meshes]
    res = {"what": "swr_character_update on dust2 (tools/character_rate.py): wall time per call, and the sum of the swr_raycast_nearest calls "
                   "it replaces (one per executed phase, same process), one MI355X, product build",
           "device": dev.name, "build": dev.build_info(), "calls": a.calls, "warmup": a.warmup,
           "wall_us": [measure(dev, model, targets, n, a.calls, a.warmup) for n in (1, 64, 1024)]}
    print(json.dumps(res))
    dev.close()


if __name__ == "__main__":
    main()
