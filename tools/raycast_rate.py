#!/usr/bin/env python3
"""Wall time of swr_raycast_nearest on dust2: median of 200 calls after 20 warm-ups of
  (a) 111 rays x the 11 dust2 meshes   one slide attempt of CharacterController.MoveWithSlide (3 x 37 rays)
  (b) 1 ray x one 1-triangle mesh      the round-trip floor: an upload, two launches, a copy and a wait
  (c) 4,096 rays x the 11 meshes
Prints one JSON line.  usage: python tools/raycast_rate.py [--calls 200] [--warmup 20]"""
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

from softwarerenderer_amd import Device, Mesh, hostmath as hm          # noqa: E402
from softwarerenderer_amd.modelloader import Model                      # noqa: E402
from softwarerenderer_amd.rasterizer import RAY_DTYPE, RAY_HIT_DTYPE, Physics      # noqa: E402


def slide_rays(n, meshes, seed=5):
    """n rays laid out as MoveWithSlide's: rings of 37 origins of radius 0.3 at three heights around a position inside the map, all
    along one move direction."""
    allp = np.concatenate([m.Vertices["position"] for m in meshes]).astype(np.float64)
    med, ext = np.median(allp, axis=0), allp.max(axis=0) - allp.min(axis=0)
    rng = np.random.default_rng(seed)
    rays = np.zeros(n, dtype=RAY_DTYPE)
    k = 0
    while k < n:
        pos = med + rng.uniform(-0.3, 0.3, 3) * ext
        ang = rng.uniform(0, 2 * np.pi)
        move = (np.cos(ang), rng.uniform(-0.2, 0.2), np.sin(ang))
        for v in range(3):
            for h in range(37):
                if k == n:
                    break
                a = 2 * np.pi * h / 37
                rays[k]["origin"] = pos + np.array([0.3 * np.cos(a), -0.5 + 0.5 * v, 0.3 * np.sin(a)])
                rays[k]["direction"] = move
                k += 1
    return rays


def timed(dev, rays, targets, calls, warmup):
    arr, kept, _ = Physics._targets(targets)
    out = np.zeros(rays.shape[0], dtype=RAY_HIT_DTYPE)
    fn, ctx = dev._lib.swr_raycast_nearest, dev._ctx
    args = (ctx, rays.ctypes.data, int(rays.shape[0]), C.addressof(arr), len(kept), 1, out.ctypes.data)
    ts = []
    for i in range(warmup + calls):
        t0 = time.perf_counter()
        rc = fn(*args)
        t1 = time.perf_counter()
        if rc:
            dev._ck(rc)
        if i >= warmup:
            ts.append((t1 - t0) * 1e6)
    return {"median_us": round(statistics.median(ts), 2), "min_us": round(min(ts), 2), "p90_us": round(sorted(ts)[int(0.9 * len(ts))], 2),
            "rays": int(rays.shape[0]), "targets": len(kept), "hits": int(out["found"].sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    dev = Device(0)
    model = Model().LoadModel(os.path.join(ROOT, "tests", "golden", "models", "dust2", "scene.gltf"))
    I = hm.identity()
    targets = [(m.Upload(dev), I, I) for m in model.Meshes]
    tris = sum(int(np.asarray(m.Indices).size) // 3 for m in model.Meshes)
    one = np.zeros(3, dtype=model.Meshes[0].Vertices.dtype)
    one["position"] = [(0, 0, 0), (1, 0, 0), (0, 1, 0)]
    one["normal"] = (0, 0, 1)
    floor_mesh = Mesh(dev, one, np.arange(3, dtype=np.uint16))
    floor_ray = np.zeros(1, dtype=RAY_DTYPE)
    floor_ray["origin"], floor_ray["direction"] = (.25, .25, 1), (0, 0, -1)
    res = {"device": dev.name, "build": dev.build_info(), "triangles": tris, "calls": a.calls, "warmup": a.warmup,
           "a_111_rays_x_11_meshes": timed(dev, slide_rays(111, model.Meshes), targets, a.calls, a.warmup),
           "b_1_ray_x_1_triangle": timed(dev, floor_ray, [(floor_mesh, I, I)], a.calls, a.warmup),
           "c_4096_rays_x_11_meshes": timed(dev, slide_rays(4096, model.Meshes), targets, a.calls, a.warmup)}
    print(json.dumps(res))
    dev.close()


if __name__ == "__main__":
    main()
