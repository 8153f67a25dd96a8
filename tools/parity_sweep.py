#!/usr/bin/env python3
"""Extended parity sweep (test infrastructure, not part of the suite): random scenes of the four generator families at random
sizes / states, HIP path against the oracle (depth bit-exact, colour <= 1 ULP, identical counters), for SECONDS of wall time.
--edges adds the adversarial families of tests/edge_scenes.py (scenes at the binning / hi-Z / walk / guard bounds) and of
tests/shade_edge_scenes.py (scenes at the guards of the speculate-and-verify shaders) and of tests/geometry_edge_scenes.py (scenes
at the branches of the near clipper, the fan and the setup discards): a random family and seed every fifth round.
usage: parity_sweep.py [--edges] [SECONDS=420] [RNG_SEED=7]"""
import sys, time
import os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import test_gpu_parity as T
from softwarerenderer_amd import Device, scenes
from softwarerenderer_amd.rasterizer import DepthTest, Program, BlendMode, CullMode
EDGES = "--edges" in sys.argv
if EDGES:
    sys.argv.remove("--edges")
    import edge_scenes, shade_edge_scenes, geometry_edge_scenes
    EDGE_FAMILIES = {**edge_scenes.FAMILIES, **shade_edge_scenes.FAMILIES, **geometry_edge_scenes.FAMILIES}
dev = Device(0)
SECONDS = float(sys.argv[1]) if len(sys.argv) > 1 else 420.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 7)
bad = n = 0; t0 = time.time()
while time.time() - t0 < SECONDS:
    kind = n % 5 if EDGES else n % 4
    seed = int(rng.integers(1, 1 << 30))
    if kind == 4:
        fam = list(EDGE_FAMILIES)[int(rng.integers(0, len(EDGE_FAMILIES)))]
        for s in EDGE_FAMILIES[fam](seed % 100000):
            try:
                T.run_both(dev, s)
            except AssertionError as e:
                bad += 1; print("MISMATCH", fam, seed % 100000, s.name, str(e)[:300], flush=True)
        n += 1
        continue
    W, H = int(rng.integers(100, 900)), int(rng.integers(100, 700))
    if kind == 0:
        s = scenes.cfg2(W, H, int(rng.integers(200, 6000)), seed=seed, min_area=float(rng.uniform(1, 50)), max_area=float(rng.uniform(100, 60000)))
    elif kind == 1:
        s = scenes.cfg3(W, H, (int(rng.integers(1, 5)), int(rng.integers(1, 5))), (int(rng.integers(4, 60)), int(rng.integers(4, 40))), tex_size=int(rng.integers(8, 300)), seed=seed,
                        program=[Program.Dust2LambertFog, Program.Phong4Point, Program.Gouraud][n % 3])
    elif kind == 2:
        s = scenes.near_clip_scene(W, H, int(rng.integers(50, 1500)), seed=seed)
    else:
        s = scenes.state_scene(W, H, int(rng.integers(100, 3000)), seed=seed, cull=list(CullMode)[n % 3], depth_test=list(DepthTest)[n % 8], blend=list(BlendMode)[n % 4])
    try:
        T.run_both(dev, s)
    except AssertionError as e:
        bad += 1; print("MISMATCH", kind, seed, W, H, str(e)[:300], flush=True)
    n += 1
    if n % 50 == 0: print("progress", n, round(time.time() - t0), flush=True)
print("scenes", n, "mismatches", bad)
