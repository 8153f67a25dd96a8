#!/usr/bin/env python3
"""User fragment programs on cfg3 (4096^2, 1 M triangles): the DUST2 restatement of tests/test_gpu_custom_program.py against the
built-in SWR_PROG_DUST2_LAMBERT_FOG -- wall-clock frame time (frames in flight, as tools/ab/frames.py measures it), raster-kernel time
(hipEvent pairs around the raster kernel only, one stream), the first compile time (empty in-process cache, the compiler's own cache
off) and the compiled kernels' registers (from the code object's metadata) -- beside those of a program that reads one varying, which
shows the interpolation of unread varyings compiled away.  usage: custom_program_numbers.py [frames] > profiles/<name>.json"""
import dataclasses
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DUMP = tempfile.mkdtemp(prefix="swr_prog_")
os.environ["SWR_PROGRAM_DUMP_DIR"] = DUMP
os.environ["AMD_COMGR_CACHE"] = "0"                 # a cold compile: no on-disk cache of the code-object manager
import numpy as np                                   # noqa: E402
from softwarerenderer_amd import Device, scenes      # noqa: E402
from test_gpu_custom_program import DUST2, VERTEX_COLOUR     # noqa: E402

FRAMES = int(sys.argv[1]) if len(sys.argv) > 1 else 100


def frame_ms(dev, scene, pipelining):
    dev.set_pipelining(pipelining)
    r = scenes.SceneRenderer(dev, scene)
    for _ in range(20):
        r.submit_frame(); dev.flush()
    dev.sync()
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(FRAMES):
            r.submit_frame(); dev.flush()
        dev.sync()
        best = min(best, 1e3 * (time.perf_counter() - t0) / FRAMES)
    r.close()
    return round(best, 4)


def raster_ms(dev, scene):
    """median raster-kernel time on one stream (pipelining 0: what kernel timings are quoted on)"""
    dev.set_pipelining(0)
    r = scenes.SceneRenderer(dev, scene)
    for _ in range(10):
        r.submit_frame(); dev.flush()
    dev.sync()
    dev.profile_reset(); dev.profile_enable(2)
    for _ in range(FRAMES):
        r.submit_frame(); dev.flush()
    dev.sync()
    ms = float(np.median(dev.raster_samples()))
    dev.profile_enable(0)
    r.close()
    return round(ms, 4)


def kernel_resources(path):
    """vgpr / sgpr counts, LDS and scratch of the two k_raster_c kernels of a code object (AMDGPU metadata note)."""
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "--notes", path], capture_output=True, text=True).stdout
    res = []
    for block in out.split("- .agpr_count")[1:]:
        def field(name):
            m = re.search(r"^    \." + name + r":\s+(\S+)", block, re.M)
            return m.group(1) if m else None
        res.append({"name": field("name"), "vgpr_count": int(field("vgpr_count")), "sgpr_count": int(field("sgpr_count")),
                    "lds_bytes": int(field("group_segment_fixed_size")), "scratch_bytes": int(field("private_segment_fixed_size"))})
    return [r for r in res if "k_raster_c" in r["name"]]


def compiled(dev, src):
    before = set(glob.glob(os.path.join(DUMP, "*.co")))
    t0 = time.perf_counter()
    pid = dev.compile_program(src)
    secs = time.perf_counter() - t0
    new = sorted(set(glob.glob(os.path.join(DUMP, "*.co"))) - before)
    return pid, round(secs, 3), kernel_resources(new[0]) if new else None


dev = Device(0)
pid, compile_s, kernels = compiled(dev, DUST2)
_, compile2_s, kernels_colour = compiled(dev, VERTEX_COLOUR)
scene = scenes.cfg3()
user = dataclasses.replace(scene, draws=[dataclasses.replace(d, program=pid) for d in scene.draws])
res = {"builtin_dust2": {}, "custom_dust2_restatement": {}}
for key, sc in (("builtin_dust2", scene), ("custom_dust2_restatement", user)):
    res[key]["frame_ms_pipelined"] = frame_ms(dev, sc, 1)
    res[key]["frame_ms_one_stream"] = frame_ms(dev, sc, 0)
    res[key]["raster_ms_median_one_stream"] = raster_ms(dev, sc)
dev.set_pipelining(1)
b, u = res["builtin_dust2"], res["custom_dust2_restatement"]
print(json.dumps({
    "config": "cfg3 4096x4096, 1,000,000 triangles, Back/LessEqual/Alpha", "device": dev.name, "frames": FRAMES, **res,
    "ratio_frame_pipelined": round(u["frame_ms_pipelined"] / b["frame_ms_pipelined"], 3),
    "ratio_frame_one_stream": round(u["frame_ms_one_stream"] / b["frame_ms_one_stream"], 3),
    "ratio_raster": round(u["raster_ms_median_one_stream"] / b["raster_ms_median_one_stream"], 3),
    "first_compile_s": compile_s, "second_program_compile_s": compile2_s,
    "kernels_dust2_restatement": kernels, "kernels_vertex_colour_program": kernels_colour,
}, indent=1))
dev.close()
