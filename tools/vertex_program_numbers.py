#!/usr/bin/env python3
"""What a user vertex program costs on cfg3 (4096^2, 1 M triangles): the DUST2 fragment restatement over the built-in vertex stage
(k_vertex) against the same fragment text with the restated Renderer.VertexShader (k_vertex_user + the module's k_setup).

Both variants run in ONE process on one card, interleaved round by round, so that whatever else the machine does falls on both; the
baseline's own run-to-run spread (max - min over the rounds) is the yardstick for the difference.  Per variant and round:
  vertex_ms            swr_profile.vertex_ms per flush, one stream (swr_set_pipelining(0)), event pairs around every stage
  frame_ms_one_stream  wall clock per frame, one stream, no events
  frame_ms_pipelined   wall clock per frame, frames in flight (swr_set_pipelining(1)), no events
and once: the first-compile time of the pair against the fragment-only program (cold: empty in-process cache, the code-object
manager's disk cache off) and the vertex kernel's resources from the code object's metadata.
usage: vertex_program_numbers.py [frames=60] [rounds=5] > profiles/<name>.json"""
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
os.environ["AMD_COMGR_CACHE"] = "0"
from softwarerenderer_amd import Device, scenes      # noqa: E402
from test_gpu_custom_program import DUST2            # noqa: E402
from vertex_program_texts import RENDERER_VS         # noqa: E402

FRAMES = int(sys.argv[1]) if len(sys.argv) > 1 else 60
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 5


def kernel_resources(path):
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "--notes", path], capture_output=True, text=True).stdout
    res = []
    for block in out.split("- .agpr_count")[1:]:
        def field(name):
            m = re.search(r"^    \." + name + r":\s+(\S+)", block, re.M)
            return m.group(1) if m else None
        res.append({"name": field("name"), "vgpr_count": int(field("vgpr_count")), "sgpr_count": int(field("sgpr_count")),
                    "lds_bytes": int(field("group_segment_fixed_size")), "scratch_bytes": int(field("private_segment_fixed_size"))})
    return [r for r in res if any(k in r["name"] for k in ("k_raster_c", "k_vertex_user", "k_setup"))]


def compiled(dev, fs, vs=None):
    before = set(glob.glob(os.path.join(DUMP, "*.co")))
    t0 = time.perf_counter()
    pid = dev.compile_program(fs, vertex_source=vs)
    secs = time.perf_counter() - t0
    new = sorted(set(glob.glob(os.path.join(DUMP, "*.co"))) - before)
    return pid, round(secs, 3), kernel_resources(new[0]) if new else None


def frames(dev, r, n):
    for _ in range(n):
        r.submit_frame(); dev.flush()
    dev.sync()


def measure(dev, r):
    out = {}
    dev.set_pipelining(0)
    frames(dev, r, 10)
    dev.profile_reset(); dev.profile_enable(1)
    frames(dev, r, FRAMES)
    p = dev.profile()
    dev.profile_enable(0)
    n = max(p["raster_launches"], 1)            # one batch per frame (the profile's `flushes` counts from swr_reset_stats)
    out["vertex_ms"] = p["vertex_ms"] / n
    out["setup_ms"] = p["setup_ms"] / n
    for key, mode in (("frame_ms_one_stream", 0), ("frame_ms_pipelined", 1)):
        dev.set_pipelining(mode)
        frames(dev, r, 20)
        t0 = time.perf_counter()
        frames(dev, r, FRAMES)
        out[key] = 1e3 * (time.perf_counter() - t0) / FRAMES
    return out


dev = Device(0)
f_only, compile_f_s, _ = compiled(dev, DUST2)
pair, compile_vf_s, kernels = compiled(dev, DUST2, RENDERER_VS)
scene = scenes.cfg3()
variants = {"fragment_only_builtin_vertex_stage": f_only, "restated_vertex_shader": pair}
renderers = {k: scenes.SceneRenderer(dev, dataclasses.replace(scene, draws=[dataclasses.replace(d, program=pid) for d in scene.draws]))
             for k, pid in variants.items()}
samples = {k: [] for k in variants}
for rnd in range(ROUNDS):
    order = list(variants) if rnd % 2 == 0 else list(variants)[::-1]        # A B, B A, A B, ...
    for k in order:
        samples[k].append(measure(dev, renderers[k]))
dev.set_pipelining(1)

res = {}
for k, rows in samples.items():
    res[k] = {}
    for key in ("vertex_ms", "setup_ms", "frame_ms_one_stream", "frame_ms_pipelined"):
        vals = sorted(r[key] for r in rows)
        res[k][key] = {"median": round(vals[len(vals) // 2], 4), "min": round(vals[0], 4), "max": round(vals[-1], 4),
                       "rounds": [round(r[key], 4) for r in rows]}
base, user = res["fragment_only_builtin_vertex_stage"], res["restated_vertex_shader"]
cmp_ = {}
for key in ("vertex_ms", "setup_ms", "frame_ms_one_stream", "frame_ms_pipelined"):
    spread = base[key]["max"] - base[key]["min"]
    diff = user[key]["median"] - base[key]["median"]
    cmp_[key] = {"baseline_spread_ms": round(spread, 4), "difference_of_medians_ms": round(diff, 4),
                 "within_baseline_spread": bool(abs(diff) <= spread)}
print(json.dumps({
    "config": "cfg3 4096x4096, 1,000,000 triangles, Back/LessEqual/Alpha", "device": dev.name, "frames_per_window": FRAMES, "rounds": ROUNDS,
    "method": "one process, variants interleaved (A B, B A, ...); spread = max - min of the baseline over the rounds",
    **res, "comparison": cmp_,
    "first_compile_s": {"fragment_only": compile_f_s, "vertex_and_fragment": compile_vf_s},
    "kernels_of_the_pair": kernels,
}, indent=1))
for r in renderers.values():
    r.close()
dev.close()
