#!/usr/bin/env python3
"""Cost of the texture slots of user programs on cfg3 (4096^2, 1 M triangles), one JSON file (default
profiles/r17_program_textures.json).
  (a) NO SLOT USED, against the parent commit: the DUST2 restatement of tests/test_gpu_custom_program.py -- a program that calls no
      slot helper -- under this tree's library and under the parent commit's (--parent-tree DIR: a built checkout of the parent
      commit; its package cannot load this tree's library or the other way round, the entry points differ).  One child process per
      run, the same code in each, in the order parent, this, parent on one GPU.  Raster kernel time (median over hipEvent pairs, one
      stream) and frame time (wall clock, frames in flight), the kernels' registers from the code objects' metadata.  The spread of
      the parent's two runs is the margin: `within_parent_spread` says whether this library's figure lies no further from the mean
      of the parent's two than they lie from each other.
  (b) SLOTS USED, this library only: LIGHTMAP (tests/program_texture_cases.py: diffuse times a 1024^2 lightmap in slot 1, nearest and
      bilinear) beside DIFFUSE, the same program without the lightmap.  A cost to report, not a threshold.
--registers-only needs no GPU: it compiles the texts (swr_program_validate) and reads the code objects.
usage: python tools/program_texture_rate.py [--out FILE] [--frames N] [--parent-tree DIR] [--registers-only]"""
import argparse
import ctypes
import dataclasses
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (a child of (a) imports the package and the DUST2 text of the tree it measures)
TREE = os.path.abspath(sys.argv[sys.argv.index("--child-no-slot") + 1]) if "--child-no-slot" in sys.argv else ROOT
sys.path.insert(0, TREE); sys.path.insert(0, os.path.join(TREE, "tests"))
os.environ["AMD_COMGR_CACHE"] = "0"

from softwarerenderer_amd import Device, Texture, _native, scenes          # noqa: E402
from test_gpu_custom_program import DUST2                                  # noqa: E402

HEAD = "__device__ float4 swr_fragment(const swr_fs_in& in, const swr_fs_env& env) {\n"
# the porting guide's example (tests/program_texture_cases.py holds the same text) and the program without the lightmap
LIGHTMAP = HEAD + """    const float4 d = swr_sample(env, in.tex_coord), l = swr_sample(env, 1, in.tex_coord);
    return make_float4(in.color.x * d.x * l.x, in.color.y * d.y * l.y, in.color.z * d.z * l.z, in.color.w * d.w);
}
"""
DIFFUSE = HEAD + """    const float4 d = swr_sample(env, in.tex_coord);
    return make_float4(in.color.x * d.x, in.color.y * d.y, in.color.z * d.z, in.color.w * d.w);
}
"""


def kernel_resources(path):
    """registers, LDS and scratch of the k_raster_c kernels of a code object (AMDGPU metadata note)"""
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "--notes", path], capture_output=True, text=True).stdout
    res = []
    for block in out.split("- .agpr_count")[1:]:
        def field(name):
            m = re.search(r"^    \." + name + r":\s+(\S+)", block, re.M)
            return m.group(1) if m else None
        res.append({"name": field("name"), "vgpr_count": int(field("vgpr_count")), "sgpr_count": int(field("sgpr_count")),
                    "lds_bytes": int(field("group_segment_fixed_size")), "scratch_bytes": int(field("private_segment_fixed_size"))})
    return [r for r in res if "k_raster_c" in r["name"]]


def registers(src):
    """The raster kernels of `src` as the tree's library compiles them; no device is touched."""
    dump = tempfile.mkdtemp(prefix="swr_prog_")
    os.environ["SWR_PROGRAM_DUMP_DIR"] = dump
    lib = _native.load()
    log = ctypes.create_string_buffer(1 << 16)
    rc = lib.swr_program_validate(src.encode(), log, len(log))
    os.environ.pop("SWR_PROGRAM_DUMP_DIR")
    if rc:
        raise RuntimeError(log.value.decode(errors="replace"))
    return kernel_resources(glob.glob(os.path.join(dump, "*.co"))[0])


def frame_ms(dev, scene, frames):
    dev.set_pipelining(1)
    r = scenes.SceneRenderer(dev, scene)
    for _ in range(20):
        r.submit_frame(); dev.flush()
    dev.sync()
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(frames):
            r.submit_frame(); dev.flush()
        dev.sync()
        best = min(best, 1e3 * (time.perf_counter() - t0) / frames)
    r.close()
    return round(best, 4)


def raster_ms(dev, scene, frames):
    dev.set_pipelining(0)
    r = scenes.SceneRenderer(dev, scene)
    for _ in range(10):
        r.submit_frame(); dev.flush()
    dev.sync()
    dev.profile_reset(); dev.profile_enable(2)
    for _ in range(frames):
        r.submit_frame(); dev.flush()
    dev.sync()
    ms = float(np.median(dev.raster_samples()))
    dev.profile_enable(0)
    dev.set_pipelining(1)
    r.close()
    return round(ms, 4)


def measure(dev, scene, pid, frames):
    user = dataclasses.replace(scene, draws=[dataclasses.replace(d, program=pid) for d in scene.draws])
    return {"raster_ms_median_one_stream": raster_ms(dev, user, frames), "frame_ms_pipelined": frame_ms(dev, user, frames)}


def child_no_slot(frames, with_gpu):
    """(a), one run, in a process of its own: prints one JSON line."""
    res = {"kernels": registers(DUST2)}
    if with_gpu:
        dev = Device(0)
        pid = dev.compile_program(DUST2)
        res.update(measure(dev, scenes.cfg3(), pid, frames), swr_build_info=dev.build_info())
        dev.destroy_program(pid)
        dev.close()
    print(json.dumps(res))


def no_slot_run(tree, frames, with_gpu):
    cmd = [sys.executable, os.path.abspath(__file__), "--child-no-slot", tree, "--frames", str(frames)] + ([] if with_gpu else ["--registers-only"])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if out.returncode:
        raise RuntimeError(f"the run in {tree} ended with {out.returncode}: {out.stderr[-2000:]}")
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def within(this, parents):
    spread = max(parents) - min(parents)
    return {"this": this, "parent_runs": parents, "parent_spread": round(spread, 4),
            "this_minus_parent_mean": round(this - sum(parents) / len(parents), 4),
            "within_parent_spread": abs(this - sum(parents) / len(parents)) <= spread,
            "slower_than_both_parent_runs": this > max(parents)}


def slots_used(scene, frames):
    dev = Device(0)
    lightmap = np.random.default_rng(5).integers(0, 256, (1024, 1024, 4), dtype=np.uint8)
    out = {}
    single = dev.compile_program(DIFFUSE)
    out["DIFFUSE (slot 0 alone)"] = measure(dev, scene, single, frames)
    pid = dev.compile_program(LIGHTMAP)
    for name, bilinear in (("LIGHTMAP, 1024^2 in slot 1, nearest", False), ("LIGHTMAP, 1024^2 in slot 1, bilinear (block-linear copy)", True)):
        t = Texture(dev, lightmap)
        t.SetBilinear(bilinear)
        dev.set_program_texture(pid, 1, t)
        out[name] = measure(dev, scene, pid, frames)
        t.Dispose()
    out["LIGHTMAP, slot 1 unbound"] = measure(dev, scene, pid, frames)
    base = out["DIFFUSE (slot 0 alone)"]
    for name, rec in out.items():
        rec["raster_over_diffuse"] = round(rec["raster_ms_median_one_stream"] / base["raster_ms_median_one_stream"], 3)
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_program_textures.json"))
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--registers-only", action="store_true")
    ap.add_argument("--child-no-slot", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    gpu = not a.registers_only
    if a.child_no_slot:
        return child_no_slot(a.frames, gpu)
    res = {"what": "texture slots of user programs on cfg3 (tools/program_texture_rate.py): (a) a program that calls no slot helper under this "
                   "library and the parent commit's, one process per run in the order parent / this / parent; (b) diffuse times a lightmap "
                   "in slot 1 beside the single-texture program", "config": "cfg3 4096x4096, 1,000,000 triangles, Back/LessEqual/Alpha",
           "frames": a.frames}
    trees = [a.parent_tree, ROOT, a.parent_tree] if a.parent_tree else [ROOT]
    runs = [dict(no_slot_run(t, a.frames, gpu), commit="this" if t == ROOT else "parent") for t in trees]
    res["no_slot_used"] = {"program": "the DUST2 restatement (tests/test_gpu_custom_program.py)", "runs_in_order": runs}
    if gpu and a.parent_tree:
        for key in ("raster_ms_median_one_stream", "frame_ms_pipelined"):
            res["no_slot_used"][key] = within(runs[1][key], [runs[0][key], runs[2][key]])
    res["registers_slots_used"] = {"diffuse": registers(DIFFUSE), "lightmap": registers(LIGHTMAP)}
    if gpu:
        res["slots_used"] = slots_used(scenes.cfg3(), a.frames)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1); f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
