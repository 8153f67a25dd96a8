"""Which k_raster_c instantiation a batch gets: the library's own choice (csrc/swr_raster_select.h, a pure function that the flush
path calls) against tests/shade_edge_scenes.py::predicted_kernel, the Python restatement that test_shade_edges_host.py and
test_gpu_shade_edges.py rely on.  The header has no HIP types, so a few-line driver around it is built with the host compiler and
fed EVERY batch of one draw and of two draws over the built-in programs x blend modes x {Less, LessEqual, Always}
(DEBUG_VARYINGS only with itself, as record_draw guarantees; no wireframe, no user program).  No GPU."""
import itertools
import os
import shutil
import subprocess
import types

import pytest

import shade_edge_scenes as S
from softwarerenderer_amd.rasterizer import BlendMode, DepthTest, Program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include "swr_raster_select.h"
int main() {            // per line: n, then n x (program, blend, depth test) -> the kernel's name and depth_only_grows
    int n;
    while (scanf("%d", &n) == 1) {
        swr::RasterTraits t;
        for (int i = 0; i < n; ++i) {
            int p, b, d;
            if (scanf("%d %d %d", &p, &b, &d) != 3) return 1;
            t.add(p, b, d);
        }
        printf("%s %d\n", swr::raster_kernel_name(swr::select_raster_kernel(t)), t.depth_only_grows ? 1 : 0);
    }
    return 0;
}
"""

PROGRAMS = (Program.FlatColor, Program.Gouraud, Program.Dust2LambertFog, Program.Phong4Point, Program.DebugVaryings)
DEPTH_TESTS = (DepthTest.Less, DepthTest.LessEqual, DepthTest.Always)


def _batches():
    kinds = [types.SimpleNamespace(program=p, blend=b, depth_test=d) for p in PROGRAMS for b in BlendMode for d in DEPTH_TESTS]
    debug = [k for k in kinds if k.program == Program.DebugVaryings]
    other = [k for k in kinds if k.program != Program.DebugVaryings]
    return [[k] for k in kinds] + [list(pair) for group in (other, debug) for pair in itertools.product(group, repeat=2)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    out = tmp_path_factory.mktemp("select")
    src, exe = str(out / "driver.cpp"), str(out / "driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "softwarerenderer_amd", "csrc"), src, "-o", exe], check=True, capture_output=True)
    return exe


def test_the_library_selects_what_predicted_kernel_says(driver):
    batches = _batches()
    assert len(batches) == 60 + 48 * 48 + 12 * 12
    text = "".join(f"{len(b)} " + " ".join(f"{int(d.program)} {int(d.blend)} {int(d.depth_test)}" for d in b) + "\n" for b in batches)
    lines = subprocess.run([driver], input=text, check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    assert len(lines) == len(batches)
    for b, line in zip(batches, lines):
        name, grows = line.split()
        what = [(d.program.name, d.blend.name, d.depth_test.name) for d in b]
        # (the library tells DEBUG_VARYINGS batches with a BlendMode.None draw apart, the restatement does not)
        assert name.replace("debug_varyings_none", "debug_varyings") == S.predicted_kernel(types.SimpleNamespace(draws=b)), what
        assert int(grows) == all(d.depth_test in (DepthTest.Less, DepthTest.LessEqual) for d in b), what
