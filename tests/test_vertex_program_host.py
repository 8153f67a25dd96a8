"""User vertex programs: the run-time compile step alone (swr_program_validate_vf needs neither a context nor a GPU), and what the
compiler allocated for the vertex kernel.

A vertex-program batch runs its own k_vertex_user in the front end, which overlaps the previous frame's raster kernel only inside the
slot swr_device.h describes (SWR_FRONT_MAX_LDS / SWR_FRONT_MAX_VGPRS, no scratch): checked in the code object's metadata, as
tests/test_resource_budget.py checks the library's own kernels in the compiler's remarks."""
import ctypes
import glob
import os
import re
import subprocess
import sys

import pytest

from softwarerenderer_amd import _native as N
from test_custom_program_host import DUST2
from vertex_program_texts import DISPLACE_VS, RENDERER_VS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/llvm/bin/llvm-readelf"


@pytest.fixture(scope="module")
def lib():
    return N.load()


def validate_vf(lib, vs, fs):
    log = ctypes.create_string_buffer(1 << 16)
    rc = lib.swr_program_validate_vf(vs.encode() if vs is not None else None, fs.encode(), log, len(log))
    return rc, log.value.decode(errors="replace")


def test_validate_accepts_the_restated_renderer_vertex_shader(lib):
    rc, log = validate_vf(lib, RENDERER_VS, DUST2)
    assert rc == N.SWR_OK, log


def test_a_syntax_error_in_the_vertex_text_names_the_half_and_the_line(lib):
    src = RENDERER_VS.replace("    out.tex_coord = in.uv;", "    out.tex_coord = in.uv\n    out +;")
    line = src.splitlines().index("    out +;") + 1
    rc, log = validate_vf(lib, src, DUST2)
    assert rc == N.SWR_ERR_INVALID_ARG
    assert f"vertex.hip:{line - 1}:" in log or f"vertex.hip:{line}:" in log, log
    assert "fragment.hip:" not in log, log
    # ... and one in the fragment text is still counted in the fragment text, behind a vertex half of any length
    bad = DUST2.replace("fog = fog * fog * (3.0f - 2.0f * fog);", "fog = fog * fog * (3.0f - 2.0f * fog)\n    fog +;")
    line = bad.splitlines().index("    fog +;") + 1
    rc, log = validate_vf(lib, RENDERER_VS, bad)
    assert rc == N.SWR_ERR_INVALID_ARG
    assert f"fragment.hip:{line - 1}:" in log or f"fragment.hip:{line}:" in log, log
    assert "vertex.hip:" not in log, log


def test_a_vertex_text_without_swr_vertex_is_named(lib):
    for src in ("__device__ void shade(const swr_vs_in& in, swr_vs_out& out) { out.color = in.color; }\n",
                "// swr_vertex goes here\n__device__ void shade(const swr_vs_in& in, swr_vs_out& out) { out.color = in.color; }\n"):
        rc, log = validate_vf(lib, src, DUST2)
        assert rc == N.SWR_ERR_INVALID_ARG
        assert "swr_vertex" in log, log


def test_a_null_vertex_source_validates_like_swr_program_validate(lib):
    broken = DUST2.replace("in.world_normal", "in.world_nrmal")
    for src in (DUST2, broken, "this is not C++"):
        a, b = ctypes.create_string_buffer(1 << 16), ctypes.create_string_buffer(1 << 16)
        rc_a = lib.swr_program_validate(src.encode(), a, len(a))
        rc_b = lib.swr_program_validate_vf(None, src.encode(), b, len(b))
        strip = lambda s: re.sub(r"comgr-[0-9a-f-]+", "comgr", s.value.decode(errors="replace"))     # (the compiler's scratch directory)
        assert rc_a == rc_b and strip(a) == strip(b)
    assert lib.swr_program_validate_vf(RENDERER_VS.encode(), None, None, 0) == N.SWR_ERR_INVALID_ARG


def test_vertex_program_entry_points_are_exported(lib):
    for name in ("swr_program_create_vf", "swr_program_validate_vf"):
        assert name in N.EXPORTS and hasattr(lib, name)


def _defines():
    txt = open(os.path.join(ROOT, "softwarerenderer_amd", "csrc", "swr_device.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define (SWR_FRONT_MAX_LDS|SWR_FRONT_MAX_VGPRS|SWR_GEOM_BLOCK) (\d+)", txt)}


def _kernels(path):
    """name -> {vgpr_count, agpr_count, lds, scratch, max_flat_workgroup_size} from the code object's AMDGPU metadata note"""
    out = subprocess.run([READELF, "--notes", path], capture_output=True, text=True, check=True).stdout
    res = {}
    for block in out.split("- .agpr_count")[1:]:
        block = "    .agpr_count" + block

        def field(name):
            return re.search(r"^\s+\." + name + r":\s+(\S+)", block, re.M).group(1)
        res[field("name")] = {"vgpr": int(field("vgpr_count")), "agpr": int(field("agpr_count")),
                              "lds": int(field("group_segment_fixed_size")), "scratch": int(field("private_segment_fixed_size")),
                              "spills": int(field("vgpr_spill_count")), "threads": int(field("max_flat_workgroup_size"))}
    return res


# The dump (SWR_PROGRAM_DUMP_DIR) is written only when a pair of texts is compiled for the first time in a process, so each pair is
# compiled in a process of its own whose environment carries the variable from the start.
_CHILD = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from softwarerenderer_amd import _native as N
from test_custom_program_host import DUST2
import vertex_program_texts as T
log = ctypes.create_string_buffer(1 << 16)
rc = N.load().swr_program_validate_vf(getattr(T, sys.argv[2]).encode(), DUST2.encode(), log, len(log))
sys.exit(0 if rc == 0 else (print(log.value.decode(errors="replace")) or 1))
"""


@pytest.mark.parametrize("vs_name", ["RENDERER_VS", "DISPLACE_VS"])
def test_the_user_vertex_kernel_fits_the_front_end_slot(tmp_path, vs_name):
    assert os.path.exists(READELF)
    env = dict(os.environ, SWR_PROGRAM_DUMP_DIR=str(tmp_path), AMD_COMGR_CACHE="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, vs_name], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    dumps = glob.glob(os.path.join(str(tmp_path), "*.co"))
    assert len(dumps) == 1, dumps
    kernels = _kernels(dumps[0])
    vk = [v for k, v in kernels.items() if "k_vertex_user" in k]
    assert len(vk) == 1, sorted(kernels)
    v, d = vk[0], _defines()
    print(vs_name, v)
    assert v["lds"] <= d["SWR_FRONT_MAX_LDS"], v
    assert (v["vgpr"] + v["agpr"] + 7) // 8 * 8 <= d["SWR_FRONT_MAX_VGPRS"], v          # allocated in granules of 8 on gfx950
    assert v["scratch"] == 0 and v["spills"] == 0, v
    assert v["threads"] == d["SWR_GEOM_BLOCK"] <= 256, v                                # at most four waves
    # the module carries the program's own k_setup and both raster kernels; the library's k_vertex is not compiled into it
    assert any("k_setup" in k for k in kernels) and sum("k_raster_c" in k for k in kernels) == 2
    assert not any(re.search(r"k_vertexE", k) for k in kernels), sorted(kernels)
