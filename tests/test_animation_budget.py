"""The skeletal-animation kernels run on the front stream beside a raster kernel (csrc/swr_animation.hip.h), so they are held to the
front end's co-residency budget of csrc/swr_device.h in what the compiler actually allocated: at most SWR_FRONT_MAX_LDS bytes of LDS
(they use none), SWR_FRONT_MAX_VGPRS registers, four waves a block, no scratch.  Read as tests/test_resource_budget.py reads the
compiler's resource remarks (its helpers, unchanged)."""
import os
import re

from test_resource_budget import CSRC, _alloc, _defines, usage      # noqa: F401  (usage: the module-scoped fixture that compiles)

KERNELS = ("swr::k_pose_sample", "swr::k_mesh_skin_batch")


def test_the_animation_kernels_fit_the_slot_of_a_retiring_raster_wave(usage):      # noqa: F811
    d = _defines()
    for k in KERNELS:
        assert k in usage, f"{k} is not in the library"
        v = usage[k]
        assert v["LDS"] == 0 <= d["SWR_FRONT_MAX_LDS"], (k, v)
        assert v["ScratchSize"] == 0, (k, v)
        assert _alloc(v["VGPRs"] + v["AGPRs"]) <= d["SWR_FRONT_MAX_VGPRS"], (k, v)
    # the kernels they must equal or sit beside are still there, within the same budget
    assert _alloc(usage["swr::k_mesh_skin"]["VGPRs"]) <= d["SWR_FRONT_MAX_VGPRS"]


def test_their_blocks_hold_at_most_four_waves_and_raise_their_priority_first():
    txt = open(os.path.join(CSRC, "swr_animation.hip.h")).read()
    deform = open(os.path.join(CSRC, "swr_mesh_deform.hip.h")).read()
    pose_block = int(re.search(r"#define SWR_POSE_BLOCK (\d+)\b", txt).group(1))
    deform_block = int(re.search(r"#define SWR_DEFORM_BLOCK (\d+)\b", deform).group(1))
    assert pose_block <= 256 and deform_block <= 256 and pose_block % 64 == 0 and deform_block % 64 == 0
    assert "__launch_bounds__(SWR_POSE_BLOCK) void k_pose_sample" in txt and "__launch_bounds__(SWR_DEFORM_BLOCK) void k_mesh_skin_batch" in txt
    for name in ("k_pose_sample", "k_mesh_skin_batch"):
        body = txt[txt.index(f"void {name}("):]
        first = body[body.index("{") + 1:].strip().splitlines()[0].strip()
        assert first == "SWR_FRONT_ENTER();", (name, first)
    assert "__shared__" not in txt
