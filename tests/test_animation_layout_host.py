"""Where a skeleton's arrays lie in its device blob, how many words a clip's pieces take (csrc/swr_animation_layout.h) and where a
batched texture probe puts its records in the scratch block (probe_layout, csrc/swr_query_layout.h), against the expressions
swr_skeleton_create, swr_pose_set_sample, swr_skeleton_add_clip and the seven probe entry points carried inline before the headers
existed, restated here line by line.  The layouts are observable -- the kernels index the blobs by them, and the 16-byte loads of the
matrices and of the probes' records need their alignment -- so they are held to those values.  The headers have no HIP types, so a
few-line driver around them is built with the host compiler, once plain and once with -fsanitize=address,undefined (a stand-alone
program: nothing loaded into Python is sanitised).  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include "swr_animation_layout.h"
#include "swr_query_layout.h"
int main() {            // per line: S n_nodes n_joints n_levels | T n_nodes | C path n_keys | P n in_bytes out0_bytes out1_bytes
    char kind;
    while (scanf(" %c", &kind) == 1) {
        unsigned long long a, b, c, d;
        if (kind == 'S') {
            if (scanf("%llu %llu %llu", &a, &b, &c) != 3) return 1;
            const swr::SkeletonLayout l = swr::skeleton_layout((size_t)a, (size_t)b, (size_t)c);
            printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", l.rest_local, l.inverse_bind, l.rest_t, l.rest_r, l.rest_s, l.parent, l.order, l.level_start,
                   l.joint_node, l.words);
        } else if (kind == 'T') {
            if (scanf("%llu", &a) != 1) return 1;
            printf("%zu\n", swr::clip_table_words((size_t)a));
        } else if (kind == 'C') {
            if (scanf("%llu %llu", &a, &b) != 2) return 1;
            printf("%zu\n", swr::clip_channel_words((int)a, (size_t)b));
        } else if (kind == 'P') {
            if (scanf("%llu %llu %llu %llu", &a, &b, &c, &d) != 4) return 1;
            const swr::ProbeLayout l = swr::probe_layout((int)a, (size_t)b, (size_t)c, (size_t)d);
            printf("%zu %zu %zu\n", l.off_out[0], l.off_out[1], l.total);
        } else return 1;
    }
    return 0;
}
"""

SKELETON_FIELDS = ("rest_local", "inverse_bind", "rest_t", "rest_r", "rest_s", "parent", "order", "level_start", "joint_node", "words")
SKELETON_SHAPES = [(1, 0, 1), (1, 1, 1), (2, 2, 2), (3, 1, 2), (64, 64, 7), (1024, 1, 1024), (65535, 65535, 1)]
TRANSLATION, ROTATION, SCALE = 0, 1, 2           # SWR_ANIM_PATH_* of include/swr.h
CHANNEL_SHAPES = [(path, n_keys) for path in (TRANSLATION, ROTATION, SCALE) for n_keys in range(1, 34)]
TABLE_NODES = (1, 2, 3, 64, 65535)
PROBE_COUNTS = (1, 2, 3, 4, 5, 255, 256, 257)
# bytes per record: in, first output, second output (0: none)
PROBES = {"sample": (8, 16, 0), "sample_depth": (12, 8, 0), "sample_lod": (12, 16, 0), "lod": (16, 4, 0), "cube_face": (12, 4, 8),
          "sample_cube": (16, 16, 0), "sample_cube_depth": (16, 8, 0)}


def skeleton_expected(n_nodes, n_joints, n_levels):
    """swr_skeleton_create, as it stood"""
    nn, nj = n_nodes, n_joints
    o_local = 0; o_ib = o_local + 16 * nn; o_t = o_ib + 16 * nj; o_r = o_t + 3 * nn; o_s = o_r + 4 * nn; o_parent = o_s + 3 * nn
    o_order = o_parent + nn; o_level = o_order + nn; o_joint = o_level + n_levels + 1; words = o_joint + nj
    return dict(rest_local=o_local, inverse_bind=o_ib, rest_t=o_t, rest_r=o_r, rest_s=o_s, parent=o_parent, order=o_order, level_start=o_level,
                joint_node=o_joint, words=words)


def skeleton_dev_expected(n_nodes, n_joints, n_levels):
    """swr_pose_set_sample's pointer arithmetic over 4-byte words, as it stood"""
    nn, nj = n_nodes, n_joints
    rest_local = 0; inverse_bind = rest_local + 16 * nn; rest_t = inverse_bind + 16 * nj; rest_r = rest_t + 3 * nn; rest_s = rest_r + 4 * nn
    parent = rest_s + 3 * nn; order = parent + nn; level_start = order + nn
    joint_node = level_start + n_levels + 1
    return dict(rest_local=rest_local, inverse_bind=inverse_bind, rest_t=rest_t, rest_r=rest_r, rest_s=rest_s, parent=parent, order=order,
                level_start=level_start, joint_node=joint_node)


def probe_expected(name, n):
    """(offset of the first output, offset of the second or None, bytes the scratch block must hold), as the entry points stood"""
    if name == "sample":
        off_out = (n * 8 + 15) & ~15
        return off_out, None, off_out + n * 16
    if name == "sample_depth":
        off_out = (n * 12 + 15) & ~15
        return off_out, None, off_out + n * 8
    if name == "sample_lod":
        off_out = (n * 12 + 15) & ~15
        return off_out, None, off_out + n * 16
    if name == "lod":
        off_out = n * 16
        return off_out, None, off_out + n * 4
    if name == "cube_face":
        off_face = (n * 12 + 15) & ~15; off_st = off_face + ((n * 4 + 15) & ~15)
        return off_face, off_st, off_st + n * 8
    if name == "sample_cube":
        off_out = n * 16
        return off_out, None, off_out + n * 16
    assert name == "sample_cube_depth"
    off_out = n * 16
    return off_out, None, off_out + n * 8


def _build(tmp_path_factory, name, extra):
    cxx = next((c for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    out = tmp_path_factory.mktemp(name)
    src, exe = str(out / "driver.cpp"), str(out / "driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *extra, "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "softwarerenderer_amd", "csrc"), src, "-o", exe], check=True, capture_output=True)
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory, "animation_layout", [])


@pytest.fixture(scope="module")
def sanitized_driver(tmp_path_factory):
    return _build(tmp_path_factory, "animation_layout_san", ["-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


PROBE_CALLS = [(name, n) for name in PROBES for n in PROBE_COUNTS]


def _run(exe):
    text = "".join(f"S {a} {b} {c}\n" for a, b, c in SKELETON_SHAPES) + "".join(f"T {n}\n" for n in TABLE_NODES) + \
           "".join(f"C {p} {k}\n" for p, k in CHANNEL_SHAPES) + "".join("P %d %d %d %d\n" % ((n,) + PROBES[name]) for name, n in PROBE_CALLS)
    done = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    lines = [list(map(int, ln.split())) for ln in done.stdout.split("\n")[:-1]]
    assert len(lines) == len(SKELETON_SHAPES) + len(TABLE_NODES) + len(CHANNEL_SHAPES) + len(PROBE_CALLS)
    it = iter(lines)
    skeletons = [dict(zip(SKELETON_FIELDS, next(it))) for _ in SKELETON_SHAPES]
    tables = [next(it)[0] for _ in TABLE_NODES]
    channels = [next(it)[0] for _ in CHANNEL_SHAPES]
    probes = [tuple(next(it)) for _ in PROBE_CALLS]
    return skeletons, tables, channels, probes


@pytest.fixture(scope="module")
def layouts(driver):
    return _run(driver)


def test_the_skeleton_layout_is_what_create_and_sample_computed(layouts):
    for shape, got in zip(SKELETON_SHAPES, layouts[0]):
        assert got == skeleton_expected(*shape), shape
        dev = skeleton_dev_expected(*shape)
        assert {k: got[k] for k in dev} == dev, shape
    assert layouts[0][SKELETON_SHAPES.index((2, 2, 2))]["words"] == 32 + 32 + 6 + 8 + 6 + 2 + 2 + 3 + 2


def test_the_blobs_regions_are_in_order_disjoint_and_cover_it(layouts):
    for (nn, nj, nl), l in zip(SKELETON_SHAPES, layouts[0]):
        regions = [("rest_local", 16 * nn), ("inverse_bind", 16 * nj), ("rest_t", 3 * nn), ("rest_r", 4 * nn), ("rest_s", 3 * nn), ("parent", nn),
                   ("order", nn), ("level_start", nl + 1), ("joint_node", nj)]
        end = 0
        for name, size in regions:
            assert l[name] == end, ((nn, nj, nl), name)          # begins where the one before it ends: in order, disjoint, no gap
            end += size
        assert end == l["words"], (nn, nj, nl)
        assert l["rest_local"] % 4 == 0 and l["inverse_bind"] % 4 == 0, (nn, nj, nl)          # float4 loads of the matrices


def test_the_clip_words_are_both_of_the_expressions_add_clip_had(layouts):
    _, tables, channels, _ = layouts
    assert tables == [3 * n for n in TABLE_NODES]
    by = dict(zip(CHANNEL_SHAPES, channels))
    assert (by[(TRANSLATION, 1)], by[(ROTATION, 1)], by[(TRANSLATION, 2)], by[(ROTATION, 2)]) == (6, 7, 10, 12)
    for (path, n_keys), got in by.items():
        comps = 4 if path == ROTATION else 3
        assert got == 2 + n_keys * (5 if path == ROTATION else 4), (path, n_keys)          # the sizing pass
        assert got == 2 + n_keys * (1 + comps), (path, n_keys)                              # the filling pass
    assert by[(SCALE, 33)] == by[(TRANSLATION, 33)]


def test_the_probe_layout_is_what_the_seven_entry_points_computed(layouts):
    for (name, n), (off0, off1, total) in zip(PROBE_CALLS, layouts[3]):
        b_in, b_out0, b_out1 = PROBES[name]
        want0, want1, want_total = probe_expected(name, n)
        assert (off0, total) == (want0, want_total), (name, n)
        assert off0 % 16 == 0 and off0 >= n * b_in, (name, n)                    # behind the input, aligned
        if b_out1:
            assert off1 == want1 and off1 % 16 == 0 and off1 >= off0 + n * b_out0 and total == off1 + n * b_out1, (name, n)
        else:
            assert want1 is None and total == off0 + n * b_out0, (name, n)
    by = dict(zip(PROBE_CALLS, layouts[3]))
    assert by[("sample", 1)] == (16, 32, 32) and by[("cube_face", 3)] == (48, 64, 88) and by[("sample_depth", 257)][0] == 3088


def test_the_sanitized_driver_agrees(layouts, sanitized_driver):
    assert _run(sanitized_driver) == layouts
