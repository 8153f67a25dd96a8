"""Where swr_raycast / swr_raycast_nearest and swr_character_update put their pieces (csrc/swr_query_layout.h, pure functions the two
calls use) against the expressions the calls carried inline before the header existed, restated here line by line.  The layout is
observable -- through allocation sizes and through which calls are staged in the pinned block -- so it is held to those values,
including the two that look odd: the pageable block of a ray query holds the upload only (the records go straight to the caller's
array), and off_trace is relative to off_down.  The header has no HIP types, so a few-line driver around it is built with the host
compiler, once plain and once with -fsanitize=address,undefined (a stand-alone program: nothing loaded into Python is sanitised).
No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include "swr_query_layout.h"
int main() {            // per line: R n_rays n_targets nearest | C n n_ring n_targets stride -> the layout's fields and whether it is staged
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'R') {
            int n, nt, nearest;
            if (scanf("%d %d %d", &n, &nt, &nearest) != 3) return 1;
            const swr::RayLayout l = swr::ray_layout(n, nt, nearest != 0);
            printf("%zu %zu %zu %zu %zu %d\n", l.pairs, l.n_out, l.off_targets, l.up_bytes, l.down_bytes, swr::query_is_staged(l.up_bytes, l.down_bytes) ? 1 : 0);
        } else if (kind == 'C') {
            int n, nr, nt; unsigned long long stride;
            if (scanf("%d %d %d %llu", &n, &nr, &nt, &stride) != 4) return 1;
            const swr::CharLayout l = swr::char_layout(n, nr, nt, (size_t)stride);
            printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d\n", l.pairs, l.off_chars, l.off_in, l.off_ring, l.off_targets, l.up_bytes, l.off_work,
                   l.off_active, l.off_rays, l.rays_bytes, l.off_down, l.off_trace, l.down_bytes, l.total, swr::query_is_staged(l.up_bytes, l.down_bytes) ? 1 : 0);
        } else return 1;
    }
    printf("%zu\n", swr::kQueryStagedBytes);
    return 0;
}
"""

# sizeof of the records: include/swr.h (the ABI, tests/test_abi.py) and the two only the kernels know (static_assert in csrc/swr_query.h)
SWR_RAY, SWR_RAY_HIT, RAY_TARGET = 24, 40, 152
SWR_CHARACTER, SWR_CHARACTER_INPUT, SWR_CHARACTER_TRACE, CHAR_WORK = 44, 16, 48, 168

RAY_FIELDS = ("pairs", "n_out", "off_targets", "up_bytes", "down_bytes", "staged")
CHAR_FIELDS = ("pairs", "off_chars", "off_in", "off_ring", "off_targets", "up_bytes", "off_work", "off_active", "off_rays", "rays_bytes", "off_down",
               "off_trace", "down_bytes", "total", "staged")


def al(b):
    return (b + 15) & ~15


def ray_expected(n_rays, n_targets, nearest):
    """raycast(), as it stood"""
    pairs = n_rays * n_targets; n_out = n_rays if nearest else pairs
    off_t = (n_rays * SWR_RAY + 15) & ~15
    up_bytes = off_t + ((n_targets * RAY_TARGET + 15) & ~15); down_bytes = n_out * SWR_RAY_HIT
    staged = up_bytes + down_bytes <= (1 << 20)
    return dict(pairs=pairs, n_out=n_out, off_targets=off_t, up_bytes=up_bytes, down_bytes=down_bytes, staged=int(staged))


def char_expected(n, n_ring, n_targets, stride):
    """character_update(), as it stood"""
    N = n; NT = n_targets
    off_chars = 0; off_in = off_chars + al(N * SWR_CHARACTER); off_ring = off_in + al(N * SWR_CHARACTER_INPUT)
    off_t = off_ring + al(n_ring * 8); up_bytes = off_t + al(NT * RAY_TARGET)
    off_work = up_bytes; off_active = off_work + al(N * CHAR_WORK); off_rays = off_active + al(N * 4)
    rays_bytes = al(N * stride * SWR_RAY)
    off_down = off_rays + 2 * rays_bytes; off_trace = al(N * SWR_CHARACTER)
    down_bytes = off_trace + N * SWR_CHARACTER_TRACE
    total = off_down + down_bytes                    # ensure(c, c->d_char, off_down + down_bytes)
    pairs = N * stride * NT
    staged = up_bytes + down_bytes <= (1 << 20)
    return dict(pairs=pairs, off_chars=off_chars, off_in=off_in, off_ring=off_ring, off_targets=off_t, up_bytes=up_bytes, off_work=off_work,
                off_active=off_active, off_rays=off_rays, rays_bytes=rays_bytes, off_down=off_down, off_trace=off_trace, down_bytes=down_bytes,
                total=total, staged=int(staged))


COUNTS, TARGETS, STRIDES = (0, 1, 2, 3, 65), (0, 1, 3, 11), (36, 54, 74, 4096)
# the shapes of the GPU tests across the threshold (tests/test_gpu_raycast.py, tests/test_gpu_character.py) first
RAY_SHAPES = [(7278, 3, 0), (7280, 3, 0), (7280, 3, 1)] + [(n, t, k) for n in COUNTS for t in TARGETS for k in (0, 1)]
CHAR_SHAPES = [(7000, 18, 1, 36), (3500, 18, 1, 36), (7000, 18, 2, 36), (3500, 18, 2, 36), (4096, 18, 0, 36)] + \
              [(n, r, t, s) for n in COUNTS for t in TARGETS for s, r in zip(STRIDES, (18, 18, 37, 2048))]


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
    return _build(tmp_path_factory, "layout", [])


@pytest.fixture(scope="module")
def sanitized_driver(tmp_path_factory):
    return _build(tmp_path_factory, "layout_san", ["-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(exe):
    text = "".join(f"R {n} {t} {k}\n" for n, t, k in RAY_SHAPES) + "".join(f"C {n} {r} {t} {s}\n" for n, r, t, s in CHAR_SHAPES)
    done = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    lines = done.stdout.split("\n")[:-1]
    assert len(lines) == len(RAY_SHAPES) + len(CHAR_SHAPES) + 1 and int(lines[-1]) == 1 << 20
    rays = [dict(zip(RAY_FIELDS, map(int, ln.split()))) for ln in lines[:len(RAY_SHAPES)]]
    chars = [dict(zip(CHAR_FIELDS, map(int, ln.split()))) for ln in lines[len(RAY_SHAPES):-1]]
    return rays, chars


@pytest.fixture(scope="module")
def layouts(driver):
    return _run(driver)


def test_the_ray_layout_is_what_raycast_computed(layouts):
    for shape, got in zip(RAY_SHAPES, layouts[0]):
        assert got == ray_expected(*shape), shape
    by = dict(zip(RAY_SHAPES, layouts[0]))
    assert by[(7278, 3, 0)]["up_bytes"] + by[(7278, 3, 0)]["down_bytes"] == 1048496 and by[(7278, 3, 0)]["staged"] == 1
    assert by[(7280, 3, 0)]["up_bytes"] + by[(7280, 3, 0)]["down_bytes"] == 1048784 and by[(7280, 3, 0)]["staged"] == 0
    assert by[(7280, 3, 1)]["down_bytes"] == 40 * 7280 and by[(7280, 3, 1)]["staged"] == 1


def test_the_character_layout_is_what_character_update_computed(layouts):
    for shape, got in zip(CHAR_SHAPES, layouts[1]):
        assert got == char_expected(*shape), shape
    by = dict(zip(CHAR_SHAPES, layouts[1]))
    for shape, total, staged in (((7000, 18, 1, 36), 1064304, 0), ((3500, 18, 1, 36), 532304, 1), ((7000, 18, 2, 36), 1064448, 0),
                                 ((3500, 18, 2, 36), 532448, 1), ((4096, 18, 0, 36), 622736, 1)):
        assert by[shape]["up_bytes"] + by[shape]["down_bytes"] == total and by[shape]["staged"] == staged, shape


def test_regions_are_in_order_disjoint_and_aligned(layouts):
    for (n, t, k), l in zip(RAY_SHAPES, layouts[0]):
        regions = [(0, n * SWR_RAY), (l["off_targets"], t * RAY_TARGET), (l["up_bytes"], l["down_bytes"])]
        _check_regions(regions, l["up_bytes"] + l["down_bytes"], (n, t, k))
        assert l["down_bytes"] == l["n_out"] * SWR_RAY_HIT and l["pairs"] == n * t
    for (n, r, t, s), l in zip(CHAR_SHAPES, layouts[1]):
        regions = [(l["off_chars"], n * SWR_CHARACTER), (l["off_in"], n * SWR_CHARACTER_INPUT), (l["off_ring"], r * 8), (l["off_targets"], t * RAY_TARGET),
                   (l["off_work"], n * CHAR_WORK), (l["off_active"], n * 4), (l["off_rays"], n * s * SWR_RAY), (l["off_rays"] + l["rays_bytes"], n * s * SWR_RAY),
                   (l["off_down"], n * SWR_CHARACTER), (l["off_down"] + l["off_trace"], n * SWR_CHARACTER_TRACE)]
        _check_regions(regions, l["total"], (n, r, t, s))
        assert l["off_work"] == l["up_bytes"] and l["total"] == l["off_down"] + l["down_bytes"] and l["pairs"] == n * s * t


def _check_regions(regions, total, what):
    end = 0
    for off, size in regions:
        assert off % 16 == 0 and off >= end, (what, regions)
        end = off + size
    assert end == total, (what, end, total)          # the last region ends the block


def test_the_sanitized_driver_agrees(layouts, sanitized_driver):
    assert _run(sanitized_driver) == layouts
