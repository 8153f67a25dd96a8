"""The edge families of tests/edge_scenes.py on the GPU: the product library against the oracle (depth words bit-exact, colour
within 1 ULP, the six counters equal), and the fenced general test build (libswr_hip_test.so) against the product, word for word.

These are the scenes that sit within rounding distance of the kernels' shortcuts -- binning's tile rejection, the hi-Z pair drop,
the fast coverage walk, the division / sqrt guards, depth_only_grows -- so a wrong margin or threshold shows up here even where the
random scenes of test_gpu_parity.py pass (tests/test_raster_edges_host.py shows on the CPU that each family reaches its bound)."""
import os

import numpy as np
import pytest

import edge_scenes as E
from softwarerenderer_amd import Device, _native, scenes
from test_gpu_parity import run_both

pytestmark = pytest.mark.gpu

SCENES = {s.name: s for s in E.all_scenes(0)}


@pytest.fixture(scope="module")
def testlib_device():
    lib = "libswr_hip_test.so"
    if not os.path.exists(os.path.join(os.path.dirname(_native.LIB_PATH), lib)):
        pytest.fail(f"{lib} is missing: __graft_entry__.build() makes it (make -C softwarerenderer_amd/csrc variants)")
    dev = Device(0, lib=lib)
    yield dev
    dev.close()


def _render(dev, scene):
    dev.reset_stats()
    r = scenes.SceneRenderer(dev, scene)
    c, d = r.render()
    st = dev.stats()
    r.close()
    return c, d, st


@pytest.mark.parametrize("name", list(SCENES))
def test_edge_family_matches_the_oracle_on_both_builds(device, testlib_device, name):
    scene = SCENES[name]
    _, st = run_both(device, scene)
    c0, d0, _ = _render(device, scene)
    c1, d1, s1 = _render(testlib_device, scene)
    assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32)), f"{name}: depth words differ between the product and the test build"
    assert np.array_equal(c0.view(np.uint32), c1.view(np.uint32)), f"{name}: colour words differ between the product and the test build"
    for k in ("fragments_tested", "fragments_shaded", "fragments_written"):
        assert s1[k] == st[k], (name, k, s1[k], st[k])
    assert st["fragments_written"] > 0, f"{name}: nothing was drawn"
