"""Post-process programs on the GPU (include/swr.h, csrc/swr_post.hip.h): k_resolve_rgba and the run-time compiled
k_post against the numpy twins of tests/post_cases.py, bit for bit and without a tolerance -- float words with assert_same_words,
bytes with equality -- through every entry point: swr_readback_post, swr_present_post_async, swr_post_device[_async], swr_post_size.
Frames are uploaded, so nothing has to render except where a test is about rendering."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import post_cases as P
import spawner
from resolve_cases import assert_same_words
from softwarerenderer_amd import Device, MainWindow, PostProgram, _native, scenes
from test_gpu_present8 import CANARY, GUARD, DeviceBytes, same_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = _native.SWR_ERR_INVALID_ARG, _native.SWR_ERR_UNSUPPORTED
DTYPE = {P.RGB32F: np.float32, P.RGB8: np.uint8, P.RGBX8: np.uint8}
CHANNELS = {P.RGB32F: 3, P.RGB8: 3, P.RGBX8: 4}
BPP = {P.RGB32F: 12, P.RGB8: 3, P.RGBX8: 4}


@pytest.fixture(scope="module")
def posts(device):
    progs = {name: PostProgram(device, text, constants=P.CONSTANTS.get(name)) for name, text in P.TEXTS.items()}
    yield progs
    for p in progs.values():
        p.close()


def same(got, want, what):
    if want.dtype == np.uint8:
        same_bytes(got, want, what)
    else:
        assert got.dtype == np.float32
        assert_same_words(got, want, what)


def c_post_size(device, kx, ky, fmt):
    w, rows, nbytes = C.c_int(-7), C.c_int(-7), C.c_size_t(7)
    rc = device._lib.swr_post_size(device._ctx, kx, ky, fmt, C.byref(w), C.byref(rows), C.byref(nbytes))
    return rc, rows.value, w.value, nbytes.value


def post_buffer(win, post, kx, ky, fmt):
    return win.PostBuffer(post, kx, ky, CHANNELS[fmt], DTYPE[fmt])


@pytest.mark.parametrize("out_size", P.OUT_SIZES)
def test_identity_equals_the_resolved_and_the_8_bit_payloads(device, posts, out_size):
    for factors in P.FACTORS:
        w, h = P.frame_size(out_size, factors)
        win = MainWindow(device, w, h)
        for fmt in P.FORMATS:
            color, depth = P.planes(out_size, factors, P.plane_kind("IDENTITY", fmt))
            win.Upload(color=color, depth=depth)
            assert c_post_size(device, *factors, fmt) == (0, out_size[1], out_size[0], out_size[0] * out_size[1] * BPP[fmt])
            got = post_buffer(win, posts["IDENTITY"], *factors, fmt)
            direct = win.ResolvedColorBuffer(*factors) if fmt == P.RGB32F else win.ColorBuffer8(*factors, CHANNELS[fmt])
            same(got, direct, ("IDENTITY against the present", out_size, factors, fmt))
            same(got, P.expected("IDENTITY", color, depth, *factors, fmt), ("IDENTITY against the twin", out_size, factors, fmt))


@pytest.mark.parametrize("out_size", P.OUT_SIZES)
@pytest.mark.parametrize("name", ["TINT", "COORDS", "BOX3", "EDGE", "SPECIALS"])
def test_every_program_equals_its_twin(device, posts, name, out_size):
    for factors in P.FACTORS:
        w, h = P.frame_size(out_size, factors)
        win = MainWindow(device, w, h)
        color, depth = P.planes(out_size, factors, P.plane_kind(name))
        win.Upload(color=color, depth=depth)
        for fmt in (P.FORMATS if name == "SPECIALS" else (P.RGB32F,)):
            got = post_buffer(win, posts[name], *factors, fmt)
            same(got, P.expected(name, color, depth, *factors, fmt), (name, out_size, factors, fmt))


def test_alpha_reaches_the_program_through_the_same_tree_and_scale(device):
    post = PostProgram(device, P.HEAD + "    return make_float4(in.color.w, swr_post_fetch(env, in.x, in.y).w, in.color.x, 0.0f);\n}\n")
    try:
        for factors in ((1, 1), (4, 2), (8, 8)):
            color, depth = P.planes((65, 5), factors, "pool")
            win = MainWindow(device, color.shape[1], color.shape[0])
            win.Upload(color=color)
            res = P.resolve_rgba(color, *factors)
            assert_same_words(win.PostBuffer(post, *factors, 3, np.float32), res[..., [3, 3, 0]], factors)
    finally:
        post.close()


def test_recorded_draws_are_flushed_before_the_program_runs(device, posts):
    s = scenes.cfg2(96, 64, 200, seed=17)
    r = scenes.SceneRenderer(device, s)
    win = r.window
    win.Upload(color=np.full((64, 96, 4), 0.25, dtype=np.float32))
    r.submit_frame()                                                  # recorded, not flushed
    got_box = win.PostBuffer(posts["BOX3"], 1, 1, 3, np.float32)
    color, depth = win.ColorBuffer, win.DepthBuffer
    assert len(np.unique(color[..., :3])) > 100                       # the frame has content, and the program saw it
    assert_same_words(got_box, P.expected("BOX3", color, depth, 1, 1), "BOX3 on a rendered frame")
    r.submit_frame()
    same_bytes(win.PostBuffer(posts["TINT"], 2, 2, 4, np.uint8), P.expected("TINT", color, depth, 2, 2, P.RGBX8), "TINT, RGBX8, (2, 2)")
    r.submit_frame()
    got_edge = win.PostBuffer(posts["EDGE"], 2, 2, 3, np.float32)
    assert np.any(depth != np.finfo(np.float32).min)                  # the draws wrote depth
    assert_same_words(got_edge, P.expected("EDGE", color, depth, 2, 2), "EDGE on a rendered frame")
    r.close()


def test_two_presents_in_flight_keep_their_frames_and_constants_and_share_the_tickets():
    """96 x 64 at (2, 2).  Present i, wait i - 2: post presents alternate with 8-bit presents on the same slots and ticket sequence;
    each post present carries constants set just before it and changed right after; no call makes the host wait for the stream."""
    dev = Device(0)                                                   # a fresh context: its staging buffers and its plane start empty
    ra = scenes.SceneRenderer(dev, scenes.cfg2(96, 64, 150, seed=5))
    rb = scenes.SceneRenderer(dev, scenes.cfg2(96, 64, 150, seed=6), window=ra.window)
    win = ra.window
    frames = []
    for r in (ra, rb):
        r.render()                                                    # synchronous frames first: sizes the pair buffers too
        frames.append((win.ColorBuffer.copy(), win.DepthBuffer.copy()))
    tint = PostProgram(dev, P.TINT)
    warm = np.zeros((32, 48, 3), dtype=np.uint8)
    ra.submit_frame()
    assert win.PresentWait(win.PresentPostAsync(tint, warm, 2, 2))    # first use allocates the plane and a staging buffer
    kinds = ["post8", "post8", "rgb8", "postf", "post8", "rgb8", "postf", "postf"]
    pinned, pending = [], []
    try:
        s0 = dev.sync_count()
        for i, kind in enumerate(kinds):
            k = (i // 2) & 1
            (ra, rb)[k].submit_frame()
            consts = np.array([1.0 + 0.125 * i, 0.5, 0.25 * i, 0.01 * i, 0.0, -0.03], dtype=np.float32)
            if kind == "rgb8":
                want = P.K.present8(frames[k][0], 2, 2, 3)
            else:
                want = P.expected("TINT", *frames[k], 2, 2, P.RGB8 if kind == "post8" else P.RGB32F, constants=consts)
            out = np.zeros_like(want)
            dev.pin(out); pinned.append(out)
            if len(pending) == 2:
                t, o, w = pending.pop(0)
                assert win.PresentWait(t)
                same(o, w, ("settled", i - 2))
            if kind == "rgb8":
                t = win.Present8Async(out, 2, 2)
            else:
                tint.SetConstants(consts)
                t = win.PresentPostAsync(tint, out, 2, 2)
                tint.SetConstants([9.0] * 64)                         # too late for the present just made
            if pending:
                assert t == pending[-1][0] + 1                        # one ticket sequence for every kind
            pending.append((t, out, want))
        assert dev.sync_count() == s0                                 # the whole loop never waited for the stream
        for t, o, w in pending:
            assert win.PresentWait(t)
            same(o, w, "tail")
    finally:
        dev.sync()
        for x in pinned:
            dev.unpin(x)
    tint.close(); ra.close(); rb.close(); dev.close()


def test_destroy_right_after_an_asynchronous_present_still_delivers(device):
    color, depth = P.planes((130, 9), (8, 8), "pool")
    win = MainWindow(device, color.shape[1], color.shape[0])
    win.Upload(color=color, depth=depth)
    post = PostProgram(device, P.BOX3)
    out = np.zeros((9, 130, 4), dtype=np.uint8)
    t = win.PresentPostAsync(post, out, 8, 8)
    pid = post._id
    post.close()                                                      # the kernel may be in flight
    assert device._lib.swr_post_destroy(device._ctx, pid) == INVALID  # the id is gone at once
    assert win.PresentWait(t)
    same_bytes(out, P.expected("BOX3", color, depth, 8, 8, P.RGBX8), "BOX3 after destroy")
    device.sync()                                                     # the parked module is unloaded here


@pytest.mark.parametrize("wait", [True, False])
def test_device_destinations(device, posts, wait):
    color, depth = P.planes((65, 5), (4, 2), "pool")
    win = MainWindow(device, color.shape[1], color.shape[0])
    win.Upload(color=color, depth=depth)
    for fmt in P.FORMATS:
        want = P.expected("TINT", color, depth, 4, 2, fmt)
        n = want.nbytes
        buf = DeviceBytes(n + GUARD)
        try:
            buf.fill(CANARY)
            s0 = device.sync_count()
            win.PostTo(posts["TINT"], buf.ptr.value, 4, 2, CHANNELS[fmt], DTYPE[fmt], wait=wait)
            assert wait or device.sync_count() == s0                  # the async form does not wait for the stream
            device.sync()
            back = buf.read()
            same(back[:n].view(DTYPE[fmt]).reshape(want.shape), want, ("device", fmt, wait))
            assert np.all(back[n:] == CANARY)
            buf.fill(CANARY)
            fn = device._lib.swr_post_device if wait else device._lib.swr_post_device_async
            for off in (1, 2, 3):                                     # a device destination must be 4-byte aligned, in every format
                assert fn(device._ctx, posts["TINT"]._id, 4, 2, fmt, C.c_void_p(buf.ptr.value + off)) == INVALID
            device.sync()
            assert np.all(buf.read() == CANARY)
        finally:
            buf.free()


def test_errors_write_nothing_issue_no_ticket_and_leave_the_context_usable(device, posts):
    lib, ctx = device._lib, device._ctx
    color, depth = P.planes((5, 3), (8, 8), "pool")                   # 40 x 24
    win = MainWindow(device, 40, 24)
    win.Upload(color=color, depth=depth)
    out = np.full((24, 40, 3), 123.0, dtype=np.float32)
    buf = DeviceBytes(out.nbytes)
    buf.fill(0x5A)
    good = posts["IDENTITY"]._id
    other_dev = Device(0)
    foreign = PostProgram(other_dev, P.IDENTITY)
    gone = PostProgram(device, P.TINT)
    gone_id = gone._id
    gone.close()

    def untouched():
        device.sync()
        return np.all(out == 123.0) and np.all(buf.read() == 0x5A)

    def all_refuse(pid, kx, ky, fmt, code=INVALID):
        t = C.c_uint64(77)
        assert lib.swr_readback_post(ctx, pid, kx, ky, fmt, out.ctypes.data) == code
        assert lib.swr_present_post_async(ctx, pid, kx, ky, fmt, out.ctypes.data, C.byref(t)) == code and t.value == 77      # no ticket
        assert lib.swr_post_device(ctx, pid, kx, ky, fmt, buf.ptr) == code
        assert lib.swr_post_device_async(ctx, pid, kx, ky, fmt, buf.ptr) == code
        assert untouched()
        same_bytes(win.PostBuffer(posts["IDENTITY"], 8, 8, 3, np.uint8), P.expected("IDENTITY", color, depth, 8, 8, P.RGB8), "usable afterwards")

    try:
        for pid in (0, -1, 999999, gone_id, foreign._id):             # unknown, destroyed, another context's
            assert foreign._id != good
            all_refuse(pid, 1, 1, P.RGB32F)
        assert lib.swr_post_destroy(ctx, foreign._id) == INVALID and lib.swr_post_set_constants(ctx, gone_id, None, 0) == INVALID
        for bad in (1, 2, 5, 12, -1):
            all_refuse(good, 1, 1, bad)
            assert c_post_size(device, 1, 1, bad) == (INVALID, -7, -7, 7)
        for bad in (0, 3, 16, -2):
            all_refuse(good, bad, 1, P.RGB8)
            all_refuse(good, 2, bad, P.RGBX8)
            assert c_post_size(device, bad, 2, P.RGB8) == (INVALID, -7, -7, 7)
        win.Resize(36, 20)                                            # neither divides by 8
        for kx, ky in ((8, 1), (1, 8)):
            t = C.c_uint64(77)
            assert lib.swr_readback_post(ctx, good, kx, ky, P.RGB32F, out.ctypes.data) == INVALID
            assert lib.swr_present_post_async(ctx, good, kx, ky, P.RGB8, out.ctypes.data, C.byref(t)) == INVALID and t.value == 77
            assert lib.swr_post_device(ctx, good, kx, ky, P.RGBX8, buf.ptr) == INVALID
            assert lib.swr_post_device_async(ctx, good, kx, ky, P.RGB8, buf.ptr) == INVALID
        assert c_post_size(device, 4, 4, P.RGBX8) == (0, 5, 9, 180) and untouched()
        win.Resize(40, 24)
        win.Upload(color=color, depth=depth)
        # NULL pointers
        t, i, z = C.c_uint64(77), C.c_int(0), C.c_size_t(0)
        assert lib.swr_post_size(ctx, 2, 2, 3, None, C.byref(i), C.byref(z)) == INVALID
        assert lib.swr_post_size(ctx, 2, 2, 3, C.byref(i), None, C.byref(z)) == INVALID
        assert lib.swr_post_size(ctx, 2, 2, 3, C.byref(i), C.byref(i), None) == INVALID
        assert lib.swr_readback_post(ctx, good, 2, 2, 3, None) == INVALID
        assert lib.swr_present_post_async(ctx, good, 2, 2, 3, None, C.byref(t)) == INVALID and t.value == 77
        assert lib.swr_present_post_async(ctx, good, 2, 2, 3, out.ctypes.data, None) == INVALID
        assert lib.swr_post_device(ctx, good, 2, 2, 3, None) == INVALID and lib.swr_post_device_async(ctx, good, 2, 2, 3, None) == INVALID
        assert lib.swr_readback_post(None, good, 2, 2, 3, out.ctypes.data) == INVALID
        pid = C.c_int(-5)
        assert lib.swr_post_create(ctx, None, C.byref(pid)) == INVALID and lib.swr_post_create(ctx, P.IDENTITY.encode(), None) == INVALID
        assert lib.swr_post_create(ctx, P.SYNTAX_ERROR.encode(), C.byref(pid)) == INVALID and pid.value == -5
        assert f"post.hip:{P.SYNTAX_ERROR_LINE}:".encode() in lib.swr_last_error(ctx)
        assert lib.swr_post_create(ctx, P.NO_ENTRY.encode(), C.byref(pid)) == INVALID and pid.value == -5
        k = (C.c_float * 65)()
        assert lib.swr_post_set_constants(ctx, good, k, 65) == INVALID and lib.swr_post_set_constants(ctx, good, None, 3) == INVALID
        assert untouched()
        # a band: a neighbour across its edge is not in this context
        win.SetBand(0, 1)
        tb = C.c_uint64(77)
        assert lib.swr_readback_post(ctx, good, 1, 1, P.RGB32F, out.ctypes.data) == UNSUPPORTED
        assert lib.swr_present_post_async(ctx, good, 1, 1, P.RGB32F, out.ctypes.data, C.byref(tb)) == UNSUPPORTED and tb.value == 77
        assert lib.swr_post_device(ctx, good, 1, 1, P.RGB32F, buf.ptr) == UNSUPPORTED
        assert lib.swr_post_device_async(ctx, good, 1, 1, P.RGB32F, buf.ptr) == UNSUPPORTED
        win.SetBandInterleaved(0, 2, 1)
        assert lib.swr_readback_post(ctx, good, 1, 1, P.RGB32F, out.ctypes.data) == UNSUPPORTED
        assert untouched()
        win.SetBand(-1, -1)
        win.Upload(color=color, depth=depth)
        same_bytes(win.PostBuffer(posts["IDENTITY"], 8, 8, 3, np.uint8), P.expected("IDENTITY", color, depth, 8, 8, P.RGB8), "usable after a band")
        # a zero-size target: SWR_OK, nothing written (a bad format, bad factors and an unknown id are still refused)
        win.Resize(0, 0)
        assert c_post_size(device, 8, 8, P.RGBX8) == (0, 0, 0, 0)
        assert lib.swr_readback_post(ctx, good, 8, 8, P.RGB8, out.ctypes.data) == 0
        assert lib.swr_post_device(ctx, good, 2, 4, P.RGBX8, buf.ptr) == 0 and lib.swr_post_device_async(ctx, good, 2, 4, P.RGB32F, buf.ptr) == 0
        assert lib.swr_present_post_async(ctx, good, 2, 2, P.RGB8, out.ctypes.data, C.byref(t)) == 0 and t.value != 77
        assert win.PresentWait(t.value)
        assert lib.swr_readback_post(ctx, good, 3, 8, P.RGB8, out.ctypes.data) == INVALID
        assert lib.swr_readback_post(ctx, good, 2, 2, 5, out.ctypes.data) == INVALID
        assert lib.swr_readback_post(ctx, gone_id, 2, 2, P.RGB8, out.ctypes.data) == INVALID
        assert win.PostBuffer(posts["IDENTITY"], 4, 4, 4, np.uint8).shape == (0, 0, 4)
        assert untouched()
    finally:
        win.SetBand(-1, -1)
        buf.free()
        foreign.close(); other_dev.close()


def test_swr_lerp_follows_the_librarys_numerics_model(tmp_path):
    """TINT written with swr_lerp, in a child process under libswr_hip_fma.so: the fused twin's words -- and not the unfused twin's."""
    color, depth = P.planes((65, 5), (1, 1), "pool")
    consts = P.constants64(P.TINT_CONSTANTS)
    np.save(tmp_path / "frame.npy", color); np.save(tmp_path / "constants.npy", consts)
    env = dict(os.environ, SWR_LIB="libswr_hip_fma.so")
    r = spawner.run([sys.executable, os.path.join(ROOT, "tests", "post_child.py"), "TINT_LERP", "1", "1", str(tmp_path / "frame.npy"),
                     str(tmp_path / "constants.npy"), str(tmp_path / "out.npy")], env=env, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "library=libswr_hip_fma.so lerp_fused=1" in r.stdout
    got = np.load(tmp_path / "out.npy")
    res = P.resolve_rgba(color, 1, 1)
    fused, unfused = P.tint_lerp_fused(res, depth, 1, 1, consts), P.tint_lerp(res, depth, 1, 1, consts)
    assert not np.array_equal(fused.view(np.uint32), unfused.view(np.uint32))       # the plane tells the two models apart
    assert_same_words(got, fused, "TINT_LERP under libswr_hip_fma.so")


def test_swr_lerp_unfused_in_the_product_library(device):
    color, depth = P.planes((65, 5), (1, 1), "pool")
    win = MainWindow(device, 65, 5)
    win.Upload(color=color)
    post = PostProgram(device, P.TINT_LERP, constants=P.TINT_CONSTANTS)
    try:
        k = P.constants64(P.TINT_CONSTANTS)
        assert_same_words(win.PostBuffer(post, 1, 1, 3, np.float32), P.tint_lerp(P.resolve_rgba(color, 1, 1), depth, 1, 1, k), "TINT_LERP")
    finally:
        post.close()
