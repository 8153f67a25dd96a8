"""Supersampled present on the GPU (include/swr.h, csrc/swr_deliver.hip.h): k_resolve_rgb against the numpy
restatement of tests/resolve_cases.py, word for word on uint32 views (NaN positions compared as NaN), through every entry point:
swr_readback_rgb_resolved, swr_resolve_rgb_device[_async], swr_present_rgb_resolved_async, swr_resolved_size."""
import ctypes as C

import numpy as np
import pytest

import resolve_cases as K
from softwarerenderer_amd import MainWindow, _native, multigpu, scenes

pytestmark = pytest.mark.gpu

SIZES = [(40, 24), (136, 72), (1032, 16)]       # partial last tile row and column; output widths 5 and 17; a wave tail (1032 = 16 * 64 + 8)


def c_resolved_size(device, kx, ky):
    w, rows = C.c_int(-7), C.c_int(-7)
    rc = device._lib.swr_resolved_size(device._ctx, kx, ky, C.byref(w), C.byref(rows))
    return rc, rows.value, w.value


def check_all_pairs(device, width, height, seed):
    win = MainWindow(device, width, height)
    plane = K.special_plane(height, width, seed)
    win.Upload(color=plane)
    for kx, ky in K.PAIRS:
        got = win.ResolvedColorBuffer(kx, ky)
        assert got.shape == (height // ky, width // kx, 3)
        assert c_resolved_size(device, kx, ky) == (0, height // ky, width // kx)
        K.assert_same_words(got, K.resolve(plane, kx, ky), (width, height, kx, ky))


@pytest.mark.parametrize("width,height", SIZES)
def test_every_factor_pair_equals_the_restatement_on_uploaded_planes(device, width, height):
    check_all_pairs(device, width, height, seed=width)


@pytest.mark.parametrize("lib", ["libswr_hip_fma_dpps.so", "libswr_hip_test.so"])
def test_the_numerics_and_test_builds_resolve_the_same_words(lib):
    """The numerics switches of the library variants do not touch this arithmetic."""
    from softwarerenderer_amd import Device
    dev = Device(0, lib=lib)
    try:
        check_all_pairs(dev, 136, 72, seed=5)
    finally:
        dev.close()


def test_factors_one_one_equal_the_flatten(device):
    win = MainWindow(device, 136, 72)
    plane = K.special_plane(72, 136, seed=9)
    plane = np.where(np.isfinite(plane), plane, np.float32(0.5)).astype(np.float32)
    win.Upload(color=plane)
    flat = win.FlatColorBuffer()
    got = win.ResolvedColorBuffer(1, 1)
    assert np.array_equal(got.view(np.uint32), flat.view(np.uint32)) and np.array_equal(flat.view(np.uint32), plane[..., :3].view(np.uint32))


def test_a_rendered_frame_is_flushed_and_then_resolved(device):
    s = scenes.cfg2(256, 192, 400, seed=31)
    r = scenes.SceneRenderer(device, s)
    r.window.Upload(color=np.full((192, 256, 4), 0.25, dtype=np.float32))
    r.submit_frame()                                                  # recorded, not flushed: the plane still holds 0.25 everywhere
    got = r.window.ResolvedColorBuffer(2, 2)
    color = r.window.ColorBuffer
    assert len(np.unique(color[..., :3])) > 100                       # the frame has content ...
    assert not np.all(got == np.float32(0.25))                        # ... and the resolve saw it
    K.assert_same_words(got, K.resolve(color, 2, 2))
    r.close()


class DeviceBuffer:
    """Caller-owned device memory straight from the HIP runtime the library already loaded."""

    def __init__(self, nbytes):
        self.hip, self.nbytes, self.ptr = C.CDLL("libamdhip64.so"), nbytes, C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(nbytes)) == 0

    def fill(self, byte):
        assert self.hip.hipMemset(self.ptr, C.c_int(byte), C.c_size_t(self.nbytes)) == 0

    def read(self, shape):
        out = np.empty(shape, dtype=np.float32)
        assert out.nbytes == self.nbytes
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), self.ptr, C.c_size_t(self.nbytes), 2) == 0        # hipMemcpyDeviceToHost
        return out

    def free(self):
        self.hip.hipFree(self.ptr)


def test_device_variants_write_the_same_words(device):
    s = scenes.cfg2(200, 120, 300, seed=12)
    r = scenes.SceneRenderer(device, s)
    want = K.resolve(r.render()[0], 4, 2)
    shape = (60, 50, 3)
    assert r.window.ResolvedSize(4, 2) == shape[:2]
    buf = DeviceBuffer(60 * 50 * 3 * 4)
    try:
        buf.fill(0xFF)
        r.submit_frame()
        r.window.ResolveTo(buf.ptr.value, 4, 2)
        device.sync()
        K.assert_same_words(buf.read(shape), want, "swr_resolve_rgb_device")
        buf.fill(0xFF)
        r.submit_frame()
        s0 = device.sync_count()
        r.window.ResolveToAsync(buf.ptr.value, 4, 2)
        assert device.sync_count() == s0                              # the async variant does not wait for the stream
        device.sync()
        K.assert_same_words(buf.read(shape), want, "swr_resolve_rgb_device_async")
    finally:
        buf.free()
    r.close()


def test_resolved_and_plain_presents_alternate_on_the_shared_slots():
    """512 x 384 at (2, 2): the resolved present shares swr_present_rgb_async's two slots, tickets and staging buffers; the two kinds
    alternate, each pinned buffer ends up with exactly its frame's words, and no present call makes the host wait for the stream."""
    from softwarerenderer_amd import Device
    dev = Device(0)
    a = scenes.cfg3(512, 384, (2, 2), (30, 20), tex_size=64, seed=91)
    b = scenes.cfg2(512, 384, 1500, seed=92)
    ra = scenes.SceneRenderer(dev, a)
    rb = scenes.SceneRenderer(dev, b, window=ra.window)
    win = ra.window
    frames = [ra.render()[0].copy(), rb.render()[0].copy()]           # synchronous frames first: sizes the pair buffers too
    want = {("plain", k): frames[k][..., :3].copy() for k in (0, 1)}
    want.update({("resolved", k): K.resolve(frames[k], 2, 2) for k in (0, 1)})
    bufs = {"resolved": np.zeros((192, 256, 3), dtype=np.float32), "plain": np.zeros((384, 512, 3), dtype=np.float32)}
    for x in bufs.values():
        dev.pin(x)

    def present(kind):
        s0 = dev.sync_count()
        t = win.PresentResolvedAsync(bufs[kind], 2, 2) if kind == "resolved" else win.PresentAsync(bufs[kind])
        assert dev.sync_count() == s0                                 # never waits for the stream
        return t

    try:
        ra.submit_frame(); t0 = present("resolved")
        rb.submit_frame(); t1 = present("plain")                      # frame b renders and is flattened while frame a's payload is copied
        assert t1 == t0 + 1                                           # one ticket sequence for both kinds
        assert win.PresentWait(t0) and win.PresentWait(t1)
        K.assert_same_words(bufs["resolved"], want[("resolved", 0)])
        K.assert_same_words(bufs["plain"], want[("plain", 1)])
        # six frames, kinds alternating (now on the other slot each), scenes changing every second frame: present i, wait i - 2
        tickets, shown = {}, {}
        for i in range(6):
            kind, k = ("plain", "resolved")[i & 1], (i // 2) & 1
            (ra, rb)[k].submit_frame()
            if kind in tickets:
                assert win.PresentWait(tickets[kind])
                K.assert_same_words(bufs[kind], want[(kind, shown[kind])], (i, kind))
            tickets[kind], shown[kind] = present(kind), k
        for kind in tickets:
            assert win.PresentWait(tickets[kind])
            K.assert_same_words(bufs[kind], want[(kind, shown[kind])], kind)
        assert win.PresentWait(tickets["resolved"]) and win.PresentWait(tickets["plain"])      # waiting twice for a ticket is harmless
    finally:
        for x in bufs.values():
            dev.unpin(x)
    ra.close(); rb.close(); dev.close()


def test_resolved_present_reports_a_stale_frame_after_a_replay():
    """The construction of test_asynchronous_present_reports_a_stale_frame_after_a_replay (tests/test_gpu_api.py) with the resolved
    payload: a batch that does not fit poisons itself, the present behind it resolves the UNCHANGED framebuffer, the wait says so
    after replaying, and presenting again delivers the frame."""
    from softwarerenderer_amd import Device
    dev = Device(0)                                                   # a fresh context: its pair buffers start empty
    small = scenes.cfg2(256, 256, 40, seed=60, min_area=10.0, max_area=60.0)
    big = scenes.cfg2(256, 256, 3000, seed=61, min_area=200.0, max_area=9000.0)
    r0 = scenes.SceneRenderer(dev, small)
    r0.render()                                                       # synchronous sizing of the pair buffers (small)
    r1 = scenes.SceneRenderer(dev, big, window=r0.window)
    out = np.zeros((128, 128, 3), dtype=np.float32)
    before = dev.replay_count()
    r1.submit_frame()                                                 # does not fit: poisoned on the device
    t = r0.window.PresentResolvedAsync(out, 2, 2)
    assert r0.window.PresentWait(t) is False                          # stale, and the batch has been replayed by now
    assert dev.replay_count() == before + 1
    stale = out.copy()
    t = r0.window.PresentResolvedAsync(out, 2, 2)                     # the caller's reaction: present again
    assert r0.window.PresentWait(t) is True
    K.assert_same_words(out, K.resolve(r0.window.ColorBuffer, 2, 2))
    assert not np.array_equal(stale, out)                             # the first payload really predated the batch
    r0.close(); r1.close(); dev.close()


@pytest.mark.parametrize("kx,ky", [(2, 8), (8, 2), (4, 4)])
def test_band_payloads_concatenate_to_the_whole_frame_resolve(device, kx, ky):
    """64 x 88: five full tile rows and one of 8 pixel rows.  Contiguous bands of 2 and 3 ranks, and interleaved one-tile-row stripes:
    every band's rows are a multiple of ky, so the bands resolve on their own."""
    W, H = 64, 88
    win = MainWindow(device, W, H)
    plane = K.special_plane(H, W, seed=kx * 10 + ky)
    try:
        win.Upload(color=plane)
        whole = win.ResolvedColorBuffer(kx, ky)
        K.assert_same_words(whole, K.resolve(plane, kx, ky), "whole frame")
        for world in (2, 3):
            parts = []
            for first, count in multigpu.band_partition(H, world):
                win.SetBand(first, count)
                y0, rows = win.band_pixel_rows()
                assert rows % ky == 0 and c_resolved_size(device, kx, ky) == (0, rows // ky, W // kx)
                win.Upload(color=plane[y0:y0 + rows])
                parts.append(win.ResolvedColorBuffer(kx, ky))
            K.assert_same_words(np.concatenate(parts), whole, ("contiguous", world))
            stripes = multigpu.stripe_rows(H, world, 1)
            frame = np.full_like(whole, 123.0)
            for rank in range(world):
                win.SetBandInterleaved(rank, world, 1)
                rows = stripes[rank]
                assert len(rows) % ky == 0 and c_resolved_size(device, kx, ky) == (0, len(rows) // ky, W // kx)
                win.Upload(color=plane[rows])
                frame[rows[::ky] // ky] = win.ResolvedColorBuffer(kx, ky)           # a stripe's blocks keep their place in the frame
            K.assert_same_words(frame, whole, ("interleaved", world))
    finally:
        win.SetBand(-1, -1)


def test_bad_arguments_are_refused_and_write_nothing(device):
    lib, ctx = device._lib, device._ctx
    INVALID = _native.SWR_ERR_INVALID_ARG
    win = MainWindow(device, 40, 24)
    win.Upload(color=K.special_plane(24, 40, seed=3))
    out = np.full((24, 40, 3), 123.0, dtype=np.float32)
    buf = DeviceBuffer(out.nbytes)
    buf.fill(0x5A)
    untouched_device = buf.read(out.shape)
    try:
        def all_refuse(kx, ky):
            t = C.c_uint64(77)
            assert c_resolved_size(device, kx, ky) == (INVALID, -7, -7)
            assert lib.swr_readback_rgb_resolved(ctx, kx, ky, out.ctypes.data) == INVALID
            assert lib.swr_present_rgb_resolved_async(ctx, kx, ky, out.ctypes.data, C.byref(t)) == INVALID and t.value == 77    # no ticket
            assert lib.swr_resolve_rgb_device(ctx, kx, ky, buf.ptr) == INVALID
            assert lib.swr_resolve_rgb_device_async(ctx, kx, ky, buf.ptr) == INVALID
            device.sync()
            assert np.all(out == np.float32(123.0)) and np.array_equal(buf.read(out.shape).view(np.uint32), untouched_device.view(np.uint32))

        for bad in (0, 3, 16, -2):
            all_refuse(bad, 1)
            all_refuse(2, bad)
            with pytest.raises(ValueError):
                win.ResolvedColorBuffer(bad, 2)
        win.Resize(36, 16)                                            # 36 is no multiple of 8
        all_refuse(8, 1)
        assert c_resolved_size(device, 4, 8) == (0, 2, 9)
        win.Resize(40, 20)                                            # nor 20
        all_refuse(1, 8)
        win.Resize(40, 24)
        # NULL pointers
        t, i = C.c_uint64(77), C.c_int(0)
        assert lib.swr_resolved_size(ctx, 2, 2, None, C.byref(i)) == INVALID and lib.swr_resolved_size(ctx, 2, 2, C.byref(i), None) == INVALID
        assert lib.swr_readback_rgb_resolved(ctx, 2, 2, None) == INVALID
        assert lib.swr_present_rgb_resolved_async(ctx, 2, 2, None, C.byref(t)) == INVALID and t.value == 77
        assert lib.swr_present_rgb_resolved_async(ctx, 2, 2, out.ctypes.data, None) == INVALID
        assert lib.swr_resolve_rgb_device(ctx, 2, 2, None) == INVALID and lib.swr_resolve_rgb_device_async(ctx, 2, 2, None) == INVALID
        assert lib.swr_readback_rgb_resolved(None, 2, 2, out.ctypes.data) == INVALID
        # a zero-size target: SWR_OK, nothing written (bad factors are still refused)
        win.Resize(0, 0)
        assert c_resolved_size(device, 8, 8) == (0, 0, 0)
        assert lib.swr_readback_rgb_resolved(ctx, 8, 8, out.ctypes.data) == 0
        assert lib.swr_resolve_rgb_device(ctx, 2, 4, buf.ptr) == 0 and lib.swr_resolve_rgb_device_async(ctx, 2, 4, buf.ptr) == 0
        assert lib.swr_present_rgb_resolved_async(ctx, 2, 2, out.ctypes.data, C.byref(t)) == 0 and t.value != 77
        assert win.PresentWait(t.value)
        assert lib.swr_readback_rgb_resolved(ctx, 3, 8, out.ctypes.data) == INVALID
        assert win.ResolvedColorBuffer(4, 4).shape == (0, 0, 3)
        device.sync()
        assert np.all(out == np.float32(123.0)) and np.array_equal(buf.read(out.shape).view(np.uint32), untouched_device.view(np.uint32))
    finally:
        buf.free()
