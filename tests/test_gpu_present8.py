"""8-bit present on the GPU (include/swr.h, csrc/swr_deliver.hip.h): k_present8 against the numpy restatement of
tests/present8_cases.py, byte for byte and without a tolerance, through every entry point: swr_readback_rgb8,
swr_resolve_rgb8_device[_async], swr_present_rgb8_async, swr_present8_size."""
import ctypes as C
import functools

import numpy as np
import pytest

import present8_cases as K
from softwarerenderer_amd import MainWindow, _native, multigpu, scenes

pytestmark = pytest.mark.gpu

# partial last tile row and column; output widths 5 and 17 (groups of four pixels straddle rows); a wave tail (1032 = 16 * 64 + 8);
# output pixel counts mod 4 of 3 (40x24 at (8, 8): 15), 2 (at (8, 4): 30) and 1 (136x72 at (8, 8): 153): every tail length
SIZES = [(40, 24), (136, 72), (1032, 16)]
CANARY = 0xA5
GUARD = 64


@functools.lru_cache(maxsize=None)
def plane(width, height, seed):
    p = K.tie_plane(height, width, seed)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def want(width, height, seed, kx, ky, bpp):
    w = K.present8(plane(width, height, seed), kx, ky, bpp)
    w.setflags(write=False)
    return w


def same_bytes(got, expect, what=""):
    assert got.dtype == np.uint8 and got.shape == expect.shape, (what, got.dtype, got.shape, expect.shape)
    bad = np.argwhere(got != expect)
    assert bad.size == 0, (what, f"{len(bad)} bytes differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]} want {expect[tuple(bad[0])]}")


def c_present8_size(device, kx, ky, bpp):
    w, rows, nbytes = C.c_int(-7), C.c_int(-7), C.c_size_t(7)
    rc = device._lib.swr_present8_size(device._ctx, kx, ky, bpp, C.byref(w), C.byref(rows), C.byref(nbytes))
    return rc, rows.value, w.value, nbytes.value


class DeviceBytes:
    """Caller-owned device memory straight from the HIP runtime the library already loaded."""

    def __init__(self, nbytes):
        self.hip, self.nbytes, self.ptr = C.CDLL("libamdhip64.so"), nbytes, C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(nbytes)) == 0

    def fill(self, byte):
        assert self.hip.hipMemset(self.ptr, C.c_int(byte), C.c_size_t(self.nbytes)) == 0
        assert self.hip.hipDeviceSynchronize() == 0                   # the fill is not ordered against the context's stream

    def read(self):
        out = np.empty(self.nbytes, dtype=np.uint8)
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), self.ptr, C.c_size_t(self.nbytes), 2) == 0        # hipMemcpyDeviceToHost
        return out

    def free(self):
        self.hip.hipFree(self.ptr)


def check_all_pairs(device, width, height, seed, guarded_device=True):
    """Every factor pair and both formats on one uploaded plane.  The host destination sits at an odd address between two guards;
    the device destination has a guard behind it that is read back separately."""
    win = MainWindow(device, width, height)
    win.Upload(color=plane(width, height, seed))
    lib, ctx = device._lib, device._ctx
    host = np.empty(GUARD + width * height * 4 + GUARD, dtype=np.uint8)
    dbuf = DeviceBytes(width * height * 4 + GUARD) if guarded_device else None
    try:
        for kx, ky in K.PAIRS:
            for bpp in (3, 4):
                expect = want(width, height, seed, kx, ky, bpp)
                rows, ow = height // ky, width // kx
                n = rows * ow * bpp
                assert c_present8_size(device, kx, ky, bpp) == (0, rows, ow, n)
                assert win.Present8Size(kx, ky, bpp) == (rows, ow, bpp)
                host[:] = CANARY
                first = GUARD + 1                                      # any alignment
                assert lib.swr_readback_rgb8(ctx, kx, ky, bpp, host.ctypes.data + first) == 0
                same_bytes(host[first:first + n].reshape(rows, ow, bpp), expect, (width, height, kx, ky, bpp))
                assert np.all(host[:first] == CANARY) and np.all(host[first + n:] == CANARY), (kx, ky, bpp, "host guard")
                if dbuf is not None:
                    dbuf.fill(CANARY)
                    assert lib.swr_resolve_rgb8_device(ctx, kx, ky, bpp, dbuf.ptr) == 0
                    device.sync()
                    back = dbuf.read()
                    same_bytes(back[:n].reshape(rows, ow, bpp), expect, (width, height, kx, ky, bpp, "device"))
                    assert np.all(back[n:] == CANARY), (kx, ky, bpp, "device guard")
    finally:
        if dbuf is not None:
            dbuf.free()


@pytest.mark.parametrize("width,height", SIZES)
def test_every_factor_pair_and_format_equals_the_restatement_and_stays_inside(device, width, height):
    check_all_pairs(device, width, height, seed=width)


@pytest.mark.parametrize("lib", ["libswr_hip_fma_dpps.so", "libswr_hip_test.so"])
def test_the_numerics_and_test_builds_deliver_the_same_bytes(lib):
    """The numerics switches of the library variants do not touch this arithmetic."""
    from softwarerenderer_amd import Device
    dev = Device(0, lib=lib)
    try:
        check_all_pairs(dev, 136, 72, seed=136, guarded_device=False)
    finally:
        dev.close()


def test_factors_one_one_equal_the_quantised_flatten(device):
    win = MainWindow(device, 136, 72)
    win.Upload(color=plane(136, 72, 136))
    flat = win.FlatColorBuffer()
    for bpp in (3, 4):
        got = win.ColorBuffer8(channels=bpp)
        same_bytes(got[..., :3], K.quantise(flat), bpp)
        assert bpp == 3 or np.all(got[..., 3] == 255)


def test_a_rendered_frame_is_flushed_and_then_delivered(device):
    s = scenes.cfg2(256, 192, 400, seed=31)
    r = scenes.SceneRenderer(device, s)
    r.window.Upload(color=np.full((192, 256, 4), 0.25, dtype=np.float32))
    r.submit_frame()                                                  # recorded, not flushed: the plane still holds 0.25 everywhere
    got = r.window.ColorBuffer8(2, 2, 3)
    color = r.window.ColorBuffer
    assert len(np.unique(color[..., :3])) > 100                       # the frame has content ...
    assert not np.all(got == 64)                                      # ... and the present saw it (0.25 * 255 = 63.75 -> 64)
    same_bytes(got, K.present8(color, 2, 2, 3))
    same_bytes(r.window.ColorBuffer8(1, 1, 4), K.present8(color, 1, 1, 4))
    r.close()


def test_device_variants_write_the_same_bytes(device):
    s = scenes.cfg2(200, 120, 300, seed=12)
    r = scenes.SceneRenderer(device, s)
    color = r.render()[0]
    for (kx, ky, bpp) in ((4, 2, 3), (1, 1, 4)):
        expect = K.present8(color, kx, ky, bpp)
        assert r.window.Present8Size(kx, ky, bpp) == expect.shape
        n = expect.size
        buf = DeviceBytes(n + GUARD)
        try:
            buf.fill(CANARY)
            r.submit_frame()
            r.window.Quantise8To(buf.ptr.value, kx, ky, bpp)
            device.sync()
            back = buf.read()
            same_bytes(back[:n].reshape(expect.shape), expect, "swr_resolve_rgb8_device")
            assert np.all(back[n:] == CANARY)
            buf.fill(CANARY)
            r.submit_frame()
            s0 = device.sync_count()
            r.window.Quantise8ToAsync(buf.ptr.value, kx, ky, bpp)
            assert device.sync_count() == s0                          # the async variant does not wait for the stream
            device.sync()
            back = buf.read()
            same_bytes(back[:n].reshape(expect.shape), expect, "swr_resolve_rgb8_device_async")
            assert np.all(back[n:] == CANARY)
        finally:
            buf.free()
    r.close()


# which present each frame of the alternation test makes; a slot serves every second present, so both orders grow a staging buffer
# that another kind of payload sized: small 8-bit first and a larger float one on the same slot, and the reverse
ORDERS = {"bytes_then_floats": ["rgb8", "rgbx8", "plain", "plain", "resolved", "rgb8", "plain", "rgbx8", "resolved"],
          "floats_then_bytes": ["plain", "plain", "rgb8", "rgbx8", "resolved", "plain", "rgb8", "resolved", "rgbx8"]}


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_float_resolved_and_8_bit_presents_alternate_on_the_shared_slots(order):
    """256 x 192: the 8-bit presents share swr_present_rgb_async's two slots, tickets and staging buffers (sized in bytes) with the
    float kinds.  Present i, wait i - 2; tickets stay in order, every buffer ends up with exactly its frame's payload, and no present
    call makes the host wait for the stream."""
    from softwarerenderer_amd import Device
    dev = Device(0)                                                   # a fresh context: its staging buffers start empty
    a = scenes.cfg3(256, 192, (2, 2), (20, 14), tex_size=64, seed=91)
    b = scenes.cfg2(256, 192, 800, seed=92)
    ra = scenes.SceneRenderer(dev, a)
    rb = scenes.SceneRenderer(dev, b, window=ra.window)
    win = ra.window
    frames = [ra.render()[0].copy(), rb.render()[0].copy()]           # synchronous frames first: sizes the pair buffers too
    expect = {"plain": lambda f: f[..., :3].copy(), "resolved": lambda f: K.R.resolve(f, 2, 2),
              "rgb8": lambda f: K.present8(f, 2, 2, 3), "rgbx8": lambda f: K.present8(f, 1, 1, 4)}
    pinned = []

    def present(kind, k):
        w = expect[kind](frames[k])
        out = np.zeros_like(w)
        dev.pin(out); pinned.append(out)
        s0 = dev.sync_count()
        if kind == "plain":
            t = win.PresentAsync(out)
        elif kind == "resolved":
            t = win.PresentResolvedAsync(out, 2, 2)
        else:
            t = win.Present8Async(out, *((2, 2) if kind == "rgb8" else (1, 1)))
        assert dev.sync_count() == s0                                 # never waits for the stream
        return t, out, w

    def settle(entry, what):
        t, out, w = entry
        assert win.PresentWait(t)
        if out.dtype == np.uint8:
            same_bytes(out, w, what)
        else:
            K.R.assert_same_words(out, w, what)

    try:
        pending = []
        for i, kind in enumerate(ORDERS[order]):
            k = (i // 2) & 1
            (ra, rb)[k].submit_frame()
            if len(pending) == 2:
                settle(pending.pop(0), (order, i - 2))
            pending.append(present(kind, k))
            if len(pending) == 2:
                assert pending[1][0] == pending[0][0] + 1             # one ticket sequence for every kind
        for entry in pending:
            settle(entry, (order, "tail"))
        assert win.PresentWait(pending[-1][0])                        # waiting twice for a ticket is harmless
    finally:
        for x in pinned:
            dev.unpin(x)
    ra.close(); rb.close(); dev.close()


def test_8_bit_present_reports_a_stale_frame_after_a_replay():
    """The construction of test_resolved_present_reports_a_stale_frame_after_a_replay (tests/test_gpu_resolve.py) with the 8-bit
    payload: a batch that does not fit poisons itself, the present behind it quantises the UNCHANGED framebuffer, the wait says so
    after replaying, and presenting again delivers the frame."""
    from softwarerenderer_amd import Device
    dev = Device(0)                                                   # a fresh context: its pair buffers start empty
    small = scenes.cfg2(256, 256, 40, seed=60, min_area=10.0, max_area=60.0)
    big = scenes.cfg2(256, 256, 3000, seed=61, min_area=200.0, max_area=9000.0)
    r0 = scenes.SceneRenderer(dev, small)
    r0.render()                                                       # synchronous sizing of the pair buffers (small)
    r1 = scenes.SceneRenderer(dev, big, window=r0.window)
    out = np.zeros((128, 128, 3), dtype=np.uint8)
    before = dev.replay_count()
    r1.submit_frame()                                                 # does not fit: poisoned on the device
    t = r0.window.Present8Async(out, 2, 2)
    assert r0.window.PresentWait(t) is False                          # stale, and the batch has been replayed by now
    assert dev.replay_count() == before + 1
    stale = out.copy()
    t = r0.window.Present8Async(out, 2, 2)                            # the caller's reaction: present again
    assert r0.window.PresentWait(t) is True
    same_bytes(out, K.present8(r0.window.ColorBuffer, 2, 2, 3))
    assert not np.array_equal(stale, out)                             # the first payload really predated the batch
    r0.close(); r1.close(); dev.close()


@pytest.mark.parametrize("kx,ky,bpp", [(2, 8, 3), (8, 2, 4), (4, 4, 3)])
def test_band_payloads_concatenate_to_the_whole_frame(device, kx, ky, bpp):
    """64 x 88: five full tile rows and one of 8 pixel rows.  Contiguous bands of 2 and 3 ranks, and interleaved one-tile-row stripes:
    a band's payload is tightly packed, so the parts concatenate to the frame's bytes."""
    W, H = 64, 88
    win = MainWindow(device, W, H)
    p = plane(W, H, kx * 10 + ky)
    try:
        win.Upload(color=p)
        whole = win.ColorBuffer8(kx, ky, bpp)
        same_bytes(whole, want(W, H, kx * 10 + ky, kx, ky, bpp), "whole frame")
        for world in (2, 3):
            parts = []
            for first, count in multigpu.band_partition(H, world):
                win.SetBand(first, count)
                y0, rows = win.band_pixel_rows()
                assert c_present8_size(device, kx, ky, bpp) == (0, rows // ky, W // kx, (rows // ky) * (W // kx) * bpp)
                win.Upload(color=p[y0:y0 + rows])
                parts.append(win.ColorBuffer8(kx, ky, bpp))
            assert b"".join(x.tobytes() for x in parts) == whole.tobytes(), ("contiguous", world)
            stripes = multigpu.stripe_rows(H, world, 1)
            frame = np.full_like(whole, 123)
            for rank in range(world):
                win.SetBandInterleaved(rank, world, 1)
                rows = stripes[rank]
                assert c_present8_size(device, kx, ky, bpp)[:3] == (0, len(rows) // ky, W // kx)
                win.Upload(color=p[rows])
                frame[rows[::ky] // ky] = win.ColorBuffer8(kx, ky, bpp)           # a stripe's blocks keep their place in the frame
            same_bytes(frame, whole, ("interleaved", world))
    finally:
        win.SetBand(-1, -1)


def test_bad_arguments_are_refused_and_write_nothing(device):
    lib, ctx = device._lib, device._ctx
    INVALID = _native.SWR_ERR_INVALID_ARG
    win = MainWindow(device, 40, 24)
    win.Upload(color=plane(40, 24, 40))
    out = np.full((24, 40, 4), 123, dtype=np.uint8)
    buf = DeviceBytes(out.nbytes)
    buf.fill(0x5A)

    def untouched():
        device.sync()
        return np.all(out == 123) and np.all(buf.read() == 0x5A)

    try:
        def all_refuse(kx, ky, bpp):
            t = C.c_uint64(77)
            assert c_present8_size(device, kx, ky, bpp) == (INVALID, -7, -7, 7)
            assert lib.swr_readback_rgb8(ctx, kx, ky, bpp, out.ctypes.data) == INVALID
            assert lib.swr_present_rgb8_async(ctx, kx, ky, bpp, out.ctypes.data, C.byref(t)) == INVALID and t.value == 77     # no ticket
            assert lib.swr_resolve_rgb8_device(ctx, kx, ky, bpp, buf.ptr) == INVALID
            assert lib.swr_resolve_rgb8_device_async(ctx, kx, ky, bpp, buf.ptr) == INVALID
            assert untouched()

        for bad in (0, 3, 16, -2):
            all_refuse(bad, 1, 3)
            all_refuse(2, bad, 4)
            with pytest.raises(ValueError):
                win.ColorBuffer8(bad, 2)
        for bad_bpp in (0, 1, 2, 5, 12, -3):
            all_refuse(1, 1, bad_bpp)
            all_refuse(2, 2, bad_bpp)
        win.Resize(36, 16)                                            # 36 is no multiple of 8
        all_refuse(8, 1, 3)
        assert c_present8_size(device, 4, 8, 4) == (0, 2, 9, 72)
        win.Resize(40, 20)                                            # nor 20
        all_refuse(1, 8, 4)
        win.Resize(40, 24)
        # a device destination must be 4-byte aligned (a host destination need not be: the first test reads into an odd address)
        for off in (1, 2, 3):
            assert lib.swr_resolve_rgb8_device(ctx, 1, 1, 3, C.c_void_p(buf.ptr.value + off)) == INVALID
            assert lib.swr_resolve_rgb8_device_async(ctx, 2, 2, 4, C.c_void_p(buf.ptr.value + off)) == INVALID
        assert untouched()
        # NULL pointers
        t, i, z = C.c_uint64(77), C.c_int(0), C.c_size_t(0)
        assert lib.swr_present8_size(ctx, 2, 2, 3, None, C.byref(i), C.byref(z)) == INVALID
        assert lib.swr_present8_size(ctx, 2, 2, 3, C.byref(i), None, C.byref(z)) == INVALID
        assert lib.swr_present8_size(ctx, 2, 2, 3, C.byref(i), C.byref(i), None) == INVALID
        assert lib.swr_readback_rgb8(ctx, 2, 2, 3, None) == INVALID
        assert lib.swr_present_rgb8_async(ctx, 2, 2, 3, None, C.byref(t)) == INVALID and t.value == 77
        assert lib.swr_present_rgb8_async(ctx, 2, 2, 3, out.ctypes.data, None) == INVALID
        assert lib.swr_resolve_rgb8_device(ctx, 2, 2, 3, None) == INVALID and lib.swr_resolve_rgb8_device_async(ctx, 2, 2, 3, None) == INVALID
        assert lib.swr_readback_rgb8(None, 2, 2, 3, out.ctypes.data) == INVALID
        # a zero-size target: SWR_OK, nothing written (a bad format or bad factors are still refused)
        win.Resize(0, 0)
        assert c_present8_size(device, 8, 8, 4) == (0, 0, 0, 0)
        assert lib.swr_readback_rgb8(ctx, 8, 8, 3, out.ctypes.data) == 0
        assert lib.swr_resolve_rgb8_device(ctx, 2, 4, 4, buf.ptr) == 0 and lib.swr_resolve_rgb8_device_async(ctx, 2, 4, 3, buf.ptr) == 0
        assert lib.swr_present_rgb8_async(ctx, 2, 2, 3, out.ctypes.data, C.byref(t)) == 0 and t.value != 77
        assert win.PresentWait(t.value)
        assert lib.swr_readback_rgb8(ctx, 3, 8, 3, out.ctypes.data) == INVALID
        assert lib.swr_readback_rgb8(ctx, 2, 2, 5, out.ctypes.data) == INVALID
        assert win.ColorBuffer8(4, 4, 4).shape == (0, 0, 4)
        assert untouched()
    finally:
        buf.free()
