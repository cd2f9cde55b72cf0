"""The arithmetic of the draw kernels (csrc/draw.hip) pinned WITHOUT a GPU.

co-tracker_amd/csrc/draw_math.h holds the quantisation of a position, the two coverage tests and the blend in host/device inline
functions.  This test compiles that header with g++ (-ffp-contract=off, the flag the device translation unit is built with) behind
plain loops (tests/host/draw_host.cpp) and compares it with the numpy restatement of tests/draw_reference.py: integers on both sides,
every comparison exact."""
import ctypes as C

import numpy as np
import pytest

import draw_reference as R
from ctk_support import host_library


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = host_library(tmp_path_factory, "draw")
    lib.host_draw_quant.restype = C.c_int
    lib.host_draw_quant.argtypes = [C.c_float, C.c_float, C.POINTER(C.c_int)]
    lib.host_draw_visible.restype = C.c_int
    lib.host_draw_visible.argtypes = [C.c_float] * 3
    lib.host_draw_mark_mask.restype = None
    lib.host_draw_mark_mask.argtypes = [C.c_int] * 3 + [C.c_void_p]
    lib.host_draw_mark_at.restype = C.c_int
    lib.host_draw_mark_at.argtypes = [C.c_int] * 4
    lib.host_draw_segment_mask.restype = None
    lib.host_draw_segment_mask.argtypes = [C.c_int] * 7 + [C.c_void_p]
    lib.host_draw_blend_table.restype = None
    lib.host_draw_blend_table.argtypes = [C.c_int, C.c_void_p]
    return lib


def quant(host, x, s):
    q = C.c_int(-12345)
    ok = host.host_draw_quant(float(np.float32(x)), float(np.float32(s)), C.byref(q))
    return bool(ok), (q.value if ok else 0)


def test_positions(host):
    nan, inf = float("nan"), float("inf")
    f32 = np.float32
    below = float(np.nextafter(f32(65536.0), f32(0.0)))
    above = float(np.nextafter(f32(65536.0), f32(inf)))
    xs = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49999997, -0.49999997, 0.50000006, 65536.0, -65536.0, below, -below, above, -above, 65535.5,
          -65535.5, 65534.5, nan, inf, -inf, 0.0, -0.0, 3.3e38, -3.3e38, 1e-45, 12.25, 100.75]
    for x in xs:
        assert quant(host, x, 1.0) == R.quant(x, 1.0), x
    # half to even, by hand
    assert [quant(host, x, 1.0)[1] for x in (0.5, -0.5, 1.5, -1.5, 2.5, -2.5)] == [0, 0, 2, -2, 2, -2]
    assert quant(host, 65536.0, 1.0) == (True, 65536) and quant(host, -65536.0, 1.0) == (True, -65536)
    assert not quant(host, above, 1.0)[0] and not quant(host, -above, 1.0)[0]
    for x in (nan, inf, -inf):
        assert not quant(host, x, 1.0)[0] and not quant(host, 1.0, x)[0]
    # the product is ONE float32 multiplication, rounded before the rint: scales that are not representable
    rng = np.random.RandomState(0)
    for x, s in zip(rng.uniform(-600, 2600, 4000).astype(f32), rng.choice([1.37, 0.81, 3.7558594, 2.8120105, 1e3, -40.0], 4000)):
        assert quant(host, x, s) == R.quant(x, s), (x, s)
    for k in range(-40, 41):  # products that land on or next to a half
        for s in (0.5, 0.25, 1.5):
            assert quant(host, k, s) == R.quant(k, s)
    assert quant(host, 3.3e38, 10.0)[0] is False and quant(host, 0.0, inf)[0] is False  # an overflowing product, 0 * inf


def test_visible_rule(host):
    nan = float("nan")
    for v, c, want in ((6.0, 6.0, 1), (6.0, -6.0, 0), (-6.0, 6.0, 0), (-6.0, -6.0, 0), (nan, 6.0, 0), (6.0, nan, 0), (80.0, 80.0, 1),
                       (-200.0, 6.0, 0)):
        assert host.host_draw_visible(v, c, 0.6) == want == int(R.visible_from_logits(v, c, 0.6)), (v, c)
    assert host.host_draw_visible(6.0, 6.0, nan) == 0


@pytest.mark.parametrize("visible", [0, 1])
def test_mark_masks_over_a_full_neighbourhood(host, visible):
    span = 40  # beyond the largest radius: everything outside is uncovered
    d = np.arange(-span, span + 1)
    dy, dx = np.meshgrid(d, d, indexing="ij")
    for r in range(1, 33):
        got = np.empty((2 * span + 1) ** 2, dtype=np.uint8)
        host.host_draw_mark_mask(r, visible, span, got.ctypes.data)
        want = R.mark_mask(dx, dy, r, bool(visible))
        assert np.array_equal(got.reshape(dx.shape).astype(bool), want), r
        assert want[span, span + r] and not want[span, span + r + 1] and want[span, span] == bool(visible)
    # far offsets (a mark at -65536 seen from pixel 32767) do not overflow
    for far in (98303, -98303, 2 ** 31 - 1, -(2 ** 31)):
        assert not host.host_draw_mark_at(far, far, 32, visible) and not host.host_draw_mark_at(0, far, 32, visible)


def segment(host, dx, dy, hw, pad=3):
    x0, x1, y0, y1 = min(dx, 0) - hw - pad, max(dx, 0) + hw + pad, min(dy, 0) - hw - pad, max(dy, 0) + hw + pad
    got = np.empty((y1 - y0 + 1) * (x1 - x0 + 1), dtype=np.uint8)
    host.host_draw_segment_mask(dx, dy, hw, x0, x1, y0, y1, got.ctypes.data)
    py, px = np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")
    return got.reshape(px.shape).astype(bool), R.segment_mask(px, py, dx, dy, hw), (px, py)


def test_every_segment_orientation(host):
    for hw in range(0, 17):
        for dx in range(-6, 7):
            for dy in range(-6, 7):
                got, want, (px, py) = segment(host, dx, dy, hw)
                assert np.array_equal(got, want), (dx, dy, hw)
                # both ends are covered, the frame of `pad` pixels around the bounding box is not
                assert want[(px == 0) & (py == 0)].all() and want[(px == dx) & (py == dy)].all()
                assert not want[0].any() and not want[-1].any() and not want[:, 0].any() and not want[:, -1].any()
    got, want, _ = segment(host, 0, 0, 0)
    assert want.sum() == 1  # dd == 0, hw == 0: a dot of one pixel
    got, want, _ = segment(host, 5, 0, 0)
    assert want.sum() == 6  # hw == 0: the pixels of the line itself


@pytest.mark.parametrize("hw", [0, 1, 16])
def test_max_jump_long_segments(host, hw):
    for dx, dy in ((4095, 4095), (-4095, 4095), (4095, -4094), (4095, 0), (0, -4095), (4095, 1), (-1, 4095), (4095, 2731)):
        # the whole box is 4096^2 pixels: windows around both ends and the middle instead
        for cx, cy in ((0, 0), (dx, dy), (dx // 2, dy // 2), (dx // 3, dy // 3)):
            x0, x1, y0, y1 = cx - 40, cx + 40, cy - 40, cy + 40
            got = np.empty(81 * 81, dtype=np.uint8)
            host.host_draw_segment_mask(dx, dy, hw, x0, x1, y0, y1, got.ctypes.data)
            py, px = np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")
            want = R.segment_mask(px, py, dx, dy, hw)
            assert np.array_equal(got.reshape(81, 81).astype(bool), want), (dx, dy, cx, cy)
            assert not want.all() and (want.any() or (hw == 0 and (cx, cy) not in ((0, 0), (dx, dy))))  # (hw = 0: lattice points only)


def test_blend(host):
    v, c = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for a in (0, 1, 127, 128, 254, 255):
        got = np.empty(256 * 256, dtype=np.uint8)
        host.host_draw_blend_table(a, got.ctypes.data)
        want = np.empty((256, 256), dtype=np.int64)
        for ci in range(256):
            want[:, ci] = R.blend(v[:, ci], ci, a)
        assert want.min() >= 0 and want.max() <= 255
        assert np.array_equal(got.reshape(256, 256), want.astype(np.uint8)), a
        if a == 255:
            assert np.array_equal(want, c)
        if a == 0:
            assert np.array_equal(want, v)
