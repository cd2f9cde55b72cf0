"""The arithmetic of the frame-ingest kernel (csrc/ingest.hip) pinned WITHOUT a GPU.

co-tracker_amd/csrc/ingest_math.h holds every floating-point step of the kernel in host/device inline functions.  This test compiles
that header with g++ (-ffp-contract=off, the flag the device translation unit is built with) behind the kernel's loop
(tests/host/ingest_host.cpp) and compares it
  * with a float64 evaluation that follows the float32 COORDINATE arithmetic (the rule of oracle/window_fp64.py for tap positions: a
    float64 coordinate would move the taps by 1e-2 grey levels at 1080p and prove nothing) and blends in float64: 3 ulp of the value;
  * with torch's F.interpolate(bilinear, align_corners=True) on the CPU, the call the predictor makes: the same bar -- and, for the
    sizes the predictor sees, bit for bit (the FMA placement of ingest_math.h was read off torch's results);
for uint8 and float32 sources, both layouts, strided sources, down- and upscaling, identity, one-row / one-column outputs, and checks
that the last row and column never read past the image.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from ctk_support import fp64_resize, host_library, nchw, source, ulps


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = host_library(tmp_path_factory, "ingest")
    lib.host_ingest_frames.restype = C.c_int
    lib.host_ingest_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_void_p, C.c_int,
                                       C.c_int, C.c_void_p]

    def run(src, layout, size, want_top=False):
        """src: uint8 / float32 tensor [F,H,W,3] ("hwc") or [F,3,H,W] ("chw"), possibly a strided view -> [F,3,h,w] float32."""
        hwc = layout == "hwc"
        Fn, H, W = (src.shape[0], src.shape[1], src.shape[2]) if hwc else (src.shape[0], src.shape[2], src.shape[3])
        if hwc:
            assert src.stride(3) == 1 and src.stride(2) == 3
            fs, rs = src.stride(0), src.stride(1)
        else:
            assert src.stride(3) == 1 and src.stride(1) == H * src.stride(2)
            fs, rs = src.stride(0), src.stride(2)
        out = torch.empty(Fn, 3, *size)
        top = C.c_long(0)
        lib.host_ingest_frames(src.data_ptr(), 0 if src.dtype == torch.uint8 else 1, int(hwc), Fn, H, W, fs, rs, out.data_ptr(), size[0],
                               size[1], C.byref(top))
        return (out, top.value) if want_top else out

    return run


CASES = [  # (H, W, h, w)
    (1080, 1920, 384, 512), (480, 640, 384, 512), (100, 100, 384, 512), (37, 53, 19, 31), (64, 96, 64, 96),
    (50, 70, 1, 40), (50, 70, 30, 1), (50, 70, 1, 1), (1, 1, 8, 12), (2, 3, 7, 9),
]


@pytest.mark.parametrize("H,W,h,w", CASES)
@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_against_fp64_and_torch(host, dtype, layout, H, W, h, w):
    src = source(dtype, layout, 1 if H > 500 else 2, H, W, seed=H + w)
    got = host(src, layout, (h, w))
    x = nchw(src, layout)
    assert ulps(got, fp64_resize(x, (h, w))) <= 3.0
    ref = F.interpolate(x, (h, w), mode="bilinear", align_corners=True)
    assert ulps(got, ref) <= 3.0
    # torch's CPU kernel takes other code paths (other roundings, inside the bar) for one-sample axes and for images a few pixels
    # wide; at the sizes a predictor sees it gives the bits of its GPU kernel, which ingest_math.h restates
    if (H, W, h, w) in CASES[:5]:
        assert torch.equal(got, ref), "the FMA placement of ingest_math.h no longer gives torch's bits"


@pytest.mark.parametrize("layout,pad", [("hwc", (5, 7)), ("hwc", (0, 11)), ("chw", (0, 9))])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_strided_source_equals_its_dense_copy(host, dtype, layout, pad):
    src = source(dtype, layout, 3, 60, 80, seed=5, pad=pad)
    assert not src.is_contiguous()
    assert torch.equal(host(src, layout, (24, 32)), host(src.contiguous(), layout, (24, 32)))
    assert torch.equal(host(src[1:], layout, (24, 32)), host(src, layout, (24, 32))[1:])  # frames are independent


def test_uint8_equals_float_of_uint8(host):
    for layout in ("hwc", "chw"):
        src = source(torch.uint8, layout, 2, 45, 61, seed=9)
        assert torch.equal(host(src, layout, (32, 48)), host(src.float(), layout, (32, 48)))


def test_layouts_agree(host):
    src = source(torch.uint8, "hwc", 2, 45, 61, seed=11)
    assert torch.equal(host(src, "hwc", (32, 48)), host(src.permute(0, 3, 1, 2).contiguous(), "chw", (32, 48)))


@pytest.mark.parametrize("H,W", [(64, 96), (1, 1), (7, 1), (384, 512)])
def test_identity_size_is_an_exact_copy(host, H, W):
    for dtype in (torch.uint8, torch.float32):
        src = source(dtype, "hwc", 1, H, W, seed=3)
        assert torch.equal(host(src, "hwc", (H, W)), nchw(src, "hwc"))


@pytest.mark.parametrize("H,W,h,w", CASES + [(1080, 1920, 1080, 1920), (3, 3, 1000, 1000), (1000, 1000, 3, 3)])
def test_never_reads_past_the_image(host, H, W, h, w):
    """The largest element index read is the last element of the last frame at most -- and exactly that one when the output has
    more than one row and column (align_corners: the last output sample IS the last input sample)."""
    for layout in ("hwc", "chw"):
        src = torch.zeros((2, H, W, 3) if layout == "hwc" else (2, 3, H, W), dtype=torch.uint8)
        _, top = host(src, layout, (h, w), want_top=True)
        assert top <= src.numel() - 1
        if h > 1 and w > 1:
            assert top == src.numel() - 1
