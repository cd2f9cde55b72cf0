"""The arithmetic of the stand-alone bilinear_sampler kernel (SURVEY 8b Op D; csrc/sampler.hip) pinned WITHOUT a GPU.

co-tracker_amd/csrc/sampler_math.h holds every floating-point step of the kernel in host/device inline functions.  This test
compiles that header with g++ (-ffp-contract=off, the flag the device translation unit is built with) behind a plain loop
(tests/host/sampler_host.cpp) and compares it BIT FOR BIT with what the reference's bilinear_sampler (model_utils.py:191-255)
computes on the CPU -- torch.nn.functional.grid_sample after the reference's coordinate scaling -- for 4-D and 5-D inputs,
align_corners True / False, padding "zeros" / "border", coordinates inside, on, and far outside the image, exact integers and
half-integers; then replays the reference's own unit test (tests/test_bilinear_sample.py:16-47).  The restated bilinear_sampler
below is itself checked against the reference's: tests/golden/bilinear_sampler.npz holds what the imported reference returned
(tests/golden/make_golden_reference.py).
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ctk_support import host_library


def ref_bilinear_sampler(input, coords, align_corners=True, padding_mode="border"):
    """model_utils.py:191-255, restated (test oracle): reorder (t,x,y)->(x,y,t), scale to [-1,1], F.grid_sample."""
    sizes = input.shape[2:]
    if len(sizes) == 3:
        coords = coords[..., [1, 2, 0]]
    if align_corners:
        coords = coords * torch.tensor([2 / max(size - 1, 1) for size in reversed(sizes)])
    else:
        coords = coords * torch.tensor([2 / size for size in reversed(sizes)])
    coords = coords - 1
    return F.grid_sample(input, coords, align_corners=align_corners, padding_mode=padding_mode)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = host_library(tmp_path_factory, "sampler")
    lib.host_bilinear_sampler.restype = C.c_int
    lib.host_bilinear_sampler.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_int, C.c_int,
                                          C.c_void_p]

    def run(inp, coords, align, pad):
        inp = inp.contiguous().float()
        coords = coords.contiguous().float()
        B, Cc = inp.shape[:2]
        sizes = inp.shape[2:]
        D = sizes[0] if len(sizes) == 3 else 0
        inner = tuple(coords.shape[1:-1])
        P = int(np.prod(inner))
        out = torch.empty((B, Cc) + inner)
        lib.host_bilinear_sampler(inp.data_ptr(), B, Cc, D, sizes[-2], sizes[-1], coords.data_ptr(), P, int(align), int(pad == "border"),
                                  out.data_ptr())
        return out

    return run


def _coords(g, n, sizes, nd):
    """(x,y) or (t,x,y) rows: uniform over [-1.5, size+0.5], plus exact integers, half-integers and the borders."""
    ext = [sizes[-1], sizes[-2]] if nd == 2 else [sizes[0], sizes[-1], sizes[-2]]
    c = torch.stack([torch.rand(n, generator=g) * (e + 2.0) - 1.5 for e in ext], dim=1)
    k = n // 4
    c[:k] = c[:k].round()
    c[k:2 * k] = c[k:2 * k].round() + 0.5
    for j, e in enumerate(ext):
        c[2 * k + j, j] = float(e - 1)
        c[2 * k + 4 + j, j] = 0.0
        c[2 * k + 8 + j, j] = float(e)
    return c


@pytest.mark.parametrize("pad", ["border", "zeros"])
@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("nd", [2, 3])
def test_host_build_of_the_kernel_arithmetic_is_bit_identical_to_grid_sample(host, nd, align, pad):
    g = torch.Generator().manual_seed(100 * nd + 10 * int(align) + (pad == "zeros"))
    for sizes in ([(12, 16), (1, 5), (7, 1)] if nd == 2 else [(5, 12, 16), (1, 9, 7), (3, 1, 4)]):
        inp = torch.randn((2, 3) + sizes, generator=g)
        n = 4096
        c = torch.stack([_coords(g, n, sizes, nd) for _ in range(2)])
        coords = c.view(2, 64, 64, nd) if nd == 2 else c.view(2, 16, 16, 16, nd)
        ref = ref_bilinear_sampler(inp, coords, align, pad)
        out = host(inp, coords, align, pad)
        assert out.shape == ref.shape
        bad = (out.view(torch.int32) != ref.view(torch.int32)) & ~((out == 0) & (ref == 0))  # (+0 / -0 are the same sample)
        assert int(bad.sum()) == 0, (sizes, int(bad.sum()), float((out - ref).abs().max()))


def test_reference_unit_test_replayed_on_the_host_build(host):
    """cotracker tests/test_bilinear_sample.py:16-47: identity sampling of an image (4-D) and a video (5-D), both conventions."""
    for align in (True, False):
        H, W = 4, 5
        inp = torch.randn(H * W).view(1, 1, H, W)
        coords = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        coords = torch.stack(coords[::-1], dim=-1).float()[None]
        if not align:
            coords = coords + 0.5
        torch.testing.assert_close(inp, host(inp, coords, align, "border"))
        T = 3
        vid = torch.stack([inp, inp + 1, inp + 2], dim=2)
        c5 = torch.meshgrid(torch.arange(T), torch.arange(W), torch.arange(H), indexing="ij")
        c5 = torch.stack(c5, dim=-1).float().permute(0, 2, 1, 3)[None]
        if not align:
            c5 = c5 + 0.5
        torch.testing.assert_close(vid, host(vid, c5, align, "border"))


def restated_oracle_cases():
    """name -> (input, coords, align_corners, padding_mode): 4-D and 5-D inputs, both conventions, both paddings."""
    g = torch.Generator().manual_seed(3)
    cases = {}
    for nd, sizes in ((2, (9, 11)), (3, (4, 9, 11))):
        inp = torch.randn((1, 2) + sizes, generator=g)
        c = _coords(g, 256, sizes, nd).view((1, 16, 16, nd) if nd == 2 else (1, 4, 8, 8, nd))
        for align in (True, False):
            for pad in ("border", "zeros"):
                cases[f"{nd}d_align{int(align)}_{pad}"] = (inp, c, align, pad)
    return cases


def test_restated_oracle_equals_the_imported_reference(golden):
    g = golden("bilinear_sampler")
    cases = restated_oracle_cases()
    assert len(cases) == 8
    for name, (_, _, align, pad) in cases.items():
        # the stored inputs, so that the comparison does not hang on the random stream of the torch that runs the test
        inp, c = torch.from_numpy(g[name + "/input"]), torch.from_numpy(g[name + "/coords"])
        assert torch.equal(torch.from_numpy(g[name + "/out"]), ref_bilinear_sampler(inp, c, align, pad)), name
