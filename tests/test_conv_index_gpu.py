"""Exact conv products on geometries that stress the carried gather indices (csrc/gemm2_stage.h offsets_step), in the
manner of test_gemm_exact_gpu.py: integer-valued bf16 operands, float64 torch reference, torch.equal.

The images the existing exact tests lack: 2 x 3 x 70 (an image row wider than one 64-deep K-step: the wgrad pixel
counter carries into the row digit less than once per step) and 3 x 5 x 6 (30 pixels per image: more than one image per
K-step, the image digit advances by 2 or 3), with Cin 72 and 192 (64 = 0 taps + 64 channels: the channel digit carries
into the tap column on most steps, for 72, and on every third, for 192).  Forward, input gradient and weight gradient
through one 256-wide tile (256x256, 8 waves) and one 128-wide tile (128x128), forced as that file forces them; the weight
gradient with 1, 2 and 3 splits whose boundaries fall inside an image row."""
import functools

import pytest
import torch
import torch.nn.functional as F

from onetrainer_amd import kernels as K
from test_gemm_exact_gpu import Case, conv_src, eff_splits, force_plan, gen, ints, nchw, nhwc, same  # noqa: F401

gpu = pytest.mark.gpu

TILES = (0, 4)                      # 256x256 and 128x128 (csrc/gemm_tiles.h)
IMAGES = ((2, 3, 70), (3, 5, 6))    # N, H, W
CINS = (72, 192)
COUT = 152
G_S1, G_S2, G_UP = (3, 1, 1, False), (3, 2, 1, False), (3, 1, 1, True)   # ksize, stride, pad, upsample


@functools.lru_cache(maxsize=None)
def conv_case(img, Cin, geom):
    k, stride, pad, up = geom
    n, H, W = img
    g = gen("conv-index", img, Cin, geom)
    x, w = ints((n, H, W, Cin), -3, 3, g), ints((COUT, k, k, Cin), -3, 3, g)
    src = conv_src(x, (k, stride, pad, up, None))
    fwd = nhwc(F.conv2d(src, nchw(w), None, stride=stride, padding=pad))
    P, Q = fwd.shape[1:3]
    c = Case(x=x, w=w, dy=ints((n, P, Q, COUT), -3, 3, g))
    c["fwd"] = fwd
    if not up:
        c["dgrad"] = nhwc(torch.nn.grad.conv2d_input((n, Cin, H, W), nchw(w), nchw(c.dy), stride=stride, padding=pad))
    c["wgrad"] = nhwc(torch.nn.grad.conv2d_weight(src, (COUT, Cin, k, k), nchw(c.dy), stride=stride, padding=pad))
    return c


def test_split_boundaries_fall_inside_an_image_row():
    """the reference-only precondition, on the CPU: with the 70-wide rows the launcher's 2 and 3 splits begin at pixel
    256, and at 192 and 384 -- columns 46, 52 and 34 of a row; with 5 x 6 images 2 splits begin at pixel 64, column 4"""
    assert [eff_splits(420, s) for s in (2, 3)] == [2, 3] and 256 % 70 and 192 % 70 and 384 % 70
    assert eff_splits(90, 2) == 2 and 64 % 6


@gpu
@pytest.mark.parametrize("img", IMAGES)
@pytest.mark.parametrize("tile", TILES)
def test_conv_fwd_index_exact(dev, force_plan, tile, img):
    with force_plan(tile) as st:
        for Cin in CINS:
            for geom in (G_S1, G_S2, G_UP):
                k, stride, pad, up = geom
                c = conv_case(img, Cin, geom)
                d = c.on(dev)
                same(st.run(K.conv2d, d.x, d.w, stride=stride, pad=pad, upsample=up), c.fwd,
                     f"conv fwd tile {tile} image {img} Cin={Cin} {geom}")
        assert not st.unsupported
        st.done()


@gpu
@pytest.mark.parametrize("img", IMAGES)
@pytest.mark.parametrize("tile", TILES)
def test_conv_dgrad_index_exact(dev, force_plan, tile, img):
    n, H, W = img
    with force_plan(tile) as st:
        for Cin in CINS:
            for geom in (G_S1, G_S2):
                k, stride, pad, _ = geom
                c = conv_case(img, Cin, geom)
                d = c.on(dev)
                same(st.run(K.conv2d_dgrad, d.dy, d.w, (H, W), stride, pad), c.dgrad,
                     f"conv dgrad tile {tile} image {img} Cin={Cin} {geom}")
        assert not st.unsupported
        st.done()


@gpu
@pytest.mark.parametrize("img", IMAGES)
@pytest.mark.parametrize("tile", TILES)
def test_conv_wgrad_index_exact(dev, force_plan, tile, img):
    with force_plan(tile) as st:
        for Cin in CINS:
            for geom in (G_S1, G_S2, G_UP):
                k, stride, pad, up = geom
                c = conv_case(img, Cin, geom)
                d = c.on(dev)
                for sp in (1, 2, 3):
                    tag = f"conv wgrad tile {tile} image {img} Cin={Cin} {geom} splits={sp}"
                    same(st.run(K.conv2d_wgrad, d.dy, d.x, k, stride, pad, upsample=up, splits=sp), c.wgrad, tag)
                    bg = torch.full((COUT,), float("nan"), device=dev)   # the colsum instance of the same tile
                    dw = st.run(K.conv2d_wgrad, d.dy, d.x, k, stride, pad, upsample=up, splits=sp, bias_grad=bg)
                    same(dw, c.wgrad, tag + " with the bias gradient")
                    same(bg, c.dy.double().sum((0, 1, 2)), tag + ": the bias gradient")
        assert not st.unsupported
        st.done()
