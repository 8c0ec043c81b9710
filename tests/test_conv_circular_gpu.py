"""Circular padding (force_circular_padding; ConvGeom.circular) through the conv GEMMs, in the manner of
test_conv_index_gpu.py: integer-valued bf16 operands in [-3, 3], float64 torch reference, torch.equal.  The reference is
F.pad(src, mode="circular") followed by an unpadded F.conv2d (for upsample: the explicitly upsampled source is padded),
and its float64 autograd gradients.

Images 2 x 2 x 2 (both margins wrap onto the same two rows), 2 x 3 x 5 and 3 x 5 x 6 (N >= 2: a wrap into the
neighbouring image shows; H != W: swapped axes show; odd sizes under stride 2: a wrapped gradient coordinate that
multiplies back), Cin 8 (K = 72: a tail K tile) and 72, through the 256x256 and the 128x128 tile and the native host
layer's plan.

Network level: with every conv wrapping, the tiny SD 1.5 / SDXL UNets are translation-equivariant on the torus, so a
latent rolled by a multiple of the total downsampling factor gives the rolled output, up to bf16 rounding and summation
order: both runs lie within _grad_parity.REL_BOUND of the same exact value, so within twice it of each other.  The same
check with zero padding must exceed the bound (measured on MI355X, 16 x 16 latent rolled by 8: see DESIGN.md)."""
import functools
import json

import pytest
import torch
import torch.nn.functional as F

import _grad_parity as GP
from onetrainer_amd import kernels as K
from onetrainer_amd.module import unet as U
from onetrainer_amd.util.config.TrainConfig import TrainConfig
from test_gemm_exact_gpu import Case, conv_src, force_plan, gen, ints, nchw, nhwc, same  # noqa: F401

gpu = pytest.mark.gpu

PLANS = (0, 4, "native")            # 256x256 and 128x128 (csrc/gemm_tiles.h), and the default plan of the native layer
IMAGES = ((2, 2, 2), (2, 3, 5), (3, 5, 6))    # N, H, W
CINS = (8, 72)
COUT = 40
GEOMS = ((3, 1, 1, False), (3, 2, 1, False), (3, 1, 1, True))   # ksize, stride, pad, upsample


@functools.lru_cache(maxsize=None)
def circular_case(img, Cin, geom):
    k, stride, pad, up = geom
    n, H, W = img
    g = gen("conv-circular", img, Cin, geom)
    x, w = ints((n, H, W, Cin), -3, 3, g), ints((COUT, k, k, Cin), -3, 3, g)
    src, w64 = conv_src(x, (k, stride, pad, up, None)).requires_grad_(), nchw(w).requires_grad_()
    y = F.conv2d(F.pad(src, (pad,) * 4, mode="circular"), w64, None, stride=stride, padding=0)
    c = Case(x=x, w=w, dy=ints((n, *y.shape[2:], COUT), -3, 3, g))
    y.backward(nchw(c.dy))
    c["fwd"], c["wgrad"] = nhwc(y.detach()), nhwc(w64.grad)
    if not up:
        c["dgrad"] = nhwc(src.grad)
    return c


def cases(with_upsample=True):
    return [(img, Cin, geom) for img in IMAGES for Cin in CINS for geom in GEOMS if with_upsample or not geom[3]]


def test_preconditions_and_config():
    """pad <= H, W and 2 pad <= k - 1 are refused by the launcher before anything is read; a reference JSON's
    force_circular_padding is a field, not an ignored extra"""
    x, w = torch.zeros(1, 2, 2, 8, dtype=torch.bfloat16), torch.zeros(8, 3, 3, 8, dtype=torch.bfloat16)
    for pad in (2, 3):   # 2 pad > k - 1; pad > H
        with pytest.raises(ValueError, match="circular"):
            K.conv2d(x, w, pad=pad, circular=True)
        with pytest.raises(ValueError, match="circular"):
            K.conv2d_dgrad(x, w, (2, 2), pad=pad, circular=True)
        with pytest.raises(ValueError, match="circular"):
            K.conv2d_wgrad(x, x, 3, pad=pad, circular=True)
    cfg = TrainConfig().from_dict(json.loads('{"force_circular_padding": true}'))
    assert cfg.force_circular_padding is True and "force_circular_padding" not in cfg.extra
    assert TrainConfig.default_values().force_circular_padding is False
    assert TrainConfig().from_dict(cfg.to_settings_dict()).force_circular_padding is True


@gpu
@pytest.mark.parametrize("plan", PLANS)
def test_conv_fwd_circular_exact(dev, force_plan, plan):
    with force_plan(plan) as st:
        for img, Cin, geom in cases():
            k, stride, pad, up = geom
            c = circular_case(img, Cin, geom)
            d = c.on(dev)
            same(st.run(K.conv2d, d.x, d.w, stride=stride, pad=pad, upsample=up, circular=True), c.fwd,
                 f"circular conv fwd {plan} image {img} Cin={Cin} {geom}")
        assert not st.unsupported
        st.done()


@gpu
@pytest.mark.parametrize("plan", PLANS)
def test_conv_dgrad_circular_exact(dev, force_plan, plan):
    with force_plan(plan) as st:
        for img, Cin, geom in cases(with_upsample=False):
            k, stride, pad, _ = geom
            c = circular_case(img, Cin, geom)
            d = c.on(dev)
            same(st.run(K.conv2d_dgrad, d.dy, d.w, img[1:], stride, pad, circular=True), c.dgrad,
                 f"circular conv dgrad {plan} image {img} Cin={Cin} {geom}")
        assert not st.unsupported
        st.done()


@gpu
@pytest.mark.parametrize("plan", PLANS)
def test_conv_wgrad_circular_exact(dev, force_plan, plan):
    with force_plan(plan) as st:
        for img, Cin, geom in cases():
            k, stride, pad, up = geom
            c = circular_case(img, Cin, geom)
            d = c.on(dev)
            for sp in (1, 2):
                same(st.run(K.conv2d_wgrad, d.dy, d.x, k, stride, pad, upsample=up, splits=sp, circular=True), c.wgrad,
                     f"circular conv wgrad {plan} image {img} Cin={Cin} {geom} splits={sp}")
        assert not st.unsupported
        st.done()


@gpu
@pytest.mark.parametrize("plan", PLANS)
def test_out_hw_zeros_are_not_wrapped(dev, force_plan, plan):
    """pad 0, stride 2, out_hw = (H/2, W/2) (the VAE Downsample2D form): the zero row and column stay zeros"""
    g = gen("conv-circular out_hw")
    x, w = ints((2, 4, 6, 8), -3, 3, g).to(dev), ints((COUT, 3, 3, 8), -3, 3, g).to(dev)
    with force_plan(plan) as st:
        on = st.run(K.conv2d, x, w, stride=2, pad=0, out_hw=(2, 3), circular=True)
        off = st.run(K.conv2d, x, w, stride=2, pad=0, out_hw=(2, 3))
        assert torch.equal(on, off)
        st.done()


# ---- network level: roll equivariance -------------------------------------------------------------
LATENT, SHIFT = 16, 8                # both tiny UNets downsample once: any even shift; half the image
ROLL_BOUND = 2 * GP.REL_BOUND        # two bf16 runs, each within REL_BOUND of the same exact value


@gpu
@pytest.mark.parametrize("cfgname", ["tiny_sd15", "tiny_sdxl"])
def test_unet_is_roll_equivariant_only_with_circular_padding(dev, cfgname):
    cfg = getattr(U, cfgname + "_config")()
    assert SHIFT % 2 ** (len(cfg.block_out_channels) - 1) == 0
    m = U.UNet2DConditionModel(cfg, dev, seed=1, trainable=False)
    g = gen("conv-circular roll", cfgname)
    B = 2
    x = torch.zeros(B, LATENT, LATENT, 8, dtype=torch.bfloat16)
    x[..., :4] = torch.randn(B, LATENT, LATENT, 4, generator=g)
    t = torch.tensor([10, 700], dtype=torch.int32, device=dev)
    ehs = torch.randn(B, 77, cfg.cross_attention_dim, generator=g).to(dev).bfloat16()
    te = tid = None
    if cfg.addition_embed:
        te = torch.randn(B, cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim,
                         generator=g).to(dev).bfloat16()
        tid = torch.tensor([[128., 128., 0., 0., 128., 128.]] * B, device=dev)
    x = x.to(dev)

    def distance(circular):
        m.circular = circular
        with torch.no_grad():
            y = m(x, t, ehs, te, tid)[..., :4].double()
            yr = m(torch.roll(x, (SHIFT, SHIFT), (1, 2)), t, ehs, te, tid)[..., :4].double()
        return ((yr - torch.roll(y, (SHIFT, SHIFT), (1, 2))).norm() / y.norm()).item()

    on, off = distance(True), distance(False)
    print(f"ROLL {cfgname}: circular {on:.5f}, zero padding {off:.5f}, bound {ROLL_BOUND:.3f}")
    assert on <= ROLL_BOUND, f"{cfgname}: not roll-equivariant with circular padding: {on} > {ROLL_BOUND}"
    assert off > ROLL_BOUND, f"{cfgname}: the check cannot fail: zero padding gives {off} <= {ROLL_BOUND}"
