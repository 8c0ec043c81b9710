"""csrc/inpaint.hip on bits: the 9-channel prologue of the mask-input models against K.ddpm_prologue (channels 0..3,
target, scaled) and torch (mask, conditioning channels), and the masked conditioning image against torch.  Every
output element is one correctly rounded fp32 operation and one bf16 rounding, so no check has a tolerance."""
import pytest
import torch

from onetrainer_amd import kernels as K

pytestmark = pytest.mark.gpu

SF = 0.13025
UNMASK = [0, 1, 0]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _coeffs(dev):
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
    acp = torch.cumprod(1 - betas, 0)
    return tuple(t.float().to(dev) for t in (acp, acp.sqrt(), (1 - acp).sqrt()))


def _inputs(dev, h, w, dtype):
    g = torch.Generator().manual_seed(h * 100 + w)
    B = 3
    lat = (torch.randn(B, h, w, 4, generator=g) * 4).to(dtype).to(dev)
    eps = torch.randn(B, h, w, 4, generator=g).to(dtype).to(dev)
    cond = (torch.randn(B, h, w, 4, generator=g) * 4).to(dtype).to(dev)
    mask = torch.rand(B, h, w, generator=g)
    mask[0, 0, 0], mask[0, -1, -1], mask[2, 0, 1] = 0.0, 1.0, 1.0 / 3.0
    blank = (torch.randn(h, w, 4, generator=g) * 4).to(dev)
    t = torch.tensor([0, 999, 437], dtype=torch.int32, device=dev)
    unmask = torch.tensor(UNMASK, dtype=torch.int32, device=dev)
    return lat, eps, t, mask.to(dev), cond, blank, unmask


@pytest.mark.parametrize("kind", [0, 1], ids=["epsilon", "v_prediction"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("hw", [(5, 3), (16, 16)], ids=["5x3", "16x16"])
def test_inpaint_prologue_bits(dev, hw, dtype, kind):
    h, w = hw
    lat, eps, t, mask, cond, blank, unmask = _inputs(dev, h, w, dtype)
    co = _coeffs(dev)
    nan = torch.full((3, h, w, K.INPAINT_CPAD), float("nan"), dtype=torch.bfloat16, device=dev)
    unet_in, target, scaled, eff = K.inpaint_prologue(lat, eps, t, co, SF, kind, mask, cond, blank, unmask,
                                                      want_mask=True, unet_in=nan)
    assert unet_in.data_ptr() == nan.data_ptr()
    assert not torch.isnan(unet_in.float()).any()   # every element of the NaN-filled output was written
    ri, rt, rs = K.ddpm_prologue(lat, eps, t, co, SF, kind)
    assert torch.equal(_bits(unet_in[..., :4]), _bits(ri[..., :4]))
    assert torch.equal(_bits(target), _bits(rt))
    assert torch.equal(_bits(scaled), _bits(rs))
    um = unmask.bool()[:, None, None]
    want_mask = torch.where(um, torch.ones_like(mask), mask)
    assert torch.equal(_bits(unet_in[..., 4]), _bits(want_mask.bfloat16()))
    assert torch.equal(_bits(eff), _bits(want_mask[:, None]))
    want_cond = torch.where(um[..., None], (blank * SF).bfloat16()[None].expand(3, h, w, 4),
                            (cond.float() * SF).bfloat16())
    assert torch.equal(_bits(unet_in[..., 5:9]), _bits(want_cond))
    assert not _bits(unet_in[..., 9:]).any()   # +0 in every pad channel
    again = K.inpaint_prologue(lat, eps, t, co, SF, kind, mask, cond, blank, unmask, want_mask=True)
    for a, b in zip((unet_in, target, scaled, eff), again):
        assert torch.equal(_bits(a), _bits(b))
    no_mask = K.inpaint_prologue(lat, eps, t, co, SF, kind, mask[:, None], cond, blank, unmask)
    assert no_mask[3] is None and torch.equal(_bits(no_mask[0]), _bits(unet_in))


def test_inpaint_prologue_argument_checks(dev):
    lat, eps, t, mask, cond, blank, unmask = _inputs(dev, 5, 3, torch.float32)
    co = _coeffs(dev)
    ok = (lat, eps, t, co, SF, 0, mask, cond, blank, unmask)
    K.inpaint_prologue(*ok)

    def bad(i, v, match):
        a = list(ok)
        a[i] = v
        with pytest.raises(ValueError, match=match):
            K.inpaint_prologue(*a)

    bad(7, cond.bfloat16(), "cond")                                   # wrong dtype
    bad(6, mask.double(), "latent_mask")
    bad(9, unmask.long(), "unmask")
    bad(2, t.long(), "timestep")
    bad(6, mask.transpose(1, 2), "latent_mask")                       # non-contiguous
    bad(7, cond.permute(0, 2, 1, 3), "cond")
    bad(0, lat.permute(0, 2, 1, 3), "latent")
    bad(8, blank[:4], "blank")                                        # mismatched blank shape
    bad(8, torch.zeros(3, 5, 4, device=dev), "blank")
    bad(8, blank[None].expand(3, 5, 3, 4).contiguous(), "blank")
    bad(5, 2, "target_kind")                                          # the flow target is not this kernel's


def test_inpaint_unmask_draw(dev):
    """p = 0 removes no mask, p = 1 every one; a rank's slice equals the global batch's; two runs agree"""
    assert not K.inpaint_unmask(64, 5, 0.0, device=dev).any()
    assert K.inpaint_unmask(64, 5, 1.0, device=dev).all()
    g = K.inpaint_unmask(64, 7, 0.5, device=dev)
    assert 8 < int(g.sum()) < 56
    assert torch.equal(K.inpaint_unmask(16, 7, 0.5, sample0=32, device=dev), g[32:48])
    assert torch.equal(K.inpaint_unmask(64, 7, 0.5, device=dev), g)
    assert not torch.equal(K.inpaint_unmask(64, 8, 0.5, device=dev), g)
    with pytest.raises(ValueError, match="probability"):
        K.inpaint_unmask(4, 0, 1.5, device=dev)


@pytest.mark.parametrize("shape", [(2, 3, 13, 9), (1, 3, 64, 64)], ids=["2x3x13x9", "1x3x64x64"])
def test_masked_conditioning_bits(dev, shape):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(H)
    img = torch.rand(shape, generator=g).to(dev)
    mask = torch.rand(B, H, W, generator=g)
    mask[mask < 0.3] = 0.0
    mask[mask > 0.7] = 1.0
    mask[0, 0, :3] = torch.tensor([0.0, 1.0, 0.5])
    mask = mask.to(dev)
    x = K.image_to_nhwc(img, 2.0, -1.0, 8)   # the encoder's input: NHWC bf16 in [-1, 1], channels 3..7 zero
    out = torch.full_like(x, float("nan"))
    got = K.masked_conditioning(x, mask, out=out)
    want = (x.float() * (1.0 - mask)[..., None]).bfloat16()
    assert torch.equal(_bits(got), _bits(want))
    assert not got[mask == 1.0].any() and torch.equal(got[mask == 0.0], x[mask == 0.0])
    assert torch.equal(_bits(K.masked_conditioning(x, mask[:, None])), _bits(want))
    with pytest.raises(ValueError, match="mask"):
        K.masked_conditioning(x, mask.double())
    with pytest.raises(ValueError, match="mask"):
        K.masked_conditioning(x, mask[:, :-1])
    with pytest.raises(ValueError, match="x"):
        K.masked_conditioning(x.float(), mask)
