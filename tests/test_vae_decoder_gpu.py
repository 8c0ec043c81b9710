"""The HIP VAE decoder (module/vae.AutoencoderKLDecoder, bf16 NHWC) against an fp32 torch decoder assembled here from
oracle.vae's blocks (diffusers' Decoder: conv_in, mid block, UpDecoderBlock2D x n with nearest-2x Upsample2D,
GroupNorm + SiLU, conv_out), same weights and latents.  Criterion: the one tests/test_vae_gpu.py applies to the
encoder, which runs on the same kernels -- max abs error <= 3e-2 of the output range, cosine >= 0.9995."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from onetrainer_amd.module import vae as V
from oracle import vae as OV

pytestmark = pytest.mark.gpu


class _Up(nn.Module):
    def __init__(self, cin, cout, layers, add_up, groups, eps):
        super().__init__()
        self.resnets = nn.ModuleList([OV.ResnetBlock2D(cin if i == 0 else cout, cout, groups, eps) for i in range(layers)])
        self.add_up = add_up
        if add_up:
            self.upsamplers = nn.ModuleList([nn.ModuleDict({"conv": nn.Conv2d(cout, cout, 3, 1, 1)})])

    def forward(self, x):
        for r in self.resnets:
            x = r(x)
        if self.add_up:
            x = self.upsamplers[0]["conv"](F.interpolate(x, scale_factor=2.0, mode="nearest"))
        return x


class _Decoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        ch = cfg.block_out_channels
        g, eps = cfg.norm_num_groups, cfg.norm_eps
        self.conv_in = nn.Conv2d(cfg.latent_channels, ch[-1], 3, 1, 1)
        self.mid_block = OV.MidBlock(ch[-1], g, eps)
        self.up_blocks = nn.ModuleList()
        cin = ch[-1]
        for i, c in enumerate(reversed(ch)):
            self.up_blocks.append(_Up(cin, c, cfg.layers_per_block + 1, i < len(ch) - 1, g, eps))
            cin = c
        self.conv_norm_out = nn.GroupNorm(g, ch[0], eps)
        self.conv_out = nn.Conv2d(ch[0], cfg.in_channels, 3, 1, 1)

    def forward(self, z):
        x = self.mid_block(self.conv_in(z))
        for b in self.up_blocks:
            x = b(x)
        return self.conv_out(F.silu(self.conv_norm_out(x)))


class _VAE(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.decoder = _Decoder(cfg)
        L = cfg.latent_channels
        self.post_quant_conv = nn.Conv2d(L, L, 1) if cfg.use_quant_conv else None

    def forward(self, z):
        return self.decoder(self.post_quant_conv(z) if self.post_quant_conv is not None else z)


def _cos(a, b):
    a, b = a.flatten().double(), b.flatten().double()
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


@pytest.mark.parametrize("quant", [True, False], ids=["quant_conv", "no_quant_conv"])
@pytest.mark.parametrize("h,w", [(8, 8), (8, 24)])
def test_decoder_matches_fp32_torch(dev, quant, h, w):
    """measured on an MI355X (the four cases): worst relative error and lowest cosine are printed below and recorded
    in DESIGN.md"""
    torch.manual_seed(0)
    cfg = V.tiny_vae_config(use_quant_conv=quant)
    dec = V.AutoencoderKLDecoder(cfg, dev, seed=2)
    ref = _VAE(cfg)
    ref.load_state_dict({k: v.float().cpu() for k, v in dec.state_dict().items()})
    lat = torch.randn(2, h, w, 4) * cfg.scaling_factor * 1.5      # scaled as the UNet sees it
    out = dec.decode(lat.to(dev))
    f = 1 << (len(cfg.block_out_channels) - 1)
    assert out.shape == (2, h * f, w * f, 8) and out.dtype == torch.bfloat16
    assert torch.count_nonzero(out[..., 3:]) == 0
    with torch.no_grad():
        # the oracle sees the same bf16-rounded scaled input
        z = (lat / cfg.scaling_factor).bfloat16().float().permute(0, 3, 1, 2)
        want = ref(z).permute(0, 2, 3, 1)
    got = out[..., :3].float().cpu()
    err = ((got - want).abs().max() / want.abs().max()).item()
    cos = _cos(got, want)
    print(f"decoder quant={quant} latent {h}x{w}: rel err {err:.3e}, cosine {cos:.6f}")
    assert err < 3e-2, f"rel err {err}"
    assert cos > 0.9995
    assert torch.equal(dec.decode(lat.to(dev).bfloat16().float()), dec.decode(lat.bfloat16().to(dev)))
