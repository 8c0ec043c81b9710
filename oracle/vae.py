"""CPU restatement (fp32 by default; any dtype through `dtype`) of diffusers AutoencoderKL.encode(...).latent_dist.mean
(the encoder half + quant_conv + DiagonalGaussianDistribution mean) and of AutoencoderKL.decode (post_quant_conv + the
decoder half), NCHW, diffusers parameter names.
TEST INFRASTRUCTURE ONLY (oracle/__init__.py).

The reference runs it through mgds EncodeVAE + SampleVAEDistribution(mode='mean') at
modules/dataLoader/StableDiffusionXLBaseDataLoader.py:65-100 (RescaleImageChannels 0..1 -> -1..1 first).
diffusers@5873377 and mgds@11ff4aa are not in this image; the graph is restated from the ddconfig
the reference pins in resources/model_config/stable_diffusion_xl/sd_xl_base.yaml (ch 128,
ch_mult [1,2,4,4], num_res_blocks 2, z_channels 4, double_z, attn only in the mid block).
FLUX.1 (FluxBaseDataLoader.py:70-71): 16 latent channels and no quant_conv (cfg.use_quant_conv False): the
mean is conv_out's first 16 channels.
PARITY UNPINNED: no reference test or fixture pins the VAE numerics.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn as nn
import torch.nn.functional as F


@dataclass
class VAEConfig:
    """the fields of module/vae.py's VAEConfig, restated so that the oracle needs no HIP library"""
    in_channels: int = 3
    block_out_channels: tuple = (128, 256, 512, 512)
    layers_per_block: int = 2
    latent_channels: int = 4
    norm_num_groups: int = 32
    norm_eps: float = 1e-6
    scaling_factor: float = 0.13025
    shift_factor: float = 0.0
    use_quant_conv: bool = True


def tiny_vae_config(latent_channels: int = 4, use_quant_conv: bool = True) -> VAEConfig:
    return VAEConfig(block_out_channels=(64, 160), layers_per_block=1, latent_channels=latent_channels,
                     use_quant_conv=use_quant_conv)


def norm_out(norm: nn.GroupNorm, x):
    """conv_norm_out of the encoder and of the decoder: GroupNorm then SiLU"""
    return F.silu(norm(x))


def upsample_nearest(x):
    """Upsample2D's interpolation: every pixel becomes a 2 x 2 block"""
    return F.interpolate(x, scale_factor=2.0, mode="nearest")


class ResnetBlock2D(nn.Module):
    """diffusers ResnetBlock2D with temb_channels=None (VAE), GroupNorm eps 1e-6."""

    def __init__(self, cin, cout, groups, eps):
        super().__init__()
        self.norm1 = nn.GroupNorm(groups, cin, eps)
        self.conv1 = nn.Conv2d(cin, cout, 3, 1, 1)
        self.norm2 = nn.GroupNorm(groups, cout, eps)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1)
        self.conv_shortcut = nn.Conv2d(cin, cout, 1) if cin != cout else None

    def forward(self, x):
        h = self.conv1(F.silu(self.norm1(x)))
        h = self.conv2(F.silu(self.norm2(h)))
        if self.conv_shortcut is not None:
            x = self.conv_shortcut(x)
        return x + h


class Downsample2D(nn.Module):
    """padding=0 variant: F.pad(x, (0, 1, 0, 1)) then 3x3 stride-2 conv."""
    PAD = (0, 1, 0, 1)     # (left, right, top, bottom)

    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, 2, 0)

    def forward(self, x):
        return self.conv(F.pad(x, self.PAD))


class VAEAttention(nn.Module):
    """single-head self-attention with GroupNorm, biased projections and the residual add."""

    def __init__(self, c, groups, eps):
        super().__init__()
        self.group_norm = nn.GroupNorm(groups, c, eps)
        self.to_q, self.to_k, self.to_v = nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c)
        self.to_out = nn.ModuleList([nn.Linear(c, c)])

    def forward(self, x):
        B, C, H, W = x.shape
        h = self.group_norm(x).view(B, C, H * W).transpose(1, 2)
        q, k, v = self.to_q(h)[:, None], self.to_k(h)[:, None], self.to_v(h)[:, None]
        o = F.scaled_dot_product_attention(q, k, v)[:, 0]
        o = self.to_out[0](o)
        return o.transpose(1, 2).reshape(B, C, H, W) + x


class DownEncoderBlock2D(nn.Module):
    def __init__(self, cin, cout, layers, add_down, groups, eps):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(cin if i == 0 else cout, cout, groups, eps) for i in range(layers)])
        if add_down:
            self.downsamplers = nn.ModuleList([Downsample2D(cout)])
        self.add_down = add_down

    def forward(self, x):
        for r in self.resnets:
            x = r(x)
        if self.add_down:
            x = self.downsamplers[0](x)
        return x


class MidBlock(nn.Module):
    def __init__(self, c, groups, eps):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(c, c, groups, eps) for _ in range(2)])
        self.attentions = nn.ModuleList([VAEAttention(c, groups, eps)])

    def forward(self, x):
        return self.resnets[1](self.attentions[0](self.resnets[0](x)))


class Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        ch = cfg.block_out_channels
        g, eps = cfg.norm_num_groups, cfg.norm_eps
        self.conv_in = nn.Conv2d(cfg.in_channels, ch[0], 3, 1, 1)
        self.down_blocks = nn.ModuleList()
        cin = ch[0]
        for i, c in enumerate(ch):
            self.down_blocks.append(DownEncoderBlock2D(cin, c, cfg.layers_per_block, i < len(ch) - 1, g, eps))
            cin = c
        self.mid_block = MidBlock(ch[-1], g, eps)
        self.conv_norm_out = nn.GroupNorm(g, ch[-1], eps)
        self.conv_out = nn.Conv2d(ch[-1], 2 * cfg.latent_channels, 3, 1, 1)

    def forward(self, x):
        x = self.conv_in(x)
        for b in self.down_blocks:
            x = b(x)
        x = self.mid_block(x)
        return self.conv_out(norm_out(self.conv_norm_out, x))


class AutoencoderKLEncoder(nn.Module):
    """parameters and every intermediate are held in `dtype` (load_state_dict casts into it)"""

    def __init__(self, cfg, dtype=torch.float32):
        super().__init__()
        self.cfg = cfg
        self.encoder = Encoder(cfg)
        q = getattr(cfg, "use_quant_conv", True)
        self.quant_conv = nn.Conv2d(2 * cfg.latent_channels, 2 * cfg.latent_channels, 1) if q else None
        self.dtype = dtype
        self.to(dtype)

    def moments(self, x):
        """x: rescaled image in [-1, 1] -> the DiagonalGaussianDistribution parameters"""
        h = self.encoder(x.to(self.dtype))
        return self.quant_conv(h) if self.quant_conv is not None else h

    def mean(self, moments):
        return moments[:, :self.cfg.latent_channels]

    def forward(self, images01):
        """images in [0, 1] NCHW -> latent_dist.mean NCHW (RescaleImageChannels + encode + mean)."""
        return self.mean(self.moments(images01 * 2.0 - 1.0))


class UpDecoderBlock2D(nn.Module):
    def __init__(self, cin, cout, layers, add_up, groups, eps):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(cin if i == 0 else cout, cout, groups, eps) for i in range(layers)])
        self.add_up = add_up
        if add_up:
            self.upsamplers = nn.ModuleList([nn.ModuleDict({"conv": nn.Conv2d(cout, cout, 3, 1, 1)})])

    def forward(self, x):
        for r in self.resnets:
            x = r(x)
        if self.add_up:
            x = self.upsamplers[0]["conv"](upsample_nearest(x))
        return x


class Decoder(nn.Module):
    """diffusers' Decoder: conv_in, the mid block, UpDecoderBlock2D over the reversed block_out_channels
    (layers_per_block + 1 resnets each, nearest-2x Upsample2D on all but the last), GroupNorm + SiLU, conv_out"""

    def __init__(self, cfg):
        super().__init__()
        ch = cfg.block_out_channels
        g, eps = cfg.norm_num_groups, cfg.norm_eps
        self.conv_in = nn.Conv2d(cfg.latent_channels, ch[-1], 3, 1, 1)
        self.mid_block = MidBlock(ch[-1], g, eps)
        self.up_blocks = nn.ModuleList()
        cin = ch[-1]
        for i, c in enumerate(reversed(ch)):
            self.up_blocks.append(UpDecoderBlock2D(cin, c, cfg.layers_per_block + 1, i < len(ch) - 1, g, eps))
            cin = c
        self.conv_norm_out = nn.GroupNorm(g, ch[0], eps)
        self.conv_out = nn.Conv2d(ch[0], cfg.in_channels, 3, 1, 1)

    def forward(self, z):
        x = self.mid_block(self.conv_in(z))
        for b in self.up_blocks:
            x = b(x)
        return self.conv_out(norm_out(self.conv_norm_out, x))


class AutoencoderKLDecoder(nn.Module):
    """the decoder half; parameters and every intermediate are held in `dtype`"""

    def __init__(self, cfg, dtype=torch.float32):
        super().__init__()
        self.cfg = cfg
        self.decoder = Decoder(cfg)
        L = cfg.latent_channels
        self.post_quant_conv = nn.Conv2d(L, L, 1) if getattr(cfg, "use_quant_conv", True) else None
        self.dtype = dtype
        self.to(dtype)

    def forward(self, z):
        """z: the VAE's own latent NCHW (AutoencoderKL.decode's argument) -> image NCHW"""
        z = z.to(self.dtype)
        return self.decoder(self.post_quant_conv(z) if self.post_quant_conv is not None else z)

    def unscale(self, latent):
        """the latent as the UNet sees it -> the VAE's own: / scaling_factor, FLUX's shift_factor added back"""
        return latent / self.cfg.scaling_factor + self.cfg.shift_factor

    def decode(self, latent):
        return self.forward(self.unscale(latent))
