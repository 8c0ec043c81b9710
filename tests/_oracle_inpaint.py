"""NumPy restatement of what csrc/inpaint.hip computes for the mask-input (inpainting) models.

  unet_input   the reference's torch.concat([scaled_noisy_latent_image, latent_mask, latent_conditioning_image *
               vae_scaling_factor], 1) cast to bf16 (BaseStableDiffusionXLSetup.py:217-273), with the removal of mgds
               RandomLatentMaskRemove folded in: a sample with unmask[b] != 0 takes an all-ones mask and the blank
               latent; 16 held channels, 9..15 zero
  conditioning cond = x * (1 - m) on the encoder's bf16 input (mgds GenerateMaskedConditioningImage, restated from its
               name and the diffusers inpainting convention)
Every element is one fp32 operation and one rounding to bf16 (round to nearest even), returned as bit patterns.
"""
from __future__ import annotations

import numpy as np


def bf16_bits(x) -> np.ndarray:
    """fp32 -> the uint16 bit pattern of its bf16 rounding (nearest even; no NaN inputs here)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits) -> np.ndarray:
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def unet_input(noisy, mask, cond, scaling_factor, unmask=None, blank=None, cpad=16) -> np.ndarray:
    """noisy / cond fp32 [B, 4, h, w] (the reference's NCHW), mask fp32 [B, 1, h, w], blank fp32 [4, h, w] ->
    bf16 bits [B, cpad, h, w]"""
    noisy, mask, cond = (np.asarray(a, dtype=np.float32) for a in (noisy, mask, cond))
    B, _, h, w = noisy.shape
    sf = np.float32(scaling_factor)
    out = np.zeros((B, cpad, h, w), dtype=np.uint16)
    for b in range(B):
        removed = unmask is not None and bool(unmask[b])
        m = np.ones_like(mask[b]) if removed else mask[b]
        c = np.asarray(blank, dtype=np.float32) if removed else cond[b]
        out[b, 0:4] = bf16_bits(noisy[b])
        out[b, 4:5] = bf16_bits(m)
        out[b, 5:9] = bf16_bits(c * sf)
    return out


def masked_conditioning(x_bits, mask) -> np.ndarray:
    """x: bf16 bits [..., C] (channels last), mask fp32 [...] -> bf16 bits of x * (1 - m)"""
    keep = np.float32(1.0) - np.asarray(mask, dtype=np.float32)
    return bf16_bits(bf16_value(x_bits) * keep[..., None])
