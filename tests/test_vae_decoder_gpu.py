"""The HIP VAE decoder (module/vae.AutoencoderKLDecoder, bf16 NHWC) against oracle.vae's fp32 decoder (diffusers'
Decoder: conv_in, mid block, UpDecoderBlock2D x n with nearest-2x Upsample2D, GroupNorm + SiLU, conv_out), same
weights and latents.  Criterion: the one tests/test_vae_gpu.py applies to the
encoder, which runs on the same kernels -- max abs error <= 3e-2 of the output range, cosine >= 0.9995."""
import pytest
import torch

import _frozen_parity as P
from onetrainer_amd.module import vae as V
from oracle import vae as OV

pytestmark = pytest.mark.gpu


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
    ref = OV.AutoencoderKLDecoder(cfg)
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
    # the per-row check of _frozen_parity.py: every pixel against the float64 oracle
    ref64 = OV.AutoencoderKLDecoder(cfg, torch.float64)
    ref64.load_state_dict(ref.state_dict())
    with torch.no_grad():
        want64 = ref64(z).permute(0, 2, 3, 1)
    P.check({"rgb": got}, {"rgb": want64}, f"decoder quant={quant} latent {h}x{w}", "vae")
    assert torch.equal(dec.decode(lat.to(dev).bfloat16().float()), dec.decode(lat.bfloat16().to(dev)))
