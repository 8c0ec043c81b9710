"""tests/_oracle_inpaint.py against the fixture recorded from the reference's own inpainting predict
(tests/golden/make_inpaint_golden.py: StableDiffusionXLFineTuneSetup.predict with model type
STABLE_DIFFUSION_XL_10_BASE_INPAINTING reaches the torch.concat and scaling lines through the stub harness, so the
fixture is the reference's UNet input, not a direct call), and against torch for what the reference leaves to mgds."""
from pathlib import Path

import numpy as np
import pytest
import torch

import _oracle_inpaint as O

GOLDEN = Path(__file__).resolve().parent / "golden" / "inpaint_input.npz"


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("step", [0, 7])
def test_unet_input_matches_the_reference(golden, step):
    noisy = golden[f"{step}/scaled_noisy_latent_image"]
    mask = golden[f"{step}/latent_mask"]
    cond = golden[f"{step}/latent_conditioning_image"]
    want = golden[f"{step}/sample_bf16_bits"].view(np.uint16)
    got = O.unet_input(noisy, mask, cond, float(golden["scaling_factor"]))
    assert want.shape[1] == 9 and got.shape[1] == 16
    assert np.array_equal(got[:, :9], want)
    assert not got[:, 9:].any()
    zeros = np.zeros(len(noisy), dtype=np.int32)
    assert np.array_equal(O.unet_input(noisy, mask, cond, float(golden["scaling_factor"]), zeros, cond[0]), got)


def test_removed_mask_takes_ones_and_the_blank(golden):
    noisy, mask, cond = (golden[f"0/{k}"] for k in ("scaled_noisy_latent_image", "latent_mask",
                                                     "latent_conditioning_image"))
    sf = float(golden["scaling_factor"])
    blank = np.random.default_rng(3).standard_normal(cond.shape[1:]).astype(np.float32)
    got = O.unet_input(noisy, mask, cond, sf, unmask=[0, 1], blank=blank)
    plain = O.unet_input(noisy, mask, cond, sf)
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1, :4], plain[1, :4])
    assert (got[1, 4] == 0x3F80).all()   # 1.0
    assert np.array_equal(got[1, 5:9], O.bf16_bits(blank * np.float32(sf)))
    ref = (torch.from_numpy(blank) * sf).bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got[1, 5:9], ref)


def test_bf16_rounding_is_torchs():
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.randn(4096, generator=g) * 3, torch.tensor([0.0, -0.0, 1.0, 1.00390625, 1.01171875, 3e-39])])
    assert np.array_equal(O.bf16_bits(x.numpy()), x.bfloat16().view(torch.int16).numpy().view(np.uint16))


def test_masked_conditioning_is_x_times_one_minus_m():
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(2, 13, 9, 8, generator=g) * 2 - 1).bfloat16()
    x[..., 3:] = 0
    m = torch.rand(2, 13, 9, generator=g)
    m[0, 0, :3] = torch.tensor([0.0, 1.0, 0.5])
    want = (x.float() * (1 - m)[..., None]).bfloat16().view(torch.int16).numpy().view(np.uint16)
    got = O.masked_conditioning(x.view(torch.int16).numpy().view(np.uint16), m.numpy())
    assert np.array_equal(got, want)
    assert not (got[0, 0, 1] & 0x7FFF).any()   # fully masked: zero (the sign is x's)
    assert np.array_equal(got[0, 0, 0], x.view(torch.int16).numpy().view(np.uint16)[0, 0, 0])
