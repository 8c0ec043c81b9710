"""Golden fixture from the reference's own inpainting predict (container only).

    python tests/golden/make_inpaint_golden.py      -> tests/golden/inpaint_input.npz

Runs StableDiffusionXLFineTuneSetup.predict (modules/modelSetup/BaseStableDiffusionXLSetup.py:214-273) through the
stub harness (tests/golden/ref_harness.py) with model type STABLE_DIFFUSION_XL_10_BASE_INPAINTING and a recording
stand-in UNet, for f32 latents at steps 0 and 7.  Per case it records what the reference's own lines take and give:
scaled_noisy_latent_image (the return value of _add_noise_discrete), batch['latent_mask'],
batch['latent_conditioning_image'], the scaling factor, and the `sample` the UNet receives --
torch.concat([scaled_noisy_latent_image, latent_mask, latent_conditioning_image * scaling_factor], 1) cast to the train
dtype (bf16), stored as its bit pattern.  Only data is stored; no reference source.  The fixture pins
tests/_oracle_inpaint.py (tests/test_inpaint_oracle.py).
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
OUT = HERE / "inpaint_input.npz"
STEPS = (0, 7)
SF = 0.13025


def inpaint_batch(B=2, h=6, w=5):
    g = torch.Generator().manual_seed(41)
    hw = lambda v: torch.full((B,), v, dtype=torch.int64)  # noqa: E731
    mask = torch.rand(B, 1, h, w, generator=g)
    mask[0, 0, 0, :3] = torch.tensor([0.0, 1.0, 0.5])
    return {"latent_image": torch.randn(B, 4, h, w, generator=g) / SF,
            "latent_mask": mask,
            "latent_conditioning_image": torch.randn(B, 4, h, w, generator=g) / SF,
            "text_encoder_1_hidden_state": torch.randn(B, 77, 768, generator=g).bfloat16(),
            "text_encoder_2_hidden_state": torch.randn(B, 77, 1280, generator=g).bfloat16(),
            "text_encoder_2_pooled_state": torch.randn(B, 1280, generator=g).bfloat16(),
            "original_resolution": (hw(64), hw(64)), "crop_offset": (hw(0), hw(0)),
            "crop_resolution": (hw(8 * h), hw(8 * w)), "loss_weight": torch.ones(B),
            "tokens_1": torch.zeros(B, 77, dtype=torch.int64), "tokens_2": torch.zeros(B, 77, dtype=torch.int64),
            "concept_type": ["STANDARD"] * B}


def main():
    sys.path.insert(0, str(HERE))
    import ref_harness
    ref_harness.install()
    from types import SimpleNamespace

    from modules.model.StableDiffusionXLModel import StableDiffusionXLModel
    from modules.modelSetup.StableDiffusionXLFineTuneSetup import StableDiffusionXLFineTuneSetup
    from modules.util.config.TrainConfig import TrainConfig
    from modules.util.enum.DataType import DataType
    from modules.util.enum.ModelType import ModelType
    from modules.util.TrainProgress import TrainProgress

    class AttrDict(dict):
        __getattr__ = dict.__getitem__

    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2

    class DDIM:
        config = AttrDict(num_train_timesteps=1000, prediction_type="epsilon")

        def __init__(self):
            self.betas, self.alphas_cumprod = betas, torch.cumprod(1 - betas, 0)

    class RecUNet(torch.nn.Module):
        def forward(self, sample, timestep, encoder_hidden_states, added_cond_kwargs):
            self.sample = sample.detach().clone()
            return SimpleNamespace(sample=sample[:, :4] * 0.5)

    mt = ModelType.STABLE_DIFFUSION_XL_10_BASE_INPAINTING
    assert mt.has_mask_input() and mt.has_conditioning_image_input()
    rec = {"scaling_factor": np.float64(SF)}
    for step in STEPS:
        model = StableDiffusionXLModel(mt)
        model.vae = torch.nn.Module()
        model.vae.config = {"scaling_factor": SF}
        model.text_encoder_1, model.text_encoder_2 = torch.nn.Module(), torch.nn.Module()
        model.train_dtype = DataType.BFLOAT_16
        model.unet = RecUNet()
        model.noise_scheduler = DDIM()
        cfg = TrainConfig.default_values()
        cfg.train_device = cfg.temp_device = "cpu"
        cfg.model_type = mt
        cfg.text_encoder.train = cfg.text_encoder_2.train = False
        setup = StableDiffusionXLFineTuneSetup(torch.device("cpu"), torch.device("cpu"), False)
        seen = {}
        add_noise = setup._add_noise_discrete

        def rec_add_noise(*a, __f=add_noise, **k):
            seen["noisy"] = __f(*a, **k)
            return seen["noisy"]

        setup._add_noise_discrete = rec_add_noise
        tp = TrainProgress()
        tp.global_step = step
        batch = inpaint_batch()
        setup.predict(model, batch, cfg, tp)
        sample = model.unet.sample
        assert sample.dtype == torch.bfloat16 and sample.shape[1] == 9
        rec[f"{step}/scaled_noisy_latent_image"] = seen["noisy"].detach().numpy().copy()
        rec[f"{step}/latent_mask"] = batch["latent_mask"].numpy().copy()
        rec[f"{step}/latent_conditioning_image"] = batch["latent_conditioning_image"].numpy().copy()
        rec[f"{step}/sample_bf16_bits"] = sample.view(torch.int16).numpy().copy()
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, len(rec), "arrays", OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
