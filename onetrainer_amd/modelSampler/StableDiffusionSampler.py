"""Training samples for SD 1.5 and SDXL on the HIP kernels (modules/modelSampler/StableDiffusionXLSampler.py:47-196
and StableDiffusionSampler.py, text to image, noise_scheduler DDIM):

    prompt + negative prompt -> text states (the checkpoint's tokenizers + the HIP CLIP encoders the model carries)
    x ~ N(0, 1) from Philox, keyed by the sample's seed
    per DDIM timestep: UNet at batch 2 on [x | x] with [negative | positive] conditioning, then one fused
        guidance + CFG rescale + DDIM step launch (kernels.cfg_ddim_step), which also writes the next UNet input
    VAE decode (module/vae.AutoencoderKLDecoder) -> 8-bit RGB (kernels.nhwc_to_rgb8) -> PIL file

The timestep table is DDIMScheduler.set_timesteps as create_noise_scheduler configures it (modules/util/create.py:
1255-1266): leading spacing, steps_offset 1, set_alpha_to_one False (the last step's alpha_prev is alphas_cumprod[0]),
clip_sample False, eta 0.  cfg_rescale is 0.7, the samplers' default argument.  DDIM and the rescale are restated from
the published formulas; diffusers is not installed here, so nothing was compared with it.  The initial latent comes
from Philox, not from torch's generator, so for a given seed the image differs from the reference's (as training noise
does).

Sampling leaves training alone: it runs under no_grad, writes no trainable parameter or gradient, draws from a Philox
stream of its own (7; training uses 1-6, keyed by the step), switches LoRA dropout off for its duration, and joins the
weight-gradient stream before and after.
"""
from __future__ import annotations

import os
import random

import torch

from .. import kernels as K
from ..module import streams as S
from ..util.config.SampleConfig import IMAGE_FORMATS, as_sample_config

CFG_RESCALE = 0.7          # StableDiffusionXLSampler.py:52 / StableDiffusionSampler.py: cfg_rescale=0.7
SAMPLE_PHILOX_STREAM = 7   # csrc/philox.h: streams 1-6 belong to training (noise, timesteps, LoRA dropout)
QUANT = 64                 # StableDiffusionXLSampler.py:72-73: height / width are rounded to multiples of 64


def ddim_table(steps: int, num_train_timesteps: int = 1000, force_last_timestep: bool = False) -> list[tuple[int, int]]:
    """[(timestep, table index of alpha_prev)] of one sample run.  prev = t - N // steps; below 0 it is
    final_alpha_cumprod = alphas_cumprod[0].  force_last_timestep prepends N - 1 (StableDiffusionXLSampler.py:96-101),
    whose prev follows the same rule."""
    steps = int(steps)
    if steps < 1 or steps >= num_train_timesteps:
        raise ValueError(f"diffusion_steps {steps} outside [1, {num_train_timesteps - 1}]")
    ratio = num_train_timesteps // steps
    ts = [int(round(i * ratio)) + 1 for i in range(steps)][::-1]
    if force_last_timestep:
        ts = [num_train_timesteps - 1] + ts
    return [(t, max(t - ratio, 0)) for t in ts]


def quantize_resolution(resolution: int, quantization: int = QUANT) -> int:
    return max(quantization, round(resolution / quantization) * quantization)


class StableDiffusionSampler:
    def __init__(self, model, device, base_model_name: str = ""):
        self.model = model
        self.device = torch.device(device)
        self.base_model_name = base_model_name
        self._tokenizers = None
        self._text_cache: dict = {}

    # ----- text -----------------------------------------------------------------------------------
    def _sdxl(self) -> bool:
        return bool(self.model.unet.cfg.addition_embed)

    def _encode(self, prompt: str, skip_1: int, skip_2: int):
        """(hidden [1, 77, ctx] bf16, pooled [1, 1280] or None) of one prompt, as dataLoader/create.py encodes
        captions for the cache"""
        key = (prompt, skip_1, skip_2)
        if key in self._text_cache:
            return self._text_cache[key]
        from ..module import text_encoder as TE
        m = self.model
        te1, te2 = getattr(m, "text_encoder_1", None), getattr(m, "text_encoder_2", None)
        if te1 is None or (self._sdxl() and te2 is None):
            raise RuntimeError("sampling a prompt needs the model's text encoders (GenericTrainer keeps them when "
                               "samples are configured) or ready prompt_states")
        if self._tokenizers is None:
            from transformers import CLIPTokenizer
            subs = ("tokenizer", "tokenizer_2") if self._sdxl() else ("tokenizer",)
            self._tokenizers = [CLIPTokenizer.from_pretrained(os.path.join(self.base_model_name, s)) for s in subs]

        def ids(tok):
            return tok(prompt, padding="max_length", max_length=77, truncation=True,
                       return_tensors="pt").input_ids.to(self.device)

        if self._sdxl():
            out = TE.encode_sdxl_text(te1, te2, ids(self._tokenizers[0]), ids(self._tokenizers[1]), skip_1, skip_2)
        else:
            out = (TE.encode_sd15_text(te1, ids(self._tokenizers[0]), skip_1), None)
        self._text_cache[key] = out
        return out

    def _conditioning(self, sc, prompt_states):
        """[negative | positive]: hidden [2, L, ctx] bf16, pooled [2, 1280] or None"""
        if prompt_states is not None:
            pos, neg = prompt_states["positive"], prompt_states["negative"]
        else:
            pos = self._encode(sc.prompt, sc.text_encoder_1_layer_skip, sc.text_encoder_2_layer_skip)
            neg = self._encode(sc.negative_prompt, sc.text_encoder_1_layer_skip, sc.text_encoder_2_layer_skip)
        hidden = torch.cat([neg[0].reshape(1, *neg[0].shape[-2:]), pos[0].reshape(1, *pos[0].shape[-2:])])
        hidden = hidden.to(self.device, torch.bfloat16).contiguous()
        pooled = None
        if self._sdxl():
            if pos[1] is None or neg[1] is None:
                raise ValueError("SDXL sampling needs the pooled text_encoder_2 state of both prompts")
            pooled = torch.cat([neg[1].reshape(1, -1), pos[1].reshape(1, -1)]).to(self.device)
        return hidden, pooled

    # ----- one image ------------------------------------------------------------------------------
    @torch.no_grad()
    def sample_image(self, sample_config, prompt_states=None) -> torch.Tensor:
        """-> uint8 [H, W, 3] on the device"""
        sc = as_sample_config(sample_config).check_supported()
        m = self.model
        dec = getattr(m, "vae_decoder", None)
        if dec is None:
            raise RuntimeError("sampling needs model.vae_decoder (module/vae.AutoencoderKLDecoder)")
        H, W = quantize_resolution(sc.height), quantize_resolution(sc.width)
        f = 1 << (len(dec.cfg.block_out_channels) - 1)
        h, w = H // f, W // f
        seed = random.randint(0, 2 ** 30) if sc.random_seed else int(sc.seed)
        ns = m.noise_scheduler
        table = ddim_table(sc.diffusion_steps, ns.config["num_train_timesteps"], sc.force_last_timestep)
        v_pred = ns.config["prediction_type"] == "v_prediction"
        lora = getattr(m, "unet_lora", None)
        drop = getattr(lora, "dropout_p", 0.0)
        S.join()
        try:
            if drop:
                lora.dropout_p = 0.0
            hidden, pooled = self._conditioning(sc, prompt_states)
            time_ids = None
            if self._sdxl():   # StableDiffusionXLSampler.py:108-120: original size, crop top-left, target size
                time_ids = torch.tensor([[H, W, 0, 0, H, W]] * 2, dtype=torch.float32, device=self.device)
            x = K.noise_stream(h * w * 4, seed, SAMPLE_PHILOX_STREAM, dtype=torch.float32,
                               device=self.device).view(1, h, w, 4)
            nxt = torch.zeros((2, h, w, 8), dtype=torch.bfloat16, device=self.device)
            nxt[..., :4] = x.to(torch.bfloat16)
            steps = torch.tensor([t for t, _ in table], dtype=torch.int32, device=self.device)
            for i, (t, t_prev) in enumerate(table):
                pred = m.unet(nxt, steps[i:i + 1], hidden, pooled, time_ids)
                K.cfg_ddim_step(pred, x, ns.coeffs, t, t_prev, float(sc.cfg_scale), CFG_RESCALE, v_pred, out=x,
                                next_in=nxt)
            image = K.nhwc_to_rgb8(dec.decode(x))
        finally:
            if drop:
                lora.dropout_p = drop
            S.join()
        return image[0]

    def sample(self, sample_config, destination: str, image_format: str = "JPG", prompt_states=None,
               on_sample=None) -> str:
        """BaseModelSampler.sample + save_sampler_output (BaseModelSampler.py:64-92): the image is written to
        destination + the format's extension; returns that path."""
        from PIL import Image
        ext, pil_format = IMAGE_FORMATS[str(getattr(image_format, "value", image_format))]
        rgb = self.sample_image(sample_config, prompt_states)
        image = Image.fromarray(rgb.cpu().numpy(), mode="RGB")
        os.makedirs(os.path.dirname(os.path.abspath(destination)), exist_ok=True)
        path = destination + ext
        image.save(path, format=pil_format)
        if on_sample is not None:
            on_sample(image)
        return path
