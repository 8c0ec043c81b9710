"""predict / calculate_loss for SDXL (and SD1.5: no add-embedding) on the HIP kernels.

Drop-in for modules/modelSetup/BaseStableDiffusionXLSetup.py:179-373 (predict, calculate_loss),
with the math of ModelSetupNoiseMixin.py:18-155, ModelSetupDiffusionMixin.py:15-38 and
ModelSetupDiffusionLossMixin.py:27-279 done by csrc/diffusion.hip:
  * noise / timesteps: Philox, seeded by the same `batch_seed` (0 if deterministic else
    global_step); counter = index in the GLOBAL batch, so DP rank r draws exactly its slice;
  * DDPM noising + target (epsilon / v_prediction) in one prologue kernel;
  * MSE (+ MIN_SNR_GAMMA / DEBIASED_ESTIMATION / P2 weights, loss_weight, scalers) on the MSE kernels; with
    masked_training, mae_strength or log_cosh_strength set, the mask-weighted MSE / MAE / log-cosh family
    (batch["latent_mask"] [B, 1, h, w], ModelSetupDiffusionLossMixin.py:36-117).
Batch contract as the reference's data loader (StableDiffusionXLBaseDataLoader.py:174-209),
with `latent_image` [B, 4, h, w]; this build's loaders hand it over as a view of channels-last
storage, so the kernels' NHWC layout costs no copy.
"""
from __future__ import annotations

from random import Random

import torch

from .. import kernels as K
from ..module import functional as Fn
from ..util.config.plain import plain
from ..util.model_type import has_mask_input
from ..util.timestep_table import TABLE_DISTS, TimestepTables

LOSS_FN = {"CONSTANT": 0, "MIN_SNR_GAMMA": 1, "DEBIASED_ESTIMATION": 2, "P2": 3}
TIMESTEP_DIST = {"UNIFORM": 0, "LOGIT_NORMAL": 1, "HEAVY_TAIL": 2, "COS_MAP": 3, "SIGMOID": 4}


def loss_plan(config, flow: bool = False) -> dict:
    """The loss decisions of ModelSetupDiffusionLossMixin for this config (config already plain()):
    batch / GA scale (LossScaler, :243-248 / :290-295), the timestep weight kernel id (:271-278 for
    DDPM: MIN_SNR_GAMMA / DEBIASED_ESTIMATION / P2, anything else unweighted; :316-319 for flow
    matching: SIGMA, anything else unweighted), the MSE / MAE / log-cosh strengths (:47-99,130-150) and the
    mask terms of masked training (:258-261, masked_loss.py:21-37).  The mask fields are read only under
    masked_training, with the reference's defaults (TrainConfig.py:933-938) where a config lacks them.
    vb_loss_strength is not read: the reference applies that term only when the model predicts variance
    values (:102,153), which SD / SDXL / FLUX never do."""
    masked = bool(config.masked_training)
    unmasked_weight, normalize = 0.1, False
    if masked:
        if float(getattr(config, "masked_prior_preservation_weight", 0.0)) != 0:
            raise NotImplementedError("masked_prior_preservation_weight != 0: the prior-preservation term needs a "
                                      "prior_target, which predict() does not produce")
        unmasked_weight = float(getattr(config, "unmasked_weight", 0.1))
        normalize = bool(getattr(config, "normalize_masked_area_loss", False))
    scaler = config.loss_scaler
    if scaler not in ("NONE", "BATCH", "GRADIENT_ACCUMULATION", "BOTH"):
        raise ValueError(f"loss_scaler {scaler!r}")
    bs = 1 if scaler in ("NONE", "GRADIENT_ACCUMULATION") else config.batch_size
    gas = 1 if scaler in ("NONE", "BATCH") else config.gradient_accumulation_steps
    fn = config.loss_weight_fn
    if flow:
        kid = 4 if fn == "SIGMA" else 0
    else:
        kid = LOSS_FN.get(fn, 0)
    return {"batch_size_scale": bs, "ga_scale": gas, "loss_fn": kid, "gamma": float(config.loss_weight_strength),
            "mse_strength": float(config.mse_strength), "mae_strength": float(config.mae_strength),
            "log_cosh_strength": float(config.log_cosh_strength), "masked": masked,
            "unmasked_weight": unmasked_weight, "normalize": normalize}


def plain_mse(plan: dict) -> bool:
    """the plan is the unmasked MSE alone: the loss stays on the MSE kernels"""
    return not plan["masked"] and plan["mae_strength"] == 0 and plan["log_cosh_strength"] == 0


def loss_mask(batch: dict, plan: dict, device, data: dict | None = None):
    """batch["latent_mask"] [B, 1, h, w] as the loss kernel reads it (f32, contiguous, on the device), or None
    when the plan is unmasked.  A mask-input model's predict() hands over the mask it fed the UNet (all ones where the
    step removed a sample's mask) as data["_loss_mask"]: the loss is weighted by that one."""
    if not plan["masked"]:
        return None
    if data is not None and data.get("_loss_mask") is not None:
        return data["_loss_mask"]
    if "latent_mask" not in batch:
        raise KeyError("latent_mask: masked_training is on, but the batch carries no 'latent_mask' "
                       "(a cache built without masks?)")
    return batch["latent_mask"].to(device, torch.float32).contiguous()


def timestep_plan(config) -> int:
    """kernel id of config.timestep_distribution (ModelSetupNoiseMixin.py:91-153): the continuous UNIFORM /
    LOGIT_NORMAL / HEAVY_TAIL and the table-driven COS_MAP / SIGMOID (util/timestep_table.py)."""
    d = config.timestep_distribution
    if d not in TIMESTEP_DIST:
        raise NotImplementedError(f"timestep distribution {d} is not on this build's hot path")
    return TIMESTEP_DIST[d]


def draw_timesteps(tables: TimestepTables, config, B, seed, sample0, N, shift, device, out=None):
    """_get_timestep_discrete (ModelSetupNoiseMixin.py:69-155, not deterministic) for samples [sample0, sample0 + B)
    of the global batch; `shift` as the setup resolved it.  COS_MAP / SIGMOID read their cumulative table from
    `tables` (built and uploaded on first use of an argument set, outside any capture)."""
    dist = timestep_plan(config)
    cdf = None
    if config.timestep_distribution in TABLE_DISTS:
        cdf = tables.cdf(config.timestep_distribution, N, int(N * config.min_noising_strength),
                         int(N * config.max_noising_strength), shift, config.noising_bias, config.noising_weight,
                         device)
    return K.timesteps(B, seed=seed, sample0=sample0, dist=dist, num_train_timesteps=N,
                       min_s=config.min_noising_strength, max_s=config.max_noising_strength, shift=shift,
                       bias=config.noising_bias, weight=config.noising_weight, device=device, out=out, cdf=cdf)


def draw_noise(config, shape, seed, offset, dtype, device, out=None, per_sample=False):
    """_create_noise (ModelSetupNoiseMixin.py:18-49) for an NHWC latent: Philox stream 1, plus the offset
    (per sample and channel) and perturbation terms when their weights are > 0, in one kernel.
    per_sample (the validation pass): every sample is the draw of a batch of one at offset 0, all terms included."""
    ow, pw = float(config.offset_noise_weight), float(config.perturbation_noise_weight)
    if per_sample:
        return K.noise_per_sample(shape, seed=seed, offset_weight=max(ow, 0.0), perturbation_weight=max(pw, 0.0),
                                  dtype=dtype, device=device, out=out)
    if ow > 0 or pw > 0:
        return K.noise_ex(shape, seed=seed, offset=offset, offset_weight=max(ow, 0.0), perturbation_weight=max(pw, 0.0),
                          dtype=dtype, device=device, out=out)
    return K.noise(shape, seed=seed, offset=offset, dtype=dtype, device=device, out=out)


def per_sample_losses(model, batch, data, plan, C, device, coeffs, v_pred, num_t=1000):
    """the loss kernels' per-sample losses f32 [B] of a prediction, forward only (no autograd node, no host read):
    element b is bit for bit what calculate_loss returns for sample b as a batch of one -- loss_weight, the timestep
    weight, the strengths and the batch / accumulation scalers of `plan` included, the division by
    gradient_accumulation_steps that train_step applies to the scalar not.  What the validation pass accumulates."""
    lw = batch.get("loss_weight")
    lw = lw.to(device, torch.float32).contiguous() if lw is not None else None
    pred, target = nhwc_pair(data, C)
    scale = float(plan["batch_size_scale"] * plan["ga_scale"])
    if plain_mse(plan):
        return K.mse_loss(pred, target, lw, mse_strength=plan["mse_strength"], scale=scale, loss_fn=plan["loss_fn"],
                          gamma=plan["gamma"], v_pred=v_pred, ga=1.0, timestep=data["timestep"], coeffs=coeffs,
                          num_t=num_t)[2]
    return K.diffusion_loss(pred, target, loss_mask(batch, plan, device, data), lw, mse_strength=plan["mse_strength"],
                            mae_strength=plan["mae_strength"], log_cosh_strength=plan["log_cosh_strength"],
                            unmasked_weight=plan["unmasked_weight"], normalize=plan["normalize"], scale=scale,
                            loss_fn=plan["loss_fn"], gamma=plan["gamma"], v_pred=v_pred, ga=1.0,
                            timestep=data["timestep"], coeffs=coeffs, num_t=num_t)[2]


def set_lora_rows(lora, batch_seed: int, per_sample_batch: int):
    """LoRA dropout state of the step about to run: the masks' seed, and whether every sample's mask rows restart
    at 0 (the validation pass; per_sample_batch = its batch size) or follow the global batch (training; 0).  Both
    are written by every step_inputs call.  The row numbering is a host flag read when a launch is issued, and a
    step being captured (trainer/step_graph.py) issues its launches without step_inputs: the validation pass
    therefore puts the flag back to 0 itself when it ends (GenericTrainer.validate).  The seed is device memory,
    read when a kernel runs, after the step_inputs that precedes every eager step and every replay."""
    if getattr(lora, "dropout_p", 0) > 0:
        lora.set_dropout_seed(batch_seed)
        lora.per_sample_batch = per_sample_batch


def report_learning_rates(model, lr_scheduler, tensorboard):
    """BaseModelSetup.report_to_tensorboard (modules/modelSetup/BaseModelSetup.py:96-119): the scheduler's
    last lr of each parameter group as `lr/<display name prefix>`, the first group of a prefix winning.  An adaptive
    optimizer's groups carry its step-size estimate `d`, and lr * d is reported, as Optimizer.maybe_adjust_lrs
    (modules/util/enum/Optimizer.py:99-105) does; for the others (no `d`) it is the identity."""
    lrs = lr_scheduler.get_last_lr()
    names = model.parameters.display_name_mapping()
    if len(lrs) != len(names):
        raise ValueError(f"{len(lrs)} learning rates for {len(names)} parameter groups")
    groups = getattr(getattr(model, "optimizer", None), "param_groups", None)
    if groups is None or len(groups) != len(lrs):
        groups = [{}] * len(lrs)
    reported = {}
    for lr, name, group in zip(lrs, names, groups):
        reported.setdefault(name.split("/")[0], lr * group.get("d", 1.0))
    for name, lr in reported.items():
        tensorboard.add_scalar(f"lr/{name}", lr, model.train_progress.global_step)


def nhwc_pair(data: dict, C: int):
    """(pred NHWC bf16 [B,h,w,cpad], target NHWC [B,h,w,C]) for the loss kernel: the private kernel
    tensors predict() returned, or -- when a caller hands [B,C,h,w] tensors of its own -- their
    NHWC restatement (pred padded to 8 channels, the kernel's 16-byte row granule)."""
    if "_predicted_nhwc" in data:
        return data["_predicted_nhwc"], data["_target_nhwc"]
    p, t = data["predicted"], data["target"]
    if p.dim() == 4 and p.shape[1] == C and p.shape[-1] != C:
        p = p.permute(0, 2, 3, 1)
        t = t.permute(0, 2, 3, 1)
    cpad = (p.shape[-1] + 7) // 8 * 8
    if cpad != p.shape[-1]:
        p = torch.nn.functional.pad(p, (0, cpad - p.shape[-1]))
    return p.to(torch.bfloat16).contiguous(), t.contiguous()


class BaseStableDiffusionXLSetup:
    def __init__(self, train_device, temp_device=None, debug_mode=False, dp_rank=0, dp_world=1):
        self.train_device = torch.device(train_device)
        self.temp_device = temp_device
        self.debug_mode = debug_mode
        self.dp_rank = dp_rank
        self.dp_world = dp_world
        # (noise, timestep[, unmask: mask-input models]) drawn outside a captured step (trainer/step_graph.py)
        self.graph_inputs = None
        self.timestep_tables = TimestepTables()   # COS_MAP / SIGMOID cumulative tables on the device

    # ------------------------------------------------------------------------------------------
    @staticmethod
    def _nhwc_latent(lat: torch.Tensor) -> torch.Tensor:
        """batch latent [B, C, h, w] (the reference contract) -> NHWC for the kernels: free when the
        tensor is a channels-last view (this build's loaders), one relayout copy otherwise (mgds)."""
        return lat.permute(0, 2, 3, 1).contiguous()

    def _text(self, model, batch, config, rand, B, per_sample=False):
        """per_sample (the validation pass): every sample takes the draws of a batch of one, so each encoder's mask
        is one draw of `rand` repeated"""
        config = plain(config)
        te1 = batch["text_encoder_1_hidden_state"]
        te2 = batch.get("text_encoder_2_hidden_state")
        pooled = batch.get("text_encoder_2_pooled_state")
        for part, key in ((config.text_encoder, "te1"), (config.text_encoder_2, "te2")):
            p = part.dropout_probability
            if p is not None and p > 0:   # StableDiffusionXLModel.py:266-281 (host mask from Random(seed))
                keep = [rand.random() > p] * B if per_sample else [rand.random() > p for _ in range(B)]
                mask = torch.tensor(keep, device=te1.device).to(te1.dtype)
                if key == "te1":
                    te1 = te1 * mask[:, None, None]
                else:
                    te2 = te2 * mask[:, None, None]
                    pooled = pooled * mask[:, None]
        ehs, pooled = model.combine_text_encoder_output(te1.to(torch.bfloat16), None if te2 is None else
                                                        te2.to(torch.bfloat16), pooled)
        return ehs, pooled

    def report_to_tensorboard(self, model, config, lr_scheduler, tensorboard):
        report_learning_rates(model, lr_scheduler, tensorboard)

    def graphable(self, config) -> bool:
        """the step has no host-random or host-varying input besides (noise, timestep), so it can be
        captured once and replayed (text dropout draws its mask on the host per step)."""
        config = plain(config)
        parts = [config.text_encoder] + ([config.text_encoder_2] if hasattr(config, "text_encoder_2") else [])
        return all(not (p.dropout_probability or 0) > 0 for p in parts)

    def step_inputs(self, model, batch: dict, config, train_progress, *, deterministic: bool = False, out=None,
                    per_sample: bool = False):
        """(noise, timestep) of this micro-step (ModelSetupNoiseMixin._create_noise /
        _get_timestep_discrete): Philox seeded by `batch_seed`, counter = GLOBAL batch index.
        per_sample (the validation pass, with deterministic): every sample gets the inputs of a batch of one on
        rank 0 -- the noise counters and the LoRA dropout rows restart at 0 for each sample."""
        config = plain(config)
        batch_seed = 0 if deterministic else train_progress.global_step
        # LoRA dropout masks: the same seed, written outside a captured step
        set_lora_rows(getattr(model, "unet_lora", None), batch_seed, batch["latent_image"].shape[0] if per_sample else 0)
        lat = batch["latent_image"]
        B = lat.shape[0]
        shape = tuple(self._nhwc_latent(lat).shape) if out is None else tuple(out[0].shape)
        _, h, w, C = shape
        sample0 = self.dp_rank * B                       # global-batch index of this rank's first sample
        noise = draw_noise(config, shape, batch_seed, sample0 * h * w * C, lat.dtype, lat.device,
                           None if out is None else out[0], per_sample=per_sample)
        N = model.noise_scheduler.config["num_train_timesteps"]
        if deterministic:
            timestep = torch.full((B,), int(N * 0.5) - 1, dtype=torch.int32, device=lat.device)
            if out is not None:
                timestep = out[1].copy_(timestep)
        else:
            timestep = draw_timesteps(self.timestep_tables, config, B, batch_seed, sample0, N, config.timestep_shift,
                                      lat.device, out=None if out is None else out[1])
        if has_mask_input(config.model_type):
            # mgds RandomLatentMaskRemove (DataLoaderText2ImageMixin.py:270-276): which samples lose their mask this
            # step -- Philox stream 8 under the same seed and global-batch counter, written beside noise and timestep
            # outside a captured step; the validation pass removes none
            p = 0.0 if deterministic else float(getattr(config, "unmasked_probability", 0.0))
            unmask = K.inpaint_unmask(B, batch_seed, p, sample0=sample0, device=lat.device,
                                      out=None if out is None else out[2])
            return noise, timestep, unmask
        return noise, timestep

    def predict(self, model, batch: dict, config, train_progress, *, deterministic: bool = False,
                per_sample: bool = False) -> dict:
        config = plain(config)
        batch_seed = 0 if deterministic else train_progress.global_step
        rand = Random(batch_seed)
        latent = self._nhwc_latent(batch["latent_image"])
        B, h, w, C = latent.shape
        sf = model.vae.config["scaling_factor"]
        ehs, pooled = self._text(model, batch, config, rand, B, per_sample)
        if self.graph_inputs is not None and not per_sample:
            inputs = self.graph_inputs
        else:
            inputs = self.step_inputs(model, batch, config, train_progress, deterministic=deterministic,
                                      per_sample=per_sample)
        noise, timestep = inputs[0], inputs[1]
        ptype = model.noise_scheduler.config["prediction_type"]
        eff_mask = None
        if has_mask_input(config.model_type):
            for key in ("latent_mask", "latent_conditioning_image", "latent_blank"):
                if key not in batch:
                    raise KeyError(f"{key}: model type {config.model_type} has a mask input, but the batch carries "
                                   f"no '{key}' (a cache built without it?)")
            cond = self._nhwc_latent(batch["latent_conditioning_image"]).to(latent.dtype)
            unet_in, target, _, eff_mask = K.inpaint_prologue(
                latent, noise, timestep, model.noise_scheduler.coeffs, sf, 1 if ptype == "v_prediction" else 0,
                batch["latent_mask"].to(latent.device, torch.float32).contiguous(), cond,
                batch["latent_blank"].to(latent.device, torch.float32).contiguous(), inputs[2],
                want_mask=bool(config.masked_training))
        else:
            unet_in, target, _ = K.ddpm_prologue(latent, noise, timestep, model.noise_scheduler.coeffs, sf,
                                                 1 if ptype == "v_prediction" else 0)
        time_ids = None
        if model.unet.cfg.addition_embed:
            time_ids = torch.stack([batch["original_resolution"][0], batch["original_resolution"][1],
                                    batch["crop_offset"][0], batch["crop_offset"][1],
                                    batch["crop_resolution"][0], batch["crop_resolution"][1]], dim=1).to(
                latent.device, torch.float32)
        pred = model.unet(unet_in, timestep, ehs, pooled, time_ids)
        # the reference contract: predicted / target are [B, 4, h, w] (BaseStableDiffusionXLSetup.py:277-291);
        # here they are views of the NHWC kernel tensors (pred carries 4 zero pad channels), which
        # calculate_loss reads directly through the private keys
        return {"loss_type": "target", "timestep": timestep,
                "predicted": pred[..., :C].permute(0, 3, 1, 2), "target": target.permute(0, 3, 1, 2),
                "prediction_type": ptype, "_predicted_nhwc": pred, "_target_nhwc": target,
                **({} if eff_mask is None else {"_loss_mask": eff_mask})}

    def calculate_loss(self, model, batch: dict, data: dict, config) -> torch.Tensor:
        plan = loss_plan(plain(config))
        lw = batch.get("loss_weight")
        lw = lw.to(self.train_device, torch.float32).contiguous() if lw is not None else None
        pred, target = nhwc_pair(data, 4)
        v_pred = data.get("prediction_type") == "v_prediction"
        scale = float(plan["batch_size_scale"] * plan["ga_scale"])
        if plain_mse(plan):
            return Fn.MSELossFn.apply(pred, target, lw, data["timestep"], model.noise_scheduler.coeffs, plan["loss_fn"],
                                      plan["gamma"], v_pred, 1.0, plan["mse_strength"], scale, 1.0 / self.dp_world)
        strengths = (plan["mse_strength"], plan["mae_strength"], plan["log_cosh_strength"])
        return Fn.DiffusionLossFn.apply(pred, target, loss_mask(batch, plan, self.train_device, data), lw,
                                        data["timestep"],
                                        model.noise_scheduler.coeffs, plan["loss_fn"], plan["gamma"], v_pred, 1.0,
                                        strengths, plan["unmasked_weight"], plan["normalize"], scale,
                                        1.0 / self.dp_world)

    def validation_losses(self, model, batch: dict, data: dict, config) -> torch.Tensor:
        """per-sample losses f32 [B] of predict()'s output, forward only (per_sample_losses)"""
        return per_sample_losses(model, batch, data, loss_plan(plain(config)), 4, self.train_device,
                                 model.noise_scheduler.coeffs, data.get("prediction_type") == "v_prediction")
