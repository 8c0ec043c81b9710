"""Factories (mirrors the parts of modules/util/create.py the hot path uses:
create_model_setup 285-353, create_optimizer 509-534 (ADAMW), 553-566 (ADAMW_8BIT), 752-767 (SCHEDULE_FREE_ADAMW), 863-881 (PRODIGY), 914-936 (ADAFACTOR) and 938-951 (CAME), create_lr_scheduler
1114-1232, create_noise_scheduler 1235-1373)."""
from __future__ import annotations

import torch

from ..model.StableDiffusionXLModel import NoiseScheduler, StableDiffusionXLModel
from ..module import unet as U
from ..util.lr_scheduler_util import create_lr_scheduler  # noqa: F401  (re-export)
from .config.plain import plain
from .model_type import has_mask_input, unet_in_channels

SCALING = {"STABLE_DIFFUSION_XL_10_BASE": 0.13025, "STABLE_DIFFUSION_15": 0.18215,
           "STABLE_DIFFUSION_XL_10_BASE_INPAINTING": 0.13025, "STABLE_DIFFUSION_15_INPAINTING": 0.18215}


def is_flux(model_type: str) -> bool:
    return model_type.startswith("FLUX")


def check_in_channels(model_type: str, in_channels: int, c0: int = 320) -> None:
    """the UNet a checkpoint or a config declares against the model type: a 4-channel UNet under an inpainting type
    (or a 9-channel one under a plain type) is refused by the weight that would not fit"""
    want = unet_in_channels(model_type)
    if (int(in_channels) != 9) == has_mask_input(model_type):
        raise ValueError(f"conv_in.weight: shape {(c0, int(in_channels), 3, 3)} != {(c0, want, 3, 3)}: model type "
                         f"{model_type} takes a UNet with {want} input channels")


def create_model(config, device, seed=0, unet_config=None, prediction_type="epsilon", flux_config=None):
    """random-weight model of the configured architecture (weights from disk: SURVEY.md §8(f) #2).
    LoRA training keeps the base network frozen (no gradient buffer)."""
    from .dtype_util import dtype_plan
    config = plain(config)
    plan = dtype_plan(config)   # ValueError for a dtype setup the build cannot train, before any allocation
    mt = config.model_type
    if is_flux(mt):
        from ..model.FluxModel import FluxModel
        from ..module import flux as FX
        tr = FX.FluxTransformer2DModel(flux_config or FX.flux_dev_config(), device, seed=seed,
                                       trainable=config.training_method != "LORA", master=plan.master)
        m = FluxModel(tr, model_type=mt)
        m.dtype_plan = plan
        return m
    if unet_config is None:
        unet_config = _unet_config_on_disk(config)
    if unet_config is None:
        if mt.startswith("STABLE_DIFFUSION_XL"):
            unet_config = U.sdxl_config()
        elif is_sd15(mt):
            unet_config = U.sd15_config()
        else:
            raise NotImplementedError(f"model type {mt}")
        unet_config.in_channels = unet_in_channels(mt)
    check_in_channels(mt, unet_config.in_channels, unet_config.block_out_channels[0])
    unet = U.UNet2DConditionModel(unet_config, device, seed=seed, trainable=config.training_method != "LORA",
                                  master=plan.master)
    ns = NoiseScheduler(device, prediction_type=prediction_type)
    m = StableDiffusionXLModel(unet, ns, SCALING.get(mt, 0.13025), model_type=mt)
    m.dtype_plan = plan
    return m


def _unet_config_on_disk(config):
    """the architecture a diffusers-layout model directory declares (`unet/config.json`, as
    diffusers' from_pretrained reads it): the backup continued from, else base_model_name.
    Single-file checkpoints carry no config and keep the model type's architecture."""
    import json
    import os
    names = []
    if getattr(config, "continue_last_backup", False) and config.training_method != "LORA":
        last = config.get_last_backup_path() if hasattr(config, "get_last_backup_path") else None
        names.append(last)
    names.append(getattr(config, "base_model_name", None))
    for name in names:
        path = os.path.join(name, "unet", "config.json") if name else None
        if path and os.path.isfile(path):
            with open(path) as f:
                return U.unet_config_from_diffusers(json.load(f))
    return None


def is_sd15(model_type: str) -> bool:
    return model_type.startswith("STABLE_DIFFUSION_15") or model_type in ("STABLE_DIFFUSION_15_INPAINTING",)


def create_model_setup(config, train_device, dp_rank=0, dp_world=1):
    """ModelType x TrainingMethod -> plugin (create.py:285-353)."""
    config = plain(config)
    if is_flux(config.model_type):
        if config.training_method == "LORA":
            from ..modelSetup.FluxLoRASetup import FluxLoRASetup as S
        elif config.training_method == "FINE_TUNE":
            from ..modelSetup.FluxFineTuneSetup import FluxFineTuneSetup as S
        else:
            raise NotImplementedError(f"training method {config.training_method}")
        return S(train_device, dp_rank=dp_rank, dp_world=dp_world)
    sd15 = is_sd15(config.model_type)
    if not sd15 and not config.model_type.startswith("STABLE_DIFFUSION_XL"):
        raise NotImplementedError(f"model type {config.model_type}")
    if config.training_method == "FINE_TUNE":
        if sd15:
            from ..modelSetup.StableDiffusionFineTuneSetup import StableDiffusionFineTuneSetup as S
        else:
            from ..modelSetup.StableDiffusionXLFineTuneSetup import StableDiffusionXLFineTuneSetup as S
        return S(train_device, dp_rank=dp_rank, dp_world=dp_world)
    if config.training_method == "LORA":
        if sd15:
            from ..modelSetup.StableDiffusionLoRASetup import StableDiffusionLoRASetup as S
        else:
            from ..modelSetup.StableDiffusionXLLoRASetup import StableDiffusionXLLoRASetup as S
        return S(train_device, dp_rank=dp_rank, dp_world=dp_world)
    raise NotImplementedError(f"training method {config.training_method}")


def adafactor_options(oc) -> dict:
    """OptimizerConfig -> transformers.Adafactor arguments, None resolved exactly as create.py:922-934 resolves it
    (scale_parameter and relative_step fall back to True there; the UI defaults, optimizer_util.py:70-82, set both
    False explicitly, and an explicit value wins)."""
    def pick(name, default):
        v = getattr(oc, name, None)
        return v if v is not None else default
    return dict(eps=pick("eps", 1e-30), eps2=pick("eps2", 1e-3), clip_threshold=pick("clip_threshold", 1.0),
                decay_rate=pick("decay_rate", -0.8), beta1=getattr(oc, "beta1", None),
                weight_decay=pick("weight_decay", 0.0), scale_parameter=pick("scale_parameter", True),
                relative_step=pick("relative_step", True), warmup_init=pick("warmup_init", False))


def came_options(oc) -> dict:
    """OptimizerConfig -> CAME arguments, None resolved exactly as create.py:944-949 resolves it (clip_threshold is
    not passed there: it stays the class default 1.0)."""
    def pick(name, default):
        v = getattr(oc, name, None)
        return v if v is not None else default
    return dict(eps=pick("eps", 1e-30), eps2=pick("eps2", 1e-16), beta1=pick("beta1", 0.9), beta2=pick("beta2", 0.999),
                beta3=pick("beta3", 0.9999), weight_decay=pick("weight_decay", 0))


def prodigy_options(oc) -> dict:
    """OptimizerConfig -> prodigyopt.Prodigy arguments, None resolved exactly as create.py:865-880 resolves it (beta3
    stays None there: the optimizer takes sqrt(beta2))."""
    def pick(name, default):
        v = getattr(oc, name, None)
        return v if v is not None else default
    return dict(beta1=pick("beta1", 0.9), beta2=pick("beta2", 0.999), beta3=pick("beta3", None), eps=pick("eps", 1e-8),
                weight_decay=pick("weight_decay", 0), decouple=pick("decouple", True),
                use_bias_correction=pick("use_bias_correction", False),
                safeguard_warmup=pick("safeguard_warmup", False), d0=pick("d0", 1e-6), d_coef=pick("d_coef", 1.0),
                growth_rate=pick("growth_rate", float("inf")), fsdp_in_use=pick("fsdp_in_use", False),
                slice_p=pick("slice_p", 1))


def check_prodigy(o, oc, groups):
    """what the fused Prodigy does not do, refused by the option's name before anything is allocated"""
    if o["slice_p"] != 1:
        raise NotImplementedError(f"PRODIGY slice_p={o['slice_p']}: only slice_p 1 (every element feeds the step-size "
                                  "estimate) is on the hot path")
    if o["fsdp_in_use"]:
        raise NotImplementedError("PRODIGY fsdp_in_use: sharded parameters are not supported (data parallel keeps "
                                  "whole, all-reduced gradients on every rank)")
    if getattr(oc, "fused_back_pass", False):
        raise NotImplementedError("PRODIGY fused_back_pass: the step needs sums over the whole store, so no "
                                  "parameter can be updated during the backward pass")
    lrs = sorted({float(g["lr"]) for g in groups if "lr" in g})
    if len(lrs) > 1:
        raise NotImplementedError(f"PRODIGY learning_rate: parameter groups with different learning rates {lrs} are "
                                  "not supported (d is one estimate for the whole store)")


def schedule_free_options(oc) -> dict:
    """OptimizerConfig -> schedulefree.AdamWScheduleFree arguments, None resolved exactly as create.py:759-766
    resolves it (warmup_steps is not an optimizer option there: it is config.learning_rate_warmup_steps)."""
    def pick(name, default):
        v = getattr(oc, name, None)
        return v if v is not None else default
    return dict(beta1=pick("beta1", 0.9), beta2=pick("beta2", 0.999), weight_decay=pick("weight_decay", 1e-2),
                eps=pick("eps", 1e-8), r=pick("r", 0), weight_lr_power=pick("weight_lr_power", 2.0),
                foreach=pick("foreach", False))


def adamw8bit_options(oc) -> dict:
    """OptimizerConfig -> bnb.optim.AdamW8bit arguments, None resolved exactly as create.py:558-565 resolves it"""
    def pick(name, default):
        v = getattr(oc, name, None)
        return v if v is not None else default
    return dict(beta1=pick("beta1", 0.9), beta2=pick("beta2", 0.999), weight_decay=pick("weight_decay", 1e-2),
                eps=pick("eps", 1e-8), min_8bit_size=pick("min_8bit_size", 4096),
                percentile_clipping=pick("percentile_clipping", 100), block_wise=pick("block_wise", True),
                is_paged=pick("is_paged", False))


def check_adamw8bit(o, oc, lr, groups):
    """what the fused 8-bit AdamW does not do, refused by the option's name before anything is allocated"""
    if not o["block_wise"]:
        raise NotImplementedError("ADAMW_8BIT block_wise=False: only the block-wise quantisation (blocks of 256) is "
                                  "on the hot path")
    if o["percentile_clipping"] != 100:
        raise NotImplementedError(f"ADAMW_8BIT percentile_clipping={o['percentile_clipping']}: only 100 (no "
                                  "percentile clipping of the gradient norm) is on the hot path")
    if o["is_paged"]:
        raise NotImplementedError("ADAMW_8BIT is_paged: paged optimizer state is not supported (the state stays in "
                                  "device memory)")
    if getattr(oc, "fused_back_pass", False):
        raise NotImplementedError("ADAMW_8BIT fused_back_pass: the 8-bit step is one launch over the whole store")
    from .optimizer.adamw8bit_fused import check_hyper
    for lr_ in [lr] + [g["lr"] for g in groups if "lr" in g]:
        check_hyper(dict(betas=(o["beta1"], o["beta2"]), eps=o["eps"], lr=lr_, weight_decay=o["weight_decay"]))


def create_optimizer(store, groups, config):
    """the fused optimizer over `store` for config.optimizer (create.py:509-534 ADAMW + patch_adamw, 914-936
    ADAFACTOR + patch_adafactor, 938-951 CAME, 863-881 PRODIGY, 752-767 SCHEDULE_FREE_ADAMW, 553-566 ADAMW_8BIT).
    Anything else is refused: there is no eager fall-back."""
    config = plain(config)
    oc = config.optimizer
    name = str(oc.optimizer)
    if name == "ADAMW":
        from .optimizer.adamw_fused import FusedAdamW
        return FusedAdamW(store, groups, lr=config.learning_rate,
                          betas=(oc.beta1 if oc.beta1 is not None else 0.9,
                                 oc.beta2 if oc.beta2 is not None else 0.999),
                          eps=oc.eps if oc.eps is not None else 1e-8,
                          weight_decay=oc.weight_decay if oc.weight_decay is not None else 1e-2,
                          stochastic_rounding=oc.stochastic_rounding)
    if name == "ADAFACTOR":
        from .optimizer.adafactor_fused import FusedAdafactor
        o = adafactor_options(oc)
        if str(getattr(config, "learning_rate_scheduler", "CONSTANT")) == "ADAFACTOR":
            raise NotImplementedError("learning_rate_scheduler ADAFACTOR (relative_step) is not on the hot path: "
                                      "set relative_step=False and a learning rate")
        return FusedAdafactor(store, groups, lr=config.learning_rate, eps=(o["eps"], o["eps2"]),
                              clip_threshold=o["clip_threshold"], decay_rate=o["decay_rate"], beta1=o["beta1"],
                              weight_decay=o["weight_decay"], scale_parameter=o["scale_parameter"],
                              relative_step=o["relative_step"], warmup_init=o["warmup_init"],
                              stochastic_rounding=bool(oc.stochastic_rounding))
    if name == "CAME":
        from .optimizer.came_fused import FusedCAME
        o = came_options(oc)
        return FusedCAME(store, groups, lr=config.learning_rate, eps=(o["eps"], o["eps2"]),
                         betas=(o["beta1"], o["beta2"], o["beta3"]), weight_decay=o["weight_decay"],
                         stochastic_rounding=bool(oc.stochastic_rounding))
    if name == "PRODIGY":
        o = prodigy_options(oc)
        check_prodigy(o, oc, groups)
        from .optimizer.prodigy_fused import FusedProdigy
        return FusedProdigy(store, groups, lr=config.learning_rate, betas=(o["beta1"], o["beta2"]), beta3=o["beta3"],
                            eps=o["eps"], weight_decay=o["weight_decay"], decouple=o["decouple"],
                            use_bias_correction=o["use_bias_correction"], safeguard_warmup=o["safeguard_warmup"],
                            d0=o["d0"], d_coef=o["d_coef"], growth_rate=o["growth_rate"],
                            stochastic_rounding=bool(oc.stochastic_rounding))
    if name == "SCHEDULE_FREE_ADAMW":
        o = schedule_free_options(oc)
        if getattr(oc, "fused_back_pass", False):
            raise NotImplementedError("SCHEDULE_FREE_ADAMW fused_back_pass: the reference offers the fused back pass "
                                      "for other optimizers only")
        from .optimizer.schedule_free_fused import FusedScheduleFreeAdamW
        # create.py:763: the raw warm-up steps, not divided by the gradient accumulation; the LR scheduler's own
        # warm-up drives group['lr'] on top of it, as in the reference
        return FusedScheduleFreeAdamW(store, groups, lr=config.learning_rate, betas=(o["beta1"], o["beta2"]),
                                      weight_decay=o["weight_decay"], eps=o["eps"],
                                      warmup_steps=config.learning_rate_warmup_steps, r=o["r"],
                                      weight_lr_power=o["weight_lr_power"], foreach=o["foreach"],
                                      stochastic_rounding=bool(oc.stochastic_rounding))
    if name == "ADAMW_8BIT":
        o = adamw8bit_options(oc)
        check_adamw8bit(o, oc, config.learning_rate, groups)
        from .optimizer.adamw8bit_fused import FusedAdamW8bit
        return FusedAdamW8bit(store, groups, lr=config.learning_rate, betas=(o["beta1"], o["beta2"]),
                              weight_decay=o["weight_decay"], eps=o["eps"], min_8bit_size=o["min_8bit_size"],
                              stochastic_rounding=bool(oc.stochastic_rounding))
    raise NotImplementedError(f"optimizer {name}: only ADAMW, ADAFACTOR and CAME (with a learning rate of "
                              "your choice), PRODIGY (which estimates it), SCHEDULE_FREE_ADAMW (which needs no "
                              "schedule) and ADAMW_8BIT (block-wise 8-bit moments) are on the hot path")


def create_ema(store, state_dict, config):
    """the EMA of the weights in `store` for config.ema (create.py:1089-1111): OFF -> None, GPU -> a shadow beside
    the store, CPU -> a host shadow; a saved state (ema/ema.pt of a backup) is loaded into it.  Any other mode is
    refused by name."""
    config = plain(config)
    mode = str(config.ema)
    if mode == "OFF":
        return None
    if mode == "GPU":
        device = store.device
    elif mode == "CPU":
        device = torch.device("cpu")
    else:
        raise NotImplementedError(f"ema mode {mode}: OFF, GPU and CPU are supported")
    from ..module.ema import FlatStoreEMA
    ema = FlatStoreEMA(store, decay=config.ema_decay, update_step_interval=config.ema_update_step_interval,
                       device=device, fp32_shadow=bool(config.ema_fp32))
    if state_dict is not None:
        ema.load_state_dict(state_dict)
    return ema
