"""LoRA plugin (mirrors modules/modelSetup/StableDiffusionXLLoRASetup.py:19-220): frozen bf16 UNet,
fp32 adapters on every Linear/Conv2d matching `lora_layers` (module/lora.py), parameter group
"unet_lora" (:66-72), fused fp32 AdamW over the adapter store (create.py:509-534 with
lora_weight_dtype FLOAT_32), shadow refresh after each update (the reference re-casts under
autocast on every forward).  With `lora_decompose` the adapters are DoRA (module/dora.py): the same store plus
dora_scale, and the refresh is the merge of every adapted weight."""
from __future__ import annotations

import torch

from ..util.dtype_util import dtype_plan
from ..module.dora import DoRAWrapper
from ..module.lora import PRESETS, LoRAUNetWrapper
from ..util.NamedParameterGroup import NamedParameterGroup, NamedParameterGroupCollection
from ..util.create import create_optimizer
from ..util.optimizer_util import restore_training_state
from .BaseStableDiffusionXLSetup import BaseStableDiffusionXLSetup
from ..util.config.plain import plain


class StableDiffusionXLLoRASetup(BaseStableDiffusionXLSetup):
    def create_parameters(self, model, config) -> NamedParameterGroupCollection:
        config = plain(config)
        pgc = NamedParameterGroupCollection()
        if config.text_encoder.train or config.text_encoder_2.train:
            raise NotImplementedError("text-encoder LoRA is outside this build's hot path (text is cached)")
        if config.unet.train:
            pgc.add_group(NamedParameterGroup("unet_lora", model.unet_lora.parameters(),
                                              config.unet.learning_rate))
        return pgc

    def setup_optimizations(self, model, config):
        config = plain(config)
        model.dtype_plan = dtype_plan(config)   # util/dtype_util.py: the config's dtypes honoured, overridden or refused
        model.train_dtype = torch.bfloat16

    @staticmethod
    def layer_filter(config):
        config = plain(config)
        if config.lora_layers:
            return config.lora_layers.split(",")
        return PRESETS.get(config.lora_layer_preset or "full", [])

    def setup_model(self, model, config):
        config = plain(config)
        if config.peft_type != "LORA":
            raise NotImplementedError("LoHa is not on this build's hot path")
        decompose = bool(getattr(config, "lora_decompose", False))
        dropout = float(config.dropout_probability or 0.0)
        if decompose and dropout > 0:
            raise NotImplementedError("DoRA with LoRA dropout > 0 is not on this build's hot path")
        if model.unet.store.trainable:
            raise ValueError("LoRA training needs a frozen base UNet (create_model(..., training_method='LORA'))")
        self.setup_optimizations(model, config)
        if model.unet_lora is None and decompose:   # DoRA (LoRAModuleWrapper with lora_decompose): module/dora.py
            model.unet_lora = DoRAWrapper(model.unet, rank=config.lora_rank, alpha=config.lora_alpha,
                                          module_filter=self.layer_filter(config), seed=0,
                                          norm_epsilon=bool(getattr(config, "lora_decompose_norm_epsilon", True)),
                                          decompose_output_axis=bool(getattr(config, "lora_decompose_output_axis",
                                                                             False)))
        if model.unet_lora is None:
            model.unet_lora = LoRAUNetWrapper(model.unet, rank=config.lora_rank, alpha=config.lora_alpha,
                                              module_filter=self.layer_filter(config), seed=0)
        if getattr(model, "lora_state_dict", None) is not None:   # LoRA file / backup (LoRALoaderMixin)
            model.unet_lora.load_state_dict(model.lora_state_dict)
            model.lora_state_dict = None
        if isinstance(model.unet_lora, DoRAWrapper):
            if dropout > 0:
                raise NotImplementedError("DoRA with LoRA dropout > 0 is not on this build's hot path")
            model.unet.dora = model.unet_lora
        else:
            model.unet.lora = model.unet_lora
            # LoRAModuleWrapper.set_dropout (LoRAModule.py:580-587); the masks are seeded per step (step_inputs) and
            # each data-parallel rank draws its rows of the global batch's mask
            model.unet_lora.set_dropout(dropout)
            model.unet_lora.dp_rank = self.dp_rank
        params = self.create_parameters(model, config)
        model.parameters = params
        model.optimizer = create_optimizer(model.unet_lora.store, params.parameters_for_optimizer(config), config)
        model.param_group_mapping = params.unique_name_mapping()
        restore_training_state(model, config)

    def setup_train_device(self, model, config):
        config = plain(config)
        pass

    def after_optimizer_step(self, model, config, train_progress):
        config = plain(config)
        model.unet_lora.refresh()
