"""Full fine-tune plugin (mirrors modules/modelSetup/StableDiffusionXLFineTuneSetup.py:26-164):
parameter groups, optimizer creation (util/create.py create_optimizer: fused AdamW, Adafactor, CAME or Prodigy), device placement."""
from __future__ import annotations

import torch

from ..util.dtype_util import dtype_plan
from ..util.NamedParameterGroup import NamedParameterGroup, NamedParameterGroupCollection
from ..util.create import create_optimizer
from ..util.optimizer_util import restore_training_state
from .BaseStableDiffusionXLSetup import BaseStableDiffusionXLSetup
from ..util.config.plain import plain


class StableDiffusionXLFineTuneSetup(BaseStableDiffusionXLSetup):
    def create_parameters(self, model, config) -> NamedParameterGroupCollection:
        config = plain(config)
        pgc = NamedParameterGroupCollection()
        if config.unet.train:
            pgc.add_group(NamedParameterGroup("unet", model.unet.parameters(), config.unet.learning_rate))
        if config.text_encoder.train or config.text_encoder_2.train:
            raise NotImplementedError("text-encoder training is outside this build's hot path (text is cached)")
        return pgc

    def setup_optimizations(self, model, config):
        # no gradient checkpointing: 288 GB HBM holds every activation;
        # no autocast: the kernels fix the compute dtype (bf16 GEMMs, fp32 norms/softmax/loss)
        config = plain(config)
        model.dtype_plan = dtype_plan(config)   # util/dtype_util.py: the config's dtypes honoured, overridden or refused
        model.train_dtype = torch.bfloat16

    def setup_model(self, model, config):
        config = plain(config)
        self.setup_optimizations(model, config)
        params = self.create_parameters(model, config)
        model.parameters = params
        model.optimizer = create_optimizer(model.unet.store, params.parameters_for_optimizer(config), config)
        model.param_group_mapping = params.unique_name_mapping()
        restore_training_state(model, config)

    def setup_train_device(self, model, config):
        config = plain(config)
        pass   # model and data are created on the train device

    def after_optimizer_step(self, model, config, train_progress):
        config = plain(config)
        pass
