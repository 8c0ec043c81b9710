"""LoRA dropout on the CPU: the mask oracle's own properties (tests/_oracle_lora_dropout.py; the GPU kernel is held to
it bit for bit in test_lora_dropout_gpu.py) and the setup boundary (dropout_probability reaches the wrapper for SDXL
and SD 1.5, the wrapper refuses rates outside [0, 1], the FLUX option check accepts dropout for plain LoRA)."""
import math

import numpy as np
import pytest

import _oracle_lora_dropout as O
from onetrainer_amd.modelSetup.FluxLoRASetup import FluxLoRASetup
from onetrainer_amd.module import unet as U
from onetrainer_amd.module.lora import LoRAWrapper
from onetrainer_amd.util import create
from onetrainer_amd.util.config.TrainConfig import TrainConfig


def test_thresholds():
    assert O.consts(0.0) == (0, 1.0)
    assert O.consts(1.0) == (2 ** 32, math.inf)
    assert O.consts(0.5) == (2 ** 31, 2.0)
    thr, scale = O.consts(0.1)
    assert thr == int(0.1 * 2 ** 32) and scale == float(np.float32(1 / 0.9))


@pytest.mark.parametrize("seed", [0, 2 ** 32 + 5, 2 ** 64 - 1])
def test_p0_keeps_all_p1_keeps_none(seed):
    assert O.keep_mask(seed, 3, 11, 63, 6, 0.0).all()
    assert not O.keep_mask(seed, 3, 11, 63, 6, 1.0).any()


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_kept_share(p):
    """n = 2^20 independent draws, each kept with probability 1 - thr / 2^32 (within 2^-32 of 1 - p): the kept count is
    binomial, its share has standard deviation sqrt(p (1 - p) / n), and 5 of them bound it (2-sided tail ~6e-7)."""
    n = 2 ** 20
    keep = O.keep_mask(1234, 5, 0, n // 128, 128, p)
    assert keep.size == n
    sd = math.sqrt(p * (1 - p) / n)
    share = keep.mean()
    print(f"p={p}: kept share {share:.6f}, expected {1 - p}, 5 sd = {5 * sd:.6f}")
    assert abs(share - (1 - p)) <= 5 * sd + 2.0 ** -32


def test_seeds_and_sites_give_other_masks():
    a = O.keep_mask(7, 0, 0, 64, 96, 0.5)
    assert not np.array_equal(a, O.keep_mask(8, 0, 0, 64, 96, 0.5))
    assert not np.array_equal(a, O.keep_mask(7 + 2 ** 32, 0, 0, 64, 96, 0.5))   # the key's high word counts
    assert not np.array_equal(a, O.keep_mask(7, 1, 0, 64, 96, 0.5))
    assert not np.array_equal(a, O.keep_mask(7, 793, 0, 64, 96, 0.5))
    assert np.array_equal(a, O.keep_mask(7, 0, 0, 64, 96, 0.5))


@pytest.mark.parametrize("width", [6, 32, 96])
def test_rank_slice_of_the_global_mask(width):
    """rows [B/2 rps, B rps) of the global batch's mask are the mask drawn with row0 = B/2 rps: what rank 1 of two
    data-parallel ranks draws (rows are sample-major, rps rows per sample)"""
    B, rps = 4, 37
    g = O.keep_mask(21, 9, 0, B * rps, width, 0.3)
    assert np.array_equal(g[B // 2 * rps:], O.keep_mask(21, 9, B // 2 * rps, B // 2 * rps, width, 0.3))
    assert np.array_equal(g[:B // 2 * rps], O.keep_mask(21, 9, 0, B // 2 * rps, width, 0.3))


# ------------------------------------------------------------------------------------------
def _cfg(**kw):
    cfg = TrainConfig.default_values()
    cfg.training_method = "LORA"
    cfg.lora_rank, cfg.lora_alpha = 4, 2.0
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _setup(cfg, monkeypatch, ucfg):
    """setup_model on a CPU host: everything but the optimizer (its fused kernels need the GPU)"""
    import onetrainer_amd.modelSetup.StableDiffusionXLLoRASetup as M
    monkeypatch.setattr(M, "create_optimizer", lambda store, groups, config: None)
    monkeypatch.setattr(M, "restore_training_state", lambda model, config: None)
    model = create.create_model(cfg, "cpu", seed=3, unet_config=ucfg)
    setup = create.create_model_setup(cfg, "cpu")
    setup.setup_model(model, cfg)
    return model, setup


@pytest.mark.parametrize("model_type", ["STABLE_DIFFUSION_XL_10_BASE", "STABLE_DIFFUSION_15"])
def test_config_sets_the_wrappers_dropout(monkeypatch, model_type):
    sd15 = model_type == "STABLE_DIFFUSION_15"
    cfg = _cfg(dropout_probability=0.1)
    if sd15:
        cfg.model_type = model_type
    model, setup = _setup(cfg, monkeypatch, U.tiny_sd15_config() if sd15 else U.tiny_sdxl_config())
    assert type(setup).__name__ == ("StableDiffusionLoRASetup" if sd15 else "StableDiffusionXLLoRASetup")
    w = model.unet_lora
    assert type(w) is LoRAWrapper and model.unet.lora is w
    assert w.dropout_p == 0.1
    assert [s.site_id for s in w.sites] == list(range(len(w.sites))) and all(s.wrapper is w for s in w.sites)
    assert all(s.drop() is w for s in w.sites)
    assert w.drop_seed.shape == (1,) and str(w.drop_seed.dtype) == "torch.int64"
    assert setup.graphable(cfg)
    # the default stays off, and then no site reports a dropout
    model0, _ = _setup(_cfg(), monkeypatch, U.tiny_sd15_config() if sd15 else U.tiny_sdxl_config())
    assert model0.unet_lora.dropout_p == 0.0 and all(s.drop() is None for s in model0.unet_lora.sites)


def test_set_dropout_refuses_rates_outside_0_1():
    w = LoRAWrapper(U.UNet2DConditionModel(U.tiny_sd15_config(), "cpu", trainable=False), rank=4, alpha=2.0)
    assert w.dropout_p == 0.0
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            w.set_dropout(bad)
    assert w.dropout_p == 0.0
    for ok in (0.0, 0.25, 1.0):
        w.set_dropout(ok)
        assert w.dropout_p == ok


def test_flux_option_check():
    assert FluxLoRASetup.check_options(_cfg(model_type="FLUX_DEV_1", dropout_probability=0.1)) == 0.1
    assert FluxLoRASetup.check_options(_cfg(model_type="FLUX_DEV_1")) == 0.0
    with pytest.raises(NotImplementedError, match="DoRA"):   # refused first, with the message it had
        FluxLoRASetup.check_options(_cfg(model_type="FLUX_DEV_1", dropout_probability=0.1, lora_decompose=True))
    with pytest.raises(NotImplementedError, match="LoHa"):
        FluxLoRASetup.check_options(_cfg(model_type="FLUX_DEV_1", dropout_probability=0.1, peft_type="LOHA"))
