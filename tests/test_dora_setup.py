"""DoRA at the setup boundary, on the CPU (structure only, as LoRAWrapper's CPU path): a config with lora_decompose
builds a DoRAWrapper on a tiny frozen UNet and wires it as the UNet's merged-weight source; its state dict has the
reference's keys and shapes (tests/golden/dora_steps.npz naming); LoHa and FLUX + lora_decompose still refuse."""
from pathlib import Path

import numpy as np
import pytest
import torch

from onetrainer_amd.modelSetup.FluxLoRASetup import FluxLoRASetup
from onetrainer_amd.module import functional as Fn
from onetrainer_amd.module import unet as U
from onetrainer_amd.module.dora import DoRAWrapper, DoraRef
from onetrainer_amd.module.lora import LoRAWrapper
from onetrainer_amd.util import create
from onetrainer_amd.util.config.TrainConfig import TrainConfig

GOLD = Path(__file__).parent / "golden" / "dora_steps.npz"


def _cfg(**kw):
    cfg = TrainConfig.default_values()
    cfg.training_method = "LORA"
    cfg.lora_rank, cfg.lora_alpha = 4, 2.0
    cfg.lora_decompose = True
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _setup(cfg, monkeypatch):
    """setup_model on a CPU host: everything but the optimizer (its fused kernels need the GPU)"""
    import onetrainer_amd.modelSetup.StableDiffusionXLLoRASetup as M
    monkeypatch.setattr(M, "create_optimizer", lambda store, groups, config: None)
    monkeypatch.setattr(M, "restore_training_state", lambda model, config: None)
    model = create.create_model(cfg, "cpu", seed=3, unet_config=U.tiny_sdxl_config())
    create.create_model_setup(cfg, "cpu").setup_model(model, cfg)
    return model


@pytest.mark.parametrize("output_axis,eps", [(False, True), (True, False)])
def test_config_builds_dora_wrapper(monkeypatch, output_axis, eps):
    cfg = _cfg(lora_decompose_output_axis=output_axis, lora_decompose_norm_epsilon=eps, lora_layer_preset="attn-mlp")
    model = _setup(cfg, monkeypatch)
    w = model.unet_lora
    assert isinstance(w, DoRAWrapper) and model.unet.dora is w and model.unet.lora is None
    assert w.output_axis == output_axis and w.eps == (float(np.finfo(np.float32).eps) if eps else 0.0)
    assert model.train_store is w.store and w.store.trainable and not model.unet.store.trainable
    assert list(model.param_group_mapping) == ["unet_lora"]
    assert all("attentions" in m for s in w.sites for m in s.modules)
    # adapted GEMMs read the merged weight, everything else the base store; no LoRA site reaches the GEMMs
    q = "down_blocks.1.attentions.0.transformer_blocks.0.attn1."
    ref = model.unet.R([q + "to_q.weight", q + "to_k.weight", q + "to_v.weight"], (384, 128))
    assert isinstance(ref, DoraRef) and ref.trainable and ref.acc() is False and ref.w.shape == (384, 128)
    assert ref.g.shape == ref.w.shape and len(ref.params) == 9 and all(p.requires_grad for p in ref.params)
    assert isinstance(model.unet.R("conv_in.weight"), Fn.PRef) and isinstance(model.unet.R("conv_in.bias"), Fn.PRef)
    assert model.unet._lo(q + "to_q") is None and model.unet._lo_fused([q + "to_q", q + "to_k", q + "to_v"]) is None
    # up = 0 at init and dora_scale = the base norm: the merged weight would be the base weight; on the CPU the
    # structure-only wrapper holds the copy it was built with
    off, n = w.site_of[q + "to_q"].span
    b0, b1 = model.unet.store.range_of([q + "to_q.weight", q + "to_k.weight", q + "to_v.weight"])
    assert torch.equal(w.wp[off:off + n], model.unet.store.data[b0:b1])


def test_state_dict_has_the_reference_naming(monkeypatch):
    gold = np.load(GOLD)
    leaves = {k.split("/", 2)[2].split(".", 2)[2] for k in gold.files if k.startswith("in_eps/state/")}
    assert leaves == {"lora_down.weight", "lora_up.weight", "dora_scale", "alpha"}
    for output_axis, case in ((False, "in_eps"), (True, "out_eps")):
        w = DoRAWrapper(U.UNet2DConditionModel(U.tiny_sd15_config(), "cpu", trainable=False), rank=4, alpha=2.0,
                        decompose_output_axis=output_axis)
        sd = {k: v.clone() for k, v in w.state_dict().items()}   # contiguous slots come back as views of the store
        mods = {k[:-len(".alpha")] for k in sd if k.endswith(".alpha")}
        assert {k[len(m) + 1:] for m in mods for k in sd if k.startswith(m + ".")} == leaves
        # Linear, 3x3 conv (conv_in unpadded) and 1x1 conv (SD 1.5 proj_in) against the golden's Linear / conv / 1x1
        pairs = (("lora_unet.time_embedding.linear_1", "lin", 160, 640), ("lora_unet.conv_in", "conv", 4, 160),
                 ("lora_unet.down_blocks.0.attentions.0.proj_in", "pw", 160, 160))
        for mine, theirs, cin, cout in pairs:
            g = gold[f"{case}/state/lora_unet.{theirs}.dora_scale"]
            got = sd[mine + ".dora_scale"]
            assert got.dim() == g.ndim and got.dtype == torch.float32
            kept = cout if output_axis else cin
            want = tuple(kept if d > 1 else 1 for d in g.shape)
            assert tuple(got.shape) == want, (mine, tuple(got.shape), g.shape)
            assert sd[mine + ".lora_down.weight"].dim() == gold[f"{case}/state/lora_unet.{theirs}.lora_down.weight"].ndim
            assert sd[mine + ".lora_up.weight"].dim() == gold[f"{case}/state/lora_unet.{theirs}.lora_up.weight"].ndim
        # dora_scale starts as the norm of the base weight, in float32
        base = w.model.store.params["time_embedding.linear_1.weight"].float()
        want = base.norm(dim=1, keepdim=True) if output_axis else base.norm(dim=0, keepdim=True)
        assert torch.allclose(sd["lora_unet.time_embedding.linear_1.dora_scale"], want, rtol=1e-6, atol=0)
        # a round trip keeps every value; a plain-LoRA state dict leaves dora_scale alone
        before = w.store.data.clone()
        w.store.data.mul_(0.5)
        w.load_state_dict({k: v.clone() for k, v in sd.items()})
        assert torch.equal(before, w.store.data)
        half = {k: v * 0.5 for k, v in sd.items() if not k.endswith("dora_scale")}
        w.load_state_dict(half)
        assert torch.equal(w.state_dict()["lora_unet.conv_in.dora_scale"], sd["lora_unet.conv_in.dora_scale"])
        assert torch.equal(w.state_dict()["lora_unet.conv_in.lora_down.weight"], half["lora_unet.conv_in.lora_down.weight"])


def test_plain_lora_is_unchanged(monkeypatch):
    cfg = _cfg(lora_decompose=False)
    model = _setup(cfg, monkeypatch)
    assert type(model.unet_lora) is LoRAWrapper and model.unet.lora is model.unet_lora and model.unet.dora is None
    assert not any(k.endswith("dora_scale") for k in model.unet_lora.state_dict())


def test_loha_dropout_and_flux_still_refuse(monkeypatch):
    with pytest.raises(NotImplementedError, match="LoHa"):
        _setup(_cfg(peft_type="LOHA"), monkeypatch)
    with pytest.raises(NotImplementedError, match="LoHa"):
        _setup(_cfg(peft_type="LOHA", lora_decompose=False), monkeypatch)
    with pytest.raises(NotImplementedError, match="dropout"):
        _setup(_cfg(dropout_probability=0.1), monkeypatch)
    cfg = _cfg(model_type="FLUX_DEV_1")
    with pytest.raises(NotImplementedError, match="DoRA"):
        FluxLoRASetup("cpu").setup_model(type("M", (), {})(), cfg)
