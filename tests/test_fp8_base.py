"""weight_dtype FLOAT_8 through the layers: the dtype plan (CPU); the adapter gradients of the tiny LoRA networks on an
fp8 base against the float64 oracle holding dq(W8); two trainer steps on an fp8 base against a bf16 base holding dq(W8).
Gradient bounds: _grad_parity.py's per-tensor scale and relative-L2 bounds (4 x the noise k of a bf16 network against
float64): the fp8 network is a bf16 network on dq with two more bf16 roundings per adapted GEMM; two HIP runs, each
within k of the truth, are within 2 k of each other.  Losses: the LoRA oracle step tests' rtol.  Adapter weights are
held to their bound through these gradients: AdamW moves every element by about lr whatever its gradient, so
comparing the weights after two steps (any two runs lie within 4 lr) could not fail."""
import pytest
import torch

import _grad_parity as G
from onetrainer_amd.dataLoader import SyntheticDataLoader as D
from onetrainer_amd.module import flux as FX, unet as U
from onetrainer_amd.module.lora import LoRAWrapper
from onetrainer_amd.trainer.GenericTrainer import GenericTrainer
from onetrainer_amd.util import create

from onetrainer_amd.util.config.TrainConfig import TrainConfig
from onetrainer_amd.util.dtype_util import dtype_plan

LR = 3e-4


def lora_cfg(kind, weight_dtype):
    cfg = TrainConfig.default_values()
    if kind == "flux":
        cfg.model_type, cfg.timestep_distribution = "FLUX_DEV_1", "LOGIT_NORMAL"
    cfg.training_method, cfg.train_dtype, cfg.weight_dtype = "LORA", "BFLOAT_16", weight_dtype
    cfg.batch_size, cfg.learning_rate, cfg.learning_rate_warmup_steps = 2, LR, 0
    cfg.lora_rank, cfg.lora_alpha = 8, 8.0
    cfg.optimizer.stochastic_rounding = False
    return cfg


@pytest.mark.parametrize("kind", ["sdxl", "flux"])
def test_dtype_plan_honours_float8_for_plain_lora(kind):
    field = ("prior" if kind == "flux" else "unet") + ".weight_dtype"
    plan = dtype_plan(lora_cfg(kind, "FLOAT_8"))
    assert plan.network == "FLOAT_8" and not [o for o in plan.overrides if o["field"] == field]
    dora = lora_cfg(kind, "FLOAT_8")
    dora.lora_decompose = True
    for cfg in (dora, lora_cfg(kind, "NFLOAT_4")):
        plan = dtype_plan(cfg)
        assert plan.network == "BFLOAT_16" and [o["build"] for o in plan.overrides if o["field"] == field] == ["BFLOAT_16"]
    ft = lora_cfg(kind, "FLOAT_8")
    ft.training_method = "FINE_TUNE"
    with pytest.raises(ValueError, match="cannot be fine-tuned"):
        dtype_plan(ft)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny_sdxl_lora", "tiny_flux_lora"])
def test_adapter_gradients_on_fp8_base_match_float64_on_dq(name):
    """one backward with trained-size adapters, so that u A reaches dx and r = t (sB)^T the output: every adapter
    gradient against the float64 oracle on dq(W8)"""
    from test_grad_parity_gpu import _grads, _micro_step
    dev, c = torch.device("cuda:0"), G.make_case(name)
    if c["flux"]:
        m8 = FX.FluxTransformer2DModel(FX.tiny_flux_config(), dev, seed=None, trainable=False, fp8=True)
    else:
        m8 = U.UNet2DConditionModel(U.tiny_sdxl_config(), dev, seed=None, trainable=False, fp8=True)
    m8.load_state_dict(c["weights"])
    m8.lora = LoRAWrapper(m8, rank=G.LORA_RANK, alpha=G.LORA_ALPHA, prefix=c["prefix"], seed=0)
    m8.lora.load_state_dict(c["lora_sd"])
    assert m8.store.fp8_rows
    dq = {k: v.float().cpu() for k, v in m8.state_dict().items()}
    _micro_step(c, m8, m8.lora.store, c["batches"][0], dev, False)
    G.check(_grads(m8, m8.lora), G.oracle_grads(dict(c, weights=dq), torch.float64, (0,)), f"{name} fp8 vs float64 on dq")


def two_steps(kind, weight_dtype, base=None):
    dev = torch.device("cuda:0")
    cfg = lora_cfg(kind, weight_dtype)
    if kind == "flux":
        fcfg = FX.tiny_flux_config()
        model = create.create_model(cfg, dev, seed=3, flux_config=fcfg)
        batch = D.synthetic_flux_batch(2, 128, 128, dev, seed=1, t5_dim=fcfg.joint_attention_dim,
                                       pooled_dim=fcfg.pooled_projection_dim, text_len=9)
    else:
        model = create.create_model(cfg, dev, seed=3, unet_config=U.tiny_sdxl_config())
        batch = D.synthetic_sdxl_batch(2, 128, 128, dev, seed=1, te1_dim=48, te2_dim=48, pooled_dim=64)
    net = model.transformer if kind == "flux" else model.unet
    if base is not None:
        net.load_state_dict(base)
    tr = GenericTrainer(cfg, model=model)
    tr.start()
    lora = model.transformer_lora if kind == "flux" else model.unet_lora
    opt, step, grads = model.optimizer, model.optimizer.step, []

    def capture(*a, **k):   # the adapter gradients as the optimizer is about to read them
        grads.append({n: v.double().cpu() for n, v in lora.state_dict(grads=True).items() if not n.endswith(".alpha")})
        return step(*a, **k)

    opt.step = capture
    losses = [tr.train_step(batch).item() for _ in range(2)]
    return net, losses, grads


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["sdxl", "flux"])
def test_fp8_base_trains_like_its_dequantised_bf16_base(kind):
    net8, loss8, g8 = two_steps(kind, "FLOAT_8")
    st = net8.store
    assert st.fp8_rows and all(n.endswith(".weight") for n in st.fp8_rows)
    # no bf16 copy: the bf16 buffer holds the other tensors only (each padded to at most 8 elements)
    rest = [s for n, s in st.slots.items() if n not in st.fp8_rows]
    assert st.data.numel() <= sum(s.numel + 8 for s in rest)
    bf16_bytes = 2 * sum(st.slots[n].numel for n in st.fp8_rows)
    assert st.data8.numel() + 4 * st.scale_rows.numel() <= 0.51 * bf16_bytes + 4 * st.scale_rows.numel()
    net16, loss16, g16 = two_steps(kind, "BFLOAT_16", base=net8.state_dict())
    assert not net16.store.fp8_rows
    print(kind, "losses fp8", loss8, "bf16 on dq", loss16)
    for a, b in zip(loss8, loss16):
        assert abs(a - b) <= 1e-3 * abs(b), (loss8, loss16)
    assert loss8[1] != loss8[0]
    # the first backward starts from identical adapters: lora_up = 0, lora_down gradients exactly zero in both runs
    assert len(g8) == 2 and any(torch.count_nonzero(v) for v in g16[0].values())
    G.check(g8[0], g16[0], f"{kind} first-step adapter gradients, fp8 base vs bf16 base on dq")
