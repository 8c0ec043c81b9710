"""Whole-network gradient parity: per-tensor scale, relative error and cosine against a float64 oracle.

Plain PyTorch on the CPU (as _norm_edges.py and _pointwise_edges.py): the case table, the oracles in any dtype, the
metrics and their bounds.  test_grad_parity_ref.py holds the constants to what this file recomputes;
test_grad_parity_gpu.py and the gradient loops of test_unet_gpu.py / test_lora_gpu.py / test_flux_gpu.py apply them to
the HIP networks.

Metrics   for one parameter tensor, g the gradient under test and r the float64 oracle gradient (both flattened):
            s   = <g, r> / <r, r>          the scale a cosine cannot see           |s - 1| <= S_BOUND
            rel = ||g - r|| / ||r||        the relative L2 error                   rel     <= REL_BOUND
            cos = <g, r> / (||g|| ||r||)   kept and printed
          A tensor whose r is identically zero has no s: g must then be exactly zero.  No case here has such a tensor
          (test_no_zero_reference_gradients): the LoRA cases draw lora_up at random, as test_dora_gpu.py does.

Oracle    oracle/unet.py, oracle/flux.py and oracle/lora.py in float64.  Weights, adapter weights, inputs and the
          upstream gradient are rounded to bf16 first, so the oracle, the bf16 CPU run and the HIP network all hold the
          same numbers.  The weights are the oracle's own initialisation (torch.manual_seed(WEIGHT_SEED)), so the table
          needs no GPU; the HIP models load them with load_state_dict.

Bounds    measured against the reference, never against the GPU.  The honest noise of a bf16 network is the same
          oracle converted to bf16 on the CPU (weights, activations, accumulated .grad all bf16; every oracle op has a
          CPU bf16 kernel, so no rounding hooks were needed), same inputs, same upstream gradient, against float64.
          k_s is the worst per-tensor |s - 1| and k_rel the worst per-tensor rel over all cases and over both forms:
          one backward of micro-batch A, and A then B accumulated into one .grad (bf16 accumulation, as the flat store
          accumulates).  Each k is taken up at its second significant digit (the project's one-step-up rule of K_TANH
          and K_BM at k's own magnitude) and S_BOUND = 4 k_s, REL_BOUND = 4 k_rel: the factor 4 covers the other
          rounding points of the HIP network (fp32 accumulators but bf16 activations and gradient stores, hardware
          exp2 and rcp).  Neither bound may exceed CAP = 0.25, so a factor 2 or 1/2, a dropped micro-batch or a sign
          flip can never pass; a case whose 4 k exceeded the cap would get other inputs, never another cap.

Measured  K_MEASURED below, per case, the larger of the one-pass and the two-pass form, with the tensor that showed it:
            tiny_sdxl       k_s 0.0144 (...attentions.1.transformer_blocks.0.norm1.weight)  k_rel 0.0399 (...ff.net.2.bias)
            tiny_sd15       k_s 0.0119 (...transformer_blocks.0.norm2.bias)                 k_rel 0.0412 (...norm1.bias)
            tiny_sdxl_lora  k_s 0.0201 (mid_block ...attn2.to_out.0.lora_down.weight)       k_rel 0.0470 (...ff.net.0.proj.lora_down)
            tiny_flux       k_s 0.0071 (transformer_blocks.0.attn.norm_added_q.weight)      k_rel 0.0221 (...attn.to_k.bias)
            tiny_flux_lora  k_s 0.0094 (...guidance_embedder.linear_1.lora_down.weight)     k_rel 0.0248 (...add_q_proj.lora_up)
          so k_s = 0.0201 -> 0.021, S_BOUND = 0.084, and k_rel = 0.0470 -> 0.047, REL_BOUND = 0.188, both inside the cap.

LoRA UNet the case's inputs were changed to stay inside the cap, as the rule above asks.  With the zero-mean upstream
          gradient of test_lora_gpu.py the bf16 oracle showed k_rel 0.055 to 0.098 over thirteen adapter seeds and
          three adapter magnitudes (4 k_rel up to 0.39), always on a lora_down of attn1.to_v, attn1.to_out.0 or
          time_emb_proj: the self-attention of a freshly initialised UNet is close to uniform, so these gradients are
          sums over tokens of a rank-8 projection of a zero-mean quantity, which cancel, and ||r|| is small against the
          network's per-element noise.  A mean of UP_MEAN_LORA_UNET = 3 in the upstream gradient (3 + randn) makes the
          sums coherent: k_rel 0.034 to 0.055 over three seeds, 0.0470 with the seed kept here.
"""
from __future__ import annotations

import functools
import math

import torch

from oracle import flux as OF
from oracle import unet as OU
from oracle.lora import OracleLoRA

CAP = 0.25
WEIGHT_SEED, LORA_SEED = 0, 4
LORA_RANK, LORA_ALPHA = 8, 4.0
UP_MEAN_LORA_UNET = 3.0   # the mean of the LoRA UNet case's upstream gradient: the docstring
CASES = ("tiny_sdxl", "tiny_sd15", "tiny_sdxl_lora", "tiny_flux", "tiny_flux_lora")

# per case: (k_s, tensor), (k_rel, tensor) of the bf16 CPU oracle against the float64 oracle (test_bounds_measured)
K_MEASURED = {
    "tiny_sdxl": {"k_s": (0.0144, "down_blocks.1.attentions.1.transformer_blocks.0.norm1.weight"),
                  "k_rel": (0.0399, "down_blocks.1.attentions.0.transformer_blocks.1.ff.net.2.bias")},
    "tiny_sd15": {"k_s": (0.0119, "down_blocks.0.attentions.1.transformer_blocks.0.norm2.bias"),
                  "k_rel": (0.0412, "down_blocks.0.attentions.1.transformer_blocks.0.norm1.bias")},
    "tiny_sdxl_lora": {"k_s": (0.0201, "lora_unet.mid_block.attentions.0.transformer_blocks.0.attn2.to_out.0.lora_down.weight"),
                       "k_rel": (0.0470, "lora_unet.mid_block.attentions.0.transformer_blocks.1.ff.net.0.proj.lora_down.weight")},
    "tiny_flux": {"k_s": (0.0071, "transformer_blocks.0.attn.norm_added_q.weight"),
                  "k_rel": (0.0221, "single_transformer_blocks.1.attn.to_k.bias")},
    "tiny_flux_lora": {"k_s": (0.0094, "lora_transformer.time_text_embed.guidance_embedder.linear_1.lora_down.weight"),
                       "k_rel": (0.0248, "lora_transformer.transformer_blocks.0.attn.add_q_proj.lora_up.weight")},
}


def ceil2(k: float) -> float:
    """k taken up at its second significant digit: 0.0143 -> 0.015, 0.043 -> 0.043, 1.822 -> 1.9"""
    if k <= 0:
        return 0.0
    q = 10.0 ** (math.floor(math.log10(k)) - 1)
    return round(math.ceil(k / q - 1e-9) * q, 12)


def _bounds():
    ks = max((v["k_s"][0] for v in K_MEASURED.values()), default=0.0)
    kr = max((v["k_rel"][0] for v in K_MEASURED.values()), default=0.0)
    return 4 * ceil2(ks), 4 * ceil2(kr)


def bf(x: torch.Tensor) -> torch.Tensor:
    """fp32 values that bf16 holds exactly"""
    return x.to(torch.bfloat16).float()


# ----- cases -------------------------------------------------------------------------------------------------------
def _unet_cfg(case):
    if case == "tiny_sd15":   # module/unet.py tiny_sd15_config, restated so that the table needs no HIP library
        return OU.UNetConfig(block_out_channels=(160, 320), down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"),
                             up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"), transformer_layers_per_block=(1, 1),
                             head_dim=None, num_heads=2, cross_attention_dim=96, use_linear_projection=False,
                             addition_embed=False, norm_num_groups=32)
    return OU.tiny_sdxl_config()


def _unet_batch(cfg, seed, t, up_mean=0.0):
    g = torch.Generator().manual_seed(seed)
    B, H, W = 2, 16, 16
    b = {"x": bf(torch.randn(B, 4, H, W, generator=g)), "t": torch.tensor(t, dtype=torch.int32),
         "ehs": bf(torch.randn(B, 77, cfg.cross_attention_dim, generator=g)), "te": None, "tid": None}
    if cfg.addition_embed:
        b["te"] = bf(torch.randn(B, cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim,
                                 generator=g))
        b["tid"] = torch.tensor([[128., 128., 0., 0., 128., 128.]] * B)
    b["up"] = bf(torch.randn(B, 4, H, W, generator=g) + up_mean)     # the upstream gradient, NCHW like the oracle's output
    return b


def _flux_batch(cfg, seed, t):
    g = torch.Generator().manual_seed(seed)
    B, h, w, L = 2, 16, 12, 7
    lat = torch.randn(B, cfg.in_channels // 4, h, w, generator=g)
    b = {"packed": bf(OF.pack_latents(lat)), "t": torch.tensor(t), "guid": torch.ones(B),
         "pooled": bf(torch.randn(B, cfg.pooled_projection_dim, generator=g)),
         "ehs": bf(torch.randn(B, L, cfg.joint_attention_dim, generator=g)), "h": h, "w": w, "L": L}
    b["up"] = bf(torch.randn(B, (h // 2) * (w // 2), cfg.in_channels, generator=g))   # [B, N, C] like the oracle's output
    return b


@functools.lru_cache(maxsize=None)
def make_case(case: str) -> dict:
    """weights (bf16-representable fp32, oracle names and shapes), adapter weights or None, micro-batches A and B
    (different inputs, timesteps and upstream gradients)"""
    flux, lora = "flux" in case, case.endswith("_lora")
    cfg = OF.tiny_flux_config() if flux else _unet_cfg(case)
    torch.manual_seed(WEIGHT_SEED)
    om = (OF.FluxTransformer2DModel if flux else OU.UNet2DConditionModel)(cfg)
    weights = {k: bf(v.detach()) for k, v in om.state_dict().items()}
    lora_sd = None
    if lora:
        prefix = "lora_transformer" if flux else "lora_unet"
        shapes = OracleLoRA(om, LORA_RANK, LORA_ALPHA, prefix=prefix).params
        g = torch.Generator().manual_seed(LORA_SEED)
        lora_sd = {k: bf(torch.randn(p.shape, generator=g) * (0.05 if flux else 0.1)) for k, p in shapes.items()}
    if flux:
        batches = (_flux_batch(cfg, 10, [0.537, 0.061]), _flux_batch(cfg, 11, [0.25, 0.9]))
    else:
        m = UP_MEAN_LORA_UNET if lora else 0.0
        batches = (_unet_batch(cfg, 10, [10, 700], m), _unet_batch(cfg, 11, [500, 3], m))
    return {"name": case, "flux": flux, "lora": lora, "cfg": cfg, "weights": weights, "lora_sd": lora_sd,
            "prefix": ("lora_transformer" if flux else "lora_unet") if lora else None, "batches": batches}


# ----- the oracle in any dtype -------------------------------------------------------------------------------------
def build_oracle(case: dict, dtype):
    """(model, {name: trained parameter}) of the oracle holding the case's weights in `dtype`"""
    om = (OF.FluxTransformer2DModel if case["flux"] else OU.UNet2DConditionModel)(case["cfg"])
    om.load_state_dict(case["weights"])
    om.to(dtype)
    if not case["lora"]:
        return om, dict(om.named_parameters())
    om.requires_grad_(False)
    ol = OracleLoRA(om, LORA_RANK, LORA_ALPHA, prefix=case["prefix"])
    ol.load_state_dict(case["lora_sd"])
    for p in ol.params.values():
        p.data = p.data.to(dtype)
    return om, ol.params


def oracle_forward(case: dict, om, b: dict, dtype):
    c = (lambda v: None if v is None else v.to(dtype))
    if case["flux"]:
        return om(c(b["packed"]), b["t"], b["guid"], c(b["pooled"]), c(b["ehs"]), torch.zeros(b["L"], 3),
                  OF.prepare_latent_image_ids(b["h"], b["w"]))
    return om(c(b["x"]), b["t"], c(b["ehs"]), c(b["te"]), b["tid"])


def oracle_grads(case: dict, dtype, which=(0,)) -> dict:
    """{name: float64 copy of .grad} after the backward passes of micro-batches `which`, in order, into one .grad
    (which accumulates in `dtype`, as the flat store's gradient buffer accumulates in its own)"""
    om, params = build_oracle(case, dtype)
    for i in which:
        b = case["batches"][i]
        (oracle_forward(case, om, b, dtype) * b["up"].to(dtype)).sum().backward()
    return {k: p.grad.detach().double() for k, p in params.items()}


@functools.lru_cache(maxsize=None)
def reference(name: str) -> dict:
    """the float64 oracle gradients of one case, computed once and shared: {"A", "B", "AB"}; treat as read-only"""
    case = make_case(name)
    a, b = oracle_grads(case, torch.float64, (0,)), oracle_grads(case, torch.float64, (1,))
    return {"A": a, "B": b, "AB": {k: a[k] + b[k] for k in a}}


@functools.lru_cache(maxsize=None)
def bf16_oracle(name: str) -> dict:
    """the bf16 CPU oracle's gradients (the noise level the bounds come from): A, B, and A then B into one .grad"""
    case = make_case(name)
    return {"A": oracle_grads(case, torch.bfloat16, (0,)), "B": oracle_grads(case, torch.bfloat16, (1,)),
            "AB": oracle_grads(case, torch.bfloat16, (0, 1))}


# ----- metrics -----------------------------------------------------------------------------------------------------
def metrics(g: torch.Tensor, r: torch.Tensor):
    """(|s - 1|, rel, cos) of one tensor, or None when r is identically zero"""
    g, r = g.detach().double().flatten().cpu(), r.detach().double().flatten().cpu()
    if g.numel() != r.numel():
        raise ValueError(f"gradient of {g.numel()} elements against a reference of {r.numel()}")
    rr = float(r @ r)
    if rr == 0.0:
        return None
    gr = float(g @ r)
    return abs(gr / rr - 1.0), float((g - r).norm()) / math.sqrt(rr), gr / (math.sqrt(rr) * float(g.norm()) + 1e-300)


def worst(grads: dict, ref: dict) -> dict:
    """{"s": (value, name), "rel": (value, name), "cos": (value, name)} over the tensors of ref; every tensor of ref
    must be in grads.  A zero reference tensor is compared exactly and reported under "zero"."""
    out = {"s": (0.0, None), "rel": (0.0, None), "cos": (2.0, None), "zero": []}
    for k, r in ref.items():
        m = metrics(grads[k], r)
        if m is None:
            if torch.count_nonzero(grads[k]) != 0:
                out["zero"].append(k)
            continue
        out["s"] = max(out["s"], (m[0], k))
        out["rel"] = max(out["rel"], (m[1], k))
        out["cos"] = min(out["cos"], (m[2], k))
    return out


def failures(grads: dict, ref: dict, s_bound: float | None = None, rel_bound: float | None = None) -> list:
    """the tensors outside a bound, as (name, |s - 1|, rel, cos)"""
    s_bound = S_BOUND if s_bound is None else s_bound
    rel_bound = REL_BOUND if rel_bound is None else rel_bound
    bad = []
    for k, r in ref.items():
        m = metrics(grads[k], r)
        if m is None:
            if torch.count_nonzero(grads[k]) != 0:
                bad.append((k, float("inf"), float("inf"), 0.0))
        elif not (m[0] <= s_bound and m[1] <= rel_bound):     # a NaN fails
            bad.append((k, *m))
    return bad


def check(grads: dict, ref: dict, label: str) -> dict:
    """print the WORST line of `label`, then assert every tensor within S_BOUND and REL_BOUND of the reference"""
    w = worst(grads, ref)
    print(f"WORST {label}: |s-1| {w['s'][0]:.4f} / {S_BOUND:.3f} ({w['s'][1]})  rel {w['rel'][0]:.4f} / "
          f"{REL_BOUND:.3f} ({w['rel'][1]})  cos {w['cos'][0]:.5f} ({w['cos'][1]})")
    bad = failures(grads, ref)
    assert not bad, f"{label}: {len(bad)} of {len(ref)} gradients outside |s-1| <= {S_BOUND}, rel <= {REL_BOUND}: " \
                    f"{[(k, round(a, 4), round(b, 4), round(c, 5)) for k, a, b, c in bad[:8]]}"
    return w


S_BOUND, REL_BOUND = _bounds()
