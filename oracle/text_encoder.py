"""CPU restatement (fp32 by default; any dtype through `dtype`) of the text encoders the reference caches text states with, taking
transformers state-dict names.  TEST INFRASTRUCTURE ONLY (oracle/__init__.py).

  * CLIP text transformer (transformers CLIPTextModel / CLIPTextModelWithProjection): token +
    position embedding, pre-LN blocks (causal self-attention with biases, quick_gelu / erf-gelu MLP),
    final LayerNorm, pooled = final-normed state at argmax(ids), optional bias-free text projection;
  * T5 encoder (transformers T5EncoderModel, v1.1 gated-GELU FFN): RMS layer norm, unscaled
    attention scores + bucketed relative position bias from block 0, gelu_new(wi_0 x) * wi_1 x.
Selection of the cached tensors follows modules/model/util/clip_util.py:6-43 (encode_clip) and
modules/model/util/t5_util.py (encode_t5), called from StableDiffusionXLModel.py:233-256,
StableDiffusionModel.py:208-217 and FluxModel.py:235-262.

Pinning: transformers is importable here (the reference pins 4.48.3; the CLIP / T5 math is the
same in the installed 5.x) and tests/test_text_encoder.py checks this restatement against
transformers' own modules with random weights -- the reference's actual dependency.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F


def _ln(x, w, b, eps):
    return F.layer_norm(x, (x.shape[-1],), w, b, eps)


def _act(x, kind):
    if kind == "quick_gelu":
        return x * torch.sigmoid(1.702 * x)
    if kind == "gelu":
        return F.gelu(x)
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def causal_mask(T: int, dtype=torch.float32) -> torch.Tensor:
    """additive [q, c] mask: -inf where c > q"""
    return torch.full((T, T), float("-inf"), dtype=dtype).triu(1)


def position_rows(B: int, T: int) -> torch.Tensor:
    """the position-table row of every token, [B, T]: its index inside its own prompt"""
    return (torch.arange(B * T) % T).view(B, T)


def eos_rows(ids: torch.Tensor) -> torch.Tensor:
    """the pooled token of every prompt: the first highest id (CLIP's EOS is the vocabulary's last entry)"""
    return ids.argmax(dim=-1)


def select_hidden(hs: list, default_layer: int, layer_skip: int) -> torch.Tensor:
    return hs[default_layer - layer_skip]


def clip_forward(sd: dict, ids: torch.Tensor, heads: int, act: str, eps: float = 1e-5, dtype=torch.float32):
    """-> (hidden_states list [emb, after layer 1, ..., after layer N] (un-normed), last_hidden_state,
    pooler_output, text_embeds or None).  Weights and every intermediate are held in `dtype`."""
    W = {k: v.to(dtype) for k, v in sd.items()}
    B, T = ids.shape
    x = W["text_model.embeddings.token_embedding.weight"][ids] + \
        W["text_model.embeddings.position_embedding.weight"][position_rows(B, T)]
    D = x.shape[-1]
    dh = D // heads
    mask = causal_mask(T, dtype)
    hs = [x]
    i = 0
    while f"text_model.encoder.layers.{i}.layer_norm1.weight" in W:
        p = f"text_model.encoder.layers.{i}."
        h = _ln(x, W[p + "layer_norm1.weight"], W[p + "layer_norm1.bias"], eps)
        q, k, v = (h @ W[p + f"self_attn.{n}_proj.weight"].t() + W[p + f"self_attn.{n}_proj.bias"] for n in "qkv")
        q, k, v = (t.view(B, T, heads, dh).transpose(1, 2) for t in (q, k, v))
        a = torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5 + mask, dim=-1) @ v
        a = a.transpose(1, 2).reshape(B, T, D)
        x = x + a @ W[p + "self_attn.out_proj.weight"].t() + W[p + "self_attn.out_proj.bias"]
        h = _ln(x, W[p + "layer_norm2.weight"], W[p + "layer_norm2.bias"], eps)
        f = _act(h @ W[p + "mlp.fc1.weight"].t() + W[p + "mlp.fc1.bias"], act)
        x = x + f @ W[p + "mlp.fc2.weight"].t() + W[p + "mlp.fc2.bias"]
        hs.append(x)
        i += 1
    last = _ln(x, W["text_model.final_layer_norm.weight"], W["text_model.final_layer_norm.bias"], eps)
    pooled = last[torch.arange(B), eos_rows(ids)]
    embeds = pooled @ W["text_projection.weight"].t() if "text_projection.weight" in W else None
    return hs, last, pooled, embeds


def encode_clip(sd, ids, heads, act, default_layer=-1, layer_skip=0, add_layer_norm=True, eps=1e-5,
                dtype=torch.float32):
    hs, last, pooled, embeds = clip_forward(sd, ids, heads, act, eps, dtype)
    out = select_hidden(hs, default_layer, layer_skip)
    if add_layer_norm:
        out = _ln(out, sd["text_model.final_layer_norm.weight"].to(dtype), sd["text_model.final_layer_norm.bias"].to(dtype), eps)
    return out, (embeds if embeds is not None else pooled)


def t5_bucket(rel: torch.Tensor, num_buckets=32, max_distance=128) -> torch.Tensor:
    """T5Attention._relative_position_bucket, bidirectional."""
    nb = num_buckets // 2
    ret = (rel > 0).long() * nb
    n = rel.abs()
    max_exact = nb // 2
    large = max_exact + (torch.log(n.float() / max_exact) / math.log(max_distance / max_exact)
                         * (nb - max_exact)).long()
    large = torch.minimum(large, torch.full_like(large, nb - 1))
    return ret + torch.where(n < max_exact, n, large)


def t5_relative_position(T: int) -> torch.Tensor:
    """[q, c]: memory position minus context position"""
    pos = torch.arange(T)
    return pos[None, :] - pos[:, None]


def t5_position_bias(table: torch.Tensor, bucket: torch.Tensor) -> torch.Tensor:
    """relative_attention_bias [buckets, heads] gathered at bucket[q, c] -> [heads, q, c]"""
    return table[bucket].permute(2, 0, 1)


def t5_score_scale(dh: int) -> float:
    """T5 leaves its scores unscaled (the 1 / sqrt(d_kv) lives in the initialisation)"""
    return 1.0


def t5_rms(x, w, eps):
    """T5LayerNorm: no mean subtraction, no bias"""
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def t5_forward(sd: dict, ids: torch.Tensor, heads: int, eps: float = 1e-6, num_buckets=32, max_distance=128,
               dtype=torch.float32):
    """-> hidden_states list as transformers builds it: [emb, after block 0, ..., after block N-2,
    final_layer_norm(after block N-1)].  Weights and every intermediate are held in `dtype`."""
    W = {k: v.to(dtype) for k, v in sd.items()}
    B, T = ids.shape
    x = W["shared.weight"][ids]
    bucket = t5_bucket(t5_relative_position(T), num_buckets, max_distance)
    bias = t5_position_bias(W["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"], bucket)
    hs = [x]
    i = 0
    while f"encoder.block.{i}.layer.0.layer_norm.weight" in W:
        p = f"encoder.block.{i}.layer."
        h = t5_rms(x, W[p + "0.layer_norm.weight"], eps)
        q, k, v = (h @ W[p + f"0.SelfAttention.{n}.weight"].t() for n in "qkv")
        dh = q.shape[-1] // heads
        q, k, v = (t.view(B, T, heads, dh).transpose(1, 2) for t in (q, k, v))
        a = torch.softmax(q @ k.transpose(-1, -2) * t5_score_scale(dh) + bias, dim=-1) @ v
        x = x + a.transpose(1, 2).reshape(B, T, -1) @ W[p + "0.SelfAttention.o.weight"].t()
        h = t5_rms(x, W[p + "1.layer_norm.weight"], eps)
        g = _act(h @ W[p + "1.DenseReluDense.wi_0.weight"].t(), "gelu_new") * (h @ W[p + "1.DenseReluDense.wi_1.weight"].t())
        x = x + g @ W[p + "1.DenseReluDense.wo.weight"].t()
        hs.append(x)
        i += 1
    hs[-1] = t5_rms(x, W["encoder.final_layer_norm.weight"], eps)
    return hs


def encode_t5(sd, ids, heads, default_layer=-1, layer_skip=0, add_layer_norm=True, eps=1e-6, num_buckets=32,
              max_distance=128, dtype=torch.float32):
    """encode_t5 (t5_util.py): hidden_states[default_layer - layer_skip], final-normed when that is not already the
    last entry and add_layer_norm"""
    hs = t5_forward(sd, ids, heads, eps, num_buckets, max_distance, dtype)
    out = select_hidden(hs, default_layer, layer_skip)
    if add_layer_norm and out is not hs[-1]:
        out = t5_rms(out, sd["encoder.final_layer_norm.weight"].to(dtype), eps)
    return out


# ----- configurations and a seeded initialisation (tests/_frozen_parity.py) ----------------------
@dataclass
class CLIPTextConfig:
    """the fields of module/text_encoder.py's CLIPTextConfig, restated so that the oracle needs no HIP library"""
    vocab_size: int = 49408
    hidden_size: int = 768
    intermediate_size: int = 3072
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    max_position_embeddings: int = 77
    hidden_act: str = "quick_gelu"
    layer_norm_eps: float = 1e-5
    projection_dim: int | None = None


def tiny_clip_config(projection: bool = False) -> CLIPTextConfig:
    return CLIPTextConfig(vocab_size=1000, hidden_size=64, intermediate_size=128, num_hidden_layers=3,
                          num_attention_heads=2, hidden_act="gelu" if projection else "quick_gelu",
                          projection_dim=64 if projection else None)


@dataclass
class T5Config:
    vocab_size: int = 32128
    d_model: int = 4096
    d_kv: int = 64
    d_ff: int = 10240
    num_layers: int = 24
    num_heads: int = 64
    relative_attention_num_buckets: int = 32
    relative_attention_max_distance: int = 128
    layer_norm_epsilon: float = 1e-6


def tiny_t5_config() -> T5Config:
    return T5Config(vocab_size=1000, d_model=64, d_kv=8, d_ff=96, num_layers=3, num_heads=8)


def clip_init(c: CLIPTextConfig, seed: int, qk_gain: float = 1.0) -> dict:
    """a seeded fp32 state dict under the transformers names.  Unlike a checkpoint-free default (0.02 normal, unit
    norms, zero biases) every layer moves the residual stream by its own size: projections are normal / sqrt(fan_in),
    norm weights 1 + 0.1 normal, biases 0.1 normal, and q / k projections carry `qk_gain` each, so the pre-softmax
    scores have a standard deviation of about qk_gain ** 2 nats."""
    g = torch.Generator().manual_seed(seed)
    D, F_ = c.hidden_size, c.intermediate_size
    n = (lambda *sh, std=1.0: torch.randn(*sh, generator=g) * std)
    sd = {"text_model.embeddings.token_embedding.weight": n(c.vocab_size, D, std=0.7),
          "text_model.embeddings.position_embedding.weight": n(c.max_position_embeddings, D, std=0.7)}
    for i in range(c.num_hidden_layers):
        p = f"text_model.encoder.layers.{i}."
        for ln in ("layer_norm1", "layer_norm2"):
            sd[p + ln + ".weight"] = 1.0 + n(D, std=0.1)
            sd[p + ln + ".bias"] = n(D, std=0.1)
        for x in "qkv":
            gain = qk_gain if x in "qk" else 1.0
            sd[p + f"self_attn.{x}_proj.weight"] = n(D, D, std=gain * D ** -0.5)
            sd[p + f"self_attn.{x}_proj.bias"] = n(D, std=0.1 * gain)
        sd[p + "self_attn.out_proj.weight"] = n(D, D, std=D ** -0.5)
        sd[p + "self_attn.out_proj.bias"] = n(D, std=0.1)
        sd[p + "mlp.fc1.weight"] = n(F_, D, std=D ** -0.5)
        sd[p + "mlp.fc1.bias"] = n(F_, std=0.1)
        sd[p + "mlp.fc2.weight"] = n(D, F_, std=F_ ** -0.5)
        sd[p + "mlp.fc2.bias"] = n(D, std=0.1)
    sd["text_model.final_layer_norm.weight"] = 1.0 + n(D, std=0.1)
    sd["text_model.final_layer_norm.bias"] = n(D, std=0.1)
    if c.projection_dim:
        sd["text_projection.weight"] = n(c.projection_dim, D, std=D ** -0.5)
    return sd


def t5_init(c: T5Config, seed: int, qk_gain: float = 1.0, bias_std: float = 1.0) -> dict:
    """as clip_init for the T5 encoder: q / k are normal * qk_gain / (sqrt(d_model) d_kv ** 0.25), so the unscaled
    scores have a standard deviation of about qk_gain ** 2 nats, and the relative_attention_bias table is normal *
    bias_std."""
    g = torch.Generator().manual_seed(seed)
    D, I = c.d_model, c.num_heads * c.d_kv
    n = (lambda *sh, std=1.0: torch.randn(*sh, generator=g) * std)
    sd = {"shared.weight": n(c.vocab_size, D)}
    for i in range(c.num_layers):
        p = f"encoder.block.{i}.layer."
        sd[p + "0.layer_norm.weight"] = 1.0 + n(D, std=0.1)
        for x in "qk":
            sd[p + f"0.SelfAttention.{x}.weight"] = n(I, D, std=qk_gain * D ** -0.5 * c.d_kv ** -0.25)
        sd[p + "0.SelfAttention.v.weight"] = n(I, D, std=D ** -0.5)
        sd[p + "0.SelfAttention.o.weight"] = n(D, I, std=I ** -0.5)
        if i == 0:
            sd[p + "0.SelfAttention.relative_attention_bias.weight"] = n(c.relative_attention_num_buckets, c.num_heads,
                                                                        std=bias_std)
        sd[p + "1.layer_norm.weight"] = 1.0 + n(D, std=0.1)
        sd[p + "1.DenseReluDense.wi_0.weight"] = n(c.d_ff, D, std=D ** -0.5)
        sd[p + "1.DenseReluDense.wi_1.weight"] = n(c.d_ff, D, std=D ** -0.5)
        sd[p + "1.DenseReluDense.wo.weight"] = n(D, c.d_ff, std=c.d_ff ** -0.5)
    sd["encoder.final_layer_norm.weight"] = 1.0 + n(D, std=0.1)
    return sd
