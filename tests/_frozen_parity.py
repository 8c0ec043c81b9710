"""Frozen-network parity: per-row relative error and per-tensor scale of the text encoders and the VAE against a
float64 oracle.

Plain PyTorch on the CPU (as _grad_parity.py): the case table, the oracles in any dtype, the metric and its bounds.
test_frozen_parity_ref.py holds the constants to what this file recomputes and plants the glue errors;
test_frozen_parity_gpu.py and the tiny-config cases of test_text_encoder_gpu.py / test_vae_gpu.py /
test_vae_decoder_gpu.py apply the bounds to the HIP networks.

Metric    a row is one token of [B T, D] or one pixel of [B H W, C]; g under test, r the float64 oracle:
            rel_row = ||g - r|| / max(||r||, 1/4 rms row norm of r)      every row <= REL_BOUND
            s       = <g, r> / <r, r> per tensor                          |s - 1| <= S_BOUND
            cos     per tensor, printed
          A max-norm over the whole tensor is set by its few largest channels or by the image interior; a row norm
          puts every token and every pixel on its own scale.  The floor keeps a latent pixel that happens to lie near
          zero from deciding the result; it may engage on at most FLOOR_SHARE = 5 % of a case's rows
          (test_row_floor_share, on the float64 reference alone).  The worst row is reported with its (batch,
          position) or (batch, y, x); the VAE's border rows (first and last row and column) apart from its interior.

Oracle    oracle/text_encoder.py and oracle/vae.py with dtype=float64.  Weights are the oracle's own seeded
          initialisation (clip_init / t5_init, the nn.Module defaults for the VAE with the norm affines perturbed),
          rounded to bf16, so the oracle, the bf16 run and the HIP model (load_state_dict) hold the same numbers.
          Images are multiples of 1/256, so 2 x - 1 is exact in bf16; decoder latents are chosen so that latent /
          scaling_factor (+ shift_factor) rounds to the same bf16 value in fp32 and in float64.

Cases     B = 3, T = 77.  clip_l_tiny / clip_g_tiny / t5_tiny are module/text_encoder.py's tiny configs; clip_h64
          (hidden 128, 2 heads, erf-gelu, projection) and t5_h64 (d_kv 64, 8 heads) have the real 64-wide heads.
          t5_h64 has relative_attention_max_distance 64: with the default 128 and T = 77 no distance reaches the last
          bucket (it starts at |q - c| = 91), so the clamp of the far buckets would never engage; with 64 it engages
          from |q - c| = 50.  sdxl / sd15 / flux are the encode_*_text dictionaries over the tiny encoders.
          enc_* / dec_* are tiny_vae_config with 4 latent channels + quant_conv and with 16 without, and a
          three-level (64, 96, 160) config; encoder images 10 x 14 and 16 x 24 (latents 5 x 7: odd, 35 mid-attention
          tokens; and 8 x 12: no multiple of any tile), the three-level one 20 x 28; decoder latents 5 x 7 and 8 x 8.

Hard      chosen here.  The q / k projections carry QK_GAIN each, so pre-softmax scores have a standard deviation of
inputs    about QK_GAIN ** 2 nats and spread over several; T5's relative_attention_bias table is normal * BIAS_STD,
          the same order, so a mask, bucket or bias mistake moves the softmax.  Every layer moves the residual stream
          by about its own size (oracle clip_init), so hidden_states[-2] is not hidden_states[-1].
          CLIP token rows (BOS 998, EOS 999 = the largest id):
            0  the empty prompt, bigG style: BOS, EOS at position 1, padded with 0
            1  a full prompt: EOS at position 76
            2  CLIP-L style: EOS at position 31, padded with the EOS id itself (argmax must take the first)
          T5 token rows: EOS id 1 at the end of 3, 33 and 77 tokens, then pad 0.  T5 has no mask here, so every row
          attends over all 77 positions and |q - c| runs from 0 to 76 in both directions: both sides of every bucket
          boundary (1 .. 8 exact, then 12, 16, 23, 32, 46, 64 with max_distance 128; 11, 14, 18, 23, 30, 39, 50 with 64).

Bounds    measured against the reference, never against the GPU.  k_rel is the worst rel_row and k_s the worst |s - 1|
          of the bf16 CPU oracle (weights and activations bf16, rounded after every op) against float64, per case
          (K_MEASURED, with the output and row that showed it).  Each k is taken up at its second significant digit
          (_grad_parity.ceil2) and REL_BOUND = 4 k_rel, S_BOUND = 4 k_s, the project's factor: the HIP networks keep
          fp32 accumulators but store bf16 activations and use hardware exp2 and rcp.  One pair per family (text,
          VAE), the larger over its cases; neither may exceed CAP = 0.25.
            text  k_rel 0.0331 (clip_g_tiny hidden_states[3], row (1, 10))   -> 0.034, REL_BOUND 0.136
                  k_s   0.00141 (sdxl text_encoder_2_pooled_state: 3 rows) -> 0.0015, S_BOUND 0.006
            VAE   k_rel 0.0344 (dec_three rgb@5x7, pixel (0, 10, 8)) -> 0.035, REL_BOUND 0.14
                  k_s   0.00028 (enc_tiny16 mean@5x7)                -> 0.00028, S_BOUND 0.00112

Changed   inputs that were changed to meet a rule above, never a bound:
inputs      * VAE outputs: with zero-centred outputs the three-channel RGB rows of the decoders sat under the floor on
              up to 8 % of a case's rows and 4 k_rel was 0.46 to 0.71.  The last convolution's bias is now +-OUT_BIAS
              (0.5 for the latent mean, 1.0 for RGB, alternating sign, growing by a quarter over the channels), the
              size of the outputs' own variation, as a decoded image has; the floor then engages on no row.
            * the three-level VAE's weight seed: seeds 8 to 12 gave the decoder k_rel 0.070, 0.025, 0.034, 0.044,
              0.027 (bf16 noise of a deep network has a heavy tail); 8 left 4 k over the cap, 10 is kept.
            * CLIP MLPs: with clip_init alone erf-gelu against quick_gelu moved no row by more than 0.4 x REL_BOUND.
              Every other MLP unit now has fc1 bias TAIL_BIAS = -2.5 and its fc2 column times TAIL_GAIN = 16, so the
              stream carries a component from the activation's negative tail, where the two kinds differ by tens of
              percent (quick_gelu(-2.5) = -0.035, gelu(-2.5) = -0.0155).
            * gelu_new against erf-gelu differs by at most 4.7e-4 absolute, under any bf16 noise, but by 30 % of the
              value at -3.6 (gelu -5.7e-4, gelu_new -4.0e-4).  Of the other MLP units every second one (index 1 :: 4)
              has fc1 bias DEEP_BIAS = -3.6, its fc1 row times DEEP_SPREAD = 0.25 (pre-activations stay within about
              -3.6 +- 0.3) and its fc2 column times DEEP_GAIN = 1000, so these units add a nearly token-independent
              vector of a fifth to a third of the row norm.  A wrong kind changes that vector's length coherently, which
              the per-tensor scale sees: |s - 1| 0.033 on clip_g_tiny hidden_states[3], 5.5 x S_BOUND (rel_row 0.17).
              T5 has no biases, so its gated units cannot be put there; the plant is caught in the erf-gelu CLIP cases.
"""
from __future__ import annotations

import contextlib
import functools
import math

import torch
import torch.nn.functional as F

from _grad_parity import bf, ceil2
from oracle import text_encoder as OT
from oracle import vae as OV

CAP = 0.25
FLOOR_SHARE = 0.05
B, T = 3, 77
QK_GAIN, BIAS_STD = 1.5, 2.0
TAIL_BIAS, TAIL_GAIN = -2.5, 16.0
DEEP_BIAS, DEEP_GAIN, DEEP_SPREAD = -3.6, 1000.0, 0.25
OUT_BIAS = {"enc": 0.5, "dec": 1.0}
VOCAB, BOS, EOS_CLIP, EOS_T5 = 1000, 998, 999, 1

CLIP_CFGS = {
    "clip_l_tiny": OT.tiny_clip_config(False),
    "clip_g_tiny": OT.tiny_clip_config(True),
    "clip_h64": OT.CLIPTextConfig(vocab_size=VOCAB, hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                                  num_attention_heads=2, hidden_act="gelu", projection_dim=128),
}
T5_CFGS = {
    "t5_tiny": OT.tiny_t5_config(),
    "t5_h64": OT.T5Config(vocab_size=VOCAB, d_model=64, d_kv=64, d_ff=96, num_layers=2, num_heads=8,
                          relative_attention_max_distance=64),
}
VAE_CFGS = {
    "tiny4": OV.tiny_vae_config(),
    "tiny16": OV.tiny_vae_config(16, False),
    "three": OV.VAEConfig(block_out_channels=(64, 96, 160), layers_per_block=1),
}
ENC_IMAGES = {"tiny4": ((10, 14), (16, 24)), "tiny16": ((10, 14), (16, 24)), "three": ((20, 28),)}
DEC_LATENTS = ((5, 7), (8, 8))
FAMILY_CASES = {"sdxl": ("clip_l_tiny", "clip_g_tiny"), "sd15": ("clip_l_tiny",), "flux": ("clip_l_tiny", "t5_tiny")}
SEEDS = {"clip_l_tiny": 1, "clip_g_tiny": 2, "clip_h64": 3, "t5_tiny": 4, "t5_h64": 5, "tiny4": 6, "tiny16": 7,
         "three": 10}
ENCODE_SELECTIONS = ((-2, 0, False), (-1, 0, True), (-1, 1, True))     # SDXL; SD 1.5; clip skip 1

TEXT_CASES = tuple(CLIP_CFGS) + tuple(T5_CFGS) + tuple(FAMILY_CASES)
VAE_CASES = tuple(f"enc_{k}" for k in VAE_CFGS) + tuple(f"dec_{k}" for k in VAE_CFGS)
CASES = TEXT_CASES + VAE_CASES

# per case: (k, output, row or None) of the bf16 CPU oracle against the float64 oracle (test_bounds_measured)
K_MEASURED = {
    "clip_l_tiny": {"k_rel": (0.0153, "last_hidden_state", (0, 29)), "k_s": (0.00097, "hidden_states[3]")},
    "clip_g_tiny": {"k_rel": (0.0331, "hidden_states[3]", (1, 10)), "k_s": (0.00058, "hidden_states[3]")},
    "clip_h64": {"k_rel": (0.0189, "last_hidden_state", (2, 42)), "k_s": (0.00030, "pooled")},
    "t5_tiny": {"k_rel": (0.0295, "encode(skip 1)", (1, 8)), "k_s": (0.00063, "hidden_states[2]")},
    "t5_h64": {"k_rel": (0.0222, "hidden_states[2]", (2, 25)), "k_s": (0.00044, "hidden_states[1]")},
    "sdxl": {"k_rel": (0.0300, "text_encoder_2_hidden_state", (1, 69)), "k_s": (0.00141, "text_encoder_2_pooled_state")},
    "sd15": {"k_rel": (0.0153, "text_encoder_hidden_state", (0, 29)), "k_s": (0.00003, "text_encoder_hidden_state")},
    "flux": {"k_rel": (0.0270, "text_encoder_2_hidden_state", (1, 8)), "k_s": (0.00047, "text_encoder_2_hidden_state")},
    "enc_tiny4": {"k_rel": (0.0108, "mean@8x12", (2, 2, 7)), "k_s": (0.00026, "mean@5x7")},
    "enc_tiny16": {"k_rel": (0.0160, "mean@8x12", (1, 4, 7)), "k_s": (0.00028, "mean@5x7")},
    "enc_three": {"k_rel": (0.0087, "mean@5x7", (1, 3, 1)), "k_s": (0.00007, "mean@5x7")},
    "dec_tiny4": {"k_rel": (0.0178, "rgb@8x8", (1, 5, 11)), "k_s": (0.00019, "rgb@5x7")},
    "dec_tiny16": {"k_rel": (0.0141, "rgb@5x7", (1, 4, 8)), "k_s": (0.00021, "rgb@5x7")},
    "dec_three": {"k_rel": (0.0344, "rgb@5x7", (0, 10, 8)), "k_s": (0.00008, "rgb@5x7")},
}


def family(case: str) -> str:
    return "vae" if case in VAE_CASES else "text"


def _bounds(fam: str):
    rows = [v for c, v in K_MEASURED.items() if family(c) == fam]
    ks = max((v["k_s"][0] for v in rows), default=0.0)
    kr = max((v["k_rel"][0] for v in rows), default=0.0)
    return 4 * ceil2(ks), 4 * ceil2(kr)


# ----- inputs ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clip_ids(seed: int = 0) -> torch.Tensor:
    g = torch.Generator().manual_seed(100 + seed)
    ids = torch.randint(1, BOS, (B, T), generator=g)
    ids[:, 0] = BOS
    ids[0, 1], ids[0, 2:] = EOS_CLIP, 0
    ids[1, T - 1] = EOS_CLIP
    ids[2, 31:] = EOS_CLIP
    return ids


@functools.lru_cache(maxsize=None)
def t5_ids(seed: int = 0) -> torch.Tensor:
    g = torch.Generator().manual_seed(200 + seed)
    ids = torch.randint(2, VOCAB, (B, T), generator=g)
    for b, n in enumerate((3, 33, 77)):
        ids[b, n - 1] = EOS_T5
        ids[b, n:] = 0
    return ids


@functools.lru_cache(maxsize=None)
def text_weights(name: str) -> dict:
    if name in CLIP_CFGS:
        sd = OT.clip_init(CLIP_CFGS[name], SEEDS[name], QK_GAIN)
        for k in sd:     # every other MLP unit works in the activation's negative tail: the docstring
            if k.endswith("mlp.fc1.bias"):
                sd[k][::2] = TAIL_BIAS
            if k.endswith("mlp.fc2.weight"):
                sd[k][:, ::2] *= TAIL_GAIN
                sd[k][:, 1::4] *= DEEP_GAIN
            if k.endswith("mlp.fc1.bias"):
                sd[k][1::4] = DEEP_BIAS
            if k.endswith("mlp.fc1.weight"):
                sd[k][1::4] *= DEEP_SPREAD
    else:
        sd = OT.t5_init(T5_CFGS[name], SEEDS[name], QK_GAIN, BIAS_STD)
    return {k: bf(v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def vae_weights(name: str, half: str) -> dict:
    """the nn.Module default initialisation under a seed, every GroupNorm affine perturbed (weight 1 + 0.1 normal,
    bias 0.1 normal: a dropped or misplaced affine must show), rounded to bf16"""
    torch.manual_seed(SEEDS[name] + (0 if half == "enc" else 50))
    om = (OV.AutoencoderKLEncoder if half == "enc" else OV.AutoencoderKLDecoder)(VAE_CFGS[name])
    g = torch.Generator().manual_seed(SEEDS[name] + 300)
    sd = {}
    for k, v in om.state_dict().items():
        if "norm" in k:
            v = (1.0 if k.endswith(".weight") else 0.0) + 0.1 * torch.randn(v.shape, generator=g)
        sd[k] = bf(v.detach())
    last = ("quant_conv" if VAE_CFGS[name].use_quant_conv else "encoder.conv_out") if half == "enc" else "decoder.conv_out"
    n = sd[last + ".bias"].numel()
    sd[last + ".bias"] = bf(OUT_BIAS[half] * (1.0 + 0.25 * torch.arange(n) / n) * (-1.0) ** torch.arange(n))
    return sd


@functools.lru_cache(maxsize=None)
def image(h: int, w: int) -> torch.Tensor:
    """[B, 3, h, w] in [0, 1], multiples of 1/256: a low-frequency pattern per channel plus noise"""
    g = torch.Generator().manual_seed(400 + h)
    y, x = torch.meshgrid(torch.arange(h) / h, torch.arange(w) / w, indexing="ij")
    ph = torch.rand(B, 3, 1, 1, generator=g) * 6.28
    img = 0.5 + 0.3 * torch.sin(6.28 * (x + 0.7 * y) + ph) + 0.35 * (torch.rand(B, 3, h, w, generator=g) - 0.5)
    return (img.clamp(0, 1) * 256).round().clamp(0, 255) / 256


@functools.lru_cache(maxsize=None)
def latent(name: str, h: int, w: int) -> torch.Tensor:
    """[B, h, w, L] NHWC fp32, scaled as the UNet sees it: z * scaling_factor for a bf16 z of unit size (minus the
    shift), kept only where fp32 and float64 arithmetic agree on bf16(latent / scaling_factor + shift)"""
    cfg = VAE_CFGS[name]
    g = torch.Generator().manual_seed(500 + h)
    z = bf(torch.randn(B, h, w, cfg.latent_channels, generator=g) * 1.5)
    lat = ((z - cfg.shift_factor) * cfg.scaling_factor).float()
    back32 = bf(lat / cfg.scaling_factor + cfg.shift_factor)
    back64 = (lat.double() / cfg.scaling_factor + cfg.shift_factor).to(torch.bfloat16).float()
    assert torch.equal(back32, back64), "the latent does not round alike in fp32 and float64: choose another seed"
    return lat


# ----- the oracle in any dtype: {output name: tensor [B, ..., C]} ----------------------------------------------------
def _clip_outputs(name: str, dtype) -> dict:
    c, sd, ids = CLIP_CFGS[name], text_weights(name), clip_ids()
    hs, last, pooled, embeds = OT.clip_forward(sd, ids, c.num_attention_heads, c.hidden_act, c.layer_norm_eps, dtype)
    out = {f"hidden_states[{i}]": h for i, h in enumerate(hs)}
    out["last_hidden_state"] = last
    out["pooled"] = embeds if embeds is not None else pooled
    for dl, skip, ln in ENCODE_SELECTIONS:
        out[f"encode({dl},{skip},{ln})"] = OT.encode_clip(sd, ids, c.num_attention_heads, c.hidden_act, dl, skip, ln,
                                                          c.layer_norm_eps, dtype)[0]
    return out


def _t5_kw(c) -> dict:
    return dict(eps=c.layer_norm_epsilon, num_buckets=c.relative_attention_num_buckets,
                max_distance=c.relative_attention_max_distance)


def _t5_outputs(name: str, dtype) -> dict:
    c, sd, ids = T5_CFGS[name], text_weights(name), t5_ids()
    hs = OT.t5_forward(sd, ids, c.num_heads, dtype=dtype, **_t5_kw(c))
    out = {f"hidden_states[{i}]": h for i, h in enumerate(hs)}
    out["encode"] = OT.encode_t5(sd, ids, c.num_heads, dtype=dtype, **_t5_kw(c))
    out["encode(skip 1)"] = OT.encode_t5(sd, ids, c.num_heads, layer_skip=1, dtype=dtype, **_t5_kw(c))
    return out


def _family_outputs(name: str, dtype) -> dict:
    """StableDiffusionXLModel / StableDiffusionModel / FluxModel .encode_text over the tiny encoders"""
    l, g, t = CLIP_CFGS["clip_l_tiny"], CLIP_CFGS["clip_g_tiny"], T5_CFGS["t5_tiny"]
    enc = (lambda n, c, ids, dl, ln: OT.encode_clip(text_weights(n), ids, c.num_attention_heads, c.hidden_act, dl, 0,
                                                    ln, c.layer_norm_eps, dtype))
    if name == "sdxl":
        h1, _ = enc("clip_l_tiny", l, clip_ids(), -2, False)
        h2, pooled = enc("clip_g_tiny", g, clip_ids(1), -2, False)
        return {"text_encoder_1_hidden_state": h1, "text_encoder_2_hidden_state": h2,
                "text_encoder_2_pooled_state": pooled}
    if name == "sd15":
        return {"text_encoder_hidden_state": enc("clip_l_tiny", l, clip_ids(), -1, True)[0]}
    _, pooled = enc("clip_l_tiny", l, clip_ids(), -1, True)
    h2 = OT.encode_t5(text_weights("t5_tiny"), t5_ids(), t.num_heads, dtype=dtype, **_t5_kw(t))
    return {"text_encoder_1_pooled_state": pooled, "text_encoder_2_hidden_state": h2}


def _vae_outputs(case: str, dtype) -> dict:
    half, name = case.split("_")
    cfg = VAE_CFGS[name]
    out = {}
    with torch.no_grad():
        if half == "enc":
            om = OV.AutoencoderKLEncoder(cfg, dtype)
            om.load_state_dict(vae_weights(name, "enc"))
            for h, w in ENC_IMAGES[name]:
                f = 1 << (len(cfg.block_out_channels) - 1)
                out[f"mean@{h // f}x{w // f}"] = om(image(h, w)).permute(0, 2, 3, 1)
        else:
            om = OV.AutoencoderKLDecoder(cfg, dtype)
            om.load_state_dict(vae_weights(name, "dec"))
            for h, w in DEC_LATENTS:
                lat = latent(name, h, w).permute(0, 3, 1, 2)
                out[f"rgb@{h}x{w}"] = om.decode(lat.double() if dtype == torch.float64 else lat).permute(0, 2, 3, 1)
    return out


def outputs(case: str, dtype) -> dict:
    """every checked output of one case from the oracle in `dtype`, as float64 copies"""
    with torch.no_grad():
        if case in CLIP_CFGS:
            out = _clip_outputs(case, dtype)
        elif case in T5_CFGS:
            out = _t5_outputs(case, dtype)
        elif case in FAMILY_CASES:
            out = _family_outputs(case, dtype)
        else:
            out = _vae_outputs(case, dtype)
    return {k: v.detach().double().contiguous() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def reference(case: str) -> dict:
    """the float64 table of one case, computed once and shared; treat as read-only"""
    return outputs(case, torch.float64)


@functools.lru_cache(maxsize=None)
def bf16_oracle(case: str) -> dict:
    """the bf16 CPU oracle's outputs: the noise level the bounds come from"""
    return outputs(case, torch.bfloat16)


# ----- metric ------------------------------------------------------------------------------------------------------
def row_metrics(g: torch.Tensor, r: torch.Tensor) -> dict:
    """g, r: [..., C] of the same shape -> rel_row per row [...], its worst with the index, the share of rows under
    the floor, |s - 1| and the cosine of the whole tensor; for [B, H, W, C] also the worst border and interior row"""
    g, r = g.detach().double().cpu(), r.detach().double().cpu()
    if g.shape != r.shape:
        raise ValueError(f"output of shape {tuple(g.shape)} against a reference of {tuple(r.shape)}")
    lead = r.shape[:-1]
    g2, r2 = g.reshape(-1, r.shape[-1]), r.reshape(-1, r.shape[-1])
    rn = r2.norm(dim=1)
    floor = 0.25 * math.sqrt(float((rn * rn).mean()))
    if floor == 0.0:
        raise ValueError("the reference is identically zero")
    rel = ((g2 - r2).norm(dim=1) / rn.clamp_min(floor)).reshape(lead)
    rel = torch.where(torch.isnan(rel), torch.full_like(rel, float("inf")), rel)       # a NaN fails
    rr, gr = float((r2 * r2).sum()), float((g2 * r2).sum())
    s_err = abs(gr / rr - 1.0)
    m = {"rel": rel, "floored": int((rn < floor).sum()), "rows": rn.numel(),
         "s": s_err if s_err == s_err else float("inf"), "cos": gr / (math.sqrt(rr) * float(g2.norm()) + 1e-300)}
    i = int(rel.argmax())
    m["worst"] = (float(rel.flatten()[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), lead)))
    if len(lead) == 3:
        border = torch.zeros(lead, dtype=torch.bool)
        border[:, 0], border[:, -1], border[:, :, 0], border[:, :, -1] = True, True, True, True
        for key, sel in (("border", border), ("interior", ~border)):
            v = torch.where(sel, rel, torch.full_like(rel, -1.0))
            j = int(v.argmax())
            m[key] = (float(v.flatten()[j]), tuple(int(x) for x in torch.unravel_index(torch.tensor(j), lead)))
    return m


def worst(got: dict, ref: dict) -> dict:
    """{"rel": (value, output, row), "s": (value, output), "cos": (value, output), "floored", "rows"} over the
    outputs of ref; every output of ref must be in got"""
    out = {"rel": (0.0, None, None), "s": (0.0, None), "cos": (2.0, None), "floored": 0, "rows": 0, "per": {}}
    for k, r in ref.items():
        m = row_metrics(got[k], r)
        out["per"][k] = m
        if out["rel"][1] is None or m["worst"][0] > out["rel"][0]:
            out["rel"] = (m["worst"][0], k, m["worst"][1])
        if out["s"][1] is None or m["s"] > out["s"][0]:
            out["s"] = (m["s"], k)
        if m["cos"] < out["cos"][0]:
            out["cos"] = (m["cos"], k)
        out["floored"] += m["floored"]
        out["rows"] += m["rows"]
    return out


def failures(got: dict, ref: dict, fam: str, factor: float = 1.0) -> list:
    """the outputs outside factor x a bound, as (output, worst rel_row, row, |s - 1|)"""
    s_bound, rel_bound = BOUNDS[fam]
    bad = []
    for k, r in ref.items():
        m = row_metrics(got[k], r)
        if not (m["worst"][0] <= factor * rel_bound and m["s"] <= factor * s_bound):
            bad.append((k, m["worst"][0], m["worst"][1], m["s"]))
    return bad


def check(got: dict, ref: dict, label: str, fam: str) -> dict:
    """print the WORST lines of `label`, then assert every row within REL_BOUND and every tensor within S_BOUND"""
    s_bound, rel_bound = BOUNDS[fam]
    w = worst(got, ref)
    print(f"WORST {label}: rel_row {w['rel'][0]:.4f} / {rel_bound:.3f} ({w['rel'][1]} at {w['rel'][2]})  |s-1| "
          f"{w['s'][0]:.5f} / {s_bound:.4f} ({w['s'][1]})  cos {w['cos'][0]:.6f} ({w['cos'][1]})")
    for k, m in w["per"].items():
        if "border" in m:
            print(f"      {label} {k}: border {m['border'][0]:.4f} at {m['border'][1]}  interior "
                  f"{m['interior'][0]:.4f} at {m['interior'][1]}")
    bad = failures(got, ref, fam)
    assert not bad, f"{label}: {len(bad)} of {len(ref)} outputs outside rel_row <= {rel_bound}, |s-1| <= {s_bound}: " \
                    f"{[(k, round(a, 4), i, round(s, 5)) for k, a, i, s in bad[:8]]}"
    return w


# ----- planted errors: the float64 oracle with one piece of glue wrong ----------------------------------------------
def _swap_act(pairs: dict):
    real = OT._act
    return lambda x, kind: real(x, pairs.get(kind, kind))


def _mask_diagonal_too(T_, dtype=torch.float32):
    """c >= q masked; row 0 keeps its only column, or it would have none"""
    m = torch.full((T_, T_), float("-inf"), dtype=dtype).triu(0)
    m[0, 0] = 0.0
    return m


def _mask_one_ahead(T_, dtype=torch.float32):
    return torch.full((T_, T_), float("-inf"), dtype=dtype).triu(2)


_REL_POSITION = OT.t5_relative_position


def _pos_rows_wrong(B_, T_):
    return (torch.arange(B_ * T_) % (T_ + 1)).clamp(max=T_ - 1).view(B_, T_)


def _bucket_far_low(rel, num_buckets=32, max_distance=128):
    """t5_bucket with the far buckets clamped at nb - 2"""
    nb = num_buckets // 2
    ret = (rel > 0).long() * nb
    n = rel.abs()
    max_exact = nb // 2
    large = max_exact + (torch.log(n.float() / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)).long()
    large = torch.minimum(large, torch.full_like(large, nb - 2))
    return ret + torch.where(n < max_exact, n, large)


def _rms_centred(x, w, eps):
    x = x - x.mean(-1, keepdim=True)
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def _encode_clip_always_normed(real):
    def f(sd, ids, heads, act, default_layer=-1, layer_skip=0, add_layer_norm=True, eps=1e-5, dtype=torch.float32):
        return real(sd, ids, heads, act, default_layer, layer_skip, True, eps, dtype)
    return f


def _upsample_shifted(x):
    up = F.interpolate(x, scale_factor=2.0, mode="nearest")
    return F.pad(up, (0, 1, 0, 1), mode="replicate")[..., 1:, 1:]


def _bias_ch_swapped(table, bucket):
    """bias[q, c, h] read as if its last two strides were (1, T): element (q, h, c) of the [T, T, H] block"""
    Tq, Tc = bucket.shape
    flat = table[bucket].reshape(Tq, Tc * table.shape[1])                        # [q, c * H + h]
    c, h = torch.arange(Tc)[:, None], torch.arange(table.shape[1])[None, :]
    return flat[:, (c + h * Tc)].permute(2, 0, 1)                               # [q, c, h] <- offset c + h * T


_CLIP, _T5, _ALLCLIP = tuple(CLIP_CFGS), tuple(T5_CFGS), tuple(CLIP_CFGS) + tuple(FAMILY_CASES)
_ENC, _DEC = tuple(f"enc_{k}" for k in VAE_CFGS), tuple(f"dec_{k}" for k in VAE_CFGS)
_QUANT = tuple(k for k, c in VAE_CFGS.items() if c.use_quant_conv)

# name -> (the cases it is planted in, [(module or class, attribute, wrong replacement), ...])
PLANTED = {
    "erf-gelu <-> quick_gelu": (_ALLCLIP, [(OT, "_act", _swap_act({"gelu": "quick_gelu", "quick_gelu": "gelu"}))]),
    "gelu_new <-> erf-gelu": (_T5 + ("clip_g_tiny", "clip_h64", "flux"),
                              [(OT, "_act", _swap_act({"gelu": "gelu_new", "gelu_new": "gelu"}))]),
    "causal mask: c >= q masked": (_ALLCLIP, [(OT, "causal_mask", _mask_diagonal_too)]),
    "causal mask: c > q + 1 allowed": (_ALLCLIP, [(OT, "causal_mask", _mask_one_ahead)]),
    "pooled row at EOS + 1": (_ALLCLIP, [(OT, "eos_rows", lambda ids: (ids.argmax(-1) + 1).clamp(max=ids.shape[1] - 1))]),
    "pooled row at the last position": (_ALLCLIP, [(OT, "eos_rows", lambda ids: torch.full((ids.shape[0],), ids.shape[1] - 1))]),
    "position index r % (T + 1)": (_ALLCLIP, [(OT, "position_rows", _pos_rows_wrong)]),
    "hidden-state index off by one in encode": (_ALLCLIP + _T5, [(OT, "select_hidden", lambda hs, dl, skip: hs[dl - skip - 1])]),
    "final LayerNorm applied when add_layer_norm=False": (_ALLCLIP, [(OT, "encode_clip", _encode_clip_always_normed(OT.encode_clip))]),
    "T5 rel = ctx - mem": (_T5 + ("flux",), [(OT, "t5_relative_position", lambda T_: -_REL_POSITION(T_))]),
    "T5 far buckets clamped one too low": (("t5_h64",), [(OT, "t5_bucket", _bucket_far_low)]),
    "T5 bias read with q and c swapped": (_T5 + ("flux",), [(OT, "t5_position_bias", lambda t, b: t[b].permute(2, 1, 0))]),
    "T5 bias read with c and h swapped": (_T5 + ("flux",), [(OT, "t5_position_bias", _bias_ch_swapped)]),
    "T5 scores scaled by d_kv ** -0.5": (_T5 + ("flux",), [(OT, "t5_score_scale", lambda dh: dh ** -0.5)]),
    "RMSNorm with mean subtraction": (_T5 + ("flux",), [(OT, "t5_rms", _rms_centred)]),
    "VAE down-sample padded (1, 0, 1, 0)": (_ENC, [(OV.Downsample2D, "PAD", (1, 0, 1, 0))]),
    "logvar rows returned instead of the mean": (_ENC, [(OV.AutoencoderKLEncoder, "mean", lambda self, m: m[:, self.cfg.latent_channels:])]),
    "quant_conv skipped": (tuple(f"enc_{k}" for k in _QUANT), [(OV.AutoencoderKLEncoder, "moments", lambda self, x: self.encoder(x.to(self.dtype)))]),
    "GroupNorm with SiLU dropped at conv_norm_out": (_ENC + _DEC, [(OV, "norm_out", lambda norm, x: norm(x))]),
    "decoder nearest up-sample shifted by one pixel": (_DEC, [(OV, "upsample_nearest", _upsample_shifted)]),
    "post_quant_conv skipped": (tuple(f"dec_{k}" for k in _QUANT), [(OV.AutoencoderKLDecoder, "forward", lambda self, z: self.decoder(z.to(self.dtype)))]),
    "latent not divided by scaling_factor": (_DEC, [(OV.AutoencoderKLDecoder, "unscale", lambda self, lat: lat + self.cfg.shift_factor)]),
}


@contextlib.contextmanager
def planted(name: str):
    """the oracle with the named error, for the duration of the block"""
    patches = PLANTED[name][1]
    saved = [(o, a, getattr(o, a)) for o, a, _ in patches]
    try:
        for o, a, v in patches:
            setattr(o, a, v)
        yield
    finally:
        for o, a, v in saved:
            setattr(o, a, v)


BOUNDS = {fam: _bounds(fam) for fam in ("text", "vae")}      # family -> (S_BOUND, REL_BOUND)
