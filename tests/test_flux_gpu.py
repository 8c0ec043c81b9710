"""FLUX.1: HIP kernels vs plain PyTorch fp32 references, and the
HIP FluxTransformer2DModel (bf16, rows t*B + b) vs the oracle restatement (fp32 CPU) -- forward, every
parameter / LoRA-adapter gradient, and the LoRA train step.  Tolerances: bf16 activations with fp32
accumulation vs fp32: forward rel err < 3e-2, gradient cosine >= 0.99 (parity unpinned: diffusers absent); every
gradient also against the float64 oracle per tensor: scale and relative L2 error (_grad_parity.py)."""
import copy

import pytest
import torch
import torch.nn.functional as F

from onetrainer_amd import kernels as K
from onetrainer_amd.module import flux as FX
from oracle import flux as OF
from oracle.lora import OracleLoRA

import _grad_parity as G

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-6)).item()


def _cos(a, b):
    a, b = a.flatten().double().cpu(), b.flatten().double().cpu()
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


def test_adaln_gated(dev):
    torch.manual_seed(0)
    T, B, D = 37, 3, 256
    x = torch.randn(T * B, D, device=dev).bfloat16()
    emb = (torch.randn(B, 3 * D, device=dev) * 0.5).bfloat16()
    y, st = K.adaln_fwd(x, emb, 0, D, B)
    xr = x.float().view(T, B, D).requires_grad_(True)
    er = emb.float().requires_grad_(True)
    ref = F.layer_norm(xr, (D,), eps=1e-6) * (1 + er[None, :, D:2 * D]) + er[None, :, :D]
    assert rel(y, ref.reshape(T * B, D)) < 1e-2
    dy = torch.randn(T * B, D, device=dev).bfloat16()
    ref.backward(dy.float().view(T, B, D))
    dmod = torch.zeros_like(emb)
    dx = K.adaln_bwd(x, dy, emb, 0, D, B, st, dmod=dmod)
    assert rel(dx, xr.grad.reshape(T * B, D)) < 2e-2
    assert rel(dmod[:, :2 * D], er.grad[:, :2 * D]) < 2e-2
    # the residual gradient summed in the dx pass (otamd_adaln_bwd_res): rounded once, within one bf16 rounding of
    # the separate add; the modulation gradients unchanged
    dres = torch.randn(T * B, D, device=dev).bfloat16()
    dmod2 = torch.zeros_like(emb)
    dx2 = K.adaln_bwd(x, dy, emb, 0, D, B, st, dmod=dmod2, dres=dres)
    ref2 = xr.grad.reshape(T * B, D) + dres.float()
    assert rel(dx2, ref2) < 2e-2
    assert (dx2.float() - (dx.float() + dres.float())).abs().max().item() <= 2 ** -7 * ref2.abs().max().item()
    assert torch.equal(dmod2, dmod)
    # gated add: out = x + gate[b] * y
    yv = torch.randn(T * B, D, device=dev).bfloat16()
    out = K.gated_add_fwd(x, yv, emb, 2 * D, B)
    gr = er.detach()[:, 2 * D:].clone().requires_grad_(True)
    yr = yv.float().view(T, B, D).requires_grad_(True)
    refo = x.float().view(T, B, D) + gr[None] * yr
    assert rel(out, refo.reshape(T * B, D)) < 1e-2
    refo.backward(dy.float().view(T, B, D))
    dyv = K.gated_add_bwd(dy, yv, emb, 2 * D, B, dmod)
    assert rel(dyv, yr.grad.reshape(T * B, D)) < 1e-2
    assert rel(dmod[:, 2 * D:], gr.grad) < 2e-2
    # the split forms (module/flux.py with the modulation branch on the weight-gradient stream): the same bits
    dmod3 = dmod.clone()
    dmod3[:, :2 * D] = 0
    K.adaln_dmod(x, dy, emb, 0, D, B, st, dmod3)
    assert torch.equal(dmod3, dmod)


def test_qknorm_rope(dev):
    torch.manual_seed(1)
    cfg = FX.tiny_flux_config()
    L, h, w, B, H = 5, 8, 6, 2, 2
    T = L + (h // 2) * (w // 2)
    D = H * 128
    x = torch.randn(T * B, 3 * D, device=dev).bfloat16()
    ws = [(1 + 0.3 * torch.randn(128, device=dev)).bfloat16() for _ in range(4)]
    cs, sn = (torch.from_numpy(a).to(dev) for a in FX.rope_tables(L, h, w, cfg))
    out = K.qknorm_rope_fwd(x, 0, D, H, B, L, ws, cs, sn)
    # reference: RMSNorm per head (text rows use the *_ctx weights) then interleaved RoPE
    xr = x.float().view(T, B, 3 * D).requires_grad_(True)
    q, k = xr[..., :D].view(T, B, H, 128), xr[..., D:2 * D].view(T, B, H, 128)
    wf = [t_.float().requires_grad_(True) for t_ in ws]

    def norm(t_, w_img, w_ctx):
        n = t_ * torch.rsqrt(t_.pow(2).mean(-1, keepdim=True) + 1e-6)
        wsel = torch.cat([w_ctx.expand(L, 128), w_img.expand(T - L, 128)])[:, None, None, :]
        return n * wsel

    def rope(t_):
        c, s = cs[:, None, None, :], sn[:, None, None, :]
        xr_, xi_ = t_.reshape(*t_.shape[:-1], -1, 2).unbind(-1)
        rot = torch.stack([-xi_, xr_], -1).flatten(3)
        return t_ * c + rot * s

    rq, rk = rope(norm(q, wf[0], wf[2])), rope(norm(k, wf[1], wf[3]))
    ref = torch.cat([rq.reshape(T * B, D), rk.reshape(T * B, D)], 1)
    assert rel(out, ref) < 1e-2
    dy = torch.randn(T * B, 2 * D, device=dev).bfloat16()
    ref.backward(dy.float())
    dx = torch.zeros(T * B, 3 * D, dtype=BF, device=dev)
    dws = [torch.zeros(128, dtype=torch.float32, device=dev) for _ in range(4)]
    K.qknorm_rope_bwd(x, 0, D, dy, H, B, L, ws, cs, sn, dx, 0, D, dw=dws)
    assert rel(dx[:, :2 * D], xr.grad.reshape(T * B, 3 * D)[:, :2 * D]) < 2e-2
    for a, b in zip(dws, wf):
        assert rel(a, b.grad) < 2e-2


def test_gelu_tanh_and_pack(dev):
    torch.manual_seed(2)
    x = torch.randn(64, 96, device=dev).bfloat16()
    y = K.gelu_tanh_fwd(x)
    xr = x.float().requires_grad_(True)
    ref = F.gelu(xr, approximate="tanh")
    assert rel(y, ref) < 1e-2
    dy = torch.randn(64, 96, device=dev).bfloat16()
    ref.backward(dy.float())
    assert rel(K.gelu_tanh_bwd(x, dy), xr.grad) < 1e-2
    B, C, h, w = 2, 16, 8, 12
    lat = torch.randn(B, C, h, w, device=dev).bfloat16()
    tok = K.flux_pack(lat.permute(0, 2, 3, 1).contiguous())
    ref = OF.pack_latents(lat.float().cpu())                    # [B, N, 4C]
    assert torch.equal(tok.float().cpu().view(-1, B, 4 * C).transpose(0, 1), ref)
    back = K.flux_unpack(tok, B, h, w, C)
    assert torch.equal(back.permute(0, 3, 1, 2).float().cpu(), lat.float().cpu())


def _inputs(cfg, B, h, w, L, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(B, cfg.in_channels // 4, h, w, generator=g)
    packed = OF.pack_latents(lat)                                 # [B, N, 64]
    t = torch.tensor([0.537, 0.061][:B])
    guid = torch.ones(B)
    pooled = torch.randn(B, cfg.pooled_projection_dim, generator=g)
    ehs = torch.randn(B, L, cfg.joint_attention_dim, generator=g)
    return lat, packed, t, guid, pooled, ehs


@pytest.mark.parametrize("lora", [False, True])
def test_flux_transformer_matches_oracle(dev, lora):
    torch.manual_seed(0)
    cfg = FX.tiny_flux_config()
    m = FX.FluxTransformer2DModel(cfg, dev, seed=1, trainable=not lora)
    ocfg = OF.tiny_flux_config()
    om = OF.FluxTransformer2DModel(ocfg)
    om.load_state_dict({k: v.float().cpu() for k, v in m.state_dict().items()})
    B, h, w, L = 2, 16, 12, 7
    lat, packed, t, guid, pooled, ehs = _inputs(cfg, B, h, w, L, dev)
    lw = ol = ol64 = None
    if lora:
        from onetrainer_amd.module.lora import LoRAWrapper
        om.requires_grad_(False)
    om64 = copy.deepcopy(om).double()
    if lora:
        lw = LoRAWrapper(m, rank=8, alpha=4.0, prefix="lora_transformer", seed=0)
        m.lora = lw
        ol = OracleLoRA(om, 8, 4.0, prefix="lora_transformer")
        g = torch.Generator().manual_seed(3)
        lw.load_state_dict({k: (torch.randn(v.shape, generator=g) * 0.05 if not k.endswith(".alpha") else v)
                            for k, v in lw.state_dict().items()})
        ol.load_state_dict({k: v for k, v in lw.state_dict().items() if not k.endswith(".alpha")})
        ol64 = OracleLoRA(om64, 8, 4.0, prefix="lora_transformer")
        ol64.load_state_dict({k: v for k, v in lw.state_dict().items() if not k.endswith(".alpha")})
        for p in ol64.params.values():
            p.data = p.data.double()
    tok = packed.bfloat16().transpose(0, 1).reshape(-1, cfg.in_channels).to(dev)   # rows t*B + b
    out = m(tok, t.to(dev), guid.to(dev), pooled.to(dev).bfloat16(), ehs.to(dev).bfloat16(), h, w)
    ref = om(packed.bfloat16().float(), t, guid, pooled.bfloat16().float(), ehs.bfloat16().float(),
             torch.zeros(L, 3), OF.prepare_latent_image_ids(h, w))
    refr = ref.transpose(0, 1).reshape(-1, cfg.in_channels)
    e = rel(out, refr.detach())
    print("flux fwd rel err", e, "cos", _cos(out, refr.detach()))
    assert e < 3e-2 and _cos(out, refr.detach()) > 0.9995
    wgt = torch.randn(out.shape)
    store = lw.store if lora else m.store
    store.begin_backward()
    (out.float() * wgt.to(dev)).sum().backward()
    store.finish_backward()
    (refr * wgt).sum().backward()
    worst = []
    if lora:
        gs = lw.state_dict(grads=True)
        for k, p in ol.params.items():
            worst.append((_cos(gs[k].float().reshape(p.shape), p.grad), k))
        assert m.store.grad is None
    else:
        gs = m.state_dict(grads=True)
        for k, p in om.named_parameters():
            worst.append((_cos(gs[k], p.grad), k))
    worst.sort()
    print("worst grad cosines:", worst[:5])
    assert worst[0][0] > 0.99, worst[:5]
    # the same weights, inputs and upstream gradient in float64: the scale and the size of the error, per tensor
    r64 = om64(packed.bfloat16().double(), t, guid, pooled.bfloat16().double(), ehs.bfloat16().double(),
               torch.zeros(L, 3), OF.prepare_latent_image_ids(h, w))
    (r64.transpose(0, 1).reshape(-1, cfg.in_channels) * wgt.double()).sum().backward()
    p64 = ol64.params if lora else dict(om64.named_parameters())
    G.check({k: gs[k].float().cpu() for k in p64}, {k: p.grad for k, p in p64.items()}, f"flux lora={lora}")


def test_flux_lora_train_steps(dev):
    from onetrainer_amd.dataLoader.SyntheticDataLoader import synthetic_flux_batch
    from onetrainer_amd.trainer.GenericTrainer import GenericTrainer
    from onetrainer_amd.util import create
    from onetrainer_amd.util.config.TrainConfig import TrainConfig
    from oracle import diffusion as OD

    cfg = TrainConfig.default_values()
    cfg.model_type = "FLUX_DEV_1"
    cfg.training_method = "LORA"
    cfg.timestep_distribution = "LOGIT_NORMAL"
    cfg.batch_size = 2
    cfg.learning_rate = 3e-4
    cfg.learning_rate_warmup_steps = 0
    cfg.lora_rank, cfg.lora_alpha = 8, 8.0
    cfg.optimizer.stochastic_rounding = False
    fcfg = FX.tiny_flux_config()
    model = create.create_model(cfg, dev, seed=3, flux_config=fcfg)
    om = OF.FluxTransformer2DModel(OF.tiny_flux_config())
    om.load_state_dict({k: v.float().cpu() for k, v in model.transformer.state_dict().items()})
    om.requires_grad_(False)
    tr = GenericTrainer(cfg, model=model)
    tr.start()
    assert type(tr.model_setup).__name__ == "FluxLoRASetup"
    ol = OracleLoRA(om, 8, 8.0, prefix="lora_transformer")
    ol.load_state_dict({k: v.float().cpu() for k, v in model.transformer_lora.state_dict().items()
                        if not k.endswith(".alpha")})
    from _oracle_opt import OracleF32AdamW
    opt = OracleF32AdamW(ol.parameters(), lr=3e-4, weight_decay=1e-2)   # fp32 adapters, pinned AdamW restatement
    res = 128
    batch = synthetic_flux_batch(2, res, res, dev, seed=1, t5_dim=fcfg.joint_attention_dim,
                                 pooled_dim=fcfg.pooled_projection_dim, text_len=9)
    base0 = model.transformer.store.data.clone()
    h = w = res // 8
    lat = batch["latent_image"].cpu().float()
    x0 = (lat - 0.1159) * 0.3611
    ours, ref = [], []
    for step in range(2):
        gs = model.train_progress.global_step
        noise = K.noise((2, h, w, 16), seed=gs, dtype=torch.float32, device=dev)
        t = K.timesteps(2, seed=gs, dist=1, device=dev)
        ours.append(tr.train_step(batch).item())
        eps = noise.cpu().permute(0, 3, 1, 2)
        tc = t.cpu().long()
        xt, _ = OD.add_noise_flow(x0, eps, tc, 1000)      # ModelSetupFlowMatchingMixin (pinned oracle)
        pred = om(OF.pack_latents(xt).bfloat16().float(), tc.float() / 1000, torch.ones(2),
                  batch["text_encoder_1_pooled_state"].float().cpu(), batch["text_encoder_2_hidden_state"].float().cpu(),
                  torch.zeros(9, 3), OF.prepare_latent_image_ids(h, w))
        pred = OF.unpack_latents(pred, h, w)
        loss = ((pred - (eps - x0)) ** 2).mean()
        loss.backward()
        opt.step()
        ref.append(loss.item())
    print("flux lora losses hip", ours, "oracle", ref)
    for a, b in zip(ours, ref):
        assert abs(a - b) <= 1e-3 * abs(b), (ours, ref)
    assert torch.equal(model.transformer.store.data, base0)
