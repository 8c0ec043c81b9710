"""Whole-network gradients of the HIP networks against the float64 oracle, per tensor: scale, relative L2 error and
cosine (_grad_parity.py; the bounds are measured on the CPU, test_grad_parity_ref.py).  One backward into a NaN-filled
gradient buffer (every first writer overwrites, unwritten tensors are zeroed, the padding between tensors is nobody's),
two micro-steps into one buffer against grad(A) + grad(B), and the trainer's 1 / (B ga) against the float64 gradient
of the mean loss."""
import pytest
import torch

import _grad_parity as G
from _norm_edges import NANBITS

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _hip(case, dev):
    """(case, HIP model holding the case's weights, adapter wrapper or None, the store that is trained)"""
    from onetrainer_amd.module import flux as FX
    from onetrainer_amd.module import unet as U
    from onetrainer_amd.module.lora import LoRAWrapper
    c = G.make_case(case)
    if c["flux"]:
        cfg = FX.tiny_flux_config()
        m = FX.FluxTransformer2DModel(cfg, dev, seed=None, trainable=not c["lora"])
    else:
        cfg = U.tiny_sd15_config() if case == "tiny_sd15" else U.tiny_sdxl_config()
        m = U.UNet2DConditionModel(cfg, dev, seed=None, trainable=not c["lora"])
    for k in type(c["cfg"]).__dataclass_fields__:      # the oracle's configuration is the HIP model's
        assert getattr(cfg, k) == getattr(c["cfg"], k), k
    m.load_state_dict(c["weights"])
    lw = None
    if c["lora"]:
        lw = LoRAWrapper(m, rank=G.LORA_RANK, alpha=G.LORA_ALPHA, prefix=c["prefix"], seed=0)
        m.lora = lw
        lw.load_state_dict(c["lora_sd"])
        assert m.store.grad is None     # frozen base: no base gradient buffer at all
    return c, m, lw, (lw.store if lw is not None else m.store)


def _forward(c, m, b, dev):
    """(the network's output, the upstream gradient in the output's layout)"""
    if c["flux"]:
        C = c["cfg"].in_channels
        tok = b["packed"].to(BF).transpose(0, 1).reshape(-1, C).to(dev)       # rows t * B + b
        out = m(tok, b["t"].to(dev), b["guid"].to(dev), b["pooled"].to(dev).to(BF), b["ehs"].to(dev).to(BF),
                b["h"], b["w"])
        return out, b["up"].transpose(0, 1).reshape(-1, C).to(dev)
    B, _, H, W = b["x"].shape
    xin = torch.zeros(B, H, W, 8, dtype=BF, device=dev)
    xin[..., :4] = b["x"].permute(0, 2, 3, 1).to(dev).to(BF)
    dv = (lambda v, dt=None: None if v is None else v.to(dev).to(dt or v.dtype))
    out = m(xin, b["t"].to(dev), dv(b["ehs"], BF), dv(b["te"], BF), dv(b["tid"]))
    return out[..., :4], b["up"].permute(0, 2, 3, 1).to(dev)


def _micro_step(c, m, store, b, dev, accumulating):
    store.accumulating = accumulating
    out, up = _forward(c, m, b, dev)
    store.begin_backward()
    (out.float() * up).sum().backward()
    store.finish_backward()


def _grads(m, lw):
    sd = (lw if lw is not None else m).state_dict(grads=True)
    return {k: v.float().cpu() for k, v in sd.items() if not k.endswith(".alpha")}


def _inside(store):
    inside = torch.zeros(store.numel, dtype=torch.bool, device=store.device)
    for s in store.slots.values():
        inside[s.offset:s.offset + s.numel] = True
    return inside


@pytest.mark.parametrize("case", G.CASES)
def test_one_backward_overwrites_nan_prefill(dev, case):
    """the gradient buffer starts as NaN everywhere, the padding between the tensors included: after one backward with
    accumulating = False no element of any tensor is NaN (every first writer overwrote, finish_backward zeroed the
    rest), the padding still holds the fill (it belongs to no tensor: the optimizers' fs_valid masks), and every
    tensor is within the bounds of the float64 oracle.  Every tensor of these configurations is a multiple of 8
    elements, so their stores have no padding today and that one assertion holds vacuously (the count is printed)."""
    c, m, lw, store = _hip(case, dev)
    bits = store.grad.view(torch.int16)
    bits.fill_(NANBITS)
    assert bool(torch.isnan(store.grad).all())
    _micro_step(c, m, store, c["batches"][0], dev, False)
    torch.cuda.synchronize()
    inside = _inside(store)
    nan = torch.isnan(store.grad)
    bad = [n for n, s in store.slots.items() if bool(nan[s.offset:s.offset + s.numel].any())]
    assert not bad, f"{len(bad)} tensors kept NaN from the pre-fill (added instead of overwritten): {bad[:8]}"
    pad = bits.view(store.numel, -1)[~inside]
    print(f"{case}: {int(inside.sum())} elements in {len(store.slots)} tensors, {pad.shape[0]} padding elements")
    assert bool((pad == NANBITS).all()), "a backward kernel wrote into the padding between two tensors"
    G.check(_grads(m, lw), G.reference(case)["A"], f"{case} one backward")


@pytest.mark.parametrize("case", G.CASES)
def test_two_micro_steps_accumulate(dev, case):
    """micro-batch A with accumulating = False, then B with accumulating = True (as GenericTrainer.train_step sets it)
    against the float64 grad(A) + grad(B); then zero_grad() and A once more against grad(A): nothing of B survives"""
    from onetrainer_amd.util.optimizer.adamw_fused import FusedAdamW
    c, m, lw, store = _hip(case, dev)
    ref = G.reference(case)
    opt = FusedAdamW(store, [{"params": [p for _, p in store.named_parameters()]}])
    A, B = c["batches"]
    _micro_step(c, m, store, A, dev, False)
    _micro_step(c, m, store, B, dev, True)
    G.check(_grads(m, lw), ref["AB"], f"{case} A then B")
    opt.zero_grad()
    assert store.accumulating is False
    _micro_step(c, m, store, A, dev, store.accumulating)
    G.check(_grads(m, lw), ref["A"], f"{case} A after zero_grad")


def _slice(batch, lo, hi):
    out = {}
    for k, v in batch.items():
        if torch.is_tensor(v):
            out[k] = v[lo:hi]
        elif isinstance(v, tuple):
            out[k] = tuple(x[lo:hi] for x in v)
        else:
            out[k] = v[lo:hi]
    return out


def test_trainer_scaling_matches_oracle(dev):
    """one GenericTrainer window on the tiny SDXL config: batch_size 2 x gradient_accumulation_steps 2 and the same
    four samples at batch_size 4 x 1, with the same injected noise and timesteps.  Both gradient buffers against each
    other and against the float64 oracle gradient of the mean loss over the four samples (the 1 / (B ga) that `coef`
    of csrc/diffusion.hip carries), and the clip's total norm against the float64 norm."""
    from onetrainer_amd.dataLoader.SyntheticDataLoader import synthetic_sdxl_batch
    from onetrainer_amd.module import unet as U
    from onetrainer_amd.trainer.GenericTrainer import GenericTrainer
    from onetrainer_amd.util import create
    from onetrainer_amd.util.config.TrainConfig import TrainConfig
    from oracle import diffusion as OD
    from oracle import unet as OU

    res, N = 128, 4
    ucfg = U.tiny_sdxl_config()
    batch = synthetic_sdxl_batch(N, res, res, dev, seed=1, te1_dim=48, te2_dim=48, pooled_dim=64)
    g = torch.Generator().manual_seed(5)
    noise = torch.randn(N, res // 8, res // 8, 4, generator=g).to(dev)          # NHWC, as step_inputs draws it
    tsteps = torch.tensor([10, 700, 500, 3], dtype=torch.int32, device=dev)

    def run(bs, ga):
        cfg = TrainConfig.default_values()
        cfg.batch_size, cfg.gradient_accumulation_steps = bs, ga
        cfg.learning_rate = 1e-4
        cfg.learning_rate_warmup_steps = 0
        cfg.optimizer.stochastic_rounding = False
        assert cfg.clip_grad_norm == 1.0
        model = create.create_model(cfg, dev, seed=3, unet_config=ucfg)
        tr = GenericTrainer(cfg, model=model)
        tr.start()
        weights = {k: v.float().cpu() for k, v in model.unet.state_dict().items()}
        pos, cap = [0], {}

        def step_inputs(*a, **k):     # the window's noise and timesteps, sample by sample
            lo = pos[0]
            pos[0] += bs
            return noise[lo:lo + bs].contiguous(), tsteps[lo:lo + bs].contiguous()

        tr.model_setup.step_inputs = step_inputs
        opt, step = model.optimizer, model.optimizer.step

        def capture(*a, **k):         # the gradients and the clip's norm as the optimizer is about to read them
            cap["grads"] = {k_: v.float().cpu() for k_, v in model.unet.state_dict(grads=True).items()}
            cap["norm"] = float(opt.clip_out[1])
            return step(*a, **k)

        opt.step = capture
        for i in range(ga):
            tr.train_step(_slice(batch, i * bs, (i + 1) * bs))
        assert pos[0] == N and "grads" in cap
        return weights, cap

    w22, c22 = run(2, 2)
    w41, c41 = run(4, 1)
    assert all(torch.equal(w22[k], w41[k]) for k in w22)

    om = OU.UNet2DConditionModel(OU.UNetConfig(**{k: getattr(ucfg, k) for k in OU.UNetConfig.__dataclass_fields__}))
    om.load_state_dict(w22)
    om.double()
    lat = batch["latent_image"].cpu().float()
    eps = noise.cpu().permute(0, 3, 1, 2)
    tc = tsteps.cpu().long()
    xt = OD.add_noise_ddpm(lat * 0.13025, eps, tc, OD.scaled_linear_betas())
    ehs = torch.cat([batch["text_encoder_1_hidden_state"], batch["text_encoder_2_hidden_state"]], -1).double().cpu()
    te = batch["text_encoder_2_pooled_state"].double().cpu()
    tid = torch.tensor([[res, res, 0, 0, res, res]] * N, dtype=torch.float32)
    pred = om(xt.bfloat16().double(), tc, ehs, te, tid)
    # the constant-weight MSE of OD.diffusion_losses, kept in float64: per-sample means, then the mean over the four
    ((pred - eps.double()) ** 2).mean(dim=(1, 2, 3)).mean().backward()
    ref = {k: p.grad.double() for k, p in om.named_parameters()}
    assert all(torch.count_nonzero(r) for r in ref.values())

    G.check(c22["grads"], ref, "trainer B=2 ga=2 vs oracle")
    G.check(c41["grads"], ref, "trainer B=4 ga=1 vs oracle")
    G.check(c22["grads"], {k: v.double() for k, v in c41["grads"].items()}, "trainer B=2 ga=2 vs B=4 ga=1")
    total = float(torch.sqrt(sum((r * r).sum() for r in ref.values())))
    print(f"clip total norm: B=2 ga=2 {c22['norm']:.6g}  B=4 ga=1 {c41['norm']:.6g}  float64 {total:.6g}")
    for n in (c22["norm"], c41["norm"]):
        assert abs(n - total) <= G.S_BOUND * total, (n, total)
