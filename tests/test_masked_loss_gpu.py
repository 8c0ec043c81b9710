"""Masked training on the HIP loss family (csrc/diffusion.hip otamd_diffusion_loss / _grad): mask-weighted
MSE / MAE / log-cosh against the reference's own ModelSetupDiffusionLossMixin results
(tests/golden/masked_losses.npz, made by tests/golden/make_masked_golden.py), from the kernel up to
scripts/train.py on the content of the reference's `#sd 1.5 masked.json` preset.

The loss tolerance is the fixture's `rtol` (4 x the reference's own fp32-vs-fp64 distance, or the project's 1e-6
when that fits inside it: see the generator).  Gradients are bf16: rtol 1e-2, atol 1e-6, as the flow-loss gradient
check of tests/test_reference_fixtures_gpu.py.
"""
import json
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from onetrainer_amd import kernels as K

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).parent / "golden"
sys.path.insert(0, str(GOLD))
from make_masked_golden import DDPM_FNS, GAMMA, STRENGTHS, case_key, grid  # noqa: E402

G = np.load(GOLD / "masked_losses.npz")
RTOL = float(G["rtol"][0])
BF = torch.bfloat16
CASES = [(fam,) + c for fam in ("ddpm", "flow") for c in grid(fam)]
IDS = [case_key(fam, m, uw, n, si, fn) for fam, m, uw, n, si, fn, vp in CASES]
C_OF = {"ddpm": 4, "flow": 16}
_cache: dict = {}


def inputs(fam, dev):
    """(pred NHWC bf16 padded to 8 / 16 channels, target NHWC f32, mask [B,1,h,w], lw, t), made once"""
    if fam not in _cache:
        C = C_OF[fam]
        pred = torch.from_numpy(G[f"{fam}_pred"].astype(np.int16)).view(BF).to(dev).permute(0, 2, 3, 1)
        pred = torch.nn.functional.pad(pred, (0, (C + 7) // 8 * 8 - C)).contiguous()   # ddpm: 4 zero pad channels
        target = torch.from_numpy(G[f"{fam}_target"]).to(dev).permute(0, 2, 3, 1).contiguous()
        mask = torch.from_numpy(G[f"{fam}_mask"]).to(dev).contiguous()
        lw = torch.from_numpy(G[f"{fam}_lw"]).to(dev)
        t = torch.from_numpy(G[f"{fam}_t"]).to(dev, torch.int32)
        _cache[fam] = (pred, target, mask, lw, t)
    return _cache[fam]


def coeffs(dev):
    if "coeffs" not in _cache:
        acp = torch.cumprod(1 - torch.from_numpy(G["betas"]), 0)
        _cache["coeffs"] = (acp.to(dev), acp.sqrt().to(dev), (1 - acp).sqrt().to(dev))
    return _cache["coeffs"]


def run(fam, dev, masked, uw, normalize, si, fn, vp, mask=None):
    pred, target, m, lw, t = inputs(fam, dev)
    mse_s, mae_s, lc_s = STRENGTHS[si]
    return K.diffusion_loss(pred, target, (m if mask is None else mask) if masked else None, lw, mse_strength=mse_s,
                            mae_strength=mae_s, log_cosh_strength=lc_s, unmasked_weight=uw, normalize=normalize,
                            loss_fn=K.LOSS_FN[fn], gamma=GAMMA, v_pred=vp, timestep=t,
                            coeffs=coeffs(dev) if fam == "ddpm" else None, num_t=1000)


def timestep_weight(fam, fn, vp, t, dev):
    """fp32 restatement of the timestep weights the fixture's grid uses (MIN_SNR_GAMMA, SIGMA)"""
    if fn == "SIGMA":
        return (t.float() + 1) / 1000
    if fn == "MIN_SNR_GAMMA":
        _, sq, s1m = coeffs(dev)
        snr = (sq / s1m)[t.long()] ** 2
        return torch.clamp(snr, max=GAMMA) / (snr + 1 if vp else snr)
    return torch.ones_like(t, dtype=torch.float32)


def restated_loss(pr, target, mask, masked, uw, normalize, strengths, w):
    """the loss formula, plainly, in fp32 torch ops: mean_b(w_b * sum_j s_j * mean(term_j * m) [/ mean(m)])"""
    d = pr - target
    terms = (d * d, d.abs(), d + torch.nn.functional.softplus(-2.0 * d) - float(np.log(2.0)))
    m = torch.clamp(mask, uw, 1).permute(0, 2, 3, 1) if masked else None
    losses = 0
    for term, s in zip(terms, strengths):
        if s == 0:
            continue
        if masked:
            term = term * m
            if normalize:
                term = term / m.mean(dim=(1, 2, 3), keepdim=True)
        losses = losses + term.mean(dim=(1, 2, 3)) * s
    return (losses * w).mean()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_losses_match_reference(dev, case):
    fam, masked, uw, normalize, si, fn, vp = case
    loss, coef, losses = run(fam, dev, masked, uw, normalize, si, fn, vp)
    ref = torch.from_numpy(G[case_key(fam, masked, uw, normalize, si, fn)])
    print("losses", losses.cpu().tolist(), "reference", ref.tolist(),
          "worst rel", ((losses.cpu() - ref).abs() / ref.abs()).max().item(), "rtol", RTOL)
    torch.testing.assert_close(losses.cpu(), ref, rtol=RTOL, atol=0)
    torch.testing.assert_close(loss.cpu()[0], ref.mean(), rtol=RTOL, atol=0)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gradient_matches_autograd(dev, case):
    fam, masked, uw, normalize, si, fn, vp = case
    pred, target, mask, lw, t = inputs(fam, dev)
    C = C_OF[fam]
    loss, coef, _ = run(fam, dev, masked, uw, normalize, si, fn, vp)
    g = K.diffusion_loss_grad(pred, target, coef, mask if masked else None, uw)
    pr = pred[..., :C].float().requires_grad_(True)
    w = lw * timestep_weight(fam, fn, vp, t, dev)
    ref = restated_loss(pr, target, mask, masked, uw, normalize, STRENGTHS[si], w)
    ref.backward()
    torch.testing.assert_close(loss[0], ref.detach(), rtol=1e-5, atol=0)   # the restatement is the same function
    torch.testing.assert_close(g[..., :C].float(), pr.grad, rtol=1e-2, atol=1e-6)
    assert torch.count_nonzero(g[..., C:]) == 0


@pytest.mark.parametrize("si", range(len(STRENGTHS)))
def test_gradient_is_zero_outside_the_mask_and_in_pad_channels(dev, si):
    pred, target, mask, lw, t = inputs("ddpm", dev)
    _, coef, _ = run("ddpm", dev, True, 0.0, True, si, "CONSTANT", False)
    g = K.diffusion_loss_grad(pred, target, coef, mask, 0.0)
    outside = (mask == 0).permute(0, 2, 3, 1).expand(-1, -1, -1, 4)
    assert outside.any() and (mask[1, :, :, :20] == 0).all()
    assert torch.count_nonzero(g[..., :4][outside]) == 0
    assert torch.count_nonzero(g[..., 4:]) == 0
    assert torch.count_nonzero(g[..., :4][~outside]) > 0.9 * (~outside).sum()


def test_mae_gradient_is_zero_where_pred_equals_target(dev):
    pred, target, mask, lw, t = inputs("ddpm", dev)
    _, coef, _ = run("ddpm", dev, True, 0.1, False, 1, "CONSTANT", False)
    g = K.diffusion_loss_grad(pred, target, coef, mask, 0.1)
    equal = pred[..., :4].float() == target
    assert equal.sum() >= 3 * 4
    assert torch.count_nonzero(g[..., :4][equal]) == 0
    assert torch.count_nonzero(g[..., :4][~equal]) == (~equal).sum()   # sign(d) * coef * m, m >= 0.1


@pytest.mark.parametrize("fn,vp", DDPM_FNS)
def test_all_ones_mask_mse_equals_mse_loss(dev, fn, vp):
    pred, target, mask, lw, t = inputs("ddpm", dev)
    loss, _, losses = run("ddpm", dev, True, 0.1, False, 0, fn, vp, mask=torch.ones_like(mask))
    l0, _, ls0 = K.mse_loss(pred, target, lw, loss_fn=K.LOSS_FN[fn], gamma=GAMMA, v_pred=vp, timestep=t,
                            coeffs=coeffs(dev))
    torch.testing.assert_close(losses, ls0, rtol=RTOL, atol=0)
    torch.testing.assert_close(loss, l0, rtol=RTOL, atol=0)


def _config(masked, uw, normalize, si, fn):
    from onetrainer_amd.util.config.TrainConfig import TrainConfig
    c = TrainConfig.default_values()
    c.masked_training, c.unmasked_weight, c.normalize_masked_area_loss = masked, uw, normalize
    c.mse_strength, c.mae_strength, c.log_cosh_strength = STRENGTHS[si]
    c.loss_weight_fn, c.loss_weight_strength = fn, GAMMA
    return c


def _setup_call(fam, dev, cfg, vp, with_mask=True):
    """calculate_loss of the family's setup on the fixture, handed over in the reference's [B, C, h, w] contract"""
    pred, target, mask, lw, t = inputs(fam, dev)
    C = C_OF[fam]
    batch = {"loss_weight": lw}
    if with_mask:
        batch["latent_mask"] = mask
    data = {"loss_type": "target", "timestep": t, "predicted": pred[..., :C].permute(0, 3, 1, 2),
            "target": target.permute(0, 3, 1, 2), "prediction_type": "v_prediction" if vp else "epsilon"}
    sched = SimpleNamespace(coeffs=coeffs(dev), config={"num_train_timesteps": 1000})
    if fam == "ddpm":
        from onetrainer_amd.modelSetup.BaseStableDiffusionXLSetup import BaseStableDiffusionXLSetup as Setup
    else:
        from onetrainer_amd.modelSetup.BaseFluxSetup import BaseFluxSetup as Setup
    return Setup(dev).calculate_loss(SimpleNamespace(noise_scheduler=sched), batch, data, cfg)


@pytest.mark.parametrize("fam,masked,uw,normalize,si,fn,vp", [
    ("ddpm", True, 0.1, True, 3, "MIN_SNR_GAMMA", True), ("ddpm", True, 0.0, False, 2, "CONSTANT", False),
    ("ddpm", False, 0.1, False, 1, "CONSTANT", False), ("flow", True, 0.1, True, 3, "SIGMA", False),
    ("flow", True, 0.0, True, 0, "SIGMA", False), ("flow", False, 0.1, False, 2, "SIGMA", False)])
def test_calculate_loss_reproduces_reference(dev, fam, masked, uw, normalize, si, fn, vp):
    loss = _setup_call(fam, dev, _config(masked, uw, normalize, si, fn), vp)
    ref = torch.from_numpy(G[case_key(fam, masked, uw, normalize, si, fn)])
    torch.testing.assert_close(loss.cpu(), ref.mean(), rtol=RTOL, atol=0)


@pytest.mark.parametrize("fam", ["ddpm", "flow"])
def test_calculate_loss_names_the_missing_mask(dev, fam):
    with pytest.raises(KeyError, match="latent_mask"):
        _setup_call(fam, dev, _config(True, 0.1, False, 0, "CONSTANT"), False, with_mask=False)


def test_loss_fn_backward_folds_grad_scale(dev):
    from onetrainer_amd.module import functional as Fn
    pred, target, mask, lw, t = inputs("ddpm", dev)
    grads = []
    for gs in (1.0, 0.5):
        p = pred.clone().requires_grad_(True)
        loss = Fn.DiffusionLossFn.apply(p, target, mask, lw, t, coeffs(dev), K.LOSS_FN["MIN_SNR_GAMMA"], GAMMA, True,
                                        1.0, STRENGTHS[3], 0.1, True, 1.0, gs)
        loss.backward()
        grads.append(p.grad.float())
    assert torch.count_nonzero(grads[0]) > 0
    assert torch.equal(grads[1], grads[0] * 0.5)   # a power of two: exact through the fp32 product and the bf16 rounding
    ref = torch.from_numpy(G[case_key("ddpm", True, 0.1, True, 3, "MIN_SNR_GAMMA")]).mean()
    torch.testing.assert_close(loss.detach().cpu(), ref, rtol=RTOL, atol=0)


# training_presets/#sd 1.5 masked.json of the reference, field for field (settings only)
SD15_MASKED_PRESET = {"base_model_name": "stable-diffusion-v1-5/stable-diffusion-v1-5", "batch_size": 4,
                      "masked_training": True, "max_noising_strength": 0.8, "model_type": "STABLE_DIFFUSION_15",
                      "normalize_masked_area_loss": True, "output_model_destination": "models/model.safetensors",
                      "output_model_format": "SAFETENSORS", "resolution": "512", "training_method": "FINE_TUNE",
                      "vae": {"weight_dtype": "FLOAT_32"}}


def test_train_script_runs_sd15_masked_preset(dev, tmp_path):
    """the masked SD 1.5 preset through scripts/train.py for one epoch, on a cache LatentCacheWriter wrote from
    samples that carry a mask (a tiny SD 1.5-shaped base stands in for the hub model, as in tests/test_cli_gpu.py)"""
    import importlib.util

    from onetrainer_amd.dataLoader.aspect_bucketing import AspectBucketing
    from onetrainer_amd.dataLoader.latent_cache import LatentCacheWriter
    from onetrainer_amd.modelSaver import StableDiffusionXLModelSaver
    from onetrainer_amd.module import unet as U
    from onetrainer_amd.module import vae as V
    from onetrainer_amd.util import create
    from onetrainer_amd.util.config.TrainConfig import TrainConfig
    torch.manual_seed(1)
    base_cfg = TrainConfig.default_values()
    base_cfg.model_type = "STABLE_DIFFUSION_15"
    base = create.create_model(base_cfg, dev, seed=5, unet_config=U.tiny_sd15_config())
    StableDiffusionXLModelSaver().save(base, None, "DIFFUSERS", str(tmp_path / "base"))
    enc = V.AutoencoderKLEncoder(V.tiny_vae_config(), dev, seed=1)
    samples = []
    for i in range(8):
        mask = torch.zeros(1, 128, 128)
        mask[:, 16 + 8 * i:96, 32:112] = 1.0
        samples.append({"image": torch.rand(3, 128, 128), "mask": mask,
                        "text": {"text_encoder_hidden_state": torch.randn(77, 96).bfloat16()}})
    cache = tmp_path / "cache"
    LatentCacheWriter(lambda im: enc.encode(im), str(cache), AspectBucketing(128, 64), dev, encode_batch=4).write(samples)
    cfg = dict(SD15_MASKED_PRESET)
    cfg.update({"base_model_name": str(tmp_path / "base"), "cache_dir": str(cache), "epochs": 1,
                "workspace_dir": str(tmp_path / "ws"), "learning_rate_warmup_steps": 0,
                "output_model_destination": str(tmp_path / "out" / "model.safetensors"), "output_dtype": "FLOAT_32"})
    path = tmp_path / "config.json"
    path.write_text(json.dumps(cfg))
    spec = importlib.util.spec_from_file_location("train_script", Path(__file__).parents[1] / "scripts" / "train.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    tr = mod.main(["--config-path", str(path)])
    assert tr.config.masked_training and tr.config.normalize_masked_area_loss and tr.data_loader.require_mask
    assert tr.model.train_progress.global_step == 2
    assert tr.loss_history and all(torch.isfinite(l).item() for l in tr.loss_history)
    sd, base_sd = tr.model.unet.state_dict(), base.unet.state_dict()
    moved = sum(not torch.equal(sd[k].float(), base_sd[k].float()) for k in sd)
    assert moved > 0.5 * len(sd)
