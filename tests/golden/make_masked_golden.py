"""Generate tests/golden/masked_losses.npz by running the REFERENCE's own loss code (container only).

    python tests/golden/make_masked_golden.py          # needs /root/reference (read-only)

Imports modules/modelSetup/mixin/ModelSetupDiffusionLossMixin.py directly, like make_golden.py, and runs its
_diffusion_losses / _flow_matching_losses with masked_training on (the __masked_losses branch with
masked_losses_with_prior, masked_prior_preservation_weight 0) and off (__unmasked_losses) for the MSE, MAE and
log-cosh terms.  Inputs and per-sample losses are recorded as .npz data; nothing of the reference's source is
stored.

Tolerance.  Each case is also recomputed in fp64 from the same formula and the same inputs (the fp32 schedule
tables included, upcast: they are inputs of the loss, not part of it).  `ref_dist` is the worst relative distance
of the reference's fp32 result from that fp64 value over the whole grid.  The kernels and the reference are both
fp32 sums in different orders, so each may sit that far from fp64 on opposite sides (x2), doubled for headroom
(x2): `rtol` = 1e-6 (the project's existing loss tolerance) when 4 * ref_dist fits inside it, else 4 * ref_dist.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent

UNMASKED_WEIGHTS = (0.0, 0.1)
STRENGTHS = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.5, 0.3, 0.2))   # mse, mae, log-cosh
DDPM_FNS = (("CONSTANT", False), ("MIN_SNR_GAMMA", True))                        # (loss weight fn, v-prediction)
GAMMA = 5.0


def case_key(family: str, masked: bool, uw: float, normalize: bool, si: int, fn: str) -> str:
    """name of one grid case's per-sample losses in the npz (tests rebuild the grid with it)"""
    return f"{family}_m{int(masked)}_uw{uw}_n{int(normalize)}_s{si}_{fn}"


def grid(family: str):
    fns = DDPM_FNS if family == "ddpm" else (("SIGMA", False),)
    for fn, vp in fns:
        for si in range(len(STRENGTHS)):
            for uw in UNMASKED_WEIGHTS:
                for normalize in (False, True):
                    yield True, uw, normalize, si, fn, vp
            yield False, 0.1, False, si, fn, vp


def bf16_bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).numpy().astype(np.uint16)


def make_inputs(B, C, h, w, seed):
    """pred bf16 / target f32 [B, C, h, w], mask f32 [B, 1, h, w]: sample 0 all ones, sample 1 zero over its left
    half, the rest a mix of exact 0, exact 1 and fractions; a few elements with pred == target and a few with
    |pred - target| = 12 (log-cosh's softplus threshold at 2 |d| > 20)."""
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(B, C, h, w, generator=g).bfloat16()
    target = torch.randn(B, C, h, w, generator=g)
    mask = torch.rand(B, 1, h, w, generator=g)
    sel = torch.rand(B, 1, h, w, generator=g)
    mask[sel < 0.25] = 0.0
    mask[sel > 0.75] = 1.0
    mask[0] = 1.0
    mask[1, :, :, : w // 2] = 0.0
    pf = pred.float()
    for b in range(B):
        for k, (c, y, x) in enumerate(((0, 0, 0), (C - 1, h - 1, w - 1), (1, h // 2, w // 2 + 1), (2, 3, w - 2))):
            target[b, c, y, x] = pf[b, c, y, x]                      # pred == target exactly
        target[b, 0, 1, w - 1] = pf[b, 0, 1, w - 1] + 12.0           # d = -12: softplus(24) takes the linear branch
        target[b, 1, 2, w - 3] = pf[b, 1, 2, w - 3] - 12.0           # d = +12
    return pred, target, mask


def fp64_losses(pred, target, mask, masked, uw, normalize, strengths, weight64):
    """the same formula in fp64: per-sample mean of (term * m) [/ mean(m)], strengths, then the fp64 weights"""
    d = pred.double() - target.double()
    terms = (d * d, d.abs(), d + torch.nn.functional.softplus(-2.0 * d) - np.log(2.0))
    losses = torch.zeros(pred.shape[0], dtype=torch.float64)
    m = torch.clamp(mask, uw, 1).double() if masked else None   # the clamp selects fp32 values: exact
    for term, s in zip(terms, strengths):
        if s == 0:
            continue
        if masked:
            term = term * m
            if normalize:
                term = term / m.mean(dim=(1, 2, 3), keepdim=True)
        losses = losses + term.mean(dim=(1, 2, 3)) * s
    return losses * weight64


def main():
    sys.path.insert(0, str(REF))
    from modules.modelSetup.mixin.ModelSetupDiffusionLossMixin import ModelSetupDiffusionLossMixin
    from modules.util.config.TrainConfig import TrainConfig
    from modules.util.DiffusionScheduleCoefficients import DiffusionScheduleCoefficients
    from modules.util.enum.LossWeight import LossWeight

    class Probe(ModelSetupDiffusionLossMixin):
        pass

    rec: dict[str, np.ndarray] = {}
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2
    rec["betas"] = betas.numpy()
    rec["strengths"] = np.array(STRENGTHS, dtype=np.float64)
    rec["unmasked_weights"] = np.array(UNMASKED_WEIGHTS, dtype=np.float64)
    rec["gamma"] = np.array([GAMMA], dtype=np.float64)
    co = DiffusionScheduleCoefficients.from_betas(betas)
    worst = 0.0

    def config(masked, uw, normalize, strengths, fn):
        c = TrainConfig.default_values()
        c.masked_training, c.unmasked_weight, c.normalize_masked_area_loss = masked, uw, normalize
        c.mse_strength, c.mae_strength, c.log_cosh_strength = strengths
        c.loss_weight_fn, c.loss_weight_strength = LossWeight[fn], GAMMA
        assert c.masked_prior_preservation_weight == 0.0
        return c

    for family, (B, C, h, w), seed, t, lw in (("ddpm", (3, 4, 24, 40), 31, [3, 517, 999], [1.0, 0.5, 2.0]),
                                              ("flow", (2, 16, 16, 12), 32, [100, 899], [1.0, 0.7])):
        pred, target, mask = make_inputs(B, C, h, w, seed)
        t, lw = torch.tensor(t, dtype=torch.int32), torch.tensor(lw)
        rec[f"{family}_pred"], rec[f"{family}_target"], rec[f"{family}_mask"] = bf16_bits(pred), target.numpy(), mask.numpy()
        rec[f"{family}_t"], rec[f"{family}_lw"] = t.numpy(), lw.numpy()
        for masked, uw, normalize, si, fn, vp in grid(family):
            c = config(masked, uw, normalize, STRENGTHS[si], fn)
            batch = {"loss_weight": lw.clone(), "latent_mask": mask.clone()}
            data = {"loss_type": "target", "timestep": t.long(), "predicted": pred.clone(), "target": target.clone()}
            w64 = lw.double()
            if family == "ddpm":
                data["prediction_type"] = "v_prediction" if vp else "epsilon"
                losses = Probe()._diffusion_losses(batch, data, c, torch.device("cpu"), betas=betas)
                if fn == "MIN_SNR_GAMMA":
                    snr = (co.sqrt_alphas_cumprod.double() / co.sqrt_one_minus_alphas_cumprod.double())[t.long()] ** 2
                    w64 = w64 * torch.clamp(snr, max=GAMMA) / (snr + 1.0 if vp else snr)
            else:
                losses = Probe()._flow_matching_losses(batch, data, c, torch.device("cpu"), sigmas=torch.zeros(1000))
                w64 = w64 * ((t.double() + 1.0) / 1000.0)
            ref64 = fp64_losses(pred, target, mask, masked, uw, normalize, STRENGTHS[si], w64)
            assert losses.dtype == torch.float32 and torch.isfinite(losses).all()
            worst = max(worst, ((losses.double() - ref64).abs() / ref64.abs()).max().item())
            rec[case_key(family, masked, uw, normalize, si, fn)] = losses.numpy()

    rtol = 1e-6 if 4.0 * worst <= 1e-6 else 4.0 * worst
    rec["ref_dist"] = np.array([worst], dtype=np.float64)
    rec["rtol"] = np.array([rtol], dtype=np.float64)
    np.savez_compressed(OUT / "masked_losses.npz", **rec)
    print("wrote", OUT / "masked_losses.npz", len(rec), "arrays; reference fp32 vs fp64:", worst, "rtol:", rtol)


if __name__ == "__main__":
    main()
