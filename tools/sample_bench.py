"""Time one training sample (SDXL, 1024 x 1024, 20 DDIM steps, random weights) and its parts on the GPU.

Each part is its own process under its own time limit, chained so that trouble ends the chain:

    timeout -k 10 300 python tools/sample_bench.py --part step   && \\
    timeout -k 10 300 python tools/sample_bench.py --part unet   && \\
    timeout -k 10 300 python tools/sample_bench.py --part decode && \\
    timeout -k 10 300 python tools/sample_bench.py --part total

Every part merges its figures into profiles/sample_bench.json (--out).  Parts:
  step    the fused guidance + rescale + DDIM kernel (kernels.cfg_ddim_step) against the same step written as the
          unfused torch expression below, and its achieved bandwidth over the bytes it must move: pred is read twice
          (statistics, then update: 2 x 2 x 16 B per pixel), x read and written (2 x 16 B), the next input written
          (2 x 16 B) = 128 B per latent pixel with the rescale, 96 B without
  unet    one UNet forward at batch 2
  decode  the VAE decoder + the 8-bit conversion
  total   StableDiffusionSampler.sample_image end to end (ready prompt states)
Times are medians of --reps runs after --warmup runs, by device events around each run.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from onetrainer_amd import kernels as K  # noqa: E402
from onetrainer_amd.model.StableDiffusionXLModel import NoiseScheduler, StableDiffusionXLModel  # noqa: E402
from onetrainer_amd.modelSampler import StableDiffusionSampler, ddim_table  # noqa: E402
from onetrainer_amd.module import unet as U  # noqa: E402
from onetrainer_amd.module import vae as V  # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return {"median_us": statistics.median(out), "min_us": min(out), "max_us": max(out), "reps": reps}


def torch_step(pred, x, coeffs, t, tp, cfg, rescale):
    """the reference's per-step expressions (StableDiffusionXLSampler.py:156-172, DDIM eta 0, epsilon) as torch ops"""
    neg, pos = pred[..., :4].float().chunk(2)
    p = neg + cfg * (pos - neg)
    dims = [1, 2, 3]
    p = rescale * (p * (pos.std(dim=dims, keepdim=True) / p.std(dim=dims, keepdim=True))) + (1 - rescale) * p
    sa, s1, sap, s1p = coeffs[1][t], coeffs[2][t], coeffs[1][tp], coeffs[2][tp]
    x0 = (x - s1 * p) / sa
    xp = sap * x0 + s1p * p
    nxt = torch.zeros_like(pred)
    nxt[..., :4] = torch.cat([xp, xp]).to(torch.bfloat16)
    return xp, nxt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["step", "unet", "decode", "total"])
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="profiles/sample_bench.json")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    h = w = a.size // 8
    res = {}
    ns = NoiseScheduler(dev)
    t, tp = ddim_table(a.steps)[a.steps // 2]
    if a.part == "step":
        g = torch.Generator(device=dev).manual_seed(0)
        pred = torch.zeros(2, h, w, 8, dtype=torch.bfloat16, device=dev)
        pred[..., :4] = torch.randn(2, h, w, 4, generator=g, device=dev).bfloat16()
        x = torch.randn(1, h, w, 4, generator=g, device=dev)
        out, nxt = torch.empty_like(x), torch.empty_like(pred)
        for name, r, nbytes in (("rescale_0.7", 0.7, 128), ("rescale_0", 0.0, 96)):
            f = timed(lambda: K.cfg_ddim_step(pred, x, ns.coeffs, t, tp, 7.0, r, False, out=out, next_in=nxt),
                      a.warmup, a.reps * 5)
            f["bytes"] = nbytes * h * w
            f["gb_per_s"] = f["bytes"] / f["median_us"] / 1e3
            res["step_kernel_" + name] = f
        res["step_torch_unfused"] = timed(lambda: torch_step(pred, x, ns.coeffs, t, tp, 7.0, 0.7), a.warmup, a.reps * 5)
        xp, _ = torch_step(pred, x, ns.coeffs, t, tp, 7.0, 0.7)
        got, _ = K.cfg_ddim_step(pred, x, ns.coeffs, t, tp, 7.0, 0.7, False)
        res["step_max_abs_diff_vs_torch"] = float((got - xp).abs().max())
    else:
        cfg = U.sdxl_config()
        states = {k: (torch.randn(1, 77, cfg.cross_attention_dim, device=dev).bfloat16(),
                      torch.randn(1, 1280, device=dev).bfloat16()) for k in ("positive", "negative")}
        if a.part in ("unet", "total"):
            unet = U.UNet2DConditionModel(cfg, dev, seed=0, trainable=False)
            model = StableDiffusionXLModel(unet, ns)
        if a.part in ("decode", "total"):
            dec = V.AutoencoderKLDecoder(V.sdxl_vae_config(), dev, seed=0)
        with torch.no_grad():
            if a.part == "unet":
                xin = torch.zeros(2, h, w, 8, dtype=torch.bfloat16, device=dev)
                hid = torch.cat([states["negative"][0], states["positive"][0]])
                pooled = torch.cat([states["negative"][1], states["positive"][1]])
                ids = torch.tensor([[a.size, a.size, 0, 0, a.size, a.size]] * 2, dtype=torch.float32, device=dev)
                ts = torch.tensor([t], dtype=torch.int32, device=dev)
                res["unet_forward_b2"] = timed(lambda: unet(xin, ts, hid, pooled, ids), a.warmup, a.reps)
            elif a.part == "decode":
                lat = torch.randn(1, h, w, 4, device=dev) * 0.13025
                res["decode_and_rgb8"] = timed(lambda: K.nhwc_to_rgb8(dec.decode(lat)), a.warmup, a.reps)
            else:
                model.vae_decoder = dec
                sampler = StableDiffusionSampler(model, dev)
                sc = {"height": a.size, "width": a.size, "diffusion_steps": a.steps, "seed": 1}
                res["sample_total"] = timed(lambda: sampler.sample_image(sc, states), 1, max(3, a.reps // 3))
    res = {k: dict(v, size=a.size, steps=a.steps) if isinstance(v, dict) else v for k, v in res.items()}
    merged = {}
    if os.path.isfile(a.out):
        with open(a.out) as f:
            merged = json.load(f)
    merged.update(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=1, sort_keys=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
