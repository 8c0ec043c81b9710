"""Time the SDXL LoRA train step at the `bench.py --model sdxl-lora` shape with LoRA dropout off and on, and the
dropout kernel on its own.

    python tools/lora_dropout_bench.py [--steps 8] [--warmup 3] [--rank 32] [--batch 4] [--res 1024] [--p 0.1]

The workload is bench.py's sdxl-lora one (training_presets "#sdxl 1.0 LoRA" + rank 32, fp32 adapters, aspect-ratio
buckets drawn by the same seeds), once with `dropout_probability` 0 (bench.py's own path: fused forward and input
gradient where the plans allow) and once with `--p` (the two-launch forms with the mask kernel in between), in one
process, so the two p50 compare.  Then the mask kernel alone (hipEvents around 20 launches, median of `--reps`) on a streaming size
([2^20, 128] bf16, 256 MiB read and 256 MiB written) and on the step's own largest t ([batch * (res / 8)^2, rank]), with
the achieved GB/s (2 bytes read + 2 written per element).  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import gc
import json
import random
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def step_times(args, p: float):
    from onetrainer_amd import kernels as K
    from onetrainer_amd.dataLoader.aspect_bucketing import ASPECTS, AspectBucketing
    from onetrainer_amd.dataLoader.SyntheticDataLoader import synthetic_sdxl_batch
    from onetrainer_amd.trainer.GenericTrainer import GenericTrainer
    from onetrainer_amd.util.config.TrainConfig import TrainConfig

    cfg = TrainConfig.default_values()
    cfg.training_method = "LORA"
    cfg.lora_rank = args.rank
    cfg.dropout_probability = p
    cfg.batch_size = args.batch
    cfg.learning_rate = 3e-4
    cfg.learning_rate_warmup_steps = 0
    cfg.resolution = str(args.res)
    tr = GenericTrainer(cfg)
    tr.start()
    dev = tr.device
    assert tr.model.unet_lora.dropout_p == p
    buckets = AspectBucketing(args.res, 64, ASPECTS[:4]).resolutions
    arb = {r: synthetic_sdxl_batch(args.batch, r[0], r[1], dev, seed=0) for r in buckets}
    order = [random.Random(1000 + i).choice(buckets) for i in range(args.warmup + args.steps + 1)]
    for r in buckets:
        tr.train_step(arb[r])
    for i in range(args.warmup):
        tr.train_step(arb[order[i]])
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    f0, d0 = K.lora_fused_counts(), K.lora_dgrad_fused_counts()
    stream = torch.cuda.current_stream()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    evs[0].record(stream)
    losses = []
    for i in range(args.steps):
        losses.append(tr.train_step(arb[order[args.warmup + i]]))
        evs[i + 1].record(stream)
    torch.cuda.synchronize()
    gc.enable()
    f1, d1 = K.lora_fused_counts(), K.lora_dgrad_fused_counts()
    ms = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(args.steps))
    out = {"p": p, "step_ms_p50": round(ms[len(ms) // 2], 2), "step_ms_min": round(ms[0], 2),
           "step_ms_max": round(ms[-1], 2), "loss": torch.stack(losses).float().mean().item(),
           "sites": len(tr.model.unet_lora.sites),
           "fused_forwards_per_step": (f1[0] - f0[0]) / args.steps,
           "fused_input_grads_per_step": (d1[0] - d0[0]) / args.steps,
           "max_mem_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)}
    del tr, arb
    gc.collect()
    torch.cuda.empty_cache()
    return out


INNER = 20   # launches per timed window (back to back on one stream: the window is the kernels, not one enqueue)


def kernel_times(args, dev):
    from onetrainer_amd import kernels as K
    seed = torch.zeros(1, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream()
    out = {}
    for name, shape in (("stream", (1 << 20, 128)), ("step_t", (args.batch * (args.res // 8) ** 2, args.rank))):
        t = torch.ones(shape, dtype=torch.bfloat16, device=dev)
        K.lora_dropout(t, seed, 1, 0, args.p)
        times = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t.fill_(1)
            torch.cuda.synchronize()
            a.record(stream)
            for _ in range(INNER):
                K.lora_dropout(t, seed, 1, 0, args.p)
            b.record(stream)
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) / INNER)
        ms = sorted(times)[len(times) // 2]
        out[name] = {"shape": list(shape), "ms": round(ms, 4), "GBps": round(4 * t.numel() / ms / 1e6, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--p", type=float, default=0.1)
    args = ap.parse_args()
    off = step_times(args, 0.0)
    on = step_times(args, args.p)
    kern = kernel_times(args, torch.device("cuda", torch.cuda.current_device()))
    print(json.dumps({
        "workload": f"SDXL LoRA rank {args.rank} train step {args.res}^2 b={args.batch}, aspect-ratio buckets, "
                    f"dropout_probability 0 and {args.p}",
        "steps": args.steps, "dropout_off": off, "dropout_on": on,
        "step_ms_p50_ratio": round(on["step_ms_p50"] / off["step_ms_p50"], 4), "kernel": kern}))


if __name__ == "__main__":
    main()
