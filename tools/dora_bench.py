"""Time a DoRA SDXL train step at the `bench.py --model sdxl-lora` shape, and the DoRA kernels on their own.

    python tools/dora_bench.py [--steps 8] [--warmup 3] [--rank 32] [--batch 4] [--res 1024] [--output-axis]

The workload is bench.py's sdxl-lora one (training_presets "#sdxl 1.0 LoRA" + rank 32, fp32 adapters, aspect-ratio
buckets drawn by the same seeds) with `lora_decompose` on, so its p50 compares with `bench.py --model sdxl-lora` and
`--model sdxl` run in the same session.  Then, on the trained state: the merge launch alone and the projection of
every site alone (hipEvents, median of `--reps`), with the bytes each must move at least (merge: W read twice and W'
written, 6 B per element; projection: G read twice and W once, 6 B per element) and the achieved GB/s.  Prints one
JSON line.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--output-axis", action="store_true")
    args = ap.parse_args()

    from onetrainer_amd.dataLoader.aspect_bucketing import ASPECTS, AspectBucketing
    from onetrainer_amd.dataLoader.SyntheticDataLoader import synthetic_sdxl_batch
    from onetrainer_amd.module import streams as S
    from onetrainer_amd.trainer.GenericTrainer import GenericTrainer
    from onetrainer_amd.util.config.TrainConfig import TrainConfig

    cfg = TrainConfig.default_values()
    cfg.training_method = "LORA"
    cfg.lora_rank = args.rank
    cfg.lora_decompose = True
    cfg.lora_decompose_output_axis = args.output_axis
    cfg.batch_size = args.batch
    cfg.learning_rate = 3e-4
    cfg.learning_rate_warmup_steps = 0
    cfg.resolution = str(args.res)
    tr = GenericTrainer(cfg)
    tr.start()
    dev = tr.device
    w = tr.model.unet_lora
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
    stream = torch.cuda.current_stream()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    evs[0].record(stream)
    losses = []
    for i in range(args.steps):
        losses.append(tr.train_step(arb[order[args.warmup + i]]))
        evs[i + 1].record(stream)
    torch.cuda.synchronize()
    gc.enable()
    step_ms = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(args.steps))
    loss = torch.stack(losses).float().mean().item()

    def timed(fn):
        out = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record(stream)
            fn()
            b.record(stream)
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b))
        return sorted(out)[len(out) // 2]

    def project_all():
        for s in w.sites:
            w.ref_for([g + ".weight" for g in s.group]).done()
        w.flush()
        S.join()

    elems = sum(e.out * e.kk * e.cin for e in w._host_table[:w._n_entries])
    merge_ms = timed(w.refresh)
    proj_ms = timed(project_all)
    print(json.dumps({
        "workload": f"SDXL DoRA rank {args.rank} train step {args.res}^2 b={args.batch}, aspect-ratio buckets, "
                    f"{'output' if args.output_axis else 'input'} axis",
        "step_ms_p50": round(step_ms[len(step_ms) // 2], 2), "step_ms_min": round(step_ms[0], 2),
        "step_ms_max": round(step_ms[-1], 2), "steps": args.steps, "loss": loss,
        "adapted_elements": elems, "modules": w._n_entries, "sites": len(w.sites),
        "merge_ms": round(merge_ms, 3), "merge_GBps": round(6 * elems / merge_ms / 1e6, 1),
        "project_ms": round(proj_ms, 3), "project_GBps": round(6 * elems / proj_ms / 1e6, 1),
        "dora_buffers_GiB": round((w.wp.numel() + w.g.numel()) * 2 / 2 ** 30, 2),
        "max_mem_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)}))


if __name__ == "__main__":
    main()
