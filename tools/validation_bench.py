"""Time one validation pass over a synthetic SDXL held-out set (64 samples at 1024 x 1024, random weights) in two
forms.  Each part is its own process under its own time limit, chained so that trouble ends the chain:

    timeout -k 10 600 python tools/validation_bench.py --part batched && \\
    timeout -k 10 600 python tools/validation_bench.py --part batch1  && \\
    python tools/validation_bench.py --part ratio

Every part merges its figures into profiles/validation_bench.json (--out).  Parts:
  batched  GenericTrainer.validate: the set at the training batch size of the benchmark config (4), per-concept sums
           kept on the device (csrc/validation.hip), one device-to-host read after the last batch
  batch1   the reference's form (modules/trainer/GenericTrainer.py:342-356) from the same pieces: batch size 1,
           predict(deterministic=True) + calculate_loss under no_grad and loss.item() after every sample
  ratio    batch1 median / batched median, from the file (no GPU)
Both read the same latent cache from disk through the same loader (one batch prefetched on a host thread).  Times are
wall-clock medians of --reps passes after --warmup passes, each pass ended by its own host read (the batch1 form's
last .item(), the batched form's single read), so nothing is left queued when the clock stops.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def write_cache(cache_dir, n, size, concepts):
    import torch
    from safetensors.torch import save_file
    os.makedirs(cache_dir, exist_ok=True)
    g = torch.Generator().manual_seed(0)
    h = w = size // 8
    index = []
    for i in range(n):
        rec = {"latent_image": (torch.randn(h, w, 4, generator=g) / 0.13025).contiguous(),
               "original_resolution": torch.tensor([size, size]), "crop_offset": torch.tensor([0, 0]),
               "crop_resolution": torch.tensor([size, size]),
               "text_encoder_1_hidden_state": torch.randn(77, 768, generator=g).bfloat16(),
               "text_encoder_2_hidden_state": torch.randn(77, 1280, generator=g).bfloat16(),
               "text_encoder_2_pooled_state": torch.randn(1280, generator=g).bfloat16()}
        fn = f"{i:08d}.safetensors"
        save_file(rec, os.path.join(cache_dir, fn))
        index.append({"file": fn, "crop_resolution": [size, size], "concept_index": i % len(concepts)})
    with open(os.path.join(cache_dir, "index.json"), "w") as f:
        json.dump({"version": 1, "samples": index, "concepts": concepts}, f)


def merge(path, res):
    merged = {}
    if os.path.isfile(path):
        with open(path) as f:
            merged = json.load(f)
    merged.update(res)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(merged, f, indent=1, sort_keys=True)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["batched", "batch1", "ratio"])
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=4, help="the benchmark config's per-GPU batch (bench.py, sdxl)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="profiles/validation_bench.json")
    a = ap.parse_args()
    if a.part == "ratio":
        with open(a.out) as f:
            m = json.load(f)
        merge(a.out, {"batch1_over_batched": m["batch1_item_per_sample"]["median_s"] / m["batched_device_sums"]["median_s"]})
        return

    import torch

    from onetrainer_amd.dataLoader.latent_cache import LatentCacheDataLoader
    from onetrainer_amd.trainer.GenericTrainer import GenericTrainer
    from onetrainer_amd.util import create
    from onetrainer_amd.util.config.TrainConfig import TrainConfig
    dev = torch.device("cuda:0")
    concepts = [{"name": "a", "path": "/a", "seed": 1}, {"name": "b", "path": "/b", "seed": 2}]
    with tempfile.TemporaryDirectory() as tmp:
        cfg = TrainConfig.default_values()
        cfg.batch_size = a.batch
        cfg.resolution = str(a.size)
        cfg.workspace_dir, cfg.cache_dir = os.path.join(tmp, "ws"), os.path.join(tmp, "cache")
        cfg.sample_definition_file_name = os.path.join(tmp, "none.json")
        cfg.validation = True
        vdir = os.path.join(cfg.cache_dir, "validation")
        write_cache(vdir, a.samples, a.size, concepts)
        model = create.create_model(cfg, dev, seed=0)
        tr = GenericTrainer(cfg, model=model)   # no training data (no cache, no concepts): only validate() runs
        tr.start()
        setup, tp = tr.model_setup, model.train_progress

        def batched():
            return tr.validate()["scalars"]

        def batch1():
            ld = LatentCacheDataLoader(vdir, 1, dev, validation=True)
            ld.start_next_epoch()
            sums, counts = {}, {}
            for b in ld.get_data_loader():
                with torch.no_grad():
                    out = setup.predict(model, b, cfg, tp, deterministic=True)
                    loss = setup.calculate_loss(model, b, out, cfg)
                c = int(b["concept_index_host"][0])
                sums[c] = sums.get(c, 0) + loss.item()
                counts[c] = counts.get(c, 0) + 1
            return [sums[c] / counts[c] for c in sorted(sums)]

        fn = batched if a.part == "batched" else batch1
        for _ in range(a.warmup):
            fn()
        times = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            means = fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        key = "batched_device_sums" if a.part == "batched" else "batch1_item_per_sample"
        merge(a.out, {key: {"median_s": statistics.median(times), "min_s": min(times), "max_s": max(times),
                            "reps": a.reps, "samples": a.samples, "size": a.size,
                            "batch": a.batch if a.part == "batched" else 1,
                            "means": [m[1] if isinstance(m, tuple) else m for m in means]}})


if __name__ == "__main__":
    main()
