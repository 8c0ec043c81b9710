"""The host side of the validation pass (trainer.GenericTrainer.validate): what happens to the per-concept
(sum, count) pairs after the single device-to-host read.

The reference (modules/trainer/GenericTrainer.py:319-389) adds loss.item() of every held-out image into a dict keyed
by the concept's seed and writes `loss/validation_step/<label>` = sum / count per seed, plus
`loss/validation_step/total_average` when more than one seed has samples.  Here the sums arrive per concept index
(csrc/validation.hip); concepts of one seed are merged in index order, which is the reference's keying.
"""
from __future__ import annotations

import torch

from ..dataLoader.create import validation_labels

TAG = "loss/validation_step/"


def gather_ranks(acc: torch.Tensor, world: int, group=None) -> torch.Tensor:
    """data parallel: one all-gather of every rank's acc [n, 2] (f64), summed in rank order -- every rank computes
    the same bits.  One process: acc itself."""
    if world <= 1:
        return acc
    import torch.distributed as dist
    parts = [torch.empty_like(acc) for _ in range(world)]
    dist.all_gather(parts, acc.contiguous(), group=group)
    total = parts[0].clone()
    for p in parts[1:]:
        total += p
    return total


def validation_scalars(acc, concepts: list[dict]) -> list[tuple[str, float]]:
    """acc: [n, 2] (sum, count) per concept index, as nested lists or a host tensor; concepts: {name, path, seed}
    per index.  -> [(tag, value)] in the reference's order: one mean per seed that has samples (seeds in the order
    of their first concept), then the total average when more than one seed has samples.  All in float64, a seed's
    concepts added in index order."""
    rows = acc.tolist() if torch.is_tensor(acc) else acc
    labels = validation_labels(concepts)
    sums: dict = {}
    counts: dict = {}
    label_of: dict = {}
    for (s, n), c, label in zip(rows, concepts, labels):
        if n <= 0:
            continue
        seed = c["seed"]
        sums[seed] = sums.get(seed, 0) + float(s)
        counts[seed] = counts.get(seed, 0) + int(n)
        label_of.setdefault(seed, label)
    out = [(TAG + label_of[seed], sums[seed] / counts[seed]) for seed in sums]
    if len(counts) > 1:
        out.append((TAG + "total_average", sum(sums[k] for k in counts) / sum(counts[k] for k in counts)))
    return out
