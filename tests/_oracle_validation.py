"""NumPy / plain-Python restatement of the validation pass's arithmetic, independent of the code under test:
the device accumulate (csrc/validation.hip) as a sequential float64 sum, and the scalar writer
(modules/trainer/GenericTrainer.py:353-389 of the reference: sums keyed by concept seed, label collisions, the total
average)."""
import os

import numpy as np


def accumulate(acc: np.ndarray, losses, concept_index) -> np.ndarray:
    """acc f64 [n, 2] (sum, count) += the batch, sample by sample in ascending b; an index outside [0, n) is
    skipped.  Returns acc (updated in place)."""
    assert acc.dtype == np.float64
    n = acc.shape[0]
    for loss, c in zip(np.asarray(losses, dtype=np.float32), np.asarray(concept_index)):
        if 0 <= int(c) < n:
            acc[int(c), 0] = acc[int(c), 0] + np.float64(loss)
            acc[int(c), 1] = acc[int(c), 1] + np.float64(1.0)
    return acc


def scalars(acc, concepts) -> list:
    """the reference's writer over per-concept sums: walk the concepts in index order as its loop walks the samples,
    keyed by seed"""
    accumulated, counts, seed_to_label, label_to_seed = {}, {}, {}, {}
    for (s, n), c in zip(acc, concepts):
        seed = c["seed"]
        label = c["name"] if c["name"] else os.path.basename(c["path"])
        if label in label_to_seed and label_to_seed[label] != seed:
            suffix = 1
            new_label = f"{label}({suffix})"
            while new_label in label_to_seed and label_to_seed[new_label] != seed:
                suffix += 1
                new_label = f"{label}({suffix})"
            label = new_label
        if seed not in seed_to_label:
            seed_to_label[seed] = label
            label_to_seed[label] = seed
        if n > 0:
            accumulated[seed] = accumulated.get(seed, 0) + float(s)
            counts[seed] = counts.get(seed, 0) + int(n)
    out = [(f"loss/validation_step/{seed_to_label[seed]}", total / counts[seed])
           for seed, total in accumulated.items()]
    if len(counts) > 1:
        out.append(("loss/validation_step/total_average",
                    sum(accumulated[k] for k in counts) / sum(counts[k] for k in counts)))
    return out
