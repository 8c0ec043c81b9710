"""The discrete timestep distributions COS_MAP and SIGMOID (ModelSetupNoiseMixin.py:119-153) as a table.

The reference builds a weight per timestep bucket and draws with torch.multinomial.  Here the host builds the
weights in float64, folds them into an fp32 cumulative table once per argument set, and the timestep kernel draws
by inverse CDF from its own Philox uniform (csrc/diffusion.hip, otamd_timesteps_ex dist 3): the first bucket whose
cumulative value exceeds u.  DESIGN.md ("Timestep distributions") states the two departures from the reference
(table cache per argument set, inverse CDF instead of torch.multinomial) and the probability error bound.
"""
from __future__ import annotations

import math

import numpy as np
import torch

TABLE_DISTS = ("COS_MAP", "SIGMOID")


def timestep_weights(dist: str, num_train_timesteps: int, min_t: int, max_t: int, shift: float, bias: float,
                     weight: float) -> np.ndarray:
    """float64 weights of the max_t - min_t buckets, unnormalised, by the reference's formulas: the linspace with
    the inverse shift applied, times the derivative of the inverse shift over the unshifted linspace (:126-130);
    COS_MAP :136-137; SIGMOID :144-149, which applies the inverse shift a second time to the shifted linspace (kept
    as the reference has it).  bias / weight = noising_bias / noising_weight, read by SIGMOID only."""
    if dist not in TABLE_DISTS:
        raise ValueError(f"timestep distribution {dist!r} has no weight table")
    T = int(max_t) - int(min_t)
    if T <= 0:
        raise ValueError(f"timestep distribution {dist}: min_noising_strength and max_noising_strength leave "
                         f"{T} timesteps of {num_train_timesteps} (min {min_t}, max {max_t}); it needs at least one")
    shift, bias, weight = float(shift), float(bias), float(weight)
    lin = np.linspace(0.0, 1.0, T, dtype=np.float64)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        x = lin / (shift - shift * lin + lin)
        derivative = shift / (shift + lin - lin * shift) ** 2.0
        if dist == "COS_MAP":
            w = 2.0 / (math.pi - 2.0 * math.pi * x + 2.0 * math.pi * x ** 2.0)
        else:
            y = x / (shift - shift * x + x)
            w = 1.0 / (1.0 + np.exp(-weight * (y - (bias + 0.5))))
        w = w * derivative
    if not np.isfinite(w).all() or (w < 0).any() or not (w > 0).any():
        raise ValueError(f"timestep distribution {dist}: the bucket weights are not finite, negative or all zero "
                         f"(timestep_shift {shift}, noising_bias {bias}, noising_weight {weight})")
    return w


def timestep_cdf(weights: np.ndarray) -> np.ndarray:
    """fp32 cumulative table of the weights: a float64 running sum over its total, rounded to fp32 once; the entries
    from the last bucket of positive weight onward (the last entry among them) are exactly 1.0.  Non-decreasing, and
    a bucket of weight 0 repeats its predecessor's value (the first one holds 0), so the strict lookup skips it."""
    w = np.asarray(weights, dtype=np.float64)
    if w.ndim != 1 or w.size == 0 or not np.isfinite(w).all() or (w < 0).any() or not (w > 0).any():
        raise ValueError("timestep_cdf: the weights must be a non-empty vector of finite values >= 0, one > 0")
    c = np.cumsum(w)
    cdf = (c / c[-1]).astype(np.float32)
    cdf[np.flatnonzero(w > 0)[-1]:] = 1.0
    return cdf


class TimestepTables:
    """The cumulative tables a setup has used, on the device, by (distribution, N, min_t, max_t, shift, noising_bias,
    noising_weight): the arguments decide the table, so a dynamic shift gets one table per resolution (the reference
    keeps its first table for good).  Entries are never dropped: the setup holds the tensors the kernel reads for as
    long as it lives, and their number is bounded by the number of resolution buckets."""

    def __init__(self):
        self.tables: dict = {}

    def cdf(self, dist: str, num_train_timesteps: int, min_t: int, max_t: int, shift: float, bias: float,
            weight: float, device) -> torch.Tensor:
        key = (dist, int(num_train_timesteps), int(min_t), int(max_t), float(shift), float(bias), float(weight),
               str(device))
        t = self.tables.get(key)
        if t is None:
            if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("timestep table built inside a stream capture: draw the step inputs outside it")
            table = timestep_cdf(timestep_weights(*key[:-1]))
            t = self.tables[key] = torch.from_numpy(table).to(device)
        return t
