"""Golden fixture from the reference's own timestep samplers (container only).

    python tests/golden/make_timestep_golden.py      -> tests/golden/timestep_dists.npz

Runs ModelSetupNoiseMixin._get_timestep_discrete (modules/modelSetup/mixin/ModelSetupNoiseMixin.py:51-155), imported
directly, on the CPU:
  * COS_MAP and SIGMOID at (N 1000, strengths 0..1, shift 1), (N 1000, 0.1..0.9, shift 3) and (N 10, 0..1, shift 0.5),
    SIGMOID with noising_weight in {0, 10, -10} and noising_bias in {0, 0.3}: per case a fresh mixin object, its fp32
    weight table (the name-mangled cache the first call fills) and 64 sampled timesteps;
  * HEAVY_TAIL at noising_weight in {0, 0.5, 1} and shift in {1, 3}: the 256 uniforms (re-drawn from an identically
    seeded generator) and the reference's int timesteps.  The share of draws whose float64 value lies inside the fp32
    error band of an integer (tests/_timestep_ref.py) is checked against the 2 % cap the tests hold, with the
    reference's own outputs; a seed that misses it is replaced by the next one.
Only data is stored: `<case>/cfg` = [N, min_noising_strength, max_noising_strength, timestep_shift, noising_bias,
noising_weight] (float64), `<case>/weights`, `<case>/t`, `<case>/u`.  No reference source.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference")
OUT = HERE / "timestep_dists.npz"
GEOMETRIES = [(1000, 0.0, 1.0, 1.0), (1000, 0.1, 0.9, 3.0), (10, 0.0, 1.0, 0.5)]   # N, min, max strength, shift
SIGMOID_WEIGHTS, SIGMOID_BIASES = (0.0, 10.0, -10.0), (0.0, 0.3)
HEAVY_WEIGHTS, HEAVY_SHIFTS = (0.0, 0.5, 1.0), (1.0, 3.0)
N_TABLE_DRAWS, N_HEAVY_DRAWS, HEAVY_CAP = 64, 256, 0.02


def table_cases():
    """(name, distribution, N, min strength, max strength, shift, bias, weight)"""
    for gi, (N, mn, mx, shift) in enumerate(GEOMETRIES):
        yield f"cos_map/g{gi}", "COS_MAP", N, mn, mx, shift, 0.0, 0.0
        for w in SIGMOID_WEIGHTS:
            for b in SIGMOID_BIASES:
                yield f"sigmoid/g{gi}_w{w:g}_b{b:g}", "SIGMOID", N, mn, mx, shift, b, w


def heavy_cases():
    for w in HEAVY_WEIGHTS:
        for shift in HEAVY_SHIFTS:
            yield f"heavy_tail/w{w:g}_s{shift:g}", 1000, 0.0, 1.0, shift, 0.0, w


def main():
    sys.path.insert(0, str(REF))
    sys.path.insert(0, str(HERE.parent))
    import _timestep_ref as R
    from modules.modelSetup.mixin.ModelSetupNoiseMixin import ModelSetupNoiseMixin
    from modules.util.config.TrainConfig import TrainConfig
    from modules.util.enum.TimestepDistribution import TimestepDistribution

    class Probe(ModelSetupNoiseMixin):
        pass

    def config(dist, mn, mx, shift, bias, weight):
        c = TrainConfig.default_values()
        c.train_device = "cpu"
        c.timestep_distribution = TimestepDistribution[dist]
        c.min_noising_strength, c.max_noising_strength = mn, mx
        c.timestep_shift, c.noising_bias, c.noising_weight = shift, bias, weight
        return c

    rec = {}
    for name, dist, N, mn, mx, shift, bias, weight in table_cases():
        p = Probe()
        g = torch.Generator(device="cpu").manual_seed(42)
        t = p._get_timestep_discrete(N, False, g, N_TABLE_DRAWS, config(dist, mn, mx, shift, bias, weight))
        w = p._ModelSetupNoiseMixin__weights
        assert w.dtype == torch.float32 and w.numel() == int(N * mx) - int(N * mn)
        rec[f"{name}/cfg"] = np.array([N, mn, mx, shift, bias, weight], dtype=np.float64)
        rec[f"{name}/weights"] = w.numpy().copy()
        rec[f"{name}/t"] = t.numpy().copy()
    for name, N, mn, mx, shift, bias, weight in heavy_cases():
        c = config("HEAVY_TAIL", mn, mx, shift, bias, weight)
        for seed in range(42, 52):
            t = Probe()._get_timestep_discrete(N, False, torch.Generator(device="cpu").manual_seed(seed),
                                               N_HEAVY_DRAWS, c).numpy()
            u = torch.rand(size=(N_HEAVY_DRAWS,), generator=torch.Generator(device="cpu").manual_seed(seed)).numpy()
            want, decided = R.heavy_tail_decided(u, N, int(N * mn), int(N * mx), shift, weight)
            assert (t[decided] == want[decided]).all(), name
            left_out = 1.0 - decided.mean()
            print(name, "seed", seed, "left out", left_out)
            if left_out <= HEAVY_CAP:
                break
        else:
            raise RuntimeError(f"{name}: no seed within the cap")
        rec[f"{name}/cfg"] = np.array([N, mn, mx, shift, bias, weight], dtype=np.float64)
        rec[f"{name}/u"] = u.copy()
        rec[f"{name}/t"] = t.copy()
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, len(rec), "arrays")


if __name__ == "__main__":
    main()
