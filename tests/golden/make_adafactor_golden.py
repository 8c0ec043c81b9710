"""Generate tests/golden/adafactor_steps.npz by running the REFERENCE's own Adafactor (container only).

    python tests/golden/make_adafactor_golden.py          # needs /root/reference (read-only) and transformers

Runs transformers.Adafactor patched by the reference's patch_adafactor (modules/util/optimizer/
adafactor_extensions.py, built as modules/util/create.py:914-936 builds it) on the CPU for STEPS steps over the shapes
and configurations of tests/_oracle_adafactor.py, once with fp32 and once with bf16 parameters (the bf16 run is the
reference's round-to-nearest result: its stochastic_rounding flag has no effect, adafactor_extensions.py:92-95).
Inputs come from tests/_oracle_adafactor.py (hashed values, not stored); the outputs are recorded as data only:
per step and tensor the second-moment states in full (they depend on the gradients alone, so once for all
configurations) and per configuration, dtype, step and tensor rms(p) and the parameters (at most SAMPLE evenly strided
elements of a tensor, to keep the file small).  Nothing of the reference's source is stored.

Measured when this file was generated (printed by this script): the share of bf16 parameter elements that an fp32
summation order moves by one bf16 ulp, oracle with fp32 (NumPy pairwise) sums against the oracle with float64 sums,
over all configurations, steps and tensors: 1 of 3,947,196 elements, 2.5e-7 (cap in the tests: 1e-3).
"""
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))
sys.path.insert(0, str(HERE.parent))
REF = Path("/root/reference")

import _oracle_adafactor as AF  # noqa: E402
from oracle import adamw as OA  # noqa: E402


def reference_run(cfg, dtype):
    sys.path.insert(0, str(REF))
    from transformers.optimization import Adafactor

    from modules.util.optimizer.adafactor_extensions import patch_adafactor
    params = [torch.nn.Parameter(torch.from_numpy(AF.param0(n, s)).to(dtype)) for n, s in AF.SHAPES]
    opt = Adafactor(params, lr=cfg["lr"], eps=(1e-30, 1e-3), clip_threshold=cfg["clip_threshold"], decay_rate=-0.8,
                    beta1=None, weight_decay=cfg["weight_decay"], scale_parameter=cfg["scale_parameter"],
                    relative_step=False, warmup_init=False)
    patch_adafactor(opt, False)
    out = []
    for k in range(AF.STEPS):
        for p, (n, s) in zip(params, AF.SHAPES):
            p.grad = torch.from_numpy(AF.grad(n, s, k)).to(dtype)
        opt.step()
        rec = {}
        for p, (n, s) in zip(params, AF.SHAPES):
            st = opt.state[p]
            rec[n] = {"p": p.detach().clone(), "rms": float(st["RMS"]),
                      **{k2: st[k2].clone().numpy() for k2 in ("exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq")
                         if k2 in st}}
        out.append(rec)
    return out


def sr_order_share():
    """oracle with fp32-ordered sums against the oracle with float64 sums: bf16 elements that differ"""
    diff = total = 0
    for cfg in AF.CONFIGS.values():
        for n, s in AF.SHAPES:
            p = {dt: AF.param0(n, s) for dt in (np.float32, np.float64)}
            st = {dt: AF.new_state(s) for dt in p}
            for k in range(AF.STEPS):
                bits = {}
                for dt in p:
                    x, _ = AF.adafactor_step(p[dt], AF.grad(n, s, k), st[dt], k + 1, sum_dtype=dt, **cfg)
                    bits[dt] = OA.f32_to_bf16_bits(x)
                p = {dt: OA.bf16_to_f32(bits[np.float64]) for dt in p}   # each step from the same parameters
                d = AF.bf16_ulps(bits[np.float32], bits[np.float64])
                assert d.max() <= 1
                diff += int((d != 0).sum())
                total += d.size
    return diff, total


def main():
    rec = {}
    for cname, cfg in AF.CONFIGS.items():
        for dname, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16)):
            for k, step in enumerate(reference_run(cfg, dtype)):
                for n, r in step.items():
                    key = f"{cname}/{dname}/{k}/{n}/"
                    if dtype == torch.float32:
                        rec[key + "p"] = AF.sample(r["p"].numpy())
                    else:
                        rec[key + "p"] = AF.sample(r["p"].view(torch.int16).numpy().astype(np.uint16))
                    rec[key + "rms"] = np.float32(r["rms"])
                    for k2 in ("exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq"):
                        if k2 in r:   # functions of the gradients alone: the same in every configuration and dtype
                            prev = rec.setdefault(f"state/{k}/{n}/{k2}", r[k2])
                            assert np.array_equal(prev, r[k2])
    out = HERE / "adafactor_steps.npz"
    np.savez_compressed(out, **rec)
    print("wrote", out, len(rec), "arrays", out.stat().st_size, "bytes")
    d, t = sr_order_share()
    print(f"fp32-ordered sums against float64 sums: {d} of {t} bf16 elements differ ({d / t:.2e})")


if __name__ == "__main__":
    main()
