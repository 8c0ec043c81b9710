"""Generate tests/golden/came_steps.npz by running the REFERENCE's own CAME (container only).

    python tests/golden/make_came_golden.py          # needs /root/reference (read-only)

Runs the reference's CAME (modules/util/optimizer/CAME.py, built as modules/util/create.py:938-951 builds it) on the
CPU for STEPS steps over the shapes of tests/_oracle_adafactor.py and the configurations of tests/_oracle_came.py,
once with fp32 and once with bf16 parameters, stochastic_rounding=False.  Inputs come from the oracles (hashed values,
not stored); the outputs are recorded as data only: per configuration, step and tensor the factored states
and the first moment (they depend on the gradients alone, so once for both dtypes), and per dtype the parameters;
every array as at most CM.SAMPLE evenly strided elements (CAME records five states where Adafactor records two, so
the stride is wider than AF.sample's to keep the file the size of adafactor_steps.npz).  Nothing
of the reference's source is stored.

Measured when this file was generated (printed by this script): the share of bf16 parameter elements that an fp32
summation order moves by one bf16 ulp, oracle with fp32 (NumPy pairwise) sums against the oracle with float64 sums,
over all configurations, steps and tensors: 6 of 4,933,995 elements, 1.2e-6 (cap in the tests: 1e-3).
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
import _oracle_came as CM  # noqa: E402
from oracle import adamw as OA  # noqa: E402

STATES = ("exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq", "exp_avg_res_row", "exp_avg_res_col")


def reference_run(cname, cfg, dtype):
    sys.path.insert(0, str(REF))
    from modules.util.optimizer.CAME import CAME
    params = [torch.nn.Parameter(torch.from_numpy(AF.param0(n, s)).to(dtype)) for n, s in AF.SHAPES]
    opt = CAME(params, lr=cfg["lr"], eps=(1e-30, 1e-16), clip_threshold=cfg["clip_threshold"], betas=cfg["betas"],
               weight_decay=cfg["weight_decay"], stochastic_rounding=False)
    out = []
    for k in range(AF.STEPS):
        for p, (n, s) in zip(params, AF.SHAPES):
            p.grad = torch.from_numpy(CM.grad(cname, n, s, k)).to(dtype)
            assert torch.equal(p.grad.float(), torch.from_numpy(CM.grad(cname, n, s, k)))   # bf16-exact inputs
        opt.step()
        rec = {}
        for p, (n, s) in zip(params, AF.SHAPES):
            st = opt.state[p]
            assert st["exp_avg"].dtype == torch.float32
            rec[n] = {"p": p.detach().clone(), "exp_avg": st["exp_avg"].clone().numpy(),
                      **{k2: st[k2].clone().numpy() for k2 in STATES if k2 in st}}
        out.append(rec)
    return out


def sr_order_share():
    """oracle with fp32-ordered sums against the oracle with float64 sums: bf16 elements that differ"""
    diff = total = 0
    for cname, cfg in CM.CONFIGS.items():
        for n, s in AF.SHAPES:
            p = AF.param0(n, s)
            st = {dt: CM.new_state(s) for dt in (np.float32, np.float64)}
            for k in range(AF.STEPS):
                bits = {dt: OA.f32_to_bf16_bits(CM.came_step(p, CM.grad(cname, n, s, k), st[dt], bf16=True,
                                                             sum_dtype=dt, **cfg)[0]) for dt in st}
                p = OA.bf16_to_f32(bits[np.float64])   # each step from the same parameters
                d = AF.bf16_ulps(bits[np.float32], bits[np.float64])
                assert d.max() <= 1
                diff += int((d != 0).sum())
                total += d.size
    return diff, total


def main():
    rec = {}
    for cname, cfg in CM.CONFIGS.items():
        for dname, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16)):
            for k, step in enumerate(reference_run(cname, cfg, dtype)):
                for n, r in step.items():
                    if dtype == torch.float32:
                        rec[f"{cname}/f32/{k}/{n}/p"] = CM.sample(r["p"].numpy())
                    else:
                        rec[f"{cname}/bf16/{k}/{n}/p"] = CM.sample(r["p"].view(torch.int16).numpy().astype(np.uint16))
                    for k2 in STATES + ("exp_avg",):
                        if k2 in r:   # functions of the gradients alone: the same for both dtypes
                            val = CM.sample(r[k2])
                            prev = rec.setdefault(f"{cname}/state/{k}/{n}/{k2}", val)
                            assert np.array_equal(prev, val)
    out = HERE / "came_steps.npz"
    np.savez_compressed(out, **rec)
    print("wrote", out, len(rec), "arrays", out.stat().st_size, "bytes")
    d, t = sr_order_share()
    print(f"fp32-ordered sums against float64 sums: {d} of {t} bf16 elements differ ({d / t:.2e})")


if __name__ == "__main__":
    main()
