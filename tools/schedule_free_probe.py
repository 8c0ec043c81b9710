"""Time the fused schedule-free AdamW step (csrc/schedule_free.hip) and one eval() + train() pair on a flat store of a
given size and form, and print the achieved GB/s against the traffic the kernel header states; the yardstick is the
fused AdamW update on the same store in the same process (equal bytes on the fp32 and master forms).  Device events
around `inner` back-to-back launches, `reps` repeats after a warm-up; the median per launch with its minimum and
maximum.  One JSON line per row.

usage: python tools/schedule_free_probe.py [--n 25165824] [--form f32|master|bf16] [--reps 15] [--inner 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from onetrainer_amd.module.param_store import FlatParamStore  # noqa: E402
from onetrainer_amd.util.optimizer.adamw_fused import FusedAdamW  # noqa: E402
from onetrainer_amd.util.optimizer.schedule_free_fused import FusedScheduleFreeAdamW  # noqa: E402

# bytes per element, read + written, as the header of csrc/schedule_free.hip counts them (and adamw.hip for AdamW);
# swap: the lerp kernel of eval() alone (read p, z; write p and, with a master, the working copy)
TRAFFIC = {"f32": {"step": 16 + 12, "adamw": 16 + 12, "swap": 8 + 4},
           "master": {"step": 14 + 14, "adamw": 14 + 14, "swap": 8 + 6},
           "bf16": {"step": 12 + 10, "adamw": 8 + 6, "swap": 6 + 2}}
TENSOR = 1 << 20   # elements of one tensor of the probe store


def timed(fn, reps, inner):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=24 << 20)
    ap.add_argument("--form", choices=sorted(TRAFFIC), default="f32")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nt = max(1, a.n // TENSOR)
    dtype = torch.float32 if a.form == "f32" else torch.bfloat16
    st = FlatParamStore([(f"t{i}", (1024, TENSOR // 1024), "a") for i in range(nt)], dtype, dev,
                        master=a.form == "master")
    n = st.numel
    st.data.copy_(torch.randn(n, device=dev) * 0.05)
    if st.master is not None:
        st.master.copy_(st.data)
    st.grad.copy_(torch.randn(n, device=dev) * 1e-3)
    groups = [{"params": [st.params[name] for name in st.order]}]
    opt = FusedScheduleFreeAdamW(st, groups, lr=1e-4, stochastic_rounding=a.form == "bf16")
    opt.train()
    opt.step()   # z taken, states non-zero

    def row(name, t, key=None):
        med, lo, hi = t
        r = {"launch": name, "form": a.form, "n": n, "ms_median": round(med, 4), "ms_min": round(lo, 4),
             "ms_max": round(hi, 4)}
        if key:
            r["bytes_per_element"] = TRAFFIC[a.form][key]
            r["GB_s"] = round(TRAFFIC[a.form][key] * n / med / 1e6, 1)
        return r

    def pair():
        opt.eval()
        opt.train()

    def lerps():   # the two lerp launches alone: train() without the kept bits of y
        opt.eval()
        opt._y_saved = None
        opt.train()

    rows = [row("schedule-free step", timed(opt.step, a.reps, a.inner), "step"),
            row("eval() + train() (clone of y, lerp, copy back)", timed(pair, a.reps, max(1, a.inner // 2)))]
    med, lo, hi = timed(lerps, a.reps, max(1, a.inner // 2))
    r = row("eval() + train() by two lerps (clone of y, two swap launches)", (med, lo, hi))
    rows.append(r)
    del opt
    adamw = FusedAdamW(st, groups, lr=1e-4, stochastic_rounding=a.form == "bf16")
    rows.append(row("adamw step (yardstick)", timed(adamw.step, a.reps, a.inner), "adamw"))
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
