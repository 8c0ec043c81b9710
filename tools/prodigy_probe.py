"""Time the three launches of a fused Prodigy step (csrc/prodigy.hip: accumulate, finalize, apply) on a flat store of
a given size and form, and print the achieved GB/s against the traffic the kernel header states; for context the
fused AdamW update on the same store.  Device events around `inner` back-to-back launches, `reps` repeats after a
warm-up; the median per launch with its minimum and maximum.  One JSON line per launch.

usage: python tools/prodigy_probe.py [--n 25165824] [--form f32|master|bf16] [--reps 15] [--inner 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from onetrainer_amd import kernels as K  # noqa: E402
from onetrainer_amd.module.param_store import FlatParamStore  # noqa: E402
from onetrainer_amd.util.optimizer.adamw_fused import FusedAdamW  # noqa: E402
from onetrainer_amd.util.optimizer.prodigy_fused import FusedProdigy  # noqa: E402

# bytes per element, read + written, as the header of csrc/prodigy.hip counts them (and adamw.hip for AdamW)
TRAFFIC = {"f32": {"accumulate": 24 + 12, "apply": 12 + 4, "adamw": 16 + 12},
           "master": {"accumulate": 22 + 12, "apply": 12 + 6, "adamw": 14 + 14},
           "bf16": {"accumulate": 20 + 12, "apply": 10 + 2, "adamw": 8 + 6}}
TENSOR = 1 << 20   # elements of one tensor of the probe store (16 chunks)


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
    opt = FusedProdigy(st, groups, lr=1.0, stochastic_rounding=a.form == "bf16")
    opt.step()   # p0 captured, states non-zero
    h = opt._hyper(1.0)
    p = st.master if st.master is not None else st.data
    w = st.data if st.master is not None else None
    launches = {
        "accumulate": lambda: K.prodigy_accumulate(p, st.grad, w, opt.p0, opt.exp_avg, opt.exp_avg_sq, opt.s,
                                                   opt._chunks, opt._n_chunks, opt._chunk_num, opt._chunk_den,
                                                   opt._state, h),
        "finalize": lambda: K.prodigy_finalize(opt._chunk_num, opt._chunk_den, opt._n_chunks, opt._state, h),
        "apply": lambda: K.prodigy_apply(p, st.grad, w, opt.exp_avg, opt.exp_avg_sq, opt._state, h,
                                         stochastic_rounding=a.form == "bf16", seed=1),
    }
    rows = []
    for name, fn in launches.items():
        med, lo, hi = timed(fn, a.reps, a.inner)
        row = {"launch": name, "form": a.form, "n": n, "chunks": opt._n_chunks, "ms_median": round(med, 4),
               "ms_min": round(lo, 4), "ms_max": round(hi, 4)}
        if name in TRAFFIC[a.form]:
            row["bytes_per_element"] = TRAFFIC[a.form][name]
            row["GB_s"] = round(TRAFFIC[a.form][name] * n / med / 1e6, 1)
        rows.append(row)
    med, lo, hi = timed(opt.step, a.reps, a.inner)
    rows.append({"launch": "step (three launches and the d copy)", "form": a.form, "n": n, "ms_median": round(med, 4),
                 "ms_min": round(lo, 4), "ms_max": round(hi, 4)})
    del opt
    adamw = FusedAdamW(st, groups, lr=1e-4, stochastic_rounding=a.form == "bf16")
    med, lo, hi = timed(adamw.step, a.reps, a.inner)
    rows.append({"launch": "adamw step (context)", "form": a.form, "n": n, "ms_median": round(med, 4),
                 "ms_min": round(lo, 4), "ms_max": round(hi, 4), "bytes_per_element": TRAFFIC[a.form]["adamw"],
                 "GB_s": round(TRAFFIC[a.form]["adamw"] * n / med / 1e6, 1)})
    for row in rows:
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
