"""Time step() of the fused 8-bit AdamW (csrc/adamw8bit.hip) against the fused fp32-state AdamW (csrc/adamw.hip, which
the 8-bit optimizer leaves untouched) on one flat store of a given size and form, in one process, alternating the two,
and print the achieved GB/s against the traffic the kernel headers state.  Device events around `inner` back-to-back
steps, `reps` repeats after a warm-up; the median per step with its minimum and maximum, and the device's current
shader and memory clocks as torch reports them.  One JSON line per row.

usage: python tools/adamw8bit_probe.py [--n 2567463684] [--form f32|master|bf16] [--reps 7] [--inner 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from onetrainer_amd.module.param_store import FlatParamStore  # noqa: E402
from onetrainer_amd.util.optimizer.adamw8bit_fused import FusedAdamW8bit  # noqa: E402
from onetrainer_amd.util.optimizer.adamw_fused import FusedAdamW  # noqa: E402

# bytes per element, read + written.  8-bit: p, g and two codes in, p (and the working copy) and two codes out, plus
# 16 B of absmax per 256 elements; AdamW: p, g, m, v in, p, m, v out (bf16 store: bf16 moments)
ABSMAX = 16 / 256
TRAFFIC = {"f32": {"8bit": 8 + 2 + 4 + 2 + ABSMAX, "adamw": 16 + 12},
           "master": {"8bit": 6 + 2 + 6 + 2 + ABSMAX, "adamw": 14 + 14},
           "bf16": {"8bit": 4 + 2 + 2 + 2 + ABSMAX, "adamw": 8 + 6}}
TENSOR = 1 << 20   # elements of one tensor of the probe store
SDXL_UNET = 2567463684


def clocks():
    try:
        return {"sclk_mhz": torch.cuda.clock_rate(), "mclk_mhz": torch.cuda.memory_clock_rate() if hasattr(torch.cuda, "memory_clock_rate") else None}
    except Exception as e:   # the query needs amdsmi; the timing does not
        return {"clocks": f"not available ({type(e).__name__})"}


def window(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=SDXL_UNET)
    ap.add_argument("--form", choices=sorted(TRAFFIC), default="master")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nt = max(1, a.n // TENSOR)
    dtype = torch.float32 if a.form == "f32" else torch.bfloat16
    st = FlatParamStore([(f"t{i}", (1024, TENSOR // 1024), "a") for i in range(nt)], dtype, dev,
                        master=a.form == "master")
    n = st.numel
    chunk = 1 << 26
    for b in range(0, n, chunk):   # filled in pieces: no fp32 temporary of the whole store
        e = min(n, b + chunk)
        st.data[b:e].copy_(torch.randn(e - b, device=dev) * 0.05)
        st.grad[b:e].copy_(torch.randn(e - b, device=dev) * 1e-3)
        if st.master is not None:
            st.master[b:e].copy_(st.data[b:e])
    groups = [{"params": [st.params[name] for name in st.order]}]
    sr = a.form == "bf16"
    opts = {"8bit": FusedAdamW8bit(st, groups, lr=1e-5, stochastic_rounding=sr),
            "adamw": FusedAdamW(st, groups, lr=1e-5, stochastic_rounding=sr)}
    for _ in range(3):   # warm-up: code objects loaded, states non-zero
        for o in opts.values():
            o.step()
    torch.cuda.synchronize()
    before = clocks()
    ms = {k: [] for k in opts}
    for _ in range(a.reps):   # alternating, so that a drift of the machine meets both
        for k, o in opts.items():
            ms[k].append(window(o.step, a.inner))
    rows = []
    for k, v in ms.items():
        med = statistics.median(v)
        rows.append({"step": k, "form": a.form, "n": n, "tensors": nt, "ms_median": round(med, 4),
                     "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                     "bytes_per_element": round(TRAFFIC[a.form][k], 4),
                     "GB_s": round(TRAFFIC[a.form][k] * n / med / 1e6, 1), "clocks_before": before,
                     "clocks_after": clocks()})
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
