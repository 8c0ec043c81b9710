"""Time one step of the fused optimizers (AdamW, Adafactor, CAME) on the bf16 store of the SDXL UNet
(2,567,486,728 elements) in one process: HIP events around step(), 3 warm-up + 10 timed steps, p50 (min - max), and
the optimizer state each constructor allocates (torch.cuda.memory_allocated around it).  One JSON line per optimizer.

usage: python tools/optimizer_step_time.py [--only ADAFACTOR,CAME] [--steps 10] [--warmup 3] [--digest]
A kernel-trace run (rocprofv3 --kernel-trace --stats -- python tools/optimizer_step_time.py --only ADAFACTOR,CAME
--warmup 1 --steps 3) gives the per-kernel split of both in one trace.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from onetrainer_amd.module import unet as U  # noqa: E402
from onetrainer_amd.util.optimizer.adafactor_fused import FusedAdafactor  # noqa: E402
from onetrainer_amd.util.optimizer.adamw_fused import FusedAdamW  # noqa: E402
from onetrainer_amd.util.optimizer.came_fused import FusedCAME  # noqa: E402


def build(name, store, params):
    groups = [{"params": params}]
    if name == "ADAMW":
        return FusedAdamW(store, groups, lr=1e-5, stochastic_rounding=True)
    if name == "ADAFACTOR":
        return FusedAdafactor(store, groups, lr=1e-5, relative_step=False, scale_parameter=False,
                              stochastic_rounding=True)
    return FusedCAME(store, groups, lr=1e-5, stochastic_rounding=True)


def sha256(t, chunk=1 << 28):
    h = hashlib.sha256()
    flat = t.detach().view(-1).view(torch.uint8)
    for i in range(0, flat.numel(), chunk):
        h.update(flat[i:i + chunk].cpu().numpy().tobytes())
    return h.hexdigest()


def moved_bytes(name, opt, n):
    """bytes one step reads and writes: per parameter (bf16 store) plus the factored states and partials"""
    if name == "ADAMW":
        return 14 * n
    states = 4 * (opt.state_buf.numel() + opt._scratch.numel())
    if name == "ADAFACTOR":
        return 10 * n + 4 * states          # each state value: read + written by its EMA, read by unorm and apply
    return 22 * n + 2 * 4 * states          # two sets of states; m's 12 B are in the 22


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--digest", action="store_true", help="after the timed steps, a sha256 of the store and of each "
                    "state buffer per optimizer")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model = U.UNet2DConditionModel(U.sdxl_config(), dev, seed=None)
    store = model.store
    g = torch.Generator(device=dev).manual_seed(1)
    store.data.copy_((torch.randn(store.numel, generator=g, device=dev) * 0.05).to(store.dtype))
    store.grad.copy_((torch.randn(store.numel, generator=g, device=dev) * 1e-3).to(store.dtype))
    params = [store.params[n] for n in store.order]
    for name in ("ADAMW", "ADAFACTOR", "CAME"):
        if a.only and name not in a.only.split(","):
            continue
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        opt = build(name, store, params)
        torch.cuda.synchronize()
        state_bytes = torch.cuda.memory_allocated() - before
        for _ in range(a.warmup):
            opt.step()
        times = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            opt.step()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        p50 = statistics.median(times)
        nbytes = moved_bytes(name, opt, store.numel)
        print(json.dumps({"optimizer": name, "numel": store.numel, "tensors": len(store.order),
                          "ms_p50": round(p50, 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3),
                          "GB_step": round(nbytes / 1e9, 2), "TB_s": round(nbytes / p50 / 1e9, 3),
                          "state_GB": round(state_bytes / 1e9, 3)}), flush=True)
        if a.digest:   # compare outputs at the size that is timed (two library builds: equal digests)
            bufs = {"store.data": store.data}
            bufs.update({k: v for k, v in sorted(vars(opt).items())
                         if k in ("exp_avg", "exp_avg_sq", "state_buf", "res_buf")})
            torch.cuda.synchronize()
            for k, v in bufs.items():
                print(json.dumps({"optimizer": name, "buffer": k, "sha256": sha256(v)}), flush=True)
        del opt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
