"""Generate tests/golden/ema_steps.npz by running the REFERENCE's own EMAModuleWrapper (needs a checkout of the
reference; nothing of its source is stored).

    python tests/golden/make_ema_golden.py <path to the reference checkout>

Runs modules/module/EMAModule.py's EMAModuleWrapper on the CPU over the shapes, schedules and hashed parameter
trajectories of tests/_oracle_ema.py, in three forms: fp32 parameters ("f32"), bf16 parameters ("bf16"), and bf16
parameters with the wrapper moved to fp32 by its own `to(device, dtype=torch.float32)` ("mixed").  The wrapper is
created from trajectory point 0 and its step s sees point s + 1, through the same-device update
`ema.add_(one_minus_decay * (parameter - ema))`.  Recorded, as data only: the shadow after every step, per schedule,
form, step and tensor (at most SAMPLE evenly strided elements of a tensor), fp32 values as such and bf16 values as
uint16 bit patterns.
"""
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))
sys.path.insert(0, str(HERE.parent))

import _oracle_ema as OE  # noqa: E402


def reference_run(form, sched):
    from modules.module.EMAModule import EMAModuleWrapper
    s = OE.SCHEDULES[sched]
    dtype = torch.bfloat16 if OE.params_are_bf16(form) else torch.float32
    cpu = torch.device("cpu")

    def point(k):
        return [torch.from_numpy(OE.param(n, sh, k, OE.params_are_bf16(form))).to(dtype) for n, sh in OE.SHAPES]

    params = [torch.nn.Parameter(t) for t in point(0)]
    ema = EMAModuleWrapper(params, decay=s["decay"], update_step_interval=s["interval"], device=cpu)
    if form == "mixed":
        ema.to(cpu, dtype=torch.float32)
    out = []
    for k in range(s["steps"]):
        for p, t in zip(params, point(k + 1)):
            p.data.copy_(t)
        ema.step(params, k)
        out.append([e.detach().clone() for e in ema.ema_parameters])
    return out


def main():
    sys.path.insert(0, str(Path(sys.argv[1]).resolve()))
    rec = {}
    for sched in OE.SCHEDULES:
        for form in OE.FORMS:
            for k, step in enumerate(reference_run(form, sched)):
                for (n, _), e in zip(OE.SHAPES, step):
                    if OE.shadow_is_bf16(form):
                        assert e.dtype == torch.bfloat16
                        v = e.view(torch.int16).numpy().astype(np.uint16)
                    else:
                        assert e.dtype == torch.float32
                        v = e.numpy()
                    rec[f"{sched}/{form}/{k}/{n}"] = OE.sample(v).copy()
    out = HERE / "ema_steps.npz"
    np.savez_compressed(out, **rec)
    print("wrote", out, len(rec), "arrays", out.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
