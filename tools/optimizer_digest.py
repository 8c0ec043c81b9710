"""Bit digests of the fused Adafactor and CAME optimizers on a small seeded store, for comparing two builds or two
revisions byte for byte (same output = same bits in every parameter and state).  Only the optimizers' public API is
used (constructors, clip_grad_norm_, step, step_parameter, state_dict), so the tool runs unchanged on other revisions.

The store holds the ten shapes the optimizer tests use plus (2, 70, 70): a matrix that spans LDS stages with batch 2,
whose second matrix starts off the 8-element alignment (4900 mod 8 = 4).  Cases: bf16 / bf16 with stochastic rounding
/ fp32 / fp32 master, global clip on / off, scale_parameter on / off (Adafactor), two parameter groups; three store
steps, then one step_parameter call on an unfactored, a packed and a big tensor.  One line per case, stage, and
state-dict key or store buffer: case, name, sha256.

usage: python tools/optimizer_digest.py > digest.txt        (OTAMD_LIB_ALT=<name> selects another library build)
"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from onetrainer_amd.module.param_store import FlatParamStore  # noqa: E402
from onetrainer_amd.util.optimizer.adafactor_fused import FusedAdafactor  # noqa: E402
from onetrainer_amd.util.optimizer.came_fused import FusedCAME  # noqa: E402

SHAPES = [("m64x70", (64, 70)), ("m300x1030", (300, 1030)), ("m2049x3", (2049, 3)), ("m1x513", (1, 513)),
          ("conv3", (3, 5, 3, 3)), ("conv1", (8, 4, 1, 1)), ("v37", (37,)), ("v5", (5,)), ("m2x4100", (2, 4100)),
          ("zero", (16, 24)), ("b2x70x70", (2, 70, 70))]
SPLIT = 5                                      # SHAPES[:SPLIT] -> group 0, the rest -> group 1
LRS = (3e-3, 1e-3)
STEPS = 3
STEP_PARAMETER = ("v37", "conv3", "b2x70x70")  # mode 0, mode 1, mode 2


def values(seed, shape, scale):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32) * scale


def param0(i, shape):
    x = values(100 + i, shape, 1.0)
    return torch.where(x < 0, -1.0, 1.0) * (0.02 + 0.03 * x.abs().clamp(max=1.0))


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def report(case, stage, st, opt):
    torch.cuda.synchronize()
    sd = opt.state_dict()
    print(case, f"{stage}.sr_seed", sd["sr_seed"])
    for idx in sorted(sd["state"]):
        for key, v in sorted(sd["state"][idx].items()):
            print(case, f"{stage}.state.{idx}.{key}", sha(v) if torch.is_tensor(v) and v.dim() else float(v))
    print(case, f"{stage}.store.data", sha(st.data))
    if st.master is not None:
        print(case, f"{stage}.store.master", sha(st.master))
    sys.stdout.flush()


def run(dev, kind, form, clip, scale):
    dtype = torch.float32 if form == "f32" else torch.bfloat16
    st = FlatParamStore([(n, s, "a" if i < SPLIT else "b") for i, (n, s) in enumerate(SHAPES)], dtype, dev,
                        master=form == "master")
    for i, (n, s) in enumerate(SHAPES):
        st.write(n, param0(i, s))
    groups = [{"params": [st.params[n] for n, _ in SHAPES[:SPLIT]], "lr": LRS[0]},
              {"params": [st.params[n] for n, _ in SHAPES[SPLIT:]], "lr": LRS[1]}]
    sr = form == "bf16_sr"
    if kind == "adafactor":
        opt = FusedAdafactor(st, groups, lr=LRS[0], relative_step=False, scale_parameter=scale, weight_decay=0.01,
                             stochastic_rounding=sr, seed=11)
    else:
        opt = FusedCAME(st, groups, lr=LRS[0], weight_decay=0.01, stochastic_rounding=sr, seed=11)
    case = f"{kind}/{form}/clip{int(clip)}" + (f"/scale{int(scale)}" if kind == "adafactor" else "")

    def set_grads(k):
        for i, (n, s) in enumerate(SHAPES):
            g = torch.zeros(s) if n == "zero" else values(1000 + 31 * k + i, s, 3.0 * 10.0 ** (-2 + min(k, 2)))
            st.params[n].grad.copy_(g)

    for k in range(STEPS):
        set_grads(k)
        if clip:
            opt.clip_grad_norm_(1.0)
        opt.step()
    report(case, "steps", st, opt)
    set_grads(STEPS)
    for n in STEP_PARAMETER:
        gi = 0 if [m for m, _ in SHAPES].index(n) < SPLIT else 1
        opt.step_parameter(st.params[n], opt.param_groups[gi], 0)
    report(case, "step_parameter", st, opt)


def main():
    dev = torch.device("cuda:0")
    for kind in ("adafactor", "came"):
        for form in ("bf16", "bf16_sr", "f32", "master"):
            for clip in (False, True):
                for scale in ((False, True) if kind == "adafactor" else (False,)):
                    run(dev, kind, form, clip, scale)


if __name__ == "__main__":
    main()
