"""Golden fixture from the reference's own DoRA code (container only).

    python tests/golden/make_dora_golden.py      -> tests/golden/dora_steps.npz

Runs LoRAModuleWrapper with lora_decompose (modules/module/LoRAModule.py:334-419, DoRAModule) through the stub harness
(tests/golden/ref_harness.py) on a tiny Linear + 3x3 Conv2d + 1x1 Conv2d net at rank 4, for both kept axes and the
norm epsilon on and off.  Per case it records the initial state dict (dora_scale included), then, with lora_up set
to non-zero values: the weight DoRAModule hands to F.linear / F.conv2d (W', fp32), the outputs in fp32 and under bf16
autocast, the gradient that reaches W' and the gradients of lora_down, lora_up and dora_scale.  Only data is stored
(the inputs and the base weights are regenerated from seeds by the functions below); no reference source.  The
fixture pins tests/_oracle_dora.py (tests/test_dora_oracle.py) and the naming the setup test checks.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
OUT = HERE / "dora_steps.npz"
RANK, ALPHA = 4, 2.0
CASES = [(axis, eps) for axis in (False, True) for eps in (True, False)]   # (decompose_output_axis, norm_epsilon)
MODULES = ("lin", "conv", "pw")


def dora_net(seed=31):
    torch.manual_seed(seed)
    net = torch.nn.Module()
    net.lin = torch.nn.Linear(16, 24)
    net.conv = torch.nn.Conv2d(8, 12, 3, padding=1)
    net.pw = torch.nn.Conv2d(12, 8, 1)
    return net


def dora_inputs(seed=32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(3, 16, generator=g), torch.randn(2, 8, 6, 6, generator=g)


def dora_forward(net, x_lin, x_conv):
    return net.lin(x_lin), net.pw(net.conv(x_conv))


def case_name(output_axis: bool, eps: bool) -> str:
    return f"{'out' if output_axis else 'in'}_{'eps' if eps else 'noeps'}"


def main():
    sys.path.insert(0, str(HERE))
    import ref_harness
    ref_harness.install()
    from modules.module.LoRAModule import LoRAModuleWrapper
    from modules.util.config.TrainConfig import TrainConfig

    rec = {}
    for output_axis, eps in CASES:
        name = case_name(output_axis, eps)
        net = dora_net()
        c = TrainConfig.default_values()
        c.lora_rank, c.lora_alpha = RANK, ALPHA
        c.lora_decompose = True
        c.lora_decompose_norm_epsilon = eps
        c.lora_decompose_output_axis = output_axis
        c.train_device = "cpu"
        torch.manual_seed(33)
        w = LoRAModuleWrapper(net, "lora_unet", c)
        for k, v in w.state_dict().items():
            rec[f"{name}/init/{k}"] = v.detach().numpy().copy()
        with torch.no_grad():
            torch.manual_seed(34)
            for m in w.lora_modules.values():
                m.lora_up.weight.copy_(torch.randn(m.lora_up.weight.shape) * 0.1)
                m.dora_scale.mul_(1 + 0.1 * torch.randn(m.dora_scale.shape))
        for k, v in w.state_dict().items():
            rec[f"{name}/state/{k}"] = v.detach().numpy().copy()
        w.hook_to_module()
        seen = {}
        for mod_name, m in w.lora_modules.items():
            def op(x, weight, bias, __op=m.op, __n=mod_name, **kw):
                if weight.requires_grad:
                    weight.retain_grad()
                seen[__n] = weight
                return __op(x, weight, bias, **kw)
            m.op = op
        x_lin, x_conv = dora_inputs()
        with torch.autocast("cpu", dtype=torch.bfloat16):
            a_lin, a_conv = dora_forward(net, x_lin, x_conv)
        rec[f"{name}/y_lin_bf16"] = a_lin.detach().float().numpy().copy()
        rec[f"{name}/y_conv_bf16"] = a_conv.detach().float().numpy().copy()
        y_lin, y_conv = dora_forward(net, x_lin, x_conv)
        (y_lin.square().sum() + y_conv.square().sum()).backward()
        rec[f"{name}/y_lin"] = y_lin.detach().numpy().copy()
        rec[f"{name}/y_conv"] = y_conv.detach().numpy().copy()
        for mod_name, m in w.lora_modules.items():
            rec[f"{name}/wp/{mod_name}"] = seen[mod_name].detach().numpy().copy()
            rec[f"{name}/g/{mod_name}"] = seen[mod_name].grad.detach().numpy().copy()
            for leaf, p in (("lora_down.weight", m.lora_down.weight), ("lora_up.weight", m.lora_up.weight),
                            ("dora_scale", m.dora_scale)):
                rec[f"{name}/grad/{m.prefix}{leaf}"] = p.grad.detach().numpy().copy()
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, len(rec), "arrays")


if __name__ == "__main__":
    main()
