"""The float64 DoRA oracle (tests/_oracle_dora.py) against the reference's own fp32 run (tests/golden/dora_steps.npz,
written by tests/golden/make_dora_golden.py): initial dora_scale, merged weight, outputs and adapter gradients, both
kept axes, epsilon on and off.  The reference computes in fp32, so it is held to the same derived fp32 bounds as the
kernels are in tests/test_dora_gpu.py; bf16 values are equal bits or one bf16 step apart."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import _oracle_dora as O

GOLD = Path(__file__).parent / "golden"
sys.path.insert(0, str(GOLD))
import make_dora_golden as MG   # noqa: E402  (the net and the inputs, regenerated from their seeds)

EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD / "dora_steps.npz")


def _okc(t):
    """reference layout ([out, in] or [out, in, kh, kw]) -> [out, kk, in] float64"""
    a = np.asarray(t, dtype=np.float64)
    if a.ndim == 2:
        return a[:, None, :]
    return a.transpose(0, 2, 3, 1).reshape(a.shape[0], -1, a.shape[1])


def _module(gold, case, m, which="state"):
    net = MG.dora_net()
    W = _okc(getattr(net, m).weight.detach().numpy())
    p = f"{case}/{which}/lora_unet.{m}."
    down, up = _okc(gold[p + "lora_down.weight"]), np.asarray(gold[p + "lora_up.weight"], dtype=np.float64)
    return W, down, up.reshape(up.shape[0], -1), np.asarray(gold[p + "dora_scale"], dtype=np.float64)


CASES = [MG.case_name(a, e) for a, e in MG.CASES]


@pytest.mark.parametrize("case", CASES)
def test_initial_state(gold, case):
    axis = int(case.startswith("out"))
    for m in MG.MODULES:
        W, down, up, scale = _module(gold, case, m, "init")
        assert not up.any() and down.any()
        want = O.norms(W, down, up, MG.ALPHA / MG.RANK, axis, 0.0)       # the norm of the base weight, no epsilon
        ref_shape = ((W.shape[0], 1) if axis else (1, W.shape[2])) + ((1, 1) if m != "lin" else ())
        assert scale.shape == ref_shape
        assert (np.abs(scale.reshape(-1) - want) <= O.norm_bound(W, down, up, 0.5, axis, 0.0)).all()
        assert float(gold[f"{case}/init/lora_unet.{m}.alpha"]) == MG.ALPHA


@torch.no_grad()
def test_merge_and_outputs(gold):
    tally = O.Bf16Tally()
    for case in CASES:
        axis, eps = int(case.startswith("out")), EPS32 if case.endswith("_eps") else 0.0
        s = MG.ALPHA / MG.RANK
        net = MG.dora_net()
        x_lin, x_conv = MG.dora_inputs()
        wps, bws = {}, {}
        for m in MG.MODULES:
            W, down, up, scale = _module(gold, case, m)
            sc = scale.reshape(-1)
            n, wp = O.merge(W, down, up, sc, s, axis, eps)
            bn = O.norm_bound(W, down, up, s, axis, eps)
            # W' = scale (Weff / n) in fp32: the error of Weff scaled, the relative error of n, three roundings
            bw = np.abs(O._bc(sc / n, axis)) * (MG.RANK + 2) * O.U * O.mag(W, down, up, s) \
                + np.abs(wp) * (O._bc(bn / n, axis) + 3 * O.U)
            got = _okc(gold[f"{case}/wp/{m}"])
            assert (np.abs(got - wp) <= bw).all(), (case, m)
            tally.add(O.bf16_round(got).reshape(-1), wp.reshape(-1), f"{case} {m}")
            wps[m], bws[m] = wp, bw
        # fp32 outputs: y = sum x w' + b, so the weight bound carried through |x| plus the dot product's own rounding
        xl = x_lin.double().numpy()
        wl, bl = wps["lin"][:, 0, :], net.lin.bias.detach().double().numpy()
        y = xl @ wl.T + bl
        by = np.abs(xl) @ bws["lin"][:, 0, :].T + (wl.shape[1] + 1) * O.U * (np.abs(xl) @ np.abs(wl).T + np.abs(bl))
        assert (np.abs(gold[f"{case}/y_lin"] - y) <= by).all(), case

        def conv_w(m, a):
            k = 3 if m == "conv" else 1
            return torch.from_numpy(a.reshape(a.shape[0], k, k, a.shape[2]).transpose(0, 3, 1, 2).copy())
        F = torch.nn.functional
        h = F.conv2d(x_conv.double(), conv_w("conv", wps["conv"]), net.conv.bias.double(), padding=1)
        ha = F.conv2d(x_conv.double().abs(), conv_w("conv", np.abs(wps["conv"])), net.conv.bias.double().abs(), padding=1)
        bh = F.conv2d(x_conv.double().abs(), conv_w("conv", bws["conv"]), padding=1) + (8 * 9 + 1) * O.U * ha
        y2 = F.conv2d(h, conv_w("pw", wps["pw"]), net.pw.bias.double())
        y2a = F.conv2d(h.abs(), conv_w("pw", np.abs(wps["pw"])), net.pw.bias.double().abs())
        by2 = F.conv2d(bh, conv_w("pw", np.abs(wps["pw"]))) + F.conv2d(h.abs(), conv_w("pw", bws["pw"])) \
            + (12 + 1) * O.U * y2a
        assert (np.abs(gold[f"{case}/y_conv"] - y2.numpy()) <= by2.numpy()).all(), case
        # under bf16 autocast the reference's up @ down is itself an autocast matmul: its result and the scaling by
        # alpha / rank are bf16 tensors, everything after (the add of W, the norm, the division) is fp32; the
        # Linear then reads x, W' and the bias rounded to bf16 once and rounds its output once.  (The kernels form
        # up @ down in fp32 whatever the autocast state: DESIGN.md, DoRA deviations.)
        def rb(a):
            return torch.from_numpy(np.asarray(a)).to(torch.bfloat16).double().numpy()
        W, down, up, scale = _module(gold, case, "lin")
        ba = rb(rb(rb(up) @ rb(down[:, 0, :])) * s)
        xa = W[:, 0, :] + ba
        na = np.sqrt((xa * xa).sum(axis=axis)) + eps
        wa = scale.reshape(1, -1) * (xa / na[None, :]) if axis == 0 else scale.reshape(-1, 1) * (xa / na[:, None])
        ya = rb(xl) @ rb(wa).T + rb(bl)
        tally.add(O.bf16_round(gold[f"{case}/y_lin_bf16"]).reshape(-1), ya.reshape(-1), f"{case} y_lin autocast")
    tally.check()


@pytest.mark.parametrize("case", CASES)
def test_projection(gold, case):
    axis, eps = int(case.startswith("out")), EPS32 if case.endswith("_eps") else 0.0
    s = MG.ALPHA / MG.RANK
    for m in MG.MODULES:
        W, down, up, scale = _module(gold, case, m)
        sc = scale.reshape(-1)
        n = O.norms(W, down, up, s, axis, eps)
        rel_n = float((O.norm_bound(W, down, up, s, axis, eps) / n).max())   # the reference divides by its fp32 n
        G = _okc(gold[f"{case}/g/{m}"])
        (d_down, d_up, d_scale), (b_down, b_up, b_scale) = O.project(G, W, down, up, sc, n, s, axis)
        p = f"{case}/grad/lora_unet.{m}."
        terms = {"lora_down.weight": W.shape[0], "lora_up.weight": W.shape[1] * W.shape[2],
                 "dora_scale": (W.size // n.size) * (MG.RANK + 1)}
        for leaf, want, b in (("lora_down.weight", d_down, b_down), ("lora_up.weight", d_up, b_up),
                              ("dora_scale", d_scale, b_scale)):
            got = np.asarray(gold[p + leaf], dtype=np.float64)
            got = _okc(got) if leaf == "lora_down.weight" else got.reshape(want.shape)
            slack = b / ((terms[leaf] + 4) * O.U) * rel_n
            err = np.abs(got - want)
            assert (err <= b + slack).all(), (case, m, leaf, float(err.max()))
            assert np.abs(want).max() > 0
