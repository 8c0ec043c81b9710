"""Flash attention for 160-wide heads (csrc/attention_wide.hip) against float64 softmax(q k^T scale) v and its
autograd gradients, per row, beside the materialized path (attn_mat_fwd / attn_mat_bwd) on the same inputs."""
import ctypes as C
import math

import pytest
import torch

from onetrainer_amd import _lib
from onetrainer_amd import kernels as K
from onetrainer_amd.module.functional import CrossAttnFn, SelfAttnFn

pytestmark = pytest.mark.gpu
B, H = 2, 2
PEAK = 37   # the peaked query of the peaked case


def ref64(q, k, v, do, scale):
    """float64 o, lse (natural log), dq, dk, dv from the bf16 operands [B, N, H*D]"""
    D = q.shape[-1] // H
    qh, kh, vh = (t.detach().cpu().double().view(B, -1, H, D).transpose(1, 2).requires_grad_(True) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) * scale
    o = torch.softmax(s, -1) @ vh
    o.backward(do.cpu().double().view(B, -1, H, D).transpose(1, 2))
    flat = lambda t: t.transpose(1, 2).reshape(B, -1, H * D)   # noqa: E731
    return {"o": flat(o.detach()), "lse": torch.logsumexp(s.detach(), -1), "dq": flat(qh.grad), "dk": flat(kh.grad),
            "dv": flat(vh.grad)}


def row_err(got, ref):
    """worst over rows [b, n, h, :] of max|got - ref| / max|ref|"""
    g, r = got.float().cpu().double().view(B, -1, H, ref.shape[-1] // H), ref.view(B, -1, H, ref.shape[-1] // H)
    return float(((g - r).abs().amax(-1) / r.abs().amax(-1)).max())


def check_bounds(what, name, got, mat, ref, cap):
    """the project's whole-tensor bound, and the worst row within 2 x the materialized path's on the same inputs"""
    e, em = row_err(got, ref), row_err(mat, ref)
    whole = float((got.float().cpu().double() - ref).abs().max() / (ref.abs().max() + 1e-6))
    print(f"WIDE {what} {name}: row err {e:.3e} materialized {em:.3e} whole {whole:.3e}")
    assert whole < cap, f"{name}: rel_err {whole:.3e}"
    assert e <= 2 * em, f"{name}: worst row {e:.3e} > 2 x materialized {em:.3e}"


def operands(Nq, Nk, D, layout, dev, peaked=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    Ch = H * D
    q, k, v, do = (torch.randn(B, n, Ch, generator=g) for n in (Nq, Nk, Nk, Nq))
    if peaked:   # query PEAK: the last key's logit ~30 above the rest, so the running max grows late, P underflows
        q[:, :, ::D], k[:, :, ::D] = 0.0, 0.0   # each head's first column carries the peak alone: other rows keep theirs
        q[:, PEAK, ::D], k[:, -1, ::D] = (30.0 * D ** 0.5) ** 0.5, (30.0 * D ** 0.5) ** 0.5
    if layout == "fused" and Nq == Nk:
        qkv = torch.cat([q, k, v], -1).to(dev, torch.bfloat16)
        q, k, v = qkv[..., :Ch], qkv[..., Ch:2 * Ch], qkv[..., 2 * Ch:]
    elif layout == "fused":
        kv = torch.cat([k, v], -1).to(dev, torch.bfloat16)
        q, k, v = q.to(dev, torch.bfloat16), kv[..., :Ch], kv[..., Ch:]
    else:
        q, k, v = (t.to(dev, torch.bfloat16) for t in (q, k, v))
    return q, k, v, do.to(dev, torch.bfloat16)


# (Nq, Nk, Dv, layout, peaked, scale): a single row and key; a partial wave; a second workgroup with a partial tail;
# one exact key tile; a partial last tile (77, 97); zero-padded head columns (136); a peaked row; an explicit scale;
# 289 keys: a wave's second and third sub-tile (both ring slots reused) and a one-key last tile, the peak on that key
# (288: wave 1's third sub-tile, so its running max jumps from a finite value and O, l are rescaled)
CASES = [(1, 1, 160, "sep", False, None), (1, 1, 136, "fused", False, None), (33, 32, 160, "sep", False, None),
         (33, 77, 136, "fused", False, None), (130, 77, 160, "fused", False, None), (130, 97, 160, "sep", True, None),
         (130, 32, 136, "sep", False, 0.11), (33, 97, 160, "fused", False, None), (130, 289, 160, "fused", True, None)]


@pytest.mark.parametrize("Nq,Nk,D,layout,peaked,scale", CASES)
def test_parity(dev, Nq, Nk, D, layout, peaked, scale):
    q, k, v, do = operands(Nq, Nk, D, layout, dev, peaked)
    sc = scale if scale is not None else D ** -0.5
    ref = ref64(q, k, v, do, sc)
    o, lse = K.attn_fwd(q, k, v, H, scale)
    dq, dk, dv = K.attn_bwd(q, k, v, o, lse, do, H, scale)
    om, P = K.attn_mat_fwd(q, k, v, H, scale)
    mq, mk, mv = K.attn_mat_bwd(q, k, v, P, do, H, scale)
    lse_err = float((lse.cpu().double() * math.log(2.0) - ref["lse"]).abs().max())
    print(f"WIDE Nq={Nq} Nk={Nk} D={D} {layout} lse err {lse_err:.3e}")
    assert lse_err <= 1e-3
    # where the reference is exactly 0 (one key: dS = P (dP - delta) = 0) the kernels leave the fp32 rounding of two
    # D-term dot products, each within D 2^-24 sum|dO v|, times scale |k| (dq) or scale |q| (dk)
    mx = lambda t: float(t.float().abs().max())   # noqa: E731
    zero = 2 * D * D * 2.0 ** -24 * mx(do) * mx(v) * sc * max(mx(q), mx(k))
    for name, got, mat, cap in (("o", o, om, 2e-2), ("dq", dq, mq, 3e-2), ("dk", dk, mk, 3e-2), ("dv", dv, mv, 3e-2)):
        r = ref[name]
        if float(r.abs().max()) == 0.0:
            assert mx(got) <= zero, f"{name}: {mx(got):.3e} where the reference is 0 (bound {zero:.3e})"
            continue
        check_bounds(f"Nq={Nq} Nk={Nk} D={D} {layout}", name, got, mat, r, cap)
    if peaked:   # query PEAK's dq (e^-30 of the others) is lost to the fp32 delta in both paths, error 1: the rest apart
        rest = lambda t: torch.cat([t[:, :PEAK], t[:, PEAK + 1:]], 1)   # noqa: E731
        check_bounds(f"Nq={Nq} Nk={Nk} D={D} {layout}", "dq but PEAK", rest(dq), rest(mq), rest(ref["dq"]), 3e-2)


def test_dispatch(dev):
    """D = 160 runs the flash kernels (aux = lse, not the materialized P); D = 168 stays materialized"""
    q, k, v, _ = operands(33, 77, 160, "sep", dev)
    _, aux = K.attn_fwd(q, k, v, H)
    assert aux.dtype == torch.float32 and tuple(aux.shape) == (B, H, 33)
    a = _lib.AttnArgs()
    a.B, a.H, a.Nq, a.Nk, a.Dv = B, H, 33, 77, 160
    assert K.lib().otamd_attn_bwd_ws_bytes(C.byref(a)) > 0
    q, k, v, _ = operands(33, 77, 168, "sep", dev)
    _, aux = K.attn_fwd(q, k, v, H)
    assert aux.dtype == torch.bfloat16 and tuple(aux.shape) == (B * H, 33, 80)


@pytest.mark.parametrize("Nq,Nk,layout", [(130, 130, "fused"), (130, 77, "fused")])
def test_deterministic(dev, Nq, Nk, layout):
    def run(src):
        q, k, v, do = src
        o, lse = K.attn_fwd(q, k, v, H)
        return (o,) + tuple(K.attn_bwd(q, k, v, o, lse, do, H))
    src = operands(Nq, Nk, 160, layout, dev)
    first, second = run(src), run(src)
    third = run(operands(Nq, Nk, 160, layout, dev))   # the same values at other addresses
    for x, y, z in zip(first, second, third):
        assert torch.equal(x, y) and torch.equal(x, z)


@pytest.mark.parametrize("cross", [False, True])
def test_autograd_functions(dev, cross):
    """SelfAttnFn / CrossAttnFn at D = 160: the saved-tensor contract with lse in place of P"""
    D, Nq, Nk = 160, 70, (77 if cross else 70)
    q, k, v, do = operands(Nq, Nk, D, "sep", dev, seed=1)
    ref = ref64(q, k, v, do, D ** -0.5)
    om, P = K.attn_mat_fwd(q, k, v, H)
    mat = dict(zip(("dq", "dk", "dv"), K.attn_mat_bwd(q, k, v, P, do, H)), o=om)
    if cross:
        q, kv = q.clone().requires_grad_(True), torch.cat([k, v], -1).requires_grad_(True)
        o = CrossAttnFn.apply(q, kv, H)
        o.backward(do)
        got = {"o": o.detach(), "dq": q.grad, "dk": kv.grad[..., :H * D], "dv": kv.grad[..., H * D:]}
    else:
        qkv = torch.cat([q, k, v], -1).requires_grad_(True)
        o = SelfAttnFn.apply(qkv, H)
        o.backward(do)
        g = qkv.grad
        got = {"o": o.detach(), "dq": g[..., :H * D], "dk": g[..., H * D:2 * H * D], "dv": g[..., 2 * H * D:]}
    for name, g in got.items():
        check_bounds(f"autograd cross={cross}", name, g, mat[name], ref[name], 2e-2 if name == "o" else 3e-2)
