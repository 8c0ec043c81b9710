"""GEMMs over a frozen e4m3 weight (csrc/gemm_w8.hip: kernels.linear_w8 / linear_w8_dgrad / quantize_fp8) against
float64 on the CPU.  The reference weight is dq = w8.to(bf16) * scale.to(bf16), LinearFp8.forward's operand.

Per-element bound: one bf16 rounding (8 significant bits: relative 2^-8) of an fp32 sum of R = K (forward) or N
(dgrad) exact bf16 x bf16 products plus the epilogue terms, each fp32 addition relative 2^-24, so
    |out - ref| <= 2^-8 |ref| + (R + 2) 2^-24 (1 + 2^-8) sum |terms|.
Shapes: the tile is 128 x 128 with 64-deep contraction steps; weights move in 16-groups, activations in 8-chunks."""
import functools

import pytest
import torch

from onetrainer_amd import kernels as K

pytestmark = pytest.mark.gpu
BF, E4 = torch.bfloat16, torch.float8_e4m3fn

# (M, N, K): one row, one 16-group, N % 16 == 8 | each of M, N, K one unit past a tile / step edge (K = step + 16) |
# several tiles each way, a three-step contraction with a tail, K past the dgrad's 128-column tile
SHAPES = [(1, 8, 16), (129, 136, 80), (130, 264, 144)]
FORMS = [("fwd", "none"), ("fwd", "bias"), ("fwd", "residual"), ("dgrad", "none"), ("dgrad", "residual")]


def dq_of(w8, scale):
    return w8.view(E4).to(BF) * scale.to(BF)[:, None]


@functools.lru_cache(maxsize=None)
def case(form, epi, shape):
    """CPU inputs and the float64 reference with its bound; the row scales are two members' scalars whose boundary
    (row 72) falls inside a tile"""
    M, N, Kd = shape
    g = torch.Generator().manual_seed(M * 1000003 + N * 1009 + Kd + len(form) + len(epi))
    w8 = torch.randint(0, 256, (N, Kd), generator=g, dtype=torch.uint8)
    w8[(w8 & 0x7F) == 0x7F] = 0x38   # no NaN bytes
    scale = torch.where(torch.arange(N) < 72, 0.0123, 0.0031).float()
    dq = dq_of(w8, scale).double()
    a = torch.randn(M, Kd if form == "fwd" else N, generator=g).to(BF)
    cols = N if form == "fwd" else Kd
    bias = torch.randn(cols, generator=g).to(BF) if epi == "bias" else None
    res = (torch.randn(M, cols, generator=g) * 20).to(BF) if epi == "residual" else None
    b = dq.T if form == "fwd" else dq
    ref, mag = a.double() @ b, a.double().abs() @ b.abs()
    for t in (bias, res):
        if t is not None:
            ref, mag = ref + t.double(), mag + t.double().abs()
    bound = 2.0 ** -8 * ref.abs() + (a.shape[1] + 2) * 2.0 ** -24 * (1 + 2.0 ** -8) * mag
    return a, w8, scale, bias, res, ref, bound


def run(form, a, w8, scale, bias, res):
    dev = lambda t: None if t is None else t.cuda()
    if form == "fwd":
        return K.linear_w8(dev(a), dev(w8), dev(scale), bias=dev(bias), residual=dev(res))
    return K.linear_w8_dgrad(dev(a), dev(w8), dev(scale), residual=dev(res))


def check(out, ref, bound):
    err = (out.cpu().double() - ref).abs()
    bad = err > bound
    assert not bad.any(), f"{int(bad.sum())} elements past the bound, worst {float((err / bound.clamp_min(1e-30)).max()):.2f} x"


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("form,epi", FORMS)
def test_parity(form, epi, shape):
    a, w8, scale, bias, res, ref, bound = case(form, epi, shape)
    out = run(form, a, w8, scale, bias, res)
    check(out, ref, bound)
    assert torch.equal(out, run(form, a, w8, scale, bias, res))   # two launches, the same bits


@pytest.mark.parametrize("shape", SHAPES[1:], ids=str)
@pytest.mark.parametrize("form", ["fwd", "dgrad"])
def test_zero_fill(form, shape):
    """the weight inside a buffer of 0x7E bytes (e4m3 448) and the activation inside one of NaNs: what lies past a
    row's end or the last row must not reach an accumulator"""
    a, w8, scale, _, _, ref, bound = case(form, "none", shape)
    N, Kd = w8.shape
    wbuf = torch.full((N + 130, Kd + 96), 0x7E, dtype=torch.uint8).cuda()
    wbuf[1:1 + N, 16:16 + Kd] = w8.cuda()
    abuf = torch.full((a.shape[0] + 130, a.shape[1]), float("nan"), dtype=BF).cuda()
    abuf[1:1 + a.shape[0]] = a.cuda()
    aw, ww, sc = abuf[1:1 + a.shape[0]], wbuf[1:1 + N, 16:16 + Kd], scale.cuda()
    out = K.linear_w8(aw, ww, sc) if form == "fwd" else K.linear_w8_dgrad(aw, ww, sc)
    check(out, ref, bound)


@pytest.mark.parametrize("form", ["fwd", "dgrad"])
def test_exact(form):
    """small-integer activations, integer e4m3 weights, power-of-two member scales: every partial sum is an fp32
    number below 2^24, so the output is the exact product rounded once to bf16, bit for bit"""
    M, N, Kd = SHAPES[2]
    g = torch.Generator().manual_seed(7)
    w8 = torch.randint(-8, 9, (N, Kd), generator=g).float().to(E4).view(torch.uint8)
    scale = torch.where(torch.arange(N) < 72, 0.5, 2.0).float()
    a = torch.randint(-4, 5, (M, Kd if form == "fwd" else N), generator=g).to(BF)
    dq = dq_of(w8, scale).double()
    ref = a.double() @ (dq.T if form == "fwd" else dq)
    assert ref.abs().max() < 2 ** 24
    out = run(form, a, w8, scale, None, None)
    assert torch.equal(out.cpu(), ref.float().to(BF))


def quant_input(name):
    if name == "ties":      # absmax 448 -> scale 1: exact midpoints of neighbouring e4m3 values, and half the least one
        w = torch.tensor([448., -448., 432., -432., 17., 19., -21., 1.0625, 1.1875, 2.0 ** -10, 3 * 2.0 ** -10, 0.,
                          9., 11., 104., 200.]).repeat(5, 1)
    elif name == "top-bin":  # |w| / scale in [400, 448]: the last two e4m3 steps and the clamp at +-448
        w = torch.linspace(400., 448., 3 * 32).view(3, 32) * 0.37 * torch.tensor([1., -1.]).repeat(16)
    elif name == "zeros":
        w = torch.zeros(2, 16)
    elif name == "odd-rows":
        w = torch.randn(3, 48, generator=torch.Generator().manual_seed(3)) * 0.02
    else:                    # more 16-groups than one sweep of the grid covers
        w = torch.randn(2049, 2048, generator=torch.Generator().manual_seed(4)) * 0.05
    return w


@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("name", ["ties", "top-bin", "zeros", "odd-rows", "large"])
def test_quantize_matches_torch_cast(name, dtype):
    w = quant_input(name).to(dtype)
    scale = torch.clamp(w.float().abs().max(), min=1e-12) / 448
    want = (w / scale).to(E4).view(torch.uint8)
    w8, rows = K.quantize_fp8(w.cuda())
    assert torch.equal(rows.cpu(), scale.expand(w.shape[0]))
    assert torch.equal(w8.cpu(), want)


def test_contract_violations_raise():
    x = torch.zeros(4, 24, dtype=BF, device="cuda")
    w8 = torch.zeros(8, 24, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="multiple of 16"):
        K.linear_w8(x, w8, torch.ones(8, device="cuda"))
