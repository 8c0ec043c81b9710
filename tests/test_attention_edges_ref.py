"""The reference-only half of the attention edge tests (no GPU): the float64 reference, the rounding-floor
emulation and the adversarial inputs of test_attention_edges_gpu.py have the properties those tests lean on."""
import math

import pytest
import torch

import _attn_edges as E


@pytest.mark.parametrize("Nq,Nk,Dv", [(200, 77, 64), (300, 300, 64), (333, 1000, 128)])
def test_floor_emulation(Nq, Nk, Dv):
    """the entitled roundings alone cost ~0.005 per row on unit-normal inputs, and leave the whole tensor far
    under the 2e-2 / 3e-2 it is held to"""
    c = E.geometry_case(2, 3, Nq, Nk, Dv)
    for n, f in c.floor.items():
        assert 2e-3 < f < 7.5e-3, (n, f)
        assert c.tol(n) == 4 * f
    assert E.lse_bound(c.ref) <= 2.0 ** -17
    emu = E.emulated(c.q, c.k, c.v, c.do, c.H, c.scale)
    for n in emu:
        w, cap = c.whole(emu[n], n)
        assert w < cap / 2, (n, w)
    # without the roundings the hand-written backward is the autograd one
    e = E.emulated(c.q, c.k, c.v, c.do, c.H, c.scale, round_=False)
    for n in e:
        assert (e[n] - c.ref[n]).abs().max() < 1e-12 * max(1.0, float(c.ref[n].abs().max()))


def test_row_metric_sees_one_row():
    """one wrong row among many: invisible to max|d| / max|ref| at 2e-2, plain per row"""
    c = E.geometry_case(2, 3, 200, 77, 64)
    ref = c.ref["o"]
    bad = E.heads(ref.clone(), 3).contiguous()
    row = bad[1, 2, 150].abs().argmax()
    bad[1, 2, 150, row] *= 1.05
    bad = E.unheads(bad)
    assert (bad - ref).abs().max() / ref.abs().max() < 2e-2
    m, where = E.row_metric(bad, ref, 3)
    assert where == (1, 2, 150) and 0.045 < m <= 0.05 + 1e-12 and m > c.tol("o")
    assert E.row_metric(torch.full_like(ref, math.nan), ref, 3)[0] == math.inf


@pytest.mark.parametrize("Dv,Nk", [(64, 77), (64, 190), (128, 190), (40, 77), (128, 2381)])
@pytest.mark.parametrize("order", ["first", "last", "grow"])
def test_peaked_rows_are_one_hot(Dv, Nk, order):
    Nq = 70 if Nk < 1000 else 16
    B, H = (2, 3) if Nk < 1000 else (1, 1)
    c, pi = E.peaked_case(B, H, Nq, Nk, Dv, order)
    assert E.peaked_margin(c, pi) >= 26.0
    o, lse2, dv = E.peaked_expect(c, pi)
    assert (c.ref["o"] - o).abs().max() < 1e-10   # 2^-9 is what it takes to move a bf16 value
    assert (c.ref["lse2"] - lse2).abs().max() < 1e-10
    assert (c.ref["dv"] - dv).abs().max() < 1e-9
    assert c.ref["dq"].abs().max() < 1e-9 and c.ref["dk"].abs().max() < 1e-9
    lo, hi = (0, 32) if order == "first" else ((Nk - 1) // 32 * 32, Nk)
    assert int(pi.min()) >= lo and int(pi.max()) < hi
    grow = E.tile_max_growth(c)
    if Nk > 1000:
        return   # the margin at the longest sequence the models run; the tile orderings are for the short ones
    if order == "first":     # the max is in tile 0 for every row
        assert max(grow) < 0
    elif order == "grow":    # some row of the block exceeds the forward's lazy-max threshold (8) on every tile
        assert min(grow) > 8.0
    if Dv == 64 and order != "grow":
        assert abs(float(lse2.max()) - 128 / E.LN2) < 1e-3   # 128 nats, 185 in log2 units


@pytest.mark.parametrize("Dv,Nk", [(64, 1), (64, 33), (64, 77), (64, 129), (64, 190), (128, 129), (128, 190)])
def test_negative_rows_expose_a_zero_key(Dv, Nk):
    c = E.negative_case(2, 3, 70, Nk, Dv)
    s = c.scale * (E.heads(c.q, 3) @ E.heads(c.k, 3).transpose(-1, -2))
    assert s.max() <= -20.0
    z = E.with_zero_key(c)
    for n in ("o", "dv") if Nk == 1 else ("o", "dq", "dk", "dv"):   # one key: dq = dk = 0 either way
        assert E.row_metric(z[n], c.ref[n], 3)[0] > 10 * c.tol(n), n
    assert (z["lse2"] - c.ref["lse2"]).abs().min() > 20.0
    # on unit-normal inputs the same phantom key hides under the whole-tensor bound
    u = E.geometry_case(2, 3, 200, 77, 64)
    zu = E.with_zero_key(u)
    assert (zu["o"] - u.ref["o"]).abs().max() / u.ref["o"].abs().max() < 2e-2


def test_softmax_rows_reference():
    g = torch.Generator().manual_seed(0)
    S = (torch.randn(7, 80, generator=g) + torch.linspace(-1e4, 1e4, 7)[:, None]) / 0.3
    p, lse = E.softmax_rows_ref(S, 77, E.f32(0.3))
    assert (p.sum(-1) - 1).abs().max() < 1e-12 and torch.isfinite(lse).all()
    # the fp32 product scale * S moves P by ~1e-3 at |scale S| ~ 1e4: part of the floor, not of the kernel's error
    p32, _ = E.softmax_rows_ref(S, 77, E.f32(0.3), round_scores=True)
    assert 1e-5 < E.rows_metric(p32, p)[0] < 4e-3
    # causal row 0 has one live column; a bias reaches its own head
    Sm = torch.randn(6, 5, 8, generator=g)
    bias = torch.randn(5, 7, 3, generator=g).double()
    pm = E.masked_softmax_ref(Sm, 7, 1.0, 5, 3, True, bias)
    assert pm[:, 0, 0].eq(1).all() and pm[:, 0, 1:].eq(0).all() and pm[:, 2, 3:].eq(0).all()
    want = torch.softmax(Sm[4, 4, :5].double() + bias[4, :5, 1], -1)
    assert (pm[4, 4, :5] - want).abs().max() < 1e-12
