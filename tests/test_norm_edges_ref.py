"""The reference-only half of the norm edge tests (no GPU): the case tables reach what they claim, the hand-written
float64 formulas are the autograd ones, an honest fp32 implementation (torch's CPU kernels, outputs rounded to bf16)
stays inside every bound of tests/_norm_edges.py on every case and input, and planted errors are rejected -- the
first three of them invisible to the whole-tensor metric of test_kernels_gpu.py."""
import math
import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import _norm_edges as E

BF = torch.bfloat16
SRC = Path(__file__).resolve().parents[1] / "onetrainer_amd" / "csrc"


# ------------------------------------------------------------------------------------------
# the tables
def test_layernorm_table_covers_every_kernel():
    src = (SRC / "norm.hip").read_text()
    assert re.search(r"const int cands\[\] = \{5, 4, 3, 6, 2, 8, 1\};", src), "ln_pick changed: update the mirror"
    assert re.search(r"#define LN_MAXCH 4\b", src) and E.LN_MAX_C == 64 * 8 * 4
    reach = {E.ln_pick(c8) for c8 in range(1, E.LN_MAX_C // 8 + 1)}
    table = {**E.LN_WIDTHS, **E.LN_WIDTHS_MORE}
    for C, pick in table.items():
        assert C % 8 == 0 and C <= E.LN_MAX_C and E.ln_pick(C // 8) == pick, C
    for C in E.LN_FALLBACK:
        assert C % 8 == 0 and C <= E.LN_MAX_C and E.ln_pick(C // 8) == (0, 0), C
    assert set(table.values()) | {(0, 0)} == reach
    # the CPL 6 and 8 instantiations exist but no C <= 2048 selects them: their first widths are 3072 and 4096
    assert not {cpl for cpl, _ in reach} & {6, 8}
    assert E.ln_pick(3072 // 8) == (6, 64) and E.ln_pick(4096 // 8) == (8, 64)
    cases = E.ln_cases()
    assert len(cases) == len(set(cases))
    for C in list(E.LN_WIDTHS) + list(E.LN_FALLBACK):
        rows = {r for c, r in cases if c == C}
        rpb = E.ln_rows_per_block(C)
        assert {1, rpb + 1, 31, 77, 333} <= rows and (rpb == 1 or rpb - 1 in rows)
    assert (8, 1027) in cases and (2048, 1027) in cases and (56, 2051) in cases
    assert 2051 > 4 * 512   # ln_bwd_kernel's grid is capped at 512 blocks of 4 rows


def test_groupnorm_and_adaln_tables_reach_their_paths():
    N, HW, C, G = E.GN_SHAPES[0]
    assert (C // G) % 8 and HW % E.gn_pix_per_block(N, HW, C)          # groups straddle chunks, ragged last block
    N, HW, C, G = E.GN_SHAPES[3]
    assert (HW + E.gn_pix_per_block(N, HW, C) - 1) // E.gn_pix_per_block(N, HW, C) > 64   # gn_colreduce wraps
    assert E.GN_SHAPES[5][2] // 8 == 512 and E.GN_SHAPES[6][2] // 8 == 257
    for N, HW, C, G in E.GN_SHAPES:
        assert C % 8 == 0 and C % G == 0 and C // 8 <= 512
    assert E.mod_splits(130, 3072, 2) == 3 and 130 % 3
    assert [E.mod_splits(T, D, B) for T, B, D in E.ADALN_SHAPES[:5]] == [1, 1, 1, 1, 2]
    assert all(D <= 4096 and D % 8 == 0 for _, _, D in E.ADALN_SHAPES)


# ------------------------------------------------------------------------------------------
# hand-written formulas == autograd; honest fp32 inside the bounds
def close64(a, b):
    assert (a - b).abs().max() <= 1e-12 * max(1.0, float(b.abs().max()))


def bfr(t):
    return t.detach().to(BF)


@pytest.mark.parametrize("inp", E.INPUTS)
@pytest.mark.parametrize("C,rows", E.ln_cases())
def test_layernorm_fp32_within_bounds(C, rows, inp):
    c = E.ln_case(C, rows, inp)
    r = c.ref
    close64(r["dx_hand"], r["dx"])
    close64(r["dgamma_hand"], r["dgamma"])
    close64(r["dbeta_hand"], r["dbeta"])
    x, g, b = (t.float().requires_grad_(True) for t in (c.x, c.gamma, c.beta))
    y, mean, rstd = torch.native_layer_norm(x, (C,), g, b, c.eps)
    y.backward(c.dy.float())
    E.check_elem(bfr(y), r["y"], r["M_y"], c.name + " y")
    E.check_row_stats(mean[:, 0], rstd[:, 0], r, c.name)
    # torch's backward evaluates the fused form: held to the bound of that formula; the formula the kernels are
    # entitled to, in fp32, meets the bound the kernels are held to
    E.check_elem(bfr(x.grad), r["dx"], r["M_dx_fused"], c.name + " dx (torch, fused form)")
    y2, mean2, rstd2, dx2, _ = E.rownorm_fp32(c.x, c.gamma.float(), c.beta.float(), c.eps, c.dy)
    E.check_elem(bfr(y2), r["y"], r["M_y"], c.name + " y (entitled form)")
    E.check_row_stats(mean2, rstd2, r, c.name + " (entitled form)")
    E.check_elem(bfr(dx2), r["dx"], r["M_dx"], c.name + " dx")
    E.check_elem(bfr(dx2 + c.dres.float()), r["dx"] + c.dres.double(), r["M_dx"] + c.dres.double().abs(),
                 c.name + " dx + dres")
    E.check_elem(bfr(dx2 + c.prev.float()), r["dx"] + c.prev.double(), r["M_dx"] + c.prev.double().abs(),
                 c.name + " dx accumulated")
    for n, grad, prev in (("dgamma", g.grad, c.pg), ("dbeta", b.grad, c.pb)):
        E.check_col(grad, r[n], r["B_" + n], f"{c.name} {n} fp32")
        E.check_col(bfr(grad), r[n], r["B_" + n], f"{c.name} {n} bf16")
        E.check_col(bfr(prev.float() + grad), r[n], r["B_" + n], f"{c.name} {n} bf16 param_acc", prev=prev)
        E.check_col(prev.float() + grad, r[n], r["B_" + n], f"{c.name} {n} fp32 param_acc", prev=prev.float())


@pytest.mark.parametrize("inp", E.INPUTS)
@pytest.mark.parametrize("silu,eps", E.GN_MODES)
@pytest.mark.parametrize("N,HW,C,G", E.GN_SHAPES)
def test_groupnorm_fp32_within_bounds(N, HW, C, G, silu, eps, inp):
    for affine in (True, False) if (silu and eps == 1e-5) else (True,):
        c = E.gn_case(N, HW, C, G, silu, eps, inp, affine)
        r = c.ref
        close64(r["dx_hand"], r["dx"])
        close64(r["dgamma_hand"], r["dgamma"])
        close64(r["dbeta_hand"], r["dbeta"])
        x = c.x.float().permute(0, 2, 1).contiguous().requires_grad_(True)
        g = (torch.ones(C) if c.gamma is None else c.gamma.float()).requires_grad_(True)
        b = (torch.zeros(C) if c.beta is None else c.beta.float()).requires_grad_(True)
        z, mean, rstd = torch.native_group_norm(x, g, b, N, C, HW, G, c.eps)
        y = F.silu(z) if silu else z
        y.backward(c.dy.float().permute(0, 2, 1))
        dx = x.grad.permute(0, 2, 1)
        E.check_elem(bfr(y.permute(0, 2, 1)), r["y"], r["M_y"], c.name + " y")
        E.check_group_stats(mean.reshape(-1), rstd.reshape(-1), r, c.name)
        E.check_elem(bfr(dx), r["dx"], r["M_dx_fused"], c.name + " dx (torch, its own fused form)")
        y2, mean2, rstd2, dx2, dg2, db2 = E.groupnorm_fp32(c.x, c.gamma, c.beta, G, c.eps, silu, c.dy)
        E.check_elem(bfr(y2), r["y"], r["M_y"], c.name + " y (entitled form)")
        E.check_group_stats(mean2, rstd2, r, c.name + " (entitled form)")
        E.check_elem(bfr(dx2), r["dx"], r["M_dx"], c.name + " dx")
        E.check_elem(bfr(dx2 + c.dres.float()), r["dx"] + c.dres.double(), r["M_dx"] + c.dres.double().abs(),
                     c.name + " dx + dres")
        E.check_elem(bfr(dx2 + c.prev.float()), r["dx"] + c.prev.double(), r["M_dx"] + c.prev.double().abs(),
                     c.name + " dx accumulated")
        E.check_col(dg2, r["dgamma"], r["B_dgamma"], c.name + " dgamma (entitled form)")
        E.check_col(db2, r["dbeta"], r["B_dbeta"], c.name + " dbeta (entitled form)")
        for n, grad, prev in (("dgamma", g.grad, c.pg), ("dbeta", b.grad, c.pb)):
            E.check_col(grad, r[n], r["B_" + n], f"{c.name} {n} fp32")
            E.check_col(bfr(prev.float() + grad), r[n], r["B_" + n], f"{c.name} {n} bf16 param_acc", prev=prev)


@pytest.mark.parametrize("inp", E.INPUTS)
@pytest.mark.parametrize("T,B,D", E.ADALN_SHAPES)
def test_adaln_fp32_within_bounds(T, B, D, inp):
    c = E.adaln_case(T, B, D, inp)
    r = c.ref
    close64(r["dx_hand"], r["dx"])
    close64(r["dshift_hand"], r["dshift"])
    close64(r["dscale_hand"], r["dscale"])
    rest = r["dmod_rest"].clone()
    rest[:, c.shift_off:c.scale_off + D] = 0
    assert not rest.any()
    x, md = c.x.float().requires_grad_(True), c.mod.float().requires_grad_(True)
    ln, mean, rstd = torch.native_layer_norm(x.view(T, B, D), (D,), None, None, c.eps)
    y = ln * (1 + md[None, :, c.scale_off:c.scale_off + D]) + md[None, :, c.shift_off:c.shift_off + D]
    y.backward(c.dy.float().view(T, B, D))
    E.check_elem(bfr(y.reshape(T * B, D)), r["y"], r["M_y"], c.name + " y")
    E.check_row_stats(mean.reshape(-1), rstd.reshape(-1), r, c.name)
    E.check_elem(bfr(x.grad), r["dx"], r["M_dx_fused"], c.name + " dx (torch, fused form)")
    mf = c.mod.float()
    y2, mean2, rstd2, dx2, _ = E.rownorm_fp32(c.x, (1 + mf[:, c.scale_off:c.scale_off + D]).repeat(T, 1),
                                              mf[:, c.shift_off:c.shift_off + D].repeat(T, 1), c.eps, c.dy)
    E.check_elem(bfr(y2), r["y"], r["M_y"], c.name + " y (entitled form)")
    E.check_row_stats(mean2, rstd2, r, c.name + " (entitled form)")
    E.check_elem(bfr(dx2), r["dx"], r["M_dx"], c.name + " dx")
    E.check_elem(bfr(dx2 + c.dres.float()), r["dx"] + c.dres.double(), r["M_dx"] + c.dres.double().abs(),
                 c.name + " dx + dres")
    E.check_col(bfr(md.grad[:, c.shift_off:c.shift_off + D]), r["dshift"], r["B_dshift"], c.name + " dshift")
    E.check_col(bfr(md.grad[:, c.scale_off:c.scale_off + D]), r["dscale"], r["B_dscale"], c.name + " dscale")


# ------------------------------------------------------------------------------------------
# planted errors: each rejected by the element-wise check; OLD records whether the whole-tensor metric at the
# bound of the existing tests (1e-2 forward and parameter gradients, 2e-2 input gradient) would have passed it
OLD: dict = {}


def rejected(fn):
    with pytest.raises(AssertionError, match="out of bound|guard"):
        fn()


def ln_hand(x, gamma, beta, eps, mean=None, rstd=None):
    x, g, b = x.double(), gamma.double(), beta.double()
    m = x.mean(-1, keepdim=True) if mean is None else mean
    rs = (((x - m) ** 2).mean(-1, keepdim=True) + eps).rsqrt() if rstd is None else rstd
    return (x - m) * rs * g + b, m, rs


def test_planted_stats_over_c_minus_8():
    c = E.ln_case(320, 77, "row_scales")
    r = c.ref
    xs = c.x.double()[:, :-8]
    m = xs.mean(-1, keepdim=True)
    rs = (((xs - m) ** 2).mean(-1, keepdim=True) + c.eps).rsqrt()
    bad = bfr(ln_hand(c.x, c.gamma, c.beta, c.eps, m, rs)[0])
    OLD["stats over C-8"] = E.whole(bad, r["y"])
    assert OLD["stats over C-8"] < 1e-2
    rejected(lambda: E.check_elem(bad, r["y"], r["M_y"], "y"))
    E.check_elem(bfr(r["y"]), r["y"], r["M_y"], "y")


def test_planted_neighbour_rstd():
    c = E.ln_case(320, 77, "row_scales")
    r = c.ref
    amax = r["dx"].abs().amax(-1)[:-1]
    amax[16::17] = math.inf   # rows 16 -> 17 step 2^-16 in scale; every other neighbour differs by a factor 2
    row = int(amax.argmin())
    bad = r["dx"].clone()
    bad[row] *= r["rstd"][row + 1] / r["rstd"][row]   # dx = rstd (...): the neighbour's factor (2 x or 1/2 x)
    bad = bfr(bad)
    OLD["neighbour's rstd"] = E.whole(bad, r["dx"])
    assert OLD["neighbour's rstd"] < 2e-2
    rejected(lambda: E.check_elem(bad, r["dx"], r["M_dx"], "dx"))


def test_planted_last_row_missing_from_dbeta():
    c = E.ln_case(320, 333, "row_scales")
    r = c.ref
    bad = (r["dbeta"] - c.dy.double()[-1]).float()
    OLD["last row missing from dbeta"] = E.whole(bad, r["dbeta"])
    assert OLD["last row missing from dbeta"] < 1e-2
    rejected(lambda: E.check_col(bad, r["dbeta"], r["B_dbeta"], "dbeta"))
    rejected(lambda: E.check_col(bfr(bad), r["dbeta"], r["B_dbeta"], "dbeta bf16"))
    E.check_col(r["dbeta"].float(), r["dbeta"], r["B_dbeta"], "dbeta")


def test_planted_chunk_in_first_channels_group():
    N, HW, C, G = E.GN_SHAPES[0]
    c = E.gn_case(N, HW, C, G, False, 1e-5, "row_scales")
    r = c.ref
    Cg = C // G
    assert Cg == 10
    grp = torch.arange(C) // 8 * 8 // Cg   # every channel of a chunk in the group of the chunk's first channel
    m, rs = r["mean"].view(N, 1, G)[:, :, grp], r["rstd"].view(N, 1, G)[:, :, grp]
    bad = bfr((c.x.double() - m) * rs * c.gamma.double() + c.beta.double())
    OLD["chunk in its first channel's group"] = E.whole(bad, r["y"])
    rejected(lambda: E.check_elem(bad, r["y"], r["M_y"], "y"))


def test_planted_dres_dropped_in_last_pixel_block():
    N, HW, C, G = E.GN_SHAPES[0]
    c = E.gn_case(N, HW, C, G, True, 1e-5, "row_scales")
    r = c.ref
    ppb = E.gn_pix_per_block(N, HW, C)
    full = r["dx"] + c.dres.double()
    bad = full.clone()
    bad[:, HW // ppb * ppb:] = r["dx"][:, HW // ppb * ppb:]
    bad = bfr(bad)
    OLD["dres dropped in the last pixel block"] = E.whole(bad, full)
    M = r["M_dx"] + c.dres.double().abs()
    rejected(lambda: E.check_elem(bad, full, M, "dx + dres"))
    E.check_elem(bfr(full), full, M, "dx + dres")


def test_planted_eps_dropped_on_tiny_rows():
    c = E.ln_case(320, 77, "tiny")
    r = c.ref
    bad = bfr(ln_hand(c.x, c.gamma, c.beta, 0.0)[0])
    OLD["eps dropped"] = E.whole(bad, r["y"])
    rejected(lambda: E.check_elem(bad, r["y"], r["M_y"], "y"))
    rs = ln_hand(c.x, c.gamma, c.beta, 0.0)[2][:, 0]
    rejected(lambda: E.check_row_stats(r["mean"].float(), rs.float(), r, "stats"))


def test_planted_adaln_wrong_modulation_row():
    T, B, D = 37, 3, 256
    c = E.adaln_case(T, B, D, "row_scales")
    r = c.ref
    md = c.mod.double()
    idx = torch.arange(T * B) // B % B   # r // B where r % B belongs
    ln = r["xhat"]
    bad = bfr(ln * (1 + md[idx, c.scale_off:c.scale_off + D]) + md[idx, c.shift_off:c.shift_off + D])
    OLD["adaLN modulation row r // B"] = E.whole(bad, r["y"])
    rejected(lambda: E.check_elem(bad, r["y"], r["M_y"], "y"))
    good = torch.arange(T * B) % B
    E.check_elem(bfr(ln * (1 + md[good, c.scale_off:c.scale_off + D]) + md[good, c.shift_off:c.shift_off + D]),
                 r["y"], r["M_y"], "y")


def test_planted_guard_row_written():
    buf, view = E.guarded((2,), 5, 16)
    view.copy_(torch.ones(2, 5, 16))
    assert E.guards_intact(buf, 5, 16) and view.shape == (2, 5, 16) and view.data_ptr() % 16 == 0
    for where in ((1, 0, 8), (0, 6, 23), (0, 3, 7), (1, 2, 24)):   # guard row above / below, guard column left / right
        b2 = buf.clone()
        b2[where] = 1.0
        assert not E.guards_intact(b2, 5, 16), where
    b2 = buf.clone()
    b2.view(torch.int16)[0, 0, 0] = E.NANBITS + 1   # another NaN is still a write
    assert not E.guards_intact(b2, 5, 16)
    w = E.wide(torch.ones(3, 16, dtype=BF), 48, 16)
    assert w.stride(0) == 48 and w.storage_offset() == 16 and bool((w == 1).all())


def test_planted_errors_report():
    """the first three planted errors pass the whole-tensor metric (asserted where they are planted); the table
    of all of them is printed for the record (pytest -s)"""
    for k, v in OLD.items():
        print(f"planted: {k}: whole-tensor metric {v:.3e}")
