"""Shared pieces of the norm edge tests (test_norm_edges_gpu.py, test_norm_edges_ref.py): float64 references of
LayerNorm, GroupNorm(+SiLU) and FLUX adaLN with their gradients, element-wise bounds, adversarial inputs and the
case tables.  Everything here is plain PyTorch on the CPU; inputs come from seeded CPU generators, so the GPU tests
and the reference-only tests see the same numbers.

Bounds (derived, not measured).  The kernels compute in fp32 and round once to bf16, so an output element may differ
from the float64 value of the bf16 operands by one bf16 rounding, 2^-8 |ref|, plus the fp32 evaluation error,
2^-17 M.  M is the float64 sum of the absolute values of the terms of the formula the kernel is entitled to use:
    LayerNorm / adaLN forward   y  = (x - mean) rstd w + b       M = rstd |w| (|x| + |mean|) + |b|
    GroupNorm apply             z  = x a + b                     M = |x a| + |b|
    LayerNorm / adaLN backward  dx = rstd (g - mean g - xhat mean(g xhat)) [+ add]
                                                                 M = rstd (|g| + mean|g| + |xhat| mean|g xhat|) + |add|
    GroupNorm backward          dx = A dz + B x + Cc [+ add]     M = |A dz| + |B x| + rstd (|mean rstd c2| + |c1|)
                                                                     + rstd (mean|gamma dz| + |xhat| mean|gamma dz xhat|) + |add|
      (Cc = rstd (mean rstd c2 - c1) is itself a difference evaluated in fp32, and c1 = mean(gamma dz), c2 =
      mean(gamma dz xhat) are sums that cancel: their summation error scales with the mean of the absolute terms,
      as in the LayerNorm form, and reaches dx as rstd (d c1 + xhat d c2).  With |Cc| alone in M an honest fp32
      evaluation misses the bound by 5 x on channels with gamma = 0, where dx = Cc.)
2^-17 is 128 fp32 half-ulps: the longest dependent addition chain of the row kernels (64 per-lane adds at 8 chunks
x 8 channels, 6 butterfly steps, a few elementwise operations) and 1-ulp hardware rsqrt / exp.
With SiLU, y = silu(z) and dz = dy silu'(z) are functions of a z that itself carries up to 2^-17 M_z: |silu'| <= 1.1
and |silu''| <= 0.5 on the real line, so M_y = 1.1 M_z + |y| and dz is allowed E_dz = 2^-17 (|dz| + 0.5 |dy| M_z),
which enters dx through A and the column sums through their terms.
Column reductions over R rows, per column: R 2^-24 sum_rows |term| (any summation order) plus the evaluation error of
the terms themselves, 2^-17 sum_rows |dy| rstd (|x| + |mean|) for dy xhat (a bf16 dy alone is exact); bf16
destinations add 2^-8 |ref|; param_acc adds the rounding of the accumulated value."""
import functools
import math

import torch

BF = torch.bfloat16
U8, U17, U22, U24 = 2.0 ** -8, 2.0 ** -17, 2.0 ** -22, 2.0 ** -24
NANBITS = 0x7FC0   # torch's bf16 NaN, the fill of every guarded destination
LN_MAX_C = 2048    # norm.hip: C <= 64 * 8 * LN_MAXCH


def f32(x: float) -> float:
    """the value the C ABI carries for a float argument (eps)"""
    return float(torch.tensor(x, dtype=torch.float32))


# ------------------------------------------------------------------------------------------
# kernel selection, mirrored from csrc/norm.hip
def ln_pick(C8: int):
    """(chunks per lane, lanes per row) of the LayerNorm row-group kernels for a row of C8 16-byte chunks, (0, 0)
    for the one-wave-per-row fallback: csrc/norm.hip ln_pick() (`const int cands[] = {5, 4, 3, 6, 2, 8, 1}`, the
    first candidate with L = C8 / CPL a power of two <= 64)."""
    for c in (5, 4, 3, 6, 2, 8, 1):
        if C8 % c:
            continue
        l = C8 // c
        if l <= 64 and l & (l - 1) == 0:
            return c, l
    return 0, 0


def ln_rows_per_block(C: int) -> int:
    """rows one 256-thread block covers: 4 waves x 64 / L rows (row-group form), 4 (fallback)"""
    cpl, L = ln_pick(C // 8)
    return 4 * (64 // L) if cpl else 4


def gn_pix_per_block(N: int, HW: int, C: int) -> int:
    """csrc/norm.hip gn_pix_per_block()"""
    C8 = C // 8
    ppp = 1 if C8 >= 256 else 256 // C8
    nb = max(1, (1024 + N - 1) // N)
    ppb = max((HW + nb - 1) // nb, 4 * ppp)
    return (ppb + ppp - 1) // ppp * ppp


def mod_splits(T: int, D: int, B: int) -> int:
    """csrc/flux.hip mod_splits(): token splits of the adaLN modulation-gradient reduction"""
    xb = (D // 8 + 255) // 256
    return min(max(1, 512 // max(1, xb * B)), max(1, (T + 63) // 64))


# ------------------------------------------------------------------------------------------
# case tables: the smallest shapes that still reach each path
LN_WIDTHS = {8: (1, 1), 16: (2, 1), 24: (3, 1), 32: (4, 1), 40: (5, 1), 320: (5, 8), 768: (3, 32), 1024: (4, 32),
             1280: (5, 32), 1536: (3, 64), 2048: (4, 64)}
# the remaining lane counts of CPL 3 / 4 / 5 (L is a run-time argument of the same instantiations), so that the
# table holds every reachable (CPL, L); run at two row counts only
LN_WIDTHS_MORE = {48: (3, 2), 96: (3, 4), 192: (3, 8), 384: (3, 16), 64: (4, 2), 128: (4, 4), 256: (4, 8),
                  512: (4, 16), 80: (5, 2), 160: (5, 4), 640: (5, 16)}
LN_FALLBACK = (56, 1000, 1152, 1992)


def ln_cases():
    """(C, rows): 1, rows-per-block +- 1, 31 (one parameter-gradient slab), 77, 333 (ragged slabs, both loops of
    ln_param_part_kernel); 1027 at the narrowest and the widest width; 2051 at C = 56 (the fallback's grid stride)"""
    out = []
    for C in list(LN_WIDTHS) + list(LN_FALLBACK):
        rpb = ln_rows_per_block(C)
        rows = sorted({1, rpb - 1, rpb + 1, 31, 77, 333} - {0})
        if C in (8, 2048):
            rows.append(1027)
        if C == 56:
            rows.append(2051)
        out += [(C, r) for r in rows]
    for C in LN_WIDTHS_MORE:
        out += [(C, ln_rows_per_block(C) + 1), (C, 77)]
    return out


GN_SHAPES = [(2, 63, 320, 32), (1, 1, 64, 32), (3, 100, 8, 1), (1, 4100, 128, 32), (2, 36, 2560, 32),
             (1, 20, 4096, 32), (1, 9, 2056, 8), (2, 49, 960, 32)]
GN_MODES = [(True, 1e-5), (False, 1e-5), (True, 1e-6), (False, 1e-6)]   # (silu, eps)
ADALN_SHAPES = [(7, 3, 8), (37, 3, 256), (5, 2, 3072), (3, 1, 4096), (66, 4, 1000), (130, 2, 3072)]
INPUTS = ("plain", "row_scales", "big_mean", "constant", "tiny", "outlier")


# ------------------------------------------------------------------------------------------
# inputs: named generators (shape, seed) -> bf16 [..., rows, C]; "row" is the index of dim -2 (the pixel for GroupNorm)
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, g):
    return torch.randn(shape, generator=g, dtype=torch.float64)


def _row_pow(shape, period=17):
    r = torch.arange(shape[-2], dtype=torch.float64)
    return (2.0 ** ((r % period) - period // 2)).view(-1, 1)


def in_plain(shape, seed, groups=None):
    return (_randn(shape, _gen(seed)) * 2 + 0.5).to(BF)


def in_row_scales(shape, seed, groups=None):
    """row r times 2^((r % 17) - 8): what a whole-tensor metric cannot see"""
    return ((_randn(shape, _gen(seed)) * 2 + 0.5) * _row_pow(shape)).to(BF)


def in_big_mean(shape, seed, groups=None):
    """40 + 0.5 N(0, 1): the bf16 grid is 0.25 there, so x - mean is real cancellation"""
    return (40 + 0.5 * _randn(shape, _gen(seed))).to(BF)


def in_constant(shape, seed, groups=None):
    """every third row (LayerNorm / adaLN) or every third (image, group) (GroupNorm) exactly constant: variance 0"""
    g = _gen(seed)
    x = (_randn(shape, g) * 2 + 0.5).to(BF)
    if groups is None:
        x[..., 0::3, :] = x[..., 0::3, :1]
    else:
        N, HW, C = shape
        xg = x.view(N, HW, groups, C // groups)
        for n in range(N):
            for gi in range(groups):
                if (n + gi) % 3 == 0:
                    xg[n, :, gi, :] = xg[n, 0, gi, 0]
    return x


def in_tiny(shape, seed, groups=None):
    """magnitudes around 2^-20: variance far below eps"""
    return ((_randn(shape, _gen(seed)) * 2 + 0.5) * 2.0 ** -20).to(BF)


def in_outlier(shape, seed, groups=None):
    """one element 2^10 among 2^-6 noise per row"""
    x = _randn(shape, _gen(seed)) * 2.0 ** -6
    C = shape[-1]
    flat = x.view(-1, C)
    r = torch.arange(flat.shape[0])
    flat[r, (r * 7 + 3) % C] = 2.0 ** 10
    return x.to(BF)


GENERATORS = {"plain": in_plain, "row_scales": in_row_scales, "big_mean": in_big_mean, "constant": in_constant,
              "tiny": in_tiny, "outlier": in_outlier}


def params(C, seed, hard):
    """(gamma, beta) bf16.  hard: gamma with zeros and negative entries, beta large against gamma"""
    g = _gen(seed)
    if not hard:
        return (_randn((C,), g) * 0.5 + 1).to(BF), (_randn((C,), g) * 0.5).to(BF)
    gamma = _randn((C,), g) * 0.5 + 0.75
    gamma[0::5] = 0
    gamma[1::7] = -gamma[1::7].abs() - 0.25
    return gamma.to(BF), (_randn((C,), g) * 8).to(BF)


def grads(shape, seed, hard):
    """(dy, dres, previous dx) bf16; hard: dy with row scales too"""
    dy = in_plain(shape, seed + 1)
    if hard:   # period 13 against the 17 of x: the rows of dx = rstd (...) then span 2^-14 .. 2^14
        dy = (dy.double() * _row_pow(shape, 13)).to(BF)
    return dy, in_plain(shape, seed + 2), in_row_scales(shape, seed + 3)


# ------------------------------------------------------------------------------------------
# float64 references
def _dsilu(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def rownorm_reference(x, w, b, eps, dy):
    """y = (x - mean) rstd w + b over the last dim of x [R, C]; w, b float64 [C] or [R, C] (leaves or functions of
    leaves that want gradients).  Autograd runs here; returns the hand-written pieces the bounds need."""
    xd = x.double().requires_grad_(True)
    mean = xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(-1, keepdim=True)
    rstd = (var + eps).rsqrt()
    y = (xd - mean) * rstd * w + b
    y.backward(dy.double())
    with torch.no_grad():
        xv, dyd, wd, bd = xd.detach(), dy.double(), w.detach(), b.detach()
        xhat = (xv - mean) * rstd
        g = dyd * wd
        m1, m2 = g.mean(-1, keepdim=True), (g * xhat).mean(-1, keepdim=True)
        C = x.shape[-1]
        r = {"y": y.detach(), "mean": mean.detach()[:, 0], "rstd": rstd.detach()[:, 0], "dx": xd.grad,
             "dx_hand": rstd * (g - m1 - xhat * m2), "xhat": xhat,
             "M_y": rstd * wd.abs() * (xv.abs() + mean.abs()) + bd.abs(),
             "M_dx": rstd * (g.abs() + g.abs().mean(-1, keepdim=True)
                             + xhat.abs() * (g * xhat).abs().mean(-1, keepdim=True)),
             # the fused form dx = A g + B x + Cc, B = rstd^3 (mean mean(g) - mean(g x)), Cc = -B mean - rstd mean(g),
             # which torch's CPU LayerNorm backward evaluates (the kernels are not entitled to it: it cancels at a
             # large mean); used only to hold torch's fp32 autograd to a bound of its own formula
             "M_dx_fused": rstd * g.abs() + rstd * g.abs().mean(-1, keepdim=True)
             + rstd ** 3 * (xv.abs() + mean.abs()) * (mean.abs() * g.abs().mean(-1, keepdim=True)
                                                      + (g * xv).abs().mean(-1, keepdim=True)),
             # dy xhat per element, and the evaluation allowance of that term
             "t_scale": dyd * xhat, "e_scale": U17 * dyd.abs() * rstd * (xv.abs() + mean.abs()), "t_shift": dyd,
             "mean_abs_x": xv.abs().mean(-1),
             "rstd_cond": 1 + (xv ** 2).sum(-1) / (C * (var.detach()[:, 0] + eps))}
    return {k: v.detach() for k, v in r.items()}


def rownorm_fp32(x, w, b, eps, dy):
    """the formulas the row kernels are entitled to, evaluated honestly in fp32 (two-pass statistics, torch's CPU
    float32 reductions); w, b float32 [C] or [R, C].  Returns fp32 (y, mean, rstd, dx, dy xhat)"""
    xf, dyf = x.float(), dy.float()
    mean = xf.mean(-1, keepdim=True)
    d = xf - mean
    rstd = torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
    xhat = d * rstd
    g = dyf * w
    dx = rstd * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    return xhat * w + b, mean[:, 0], rstd[:, 0], dx, dyf * xhat


def layernorm_reference(x, gamma, beta, eps, dy):
    w, b = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    r = rownorm_reference(x, w, b, eps, dy)
    R = x.shape[0]
    r.update(dgamma=w.grad, dbeta=b.grad, dgamma_hand=r["t_scale"].sum(0), dbeta_hand=r["t_shift"].sum(0),
             B_dgamma=R * U24 * r["t_scale"].abs().sum(0) + r["e_scale"].sum(0),
             B_dbeta=R * U24 * r["t_shift"].abs().sum(0))
    return r


def adaln_reference(x, mod, shift_off, scale_off, B, eps, dy):
    """LN(x) (1 + scale[b]) + shift[b], row r of sample r % B; mod [B, ldm] bf16.  dshift / dscale: [B, D]"""
    R, D = x.shape
    T = R // B
    md = mod.double().requires_grad_(True)
    w = (1 + md[:, scale_off:scale_off + D]).repeat(T, 1)
    b = md[:, shift_off:shift_off + D].repeat(T, 1)
    r = rownorm_reference(x, w, b, eps, dy)
    per = lambda t: t.view(T, B, D)   # noqa: E731
    r.update(dshift=md.grad[:, shift_off:shift_off + D], dscale=md.grad[:, scale_off:scale_off + D],
             dshift_hand=per(r["t_shift"]).sum(0), dscale_hand=per(r["t_scale"]).sum(0),
             B_dscale=T * U24 * per(r["t_scale"]).abs().sum(0) + per(r["e_scale"]).sum(0),
             B_dshift=T * U24 * per(r["t_shift"]).abs().sum(0), dmod_rest=md.grad)
    return r


def groupnorm_reference(x, gamma, beta, G, eps, silu, dy):
    """x [N, HW, C] bf16, gamma / beta bf16 [C] or None (1 / 0)"""
    N, HW, C = x.shape
    Cg = C // G
    xd = x.double().requires_grad_(True)
    w = (torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()).requires_grad_(True)
    b = (torch.zeros(C, dtype=torch.float64) if beta is None else beta.double()).requires_grad_(True)
    xg = xd.view(N, HW, G, Cg)
    mean = xg.mean((1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean((1, 3), keepdim=True)
    rstd = (var + eps).rsqrt()
    z = ((xg - mean) * rstd).reshape(N, HW, C) * w + b
    y = z * torch.sigmoid(z) if silu else z
    y.backward(dy.double())
    with torch.no_grad():
        ch = lambda t: t.expand(N, 1, G, Cg).reshape(N, 1, C)   # noqa: E731  per (n, g) -> per (n, channel)
        xv, dyd, wd, bd = xd.detach(), dy.double(), w.detach(), b.detach()
        mc, rc = ch(mean), ch(rstd)
        xhat = (xv - mc) * rc
        a = rc * wd
        bb = bd - mc * a
        zz = xv * a + bb
        M_z = (xv * a).abs() + bb.abs()
        dz = dyd * _dsilu(zz) if silu else dyd
        E_dz = U17 * (dz.abs() + 0.5 * dyd.abs() * M_z) if silu else torch.zeros_like(dz)
        grp = lambda t: t.view(N, HW, G, Cg).mean((1, 3), keepdim=True)   # noqa: E731
        c1, c2 = ch(grp(wd * dz)), ch(grp(wd * dz * xhat))
        gsum = lambda t: ch(grp(t))   # noqa: E731
        A, Bc, Cc = a, -rc * rc * c2, rc * (mc * rc * c2 - c1)
        R = N * HW
        e_xhat = U17 * dz.abs() * rc * (xv.abs() + mc.abs())
        r = {"y": y, "mean": mean.reshape(N * G), "rstd": rstd.reshape(N * G), "dx": xd.grad,
             "dx_hand": A * dz + Bc * xv + Cc, "dgamma": w.grad, "dbeta": b.grad,
             "mean_abs_x": xv.abs().view(N, HW, G, Cg).mean((1, 3)).reshape(N * G),
             "rstd_cond": (1 + (xv ** 2).view(N, HW, G, Cg).mean((1, 3), keepdim=True) / (var + eps)).reshape(N * G),
             "dgamma_hand": (dz * xhat).sum((0, 1)), "dbeta_hand": dz.sum((0, 1)),
             "M_y": 1.1 * M_z + y.abs() if silu else M_z,
             "M_dx": (A * dz).abs() + (Bc * xv).abs() + rc * ((mc * rc * c2).abs() + c1.abs()) + A.abs() * E_dz / U17
             + rc * (gsum(wd.abs() * (dz.abs() + E_dz / U17))
                     + xhat.abs() * gsum(wd.abs() * (dz.abs() + E_dz / U17) * xhat.abs())),
             # torch's CPU backward gets B from rstd^3 (mean mean(gamma dz) - mean(gamma dz x)): the bound of that
             # formula, used only for torch's fp32 autograd
             "M_dx_fused": (A * dz).abs() + A.abs() * E_dz / U17 + rc * ch(grp((wd * dz).abs()))
             + rc ** 3 * (xv.abs() + mc.abs()) * (mc.abs() * ch(grp((wd * dz).abs())) + ch(grp((wd * dz * xv).abs()))),
             "B_dgamma": R * U24 * (dz * xhat).abs().sum((0, 1)) + (E_dz * xhat.abs() + e_xhat).sum((0, 1)),
             "B_dbeta": R * U24 * dz.abs().sum((0, 1)) + E_dz.sum((0, 1))}
    return {k: v.detach() for k, v in r.items()}


def groupnorm_fp32(x, gamma, beta, G, eps, silu, dy):
    """the formulas the GroupNorm kernels are entitled to, evaluated honestly in fp32: statistics folded in double
    and rounded to fp32, then a = rstd gamma, b = beta - mean a, z = x a + b, dx = A dz + B x + Cc with fp32
    group means.  Returns fp32 (y, mean, rstd, dx, dgamma, dbeta)"""
    N, HW, C = x.shape
    Cg = C // G
    xg = x.double().view(N, HW, G, Cg)
    m64 = xg.mean((1, 3), keepdim=True)
    mean = m64.float()
    rstd = ((xg * xg).mean((1, 3), keepdim=True) - m64 * m64).clamp_min(0).add(eps).rsqrt().float()
    ch = lambda t: t.expand(N, 1, G, Cg).reshape(N, 1, C)   # noqa: E731
    grp = lambda t: ch(t.view(N, HW, G, Cg).mean((1, 3), keepdim=True))   # noqa: E731
    xf, dyf = x.float(), dy.float()
    w = torch.ones(C) if gamma is None else gamma.float()
    b = torch.zeros(C) if beta is None else beta.float()
    mc, rc = ch(mean), ch(rstd)
    a = rc * w
    bb = b - mc * a
    z = xf * a + bb
    y = z * torch.sigmoid(z) if silu else z
    dz = dyf * _dsilu(z) if silu else dyf
    xhat = (xf - mc) * rc
    c1, c2 = grp(w * dz), grp(w * dz * xhat)
    dx = a * dz + ((-rc * rc * c2) * xf + rc * (mc * rc * c2 - c1))
    return y, mean.reshape(-1), rstd.reshape(-1), dx, (dz * xhat).sum((0, 1)), dz.sum((0, 1))


# ------------------------------------------------------------------------------------------
# the checks: every element, worst offender named
def whole(got, ref) -> float:
    """the metric of test_kernels_gpu.py / test_flux_gpu.py: max|got - ref| / max|ref| over the whole tensor"""
    return float((got.double().cpu() - ref).abs().max() / (ref.abs().max() + 1e-6))


def _fail(what, err, tol, got, ref):
    over = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err - tol)
    i = int(over.argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), err.shape))
    n = int((~(err <= tol)).sum())
    raise AssertionError(f"{what}: {n} of {err.numel()} elements out of bound; worst at {idx}: got "
                         f"{float(got.flatten()[i])!r} ref {float(ref.flatten()[i])!r} |d| {float(err.flatten()[i]):.3e} "
                         f"bound {float(tol.flatten()[i]):.3e}")


def check_abs(got, ref, tol, what):
    """|got - ref| <= tol on every element (a NaN fails)"""
    got = got.detach().double().cpu().reshape(ref.shape)
    tol = tol.expand_as(ref) if isinstance(tol, torch.Tensor) else torch.full_like(ref, tol)
    err = (got - ref).abs()
    if not bool((err <= tol).all()):
        _fail(what, err, tol, got, ref)


def check_elem(got, ref, M, what, rnd=U8):
    """one output rounding (bf16: 2^-8 |ref|) plus 2^-17 M"""
    check_abs(got, ref, rnd * ref.abs() + U17 * M.expand_as(ref), what)


def check_col(got, ref, bound, what, prev=None):
    """a column reduction into its destination's dtype; prev: the destination's earlier content (param_acc): the
    fp32 sum with the new value is rounded (2^-24) and stored in the destination's dtype"""
    rnd = U8 if got.dtype == BF else U24
    if prev is not None:
        ref = ref + prev.double().cpu()
        rnd += U24
    check_abs(got, ref, bound + rnd * ref.abs(), what)


def check_row_stats(mean, rstd, r, what):
    """saved LayerNorm / adaLN statistics (fp32)"""
    check_abs(mean, r["mean"], U17 * r["mean_abs_x"], what + " mean")
    check_abs(rstd.double().cpu() / r["rstd"], torch.ones_like(r["rstd"]), U17 * r["rstd_cond"] + U22, what + " rstd")


def check_group_stats(mean, rstd, r, what):
    """GroupNorm statistics are folded in double and rounded to fp32: the fp32 rounding of the float64 value, times 4.
    What is folded are fp32 partial sums of x and x^2 (one pass), so the bounds of the row statistics apply on top:
    2^-17 mean|x| on the mean (a group mean cancels: torch's fp32 mean is 23 ulps of the result off on row_scales)
    and 2^-17 (1 + sum x^2 / (cnt (var + eps))) on rstd."""
    check_abs(mean, r["mean"], 4 * U24 * r["mean"].abs() + U17 * r["mean_abs_x"], what + " mean")
    check_abs(rstd.double().cpu() / r["rstd"], torch.ones_like(r["rstd"]), 4 * U24 + U17 * r["rstd_cond"],
              what + " rstd")


# ------------------------------------------------------------------------------------------
# guarded destinations: NaN-filled buffers with a guard row above and below and guard columns left and right
def guarded(lead, rows, C, ld=None, device="cpu"):
    """(buffer [*lead, rows + 2, ld], the [*lead, rows, C] slice at row 1, column 8)"""
    ld = C + 16 if ld is None else ld
    buf = torch.full((*lead, rows + 2, ld), math.nan, dtype=BF, device=device)
    return buf, buf[..., 1:rows + 1, 8:8 + C]


def guards_intact(buf, rows, C) -> bool:
    """everything outside the slice still holds the fill's bits"""
    bits = buf.cpu().view(torch.int16).clone()
    bits[..., 1:rows + 1, 8:8 + C] = NANBITS
    return bool((bits == NANBITS).all())


def wide(t, ld, off=0):
    """t as a column slice (offset off) of a [*, ld] buffer filled with NaN"""
    buf = torch.full((*t.shape[:-1], ld), math.nan, dtype=t.dtype, device=t.device)
    buf[..., off:off + t.shape[-1]] = t
    return buf[..., off:off + t.shape[-1]]


# ------------------------------------------------------------------------------------------
# cases: operands and the reference, built once per key
class Case:
    pass


def _seed(*k):
    s = 12345
    for v in k:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return s


@functools.lru_cache(maxsize=4)
def ln_case(C, rows, inp, eps=1e-5):
    c = Case()
    hard = inp != "plain"
    s = _seed(C, rows, INPUTS.index(inp))
    c.C, c.rows, c.eps, c.name = C, rows, f32(eps), f"layernorm C={C} rows={rows} {inp}"
    c.x = GENERATORS[inp]((rows, C), s)
    c.gamma, c.beta = params(C, s + 7, hard)
    c.dy, c.dres, c.prev = grads((rows, C), s, hard)
    g = _gen(s + 9)
    c.pg, c.pb = (_randn((C,), g) * 4).to(BF), (_randn((C,), g) * 4).to(BF)   # earlier content for param_acc
    c.ref = layernorm_reference(c.x, c.gamma, c.beta, c.eps, c.dy)
    return c


@functools.lru_cache(maxsize=4)
def gn_case(N, HW, C, G, silu, eps, inp, affine=True):
    c = Case()
    hard = inp != "plain"
    s = _seed(N, HW, C, G, INPUTS.index(inp))
    c.N, c.HW, c.C, c.G, c.silu, c.eps = N, HW, C, G, silu, f32(eps)
    c.name = f"groupnorm N={N} HW={HW} C={C} G={G} silu={silu} eps={eps} {inp}" + ("" if affine else " no affine")
    c.x = GENERATORS[inp]((N, HW, C), s, groups=G)
    c.gamma, c.beta = params(C, s + 7, hard) if affine else (None, None)
    c.dy, c.dres, c.prev = grads((N, HW, C), s, hard)
    g = _gen(s + 9)
    c.pg, c.pb = (_randn((C,), g) * 4).to(BF), (_randn((C,), g) * 4).to(BF)
    c.ref = groupnorm_reference(c.x, c.gamma, c.beta, G, c.eps, silu, c.dy)
    return c


@functools.lru_cache(maxsize=4)
def adaln_case(T, B, D, inp, eps=1e-6):
    """modulation buffer 6 D wide, shift at 3 D and scale at 4 D"""
    c = Case()
    hard = inp != "plain"
    s = _seed(T, B, D, INPUTS.index(inp), 3)
    c.T, c.B, c.D, c.eps, c.name = T, B, D, f32(eps), f"adaln T={T} B={B} D={D} {inp}"
    c.shift_off, c.scale_off = 3 * D, 4 * D
    c.x = GENERATORS[inp]((T * B, D), s)
    g = _gen(s + 7)
    c.mod = (_randn((B, 6 * D), g) * (2.0 if hard else 0.5)).to(BF)
    if hard:   # 1 + scale exactly zero and negative in places
        c.mod[:, c.scale_off:c.scale_off + D:5] = -1
    c.dy, c.dres, _ = grads((T * B, D), s, hard)
    c.ref = adaln_reference(c.x, c.mod, c.shift_off, c.scale_off, B, c.eps, c.dy)
    return c
