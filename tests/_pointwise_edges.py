"""Shared pieces of the pointwise / row kernel edge tests (test_pointwise_edges_gpu.py, test_pointwise_edges_ref.py):
float64 references of the kernels of csrc/flux.hip (without adaLN), csrc/text.hip (without the masked softmax) and
csrc/elementwise.hip, their element-wise bounds, inputs and case tables.  Plain PyTorch on the CPU, seeded CPU
generators; the rule of the bounds is the one at the top of _norm_edges.py: one rounding of the destination
(bf16: 2^-8 |ref|) plus 2^-17 M, M the float64 sum of the absolute terms of the formula the kernel is entitled to;
sums over R terms add R 2^-24 sum|term|; a bf16 destination and an accumulation onto a prior value add their own
rounding.  Every `*_math` below is written once over a dtype: in float64 it is the reference, in float32 it is the
honest evaluation that test_pointwise_edges_ref.py holds to the same bounds.  TINY = 2^-126 is added where a result
can be subnormal (the device may flush it to zero).

qknorm_rope forward   rr = rsqrt(mean_128(x^2) + eps), n_j = x_j rr w_j,
                      out_2i = n_2i c_2i - n_2i+1 s_2i, out_2i+1 = n_2i+1 c_2i+1 + n_2i s_2i+1
                      M = the two absolute products.  (rr is a sum of 128 positive terms and one rsqrt: a few ulps of
                      relative error, inside 2^-17 of every product.)
qknorm_rope backward  dn = rope^T(dy): dn_2i = g_2i c_2i + g_2i+1 s_2i+1, dn_2i+1 = g_2i+1 c_2i+1 - g_2i s_2i;
                      A = the two absolute products of dn.  v = dn w, dx = rr (v - xhat mean(v xhat)),
                      M = rr (A |w| + |xhat| mean(A |w| |xhat|)).
                      dw[type][c] = sum over the rows of the type and the H heads of dn xhat: R = rows H terms,
                      bound R 2^-24 sum(A |xhat|) + 2^-17 sum(A |xhat|) (the second part: the evaluation of the terms).
                      Types (q_img, k_img, q_ctx, k_ctx); a row is ctx iff r // B < L and ctx weights are given.
gated add             out = x + gate[b] y (one fma): M = |x| + |gate y|.  dy = gate[b] dout, one product: one bf16
                      rounding plus one fp32 ulp.  dgate[b][c] = sum_t dout y: T 2^-24 sum|dout y|, then bf16.
gelu_tanh, act kind 2 y = 0.5 x (1 + tanh(u)), u = sqrt(2/pi) (x + 0.044715 x^3).  On the negative tail 1 + tanh(u)
                      cancels: tanhf is k ulps (2^-24 at -1) off, which no relative bound covers, so the bound gets
                      the absolute floor K 2^-24 |x| (per unit of upstream gradient).  k is the worst error of the
                      CPU fp32 evaluation over the sweep beyond the relative part 2^-17 |y|, in units of 2^-24 |x|:
                      0.249, taken as 0.3 (one decimal up, so that another libm's last bit does not move it), and
                      K_TANH = 4 k = 1.2 for the device library (test_activation_floors_measured holds K to 4 k).
                      The derivative is 0.5 (1 + th) + 0.5 x (1 - th^2) du, du = sqrt(2/pi) (1 + 0.134145 x^2):
                      1 - th^2 cancels too and moves by 2 |th| k 2^-24, so the floor of the backward is
                      K 2^-24 (0.5 + |x| du) per unit of dy.  In those units the CPU fp32 derivative shows k = 0.468,
                      taken as 0.5: K_TANH_BWD = 2.  In units of |x| alone it shows 1.75 at x = -5.16 (du = 3.6
                      there), above K_TANH: the |x| form does not hold an honest evaluation, and the ref file says so.
act kind 1 (erf)      y = 0.5 x (1 + erf(x / sqrt 2)): the same, k = 0.453, taken as 0.5, K_ERF = 2.
act kind 0, SiLU      y = x / (1 + e), e = exp(-a), a = 1.702 x (quick_gelu) or x (SiLU): no cancellation, the plain
                      relative bound.  The fast exponential takes 2^(a log2 e): the rounded argument moves e by
                      |a| 2^-24 relative, the hardware exp2 and rcp by an ulp each; y moves by e / (1 + e) of that:
                      M = |y| (1 + (|a| + 2) e / (1 + e) / 64)   [2^-17 / 64 = 2 x 2^-24].
                      dsilu = s (1 + x (1 - s)): s carries E_s = s 2^-24 (2 + 2 (1 - s) (|x| + 2)),
                      bound |1 + x - 2 x s| E_s + 2^-17 s (1 + |x| (1 - s)).
GEGLU                 out = a g Phi(g).  The kernel takes Phi from Abramowitz & Stegun 7.1.26 (common.h), whose
                      published error is 1.5e-7 on erf, 0.75e-7 on Phi, absolute: the honest formula is that one.
                      The tail 0.5 poly e^(-z^2) in fp32: (z^2 + 8) ulps of itself, at most 5 x 2^-24 absolute.
                      E_CDF = 0.75e-7 + 5 x 2^-24 per unit of |a g|.  Backward: da = d g Phi (the same), dg = d a (Phi +
                      g pdf), pdf = e^(-g^2/2) / sqrt(2 pi) with |g| pdf (g^2 / 2 + 2) <= 0.6 ulps: E_CDF + 0.6 x 2^-24.
rmsnorm               y = bf16(x rs) w, rs = rsqrt(mean(x^2) + eps): the intermediate rounding may land on either side
                      of a tie, so an element passes if it is within one bf16 rounding of w bf16(n (1 +- 2^-17)) for
                      either sign, n the float64 normalised value.
bit-exact             embed_tokens (fp32 add of two bf16, RNE), add, cast_f32 (one fp32 add when accumulating),
                      concat_channels, flux_pack / unpack, conv_weight_transpose, image_to_nhwc at mul 2, add -1
                      (2 x is exact, so the fma is one rounding); padded channels are +0.  General mul:
                      2^-8 |ref| + 2^-23 (|x mul| + |add|).
timestep_embedding    a = t exp(-ln(10000) k / half) in fp32, [cos a | sin a]: 2^-8 |ref| + |a| 2^-21 (the error of the
                      argument through |d cos| <= 1).
upsample2x_bwd        four bf16 (five with the prior value) summed in fp32: R 2^-24 sum|term|, then bf16.
colsum                per column R 2^-24 sum|x| over the R rows of the group, plus destination / accumulate rounding."""
import functools
import math

import torch

import _norm_edges as N
from _norm_edges import BF, NANBITS, U8, U17, U24, Case, _gen, _randn, _seed, f32, guarded, guards_intact, whole, wide  # noqa: F401

F64, F32 = torch.float64, torch.float32
TINY = 2.0 ** -126
K_TANH, K_ERF, K_TANH_BWD = 1.2, 2.0, 2.0   # 4 x (0.3, 0.5, 0.5): the docstring
# the k behind them: the largest the CPU fp32 evaluation has shown (torch's erf is another vector routine on other
# CPUs and shows 0.240 there)
K_MEASURED = {"tanh": 0.249, "erf": 0.453, "tanh derivative": 0.468}
E_CDF = 0.75e-7 + 5 * U24
GRID_CAP = 16384          # blocks of every grid-stride kernel here (flux.hip gfor, text.hip / elementwise.hip grid_for)
QK_BWD_CAP = 1024         # blocks of 4 waves of qknorm_rope_bwd_kernel
mod_splits = N.mod_splits


def colsum_rpb(rpg: int, ncols: int, groups: int) -> int:
    """csrc/elementwise.hip colsum_rpb(): rows one first-pass block sums"""
    cb = (ncols + 255) // 256
    rpb = rpg
    while rpb > 128 and cb * groups * ((rpg + rpb - 1) // rpb) < 2048:
        rpb = (rpb + 1) // 2
    return rpb


# ------------------------------------------------------------------------------------------
# the checks: every element, the worst |err| / bound per kernel kept for the report
WORST: dict = {}


def note(kernel, ratio, what):
    if kernel not in WORST or not ratio <= WORST[kernel][0]:
        WORST[kernel] = (ratio, what)


def check(kernel, got, ref, tol, what):
    got = got.detach().double().cpu().reshape(ref.shape)
    tol = tol.expand_as(ref) if isinstance(tol, torch.Tensor) else torch.full_like(ref, tol)
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    note(kernel, float(ratio.max()) if ratio.numel() else 0.0, what)
    if not bool((err <= tol).all()):
        N._fail(what, err, tol, got, ref)


def check_elem(kernel, got, ref, M, what, floor=0.0):
    check(kernel, got, ref, U8 * ref.abs() + U17 * M + floor, what)


def check_col(kernel, got, ref, bound, what, prev=None):
    """N.check_col with the ratio kept"""
    rnd = U8 if got.dtype == BF else U24
    if prev is not None:
        ref = ref + prev.double().cpu()
        rnd += U24
    check(kernel, got, ref, bound + rnd * ref.abs(), what)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def check_bits(kernel, got, ref, what):
    ok = got.shape == ref.shape and got.dtype == ref.dtype and torch.equal(bits(got), bits(ref))
    note(kernel, 0.0 if ok else math.inf, what)
    if not ok:
        bad = bits(got) != bits(ref)
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ in bits; first at flat index "
                             f"{i}: got {float(got.flatten()[i])!r} ref {float(ref.flatten()[i])!r}")


def interleave(e, o):
    return torch.stack([e, o], -1).flatten(-2)


# ------------------------------------------------------------------------------------------
# qknorm_rope
QK_SHAPES = [(1, 1, 1, 0), (2, 1, 1, 1), (3, 1, 3, 1), (29, 2, 2, 5), (7, 3, 24, 7), (7, 3, 24, 0), (1030, 2, 1, 5)]
QK_INPUTS = ("plain", "head_scales", "zero_head", "outlier")
QK_DW_SHAPES = [(29, 2, 2, 5), (1030, 2, 1, 5)]
QK_DW_MODES = ("f32", "f32_acc", "bf16", "bf16_acc", "only_dwk", "none")


def qk_geom(H):
    """x is a view with q at 4 and k at H 128 + 12 of rows 3 H 128 + 8 wide; dx goes to 8 and H 128 + 12 of a wider
    buffer (both k offsets are 4 mod 8: 8-byte but not 16-byte aligned)"""
    return {"ldx": 3 * H * 128 + 8, "qoff": 4, "koff": H * 128 + 12, "lddx": 3 * H * 128 + 24, "dxqoff": 8,
            "dxkoff": H * 128 + 12, "lddy": 2 * H * 128 + 8}


def qk_math(c, dt, plant=None):
    """x [rows, 2, H, 128] (q | k), dy likewise, w [4, 128], cs / sn [T, 128] -> out, dx [rows, 2, H, 128], dw [4, 128]
    and the M / bound terms; every operation in dtype dt"""
    x, dy, w, cs, sn = (t.to(dt) for t in (c.xq, c.dyq, c.w, c.cs, c.sn))
    rows, B, H, L = c.rows, c.B, c.H, c.L
    t = torch.arange(rows) // B
    isctx = (t < (L + 1 if plant == "ctx_row_L" else L)) & c.ctx
    wt = torch.stack([w[0 + 2 * isctx.long()], w[1 + 2 * isctx.long()]], 1)[:, :, None, :]   # [rows, 2, 1, 128]
    rr = torch.rsqrt((x * x).mean(-1, keepdim=True) + c.eps)
    xh = x * rr
    n = xh * wt
    cc, ss = cs[t][:, None, None, :], sn[t][:, None, None, :]
    ev, od = (lambda v: v[..., 0::2]), (lambda v: v[..., 1::2])
    co = ev(cc) if plant == "rope_cos_even" else od(cc)
    out = interleave(ev(n) * ev(cc) - od(n) * ev(ss), od(n) * co + ev(n) * od(ss))
    M_out = interleave((ev(n) * ev(cc)).abs() + (od(n) * ev(ss)).abs(), (od(n) * co).abs() + (ev(n) * od(ss)).abs())
    dn = interleave(ev(dy) * ev(cc) + od(dy) * od(ss), od(dy) * od(cc) - ev(dy) * ev(ss))
    A = interleave((ev(dy) * ev(cc)).abs() + (od(dy) * od(ss)).abs(), (od(dy) * od(cc)).abs() + (ev(dy) * ev(ss)).abs())
    v = dn * wt
    dx = rr * (v - xh * (v * xh).mean(-1, keepdim=True))
    M_dx = rr * (A * wt.abs() + xh.abs() * (A * wt.abs() * xh.abs()).mean(-1, keepdim=True))
    term, aterm = dn * xh, A * xh.abs()
    if plant == "odd_H_skip" and H % 2:   # the upper half-wave's last head step (head H - 2) never runs
        dx = dx.clone()
        dx[:, :, H - 2] = 0
        term = term.clone()
        term[:, :, H - 2] = 0
    dw, B_dw = torch.zeros(4, 128, dtype=dt), torch.zeros(4, 128, dtype=F64)
    for isk in range(2):
        for cx in range(2):
            m = isctx == bool(cx)
            ty = isk + 2 * cx
            if plant == "dw_second_sweep":   # waves past the first sweep of the 1024 x 4 grid add into the other stream
                first = (2 * torch.arange(rows) + isk) < 4 * QK_BWD_CAP
                dw[ty] = term[m & first, isk].sum((0, 1)) + term[(isctx != bool(cx)) & ~first, isk].sum((0, 1))
            else:
                dw[ty] = term[m, isk].sum((0, 1))
            B_dw[ty] = (int(m.sum()) * H * U24 + U17) * aterm[m, isk].double().sum((0, 1))
    return {"out": out, "M_out": M_out, "dx": dx, "M_dx": M_dx, "dw": dw, "B_dw": B_dw}


def qk_forward_autograd(c):
    """the forward alone in float64 under autograd -> (dx, dw)"""
    x, w = c.xq.double().requires_grad_(True), c.w.double().requires_grad_(True)
    t = torch.arange(c.rows) // c.B
    isctx = ((t < c.L) & c.ctx).long()
    wt = torch.stack([w[2 * isctx], w[1 + 2 * isctx]], 1)[:, :, None, :]
    n = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + c.eps) * wt
    cc, ss = c.cs.double()[t][:, None, None, :], c.sn.double()[t][:, None, None, :]
    ne, no = n[..., 0::2], n[..., 1::2]
    out = interleave(ne * cc[..., 0::2] - no * ss[..., 0::2], no * cc[..., 1::2] + ne * ss[..., 1::2])
    out.backward(c.dyq.double())
    return out.detach(), x.grad, w.grad


@functools.lru_cache(maxsize=4)
def qk_case(T, B, H, L, ctx, inp):
    c = Case()
    s = _seed(T, B, H, L, int(ctx), QK_INPUTS.index(inp), 11)
    g = _gen(s)
    rows = T * B
    c.T, c.B, c.H, c.L, c.ctx, c.rows, c.eps = T, B, H, L, ctx, rows, f32(1e-6)
    c.name = f"qknorm_rope T={T} B={B} H={H} L={L} {'ctx' if ctx else 'single'} {inp}"
    xq = _randn((rows, 2, H, 128), g)
    r = torch.arange(rows).view(-1, 1, 1, 1)
    k = torch.arange(2).view(1, 2, 1, 1)
    h = torch.arange(H).view(1, 1, H, 1)
    if inp == "head_scales":
        xq = xq * 2.0 ** (((h * 5 + r * 3 + k) % 17) - 8)
    elif inp == "zero_head":
        xq = xq * (h != r % H)
    elif inp == "outlier":
        xq = xq * 2.0 ** -6
        xq.view(-1, 128)[torch.arange(rows * 2 * H), (torch.arange(rows * 2 * H) * 7 + 3) % 128] = 2.0 ** 10
    c.xq = xq.to(BF)
    w = (1 + 0.3 * _randn((4, 128), g))
    w[:, 3] = 0
    w[:, 5] = -w[:, 5].abs() - 0.25
    c.w = w.to(BF)
    ang = (torch.rand((T, 128), generator=g, dtype=F64) * 2 - 1) * math.pi   # independent per element
    c.cs, c.sn = torch.cos(ang).float(), torch.sin(ang).float()
    dy = _randn((rows, 2, H, 128), g)
    if inp != "plain":
        dy = dy * 2.0 ** ((r % 13) - 6)
    c.dyq = dy.to(BF)
    c.pdw = (_randn((4, 128), g) * 4).to(BF)   # earlier content for dw_acc
    G = qk_geom(H)
    c.x = _randn((rows, G["ldx"]), g).to(BF)   # the q | k | v buffer the kernel reads
    c.x[:, G["qoff"]:G["qoff"] + H * 128] = c.xq[:, 0].reshape(rows, -1)
    c.x[:, G["koff"]:G["koff"] + H * 128] = c.xq[:, 1].reshape(rows, -1)
    c.dy = c.dyq.reshape(rows, 2 * H * 128)
    c.ref = qk_math(c, F64)
    return c


def qk_flat(t):
    """[rows, 2, H, 128] -> [rows, 2 H 128] = [q | k]"""
    return t.reshape(t.shape[0], -1)


# ------------------------------------------------------------------------------------------
# gated add
GA_SHAPES = [(1, 1, 8), (7, 3, 8), (37, 3, 256), (66, 4, 1000), (130, 2, 3072), (70, 1, 2056)]
GA_INPUTS = ("plain", "row_scales")


def ga_math(c, dt, plant=None):
    x, y, dout, mod = (t.to(dt) for t in (c.x, c.y, c.dout, c.mod))
    T, B, D = c.T, c.B, c.D
    r = torch.arange(T * B)
    g = mod[:, c.gate_off:c.gate_off + D][(r // T) if plant == "gate_row" else (r % B)]
    prod = (dout * y).view(T, B, D)
    keep = T
    if plant == "ragged_chunk":
        S = mod_splits(T, D, B)
        keep = (S - 1) * ((T + S - 1) // S) if S > 1 else T
    return {"out": x + g * y, "M_out": x.abs() + (g * y).abs(), "dy": g * dout, "dgate": prod[:keep].sum(0),
            "B_dgate": T * U24 * prod.double().abs().sum(0)}


@functools.lru_cache(maxsize=4)
def ga_case(T, B, D, inp):
    c = Case()
    s = _seed(T, B, D, GA_INPUTS.index(inp), 5)
    c.T, c.B, c.D, c.gate_off, c.ldm = T, B, D, 2 * D, 3 * D + 8
    c.name = f"gated_add T={T} B={B} D={D} {inp}"
    gen = N.GENERATORS[inp]
    c.x, c.y, c.dout = gen((T * B, D), s), gen((T * B, D), s + 1), gen((T * B, D), s + 2)
    c.mod = (_randn((B, c.ldm), _gen(s + 3)) * (0.5 if inp == "plain" else 2.0)).to(BF)
    c.ref = ga_math(c, F64)
    return c


# ------------------------------------------------------------------------------------------
# activations
ACT_SHAPES = [(1, 8), (7, 24), (77, 2048)]
C0, C1 = 0.7978845608028654, 0.044715


def act_input(shape, seed, silu=False):
    """bf16 [rows, C] holding +-0, +-2^-20, +-60 (SiLU: +-100 too) and a sweep of 2^11 values over [-12, 12]"""
    sp = [0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 60.0, -60.0] + ([100.0, -100.0] if silu else [12.0, -12.0])
    pool = torch.cat([torch.tensor(sp, dtype=F64), torch.linspace(-12, 12, 2 ** 11, dtype=F64)]).to(BF)
    n = shape[0] * shape[1]
    if n <= pool.numel():
        idx = torch.cat([torch.arange(8), 8 + torch.linspace(0, 2 ** 11 - 1, n - 8).long()])
    else:
        idx = torch.arange(n) % pool.numel()
        idx = idx[torch.randperm(n, generator=_gen(seed))]
    return pool[idx].view(shape)


def _phi(x):
    """Phi(x), pdf(x): float64 exactly; float32 as the kernel is entitled to (Abramowitz & Stegun 7.1.26)"""
    if x.dtype == F64:
        return 0.5 * torch.special.erfc(-x * math.sqrt(0.5)), torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    z = x.abs() * 0.70710678118654752
    t = 1 / (0.3275911 * z + 1)
    poly = t * (t * (t * (t * (t * 1.061405429 - 1.453152027) + 1.421413741) - 0.284496736) + 0.254829592)
    e = torch.exp(-z * z)
    tail = 0.5 * poly * e
    return torch.where(x < 0, tail, 1 - tail), 0.39894228040143268 * e


def act_math(kind, x, dt):
    """kind: 'quick', 'erf', 'tanh', 'silu' -> (y, dy/dx, E_y, E_d): values in dt, allowances (float64, without the
    destination's rounding) per unit of what multiplies them"""
    v = x.to(dt)
    xd = x.double()
    if kind in ("tanh", "erf"):
        if kind == "tanh":
            th = torch.tanh(C0 * (v + C1 * v * v * v))
            du = C0 * (1 + 3 * C1 * v * v)
            k = K_TANH
        else:
            th, du, k = torch.erf(v * 0.70710678118654752), None, K_ERF
        y = 0.5 * v * (1 + th)
        if kind == "tanh":
            d = 0.5 * (1 + th) + 0.5 * v * (1 - th * th) * du
            Md = (0.5 * (1 + th)).abs() + (0.5 * v * (1 - th * th) * du).abs()
            Ed = U17 * Md.double() + K_TANH_BWD * U24 * (0.5 + xd.abs() * du.double())
        else:
            d, Ed = None, None
        return y, d, U17 * y.double().abs() + k * U24 * xd.abs(), Ed
    a = v * 1.702 if kind == "quick" else v
    s, s1 = torch.sigmoid(a), torch.sigmoid(-a)   # s1 = e / (1 + e)
    y = v * s
    Ey = y.double().abs() * U17 * (1 + (a.double().abs() + 2) * s1.double() / 64)
    if kind == "quick":
        return y, None, Ey, None
    d = s * (1 + v * s1)
    Es = s.double() * U24 * (2 + 2 * s1.double() * (xd.abs() + 2))
    Ed = (1 + xd - 2 * xd * s.double()).abs() * Es + U17 * s.double() * (1 + xd.abs() * s1.double())
    return y, d, Ey, Ed


def geglu_math(h, dout, dt):
    """h = [a | g] bf16 [M, 2F], dout [M, F] -> out, da, dg (dt) and their tolerances (float64, complete)"""
    F_ = h.shape[1] // 2
    a, g, d = h[:, :F_].to(dt), h[:, F_:].to(dt), dout.to(dt)
    cdf, pdf = _phi(g)
    ad, gd, dd = h[:, :F_].double(), h[:, F_:].double(), dout.double()
    c64, p64 = _phi(gd)
    out, da, dg = a * g * cdf, d * g * cdf, d * a * (cdf + g * pdf)
    r_out, r_da, r_dg = ad * gd * c64, dd * gd * c64, dd * ad * (c64 + gd * p64)
    return {"out": out, "da": da, "dg": dg,
            "T_out": (U8 + U17) * r_out.abs() + (ad * gd).abs() * E_CDF + TINY,
            "T_da": (U8 + U17) * r_da.abs() + (dd * gd).abs() * E_CDF + TINY,
            "T_dg": U8 * r_dg.abs() + (dd * ad).abs() * (U17 * (c64 + gd.abs() * p64) + E_CDF + 0.6 * U24) + TINY}


# ------------------------------------------------------------------------------------------
# rmsnorm
RMS_CS, RMS_ROWS = (8, 504, 512, 520, 768, 4096), (1, 3, 4, 5, 77)
RMS_INPUTS = ("plain", "row_scales", "tiny", "constant", "outlier")
RMS_STRIDE_CASE = (65541, 8)   # rows past 4 x GRID_CAP


def rms_cases():
    return [(r, C) for C in RMS_CS for r in RMS_ROWS] + [RMS_STRIDE_CASE]


def rms_math(x, w, eps, dt, plant=None):
    """y before the final rounding, in dt: bf16(x rs) w"""
    v = x.to(dt)
    src = v[:, :512] if plant == "mean_512" else v
    rs = torch.rsqrt((src * src).mean(-1, keepdim=True) + eps)
    return (v * rs).to(BF).to(dt) * w.to(dt)


def check_rms(kernel, got, x, w, eps, what):
    xd, wd = x.double(), w.double()
    n = xd * torch.rsqrt((xd * xd).mean(-1, keepdim=True) + eps)
    g = got.detach().double().cpu()
    best = None
    for sgn in (-1.0, 1.0):
        cand = wd * (n * (1 + sgn * U17)).to(BF).double()
        ratio = (g - cand).abs() / (U8 * cand.abs() + TINY)
        best = ratio if best is None else torch.minimum(best, ratio)
    best = torch.where(torch.isnan(best), torch.full_like(best, math.inf), best)
    note(kernel, float(best.max()), what)
    if not bool((best <= 1).all()):
        i = int(best.argmax())
        raise AssertionError(f"{what}: {int((best > 1).sum())} of {best.numel()} elements out of bound; worst at flat "
                             f"index {i}: got {float(g.flatten()[i])!r}, w bf16(n) = "
                             f"{float((wd * n.to(BF).double()).flatten()[i])!r}, ratio {float(best.flatten()[i]):.3f}")


@functools.lru_cache(maxsize=4)
def rms_case(rows, C, inp):
    c = Case()
    s = _seed(rows, C, RMS_INPUTS.index(inp), 17)
    c.rows, c.C, c.eps, c.name = rows, C, f32(1e-6), f"rmsnorm rows={rows} C={C} {inp}"
    c.x = N.GENERATORS[inp]((rows, C), s)
    c.w = N.params(C, s + 7, inp != "plain")[0]
    return c


# ------------------------------------------------------------------------------------------
# embed_tokens
EMBED_CASES = [(2, 77, 768, 1000), (3, 5, 8, 7)]


@functools.lru_cache(maxsize=4)
def embed_case(B, T, D, vocab):
    c = Case()
    g = _gen(_seed(B, T, D, vocab))
    c.ids = torch.randint(0, vocab, (B, T), generator=g, dtype=torch.int64)
    c.ids.view(-1)[:5] = torch.tensor([-1, 0, vocab - 1, vocab, 2 ** 40])
    c.tok, c.pos = _randn((vocab, D), g).to(BF), _randn((T, D), g).to(BF)
    c.name = f"embed_tokens B={B} T={T} D={D} vocab={vocab}"
    return c


def embed_math(c, with_pos, plant=None):
    ids = c.ids.view(-1)
    ids = ids % c.tok.shape[0] if plant == "no_clamp" else ids.clamp(0, c.tok.shape[0] - 1)
    v = c.tok[ids].float()
    if with_pos:
        v = v + c.pos[torch.arange(ids.numel()) % c.ids.shape[1]].float()
    return v.to(BF)


# ------------------------------------------------------------------------------------------
# elementwise.hip
UPS_CASES = [(1, 1, 1, 8), (2, 3, 5, 24)]
COLSUM_CASES = [(1, 8, 1), (9, 24, 4), (1000, 264, 1000), (4096 * 3 + 7, 72, None)]
COLSUM_SLICE = (77, 40, 16, 11)   # rows, width of the buffer, column offset of the slice, rows per group; N = 16
CAST_NS = (1, 1000)
TS_T, TS_DIMS = (0.0, 0.5, 1.0, 250.25, 999.0, 1000.0), (2, 256, 320)
IMG_CASES = [(2, 3, 3, 5, 8), (1, 4, 2, 2, 8), (1, 9, 1, 7, 16)]
IMG_MULADD = [(2.0, -1.0), (0.7, 0.1)]
PACK_CASES = [(1, 2, 2, 1), (2, 8, 12, 16)]


def ups_math(dup, prev, dt, plant=None):
    """dup [N, 2H, 2W, C] -> sum of each 2x2 block (+ prev) and the bound of the sum"""
    Nn, H2, W2, C = dup.shape
    v = dup.to(dt).view(Nn, H2 // 2, 2, W2 // 2, 2, C)
    s = v[:, :, 0, :, 0] + v[:, :, 0, :, 1] + v[:, :, 1, :, 0] + v[:, :, 1, :, 1]
    ab = v.double().abs().sum((2, 4))
    R = 4
    if prev is not None:
        ab, R = ab + prev.double().abs(), 5
        if plant != "ups_no_acc":
            s = s + prev.to(dt)
    return s, R * U24 * ab


def colsum_math(x, rpg, dt, plant=None):
    """x [M, N] -> [groups, N] sums and the bound R 2^-24 sum|x|"""
    M, Ncol = x.shape
    rpg = M if rpg is None else rpg
    G = (M + rpg - 1) // rpg
    pad = torch.zeros(G * rpg - M, Ncol, dtype=dt)
    v = torch.cat([x.to(dt), pad]).view(G, rpg, Ncol)
    s = v.sum(1)
    if plant == "colsum_ragged" and M % rpg:
        s[-1] = 0
    return s, rpg * U24 * v.double().abs().sum(1)


def ts_math(t, dim, dt):
    """[cos a | sin a], a = t exp(-ln(10000) k / half); dt float32: the kernel's chain"""
    half = dim // 2
    k = torch.arange(half, dtype=dt)
    if dt == F32:
        a = t.float()[:, None] * torch.exp((torch.tensor(-9.210340371976184, dtype=F32) * k) / half)
    else:
        a = t.double()[:, None] * torch.exp(-math.log(10000.0) * k / half)
    return torch.cat([torch.cos(a), torch.sin(a)], 1), torch.cat([a, a], 1).double().abs()


def img_math(img, mul, add, cpad, dt):
    """[B, C, H, W] fp32 -> NHWC [B, H, W, cpad], x mul + add, zero padded; dt float32: x * mul + add as one fma is
    what the kernel does, which for mul = 2 equals the two-operation form"""
    B, C, H, W = img.shape
    out = torch.zeros(B, H, W, cpad, dtype=dt)
    v = img.to(dt).permute(0, 2, 3, 1)
    out[..., :C] = v * torch.tensor(mul, dtype=F32).to(dt) + torch.tensor(add, dtype=F32).to(dt)
    M = torch.zeros(B, H, W, cpad, dtype=F64)
    M[..., :C] = (img.double().permute(0, 2, 3, 1) * f32(mul)).abs() + abs(f32(add))
    return out, M


def pack_math(lat):
    """NHWC [B, h, w, C] -> packed [(h/2)(w/2) B, 4 C], rows t B + b, channel c 4 + dy 2 + dx"""
    B, h, w, C = lat.shape
    v = lat.view(B, h // 2, 2, w // 2, 2, C).permute(1, 3, 0, 5, 2, 4)
    return v.reshape((h // 2) * (w // 2) * B, 4 * C)


def unpack_math(tok, B, h, w, C):
    v = tok.view(h // 2, w // 2, B, C, 2, 2).permute(2, 0, 4, 1, 5, 3)
    return v.reshape(B, h, w, C)


def bf_randn(shape, seed, scale=1.0):
    return (_randn(shape, _gen(seed)) * scale).to(BF)


# ------------------------------------------------------------------------------------------
# guarded destinations: every element of a NaN-filled bf16 buffer outside the destination keeps the fill's bits
def outside_intact(buf, view_fn) -> bool:
    """view_fn(t) returns the destination's view of a tensor shaped like buf"""
    b = buf.detach().cpu().view(torch.int16).clone()
    view_fn(b).fill_(NANBITS)
    return bool((b == NANBITS).all())

# ------------------------------------------------------------------------------------------
# checks shared by the CPU and the GPU file
def r16(t):
    return t.to(BF)


def ga_check(key, c, h):
    r = c.ref
    check_elem(key + "gated_add_fwd", r16(h["out"]), r["out"], r["M_out"], c.name + " out")
    check(key + "gated_add_bwd dy", r16(h["dy"]), r["dy"], (U8 + U24) * r["dy"].abs(), c.name + " dy")
    check_col(key + "gated_add_bwd dgate", r16(h["dgate"]), r["dgate"], r["B_dgate"], c.name + " dgate")


def act_check(key, kind, x, y, what, g=None):
    """y = act(x) (* g)"""
    r, _, Ey, _ = act_math(kind, x, F64)
    if g is not None:
        r, Ey = r * g.double(), Ey * g.double().abs()
    check(key, y, r, U8 * r.abs() + Ey + TINY, what)


def dact_check(key, kind, x, dy, dx, what):
    _, d, _, Ed = act_math(kind, x, F64)
    r = d * dy.double()
    check(key, dx, r, U8 * r.abs() + Ed * dy.double().abs() + TINY, what)
