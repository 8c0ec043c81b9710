"""Attention kernels against a float64 reference, row by row, at the tile edges, on inputs where the softmax
matters, inside guarded buffers; the row-softmax kernels and the materialized path directly (GPU).

Tolerances are derived, not chosen (tests/_attn_edges.py): per (b, h, token) row the kernel must stay within
4 x the error of the float64 reference carrying only the roundings the algorithm is entitled to, and the
whole-tensor bounds of test_kernels_gpu.py (2e-2 forward, 3e-2 backward) stay in force beside it.
tests/test_attention_edges_ref.py shows on the CPU that each detector has teeth."""
import ctypes as C
import math

import pytest
import torch

import _attn_edges as E
from onetrainer_amd import kernels as K

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float("nan")
B_, H_ = 2, 3   # every geometry case: batch and head strides cannot be swapped unnoticed

WORST: dict = {}   # route -> (kernel / floor ratio, case) of the worst row seen


def fwd_route(Dv):
    return "fwd64" if Dv <= 64 else "fwd128"


def bwd_routes(Nk, Dv):
    """kernel that writes (dq, dk / dv)"""
    if Nk <= 128 and Dv <= 64:
        return "cross", "cross"
    return ("dq64", "dkv64") if Dv <= 64 else ("dq128", "dkv128")


def note(route, ratio, what):
    if ratio > WORST.get(route, (-1.0, ""))[0]:
        WORST[route] = (ratio, what)


def nan_like(t):
    return torch.full_like(t, NAN)


def operands(c, layout, dev):
    """(q, k, v, do) on the device and NaN-filled (o, dq, dk, dv) in the layout's buffers"""
    q, k, v, do = (t.to(dev) for t in (c.q, c.k, c.v, c.do))
    Cc = q.shape[2]
    if layout == "fused":    # q, k, v: column slices of one [B, N, 3 H Dv] projection output; gradients likewise
        qkv = torch.cat([q, k, v], dim=-1)
        g = nan_like(qkv)
        q, k, v = qkv[..., :Cc], qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:]
        dq, dk, dv = g[..., :Cc], g[..., Cc:2 * Cc], g[..., 2 * Cc:]
    elif layout == "kv":     # k, v: halves of a [B, Nk, 2 H Dv] buffer
        kv = torch.cat([k, v], dim=-1)
        g = nan_like(kv)
        k, v = kv[..., :Cc], kv[..., Cc:]
        dq, dk, dv = nan_like(q), g[..., :Cc], g[..., Cc:]
    else:
        dq, dk, dv = nan_like(q), nan_like(k), nan_like(v)
    return (q, k, v, do), (nan_like(q).contiguous(), dq, dk, dv)


def run(c, layout, dev, cast_stream=None, explicit_scale=False):
    (q, k, v, do), (o, dq, dk, dv) = operands(c, layout, dev)
    sc = c.scale if explicit_scale else None
    o, lse = K.attn_fwd(q, k, v, c.H, scale=sc, out=o)
    K.attn_bwd(q, k, v, o, lse, do, c.H, scale=sc, dq=dq, dk=dk, dv=dv, cast_stream=cast_stream)
    if cast_stream is not None:
        torch.cuda.current_stream().wait_stream(cast_stream)
    return {"o": o, "lse2": lse, "dq": dq, "dk": dk, "dv": dv}


def check(c, got, what, names=("o", "lse2", "dq", "dk", "dv")):
    """every row of every tensor within the case's derived tolerance; lse absolutely"""
    Nk, Dv = c.k.shape[1], c.k.shape[2] // c.H
    route = dict(zip(("dq", "dk", "dv"), (bwd_routes(Nk, Dv)[0],) + (bwd_routes(Nk, Dv)[1],) * 2), o=fwd_route(Dv))
    fails = []
    for n in names:
        g = got[n].float().cpu()
        if n == "lse2":
            err, bound = float((g.double() - c.ref[n]).abs().max()), E.lse_bound(c.ref)
            print(f"EDGE {what} lse err {err:.3e} bound {bound:.3e}")
            if not err <= bound:
                fails.append(f"lse: {err:.3e} > {bound:.3e}")
            continue
        if float(c.ref[n].abs().max()) == 0.0:   # one key: the softmax is constant, dq = dk = 0 (Case.zero_bound)
            err, bound = float(g.double().abs().max()), c.zero_bound(n)
            print(f"EDGE {what} {n} reference 0, |got| {err:.3e} bound {bound:.3e}")
            if not err <= bound:
                fails.append(f"{n}: |got| {err:.3e} > {bound:.3e} where the reference is 0")
            continue
        m, where = E.row_metric(g, c.ref[n], c.H)
        floor, tol = c.floor[n], c.tol(n)
        ratio = m / floor if floor > 0 else (0.0 if m == 0 else math.inf)
        print(f"EDGE {what} {route[n]} {n} row err {m:.3e} floor {floor:.3e} ratio {ratio:.2f} tol {tol:.3e}")
        note(route[n], ratio, what)
        if not m <= tol:
            fails.append(f"{n} ({route[n]}): row (b, h, token) = {where} off by {m:.3e} > {tol:.3e} "
                         f"(floor {floor:.3e})")
        w, cap = c.whole(g, n)
        if not w <= cap:
            fails.append(f"{n} ({route[n]}): max|d| / max|ref| = {w:.3e} > {cap:.0e}")
    assert not fails, f"{what}: " + "; ".join(fails)


def layouts_for(Nq, Nk):
    return ("dense", "kv", "fused") if Nq == Nk else ("dense", "kv")


# ------------------------------------------------------------------------------------------
# 2. edge geometry: every route at its tile edges, three operand layouts
CROSS_NK, CROSS_NQ = (1, 31, 32, 33, 64, 65, 96, 97, 128), (1, 63, 64, 65, 129)
PAIR64_NK, PAIR128_NK, PAIR_NQ = (129, 191, 193, 257), (1, 33, 64, 65, 127, 129), (1, 31, 33, 127, 129, 257)


def geometry(c, dev, what, **kw):
    Nq, Nk = c.q.shape[1], c.k.shape[1]
    for layout in layouts_for(Nq, Nk):
        check(c, run(c, layout, dev, **kw), f"{what} {layout}")


@pytest.mark.parametrize("Nk", CROSS_NK)
@pytest.mark.parametrize("Nq", CROSS_NQ)
@pytest.mark.parametrize("Dv", [8, 40, 64])
def test_geometry_cross(dev, Dv, Nq, Nk):
    """forward D = 64 + the one-pass cross backward (Nk <= 128, Dv <= 64)"""
    geometry(E.geometry_case(B_, H_, Nq, Nk, Dv), dev, f"geom Dv={Dv} Nq={Nq} Nk={Nk}")


@pytest.mark.parametrize("Nk", PAIR64_NK)
@pytest.mark.parametrize("Nq", PAIR_NQ)
@pytest.mark.parametrize("Dv", [8, 40, 64])
def test_geometry_pair_d64(dev, Dv, Nq, Nk):
    """forward D = 64 + the dQ and dK/dV kernels at D = 64"""
    geometry(E.geometry_case(B_, H_, Nq, Nk, Dv), dev, f"geom Dv={Dv} Nq={Nq} Nk={Nk}")


@pytest.mark.parametrize("Nk", PAIR128_NK)
@pytest.mark.parametrize("Nq", PAIR_NQ)
@pytest.mark.parametrize("Dv", [72, 128])
def test_geometry_pair_d128(dev, Dv, Nq, Nk):
    """the D = 128 kernels; at Dv = 72 they run mostly on padding"""
    geometry(E.geometry_case(B_, H_, Nq, Nk, Dv), dev, f"geom Dv={Dv} Nq={Nq} Nk={Nk}")


@pytest.mark.parametrize("Dv,Nq,Nk,scale", [(64, 65, 77, 1.0), (40, 129, 97, 0.05), (64, 129, 193, 0.05),
                                            (64, 127, 191, 1.0), (128, 127, 129, 1.0), (72, 129, 65, 0.05)])
def test_explicit_scale(dev, Dv, Nq, Nk, scale):
    geometry(E.geometry_case(B_, H_, Nq, Nk, Dv, scale), dev, f"scale={scale} Dv={Dv} Nq={Nq} Nk={Nk}",
             explicit_scale=True)


def split_count(c, dev):
    """the dK / dV partial-slab count the library plans: slab bytes / (2 slabs x 4 bytes x B Nk H Dv); 0 = no slabs"""
    q, k, v = (t.to(dev) for t in (c.q, c.k, c.v))
    a = K._attn_args(q, k, v, c.H, None)
    nbytes = K.lib().otamd_attn_bwd_slab_bytes(C.byref(a))
    assert nbytes >= 0 and nbytes % (2 * 4 * k.numel()) == 0
    return nbytes // (2 * 4 * k.numel())


# (B, H, Nq, Nk, Dv) -> split / chunk count.  The first two leave trailing splits empty (the kernel's per-split
# length is 192 queries: splits 11..15 get none and must still write zeros, there is no memset); chunk counts
# 2, 4, 5, 6, 7 walk the cast kernel's unroll-by-4 and its remainder loop; B H = 512 at Nq = 1025 is two chunks of
# 9 and 8 rounds (the kernel re-derives 576 queries per chunk from the count), Nq = 2048 two chunks of the full 16.
SPLITS = [((1, 2, 2049, 256, 64), 16), ((1, 1, 2049, 129, 128), 16), ((1, 1, 65, 77, 64), 2), ((1, 1, 193, 77, 64), 4),
          ((1, 1, 289, 77, 64), 5), ((1, 1, 321, 77, 64), 6), ((1, 1, 400, 77, 64), 7), ((4, 128, 1025, 8, 8), 2),
          ((4, 128, 2048, 8, 8), 2)]


@pytest.mark.parametrize("shape,count", SPLITS, ids=lambda x: "x".join(map(str, x)) if isinstance(x, tuple) else str(x))
def test_split_bookkeeping(dev, shape, count):
    """the planned count is the one this case is about; both host routes (otamd_attn_bwd and, with cast_stream,
    otamd_attn_bwd_ex) are right row by row and bit-identical run to run, into fresh NaN-filled outputs"""
    c = E.geometry_case(*shape)
    assert split_count(c, dev) == count
    what = "split " + "x".join(map(str, shape))
    first = run(c, "dense", dev)
    check(c, first, what)
    side = torch.cuda.Stream(device=dev)
    for stream in (None, side, side):
        again = run(c, "kv", dev, cast_stream=stream)
        for n in ("o", "lse2", "dq", "dk", "dv"):
            assert torch.equal(again[n], first[n]), f"{what}: {n} differs between runs (cast_stream={stream})"


# ------------------------------------------------------------------------------------------
# 3. inputs that make the softmax matter
ROUTE_SHAPES = [(70, 77, 64), (70, 190, 64), (70, 190, 128)]   # cross + fwd64, dq64 / dkv64, fwd128 + dq128 / dkv128


@pytest.mark.parametrize("order", ["first", "last", "grow"])
@pytest.mark.parametrize("Nq,Nk,Dv", ROUTE_SHAPES)
def test_peaked_rows(dev, Nq, Nk, Dv, order):
    """one-hot softmax (margin >= 26 nats, matching scores up to 185 / 261 log2 units): o is v[pi] to the bit (the
    winning probability is 1 to fp32 rounding, the rest < 1e-11: nothing near the 2^-9 it takes to move a bf16
    value), lse is the matching score, dv[j] the sum of do_i over pi(i) = j within one bf16 rounding per element
    (plus the fp32 sum's 2^-18), dq and dk ~0 within one bf16 rounding of dP."""
    c, pi = E.peaked_case(B_, H_, Nq, Nk, Dv, order)
    o_want, lse_want, dv_want = E.peaked_expect(c, pi)
    what = f"peaked {order} Nq={Nq} Nk={Nk} Dv={Dv}"
    for layout in ("dense", "kv"):
        got = {n: t.float().cpu().double() for n, t in run(c, layout, dev).items()}
        bad = (got["o"] != o_want).nonzero()
        assert bad.numel() == 0, f"{what} {layout}: o != v[pi] at {bad[0].tolist()} ({bad.shape[0]} elements)"
        lerr = float((got["lse2"] - lse_want).abs().max())
        print(f"EDGE {what} {layout} lse err {lerr:.3e} bound {E.lse_bound(c.ref):.3e}")
        assert lerr <= E.lse_bound(c.ref), f"{what} {layout}: lse off by {lerr:.3e}"
        over = ((got["dv"] - dv_want).abs() - (2.0 ** -8 * dv_want.abs() + 2.0 ** -18)).max()
        assert over <= 0, f"{what} {layout}: dv off by {float(over):.3e} beyond one bf16 rounding"
        for n in ("dq", "dk"):
            err = float((got[n] - c.ref[n]).abs().max())
            print(f"EDGE {what} {layout} {n} |err| {err:.3e} bound {c.zero_bound(n):.3e}")
            assert err <= c.zero_bound(n), f"{what} {layout}: {n} off by {err:.3e} > {c.zero_bound(n):.3e}"


@pytest.mark.parametrize("Nk,Dv", [(1, 64), (33, 64), (77, 64), (129, 64), (190, 64), (129, 128), (190, 128)])
def test_negative_rows(dev, Nk, Dv):
    """every true score <= -20 nats: a zero-filled key past Nk that slipped through a mask would take all the
    weight (tests/test_attention_edges_ref.py::test_negative_rows_expose_a_zero_key)"""
    c = E.negative_case(B_, H_, 70, Nk, Dv)
    for layout in ("dense", "kv"):
        check(c, run(c, layout, dev), f"negative Nk={Nk} Dv={Dv} {layout}")


# ------------------------------------------------------------------------------------------
# 4. nothing read or written outside the operands
def guarded(t, dev, extra_rows, extra_cols, guard):
    """t [B, N, C] as a view into a NaN-filled flat buffer: `guard` elements before and after, extra rows after N
    inside each batch stride, extra columns after C in each row.  Returns (view, flat)."""
    B, N, Cc = t.shape
    R, W = N + extra_rows, Cc + extra_cols
    flat = torch.full((2 * guard + B * R * W,), NAN, dtype=BF, device=dev)
    view = flat[guard:guard + B * R * W].view(B, R, W)[:, :N, :Cc]
    if t is not None:
        view.copy_(t.to(dev))
    return view, flat


def outside_unchanged(view, flat, before):
    """every byte outside `view` is as before (raw int16), and no NaN is left inside"""
    assert not torch.isnan(view.float()).any(), "NaN left inside the output view"
    now, was = flat.view(torch.int16).clone(), before.view(torch.int16).clone()
    for raw in (now, was):
        raw.view(BF)[view.storage_offset() - flat.storage_offset():].as_strided(view.shape, view.stride()).zero_()
    return torch.equal(now, was)


@pytest.mark.parametrize("Dv", [40, 72])
@pytest.mark.parametrize("Nk", [77, 129])
@pytest.mark.parametrize("Nq", [45, 100])
def test_guarded_buffers(dev, Dv, Nk, Nq):
    """operands and outputs inside larger NaN buffers (guards of 24 and 40 elements, 3 extra rows per batch, 8 or
    16 extra columns: bases stay 16-byte aligned, strides multiples of 8): a read outside an operand poisons the
    result, a write outside an output changes a byte"""
    c = E.geometry_case(B_, H_, Nq, Nk, Dv)
    what = f"guarded Dv={Dv} Nq={Nq} Nk={Nk}"
    (q, _), (k, _), (v, _), (do, _) = (guarded(t, dev, 3, ec, g) for t, ec, g in
                                       ((c.q, 8, 24), (c.k, 16, 40), (c.v, 8, 40), (c.do, 16, 24)))
    outs = {n: guarded(torch.full_like(t, NAN), dev, 3, ec, g) for n, t, ec, g in
            (("o", c.q, 16, 40), ("dq", c.q, 8, 24), ("dk", c.k, 8, 24), ("dv", c.k, 16, 40))}
    before = {n: f.clone() for n, (_, f) in outs.items()}
    ins_before = [t.clone() for t in (q, k, v, do)]
    o, lse = K.attn_fwd(q, k, v, c.H, out=outs["o"][0])
    assert o.data_ptr() == outs["o"][0].data_ptr()
    K.attn_bwd(q, k, v, o, lse, do, c.H, dq=outs["dq"][0], dk=outs["dk"][0], dv=outs["dv"][0])
    got = {n: vw for n, (vw, _) in outs.items()}
    got["lse2"] = lse
    assert all(torch.isfinite(t.float()).all() for t in got.values()), f"{what}: non-finite output"
    check(c, got, what)
    for n, (vw, flat) in outs.items():
        assert outside_unchanged(vw, flat, before[n]), f"{what}: bytes outside {n} changed"
    for t, was in zip((q, k, v, do), ins_before):
        assert torch.equal(t, was)


@pytest.mark.parametrize("python_host", [False, True])
def test_einval_surfaces(dev, python_host):
    """a token stride that is no multiple of 8 and a base that is not 16-byte aligned are refused on the host
    (OTAMD_EINVAL) by both host layers, before anything is launched"""
    c = E.geometry_case(B_, H_, 33, 33, 64)
    q, k, v, do = (t.to(dev) for t in (c.q, c.k, c.v, c.do))
    Bq, N, Cc = q.shape
    odd = torch.zeros(Bq, N, Cc + 4, dtype=BF, device=dev)[..., :Cc]          # token stride C + 4
    off = torch.zeros(Bq * N * Cc + 8, dtype=BF, device=dev)[4:4 + Bq * N * Cc].view(Bq, N, Cc)   # base + 8 bytes
    assert odd.stride(1) % 8 == 4 and off.data_ptr() % 16 == 8
    ctx = K.python_host() if python_host else torch.no_grad()
    with ctx:
        o, lse = K.attn_fwd(q, k, v, c.H)
        for bad in (odd, off):
            with pytest.raises(RuntimeError, match="otamd_attn_fwd: invalid arguments"):
                K.attn_fwd(bad, k, v, c.H)
            with pytest.raises(RuntimeError, match="otamd_attn_fwd: invalid arguments"):
                K.attn_fwd(q, k, bad, c.H)
            with pytest.raises(RuntimeError, match="otamd_attn_fwd: invalid arguments"):
                K.attn_fwd(q, k, v, c.H, out=bad)
            with pytest.raises(RuntimeError, match="otamd_attn_bwd: invalid arguments"):
                K.attn_bwd(q, k, v, o, lse, do, c.H, dk=bad)
            with pytest.raises(RuntimeError, match="otamd_attn_bwd: invalid arguments"):
                K.attn_bwd(q, k, v, o, lse, bad, c.H)


# ------------------------------------------------------------------------------------------
# 5. the row-softmax kernels and the materialized path, directly
def ulp32_t(x):
    return 2.0 ** (torch.floor(torch.log2(x.abs().clamp_min(1.0))) - 23)


def softmax_rows_input(rows, ncols, width, scale, seed):
    """fp32 S [rows, width] with NaN pad columns: unit-normal rows, constant rows (small and at 1e4), rows around
    offsets up to +-1e4 and one row spanning -1e4 .. 1e4 (all as values of scale * S)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, ncols, generator=g, dtype=torch.float64) * 3
    offs = torch.linspace(-1e4, 1e4, rows, dtype=torch.float64)[torch.randperm(rows, generator=g)]
    x += (offs * (torch.arange(rows) % 2))[:, None]   # every other row sits at a large offset
    x[0] = 0.5
    if rows > 3:
        x[1] = 1e4
        x[2] = torch.linspace(-1e4, 1e4, ncols, dtype=torch.float64) if ncols > 1 else -1e4
    S = torch.full((rows, width), NAN, dtype=torch.float32)
    S[:, :ncols] = (x / scale).float()
    return S


def softmax_rows_check(dev, rows, ncols, npad, scale, what):
    scale = E.f32(scale)
    S = softmax_rows_input(rows, ncols, npad, scale, rows + ncols)
    ref, lse_ref = E.softmax_rows_ref(S, ncols, scale)
    emu, _ = E.softmax_rows_ref(S, ncols, scale, round_scores=True)
    floor = E.rows_metric(E.rb(emu), ref)[0]
    P = torch.full((rows, npad), NAN, dtype=BF, device=dev)
    lse = torch.full((rows,), NAN, dtype=torch.float32, device=dev)
    K.softmax_rows_fwd(S.to(dev), P, lse, ncols, scale)
    Pc = P.float().cpu().double()
    assert (Pc[:, ncols:] == 0).all(), f"{what}: pad columns of P are not exact zeros"
    m, where = E.rows_metric(Pc[:, :ncols], ref)
    print(f"EDGE {what} softmax_fwd row err {m:.3e} floor {floor:.3e}")
    note("softmax_fwd", m / floor if floor > 0 else 0.0 if m == 0 else math.inf, what)
    assert m <= 4 * floor, f"{what}: P row {where[2]} off by {m:.3e} > 4 x {floor:.3e}"
    # lse (natural log): fp32 spacing at the magnitude of the row's largest |scale S| / |lse|, x 4
    mag = torch.maximum(lse_ref.abs(), (S[:, :ncols].double() * scale).abs().amax(-1))
    lerr = (lse.cpu().double() - lse_ref).abs()
    assert (lerr <= 4 * ulp32_t(mag)).all(), f"{what}: lse off by {float((lerr / ulp32_t(mag)).max()):.1f} fp32 spacings"
    # backward from the kernel's own P (bf16) and a fp32 dP with NaN pad columns
    g = torch.Generator().manual_seed(7)
    dP = torch.full((rows, npad), NAN, dtype=torch.float32)
    dP[:, :ncols] = torch.randn(rows, ncols, generator=g)
    Pin = P.clone()
    Pin[:, ncols:] = NAN
    dS = torch.full((rows, npad), NAN, dtype=BF, device=dev)
    K.softmax_rows_bwd(Pin, dP.to(dev), dS, ncols, scale)
    p64, d64 = Pc[:, :ncols], dP[:, :ncols].double()
    dref = scale * p64 * (d64 - (p64 * d64).sum(-1, keepdim=True))
    dSc = dS.float().cpu().double()
    assert (dSc[:, ncols:] == 0).all(), f"{what}: pad columns of dS are not exact zeros"
    if float(dref.abs().max()) == 0.0:   # one column: dS = 0 exactly (P = 1, the row sum is dP itself)
        assert (dSc[:, :ncols] == 0).all()
        return
    dfloor = E.rows_metric(E.rb(dref), dref)[0]
    m, where = E.rows_metric(dSc[:, :ncols], dref)
    print(f"EDGE {what} softmax_bwd row err {m:.3e} floor {dfloor:.3e}")
    note("softmax_bwd", m / dfloor if dfloor > 0 else 0.0 if m == 0 else math.inf, what)
    assert m <= 4 * dfloor, f"{what}: dS row {where[2]} off by {m:.3e} > 4 x {dfloor:.3e}"


@pytest.mark.parametrize("extra", [0, 8])
@pytest.mark.parametrize("ncols", [1, 3, 4, 5, 77, 255, 256, 257, 1023])
def test_softmax_rows(dev, ncols, extra):
    npad = (ncols + 7) // 8 * 8 if extra == 0 else ncols + 8
    npad = (npad + 3) // 4 * 4   # the library wants whole 4-element groups
    softmax_rows_check(dev, 11, ncols, npad, 0.3, f"softmax_rows ncols={ncols} pad={npad}")


def test_softmax_rows_grid_stride(dev):
    """more rows than 65536 blocks x 4: the grid-stride loop, with a row count that is no multiple of 4"""
    softmax_rows_check(dev, 65536 * 4 + 3, 8, 16, 0.3, "softmax_rows grid-stride")


def masked_direct(dev, BH, Nq, H, ncols, npad, scale, causal, bias_qch, order, what, seed=0):
    """otamd_softmax_masked_fwd on a random S; bias_qch: float64 [Nq, ncols, H] (bf16 values) or None, laid out
    in memory in `order` (a permutation of 'qch')"""
    scale = E.f32(scale)
    g = torch.Generator().manual_seed(seed)
    S = torch.full((BH, Nq, npad), NAN, dtype=torch.float32)
    S[..., :ncols] = torch.randn(BH, Nq, ncols, generator=g) * 3
    ref = E.masked_softmax_ref(S, ncols, scale, Nq, H, causal, bias_qch)
    x32 = (S[..., :ncols].double() * scale).float().double()
    if bias_qch is not None:
        x32 = (x32 + bias_qch.permute(2, 0, 1).repeat(BH // H, 1, 1)).float().double()
    emu = E.masked_softmax_ref(x32, ncols, 1.0, Nq, H, causal, None)
    floor = E.rows_metric(E.rb(emu).reshape(BH * Nq, ncols), ref.reshape(BH * Nq, ncols))[0]
    bias, strides = None, (0, 0, 0)
    if bias_qch is not None:
        perm = ["qch".index(ch) for ch in order]
        bias = bias_qch.permute(perm).contiguous().to(BF).to(dev)
        st = dict(zip(order, bias.stride()))
        strides = (st["q"], st["c"], st["h"])
    P = torch.full((BH, Nq, npad), NAN, dtype=BF, device=dev)
    Sd = S.to(dev)
    K.check(K.lib().otamd_softmax_masked_fwd(Sd.data_ptr(), npad, P.data_ptr(), npad, BH * Nq, ncols, npad, scale, Nq,
                                             H, int(causal), None if bias is None else bias.data_ptr(), *strides,
                                             K.stream_handle()), "otamd_softmax_masked_fwd")
    Pc = P.float().cpu().double()
    assert (Pc[..., ncols:] == 0).all(), f"{what}: pad columns are not exact zeros"
    if causal:
        dead = torch.arange(ncols)[None, :] > torch.arange(Nq)[:, None]
        assert (Pc[..., :ncols][:, dead] == 0).all(), f"{what}: masked columns are not exact zeros"
    m, where = E.rows_metric(Pc[..., :ncols].reshape(BH * Nq, ncols), ref.reshape(BH * Nq, ncols))
    print(f"EDGE {what} softmax_masked row err {m:.3e} floor {floor:.3e}")
    note("softmax_masked", m / floor if floor > 0 else 0.0 if m == 0 else math.inf, what)
    assert m <= 4 * floor, f"{what}: P row {where[2]} off by {m:.3e} > 4 x {floor:.3e}"


def t5_bias(Nq, ncols, H, mag, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(Nq, ncols, H, generator=g) * mag).to(BF).double()


@pytest.mark.parametrize("order", ["hqc", "qch", "qhc"])
@pytest.mark.parametrize("causal", [False, True])
def test_softmax_masked_bias(dev, order, causal):
    """T5-style bias with H = 3 in each stride order, alone and under the causal mask; unit and large magnitudes"""
    for mag in (1.0, 300.0):
        masked_direct(dev, 6, 77, 3, 77, 80, 0.125, causal, t5_bias(77, 77, 3, mag), order,
                      f"masked bias {order} causal={causal} mag={mag}")


@pytest.mark.parametrize("Nq,ncols,npad", [(1, 1, 8), (77, 77, 80), (100, 77, 80), (40, 77, 88)])
def test_softmax_masked_causal(dev, Nq, ncols, npad):
    """causal: row 0 has one live column; Nq > Nk rows see every key"""
    masked_direct(dev, 6, Nq, 3, ncols, npad, 1.0, True, None, "qch", f"masked causal Nq={Nq} ncols={ncols}")


def test_softmax_masked_grid_stride(dev):
    """more rows than 16384 blocks x 4 (65537 = one batch-head of 65537 queries, 8 columns, causal)"""
    masked_direct(dev, 1, 16384 * 4 + 1, 1, 8, 8, 1.0, True, None, "qch", "masked grid-stride")


@pytest.mark.parametrize("Nq,Nk,causal,with_bias", [(1, 1, True, False), (77, 77, True, False), (100, 77, True, False),
                                                    (77, 77, False, True), (77, 77, True, True)])
def test_attn_masked_fwd(dev, Nq, Nk, causal, with_bias):
    """the whole masked forward (CLIP causal, T5 bias) per row against float64; floor: P and o rounded to bf16"""
    D = 64
    c = E.geometry_case(B_, H_, Nq, Nk, D)
    scale = c.scale
    bias_qch = t5_bias(Nq, Nk, H_, 2.0) if with_bias else None
    s = E.heads(c.q, H_) @ E.heads(c.k, H_).transpose(-1, -2)
    p = E.masked_softmax_ref(s.reshape(B_ * H_, Nq, Nk), Nk, scale, Nq, H_, causal, bias_qch).reshape(B_, H_, Nq, Nk)
    ref = E.unheads(p @ E.heads(c.v, H_))
    floor = E.row_metric(E.rb(E.unheads(E.rb(p) @ E.heads(c.v, H_))), ref, H_)[0]
    bias, strides = None, (0, 0, 0)
    if with_bias:
        bias = bias_qch.permute(2, 0, 1).contiguous().to(BF).to(dev)   # [H, Nq, Nk]
        strides = (Nk, 1, Nq * Nk)
    q, k, v = (t.to(dev) for t in (c.q, c.k, c.v))
    o = K.attn_masked_fwd(q, k, v, H_, scale=scale, causal=causal, bias=bias, bias_strides=strides)
    m, where = E.row_metric(o.float(), ref, H_)
    what = f"attn_masked Nq={Nq} Nk={Nk} causal={causal} bias={with_bias}"
    print(f"EDGE {what} row err {m:.3e} floor {floor:.3e}")
    note("attn_masked", m / floor if floor > 0 else 0.0 if m == 0 else math.inf, what)
    assert m <= 4 * floor, f"{what}: row {where} off by {m:.3e} > 4 x {floor:.3e}"
    assert float((o.float().cpu().double() - ref).abs().max() / ref.abs().max()) <= E.FWD_CAP


@pytest.mark.parametrize("Nk", [1, 7, 9, 77])
def test_attn_mat_wide_heads(dev, Nk):
    """the materialized path at D = 160 (batched GEMMs + softmax_rows_fwd / _bwd), dense and fused, per row"""
    D = 160
    for layout, Nq in (("dense", 70), ("kv", 70), ("fused", Nk)):
        c = E.geometry_case(B_, H_, Nq, Nk, D)
        (q, k, v, do), (o, dq, dk, dv) = operands(c, layout, dev)
        o, P = K.attn_mat_fwd(q, k, v, c.H, out=o)
        assert (P[..., Nk:] == 0).all()
        K.attn_mat_bwd(q, k, v, P, do, c.H, dq=dq, dk=dk, dv=dv)
        what = f"mat D=160 Nq={Nq} Nk={Nk} {layout}"
        got = {"o": o, "dq": dq, "dk": dk, "dv": dv}
        for n in ("o", "dq", "dk", "dv"):
            g = got[n].float().cpu()
            if float(c.ref[n].abs().max()) == 0.0:
                assert float(g.abs().max()) <= c.zero_bound(n), f"{what}: {n} where the reference is 0"
                continue
            m, where = E.row_metric(g, c.ref[n], c.H)
            print(f"EDGE {what} mat {n} row err {m:.3e} floor {c.floor[n]:.3e}")
            note("mat", m / c.floor[n] if c.floor[n] > 0 else 0.0 if m == 0 else math.inf, what)
            assert m <= c.tol(n), f"{what}: {n} row {where} off by {m:.3e} > {c.tol(n):.3e} (floor {c.floor[n]:.3e})"
            w, cap = c.whole(g, n)
            assert w <= cap, f"{what}: {n} max|d| / max|ref| = {w:.3e} > {cap:.0e}"


def test_worst_ratios_report():
    """the worst kernel / floor ratio per kernel route over this module's cases (all asserted <= 4 above)"""
    for route in sorted(WORST):
        print(f"EDGE worst {route}: {WORST[route][0]:.2f} x floor at {WORST[route][1]}")
    assert all(r <= E.FLOOR_FACTOR for r, _ in WORST.values())
