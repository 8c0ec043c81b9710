"""The kernels of csrc/flux.hip (without adaLN), csrc/text.hip (without the masked softmax) and csrc/elementwise.hip
against float64 references, element by element, on the shapes that reach every path, on hard inputs, with strided
operands and inside guarded buffers (GPU).  Bounds are derived (tests/_pointwise_edges.py);
tests/test_pointwise_edges_ref.py shows on the CPU that an honest fp32 evaluation meets them and planted errors do
not.  The last test prints the worst |err| / bound per kernel."""
import ctypes
import math

import pytest
import torch

import _pointwise_edges as E
from _pointwise_edges import U8, U24
from onetrainer_amd import kernels as K

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64


def both(fn):
    """fn() through the native host layer, then through the ctypes path"""
    assert K.host_layer() == "native"
    a = fn()
    with K.python_host():
        b = fn()
    return a, b


def same(a, b, what=""):
    if isinstance(a, (tuple, list)):
        for x, y in zip(a, b):
            same(x, y, what)
        return
    assert a.shape == b.shape and a.dtype == b.dtype, what
    bits = {2: torch.int16, 4: torch.int32}[a.element_size()]
    assert torch.equal(a.contiguous().view(bits), b.contiguous().view(bits)), what   # bit-equal, NaN included


def nans(shape, dtype, dev):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), math.nan, dtype=dtype, device=dev)


def flat(n, dtype, dev, init=None):
    """(NaN-filled buffer of n + 16, its [8, 8 + n) destination), the destination optionally preset"""
    buf = nans(n + 16, dtype, dev)
    if init is not None:
        buf[8:8 + n].copy_(init.reshape(-1))
    return buf, buf[8:8 + n]


def flat_ok(buf) -> bool:
    """the 8 elements either side of the destination keep the fill's bits"""
    fill = E.bits(nans(8, buf.dtype, "cpu"))
    return torch.equal(E.bits(buf[:8]), fill) and torch.equal(E.bits(buf[-8:]), fill)


def raw(name, *args):
    K.check(getattr(K.lib(), name)(*[K._p(a) if isinstance(a, torch.Tensor) else a for a in args], K.stream_handle()), name)


def status(name, *args):
    return getattr(K.lib(), name)(*[K._p(a) if isinstance(a, torch.Tensor) else a for a in args], K.stream_handle())


# ------------------------------------------------------------------------------------------
# qknorm_rope
def qk_run(c, dev, dw, dw_acc=False):
    """forward into a guarded buffer, backward into a NaN-filled wider dx; returns (dx buffer view, dw list)"""
    H, rows, HD = c.H, c.rows, c.H * 128
    G = E.qk_geom(H)
    x, cs, sn = c.x.to(dev), c.cs.to(dev), c.sn.to(dev)
    w = [c.w[i].to(dev).clone() if (c.ctx or i < 2) else None for i in range(4)]
    dy = E.wide(c.dy.to(dev), G["lddy"])
    dxbuf = nans((rows + 2, G["lddx"]), BF, dev)
    dx = dxbuf[1:rows + 1]
    K.qknorm_rope_bwd(x, G["qoff"], G["koff"], dy, H, c.B, c.L, w, cs, sn, dx, G["dxqoff"], G["dxkoff"], dw=dw,
                      dw_acc=dw_acc, eps=c.eps)
    r = c.ref
    got = torch.stack([dx[:, G["dxqoff"]:G["dxqoff"] + HD], dx[:, G["dxkoff"]:G["dxkoff"] + HD]], 1)
    E.check_elem("qknorm_rope_bwd dx", got, r["dx"].reshape(rows, 2, HD), r["M_dx"].reshape(rows, 2, HD), c.name + " dx")

    b = dxbuf.cpu().view(torch.int16).clone()
    b[1:rows + 1, G["dxqoff"]:G["dxqoff"] + HD] = E.NANBITS
    b[1:rows + 1, G["dxkoff"]:G["dxkoff"] + HD] = E.NANBITS
    assert bool((b == E.NANBITS).all()), c.name + " dx guards"
    return x, w, cs, sn, G


@pytest.mark.parametrize("inp", E.QK_INPUTS)
@pytest.mark.parametrize("ctx", [True, False])
@pytest.mark.parametrize("T,B,H,L", E.QK_SHAPES)
def test_qknorm_rope(dev, T, B, H, L, ctx, inp):
    c = E.qk_case(T, B, H, L, ctx, inp)
    r, rows, HD = c.ref, c.rows, H * 128
    bufs, dws = zip(*[flat(128, F32, dev) for _ in range(4)])
    x, w, cs, sn, G = qk_run(c, dev, list(dws))
    assert all(flat_ok(b) for b in bufs), c.name + " dw guards"
    for i in range(4):
        E.check_col("qknorm_rope_bwd dw", dws[i], r["dw"][i], r["B_dw"][i], f"{c.name} dw[{i}] f32")
    obuf, o = E.guarded((), rows, 2 * HD, device=dev)
    K.qknorm_rope_fwd(x, G["qoff"], G["koff"], H, B, L, w, cs, sn, eps=c.eps, out=o)
    E.check_elem("qknorm_rope_fwd", o, r["out"].reshape(rows, 2 * HD), r["M_out"].reshape(rows, 2 * HD), c.name + " out")
    assert E.guards_intact(obuf, rows, 2 * HD), c.name + " fwd guards"


@pytest.mark.parametrize("mode", E.QK_DW_MODES)
@pytest.mark.parametrize("T,B,H,L", E.QK_DW_SHAPES)
def test_qknorm_rope_dw_modes(dev, T, B, H, L, mode):
    c = E.qk_case(T, B, H, L, True, "head_scales")
    r = c.ref
    dt = BF if mode.startswith("bf16") else F32
    acc = mode.endswith("_acc")
    prev = c.pdw.to(dev).to(dt)
    bufs, views = zip(*[flat(128, dt, dev, prev[i] if acc else None) for i in range(4)])
    dws = [None] * 4 if mode == "none" else [None, views[1], None, None] if mode == "only_dwk" else list(views)
    qk_run(c, dev, dws, dw_acc=acc)
    assert all(flat_ok(b) for b in bufs), f"{c.name} dw guards {mode}"
    for b, v, d in zip(bufs, views, dws):
        if d is None:   # a destination that was not given is not written
            assert torch.equal(E.bits(v), E.bits(nans(128, dt, "cpu"))), f"{c.name} dw not given {mode}"
    for i, d in enumerate(dws):
        if d is not None:
            E.check_col("qknorm_rope_bwd dw", d, r["dw"][i], r["B_dw"][i], f"{c.name} dw[{i}] {mode}",
                        prev=prev[i] if acc else None)


# ------------------------------------------------------------------------------------------
# gated add
@pytest.mark.parametrize("inp", E.GA_INPUTS)
@pytest.mark.parametrize("T,B,D", E.GA_SHAPES)
def test_gated_add(dev, T, B, D, inp):
    c = E.ga_case(T, B, D, inp)
    R, go = T * B, c.gate_off
    x, y, dout = E.wide(c.x.to(dev), D + 8), E.wide(c.y.to(dev), 2 * D + 8, D), E.wide(c.dout.to(dev), D + 16, 8)
    mod = c.mod.to(dev)
    obuf, o = E.guarded((), R, D, device=dev)
    K.gated_add_fwd(x, y, mod, go, B, out=o)
    dbuf, d = E.guarded((), R, D, ld=D + 40, device=dev)
    dmod = torch.full_like(mod, math.nan)
    K.gated_add_bwd(dout, y, mod, go, B, dmod, dy=d)
    E.ga_check("", c, {"out": o, "dy": d, "dgate": dmod[:, go:go + D]})
    assert E.guards_intact(obuf, R, D) and E.guards_intact(dbuf, R, D), c.name + " guards"
    assert E.outside_intact(dmod, lambda t: t[:, go:go + D]), c.name + " dmod outside the gate chunk"


# ------------------------------------------------------------------------------------------
# activations
@pytest.mark.parametrize("shape", E.ACT_SHAPES)
def test_activations(dev, shape):
    rows, C = shape
    xc, dyc, xsc = E.act_input(shape, 5), E.bf_randn(shape, 6, 2.0), E.act_input(shape, 5, silu=True)
    x, dy, xs = E.wide(xc.to(dev), C + 8), E.wide(dyc.to(dev), C + 16, 8), xsc.to(dev)
    nm = f"{shape}"
    # gelu_tanh forward / backward: strided sources, guarded destinations
    obuf, o = E.guarded((), rows, C, device=dev)
    K.gelu_tanh_fwd(x, out=o)
    E.act_check("gelu_tanh_fwd", "tanh", xc, o, "gelu_tanh_fwd " + nm)
    dbuf, d = E.guarded((), rows, C, ld=C + 24, device=dev)
    K.gelu_tanh_bwd(x, dy, dx=d)
    E.dact_check("gelu_tanh_bwd", "tanh", xc, dyc, d, "gelu_tanh_bwd " + nm)
    assert E.guards_intact(obuf, rows, C) and E.guards_intact(dbuf, rows, C), "gelu_tanh guards " + nm
    # act_fwd: out of place (guarded) and in place (strided); gated_act with ldh > 2F
    h = E.wide(torch.cat([xc, dyc], 1).to(dev), 2 * C + 8)
    for kind, name in ((K.ACT_QUICK_GELU, "quick"), (K.ACT_GELU_ERF, "erf"), (K.ACT_GELU_TANH, "tanh")):
        obuf, o = E.guarded((), rows, C, device=dev)
        K.act_fwd(x, kind, out=o)
        E.act_check("act_fwd " + name, name, xc, o, f"act_fwd {name} {nm}")
        assert E.guards_intact(obuf, rows, C), f"act_fwd {name} guards {nm}"
        ibuf, i = E.guarded((), rows, C, device=dev)
        i.copy_(x)
        K.act_fwd(i, kind)
        same(i, o, f"act_fwd {name} in place {nm}")
        assert E.guards_intact(ibuf, rows, C), f"act_fwd {name} in place guards {nm}"
        gbuf, g = E.guarded((), rows, C, device=dev)   # ldh = 2 C + 8, ldo = C + 16
        raw("otamd_gated_act_fwd", h, h.stride(0), g, g.stride(0), rows, C, kind)
        E.act_check("gated_act_fwd " + name, name, xc, g, f"gated_act_fwd {name} {nm}", g=dyc)
        assert E.guards_intact(gbuf, rows, C), f"gated_act_fwd {name} guards {nm}"
        same(K.gated_act_fwd(h, kind), g, f"gated_act_fwd {name} dense destination {nm}")
    # SiLU (dense), destinations inside guards
    n, dyd = rows * C, dyc.to(dev)
    sbuf, sy = flat(n, BF, dev)
    raw("otamd_silu_fwd", xs, sy, n)
    E.act_check("silu_fwd", "silu", xsc, sy.view(rows, C), "silu_fwd " + nm)
    bbuf, sdx = flat(n, BF, dev)
    raw("otamd_silu_bwd", xs, dyd, sdx, n)
    E.dact_check("silu_bwd", "silu", xsc, dyc, sdx.view(rows, C), "silu_bwd " + nm)
    assert flat_ok(sbuf) and flat_ok(bbuf), "silu guards " + nm
    same(K.silu_fwd(xs).view(-1), sy, "silu_fwd wrapper " + nm)
    same(K.silu_bwd(xs, dyd).view(-1), sdx, "silu_bwd wrapper " + nm)
    # GEGLU: both hosts, then strided / guarded through the ctypes path
    hc = torch.cat([E.bf_randn(shape, 7, 2.0), xc], 1)
    hd, hs = hc.to(dev), E.wide(hc.to(dev), 2 * C + 8)
    m = E.geglu_math(hc, dyc, F64)
    f1, f2 = both(lambda: K.geglu_fwd(hd))
    same(f1, f2, "geglu_fwd hosts " + nm)
    b1, b2 = both(lambda: K.geglu_bwd(hd, dyc.to(dev)))
    same(b1, b2, "geglu_bwd hosts " + nm)
    obuf, o = E.guarded((), rows, C, device=dev)
    K.geglu_fwd(hs, out=o)
    same(o, f1, "geglu_fwd strided " + nm)
    dbuf, d = E.guarded((), rows, 2 * C, device=dev)
    K.geglu_bwd(hs, dy, dh=d)
    same(d, b1, "geglu_bwd strided " + nm)
    assert E.guards_intact(obuf, rows, C) and E.guards_intact(dbuf, rows, 2 * C), "geglu guards " + nm
    E.check("geglu_fwd", f1, m["out"], m["T_out"], "geglu_fwd " + nm)
    E.check("geglu_bwd", b1[:, :C], m["da"], m["T_da"], "geglu_bwd da " + nm)
    E.check("geglu_bwd", b1[:, C:], m["dg"], m["T_dg"], "geglu_bwd dg " + nm)


def test_geglu_no_rows(dev):
    h, o = nans((1, 16), BF, dev), nans((1, 8), BF, dev)
    assert status("otamd_geglu_fwd", h, 16, o, 8, 0, 8) == 0
    assert status("otamd_geglu_bwd", h, 16, o, 8, h, 16, 0, 8) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all()) and bool(torch.isnan(h).all())


# ------------------------------------------------------------------------------------------
# text.hip rows
@pytest.mark.parametrize("inp", E.RMS_INPUTS)
@pytest.mark.parametrize("rows,C", E.rms_cases())
def test_rmsnorm(dev, rows, C, inp):
    c = E.rms_case(rows, C, inp)
    x, w = E.wide(c.x.to(dev), C + 8), c.w.to(dev)
    obuf, o = E.guarded((), rows, C, device=dev)
    raw("otamd_rmsnorm_fwd", x, x.stride(0), o, o.stride(0), rows, C, c.eps, w)
    E.check_rms("rmsnorm_fwd", o, c.x, c.w, c.eps, c.name)
    assert E.guards_intact(obuf, rows, C), c.name + " guards"
    same(K.rmsnorm_fwd(x, w, c.eps), o, c.name + " dense destination")


@pytest.mark.parametrize("with_pos", [True, False])
@pytest.mark.parametrize("B,T,D,vocab", E.EMBED_CASES)
def test_embed_tokens(dev, B, T, D, vocab, with_pos):
    c = E.embed_case(B, T, D, vocab)
    ids, tok, pos = c.ids.to(dev), c.tok.to(dev), c.pos.to(dev) if with_pos else None
    buf, o = flat(B * T * D, BF, dev)
    raw("otamd_embed_tokens", ids, B * T, T, tok, pos, o, D, vocab)
    E.check_bits("embed_tokens", o.view(B * T, D).cpu(), E.embed_math(c, with_pos), f"{c.name} pos={with_pos}")
    assert flat_ok(buf), c.name + " guards"
    same(K.embed_tokens(ids, tok, pos).view(-1), o, c.name + " wrapper")


# ------------------------------------------------------------------------------------------
# elementwise.hip
@pytest.mark.parametrize("N,H,W,C", E.UPS_CASES)
def test_upsample2x_bwd(dev, N, H, W, C):
    dup, prev = E.bf_randn((N, 2 * H, 2 * W, C), 1, 2.0), E.bf_randn((N, H, W, C), 2, 4.0)
    for p in (None, prev):
        buf = nans(N * H * W * C + 16, BF, dev)
        o = buf[8:-8].view(N, H, W, C)
        if p is not None:
            o.copy_(p)
        K.upsample2x_bwd(dup.to(dev), out=o, accumulate=p is not None)
        r, b = E.ups_math(dup, p, F64)
        E.check("upsample2x_bwd", o, r, U8 * r.abs() + b, f"upsample2x_bwd {N, H, W, C} acc={p is not None}")
        assert bool(torch.isnan(buf[:8]).all()) and bool(torch.isnan(buf[-8:]).all())


def colsum_run(dev, xc, xd, rpg, what):
    M, Nc = xc.shape
    groups = (M + (rpg or M) - 1) // (rpg or M)
    r, b = E.colsum_math(xc, rpg, F64)
    prev = E.bf_randn((groups, Nc), 4, 4.0)
    for dt in (F32, BF):
        for acc in (False, True):
            buf = nans(groups * Nc + 16, dt, dev)
            o = buf[8:-8].view(groups, Nc)
            if acc:
                o.copy_(prev)
            K.colsum(xd, rows_per_group=rpg, out=o, accumulate=acc)
            E.check_col("colsum", o, r, b, f"colsum {what} {dt} acc={acc}", prev=prev.to(dt) if acc else None)
            assert bool(torch.isnan(buf[:8]).all()) and bool(torch.isnan(buf[-8:]).all()), what + " guards"


@pytest.mark.parametrize("M,Nc,rpg", E.COLSUM_CASES)
def test_colsum(dev, M, Nc, rpg):
    x = E.N.in_row_scales((M, Nc), 3)
    colsum_run(dev, x, x.to(dev), rpg, f"{M, Nc, rpg}")


def test_colsum_column_slice(dev):
    M, ld, Nc, rpg = E.COLSUM_SLICE
    x = E.N.in_row_scales((M, Nc), 5)
    colsum_run(dev, x, E.wide(x.to(dev), ld, 8), rpg, f"slice {M, ld, Nc, rpg}")


def test_cast_add_concat_transpose(dev):
    for n in E.CAST_NS:
        x = (E._randn((n,), E._gen(n)) * 3).float()
        prev = E.bf_randn((n,), n + 1, 4.0)
        for dt in (BF, F32):
            for acc in (False, True):
                buf = nans(n + 16, dt, dev)
                o = buf[8:8 + n]
                if acc:
                    o.copy_(prev)
                K.cast_f32_bf16(x.to(dev), out=o, accumulate=acc)
                ref = ((prev.float() + x) if acc else x).to(dt)
                E.check_bits("cast_f32", o.cpu(), ref, f"cast_f32 n={n} {dt} acc={acc}")
                assert bool(torch.isnan(buf[:8]).all()) and bool(torch.isnan(buf[8 + n:]).all())
    a, b = E.N.in_row_scales((7, 24), 1), E.N.in_plain((7, 24), 2)
    buf, o = flat(a.numel(), BF, dev)
    K.add(a.to(dev), b.to(dev), out=o.view(7, 24))
    E.check_bits("add", o.view(7, 24).cpu(), (a.float() + b.float()).to(BF), "add")
    assert flat_ok(buf), "add guards"
    ca, cb = E.bf_randn((2, 5, 8), 3), E.bf_randn((2, 5, 8), 4)
    sa, sb = E.wide(ca.to(dev), 24, 8), E.wide(cb.to(dev), 16)
    buf, o = flat(2 * 5 * 16, BF, dev)
    raw("otamd_concat_channels", sa, 24, 8, sb, 16, 8, o, 10)
    E.check_bits("concat_channels", o.view(2, 5, 16).cpu(), torch.cat([ca, cb], -1), "concat_channels strided")
    assert flat_ok(buf), "concat_channels guards"
    same(K.concat_channels(sa, sb).view(-1), o, "concat_channels wrapper")
    w = E.bf_randn((5, 3, 3, 7), 5)
    buf, o = flat(w.numel(), BF, dev)
    raw("otamd_conv_weight_transpose", w.to(dev), o, 5, 9, 7)
    E.check_bits("conv_weight_transpose", o.view(7, 3, 3, 5).cpu(), w.permute(3, 1, 2, 0).contiguous(),
                 "conv_weight_transpose")
    assert flat_ok(buf), "conv_weight_transpose guards"
    same(K.conv_weight_transpose(w.to(dev)).view(-1), o, "conv_weight_transpose wrapper")


@pytest.mark.parametrize("dim", E.TS_DIMS)
def test_timestep_embedding(dev, dim):
    t = torch.tensor(E.TS_T, dtype=F32)
    obuf = nans((len(E.TS_T) + 2, dim + 8), BF, dev)
    o = obuf[1:-1, :dim]
    K.timestep_embedding(t.to(dev), dim, out=o)
    r, a = E.ts_math(t, dim, F64)
    E.check("timestep_embedding", o, r, U8 * r.abs() + a * 2.0 ** -21, f"timestep_embedding dim={dim} ldo={dim + 8}")
    assert E.outside_intact(obuf, lambda v: v[1:-1, :dim]), "timestep_embedding guards"


@pytest.mark.parametrize("mul,add", E.IMG_MULADD)
@pytest.mark.parametrize("B,C,H,W,cpad", E.IMG_CASES)
def test_image_to_nhwc(dev, B, C, H, W, cpad, mul, add):
    img = torch.rand((B, C, H, W), generator=E._gen(9), dtype=F32)
    buf, o = flat(B * H * W * cpad, BF, dev)
    raw("otamd_image_to_nhwc", img.to(dev), B, C, H, W, mul, add, o, cpad)
    assert flat_ok(buf), "image_to_nhwc guards"
    same(K.image_to_nhwc(img.to(dev), mul, add, cpad).view(-1), o, "image_to_nhwc wrapper")
    got = o.view(B, H, W, cpad).cpu()
    nm = f"image_to_nhwc {B, C, H, W, cpad} mul={mul}"
    if (mul, add) == (2.0, -1.0):
        ref = torch.zeros(B, H, W, cpad, dtype=BF)
        ref[..., :C] = (img * 2.0 - 1.0).permute(0, 2, 3, 1).to(BF)
        E.check_bits("image_to_nhwc", got, ref, nm)
    else:
        r, M = E.img_math(img, mul, add, cpad, F64)
        E.check("image_to_nhwc", got, r, U8 * r.abs() + 2.0 ** -23 * M, nm)
    assert not E.bits(got[..., C:]).any(), nm + " padded channels are +0"


@pytest.mark.parametrize("B,h,w,C", E.PACK_CASES)
def test_flux_pack(dev, B, h, w, C):
    lat = E.bf_randn((B, h, w, C), 6)
    src = E.wide(lat.to(dev), C + 8)
    buf, tok = flat(lat.numel(), BF, dev)
    raw("otamd_flux_pack", src, tok, B, h, w, C, C + 8, 0)
    assert flat_ok(buf), "flux_pack guards"
    tok = tok.view((h // 2) * (w // 2) * B, 4 * C)
    same(K.flux_pack(src), tok, "flux_pack wrapper")
    E.check_bits("flux_pack", tok.cpu(), E.pack_math(lat), f"flux_pack {B, h, w, C} ldl={C + 8}")
    E.check_bits("flux_pack", K.flux_unpack(tok, B, h, w, C).cpu(), lat, f"flux_unpack {B, h, w, C}")
    obuf = nans((B, h, w, C + 8), BF, dev)
    raw("otamd_flux_pack", tok, obuf, B, h, w, C, C + 8, 1)
    E.check_bits("flux_pack", obuf[..., :C].cpu(), lat, f"flux_unpack {B, h, w, C} ldl={C + 8}")
    assert E.outside_intact(obuf, lambda v: v[..., :C]), "flux_unpack guards"


# ------------------------------------------------------------------------------------------
# one launch past the 16384-block cap of each grid-stride kernel against the same op over the two halves of the rows
# (each half is covered at small size above); compared bit for bit on the device
BIG = 4 * 1024 * 1024 + 3   # 16-byte chunks (8-wide kernels) or elements (scalar kernels): 16384 x 256 + 3


def dev_randn(shape, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(shape, generator=g, device=dev, dtype=F32).to(BF)


def halves(fn, rows, *ts, cut=None):
    """fn(*row slices) -> tensor; whole against the two halves"""
    cut = rows // 2 if cut is None else cut
    whole = fn(*ts)
    parts = torch.cat([fn(*[t[:cut] for t in ts]), fn(*[t[cut:] for t in ts])])
    assert torch.equal(whole.view(torch.int16), parts.view(torch.int16))


def gs_rows(fn, widths, rows=BIG):
    """fn over [rows, w] bf16 operands (one per width) against fn over the two halves of the rows"""
    return lambda d: halves(fn, rows, *[dev_randn((rows, w), d, k + 1) for k, w in enumerate(widths)])


def gs_gated_add(d):
    mod = dev_randn((1, 16), d, 3)   # B = 1, so that r % B is the same in a half
    halves(lambda x, y: K.gated_add_fwd(x, y, mod, 8, 1), BIG, dev_randn((BIG, 8), d, 1), dev_randn((BIG, 8), d, 2))


def gs_embed(d):
    tok, pos, rows = dev_randn((50, 8), d, 1), dev_randn((77, 8), d, 2), BIG // 77 + 1   # whole sequences per half
    halves(lambda ids: K.embed_tokens(ids, tok, pos), rows, torch.randint(0, 50, (rows, 77), device=d))


def gs_timestep(d):
    halves(lambda t: K.timestep_embedding(t, 256), 32769, torch.rand(32769, device=d) * 1000)   # 32769 x 128 threads


def gs_image(d):
    halves(K.image_to_nhwc, 2, torch.rand((2, 1, 1, BIG // 2 + 1), device=d))   # one thread per pixel


GS = {
    "gelu_tanh_fwd": gs_rows(K.gelu_tanh_fwd, (8,)),
    "gelu_tanh_bwd": gs_rows(K.gelu_tanh_bwd, (8, 8)),
    "gated_add_fwd": gs_gated_add,
    "act_fwd": gs_rows(lambda x: K.act_fwd(x, K.ACT_GELU_ERF, out=torch.empty_like(x)), (8,)),
    "gated_act_fwd": gs_rows(lambda h: K.gated_act_fwd(h, K.ACT_GELU_TANH), (16,)),
    "geglu_fwd": gs_rows(K.geglu_fwd, (16,)),
    "geglu_bwd": gs_rows(K.geglu_bwd, (16, 8)),
    "silu_fwd": gs_rows(K.silu_fwd, (8,)),
    "silu_bwd": gs_rows(K.silu_bwd, (8, 8)),
    "add": gs_rows(K.add, (8, 8)),
    "concat_channels": gs_rows(K.concat_channels, (8, 8)),
    "upsample2x_bwd": lambda d: halves(K.upsample2x_bwd, BIG, dev_randn((BIG, 2, 2, 8), d, 1)),
    "timestep_embedding": gs_timestep,
    "image_to_nhwc": gs_image,
    "embed_tokens": gs_embed,
}


@pytest.mark.parametrize("op", sorted(GS))
def test_grid_stride(dev, op):
    GS[op](dev)
    E.note(op + " (grid stride)", 0.0, "one launch past the cap == two launches over the halves")


def test_grid_stride_scalar_kernels(dev):
    """the element-wise kernels whose result is a permutation or one IEEE operation: against torch on the device"""
    x = torch.randn(BIG, device=dev)
    prev = dev_randn((BIG,), dev, 2)
    assert torch.equal(K.cast_f32_bf16(x).view(torch.int16), x.to(BF).view(torch.int16))
    o = prev.clone()
    K.cast_f32_bf16(x, out=o, accumulate=True)
    assert torch.equal(o.view(torch.int16), (prev.float() + x).to(BF).view(torch.int16))
    w = dev_randn((BIG // 4 + 1, 1, 1, 4), dev, 3)
    assert torch.equal(K.conv_weight_transpose(w), w.permute(3, 1, 2, 0).contiguous())
    lat = dev_randn((1, 2, BIG // 4 + 2, 2), dev, 4)
    tok = K.flux_pack(lat)
    assert torch.equal(tok, E.pack_math(lat)) and torch.equal(K.flux_unpack(tok, *lat.shape), lat)
    # mod_reduce_kernel: B D past the cap with one token per sample, where dgate = bf16(dout y) and dy = bf16(gate dout)
    B, D = 1026, 4096
    dout, y, mod = dev_randn((B, D), dev, 5), dev_randn((B, D), dev, 6), dev_randn((B, D), dev, 7)
    dmod = torch.empty_like(mod)
    dy = K.gated_add_bwd(dout, y, mod, 0, B, dmod)
    assert torch.equal(dmod.view(torch.int16), (dout.float() * y.float()).to(BF).view(torch.int16))
    assert torch.equal(dy.view(torch.int16), (mod.float() * dout.float()).to(BF).view(torch.int16))
    for k in ("cast_f32", "conv_weight_transpose", "flux_pack", "gated_add_bwd mod_reduce"):
        E.note(k + " (grid stride)", 0.0, "bit-equal to torch on the device")


# ------------------------------------------------------------------------------------------
def test_einval_surfaces(dev):
    """preconditions the kernels rely on are refused by the C entry points (status OTAMD_EINVAL = 1 from the raw
    call) before anything is launched: the NaN-filled destinations keep their bits"""
    EINVAL = 1
    dim = 16
    t1, o1 = torch.ones(1, device=dev), nans((1, dim), BF, dev)
    # first, and the gate for the calls below: with one row the row stride is never used, so where the check is
    # absent this call only writes the row it was given and the test ends here
    assert status("otamd_timestep_embedding", t1, 1, dim, o1, dim - 2) == EINVAL
    n = 3
    t, o = torch.ones(n, device=dev), nans((n, dim), BF, dev)
    for ldo in (dim - 2, 0, -dim):
        assert status("otamd_timestep_embedding", t, n, dim, o, ldo) == EINVAL
    assert status("otamd_timestep_embedding", t, n, 0, o, dim) == EINVAL
    T, B, D = 4, 2, 16
    z = lambda *s: torch.ones(s, dtype=BF, device=dev)   # noqa: E731
    dout, y, dy, mod = z(T * B, D), z(T * B, D), nans((T * B, D), BF, dev), z(B, 4 * D + 8)
    dmod = torch.full_like(mod, math.nan)
    part = torch.empty(K.lib().otamd_mod_part_floats(T, D, B) + 4, device=dev)

    def ga(m, goff, p=part):
        return status("otamd_gated_add_bwd", dout, D, y, D, dy, D, T * B, D, m, mod.stride(0), goff, B, dmod, p)

    assert ga(mod, 4) == EINVAL and ga(mod, 12) == EINVAL and ga(mod, -8) == EINVAL
    assert ga(mod.view(-1)[4:], 8) == EINVAL   # mod 8-byte but not 16-byte aligned
    assert part[2:].data_ptr() % 16 == 8 and ga(mod, 8, part[2:]) == EINVAL   # the float4 stores of the partials
    # q/k norm weights that are not 8-byte aligned; weight gradients that are not aligned to their element
    c = E.qk_case(2, 1, 1, 1, True, "plain")
    G = E.qk_geom(1)
    x, cs, sn, dyq = c.x.to(dev), c.cs.to(dev), c.sn.to(dev), c.dy.to(dev)
    good = [c.w[i].to(dev).clone() for i in range(4)]
    odd = torch.ones(136, dtype=BF, device=dev)[2:130]
    assert odd.data_ptr() % 8 == 4
    dx = nans((2, G["lddx"]), BF, dev)
    ws = torch.empty(512 * 1024, device=dev)

    def qk(w):
        a = K._qk_args(x, G["qoff"], G["koff"], 1, 1, 1, w, cs, sn, c.eps)
        a.y, a.ldy, a.yqoff, a.ykoff = K._p(dx), G["lddx"], G["dxqoff"], G["dxkoff"]
        a.dy, a.lddy, a.dyqoff, a.dykoff = K._p(dyq), 256, 0, 128
        return a

    for i in range(4):
        w = list(good)
        w[i] = odd
        a = qk(w)
        assert K.lib().otamd_qknorm_rope_fwd(ctypes.byref(a), K.stream_handle()) == EINVAL, f"weight {i}"
        assert K.lib().otamd_qknorm_rope_bwd(ctypes.byref(a), None, None, None, None, 1, 0, None,
                                             K.stream_handle()) == EINVAL, f"weight {i} bwd"
    a = qk(good)
    dwb = nans(256, BF, dev)
    for i in range(4):
        for f32, off in ((1, 2), (0, 1)):   # an fp32 destination 2 bytes off, a bf16 destination 1 byte off
            ptrs = [None] * 4
            ptrs[i] = dwb.data_ptr() + off
            assert K.lib().otamd_qknorm_rope_bwd(ctypes.byref(a), *ptrs, f32, 0, K._p(ws),
                                                 K.stream_handle()) == EINVAL, f"dw {i} f32={f32} off={off}"
    torch.cuda.synchronize()
    for d in (o, dy, dmod, dx, dwb):
        assert bool(torch.isnan(d).all()), "a refused call wrote"


KERNELS = ["qknorm_rope_fwd", "qknorm_rope_bwd dx", "qknorm_rope_bwd dw", "gated_add_fwd", "gated_add_bwd dy",
           "gated_add_bwd dgate", "gelu_tanh_fwd", "gelu_tanh_bwd", "flux_pack", "embed_tokens", "act_fwd quick",
           "act_fwd erf", "act_fwd tanh", "gated_act_fwd quick", "gated_act_fwd erf", "gated_act_fwd tanh", "rmsnorm_fwd",
           "geglu_fwd", "geglu_bwd", "silu_fwd", "silu_bwd", "concat_channels", "upsample2x_bwd", "colsum",
           "conv_weight_transpose", "cast_f32", "timestep_embedding", "add", "image_to_nhwc"]


def test_worst_ratios_report():
    """the worst |err| / bound of every kernel whose tests ran in this process; all at most 1"""
    rows = {k: v for k, v in E.WORST.items() if not k.startswith("cpu:")}
    print()
    for k in sorted(rows):
        print(f"{k:40s} {rows[k][0]:8.3f}  {rows[k][1]}")
    missing = [k for k in KERNELS if k not in rows]
    if missing:
        print("not run in this process:", missing)
    assert all(v[0] <= 1 for v in rows.values())
