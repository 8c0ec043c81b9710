"""GroupNorm(+SiLU), LayerNorm and FLUX adaLN kernels against float64 references, element by element, on every kernel
the dispatchers can pick, in every mode, on hard inputs and inside guarded buffers (GPU).

Bounds are derived, not chosen (tests/_norm_edges.py): one bf16 rounding of the float64 value plus 2^-17 times the
absolute terms of the formula the kernel is entitled to, on every element.  tests/test_norm_edges_ref.py shows on
the CPU that an honest fp32 evaluation meets them and that planted errors do not."""
import math

import pytest
import torch

import _norm_edges as E
from onetrainer_amd import kernels as K

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F32 = torch.float32


def both(fn):
    """fn() through the native host layer, then through the ctypes path"""
    assert K.host_layer() == "native"
    a = fn()
    with K.python_host():
        b = fn()
    return a, b


def same(a, b, what=""):
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            same(x, y, what)
        return
    if a is None:
        assert b is None, what
        return
    assert a.shape == b.shape and a.dtype == b.dtype, what
    bits = torch.int16 if a.dtype == BF else torch.int32
    assert torch.equal(a.contiguous().view(bits), b.contiguous().view(bits)), what   # bit-equal, NaN included


def nans(n, dtype, dev):
    return torch.full((n,), math.nan, dtype=dtype, device=dev)


def dabs(t):
    return t.double().abs()


# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inp", E.INPUTS)
@pytest.mark.parametrize("C,rows", E.ln_cases())
def test_layernorm(dev, C, rows, inp):
    c = E.ln_case(C, rows, inp)
    r, nm = c.ref, c.name
    rowgroup = E.ln_pick(C // 8)[0] != 0
    x, g, b, dy, dres, prev, pg, pb = (t.to(dev) for t in (c.x, c.gamma, c.beta, c.dy, c.dres, c.prev, c.pg, c.pb))
    # forward, native and ctypes host
    (y, st), (y2, st2) = both(lambda: K.layernorm_fwd(x, g, b, c.eps))
    same((y, st), (y2, st2), nm + " fwd hosts")
    E.check_elem(y, r["y"], r["M_y"], nm + " y")
    E.check_row_stats(st[0], st[1], r, nm)
    # strided x (column slice of a 3 C wide buffer), out= inside guards
    xs, dys, drs = E.wide(x, 3 * C, C), E.wide(dy, C + 8), E.wide(dres, 3 * C, 2 * C)
    obuf, o = E.guarded((), rows, C, device=dev)
    yo, sto = K.layernorm_fwd(xs, g, b, c.eps, out=o)
    same((yo, sto), (y, st), nm + " fwd strided")
    assert E.guards_intact(obuf, rows, C), nm + " fwd guards"
    # backward: fp32 parameter gradients
    dx, dg, db = K.layernorm_bwd(x, dy, g, st)
    E.check_elem(dx, r["dx"], r["M_dx"], nm + " dx")
    E.check_col(dg, r["dgamma"], r["B_dgamma"], nm + " dgamma fp32")
    E.check_col(db, r["dbeta"], r["B_dbeta"], nm + " dbeta fp32")
    dxn, n1, n2 = K.layernorm_bwd(x, dy, g, st, need_param_grads=False)
    assert n1 is None and n2 is None
    same(dxn, dx, nm + " dx without parameter gradients")
    # bf16 destinations; then accumulated onto earlier content
    bg, bb = nans(C, BF, dev), nans(C, BF, dev)
    K.layernorm_bwd(x, dy, g, st, dgamma=bg, dbeta=bb)
    E.check_col(bg, r["dgamma"], r["B_dgamma"], nm + " dgamma bf16")
    E.check_col(bb, r["dbeta"], r["B_dbeta"], nm + " dbeta bf16")
    ag, ab = pg.clone(), pb.clone()
    K.layernorm_bwd(x, dy, g, st, dgamma=ag, dbeta=ab, param_acc=True)
    E.check_col(ag, r["dgamma"], r["B_dgamma"], nm + " dgamma bf16 param_acc", prev=pg)
    E.check_col(ab, r["dbeta"], r["B_dbeta"], nm + " dbeta bf16 param_acc", prev=pb)
    fg, fb = pg.float(), pb.float()
    K.layernorm_bwd(x, dy, g, st, dgamma=fg, dbeta=fb, param_acc=True)
    E.check_col(fg, r["dgamma"], r["B_dgamma"], nm + " dgamma fp32 param_acc", prev=pg.float())
    E.check_col(fb, r["dbeta"], r["B_dbeta"], nm + " dbeta fp32 param_acc", prev=pb.float())
    # the parameter-gradient half alone, both hosts; bit-equal to the fused call where both run the slab kernels
    sg, sb, sg2, sb2 = (nans(C, F32, dev) for _ in range(4))
    K.layernorm_param_grad(x, dy, st, sg, sb)
    with K.python_host():
        K.layernorm_param_grad(xs, dys, st, sg2, sb2)
    same((sg, sb), (sg2, sb2), nm + " param_grad hosts / strides")
    E.check_col(sg, r["dgamma"], r["B_dgamma"], nm + " param_grad dgamma")
    E.check_col(sb, r["dbeta"], r["B_dbeta"], nm + " param_grad dbeta")
    if rowgroup:
        same((sg, sb), (dg, db), nm + " param_grad alone against fused")
    hg, hb = pg.clone(), pb.clone()
    K.layernorm_param_grad(x, dy, st, hg, hb, param_acc=True)
    E.check_col(hg, r["dgamma"], r["B_dgamma"], nm + " param_grad dgamma bf16 param_acc", prev=pg)
    E.check_col(hb, r["dbeta"], r["B_dbeta"], nm + " param_grad dbeta bf16 param_acc", prev=pb)
    # dx + dres in one pass (fallback widths: two passes, the sum of two bf16 values rounded again)
    dr1, dr2 = both(lambda: K.layernorm_bwd_res(x, dy, dres, g, st))
    same(dr1, dr2, nm + " bwd_res hosts")
    M = r["M_dx"] + dabs(c.dres)
    if rowgroup:
        E.check_elem(dr1, r["dx"] + c.dres.double(), M, nm + " dx + dres")
        same(K.layernorm_bwd_res(xs, dys, drs, g, st), dr1, nm + " bwd_res strided")
    else:
        same(dr1, (dx.float() + dres.float()).to(BF), nm + " bwd_res two passes")
        E.check_abs(dr1, r["dx"] + c.dres.double(), E.U8 * (dabs(r["dx"]) + dabs(r["dx"] + c.dres.double()))
                    + E.U17 * M, nm + " dx + dres (two roundings)")
    # accumulate onto earlier dx, strided operands, guarded destination
    abuf, a = E.guarded((), rows, C, device=dev)
    a.copy_(prev)
    K.layernorm_bwd(xs, dys, g, st, dx=a, accumulate=True, need_param_grads=False)
    E.check_elem(a, r["dx"] + c.prev.double(), r["M_dx"] + dabs(c.prev), nm + " dx accumulated")
    assert E.guards_intact(abuf, rows, C), nm + " accumulate guards"
    dbuf, d = E.guarded((), rows, C, ld=3 * C + 16, device=dev)
    K.layernorm_bwd(xs, dys, g, st, dx=d, need_param_grads=False)
    same(d, dx, nm + " dx strided")
    assert E.guards_intact(dbuf, rows, C), nm + " bwd guards"


# ------------------------------------------------------------------------------------------
def gn_run(c, dev, affine_note=""):
    N, HW, C, G, silu = c.N, c.HW, c.C, c.G, c.silu
    r, nm = c.ref, c.name + affine_note
    x, dy, dres, prev, pg, pb = (t.to(dev) for t in (c.x, c.dy, c.dres, c.prev, c.pg, c.pb))
    g = None if c.gamma is None else c.gamma.to(dev)
    b = None if c.beta is None else c.beta.to(dev)
    xs, dys, drs = E.wide(x, 3 * C, C), E.wide(dy, C + 8), E.wide(dres, 3 * C, 2 * C)
    # one buffer for all images: the image stride must equal HW rows, so guard rows sit around the whole block
    obuf, o = E.guarded((), N * HW, C, device=dev)
    o = o.view(N, HW, C)
    y, st = K.groupnorm_fwd(xs, g, b, G, c.eps, silu, out=o)
    E.check_elem(y, r["y"], r["M_y"], nm + " y")
    E.check_group_stats(st[0], st[1], r, nm)
    assert E.guards_intact(obuf, N * HW, C), nm + " fwd guards"
    if g is not None:
        (y1, st1), (y2, st2) = both(lambda: K.groupnorm_fwd(x, g, b, G, c.eps, silu))
        same((y1, st1), (y2, st2), nm + " fwd hosts")
        same((y1, st1), (y, st), nm + " fwd strided")
    # backward into a guarded dx: fp32 parameter gradients
    dbuf, d = E.guarded((), N * HW, C, ld=3 * C + 16, device=dev)
    d = d.view(N, HW, C)
    dx, dg, db = K.groupnorm_bwd(xs, dys, g, G, silu, st, dx=d)
    E.check_elem(dx, r["dx"], r["M_dx"], nm + " dx")
    E.check_col(dg, r["dgamma"], r["B_dgamma"], nm + " dgamma fp32")
    E.check_col(db, r["dbeta"], r["B_dbeta"], nm + " dbeta fp32")
    assert E.guards_intact(dbuf, N * HW, C), nm + " bwd guards"
    d2 = torch.full_like(x, math.nan)
    _, n1, n2 = K.groupnorm_bwd(x, dy, g, G, silu, st, dx=d2, need_param_grads=False)
    assert n1 is None and n2 is None
    same(d2, dx, nm + " dx without parameter gradients")
    # bf16 destinations, then accumulated; fp32 accumulated
    bg, bb = nans(C, BF, dev), nans(C, BF, dev)
    K.groupnorm_bwd(x, dy, g, G, silu, st, dx=d2, dgamma=bg, dbeta=bb)
    E.check_col(bg, r["dgamma"], r["B_dgamma"], nm + " dgamma bf16")
    E.check_col(bb, r["dbeta"], r["B_dbeta"], nm + " dbeta bf16")
    ag, ab = pg.clone(), pb.clone()
    K.groupnorm_bwd(x, dy, g, G, silu, st, dx=d2, dgamma=ag, dbeta=ab, param_acc=True)
    E.check_col(ag, r["dgamma"], r["B_dgamma"], nm + " dgamma bf16 param_acc", prev=pg)
    E.check_col(ab, r["dbeta"], r["B_dbeta"], nm + " dbeta bf16 param_acc", prev=pb)
    fg, fb = pg.float(), pb.float()
    K.groupnorm_bwd(x, dy, g, G, silu, st, dx=d2, dgamma=fg, dbeta=fb, param_acc=True)
    E.check_col(fg, r["dgamma"], r["B_dgamma"], nm + " dgamma fp32 param_acc", prev=pg.float())
    E.check_col(fb, r["dbeta"], r["B_dbeta"], nm + " dbeta fp32 param_acc", prev=pb.float())
    # dx + dres in the apply pass, guarded
    rbuf, rd = E.guarded((), N * HW, C, device=dev)
    rd = rd.view(N, HW, C)
    K.groupnorm_bwd(xs, dys, g, G, silu, st, dx=rd, dres=drs, need_param_grads=False)
    E.check_elem(rd, r["dx"] + c.dres.double(), r["M_dx"] + dabs(c.dres), nm + " dx + dres")
    assert E.guards_intact(rbuf, N * HW, C), nm + " bwd_res guards"
    # accumulate onto earlier dx
    a = prev.clone()
    K.groupnorm_bwd(x, dy, g, G, silu, st, dx=a, accumulate=True, need_param_grads=False)
    E.check_elem(a, r["dx"] + c.prev.double(), r["M_dx"] + dabs(c.prev), nm + " dx accumulated")
    if g is not None:   # no destinations: native and ctypes host
        same(*both(lambda: K.groupnorm_bwd(x, dy, g, G, silu, st)), nm + " bwd hosts")
        r1, r2 = both(lambda: K.groupnorm_bwd(x, dy, g, G, silu, st, dres=dres))
        same(r1, r2, nm + " bwd_res hosts")
        same(r1[0], rd, nm + " bwd_res strided")
        same(r1[1:], (dg, db), nm + " bwd_res parameter gradients")


@pytest.mark.parametrize("inp", E.INPUTS)
@pytest.mark.parametrize("silu,eps", E.GN_MODES)
@pytest.mark.parametrize("N,HW,C,G", E.GN_SHAPES)
def test_groupnorm(dev, N, HW, C, G, silu, eps, inp):
    gn_run(E.gn_case(N, HW, C, G, silu, eps, inp), dev)


@pytest.mark.parametrize("inp", E.INPUTS)
@pytest.mark.parametrize("N,HW,C,G", E.GN_SHAPES)
def test_groupnorm_null_affine(dev, N, HW, C, G, inp):
    """gamma = beta = nullptr through the ctypes path (out= / dx= given)"""
    gn_run(E.gn_case(N, HW, C, G, True, 1e-5, inp, False), dev)


# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inp", E.INPUTS)
@pytest.mark.parametrize("T,B,D", E.ADALN_SHAPES)
def test_adaln(dev, T, B, D, inp):
    c = E.adaln_case(T, B, D, inp)
    r, nm = c.ref, c.name
    R, so, co = T * B, c.shift_off, c.scale_off
    x, dy, dres, mod = (t.to(dev) for t in (c.x, c.dy, c.dres, c.mod))
    xs, dys, drs = E.wide(x, 3 * D, D), E.wide(dy, D + 8), E.wide(dres, 3 * D, 2 * D)
    y, st = K.adaln_fwd(x, mod, so, co, B, eps=c.eps)
    E.check_elem(y, r["y"], r["M_y"], nm + " y")
    E.check_row_stats(st[0], st[1], r, nm)
    obuf, o = E.guarded((), R, D, device=dev)
    same(K.adaln_fwd(xs, mod, so, co, B, eps=c.eps, out=o), (y, st), nm + " fwd strided")
    assert E.guards_intact(obuf, R, D), nm + " fwd guards"

    def check_dmod(dm, what):
        E.check_col(dm[:, so:so + D], r["dshift"], r["B_dshift"], f"{nm} dshift {what}")
        E.check_col(dm[:, co:co + D], r["dscale"], r["B_dscale"], f"{nm} dscale {what}")
        rest = dm.cpu().view(torch.int16).clone()
        rest[:, so:co + D] = E.NANBITS
        assert bool((rest == E.NANBITS).all()), f"{nm} dmod outside the two chunks {what}"

    dmod = torch.full_like(mod, math.nan)
    dx = K.adaln_bwd(x, dy, mod, so, co, B, st, dmod=dmod)
    E.check_elem(dx, r["dx"], r["M_dx"], nm + " dx")
    check_dmod(dmod, "fused")
    same(K.adaln_bwd(x, dy, mod, so, co, B, st), dx, nm + " dx without dmod")
    # the split form: the same bits
    dmod2 = torch.full_like(mod, math.nan)
    K.adaln_dmod(xs, dys, mod, so, co, B, st, dmod2)
    same(dmod2, dmod, nm + " adaln_dmod alone")
    # dres, strided operands, guarded dx
    dbuf, d = E.guarded((), R, D, ld=3 * D + 16, device=dev)
    dmod3 = torch.full_like(mod, math.nan)
    K.adaln_bwd(xs, dys, mod, so, co, B, st, dmod=dmod3, dx=d, dres=drs)
    E.check_elem(d, r["dx"] + c.dres.double(), r["M_dx"] + dabs(c.dres), nm + " dx + dres")
    assert E.guards_intact(dbuf, R, D), nm + " bwd_res guards"
    same(dmod3, dmod, nm + " dmod with dres")
    dbuf, d = E.guarded((), R, D, device=dev)
    K.adaln_bwd(xs, dys, mod, so, co, B, st, dx=d)
    same(d, dx, nm + " dx strided")
    assert E.guards_intact(dbuf, R, D), nm + " bwd guards"


# ------------------------------------------------------------------------------------------
def refused(fn, outs):
    """raises through check() and launches nothing: the NaN-filled destinations keep their bits"""
    before = [o.clone() for o in outs]
    with pytest.raises(RuntimeError, match="status"):
        fn()
    torch.cuda.synchronize()
    for o, b in zip(outs, before):
        same(o, b, "destination of a refused call")


def test_limits_are_refused(dev):
    def bf(*s):
        return torch.ones(*s, dtype=BF, device=dev)

    def nan(*s):
        return torch.full(s, math.nan, dtype=BF, device=dev)

    f = lambda n: torch.ones(n, dtype=F32, device=dev)   # noqa: E731
    # LayerNorm: C = 2056, C % 8, row stride % 8 -- native and ctypes host
    for C, ld in ((2056, 2056), (12, 16), (16, 20)):
        x, dy = bf(5, ld)[:, :C], bf(5, ld)[:, :C]
        g, b, o, st = bf(C), bf(C), nan(5, C), (f(5), f(5))
        with pytest.raises(RuntimeError, match="status"):
            K.layernorm_fwd(x, g, b, 1e-5)
        refused(lambda: K.layernorm_fwd(x, g, b, 1e-5, out=o), [o])
        refused(lambda: K.layernorm_bwd(x, dy, g, st, dx=o), [o])
        pgr = [torch.full((C,), math.nan, device=dev) for _ in range(2)]
        refused(lambda: K.layernorm_param_grad(x, dy, st, *pgr), pgr)
        with K.python_host():
            refused(lambda: K.layernorm_param_grad(x, dy, st, *pgr), pgr)
        with pytest.raises(RuntimeError, match="status"):
            K.layernorm_bwd_res(x, dy, dy, g, st)
    # GroupNorm: C = 4104 (513 threads), C % 8, row stride % 8
    for C, ld, G in ((4104, 4104, 8), (12, 16, 1), (16, 20, 2)):
        x, dy = bf(1, 6, ld)[..., :C], bf(1, 6, ld)[..., :C]
        g, b, o = bf(C), bf(C), nan(1, 6, C)
        st = (f(G), f(G), f(C), f(C))
        with pytest.raises(RuntimeError, match="status"):
            K.groupnorm_fwd(x, g, b, G, 1e-5, True)
        refused(lambda: K.groupnorm_fwd(x, g, b, G, 1e-5, True, out=o), [o])
        refused(lambda: K.groupnorm_bwd(x, dy, g, G, True, st, dx=o), [o])
        refused(lambda: K.groupnorm_bwd(x, dy, g, G, True, st, dx=o, dres=dy.contiguous()), [o])
        with pytest.raises(RuntimeError, match="status"):
            K.groupnorm_bwd(x, dy, g, G, True, st)
    # adaLN: D = 4104, D % 8, row stride % 8
    for D, ld in ((4104, 4104), (12, 16), (16, 20)):
        x, dy = bf(4, ld)[:, :D], bf(4, ld)[:, :D]
        mod, o, st = bf(2, 2 * ld), nan(4, D), (f(4), f(4))
        refused(lambda: K.adaln_fwd(x, mod, 0, 0, 2, out=o), [o])
        refused(lambda: K.adaln_bwd(x, dy, mod, 0, 0, 2, st, dx=o), [o])
        refused(lambda: K.adaln_bwd(x, dy, mod, 0, 0, 2, st, dx=o, dres=dy), [o])
