"""Exact GEMM tests: bf16 operands that hold small integers make every product and every partial sum an integer below
2^24, so the fp32 accumulation is exact in any order -- on any tile, with any split-K count, through the split-K slabs
and through the fused-LoRA second K segment.  The epilogue alpha * acc + bias + rowvec + residual (+ C) is computed in
fp32 and rounded once (csrc/gemm.h gemm_store4 / gemm_store8 / splitk_combine), so with a power-of-two alpha and integer
epilogue operands the output must be bit-identical to round_to_bf16(exact) (or to exact, for fp32 outputs), where
`exact` is a float64 CPU reference of the same operation.  Everything is compared with torch.equal: a dropped,
duplicated or misplaced element, K chunk, conv tap, split or epilogue term changes at least one output bit.

Every case runs on every tile of the catalogue through otamd_gemm_explicit (force_plan, which also counts the launches
and checks each OTAMD_EUNSUPPORTED against the allow-list of test_gemm_gpu.py), and on the default plan through both
host paths (the native layer and the ctypes one).

Shapes per tile (BM x BN): M = 2 BM + 24 (more than one tile row, ragged tail that is no multiple of 16), N = BN + 20
where only N % 4 is required (N % 8 == 4: the 4-column store tail) and BN + 24 where N % 8 is, K of 1 to 17 K-steps."""
import contextlib
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

from onetrainer_amd import kernels as K
from test_gemm_gpu import TILES, UNSUPPORTED_OK, ExplicitPlan, Unsupported

gpu = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32

# tile code -> (BM, BN): csrc/gemm_tiles.h, checked against otamd_gemm_tile_dims on the GPU (test_tile_dims)
DIMS = {-1: (128, 128), 0: (256, 256), 1: (256, 128), 2: (128, 256), 3: (256, 256), 4: (128, 128), 5: (128, 64),
        6: (64, 128), 7: (128, 160), 8: (256, 160), 9: (128, 64), 10: (64, 128)}
PLANS = (*TILES, "native", "python")   # every explicit tile, and the default plan through both host paths
KS = (8, 64, 72, 192, 200, 320, 1032)  # 1 to 17 K-steps of 64 with ragged tails; cycles the 2- and 4-deep LDS rings
SENTINEL = -512.0                      # pre-fill of the columns around a sliced output (a bf16 value)


def dims(plan):
    return DIMS[plan] if isinstance(plan, int) else (128, 128)


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(("gemm-exact",) + tuple(key)).encode()))


def ints(shape, lo, hi, g):
    """bf16 tensor of integers drawn uniformly from [lo, hi] (CPU; every value is exact in bf16 for |v| <= 256)"""
    assert -256 <= lo <= hi <= 256
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(BF)


def expected(ref64, dtype):
    assert ref64.dtype == torch.float64 and ref64.abs().max().item() < 2 ** 24   # fp32 sums of integers stay exact
    r = ref64.float()
    assert torch.equal(r.double(), ref64)   # the exact value is an fp32 number (integers, or halves with alpha = 0.5)
    return r if dtype == F32 else r.to(BF)


def same(out, ref64, what):
    want = expected(ref64.reshape(out.shape), out.dtype)
    got = out.detach().cpu()
    if not torch.equal(got, want):
        bad = got.float() != want.float()
        i = tuple(bad.nonzero()[0].tolist())
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact result, first at {i}: "
                    f"got {got[i].item()} want {want[i].item()}")


def rounding_exercised(ref64):
    """a bf16 output must round: >= 100 elements that are no bf16 number, and an exact tie (an odd integer between
    256 and 512 lies halfway between two bf16 numbers)"""
    r = ref64.float()
    assert int((r.to(BF).float() != r).sum()) >= 100
    a = r.abs()
    assert bool(((a > 256) & (a < 512) & (a % 2 == 1)).any())


def padded(t, start, width, fill=0.0):
    """t's values as a column slice [:, start:start+N] of a wider [rows, width] buffer (row stride != N)"""
    big = torch.full((t.shape[0], width), fill, dtype=t.dtype)
    big[:, start:start + t.shape[1]] = t
    return big


def wide_slice(t):     # 16-byte aligned column slice with a row stride that is a multiple of 8: the wide epilogue
    n = t.shape[1]
    return padded(t, 8, (n + 8 + 7) // 8 * 8 + 8), 8


def narrow_width(n):   # row stride with % 8 == 4 around an n-column slice starting at column 4: gemm_wide_ok() false
    return n + 8 + (4 if n % 8 == 0 else 0)


class Case(dict):
    """operands and float64 references of one shape (CPU, computed once); .on(dev) gives the device copies"""
    __getattr__ = dict.__getitem__

    def on(self, dev):
        if "_dev" not in self:
            self["_dev"] = Case({k: v.to(dev) for k, v in self.items() if isinstance(v, torch.Tensor) and v.dtype == BF})
        return self["_dev"]


# ---- plans ----------------------------------------------------------------------------------------
class _Plan:
    def __init__(self):
        self.launches, self.unsupported, self.issued = 0, [], 0

    def run(self, fn, *args, **kw):
        """one op that issues one GEMM; None when the explicit plan has no instance for its operand form"""
        self.issued += 1
        try:
            return fn(*args, **kw)
        except Unsupported:
            return None

    def done(self, more=0):
        assert self.launches > 0
        assert all(u in UNSUPPORTED_OK for u in self.unsupported)
        assert self.launches + len(self.unsupported) == self.issued + more, \
            (self.launches, self.unsupported, self.issued, more)


class Forced(_Plan, ExplicitPlan):
    def __init__(self, tile, splits):
        _Plan.__init__(self)
        ExplicitPlan.__init__(self, tile, splits)


class PythonDefault(_Plan):
    """the default plan through the ctypes host path: kernels._gemm itself, counted"""

    def __init__(self, gemm):
        super().__init__()
        self.gemm = gemm

    def __call__(self, a, splits, device):
        self.gemm(a, splits, device)
        self.launches += 1


class NativeDefault(_Plan):
    """the default plan through the native host layer (no Python hook below the op: ops are counted)"""

    def run(self, fn, *args, **kw):
        assert K.host_layer() == "native"
        out = super().run(fn, *args, **kw)
        self.launches += 1
        return out


@pytest.fixture
def force_plan(monkeypatch):
    """force_plan(tile, splits): the ops below launch otamd_gemm_explicit(tile, splits) from the ctypes host path,
    with a workspace from kernels._ws_bytes.  force_plan("python") / ("native"): the default plan through either host
    path.  Yields the plan's counters."""
    @contextlib.contextmanager
    def enter(plan, splits=1):
        if plan == "native":
            assert K.host_layer() == "native", "the native host layer is not built / not active"
            yield NativeDefault()
            return
        st = PythonDefault(K._gemm) if plan == "python" else Forced(plan, splits)
        with monkeypatch.context() as m, K.python_host():
            m.setattr(K, "_gemm", st)
            assert K.host_layer() == "python"
            yield st
    return enter


# ---- cases ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def linear_case(M, N, Kd):
    g = gen("linear", M, N, Kd)
    c = Case(x=ints((M, Kd), -3, 3, g), w=ints((N, Kd), -3, 3, g), bias=ints((N,), -40, 40, g),
             rowvec=ints(((M + 99) // 100, N), -40, 40, g), res=ints((M, N), -40, 40, g), c0=ints((M, N), -100, 100, g))
    c["rv_wide"], _ = wide_slice(c.rowvec)
    c["res_wide"], _ = wide_slice(c.res)
    c["res_narrow"] = padded(c.res, 4, narrow_width(N))
    c["P"] = c.x.double() @ c.w.double().t()
    return c


@functools.lru_cache(maxsize=None)
def dgrad_case(M, Nl, Kd):
    g = gen("dgrad", M, Nl, Kd)
    c = Case(dy=ints((M, Nl), -3, 3, g), w=ints((Nl, Kd), -3, 3, g), res=ints((M, Kd), -40, 40, g),
             c0=ints((M, Kd), -100, 100, g))
    c["res_wide"], _ = wide_slice(c.res)
    c["P"] = c.dy.double() @ c.w.double()
    return c


WGRAD_T = 1416   # tokens: no multiple of 64; effective split counts 1, 2, 3, 5, 8 for the requested 1, 2, 3, 5, 8


def eff_splits(Kd, s):
    """the split count the launcher makes of a request (gemm.hip gemm_impl: whole 64-deep K steps per split)"""
    kps = (-(-Kd // s) + 63) // 64 * 64
    return -(-Kd // kps)


@functools.lru_cache(maxsize=None)
def wgrad_case(T, N, Kd):
    g = gen("wgrad", T, N, Kd)
    c = Case(dy=ints((T, N), -3, 3, g), x=ints((T, Kd), -3, 3, g), c0=ints((N, Kd), -100, 100, g),
             db0=ints((N,), -100, 100, g))
    c["P"] = c.dy.double().t() @ c.x.double()
    c["db"] = c.dy.double().sum(0)
    return c


def nchw(t):
    return t.permute(0, 3, 1, 2).double()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# conv geometries: (ksize, stride, pad, upsample, out_hw); input 2 x 9 x 7 (ragged M)
G_S1, G_S2, G_UP, G_1X1, G_OUTHW = (3, 1, 1, False, None), (3, 2, 1, False, None), (3, 1, 1, True, None), \
    (1, 1, 0, False, None), (3, 2, 0, False, (5, 4))
IMG = (2, 9, 7)


def conv_src(x, geom):
    """the NCHW float64 image the conv reads: the nearest-2x upsample and the out_hw one-sided zero padding (taps past
    the bottom / right edge read zeros) restated in plain torch"""
    k, stride, pad, up, out_hw = geom
    xin = nchw(x)
    if up:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    if out_hw is not None:
        pb = (out_hw[0] - 1) * stride + k - 2 * pad - xin.shape[2]
        pr = (out_hw[1] - 1) * stride + k - 2 * pad - xin.shape[3]
        assert pb >= 0 and pr >= 0
        xin = F.pad(xin, (0, pr, 0, pb))
    return xin


@functools.lru_cache(maxsize=None)
def conv_case(Cin, Cout, geom):
    k, stride, pad, up, out_hw = geom
    g = gen("conv", Cin, Cout, geom)
    n, H, W = IMG
    x, w = ints((n, H, W, Cin), -3, 3, g), ints((Cout, k, k, Cin), -3, 3, g)
    base = nhwc(F.conv2d(conv_src(x, geom), nchw(w), None, stride=stride, padding=pad))
    P, Q = base.shape[1:3]
    c = Case(x=x, w=w, bias=ints((Cout,), -40, 40, g), rowvec=ints((n, Cout), -40, 40, g),
             res=ints((n, P, Q, Cout), -40, 40, g), dy=ints((n, P, Q, Cout), -3, 3, g),
             c0=ints((n, H, W, Cin), -100, 100, g), db0=ints((Cout,), -100, 100, g))
    c["fwd"] = base
    if out_hw is None and not up:
        c["dgrad"] = nhwc(torch.nn.grad.conv2d_input((n, Cin, H, W), nchw(w), nchw(c.dy), stride=stride, padding=pad))
    if out_hw is None:
        c["wgrad"] = nhwc(torch.nn.grad.conv2d_weight(conv_src(x, geom), (Cout, Cin, k, k), nchw(c.dy), stride=stride,
                                                      padding=pad))
        c["db"] = c.dy.double().sum((0, 1, 2))
    return c


def conv_cout(bn):
    return min(bn + 24, 152)   # capped: the conv cases stay small


@functools.lru_cache(maxsize=None)
def block_diag(P, pw, r, seed, lo=-3, hi=3):
    """a fused group's up operand: block-diagonal [P*pw, P*r]"""
    g = gen("block", P, pw, r, seed)
    up = torch.zeros(P * pw, P * r, dtype=BF)
    for p in range(P):
        up[p * pw:(p + 1) * pw, p * r:(p + 1) * r] = ints((pw, r), lo, hi, g)
    return up


# ---- the reference-only preconditions, on the CPU --------------------------------------------------
def test_reference_preconditions():
    """the K = 1032 bf16 outputs round (>= 100 unrepresentable elements and an exact tie), every sum stays below
    2^24 (expected() asserts it), and the split requests of the weight gradient reach 1, 2, 3, 5 and 8 splits"""
    for bm, bn in sorted(set(DIMS.values())):
        M = 2 * bm + 24
        rounding_exercised(linear_case(M, bn + 20, 1032).P)
        rounding_exercised(dgrad_case(M, 1032, bn + 24).P)
        expected(linear_case(M, bn + 20, 1032).P, BF)
        c = wgrad_case(WGRAD_T, M, bn + 24)
        rounding_exercised(c.P)
        expected(c.P + c.c0.double(), BF)
    assert [eff_splits(WGRAD_T, s) for s in (1, 2, 3, 5, 8)] == [1, 2, 3, 5, 8]
    assert WGRAD_T % 64 and [eff_splits(1032, s) for s in (3, 5)] == [3, 5]


@gpu
def test_tile_dims(dev):
    for t in TILES:
        assert K._tile_dims(t) == DIMS[t]


# ---- linear forward (K, K) ------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("plan", PLANS)
def test_linear_fwd_exact(dev, force_plan, plan):
    bm, bn = dims(plan)
    M, N = 2 * bm + 24, bn + 20   # N % 8 == 4: the 4-column tail of the wide store path
    W = narrow_width(N)
    with force_plan(plan) as st:
        for Kd in KS:
            c = linear_case(M, N, Kd)
            d = c.on(dev)
            bias, rowvec, res = c.bias.double(), c.rowvec.double().repeat_interleave(100, 0)[:M], c.res.double()
            rv_wide, res_wide, res_narrow = d.rv_wide[:, 8:8 + N], d.res_wide[:, 8:8 + N], d.res_narrow[:, 4:4 + N]
            full = c.P + bias + rowvec + res
            tag = f"linear fwd {plan} K={Kd}"
            same(st.run(K.linear, d.x, d.w), c.P, tag)
            same(st.run(K.linear, d.x, d.w, bias=d.bias), c.P + bias, tag + " bias")
            # bias + rowvec (100 rows per vector: no divisor of BM) + residual from a column slice (ldr != N)
            same(st.run(K.linear, d.x, d.w, bias=d.bias, rowvec=rv_wide, rows_per_vec=100, residual=res_wide), full,
                 tag + " bias+rowvec+residual")
            # ... with epilogue operands that rule the 16-byte accesses out: the narrow epilogue
            same(st.run(K.linear, d.x, d.w, bias=d.bias, rowvec=d.rowvec, rows_per_vec=100, residual=res_narrow), full,
                 tag + " bias+rowvec+residual narrow operands")
            same(st.run(K.linear, d.x, d.w, out=d.c0.clone(), accumulate=True), c.P + c.c0.double(), tag + " accumulate")
            same(st.run(K.linear, d.x, d.w, out_dtype=F32), c.P, tag + " fp32")
            same(st.run(K.linear, d.x, d.w, out=d.c0.float(), accumulate=True), c.P + c.c0.double(),
                 tag + " fp32 accumulate")
            for alpha in (0.5, 2.0, -1.0):
                same(st.run(K.linear, d.x, d.w, bias=d.bias, alpha=alpha), alpha * c.P + bias, tag + f" alpha={alpha}")
            # output written into big[:, 4:4+N] with a row stride % 8 == 4: the narrow path, bf16 and fp32 C; and into
            # a 16-byte aligned slice with a row stride % 8 == 0: the wide path, whose last 8-column granule of a row is
            # the 4-column tail (a contiguous C of this N has ldc % 8 == 4 and takes the narrow path)
            for c0_, width, dt, acc in ((s_, w_, dt_, acc_) for s_, w_ in ((4, W), (8, (N + 15) // 8 * 8 + 8))
                                        for dt_ in (BF, F32) for acc_ in (False, True)):
                big = torch.full((M, width), SENTINEL, dtype=dt, device=dev)
                out = big[:, c0_:c0_ + N]
                ref = 0.5 * c.P + full - c.P
                if acc:
                    out.copy_(d.c0)
                    ref = ref + c.c0.double()
                st.run(K.linear, d.x, d.w, bias=d.bias, rowvec=rv_wide, rows_per_vec=100, residual=res_wide, out=out,
                       alpha=0.5, accumulate=acc)
                same(out, ref, tag + f" out sliced at column {c0_} of {width} {dt} accumulate={acc}")
                rest = torch.cat([big[:, :c0_], big[:, c0_ + N:]], 1)
                assert bool((rest == SENTINEL).all()), tag + " wrote outside its output slice"
            if Kd == 1032:
                rounding_exercised(c.P)
        st.done()


@gpu
@pytest.mark.parametrize("tile", TILES)
def test_linear_fwd_splitk_exact(dev, force_plan, tile):
    """split-K on a forward GEMM (explicit plans only): the 8-wide combine with 16-byte operands, and its fall-through
    when an epilogue operand rules them out while C itself allows the 8-wide form (splitk_combine<8>)"""
    bm, bn = DIMS[tile]
    M, Kd = 2 * bm + 24, 1032
    for N, sp in ((bn + 24, 3), (bn + 24, 5), (bn + 20, 3), (bn + 20, 5)):   # N % 8 == 4: the 4-wide combine
        c = linear_case(M, N, Kd)
        d = c.on(dev)
        bias, res = c.bias.double(), c.res.double()
        res_wide, res_narrow = d.res_wide[:, 8:8 + N], d.res_narrow[:, 4:4 + N]
        with force_plan(tile, sp) as st:
            tag = f"linear fwd tile {tile} N={N} splits={sp}"
            same(st.run(K.linear, d.x, d.w), c.P, tag)
            same(st.run(K.linear, d.x, d.w, bias=d.bias, residual=res_wide, alpha=0.5), 0.5 * c.P + bias + res,
                 tag + " wide epilogue")
            same(st.run(K.linear, d.x, d.w, bias=d.bias, residual=res_narrow, alpha=0.5), 0.5 * c.P + bias + res,
                 tag + " narrow residual")
            same(st.run(K.linear, d.x, d.w, bias=d.bias, residual=res_narrow, out=d.c0.clone(), accumulate=True),
                 c.P + bias + res + c.c0.double(), tag + " narrow residual accumulate")
            same(st.run(K.linear, d.x, d.w, bias=d.bias, residual=res_narrow, out_dtype=F32), c.P + bias + res,
                 tag + " narrow residual fp32")
            st.done()


# ---- linear dgrad (K, MN) -------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("plan", PLANS)
def test_linear_dgrad_exact(dev, force_plan, plan):
    bm, bn = dims(plan)
    M, Kd = 2 * bm + 24, bn + 24
    with force_plan(plan) as st:
        for Nl in KS:
            c = dgrad_case(M, Nl, Kd)
            d = c.on(dev)
            tag = f"linear dgrad {plan} K={Nl}"
            same(st.run(K.linear_dgrad, d.dy, d.w), c.P, tag)
            same(st.run(K.linear_dgrad, d.dy, d.w, residual=d.res_wide[:, 8:8 + Kd]), c.P + c.res.double(),
                 tag + " residual")
            same(st.run(K.linear_dgrad, d.dy, d.w, out=d.c0.clone(), accumulate=True), c.P + c.c0.double(),
                 tag + " accumulate")
            same(st.run(K.linear_dgrad, d.dy, d.w, out=torch.empty(M, Kd, device=dev)), c.P, tag + " fp32")
            if Nl == 1032:
                rounding_exercised(c.P)
        st.done()


# ---- linear wgrad (MN, MN), split-K ---------------------------------------------------------------
@gpu
@pytest.mark.parametrize("plan", PLANS)
def test_linear_wgrad_exact(dev, force_plan, plan):
    bm, bn = dims(plan)
    T, N, Kd = WGRAD_T, 2 * bm + 24, bn + 24
    c = wgrad_case(T, N, Kd)
    d = c.on(dev)
    c0, db, db0 = c.c0.double(), c.db, c.db0.double()
    rounding_exercised(c.P)
    with force_plan(plan) as st:
        for sp in (1, 2, 3, 5, 8):   # 5 and 8 reach the unrolled loop of the split-K reduce
            tag = f"linear wgrad {plan} splits={sp}"
            same(st.run(K.linear_wgrad, d.dy, d.x, splits=sp), c.P, tag)
            same(st.run(K.linear_wgrad, d.dy, d.x, splits=sp, alpha=0.5), 0.5 * c.P, tag + " alpha=0.5")
            same(st.run(K.linear_wgrad, d.dy, d.x, splits=sp, out=d.c0.clone(), accumulate=True), c.P + c0,
                 tag + " accumulate")
            same(st.run(K.linear_wgrad, d.dy, d.x, splits=sp, out=d.c0.float(), accumulate=True, alpha=2.0),
                 2.0 * c.P + c0, tag + " fp32 accumulate")
            for dt in (BF, F32):     # fused bias gradient: overwritten and accumulated, itself exact
                bg = torch.full((N,), float("nan"), dtype=dt, device=dev)
                same(st.run(K.linear_wgrad, d.dy, d.x, splits=sp, bias_grad=bg), c.P, tag + f" bias_grad {dt}")
                same(bg, db, tag + f" the bias gradient {dt}")
                bg = d.db0.to(dt, copy=True)
                same(st.run(K.linear_wgrad, d.dy, d.x, splits=sp, bias_grad=bg, bias_acc=True), c.P,
                     tag + f" bias_grad {dt} accumulated")
                same(bg, db + db0, tag + f" the accumulated bias gradient {dt}")
            if sp in (1, 5):         # written to a sliced out whose row stride rules the 16-byte accesses out
                for dt in (BF, F32):
                    big = torch.full((N, narrow_width(Kd)), SENTINEL, dtype=dt, device=dev)
                    out = big[:, 4:4 + Kd]
                    out.copy_(d.c0)
                    st.run(K.linear_wgrad, d.dy, d.x, splits=sp, out=out, accumulate=True)
                    same(out, c.P + c0, tag + f" sliced out {dt}")
                    rest = torch.cat([big[:, :4], big[:, 4 + Kd:]], 1)
                    assert bool((rest == SENTINEL).all()), tag + " wrote outside its output slice"
        st.done()


# ---- convolution ----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("plan", PLANS)
def test_conv_fwd_exact(dev, force_plan, plan):
    Cout = conv_cout(dims(plan)[1])
    with force_plan(plan) as st:
        for Cin in (8, 40):       # K = 72 / 360: taps straddle the 64-deep K steps
            for geom in (G_S1, G_S2, G_UP, G_1X1, G_OUTHW):
                k, stride, pad, up, out_hw = geom
                c = conv_case(Cin, Cout, geom)
                d = c.on(dev)
                tag = f"conv fwd {plan} Cin={Cin} {geom}"
                y = st.run(K.conv2d, d.x, d.w, stride=stride, pad=pad, upsample=up, out_hw=out_hw)
                same(y, c.fwd, tag)
                y = st.run(K.conv2d, d.x, d.w, bias=d.bias, stride=stride, pad=pad, upsample=up, out_hw=out_hw,
                           rowvec=d.rowvec, residual=d.res)
                same(y, c.fwd + c.bias.double() + c.rowvec.double()[:, None, None, :] + c.res.double(),
                     tag + " bias+rowvec+residual")
        st.done()


@gpu
@pytest.mark.parametrize("plan", PLANS)
def test_conv_dgrad_exact(dev, force_plan, plan):
    Cout = conv_cout(dims(plan)[1])
    n, H, W = IMG
    with force_plan(plan) as st:
        for Cin in (8, 40):
            for geom in (G_S1, G_S2, G_1X1):
                k, stride, pad, _, _ = geom
                c = conv_case(Cin, Cout, geom)
                d = c.on(dev)
                tag = f"conv dgrad {plan} Cin={Cin} {geom}"
                dx = st.run(K.conv2d_dgrad, d.dy, d.w, (H, W), stride, pad)
                if dx is not None:
                    same(dx, c.dgrad, tag)
                dx = st.run(K.conv2d_dgrad, d.dy, d.w, (H, W), stride, pad, out=d.c0.clone(), accumulate=True)
                if dx is not None:
                    same(dx, c.dgrad + c.c0.double(), tag + " accumulate")
        if plan == -1:   # the v1 kernel cannot read the stored conv weight in place: every launch refused
            assert st.launches == 0 and st.unsupported == [(-1, "conv_wt")] * st.issued
            same(st.run(K.conv2d, d.x, d.w, stride=stride, pad=pad), c.fwd, "conv fwd on the v1 kernel")
        st.done()


@gpu
@pytest.mark.parametrize("plan", PLANS)
def test_conv_wgrad_exact(dev, force_plan, plan):
    Cout = conv_cout(dims(plan)[1])
    with force_plan(plan) as st:
        for Cin in (8, 40):
            for geom in (G_S1, G_S2, G_UP):
                k, stride, pad, up, _ = geom
                c = conv_case(Cin, Cout, geom)
                d = c.on(dev)
                for sp in (1, 3, 5, 8):
                    tag = f"conv wgrad {plan} Cin={Cin} {geom} splits={sp}"
                    same(st.run(K.conv2d_wgrad, d.dy, d.x, k, stride, pad, upsample=up, splits=sp), c.wgrad, tag + " plain")
                    bg = torch.full((Cout,), float("nan"), device=dev)
                    dw = st.run(K.conv2d_wgrad, d.dy, d.x, k, stride, pad, upsample=up, splits=sp, bias_grad=bg)
                    same(dw, c.wgrad, tag)
                    same(bg, c.db, tag + " the bias gradient")
                    bg = d.db0.clone()
                    dw = st.run(K.conv2d_wgrad, d.dy, d.x, k, stride, pad, upsample=up, splits=sp, bias_grad=bg,
                                bias_acc=True, out=torch.empty(Cout, k, k, Cin, device=dev))
                    same(dw, c.wgrad, tag + " fp32")
                    same(bg, c.db + c.db0.double(), tag + " the accumulated bf16 bias gradient")
        st.done()


# ---- second K segment (LoRA product fused into its base GEMM) -------------------------------------
@gpu
@pytest.mark.parametrize("plan", PLANS)
def test_second_segment_exact(dev, force_plan, plan):
    """lora = (t, b2) on linear forward, linear dgrad and conv forward against the integer truth x w^T + t b2^T"""
    bm, bn = dims(plan)
    M, N = 2 * bm + 24, bn + 24
    n, H, W = IMG
    with force_plan(plan) as st:
        for K1 in (64, 320):          # the split point must be a multiple of 64 (kernels._seg2)
            c, cd = linear_case(M, N, K1), dgrad_case(M, K1, N)
            d, dd = c.on(dev), cd.on(dev)
            same(st.run(K.linear, d.x, d.w), c.P, f"linear {plan} K={K1}")
            for r in (8, 32):
                g = gen("seg2", M, N, K1, r)
                t, b2, a2 = ints((M, r), -3, 3, g), ints((N, r), -3, 3, g), ints((r, N), -3, 3, g)
                y = st.run(K.linear, d.x, d.w, bias=d.bias, lora=(t.to(dev), b2.to(dev)))
                if y is not None:
                    same(y, c.P + c.bias.double() + t.double() @ b2.double().t(), f"linear + lora {plan} K={K1} r={r}")
                dx = st.run(K.linear_dgrad, dd.dy, dd.w, lora=(t.to(dev), a2.to(dev)))
                if dx is not None:
                    same(dx, cd.P + t.double() @ a2.double(), f"linear dgrad + lora {plan} K={K1} r={r}")
        Cout = conv_cout(bn)
        c = conv_case(64, Cout, G_S1)   # K = 576: a multiple of 64
        d = c.on(dev)
        for r in (8, 32):
            g = gen("seg2 conv", Cout, r)
            t, b2 = ints((n, H, W, r), -3, 3, g), ints((Cout, r), -3, 3, g)
            y = st.run(K.conv2d, d.x, d.w, bias=d.bias, lora=(t.to(dev), b2.to(dev)))
            if y is not None:
                same(y, c.fwd + c.bias.double() + t.double() @ b2.double().t(), f"conv + lora {plan} r={r}")
        if isinstance(plan, int):
            assert bool(st.unsupported) == any(u == (plan, "seg2") for u in UNSUPPORTED_OK)
        st.done()


# ---- LoRA projection fused into the base GEMM's K loop (GemmArgs.D) --------------------------------
FUSED_TILES = (1, 4, 7, 8)   # the tiles with fused instances (gemm2_tiles_e.hip)


def fused(st, fn, *args, tile, **kw):
    """fn(..., tile=tile) must run as the one fused launch: a refusal falls back to two launches through _gemm"""
    before = st.launches
    out = fn(*args, tile=tile, **kw)
    assert st.launches == before, "the fused form fell back to two launches"
    return out


@gpu
@pytest.mark.parametrize("parts", (1, 3))
@pytest.mark.parametrize("tile", FUSED_TILES)
def test_linear_lora_fused_exact(dev, force_plan, tile, parts):
    """y and the stored t of linear_lora against the truth.  t is rounded to bf16 inside the kernel by design, so x and
    down come from {-1, 0, 1} and |t| <= 256, where bf16 holds every integer."""
    bm, bn = DIMS[tile]
    M, Kd, r, pw = 2 * bm + 24, 192, 32, bn
    N = parts * pw
    g = gen("lora fwd", tile, parts)
    x, down, w = ints((M, Kd), -1, 1, g), ints((parts * r, Kd), -1, 1, g), ints((N, Kd), -3, 3, g)
    up2, bias, res = block_diag(parts, pw, r, 1), ints((N,), -40, 40, g), ints((M, N), -40, 40, g)
    t_ref = x.double() @ down.double().t()
    assert t_ref.abs().max().item() <= 256
    y_ref = x.double() @ w.double().t() + t_ref @ up2.double().t() + bias.double() + res.double()
    xd, wd, dnd, upd, bd, rd = (v.to(dev) for v in (x, w, down, up2, bias, res))
    with force_plan("python") as st:
        t = torch.full((M, parts * r), float("nan"), dtype=BF, device=dev)
        y = fused(st, K.linear_lora, xd, wd, bd, rd, dnd, upd, t, r, pw, tile=tile)
        same(t, t_ref, f"linear_lora tile {tile} parts {parts}: t")
        same(y, y_ref, f"linear_lora tile {tile} parts {parts}: y")
        t.fill_(float("nan"))     # the planned form (fused or two launches, as the plan tables say)
        y = K.linear_lora(xd, wd, bd, rd, dnd, upd, t, r, pw)
        same(t, t_ref, "linear_lora planned (ctypes): t")
        same(y, y_ref, "linear_lora planned (ctypes): y")
    with force_plan("native") as st:
        t.fill_(float("nan"))
        y = st.run(K.linear_lora, xd, wd, bd, rd, dnd, upd, t, r, pw)
        same(t, t_ref, "linear_lora planned (native): t")
        same(y, y_ref, "linear_lora planned (native): y")
        st.done()


@gpu
@pytest.mark.parametrize("tile", FUSED_TILES)
def test_conv_lora_fused_exact(dev, force_plan, tile):
    bm, bn = DIMS[tile]
    n, H, W = IMG
    Cin, Cout, r = 64, bn, 32
    g = gen("lora conv", tile)
    x, down, w = ints((n, H, W, Cin), -1, 1, g), ints((r, 3, 3, Cin), -1, 1, g), ints((Cout, 3, 3, Cin), -3, 3, g)
    up2, bias, rowvec = ints((Cout, r), -3, 3, g), ints((Cout,), -40, 40, g), ints((n, Cout), -40, 40, g)
    res = ints((n, H, W, Cout), -40, 40, g)
    t_ref = nhwc(F.conv2d(nchw(x), nchw(down), padding=1))
    assert t_ref.abs().max().item() <= 256
    y_ref = nhwc(F.conv2d(nchw(x), nchw(w), bias.double(), padding=1)) + t_ref @ up2.double().t() \
        + rowvec.double()[:, None, None, :] + res.double()
    xd, wd, dnd, upd, bd, rvd, rd = (v.to(dev) for v in (x, w, down, up2, bias, rowvec, res))
    with force_plan("python") as st:
        t = torch.full((n, H, W, r), float("nan"), dtype=BF, device=dev)
        y = fused(st, K.conv2d_lora, xd, wd, bd, 1, 1, False, rd, rvd, dnd, upd, t, r, tile=tile)
        same(t, t_ref, f"conv2d_lora tile {tile}: t")
        same(y, y_ref, f"conv2d_lora tile {tile}: y")
    with force_plan("native") as st:
        t.fill_(float("nan"))
        y = st.run(K.conv2d_lora, xd, wd, bd, 1, 1, False, rd, rvd, dnd, upd, t, r)
        same(t, t_ref, "conv2d_lora planned (native): t")
        same(y, y_ref, "conv2d_lora planned (native): y")
        st.done()


@gpu
@pytest.mark.parametrize("parts", (1, 3))
@pytest.mark.parametrize("tile", FUSED_TILES)
def test_linear_dgrad_lora_fused_exact(dev, force_plan, tile, parts):
    """dx = dy w + u down with u = dy up2 stored: u is rounded to bf16 by design, dy and up2 come from {-1, 0, 1}"""
    bm, bn = DIMS[tile]
    M, N, Kd, r = 2 * bm + 24, 192, 2 * bn, 32
    pw = N // parts
    g = gen("lora dgrad", tile, parts)
    dy, w, down = ints((M, N), -1, 1, g), ints((N, Kd), -3, 3, g), ints((parts * r, Kd), -3, 3, g)
    up2 = block_diag(parts, pw, r, 2, -1, 1)
    upT = torch.cat([up2[p * pw:(p + 1) * pw, p * r:(p + 1) * r].t() for p in range(parts)], 1).contiguous()
    downT = down.t().contiguous()
    u_ref = dy.double() @ up2.double()
    assert u_ref.abs().max().item() <= 256
    dx_ref = dy.double() @ w.double() + u_ref @ down.double()
    dyd, wd, upd, dnd, upTd, dnTd = (v.to(dev) for v in (dy, w, up2, down, upT, downT))
    with force_plan("python") as st:
        u = torch.full((M, parts * r), float("nan"), dtype=BF, device=dev)
        dx = fused(st, K.linear_dgrad_lora, dyd, wd, upd, dnd, upTd, dnTd, u, tile=tile)
        same(u, u_ref, f"linear_dgrad_lora tile {tile} parts {parts}: u")
        same(dx, dx_ref, f"linear_dgrad_lora tile {tile} parts {parts}: dx")
    with force_plan("native") as st:
        u.fill_(float("nan"))
        dx = st.run(K.linear_dgrad_lora, dyd, wd, upd, dnd, upTd, dnTd, u)
        same(u, u_ref, "linear_dgrad_lora planned (native): u")
        same(dx, dx_ref, "linear_dgrad_lora planned (native): dx")
        st.done()


# ---- batched GEMM, as the materialised attention issues it -----------------------------------------
@gpu
@pytest.mark.parametrize("plan", (*TILES, "python"))
def test_batched_exact(dev, force_plan, plan):
    """kernels.gemm_batched with batch = B * H, bdiv = H and the real strides of [B, tokens, H * D] activations, in the
    operand-mode pairs of attn_mat_fwd / attn_mat_bwd -- (K, K) into fp32 scores, (K, MN) and (MN, MN) into bf16
    activations -- and (MN, K)"""
    bm, bn = dims(plan)
    B, H, D = 2, 3, 40
    Nq, Nk = bm + 24, bn + 24
    g = gen("batched", Nq, Nk)
    q, k = ints((B, Nq, H * D), -3, 3, g), ints((B, Nk, H * D), -3, 3, g)
    Pm, kt = ints((B * H, Nq, Nk), -3, 3, g), ints((B * H, D, Nq), -3, 3, g)
    q4, k4 = q.double().view(B, Nq, H, D), k.double().view(B, Nk, H, D)
    P4 = Pm.double().view(B, H, Nq, Nk)
    qd, kd, Pd, ktd = (v.to(dev) for v in (q, k, Pm, kt))
    zs = (H * Nq * Nk, Nq * Nk)
    with force_plan(plan) as st:
        # scores S = q k^T: (K, K), fp32 out
        S = torch.full((B * H, Nq, Nk), float("nan"), device=dev)
        st.run(K.gemm_batched, qd, H * D, K.OPM_K, kd, H * D, K.OPM_K, S, Nk, Nq, Nk, D, B * H, H, (Nq * H * D, D),
               (Nk * H * D, D), zs, alpha=0.5)
        same(S, 0.5 * torch.einsum("bqhd,bkhd->bhqk", q4, k4), f"batched (K, K) {plan}")
        # o = P v: (K, MN), bf16 out in the activation layout
        o = torch.full((B, Nq, H * D), float("nan"), dtype=BF, device=dev)
        st.run(K.gemm_batched, Pd, Nk, K.OPM_K, kd, H * D, K.OPM_MN, o, H * D, Nq, D, Nk, B * H, H, zs,
               (Nk * H * D, D), (Nq * H * D, D))
        same(o, torch.einsum("bhqk,bkhd->bqhd", P4, k4), f"batched (K, MN) {plan}")
        # dk = dS^T q: (MN, MN), accumulated onto a bf16 activation
        dk0 = ints((B, Nk, H * D), -100, 100, g)
        dk = dk0.to(dev)
        st.run(K.gemm_batched, Pd, Nk, K.OPM_MN, qd, H * D, K.OPM_MN, dk, H * D, Nk, D, Nq, B * H, H, zs,
               (Nq * H * D, D), (Nk * H * D, D), accumulate=True)
        same(dk, torch.einsum("bhqk,bqhd->bkhd", P4, q4) + dk0.double().view(B, Nk, H, D), f"batched (MN, MN) {plan}")
        # (MN, K): C_z = A_z^T B_z^T with A_z = P_z [Nq, Nk] (MN-mode) and B_z [D, Nq] (K-mode)
        c = torch.full((B, Nk, H * D), float("nan"), dtype=BF, device=dev)
        st.run(K.gemm_batched, Pd, Nk, K.OPM_MN, ktd, Nq, K.OPM_K, c, H * D, Nk, D, Nq, B * H, H, zs,
               (H * D * Nq, D * Nq), (Nk * H * D, D))
        same(c, torch.einsum("bhqk,bhdq->bkhd", P4, kt.double().view(B, H, D, Nq)), f"batched (MN, K) {plan}")
        assert not st.unsupported
        st.done()
