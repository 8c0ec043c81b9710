"""GEMM engine parity vs a plain PyTorch fp32 reference of the same op (GPU)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from onetrainer_amd import kernels as K

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def rnd(*s, dev, scale=1.0):
    return (torch.randn(*s, device=dev) * scale).to(BF)


def close(out, ref, tol=2e-2):
    out = out.float()
    err = (out - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-6
    assert err / scale < tol, f"max err {err} vs scale {scale}"


@pytest.mark.parametrize("M,N,Kd", [(128, 128, 64), (256, 384, 320), (77, 640, 2048), (4100, 1280, 640), (8, 1280, 320)])
def test_linear_fwd(dev, M, N, Kd):
    torch.manual_seed(0)
    x, w = rnd(M, Kd, dev=dev), rnd(N, Kd, dev=dev, scale=0.05)
    b, r = rnd(N, dev=dev), rnd(M, N, dev=dev)
    y = K.linear(x, w, bias=b, residual=r)
    ref = x.float() @ w.float().t() + b.float() + r.float()
    close(y, ref)


def test_linear_asymmetric_exact(dev):
    # integer-valued operands: exact in bf16/fp32, catches any transposed fragment map
    torch.manual_seed(1)
    M, N, Kd = 256, 256, 128
    x = torch.randint(-3, 4, (M, Kd), device=dev).to(BF)
    w = torch.randint(-3, 4, (N, Kd), device=dev).to(BF)
    y = K.linear(x, w, out_dtype=torch.float32)
    assert torch.equal(y, x.float() @ w.float().t())
    dy = torch.randint(-2, 3, (M, N), device=dev).to(BF)
    dx = K.linear_dgrad(dy, w, out=torch.empty(M, Kd, device=dev, dtype=torch.float32))
    assert torch.equal(dx, dy.float() @ w.float())
    dw = K.linear_wgrad(dy, x, out=torch.empty(N, Kd, device=dev, dtype=torch.float32))
    assert torch.equal(dw, dy.float().t() @ x.float())


@pytest.mark.parametrize("M,N,Kd", [(256, 640, 640), (4096, 640, 5120), (300, 2048, 640)])
def test_linear_dgrad(dev, M, N, Kd):
    torch.manual_seed(2)
    dy, w = rnd(M, N, dev=dev), rnd(N, Kd, dev=dev, scale=0.05)
    dx = K.linear_dgrad(dy, w)
    close(dx, dy.float() @ w.float())


@pytest.mark.parametrize("T,N,Kd", [(4096, 640, 640), (16384, 1280, 1280), (312, 640, 2048), (8, 1280, 2816)])
def test_linear_wgrad(dev, T, N, Kd):
    torch.manual_seed(3)
    dy, x = rnd(T, N, dev=dev), rnd(T, Kd, dev=dev)
    dw = K.linear_wgrad(dy, x, out=torch.empty(N, Kd, device=dev, dtype=torch.float32))
    close(dw, dy.float().t() @ x.float(), tol=1e-2)


def nchw(x):
    return x.permute(0, 3, 1, 2).float()


def to_nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("N,H,W,Cin,Cout,stride,up", [
    (2, 16, 16, 64, 128, 1, False), (2, 32, 24, 320, 320, 1, False), (1, 16, 16, 128, 64, 2, False),
    (2, 8, 8, 128, 128, 1, True), (1, 64, 64, 8, 320, 1, False), (1, 16, 16, 320, 8, 1, False),
    (2, 16, 8, 64, 72, 2, False)])
def test_conv_fwd_dgrad_wgrad(dev, N, H, W, Cin, Cout, stride, up):
    torch.manual_seed(4)
    x = rnd(N, H, W, Cin, dev=dev)
    w = rnd(Cout, 3, 3, Cin, dev=dev, scale=0.05)
    b = rnd(Cout, dev=dev)
    y = K.conv2d(x, w, bias=b, stride=stride, pad=1, upsample=up)
    xr = nchw(x).requires_grad_(True)
    xin = F.interpolate(xr, scale_factor=2.0, mode="nearest") if up else xr
    wr = w.permute(0, 3, 1, 2).float().requires_grad_(True)
    ref = F.conv2d(xin, wr, b.float(), stride=stride, padding=1)
    close(y, to_nhwc(ref))
    dy = rnd(*y.shape, dev=dev)
    ref.backward(nchw(dy))
    dw = K.conv2d_wgrad(dy, x, 3, stride, 1, upsample=up, out=torch.empty_like(w, dtype=torch.float32))
    close(dw, wr.grad.permute(0, 2, 3, 1), tol=1e-2)
    # dgrad reads the stored [Cout][3][3][Cin] weight in place (B operand OPM_CONV_WT)
    if up:
        dx = K.upsample2x_bwd(K.conv2d_dgrad(dy, w, (2 * H, 2 * W), 1, 1))
    else:
        dx = K.conv2d_dgrad(dy, w, (H, W), stride, 1)
    close(dx, to_nhwc(xr.grad))


@pytest.fixture
def autotune():
    K.set_gemm_autotune(True)
    K.gemm_autotune_cache().clear()
    yield
    K.set_gemm_autotune(False)
    K.gemm_autotune_cache().clear()


def test_autotuned_plans(dev, autotune):
    """autotuned (tile, split-K) plans: same products as the fp32 reference, accumulate and in-place
    residual epilogues untouched by the tuner's candidate runs, cached per signature."""
    torch.manual_seed(5)
    x, w = rnd(4096, 1280, dev=dev), rnd(1280, 1280, dev=dev, scale=0.05)
    r = rnd(4096, 1280, dev=dev)
    y = K.linear(x, w, residual=r)
    close(y, x.float() @ w.float().t() + r.float())
    acc = torch.ones(1280, 1280, device=dev, dtype=torch.float32)
    dy = rnd(4096, 1280, dev=dev)
    K.linear_wgrad(dy, x, out=acc, accumulate=True)
    close(acc, dy.float().t() @ x.float() + 1.0, tol=1e-2)
    dx = K.linear_dgrad(dy, w)
    close(dx, dy.float() @ w.float())
    xc = rnd(2, 32, 32, 320, dev=dev)
    wc = rnd(320, 3, 3, 320, dev=dev, scale=0.05)
    yc = K.conv2d(xc, wc, pad=1)
    ref = F.conv2d(nchw(xc), wc.permute(0, 3, 1, 2).float(), padding=1)
    close(yc, to_nhwc(ref))
    dxc = K.conv2d_dgrad(yc, wc, (32, 32), 1, 1)
    refd = torch.nn.grad.conv2d_input(nchw(xc).shape, wc.permute(0, 3, 1, 2).float(), nchw(yc), padding=1)
    close(dxc, to_nhwc(refd))
    n = len(K.gemm_autotune_cache())
    assert n >= 5
    for t, s in K.gemm_autotune_cache().values():
        assert -1 <= t <= 8 and s >= 1
    K.linear(x, w, residual=r)           # cached: no new entries
    assert len(K.gemm_autotune_cache()) == n




# ---- explicit plans: every catalogue tile really launched -----------------------------------------
TILES = (-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10)
EUNSUPPORTED = 3   # OTAMD_EUNSUPPORTED (csrc/common.h)


def operand_form(a) -> str:
    """the operand form of a GemmArgs, as far as the launchers tell forms apart when they pick an instance"""
    if a.D:
        return "lora_down"   # LoRA projection fused into the K loop (GemmArgs.D, gemm2_tiles_e.hip)
    if a.A2:
        return "seg2"        # second K segment (GemmArgs.A2)
    if a.bmode == K.OPM_CONV_WT:
        return "conv_wt"     # conv dgrad reading the stored weight in place
    return "plain"


# Every (tile, operand form) otamd_gemm_explicit may answer with OTAMD_EUNSUPPORTED, read off the launchers:
#   gemm.hip gemm_impl   `v2_only && tile < 0`: the v1 kernel (tile -1) has no conv-weight B, no second K segment and
#                        no fused LoRA projection;
#   gemm2_tiles_a.hip    `tile == 3 && !seg2`: the 4-wave 256x256 tile has no second-segment instance;
#   gemm2_kernel.h pick2 `NS != 2 -> nullptr` under seg2: the ring-4 tiles 9 / 10 have no second-segment instance;
#   gemm2_tiles_e.hip    gemm2_pick_ld has instances for tiles 1, 4, 7, 8 only.
# Not on the list, because the launcher does not refuse them: the fused column sums (GemmArgs.colsum) on tiles -1 and 3
# run on tile 0 (gemm_impl: `a.colsum && (tile < 0 || tile == 3)`), and every plain form has an instance on every tile.
UNSUPPORTED_OK = frozenset(
    {(-1, "conv_wt"), (-1, "seg2"), (3, "seg2"), (9, "seg2"), (10, "seg2")}
    | {(t, "lora_down") for t in TILES if t not in (1, 4, 7, 8)})


class Unsupported(Exception):
    """otamd_gemm_explicit answered OTAMD_EUNSUPPORTED for a (tile, operand form) on the allow-list"""


class ExplicitPlan:
    """stands in for kernels._gemm: launches otamd_gemm_explicit(tile, splits) and counts what it did.  The split
    count is the op's own (`splits=` of the weight gradients) when it passes one, else `self.splits`."""

    def __init__(self, tile, splits=1):
        self.tile, self.splits = tile, splits
        self.launches, self.unsupported = 0, []

    def __call__(self, a, op_splits, device):
        sp = 1 if a.batch > 1 else (op_splits or self.splits)   # batched GEMMs have no split-K
        ws_bytes = K._ws_bytes(a, sp)
        ws = K.workspace(ws_bytes, device) if ws_bytes else None
        rc = K.lib().otamd_gemm_explicit(C.byref(a), self.tile, sp, K._p(ws), ws_bytes, K.stream_handle())
        if rc == EUNSUPPORTED:
            key = (self.tile, operand_form(a))
            assert key in UNSUPPORTED_OK, f"OTAMD_EUNSUPPORTED for {key}: not on the allow-list"
            self.unsupported.append(key)
            raise Unsupported(key)
        K.check(rc, "otamd_gemm_explicit")
        self.launches += 1


def supported(fn, *args, **kw):
    """fn's result, or None when the explicit plan has no instance for it (allow-listed: ExplicitPlan checks)"""
    try:
        return fn(*args, **kw)
    except Unsupported:
        return None


@pytest.mark.parametrize("tile", TILES)
def test_every_tile_explicit(dev, tile, monkeypatch):
    """every engine tile (4 = 128x128 with 8 waves, 2 workgroups per CU; 5 / 6 = 128x64 / 64x128; 7 / 8 = 128x160 /
    256x160, 20 DMA pieces over 8 waves and 320-byte MN rows; 9 / 10 = 5 / 6 on a 4-deep LDS ring) through otamd_gemm_explicit: linear fwd (+bias +residual), dgrad, wgrad (split-K),
    conv fwd / dgrad / wgrad, ragged sizes, and K of 1 to 5 K-steps (ring prologue and tail wait counts).

    The body runs under python_host(): with the native host layer loaded the ops never reach kernels._gemm, and the
    patched plan would not be launched at all.  The launch count at the end says that every GEMM of the body went
    through this tile's explicit plan (or was refused with an allow-listed OTAMD_EUNSUPPORTED)."""
    torch.manual_seed(11)
    plan = ExplicitPlan(tile)
    monkeypatch.setattr(K, "_gemm", plan)
    issued = 0
    with K.python_host():
        x, w, b = rnd(1000, 640, dev=dev), rnd(328, 640, dev=dev, scale=0.05), rnd(328, dev=dev)
        r = rnd(1000, 328, dev=dev)
        close(K.linear(x, w, bias=b, residual=r), x.float() @ w.float().t() + b.float() + r.float())
        dy = rnd(1000, 328, dev=dev)
        close(K.linear_dgrad(dy, w), dy.float() @ w.float())
        issued += 2
        for sp in (1, 3):
            plan.splits = sp
            close(K.linear_wgrad(dy, x), dy.float().t() @ x.float(), tol=1e-2)
            # fused bias gradient (GemmArgs.colsum; the 4-wave / v1 tiles run it on tile 0)
            db = torch.full((328,), 0.5, dtype=BF, device=dev)
            close(K.linear_wgrad(dy, x, bias_grad=db, bias_acc=True), dy.float().t() @ x.float(), tol=1e-2)
            close(db, dy.float().sum(0) + 0.5, tol=1e-2)
            db32 = torch.empty(328, device=dev)
            K.linear_wgrad(dy, x, bias_grad=db32)
            close(db32, dy.float().sum(0), tol=2e-3)
            issued += 3
        plan.splits = 1
        for kd in (64, 72, 136, 200, 320):     # 1, 2, 3, 4, 5 K-steps
            xs, ws_ = rnd(300, kd, dev=dev), rnd(200, kd, dev=dev, scale=0.05)
            close(K.linear(xs, ws_), xs.float() @ ws_.float().t())
            dys = rnd(300, 200, dev=dev)
            close(K.linear_dgrad(dys, ws_[:, :kd]), dys.float() @ ws_.float())
            issued += 2
        xc = rnd(2, 24, 20, 64, dev=dev)
        wc = rnd(96, 3, 3, 64, dev=dev, scale=0.05)
        yc = K.conv2d(xc, wc, pad=1)
        close(yc, to_nhwc(F.conv2d(nchw(xc), wc.permute(0, 3, 1, 2).float(), padding=1)))
        dxc = supported(K.conv2d_dgrad, yc, wc, (24, 20), 1, 1)
        if dxc is not None:
            refd = torch.nn.grad.conv2d_input(nchw(xc).shape, wc.permute(0, 3, 1, 2).float(), nchw(yc), padding=1)
            close(dxc, to_nhwc(refd))
        # conv weight gradient with the fused bias gradient
        dbc = torch.empty(96, device=dev)
        dwc = K.conv2d_wgrad(yc, xc, 3, 1, 1, bias_grad=dbc)
        refw = torch.nn.grad.conv2d_weight(nchw(xc), (96, 64, 3, 3), nchw(yc), padding=1)
        close(dwc, refw.permute(0, 2, 3, 1), tol=2e-2)
        close(dbc, yc.float().sum((0, 1, 2)), tol=2e-3)
        issued += 3
    assert issued == 21
    assert plan.launches + len(plan.unsupported) == issued, (plan.launches, plan.unsupported)
    assert plan.unsupported == ([(-1, "conv_wt")] if tile == -1 else []), plan.unsupported
