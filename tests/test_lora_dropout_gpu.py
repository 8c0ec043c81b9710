"""LoRA dropout on the GPU: the mask kernel (csrc/lora_dropout.hip) against the host oracle bit for bit, the autograd
wiring against the same K.* primitives with the oracle's mask applied in torch (exact: no tolerance), dropout 0 against
a wrapper that never set it, and training through the setups and GenericTrainer: repeatable, resumable, one mask per
step, the same under a replayed step graph, and free of stream races."""
import os

import numpy as np
import pytest
import torch

import _oracle_lora_dropout as O
from onetrainer_amd import _lib
from onetrainer_amd import kernels as K
from onetrainer_amd.dataLoader.SyntheticDataLoader import synthetic_flux_batch, synthetic_sdxl_batch
from onetrainer_amd.module import flux as FX
from onetrainer_amd.module import flux_ops as FO
from onetrainer_amd.module import functional as Fn
from onetrainer_amd.module import streams as S
from onetrainer_amd.module import unet as U
from onetrainer_amd.module.lora import LoRAWrapper
from onetrainer_amd.module.param_store import FlatParamStore
from onetrainer_amd.module.stream_hazards import StreamHazardCheck
from onetrainer_amd.trainer.GenericTrainer import GenericTrainer
from onetrainer_amd.util import create
from onetrainer_amd.util.config.TrainConfig import TrainConfig

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NANBITS = 0x7FC0
GUARD = 16                       # bf16 elements before and after the tensor: 32 bytes, so the slice stays 8-byte aligned
GRID_QUADS = 2048 * 256          # quads of one grid pass (LORA_DROP_MAX_BLOCKS x 256 threads)
EINVAL = 1


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _seed_tensor(seed, dev):
    seed &= 2 ** 64 - 1
    return torch.tensor([seed - 2 ** 64 if seed >= 2 ** 63 else seed], dtype=torch.int64, device=dev)


def _values(M, width, key):
    """bf16 inputs with both signs, zeros of both signs and a few large and tiny magnitudes"""
    g = torch.Generator().manual_seed(1000 + key)
    v = torch.randn(M, width, generator=g) * 3
    flat = v.view(-1)
    for i, x in enumerate((0.0, -0.0, 3.0e38, -3.0e38, 2.0 ** -100, 65280.0)):
        if i < flat.numel():
            flat[(i * 7) % flat.numel()] = x
    return v.to(BF)


def _run_guarded(v, seed, site, row0, p, dev, shift=0):
    """the kernel on v inside a NaN-filled buffer; (output bits, guards intact)"""
    M, width = v.shape
    n = M * width
    buf = torch.full((n + 2 * GUARD + shift,), float("nan"), dtype=BF, device=dev)
    lo = GUARD + shift
    t = buf[lo:lo + n].view(M, width)
    t.copy_(v)
    K.lora_dropout(t, _seed_tensor(seed, dev), site, row0, p)
    b = _bits(buf)
    ok = bool((b[:lo] == NANBITS).all() and (b[lo + n:] == NANBITS).all())
    return b[lo:lo + n].reshape(M, width), ok


def _expect(v, seed, site, row0, p):
    M, width = v.shape
    return _bits(O.apply(v, O.keep_mask(seed, site, row0, M, width, p), p))


@pytest.mark.parametrize("width", [1, 4, 6, 32, 96, 128])
def test_kernel_matches_oracle_bitwise(dev, width):
    """every output bf16 word and the guard elements, over M x row0 x site x seed x p at this width (1: rank 1, 6: a
    partial quad, 96: q|k|v at rank 32, 128: a 4-part FLUX group); the second row0 puts (row0 + m) * Wq across 2^32"""
    Wq = (width + 3) // 4
    n = 0
    for M in (1, 63, 257):
        v = _values(M, width, M * 131 + width)
        for row0 in (0, 2 ** 32 // Wq - M // 2):
            for site in (0, 793):
                for seed in (0, 2 ** 32 + 5, 2 ** 64 - 1):
                    for p in (0.0, 0.1, 0.5, 1.0):
                        got, ok = _run_guarded(v, seed, site, row0, p, dev)
                        what = f"M={M} width={width} row0={row0} site={site} seed={seed} p={p}"
                        assert ok, what + ": wrote outside the tensor"
                        want = _expect(v, seed, site, row0, p)
                        assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {got.size} words differ"
                        if p == 0.0:
                            assert np.array_equal(got, _bits(v)), what + ": p = 0 changed a value"
                        if p == 1.0:
                            assert not got.any(), what + ": p = 1 kept a value (or wrote -0)"
                        n += 1
    assert n == 3 * 2 * 2 * 3 * 4


@pytest.mark.parametrize("M,width", [(4099, 516), (4099, 514)])
def test_kernel_beyond_one_grid_pass(dev, M, width):
    """M * ceil(width / 4) above the threads of one grid pass: the stride loop, on the 8-byte path (516) and on the
    element path with a partial quad (514)"""
    assert M * ((width + 3) // 4) > GRID_QUADS
    v = _values(M, width, 5)
    got, ok = _run_guarded(v, 2 ** 32 + 5, 793, 77, 0.1, dev)
    assert ok
    assert np.array_equal(got, _expect(v, 2 ** 32 + 5, 793, 77, 0.1))


def test_kernel_element_path_on_a_2_byte_aligned_tensor(dev):
    """width % 4 == 0 but the tensor starts 2 bytes off an 8-byte boundary: the element path, same bits"""
    v = _values(63, 32, 9)
    got, ok = _run_guarded(v, 11, 2, 5, 0.5, dev, shift=1)
    assert ok
    assert np.array_equal(got, _expect(v, 11, 2, 5, 0.5))


def test_kernel_twice_gives_the_same_bits(dev):
    v = _values(257, 96, 3).to(dev)
    sd = _seed_tensor(99, dev)
    a = K.lora_dropout(v.clone(), sd, 4, 1000, 0.25)
    b = K.lora_dropout(v.clone(), sd, 4, 1000, 0.25)
    assert np.array_equal(_bits(a), _bits(b))
    assert not np.array_equal(_bits(a), _bits(K.lora_dropout(v.clone(), _seed_tensor(100, dev), 4, 1000, 0.25)))
    # a 4-D t (the conv form [N, P, Q, r]) is its [N P Q, r] rows
    c = K.lora_dropout(v.clone().view(1, 257, 3, 32), sd, 4, 0, 0.25)
    assert np.array_equal(_bits(c).reshape(-1, 32), _expect(v.cpu().view(-1, 32), 99, 4, 0, 0.25))


def test_kernel_argument_checks(dev):
    L = _lib.lib()
    t = torch.ones(8, 8, dtype=BF, device=dev)
    sd = torch.zeros(2, dtype=torch.int64, device=dev)
    st = K.stream_handle()

    def raw(tp, M, width, sp, site, row0, thr):
        return L.otamd_lora_dropout(tp, M, width, sp, site, row0, thr, 1.0, st)

    tp, sp = t.data_ptr(), sd.data_ptr()
    assert raw(None, 8, 8, sp, 0, 0, 0) == EINVAL
    assert raw(tp, 8, 8, None, 0, 0, 0) == EINVAL
    assert raw(tp, 8, 8, sp, 0, 0, 2 ** 32 + 1) == EINVAL
    assert raw(tp, 8, 8, sp, -1, 0, 0) == EINVAL
    assert raw(tp, 8, 8, sp, 2 ** 24, 0, 0) == EINVAL
    assert raw(tp, 8, 8, sp, 0, -1, 0) == EINVAL
    assert raw(tp, 8, 8, sp, 0, 2 ** 39 - 7, 0) == EINVAL        # (row0 + M) * Wq = 2^40 + 2
    assert raw(tp, 1, 4, sp, 0, 2 ** 40, 0) == EINVAL            # (2^40 + 1) * 1
    assert raw(tp, 8, 0, sp, 0, 0, 0) == EINVAL
    assert raw(tp + 1, 4, 8, sp, 0, 0, 0) == EINVAL              # not a bf16 address
    assert raw(tp, 8, 8, sp + 4, 0, 0, 0) == EINVAL              # not a 64-bit address
    torch.cuda.synchronize()
    assert bool((t == 1).all())                                  # none of them launched
    # the largest admissible counters run: thr = 2^32, site 2^24 - 1, (row0 + M) * Wq = 2^40
    assert raw(tp, 8, 8, sp, 2 ** 24 - 1, 2 ** 39 - 8, 2 ** 32) == 0
    torch.cuda.synchronize()
    assert not _bits(t).any()
    t.fill_(1)
    K.lora_dropout(t, sd[:1], 2 ** 24 - 1, 2 ** 39 - 8, 0.5)
    assert np.array_equal(_bits(t), _expect(torch.ones(8, 8, dtype=BF), 0, 2 ** 24 - 1, 2 ** 39 - 8, 0.5))
    # the front end refuses what the C entry cannot see
    with pytest.raises(ValueError):
        K.lora_dropout(torch.ones(8, 8, device=dev), sd[:1], 0, 0, 0.5)             # fp32
    with pytest.raises(ValueError):
        K.lora_dropout(torch.ones(8, 16, dtype=BF, device=dev)[:, :8], sd[:1], 0, 0, 0.5)   # not contiguous
    with pytest.raises(ValueError):
        K.lora_dropout(t, sd[:1].int(), 0, 0, 0.5)                                  # seed dtype
    with pytest.raises(ValueError):
        K.lora_dropout(t, sd[:1], 0, 0, 1.5)
    with pytest.raises(ValueError):
        K.lora_dropout(t, sd[:1], 2 ** 24, 0, 0.5)
    with pytest.raises(ValueError):
        K.lora_dropout(t, sd[:1], 0, 2 ** 40, 0.5)


# ------------------------------------------------------------------------------------------
# wiring: the autograd functions against the same kernels.py primitives with the oracle's mask applied in torch
SPECS = [("lin.weight", (320, 320), "linear", 320), ("lin32.weight", (320, 320), "linear", 320),
         ("conv.weight", (32, 16, 3, 3), "conv", 144), ("upc.weight", (32, 16, 3, 3), "conv", 144),
         ("blk.attn1.to_q.weight", (64, 64), "linear", 64), ("blk.attn1.to_k.weight", (64, 64), "linear", 64),
         ("blk.attn1.to_v.weight", (64, 64), "linear", 64),
         ("seg_a.weight", (128, 64), "linear", 64), ("seg_b.weight", (128, 64), "linear", 64)]
QKV = ["blk.attn1.to_q", "blk.attn1.to_k", "blk.attn1.to_v"]
P_DROP, SEED = 0.3, 2 ** 32 + 5


class Net:
    """the model surface LoRAWrapper reads (specs, store, device) over a frozen bf16 store of the shapes above"""

    def __init__(self, dev):
        self.device, self.specs = dev, SPECS
        self.store = FlatParamStore([(n, U._store_shape(n, sh, k, None), "net") for n, sh, k, _ in SPECS], BF, dev,
                                    trainable=False)
        g = torch.Generator(device=dev).manual_seed(5)
        with torch.no_grad():
            for n, _, _, fan in SPECS:
                p = self.store.params[n]
                p.copy_((torch.rand(p.shape, generator=g, device=dev) * 2 - 1) / fan ** 0.5)


def _wrapper(dev, rank, p=P_DROP):
    net = Net(dev)
    w = LoRAWrapper(net, rank=rank, alpha=float(rank), seed=0)
    g = torch.Generator(device=dev).manual_seed(7 + rank)
    with torch.no_grad():
        for n, prm in w.store.named_parameters():
            if n.endswith("lora_up.weight"):
                prm.copy_(torch.randn(prm.shape, generator=g, device=dev) * 0.05)
    w.refresh()
    w.set_dropout(p)
    w.set_dropout_seed(SEED)
    torch.cuda.synchronize()
    return net, w


def _mask(t, site, row0=0):
    """t (bf16, device) under the oracle's mask of `site` at SEED / P_DROP"""
    width = t.shape[-1]
    keep = O.keep_mask(SEED, site.site_id, row0, t.numel() // width, width, P_DROP)
    return O.apply(t, keep, P_DROP)


def _rand(dev, shape, key, scale=1.0):
    g = torch.Generator().manual_seed(key)
    return (torch.randn(shape, generator=g) * scale).to(BF).to(dev)


def _same(a, b, what):
    a, b = a.detach().contiguous(), b.detach().contiguous()
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(a.view(torch.int16 if a.dtype == BF else torch.int32),
                       b.view(torch.int16 if b.dtype == BF else torch.int32)), what + ": bits differ"


def _linear_reference(x2, dy2, wmat, site, need_dx, row0=0):
    """(y, dx, dA, [dB_p]) of one LoRA linear from the unfused kernels and the hand-masked t / u"""
    t = _mask(K.linear(x2, site.down), site, row0)
    y = K.linear(x2, wmat, lora=(t, site.up2))
    u = _mask(K.linear_dgrad(dy2, site.up2), site, row0)
    dA = K.linear_wgrad(u, x2, out=torch.empty_like(site.g_down))
    r = site.rank
    dB = [K.linear_wgrad(dy2[:, n0:n1], t[:, p * r:(p + 1) * r], out=torch.empty_like(g), alpha=site.scale)
          for p, (g, (n0, n1)) in enumerate(zip(site.g_up, site.ranges))]
    dx = K.linear_dgrad(dy2, wmat, lora=(u, site.down)) if need_dx else None
    return y, dx, dA, dB


def _check_site_grads(site, dA, dB, what):
    _same(site.g_down, dA, what + " dA")
    for p, (g, ref) in enumerate(zip(site.g_up, dB)):
        _same(g, ref, f"{what} dB[{p}]")
        assert g.abs().sum() > 0, what


@pytest.mark.parametrize("case,rank,need_dx", [("lin", 8, True), ("lin32", 32, True), ("qkv", 32, True),
                                                ("qkv", 8, True), ("lin", 8, False), ("qkv", 32, False)])
def test_linear_wiring_is_exact(dev, case, rank, need_dx):
    """a Linear (320 x 320 at rank 8, the smallest rank the GEMMs take, and at rank 32 where the fused forms would
    otherwise run) and a q|k|v group;
    need_dx = False goes through the weight-gradient stream with the mask launched inside the region"""
    net, w = _wrapper(dev, rank)
    if case == "qkv":
        site, wref = w.site_for(QKV), Fn.PRef(net.store, [m + ".weight" for m in QKV], (192, 64))
    else:
        site, wref = w.site_of[case], Fn.PRef(net.store, case + ".weight")
    M, Kd = 130, wref.w.shape[1]
    x = _rand(dev, (2, M // 2, Kd), 1).requires_grad_(need_dx)
    dy = _rand(dev, (2, M // 2, wref.w.shape[0]), 2, 0.1)
    assert (need_dx or S.side_stream() is not None) and site.drop() is w
    f0, d0 = K.lora_fused_counts(), K.lora_dgrad_fused_counts()
    w.store.begin_backward()
    y = Fn.linear(x, wref, lora=site)
    y.backward(dy)
    w.store.finish_backward()
    torch.cuda.synchronize()
    assert K.lora_fused_counts() == f0 and K.lora_dgrad_fused_counts() == d0, "a fused LoRA form ran under dropout"
    x2, dy2 = x.detach().view(M, Kd), dy.view(M, -1)
    y_ref, dx_ref, dA, dB = _linear_reference(x2, dy2, wref.w, site, need_dx)
    what = f"{case} r={rank} dx={need_dx}"
    _same(y.view(M, -1), y_ref, what + " y")
    if need_dx:
        _same(x.grad.view(M, Kd), dx_ref, what + " dx")
    _check_site_grads(site, dA, dB, what)
    # and the mask did something: the same call without dropout gives another y
    w.set_dropout(0.0)
    assert not torch.equal(Fn.linear(x.detach(), wref, lora=site), y.detach())


@pytest.mark.parametrize("name,stride,upsample", [("conv", 2, False), ("upc", 1, True), ("conv", 1, False)])
def test_conv_wiring_is_exact(dev, name, stride, upsample):
    net, w = _wrapper(dev, 8)
    site, wref = w.site_of[name], Fn.PRef(net.store, name + ".weight")
    N, H, W_ = 2, 10, 6
    x = _rand(dev, (N, H, W_, 16), 3).requires_grad_(True)
    P, Q = K.conv_out_hw(H, W_, 3, stride, 1, upsample)
    dy = _rand(dev, (N, P, Q, 32), 4, 0.1)
    f0 = K.lora_fused_counts()
    w.store.begin_backward()
    y = Fn.conv(x, wref, stride=stride, upsample=upsample, lora=site)
    y.backward(dy)
    w.store.finish_backward()
    torch.cuda.synchronize()
    assert K.lora_fused_counts() == f0
    xd, M, r = x.detach(), N * P * Q, site.rank
    t = _mask(K.conv2d(xd, site.down, stride=stride, pad=1, upsample=upsample), site)
    y_ref = K.conv2d(xd, wref.w, stride=stride, pad=1, upsample=upsample, lora=(t, site.up2))
    dy2 = dy.reshape(M, 32)
    u = _mask(K.linear_dgrad(dy2, site.up2), site).view(N, P, Q, r)
    dA = K.conv2d_wgrad(u, xd, 3, stride, 1, upsample=upsample, out=torch.empty_like(site.g_down))
    dB = K.linear_wgrad(dy2, t.reshape(M, r), out=torch.empty_like(site.g_up[0]), alpha=site.scale)
    if upsample:
        dup = K.conv2d_dgrad(dy, wref.w, (2 * H, 2 * W_), 1, 1)
        K.conv2d_dgrad(u, site.down, (2 * H, 2 * W_), 1, 1, out=dup, accumulate=True)
        dx_ref = K.upsample2x_bwd(dup)
    else:
        dx_ref = K.conv2d_dgrad(dy, wref.w, (H, W_), stride, 1)
        K.conv2d_dgrad(u, site.down, (H, W_), stride, 1, out=dx_ref, accumulate=True)
    what = f"{name} stride={stride} up={upsample}"
    _same(y, y_ref, what + " y")
    _same(x.grad, dx_ref, what + " dx")
    _check_site_grads(site, dA, [dB], what)


@pytest.mark.parametrize("need_dx", [True, False])
def test_flux_rows_linear_wiring_is_exact(dev, need_dx):
    """the segmented linear of the FLUX double blocks: two row segments with their own weights and sites, each
    segment's t indexed from row 0"""
    net, w = _wrapper(dev, 8)
    sa, sb = w.site_of["seg_a"], w.site_of["seg_b"]
    wa, wb = Fn.PRef(net.store, "seg_a.weight"), Fn.PRef(net.store, "seg_b.weight")
    R, r0 = 72, 24
    x = _rand(dev, (R, 64), 5).requires_grad_(need_dx)
    dy = _rand(dev, (R, 128), 6, 0.1)
    segs = [(0, r0, wa, None, sa), (r0, R, wb, None, sb)]
    w.store.begin_backward()
    y = FO.rows_linear(x, segs)
    y.backward(dy)
    w.store.finish_backward()
    torch.cuda.synchronize()
    xd = x.detach()
    for (a, b, wref, _, site) in segs:
        y_ref, dx_ref, dA, dB = _linear_reference(xd[a:b], dy[a:b], wref.w, site, need_dx)
        _same(y[a:b], y_ref, f"rows [{a}, {b}) y")
        if need_dx:
            _same(x.grad[a:b], dx_ref, f"rows [{a}, {b}) dx")
        _check_site_grads(site, dA, dB, f"rows [{a}, {b})")


def test_dp_rank_draws_its_rows_of_the_global_mask(dev):
    """rank 1 of 2 with M local rows masks t as rows [M, 2 M) of the global tensor"""
    net, w = _wrapper(dev, 8)
    site = w.site_of["lin"]
    t = _rand(dev, (48, 8), 8)
    w.dp_rank = 1
    got = w.dropout(t.clone(), site)
    _same(got, _mask(t, site, row0=48), "rank 1")
    full = O.apply(torch.cat([t, t]), O.keep_mask(SEED, site.site_id, 0, 96, 8, P_DROP), P_DROP)
    _same(got, full[48:], "global rows")


# ------------------------------------------------------------------------------------------
def _tiny_unet_pass(dev, set_zero):
    m = U.UNet2DConditionModel(U.tiny_sdxl_config(), dev, seed=1, trainable=False)
    lw = LoRAWrapper(m, rank=32, alpha=16.0, seed=0)
    if set_zero:
        lw.set_dropout(0.0)
    g = torch.Generator().manual_seed(3)
    sd = {k: (torch.randn(v.shape, generator=g) * 0.1 if not k.endswith(".alpha") else v)
          for k, v in lw.state_dict().items()}
    lw.load_state_dict(sd)
    m.lora = lw
    cfg = m.cfg
    B, H, W_ = 2, 16, 16
    xin = torch.zeros(B, H, W_, 8, dtype=BF, device=dev)
    xin[..., :4] = _rand(dev, (B, H, W_, 4), 11)
    t = torch.tensor([10, 700], dtype=torch.int32, device=dev)
    ehs = _rand(dev, (B, 77, cfg.cross_attention_dim), 12)
    te = _rand(dev, (B, cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim), 13)
    tid = torch.tensor([[128., 128., 0., 0., 128., 128.]] * B, device=dev)
    c0 = K.lora_fused_counts() + K.lora_dgrad_fused_counts()
    out = m(xin, t, ehs, te, tid)
    lw.store.begin_backward()
    (out[..., :4].float() * _rand(dev, (B, H, W_, 4), 14).float()).sum().backward()
    lw.store.finish_backward()
    torch.cuda.synchronize()
    c1 = K.lora_fused_counts() + K.lora_dgrad_fused_counts()
    return out.detach().clone(), lw.store.grad.clone(), tuple(b - a for a, b in zip(c0, c1))


def test_dropout_zero_is_untouched(dev):
    """set_dropout(0.0) against a wrapper that never set it: the same bits, and the fused / two-launch counters of
    the forward and of the input gradient advance by the same amounts"""
    y0, g0, c0 = _tiny_unet_pass(dev, False)
    y1, g1, c1 = _tiny_unet_pass(dev, True)
    _same(y0, y1, "forward")
    _same(g0, g1, "adapter gradients")
    assert c0 == c1 and sum(c0) > 0, (c0, c1)


# ------------------------------------------------------------------------------------------
def _cfg(tmp, **kw):
    cfg = TrainConfig.default_values()
    cfg.batch_size = 2
    cfg.learning_rate = 1e-3
    cfg.learning_rate_warmup_steps = 0
    cfg.workspace_dir = str(tmp)
    cfg.training_method = "LORA"
    cfg.lora_rank, cfg.lora_alpha = 8, 8.0
    cfg.dropout_probability = 0.25
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _trainer(cfg, dev):
    if cfg.model_type == "FLUX_DEV_1":
        model = create.create_model(cfg, dev, seed=3, flux_config=FX.tiny_flux_config())
    else:
        model = create.create_model(cfg, dev, seed=3, unet_config=U.tiny_sdxl_config())
    tr = GenericTrainer(cfg, model=model)
    tr.start()
    return tr


def _sdxl_batch(dev, b=2):
    return synthetic_sdxl_batch(b, 128, 128, dev, seed=1, te1_dim=48, te2_dim=48, pooled_dim=64)


def _step_mask(w, dev):
    """the mask the wrapper's current seed gives site 0 on a tensor of ones"""
    return _bits(w.dropout(torch.ones(64, 32, dtype=BF, device=dev), w.sites[0]))


def test_sdxl_training_repeats_and_resumes(dev, tmp_path):
    batch = _sdxl_batch(dev)

    def run(tmp, steps, backup_after=None):
        tr = _trainer(_cfg(tmp), dev)
        w = tr.model.unet_lora
        assert type(w) is LoRAWrapper and w.dropout_p == 0.25 and tr.model.unet.lora is w
        before = w.store.data.clone()
        losses, masks, path = [], [], None
        for i in range(steps):
            gs = tr.model.train_progress.global_step
            losses.append(tr.train_step(batch).item())
            assert int(w.drop_seed.item()) == gs          # the step's masks were keyed by its global_step
            masks.append(_step_mask(w, dev))
            if backup_after == i + 1:
                path = tr.backup()
        torch.cuda.synchronize()
        assert not torch.equal(before, w.store.data)
        return losses, masks, w.store.data.clone(), path

    la, ma, wa, path = run(tmp_path / "a", 4, backup_after=2)
    assert all(np.isfinite(la)), la
    for m0, m1 in zip(ma, ma[1:]):
        assert not np.array_equal(m0, m1)                 # consecutive steps draw other masks
    assert 0 < (ma[0] == 0).mean() < 1
    lb, _, wb, _ = run(tmp_path / "b", 4)
    assert la == lb and torch.equal(wa, wb)
    # against the same run without dropout: the mask reaches the loss
    tr0 = _trainer(_cfg(tmp_path / "c", dropout_probability=0.0), dev)
    l0 = [tr0.train_step(batch).item() for _ in range(2)]
    assert l0[1] != la[1]                                 # (step 0 has up = 0: the adapters do not reach the output yet)
    # resumed from the backup taken after step 2: steps 3 and 4 continue bit for bit
    assert path and os.path.isdir(path)
    rs = _trainer(_cfg(tmp_path / "a", continue_last_backup=True), dev)
    assert rs.model.train_progress.global_step == 2 and rs.model.unet_lora.dropout_p == 0.25
    lr_ = [rs.train_step(batch).item() for _ in range(2)]
    torch.cuda.synchronize()
    assert lr_ == la[2:], (lr_, la)
    assert torch.equal(rs.model.unet_lora.store.data, wa)


def test_flux_training_repeats(dev, tmp_path):
    fcfg = FX.tiny_flux_config()
    batch = synthetic_flux_batch(2, 128, 128, dev, seed=1, t5_dim=fcfg.joint_attention_dim,
                                 pooled_dim=fcfg.pooled_projection_dim, text_len=9)

    def run(tmp, p):
        tr = _trainer(_cfg(tmp, model_type="FLUX_DEV_1", timestep_distribution="LOGIT_NORMAL", dropout_probability=p),
                      dev)
        w = tr.model.transformer_lora
        assert type(tr.model_setup).__name__ == "FluxLoRASetup" and w.dropout_p == p
        before = w.store.data.clone()
        losses, masks = [], []
        for _ in range(3):
            losses.append(tr.train_step(batch).item())
            masks.append(_step_mask(w, dev))
        torch.cuda.synchronize()
        assert not torch.equal(before, w.store.data)
        return losses, masks, w.store.data.clone()

    la, ma, wa = run(tmp_path / "a", 0.25)
    assert all(np.isfinite(la)), la
    assert not np.array_equal(ma[0], ma[1]) and not np.array_equal(ma[1], ma[2])
    lb, _, wb = run(tmp_path / "b", 0.25)
    assert la == lb and torch.equal(wa, wb)
    l0, _, _ = run(tmp_path / "c", 0.0)
    assert l0[1] != la[1]


def test_step_graph_matches_eager_with_dropout(dev, tmp_path, monkeypatch):
    """the replayed step draws the eager run's masks: losses step by step and the adapters, bit-identical.  The seed
    lives in device memory and is written before every replay, so equal losses also show that successive replays
    draw new masks (the eager run's differ from step to step: test_sdxl_training_repeats_and_resumes)."""
    def run(graphs: bool):
        monkeypatch.setenv("OTAMD_STEP_GRAPH", "1" if graphs else "0")   # opt-in
        tr = _trainer(_cfg(tmp_path / ("g" if graphs else "e")), dev)
        assert (tr.graphs is not None) == graphs
        assert tr.model_setup.graphable(tr.config)
        a = _sdxl_batch(dev)
        losses = [tr.train_step(a).clone() for _ in range(5)]
        torch.cuda.synchronize()
        return torch.stack(losses).cpu(), tr.model.unet_lora.store.data.clone(), tr

    l0, p0, _ = run(False)
    l1, p1, tr1 = run(True)
    assert len(tr1.graphs.entries) == 1
    assert torch.equal(l0, l1), (l0, l1)
    assert torch.equal(p0, p1)
    assert len(set(l0.tolist())) == 5


def test_dropout_step_has_no_stream_races(dev, tmp_path):
    tr = _trainer(_cfg(tmp_path, batch_size=1), dev)
    batch = _sdxl_batch(dev, 1)
    tr.train_step(batch)
    torch.cuda.synchronize()
    with StreamHazardCheck() as chk:
        tr.train_step(batch)
    torch.cuda.synchronize()
    assert chk.regions > 10 and chk.kernel_calls > 100 and chk.checked > 100, chk.report()
    assert not chk.hazards, chk.report()
