"""Deferred grouped split-K reduces on the weight-gradient stream (otamd_gemm_defer_*, module/streams.defer_*).

The LoRA adapter gradients are split-K GEMMs (rank-wide outputs, K = tokens); deferring their reduces and launching
them grouped must not change a bit: each output is still summed in split order.  Checked on whole backward passes
(overwrite and gradient-accumulation micro-steps) of the tiny SDXL LoRA and the full-width SDXL LoRA r32 at 512^2,
b=1 (the C4 bench configuration), plus the flush-before-read guard on a direct GEMM chain.  The LayerNorm parameter reduces (otamd_layernorm_defer_*) are
deferred the same way on the main stream: checked on full fine-tune steps of the tiny SDXL UNet and at SDXL 512^2.
Both sit on one host queue (csrc/defer.h); its edges -- a full batch, an arena that wraps, an item too large to defer,
end on another stream -- are walked on direct kernel calls at the end of this file.
"""
import copy

import pytest
import torch

from onetrainer_amd import kernels as K
from onetrainer_amd.dataLoader.SyntheticDataLoader import synthetic_sdxl_batch
from onetrainer_amd.module import streams as S
from onetrainer_amd.module import unet as U
from onetrainer_amd.trainer.GenericTrainer import GenericTrainer
from onetrainer_amd.util import create
from onetrainer_amd.util.config.TrainConfig import TrainConfig

pytestmark = pytest.mark.gpu


def _lora_trainer(dev, ucfg, rank):
    cfg = TrainConfig.default_values()
    cfg.batch_size = 1
    cfg.learning_rate_warmup_steps = 0
    cfg.gradient_accumulation_steps = 1000   # no optimizer update: every micro-step sees the same weights
    cfg.training_method, cfg.lora_rank = "LORA", rank
    model = create.create_model(cfg, dev, seed=5, unet_config=ucfg)
    tr = GenericTrainer(cfg, model=model)
    tr.start()
    return tr


def _two_microsteps(tr, batch, defer, monkeypatch):
    """an overwrite micro-step and an accumulating one from the same progress state; the grads after each"""
    monkeypatch.setattr(S, "_DEFER", defer)
    model = tr.model
    tp0 = copy.deepcopy(model.train_progress)
    store = model.train_store
    store.accumulating = False
    out = []
    for _ in range(2):
        loss = tr.train_step(batch)
        torch.cuda.synchronize()
        out.append((loss.clone(), store.grad.clone()))
    model.train_progress = tp0
    store.accumulating = False
    return out


@pytest.mark.parametrize("which", ["tiny_r8", "sdxl_r32_512"])
def test_deferred_reduces_bit_identical(dev, which, monkeypatch):
    if which == "tiny_r8":
        tr = _lora_trainer(dev, U.tiny_sdxl_config(), 8)
        batch = synthetic_sdxl_batch(1, 256, 256, dev, seed=0, te1_dim=48, te2_dim=48, pooled_dim=64)
    else:
        tr = _lora_trainer(dev, None, 32)
        batch = synthetic_sdxl_batch(1, 512, 512, dev, seed=0)
    assert S.side_stream() is not None
    tr.train_step(batch)   # plan / workspace warm-up
    torch.cuda.synchronize()
    tr.model.train_store.accumulating = False
    ref = _two_microsteps(tr, batch, False, monkeypatch)
    g0, l0 = K.defer_reduces_stats()
    got = _two_microsteps(tr, batch, True, monkeypatch)
    g1, l1 = K.defer_reduces_stats()
    deferred, launches = g1 - g0, l1 - l0
    if which != "tiny_r8":   # the tiny UNet's few-token GEMMs mostly run unsplit
        assert deferred > 0 and launches > 0, (deferred, launches)
        assert launches * 4 <= deferred, (deferred, launches)   # grouped: many reduces per launch
    for (la, ga), (lb, gb) in zip(ref, got):
        assert torch.equal(la, lb)
        assert torch.equal(ga, gb), (ga.float() - gb.float()).abs().max().item()
    assert ref[0][1].abs().sum().item() > 0
    assert not torch.equal(ref[0][1], ref[1][1])   # the second micro-step accumulated
    assert K.defer_reduces_pending(S.side_stream()) == 0
    print(f"{which}: {deferred // 2} deferred reduces in {launches // 2} grouped launches per backward")


def test_defer_flushes_before_dependent_gemm(dev):
    """a GEMM that reads a pending output as its operand flushes the pending reduces first; a GEMM whose output
    lies outside the registered gradient range is not deferred"""
    side = S.side_stream()
    g = torch.Generator(device=dev).manual_seed(1)
    BF = torch.bfloat16
    x = torch.randn(8192, 256, device=dev, generator=g).to(BF)
    dy = torch.randn(8192, 32, device=dev, generator=g).to(BF)
    grads = torch.zeros(32 * 256 + 64 * 256, device=dev, dtype=BF)
    w1 = grads[:32 * 256].view(32, 256)
    y2 = torch.randn(64, 32, device=dev, generator=g).to(BF)
    ref1 = K.linear_wgrad(dy, x)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        K.defer_reduces_begin(side, grads)
        K.linear_wgrad(dy, x, out=w1)                     # split-K over 8192 tokens: deferred
        assert K.defer_reduces_pending(side) == 1
        z = K.linear_dgrad(y2, w1)                        # reads w1: must see the reduced value
        assert K.defer_reduces_pending(side) == 0
        outside = K.linear_wgrad(dy, x)                   # not in the gradient buffer: immediate reduce
        assert K.defer_reduces_pending(side) == 0
        K.defer_reduces_end(side)
    torch.cuda.synchronize()
    assert torch.equal(w1, ref1) and torch.equal(outside, ref1)
    assert torch.equal(z, K.linear_dgrad(y2, ref1))


def _ft_trainer(dev, ucfg):
    cfg = TrainConfig.default_values()
    cfg.batch_size = 1
    cfg.learning_rate_warmup_steps = 0
    cfg.gradient_accumulation_steps = 1000
    model = create.create_model(cfg, dev, seed=5, unet_config=ucfg)
    tr = GenericTrainer(cfg, model=model)
    tr.start()
    return tr


@pytest.mark.parametrize("which", ["tiny", "sdxl_512"])
def test_deferred_layernorm_param_reduces_bit_identical(dev, which, monkeypatch):
    if which == "tiny":
        tr = _ft_trainer(dev, U.tiny_sdxl_config())
        batch = synthetic_sdxl_batch(1, 256, 256, dev, seed=0, te1_dim=48, te2_dim=48, pooled_dim=64)
    else:
        tr = _ft_trainer(dev, None)
        batch = synthetic_sdxl_batch(1, 512, 512, dev, seed=0)
    tr.train_step(batch)
    torch.cuda.synchronize()
    tr.model.train_store.accumulating = False
    monkeypatch.setattr(S, "_LN_DEFER", False)
    ref = _two_microsteps(tr, batch, True, monkeypatch)
    monkeypatch.setattr(S, "_LN_DEFER", True)
    main = torch.cuda.current_stream()
    n0, l0, _ = K.ln_defer_stats(main)
    got = _two_microsteps(tr, batch, True, monkeypatch)
    n1, l1, pending = K.ln_defer_stats(main)
    assert pending == 0
    deferred, launches = n1 - n0, l1 - l0
    assert deferred > 0 and launches > 0 and launches * 2 <= deferred, (deferred, launches)
    for (la, ga), (lb, gb) in zip(ref, got):
        assert torch.equal(la, lb)
        assert torch.equal(ga, gb), (ga.float() - gb.float()).abs().max().item()
    assert not torch.equal(ref[0][1], ref[1][1])
    print(f"{which}: {deferred // 2} LayerNorm parameter reduces in {launches // 2} grouped launches per backward")


def test_layernorm_defer_flush_order(dev):
    """a pending reduce into the same dgamma is flushed before the next one is recorded (accumulation stays ordered);
    flush / end leave nothing pending and the sums equal the immediate path's"""
    g = torch.Generator(device=dev).manual_seed(3)
    BF = torch.bfloat16
    x = torch.randn(4096, 1280, device=dev, generator=g).to(BF)
    dy = torch.randn(4096, 1280, device=dev, generator=g).to(BF)
    gamma = torch.ones(1280, device=dev, dtype=BF)
    beta = torch.zeros(1280, device=dev, dtype=BF)
    _, stats = K.layernorm_fwd(x, gamma, beta, 1e-5)
    dg0, db0 = torch.zeros(1280, device=dev), torch.zeros(1280, device=dev)
    K.layernorm_param_grad(x, dy, stats, dg0, db0)
    K.layernorm_param_grad(x, dy, stats, dg0, db0, param_acc=True)
    main = torch.cuda.current_stream()
    dg, db = torch.zeros(1280, device=dev), torch.zeros(1280, device=dev)
    K.ln_defer_begin(main)
    K.layernorm_param_grad(x, dy, stats, dg, db)
    assert K.ln_defer_stats(main)[2] == 1
    K.layernorm_param_grad(x, dy, stats, dg, db, param_acc=True)   # same destination: the first is flushed
    assert K.ln_defer_stats(main)[2] == 1
    K.ln_defer_flush(main)
    assert K.ln_defer_stats(main)[2] == 0
    K.ln_defer_end(main)
    torch.cuda.synchronize()
    assert torch.equal(dg, dg0) and torch.equal(db, db0)


# ---- the queue's edges on direct kernel calls (csrc/defer.h under both users): batch rollover, arena wrap, end_on ----
BF, F32 = torch.bfloat16, torch.float32


def _fresh_stream(user, dev):
    """a stream that has no cached arena yet, so begin(nbytes=1 MiB) really allocates a 1 MiB arena (torch hands out
    its pool's streams again and again; K._ARENAS keeps an arena per raw stream and only ever grows it)"""
    for _ in range(64):
        s = torch.cuda.Stream(device=dev)
        if (user, s.cuda_stream) not in K._ARENAS:
            return s
    raise AssertionError("no stream without a cached arena")


def _ws_need(M, N, splits):
    """arena bytes of one deferred split-K GEMM: otamd_gemm_ws_bytes, in the arena's 256-byte units"""
    a = K._new_args()
    a.M, a.N = M, N
    return (K._ws_bytes(a, splits) + 255) // 256 * 256


def test_gemm_defer_batch_rollover(dev):
    """41 deferred GEMMs on the side stream: the 41st finds the batch of 40 full, so that batch goes out and one is
    left pending; fused column sums (fp32 / bf16, overwrite / accumulate) ride in the grouped reduce"""
    side = S.side_stream()
    assert side is not None
    g = torch.Generator(device=dev).manual_seed(11)
    dy = torch.randn(2048, 32, device=dev, generator=g).to(BF)
    x = torch.randn(2048, 64, device=dev, generator=g).to(BF)
    n, sl = 41, 32 * 64
    grads = torch.zeros(n * sl + 4 * 64, device=dev, dtype=BF)
    bias = {3: (0, True, False), 17: (1, True, True), 29: (2, False, False), 40: (3, False, True)}   # call: j, f32, acc

    def bias_slice(buf, j, f32):   # 32 column sums in 64 bf16 elements of the buffer's tail: fp32, or bf16 in half
        b = buf[n * sl + 64 * j:n * sl + 64 * (j + 1)]
        return b.view(F32) if f32 else b[:32]

    for j, f32, acc in bias.values():
        if acc:   # something to accumulate onto
            bias_slice(grads, j, f32).copy_(torch.randn(32, device=dev, generator=g))
    ref = grads.clone()

    def run(buf, each):
        for i in range(n):
            kw = {}
            if i in bias:
                j, f32, acc = bias[i]
                kw = dict(bias_grad=bias_slice(buf, j, f32), bias_acc=acc)
            K.linear_wgrad(dy, x, out=buf[i * sl:(i + 1) * sl].view(32, 64), splits=4, alpha=(i + 1) / 8, **kw)
            each(i)

    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        run(ref, lambda i: None)
        g0, l0 = K.defer_reduces_stats()
        K.defer_reduces_begin(side, grads)

        def each(i):
            assert K.defer_reduces_pending(side) == (i + 1 if i < 40 else 1), i
        run(grads, each)
        assert K.defer_reduces_stats() == (g0 + 40, l0 + 1)
        K.defer_reduces_end(side)
        assert K.defer_reduces_stats() == (g0 + 41, l0 + 2)
        assert K.defer_reduces_pending(side) == 0
    torch.cuda.synchronize()
    for i in range(n):
        assert torch.equal(grads[i * sl:(i + 1) * sl], ref[i * sl:(i + 1) * sl]), i
        assert grads[i * sl:(i + 1) * sl].float().abs().sum().item() > 0, i
    # each column-sum slice in its own dtype (the fp32 ones' halves, read as bf16, can spell a NaN) ...
    for j, f32, _ in bias.values():
        assert torch.equal(bias_slice(grads, j, f32), bias_slice(ref, j, f32)), j
        assert bias_slice(grads, j, f32).float().abs().sum().item() > 0, j
    # ... and nothing beside them was touched
    for j in (2, 3):
        assert not grads[n * sl + 64 * j + 32:n * sl + 64 * (j + 1)].any()


def test_gemm_defer_arena_wrap(dev):
    """a 1 MiB arena: the first GEMM whose slabs no longer fit sends the pending batch out; a GEMM that needs more
    than the whole arena is not deferred"""
    side = _fresh_stream("gemm", dev)
    M, N, T, splits = 64, 320, 2048, 4
    need = _ws_need(M, N, splits)
    fit = (1 << 20) // need
    assert 2 <= fit <= 4, (need, fit)
    big_m, big_n = 128, 1024
    assert _ws_need(big_m, big_n, splits) > 1 << 20
    g = torch.Generator(device=dev).manual_seed(12)
    dy = torch.randn(T, M, device=dev, generator=g).to(BF)
    x = torch.randn(T, N, device=dev, generator=g).to(BF)
    dy2 = torch.randn(T, big_m, device=dev, generator=g).to(BF)
    x2 = torch.randn(T, big_n, device=dev, generator=g).to(BF)
    n = fit + 2
    grads = torch.zeros(n * M * N + big_m * big_n, device=dev, dtype=BF)
    ref = grads.clone()

    def run(buf, each):
        for i in range(n):
            K.linear_wgrad(dy, x, out=buf[i * M * N:(i + 1) * M * N].view(M, N), splits=splits, alpha=(i + 1) / 4)
            each(i)
            if i == fit:   # right after the wrap, with one reduce pending
                K.linear_wgrad(dy2, x2, out=buf[n * M * N:].view(big_m, big_n), splits=splits)
                each(i)

    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        run(ref, lambda i: None)
        g0, l0 = K.defer_reduces_stats()
        K.defer_reduces_begin(side, grads, nbytes=1 << 20)
        assert K._ARENAS[("gemm", side.cuda_stream)].numel() == 1 << 20

        def each(i):   # 1 .. fit, then the wrap: 1, 2 (unchanged by the GEMM that is too large to defer)
            assert K.defer_reduces_pending(side) == (i + 1 if i < fit else i + 1 - fit), i
        run(grads, each)
        assert K.defer_reduces_stats() == (g0 + fit, l0 + 1)
        K.defer_reduces_end(side)
        assert K.defer_reduces_stats() == (g0 + n, l0 + 2)
        assert K.defer_reduces_pending(side) == 0
    torch.cuda.synchronize()
    assert torch.equal(grads, ref)
    assert grads[n * M * N:].float().abs().sum().item() > 0 and grads[:M * N].float().abs().sum().item() > 0


def _ln_inputs(dev, rows, C, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(rows, C, device=dev, generator=g).to(BF)
    dy = torch.randn(rows, C, device=dev, generator=g).to(BF)
    _, stats = K.layernorm_fwd(x, torch.ones(C, device=dev, dtype=BF), torch.zeros(C, device=dev, dtype=BF), 1e-5)
    return x, dy, stats


def test_layernorm_defer_batch_rollover(dev):
    """65 deferred parameter reduces into 65 (dgamma, dbeta) pairs: the 65th finds the batch of 64 full; fp32 and
    bf16 destinations, overwritten and accumulated"""
    n, C = 65, 64
    x, dy, stats = _ln_inputs(dev, 64, C, 13)
    g = torch.Generator(device=dev).manual_seed(14)
    init = [torch.randn(2, C, device=dev, generator=g).to(F32 if i % 2 else BF) for i in range(n)]
    ref = [t.clone() for t in init]
    got = [t.clone() for t in init]

    def run(dst, each):
        for i in range(n):   # i % 2: fp32 / bf16, i % 4 >= 2: accumulate
            K.layernorm_param_grad(x, dy, stats, dst[i][0], dst[i][1], param_acc=i % 4 >= 2)
            each(i)

    s = _fresh_stream("layernorm", dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        run(ref, lambda i: None)
        n0, l0, p0 = K.ln_defer_stats(s)
        assert p0 == 0
        K.ln_defer_begin(s, nbytes=1 << 20)

        def each(i):
            assert K.ln_defer_stats(s)[2] == (i + 1 if i < 64 else 1), i
        run(got, each)
        assert K.ln_defer_stats(s) == (n0 + 64, l0 + 1, 1)
        K.ln_defer_end(s)
        assert K.ln_defer_stats(s) == (n0 + 65, l0 + 2, 0)
    torch.cuda.synchronize()
    for i in range(n):
        assert torch.equal(got[i], ref[i]), i
        assert not torch.equal(got[i], init[i]), i


def test_layernorm_defer_arena_wrap(dev):
    """a 1 MiB arena: at 1024 x 1280 the parameter pass writes 32 slabs (32 * 2 * 1280 * 4 = 327,680 bytes), so three
    fit and the fourth wraps; at 4096 x 1280 its 128 slabs (1,310,720 bytes) exceed the arena: not deferred"""
    C = 1280
    x, dy, stats = _ln_inputs(dev, 1024, C, 15)
    xb, dyb, statsb = _ln_inputs(dev, 4096, C, 16)
    ref = [torch.zeros(2, C, device=dev) for _ in range(5)]
    got = [torch.zeros(2, C, device=dev) for _ in range(5)]

    def run(dst, each):
        for i in range(4):
            K.layernorm_param_grad(x, dy, stats, dst[i][0], dst[i][1])
            each(i)
        K.layernorm_param_grad(xb, dyb, statsb, dst[4][0], dst[4][1])
        each(4)

    s = _fresh_stream("layernorm", dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        run(ref, lambda i: None)
        n0, l0, _ = K.ln_defer_stats(s)
        K.ln_defer_begin(s, nbytes=1 << 20)
        assert K._ARENAS[("layernorm", s.cuda_stream)].numel() == 1 << 20

        def each(i):
            assert K.ln_defer_stats(s)[2] == (1, 2, 3, 1, 1)[i], i
        run(got, each)
        assert K.ln_defer_stats(s) == (n0 + 3, l0 + 1, 1)
        K.ln_defer_end(s)
        assert K.ln_defer_stats(s) == (n0 + 4, l0 + 2, 0)
    torch.cuda.synchronize()
    for i in range(5):
        assert torch.equal(got[i], ref[i]), i
        assert got[i].abs().sum().item() > 0


def test_layernorm_defer_end_on_other_stream(dev):
    """reduces recorded on the main stream go out on the side stream at end (as module/streams.defer_end does after
    side.wait_stream(main)); after the join the sums equal the immediate path's"""
    side = S.side_stream()
    assert side is not None
    main = torch.cuda.current_stream()
    C = 640
    x, dy, stats = _ln_inputs(dev, 512, C, 17)
    ref = [torch.zeros(2, C, device=dev) for _ in range(3)]
    got = [torch.zeros(2, C, device=dev) for _ in range(3)]
    for r in ref:
        K.layernorm_param_grad(x, dy, stats, r[0], r[1])
    n0, l0, p0 = K.ln_defer_stats(main)
    assert p0 == 0
    K.ln_defer_begin(main)
    for t in got:
        K.layernorm_param_grad(x, dy, stats, t[0], t[1])
    assert K.ln_defer_stats(main) == (n0, l0, 3)
    side.wait_stream(main)
    K.ln_defer_end(main, launch=side)
    assert K.ln_defer_stats(main) == (n0 + 3, l0 + 1, 0) and K.ln_defer_stats(side)[2] == 0
    main.wait_stream(side)   # the join
    torch.cuda.synchronize()
    for a, b in zip(got, ref):
        assert torch.equal(a, b) and a.abs().sum().item() > 0
