"""The group look-up the flat-store kernels share (csrc/flat_store.h: fs_find_group, fs_valid) at its limit: eight
parameter groups, the maximum, over a store whose tensors end inside a vector, one of them a single element.  Every
tensor is its own group with its own lr and weight_decay, so an element stepped with a neighbour's group shows at
once.  Each optimizer is compared with its own oracle, with the equality its own test uses: bits for the bf16 and
master AdamW, schedule-free AdamW and 8-bit AdamW, atol 1e-8 for the fp32 AdamW (test_optimizer_gpu.py)."""
import numpy as np
import pytest
import torch

import _oracle_adafactor as AF
import _oracle_adamw8bit as A8
import _oracle_schedule_free as SF
from onetrainer_amd import _lib
from onetrainer_amd import kernels as K
from onetrainer_amd.module.param_store import FlatParamStore
from onetrainer_amd.util.optimizer.adamw8bit_fused import FusedAdamW8bit
from onetrainer_amd.util.optimizer.adamw_fused import FusedAdamW
from onetrainer_amd.util.optimizer.schedule_free_fused import FusedScheduleFreeAdamW
from oracle import adamw as OA

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [3, 8, 9, 17, 1, 64, 7, 250]
NAMES = [f"t{i}" for i in range(len(SIZES))]
CFG = [dict(lr=1e-3 * (1 + i / 4), weight_decay=(0.0 if i == 2 else 0.01 * (i + 1))) for i in range(len(SIZES))]
LCG = (6364136223846793005, 1442695040888963407)
FORMS = ["bf16", "bf16_sr", "f32", "master"]
STEPS = 2   # the second one with a pending clip


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().astype(np.uint16).reshape(-1)


def make_store(dev, form):
    dtype = torch.float32 if form == "f32" else torch.bfloat16
    st = FlatParamStore([(n, (s,), f"g{i}") for i, (n, s) in enumerate(zip(NAMES, SIZES))], dtype, dev,
                        master=form == "master")
    for n, s in zip(NAMES, SIZES):
        st.write(n, torch.from_numpy(AF.param0(n, (s,))))
    return st


def param_groups(st, **extra):
    return [dict(params=[st.params[n]], **cfg, **extra) for n, cfg in zip(NAMES, CFG)]


def set_grads(st, k):
    """bf16-exact gradients; step 1's are large enough for the clip to bite"""
    for n, s in zip(NAMES, SIZES):
        g = AF.hashed((s,), 7000 + 13 * k + sum(map(ord, n)), 1e-2) * F(300.0 if k == 1 else 1.0)
        st.params[n].grad.copy_(torch.from_numpy(g))


def grad_np(st, n, coef, bf16_round):
    g = st.params[n].grad.float().cpu().numpy().reshape(-1)
    if coef is None:
        return g
    return OA.rbf(g * coef) if bf16_round else g * coef


def value(st, n):
    return st.value(n).detach().float().cpu().numpy().reshape(-1)


def source(st):
    return st.master if st.master is not None else st.data


def padding(st, dev):
    mask = torch.ones(st.numel, dtype=torch.bool, device=dev)
    for n in NAMES:
        mask[st.slots[n].offset:st.slots[n].offset + st.slots[n].numel] = False
    assert int(mask.sum()) == sum(-s % 8 for s in SIZES) > 0
    return mask


def pad_bytes(bufs, mask):
    return [b[mask].clone().view(torch.uint8) for b in bufs]


def clip(opt):
    """clip_grad_norm_(1.0): the device coefficient as an fp32 scalar"""
    opt.clip_grad_norm_(1.0)
    coef = F(opt.clip_out[0].item())
    assert 0 < coef < 1 and opt._pending_clip
    return coef


def idx(st, n):
    return np.arange(st.slots[n].offset, st.slots[n].offset + st.slots[n].numel)


def test_the_store_has_the_edges_the_case_needs(dev):
    st = make_store(dev, "f32")
    opt = FusedAdamW(st, param_groups(st))
    assert len(opt._ranges) == 8 and [e - b for b, e in opt._ranges] == SIZES
    assert all(b % 8 == 0 for b, _ in opt._ranges) and sum(e % 8 != 0 for _, e in opt._ranges) == 6
    assert st.numel == sum((s + 7) // 8 * 8 for s in SIZES)


@pytest.mark.parametrize("form", FORMS)
def test_adamw_steps_every_tensor_with_its_own_group(dev, form):
    st = make_store(dev, form)
    opt = FusedAdamW(st, param_groups(st), stochastic_rounding=form == "bf16_sr", seed=77)
    is_bf16 = form.startswith("bf16")
    zeros = (lambda s: np.zeros(s, np.uint16)) if is_bf16 else (lambda s: np.zeros(s, F))
    ref = {n: ((bits(st.params[n]) if is_bf16 else value(st, n)), zeros(s), zeros(s)) for n, s in zip(NAMES, SIZES)}
    pad = padding(st, dev)
    bufs = [source(st), st.data, opt.exp_avg, opt.exp_avg_sq]
    pad0 = pad_bytes(bufs, pad)
    for k in range(STEPS):
        set_grads(st, k)
        coef = None
        if k == 1:
            coef = clip(opt)
            if is_bf16:   # the bf16 coefficient is the oracle's, bit for bit (test_optimizer_gpu.py)
                assert coef == OA.clip_grad_norm_bf16([bits(st.params[n].grad) for n in NAMES], 1.0)[2]
        seed = (opt.seed * LCG[0] + LCG[1]) & 0xFFFFFFFFFFFFFFFF
        opt.step()
        assert opt.seed == (seed if is_bf16 else 77) and not opt._pending_clip and opt.steps == [k + 1] * 8
        for n, cfg in zip(NAMES, CFG):
            p, m, v = ref[n]
            sl = slice(st.slots[n].offset, st.slots[n].offset + st.slots[n].numel)
            kw = dict(lr=cfg["lr"], weight_decay=cfg["weight_decay"], clip_coef=coef)
            if is_bf16:
                rand = OA.sr_bits(seed, idx(st, n)) if form == "bf16_sr" else None
                p, m, v = OA.adamw_step_bf16(p, bits(st.params[n].grad), m, v, k + 1, rand16=rand, **kw)
                assert np.array_equal(bits(st.params[n]), p), (n, k, "p")
                assert np.array_equal(bits(opt.exp_avg[sl]), m) and np.array_equal(bits(opt.exp_avg_sq[sl]), v), (n, k)
            elif form == "master":
                p, m, v, w = OA.adamw_step_master(p, bits(st.params[n].grad), m, v, k + 1, **kw)
                assert np.array_equal(value(st, n), p), (n, k, "p")
                assert np.array_equal(bits(st.params[n]), w), (n, k, "working copy")
                assert np.array_equal(opt.exp_avg[sl].cpu().numpy(), m), (n, k, "m")
                assert np.array_equal(opt.exp_avg_sq[sl].cpu().numpy(), v), (n, k, "v")
            else:
                p, m, v = OA.adamw_step_f32(p, grad_np(st, n, None, False), m, v, k + 1, **kw)
                np.testing.assert_allclose(value(st, n), p, rtol=0, atol=1e-8, err_msg=f"{n} step {k}")
                np.testing.assert_allclose(opt.exp_avg[sl].cpu().numpy(), m, rtol=0, atol=1e-8, err_msg=f"{n} step {k}")
            ref[n] = (p, m, v)
    assert all(torch.equal(a, b) for a, b in zip(pad0, pad_bytes(bufs, pad)))


def sf_check(st, form, n, x, seed=None):
    """tensor n against the oracle's fp32 value x before the output rounding, bit for bit"""
    if form in ("f32", "master"):
        assert np.array_equal(value(st, n), x), n
        if form == "master":
            assert np.array_equal(bits(st.params[n]), OA.f32_to_bf16_bits(x)), n
    elif seed is not None:
        assert np.array_equal(bits(st.params[n]), np.asarray(OA.copy_stochastic(x, OA.sr_bits(seed, idx(st, n)))).reshape(-1)), n
    else:
        assert np.array_equal(bits(st.params[n]), OA.f32_to_bf16_bits(x)), n


@pytest.mark.parametrize("form", FORMS)
def test_schedule_free_step_and_mode_switches(dev, form):
    st = make_store(dev, form)
    opt = FusedScheduleFreeAdamW(st, param_groups(st), stochastic_rounding=form == "bf16_sr", seed=77)
    opt.train()
    is_bf16 = form.startswith("bf16")
    ogroups = [SF.new_group(**cfg) for cfg in CFG]
    oz = [None] * len(NAMES)
    ov = [np.zeros(s, F) for s in SIZES]
    pad = padding(st, dev)
    bufs = [source(st), st.data, opt.z, opt.exp_avg_sq]
    pad0 = pad_bytes(bufs, pad)
    for k in range(STEPS):
        set_grads(st, k)
        coef = clip(opt) if k == 1 else None
        before = [value(st, n) for n in NAMES]
        seed = (opt.seed * LCG[0] + LCG[1]) & 0xFFFFFFFFFFFFFFFF
        opt.step()
        assert opt.seed == (seed if is_bf16 else 77) and not opt._pending_clip
        for i, n in enumerate(NAMES):
            sc = SF.group_scalars(ogroups[i])
            x, oz[i], ov[i], _ = SF.sf_step(before[i], grad_np(st, n, coef, is_bf16), oz[i], ov[i], sc,
                                            clipped=coef is not None)
            views = {key: v.cpu().numpy().reshape(-1) for key, v in opt._views(n).items()}
            assert np.array_equal(views["z"], oz[i]) and np.array_equal(views["exp_avg_sq"], ov[i]), (n, k)
            sf_check(st, form, n, x, seed if form == "bf16_sr" else None)
    y_bits, w_bits = source(st).clone(), st.data.clone()
    y = [value(st, n) for n in NAMES]
    opt.eval()
    for i, n in enumerate(NAMES):
        x, _ = SF.sf_swap(y[i], opt._views(n)["z"].cpu().numpy().reshape(-1), SF.eval_weight(0.9))
        sf_check(st, form, n, x)                                # the swap always rounds to nearest
    assert not torch.equal(source(st), y_bits)
    opt.train()
    assert torch.equal(source(st).view(torch.uint8), y_bits.view(torch.uint8))
    assert torch.equal(st.data.view(torch.uint8), w_bits.view(torch.uint8))
    assert all(torch.equal(a, b) for a, b in zip(pad0, pad_bytes(bufs, pad)))


@pytest.mark.parametrize("form", ["f32", "bf16"])
def test_adamw8bit_steps_every_tensor_with_its_own_group(dev, form):
    st = make_store(dev, form)
    opt = FusedAdamW8bit(st, param_groups(st), min_8bit_size=16, stochastic_rounding=False, seed=77)
    assert [opt._seg_of[n][0] for n in NAMES] == [s >= 16 for s in SIZES]
    assert [t.group for t in opt._table_host] == list(range(8))
    ost = [A8.new_state(s, s >= 16) for s in SIZES]
    pad = padding(st, dev)
    bufs = [source(st), st.data, opt.code1, opt.code2]
    pad0 = pad_bytes(bufs, pad)
    assert bool((opt.code1[pad] == A8.ZERO1).all())
    for k in range(STEPS):
        set_grads(st, k)
        coef = clip(opt) if k == 1 else None
        before = [value(st, n) for n in NAMES]
        opt.step()
        assert opt.steps == [k + 1] * 8 and not opt._pending_clip
        for i, n in enumerate(NAMES):
            cfg = dict(CFG[i], betas=(0.9, 0.999), eps=1e-8)
            x, _, _ = A8.step(before[i], grad_np(st, n, coef, form == "bf16"), ost[i], A8.group_scalars(cfg, k + 1))
            got = {key: v.detach().cpu().numpy().reshape(-1) for key, v in opt._views(n).items()}
            if "code1" in ost[i]:
                for key in ("code1", "code2", "absmax1", "absmax2"):
                    assert np.array_equal(got[key.replace("code", "state")], ost[i][key]), (n, k, key)
            else:
                assert np.array_equal(got["state1"], ost[i]["m"]) and np.array_equal(got["state2"], ost[i]["v"]), (n, k)
            if form == "f32":
                assert np.array_equal(value(st, n), x), (n, k)
            else:
                assert np.array_equal(bits(st.params[n]), OA.f32_to_bf16_bits(x)), (n, k)
    assert all(torch.equal(a, b) for a, b in zip(pad0, pad_bytes(bufs, pad)))


def test_a_ninth_group_is_refused_before_any_launch(dev):
    """nine group structs over the same store: refused by the Python checks or by the library's (invalid arguments),
    and no buffer changes"""
    st = make_store(dev, "bf16")
    set_grads(st, 0)
    edges = [(st.slots[n].offset, st.slots[n].offset + st.slots[n].numel) for n in NAMES]
    edges = edges[:-1] + [(edges[-1][0], edges[-1][0] + 128), (edges[-1][0] + 128, edges[-1][1])]   # t7 in two groups
    assert len(edges) == 9
    m, v = torch.zeros_like(st.data), torch.zeros_like(st.data)
    z, v32 = torch.zeros(st.numel, device=dev), torch.zeros(st.numel, device=dev)
    start = [t.clone() for t in (st.data, m, v, z, v32)]
    adamw = [_lib.AdamwGroup(begin=b, end=e, wd_factor=0.5, one_minus_beta1=0.1, beta2=0.999, one_minus_beta2=1e-3,
                             bc2_sqrt=0.03, eps=1e-8, neg_step_size=-1e-2) for b, e in edges]
    sf = [_lib.SfGroup(begin=b, end=e, lr=1e-2, a_y=-1e-2, ckp1=1.0, beta2=0.999, one_minus_beta2=1e-3, inv_bc2=1e3,
                       eps=1e-8, weight_decay=0.0, first=1) for b, e in edges]
    swap = [_lib.SfSwapGroup(begin=b, end=e, w=0.5) for b, e in edges]
    refused = (ValueError, RuntimeError)
    with pytest.raises(refused):
        K.adamw_bf16(st.data, st.grad, m, v, adamw, stochastic_rounding=False)
    with pytest.raises(refused):
        K.sf_adamw_step(st.data, st.grad, None, z, v32, sf)
    with pytest.raises(refused):
        K.sf_swap(st.data, None, z, swap)
    opt = FusedAdamW8bit(st, param_groups(st), min_8bit_size=16)
    nine = [_lib.A8Group() for _ in range(9)]
    with pytest.raises(refused):
        K.adamw8bit_step(st.data, st.grad, None, opt.code1, opt.code2, opt.absmax1, opt.absmax2, opt.m32, opt.v32,
                         opt._qmap, opt._table, opt._table_host, opt._n_segs, nine)
    assert K.adamw8bit_check(opt._table_host, opt._n_segs, st.numel, opt.absmax1.numel(), opt.m32.numel(), 9) == _lib.OTAMD_EINVAL
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(start, (st.data, m, v, z, v32)))
    # eight of them are taken
    K.adamw_bf16(st.data, st.grad, m, v, adamw[:7] + [_lib.AdamwGroup(begin=edges[7][0], end=edges[8][1], wd_factor=0.5,
                 one_minus_beta1=0.1, beta2=0.999, one_minus_beta2=1e-3, bc2_sqrt=0.03, eps=1e-8, neg_step_size=-1e-2)],
                 stochastic_rounding=False)
    torch.cuda.synchronize()
    assert not torch.equal(start[0], st.data)
