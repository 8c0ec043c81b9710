"""Fused 8-bit AdamW (csrc/adamw8bit.hip, util/optimizer/adamw8bit_fused.py) on the GPU against the restatement
tests/_oracle_adamw8bit.py.  The oracle declares no unpinned operation, so codes, absmax, fp32 moments and fp32
parameters must be bit-identical.  bitsandbytes, which the reference imports, is not in the reference tree: nothing
here is compared with it."""
import numpy as np
import pytest
import torch

import _oracle_adafactor as AF
import _oracle_adamw8bit as A8
from onetrainer_amd import _lib
from onetrainer_amd import kernels as K
from onetrainer_amd.module.param_store import FlatParamStore
from onetrainer_amd.util.optimizer.adamw8bit_fused import FusedAdamW8bit
from oracle import adamw as OA

pytestmark = pytest.mark.gpu

NAMES = [n for n, _ in A8.SHAPES]
FORMS = ["f32", "master", "bf16", "bf16_sr"]
LCG = (6364136223846793005, 1442695040888963407)
GROUP_OF = [0 if i < A8.SPLIT else 1 for i in range(len(NAMES))]
F = np.float32


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().astype(np.uint16)


def make(dev, form, seed=11, **kw):
    dtype = torch.float32 if form == "f32" else torch.bfloat16
    st = FlatParamStore([(n, s, "a" if i < A8.SPLIT else "b") for i, (n, s) in enumerate(A8.SHAPES)], dtype, dev,
                        master=form == "master")
    for n, s in A8.SHAPES:
        st.write(n, torch.from_numpy(AF.param0(n, s)))
    groups = [dict(params=[st.params[n] for n in part], **cfg)
              for part, cfg in zip((NAMES[:A8.SPLIT], NAMES[A8.SPLIT:]), A8.GROUP_CFG)]
    return st, FusedAdamW8bit(st, groups, stochastic_rounding=form == "bf16_sr", seed=seed, **kw)


def set_grads(st, k, mult=1.0):
    for n, s in A8.SHAPES:
        st.params[n].grad.copy_(torch.from_numpy(A8.case_grad(n, s, k) * F(mult)))


def set_lr(opt, k):
    for g, cfg in zip(opt.param_groups, A8.GROUP_CFG):
        g["lr"] = cfg["lr"] * A8.LR_FACTORS[k]


def value(st, n):
    return st.value(n).detach().float().cpu().numpy().reshape(-1)


def source(st):
    return st.master if st.master is not None else st.data


def state_np(opt, n):
    return {k: v.detach().cpu().numpy().reshape(-1) for k, v in opt._views(n).items()}


def all_state(opt):
    return [opt.code1, opt.code2, opt.absmax1, opt.absmax2, opt.m32, opt.v32]


def padding_mask(st, dev):
    mask = torch.ones(st.numel, dtype=torch.bool, device=dev)
    for n in NAMES:
        mask[st.slots[n].offset:st.slots[n].offset + st.slots[n].numel] = False
    return mask


def test_the_store_has_the_edges_the_cases_need(dev):
    st, opt = make(dev, "f32")
    (b0, e0), (b1, e1) = opt._ranges
    assert e0 % 8 != 0 and b1 == (e0 + 7) // 8 * 8          # the groups' boundary lies inside an 8-element vector
    assert [st.slots[n].numel for n in NAMES] == [1, 7, 8, 9, 4095, 4096, 4097, 4099, 70001]
    # 4095 takes the fp32 path, 4096 and 4097 the 8-bit one with 16 and 17 blocks
    assert [opt._seg_of[n][0] for n in NAMES] == [False] * 5 + [True] * 4
    assert [opt._seg_of[n][2] for n in NAMES[4:]] == [16, 16, 17, 17, 274]
    assert {t.group for t in opt._table_host} == {0, 1} and opt._table_host[6].group == 0 and opt._table_host[7].group == 1


@pytest.mark.parametrize("form", FORMS)
def test_five_steps_against_the_oracle(dev, form):
    is_bf16 = form.startswith("bf16")
    st, opt = make(dev, form)
    ost = [A8.new_state(A8.numel(s), A8.numel(s) >= 4096) for _, s in A8.SHAPES]
    pad = padding_mask(st, dev)
    last_m = [None] * len(NAMES)
    for k in range(A8.STEPS):
        set_grads(st, k)
        set_lr(opt, k)
        before = [value(st, n) for n in NAMES]
        seed = (opt.seed * LCG[0] + LCG[1]) & 0xFFFFFFFFFFFFFFFF
        opt.step()
        assert opt.seed == (seed if is_bf16 else 11) and opt.steps == [k + 1, k + 1]
        for i, (n, s) in enumerate(A8.SHAPES):
            cfg = dict(A8.GROUP_CFG[GROUP_OF[i]], lr=opt.param_groups[GROUP_OF[i]]["lr"])
            g = st.params[n].grad.float().cpu().numpy().reshape(-1)
            x, last_m[i], _ = A8.step(before[i], g, ost[i], A8.group_scalars(cfg, k + 1))
            got = state_np(opt, n)
            if "code1" in ost[i]:
                for key in ("code1", "code2", "absmax1", "absmax2"):
                    mine = got[key.replace("code", "state")]
                    bad = int(np.count_nonzero(mine != ost[i][key]))
                    print(f"{form} step {k} {n} {key}: {bad} of {mine.size} differ from the oracle")
                    assert bad == 0, (n, k, key)
            else:
                assert np.array_equal(got["state1"], ost[i]["m"]) and np.array_equal(got["state2"], ost[i]["v"]), (n, k)
            now = value(st, n)
            if form in ("f32", "master"):
                assert np.array_equal(now, x), (n, k)
                if form == "master":   # the working copy is rne(master), bit for bit
                    assert np.array_equal(bits(st.params[n]).reshape(-1), OA.f32_to_bf16_bits(now)), (n, k)
            elif form == "bf16":
                assert np.array_equal(bits(st.params[n]).reshape(-1), OA.f32_to_bf16_bits(x)), (n, k)
            else:
                gb = bits(st.params[n]).reshape(-1)
                u = x.view(np.uint32)
                lo = (u >> 16).astype(np.uint16)
                hi = np.where(u & 0xFFFF, lo + np.uint16(1), lo).astype(np.uint16)
                assert np.all((gb == lo) | (gb == hi)), (n, k)   # one of the two bf16 neighbours of the fp32 value
                slot = st.slots[n]
                want = OA.copy_stochastic(x, OA.sr_bits(seed, np.arange(slot.offset, slot.offset + slot.numel)))
                assert np.array_equal(gb, np.asarray(want).reshape(-1)), (n, k)
            # the step moved it (a single bf16 element may round back to itself: the large tensors stand for the store)
            assert not np.array_equal(now, before[i]) or (is_bf16 and x.size < 4096), (n, k)
        # the padding belongs to no block: it keeps the codes of 0 and its zeros
        assert pad.any() and bool((opt.code1[pad] == A8.ZERO1).all()) and not opt.code2[pad].any()
        assert not source(st)[pad].any() and not st.data[pad].any()
    # the all-zero block has absmax exactly 0 and the codes of 0; its neighbours do not
    zs = state_np(opt, A8.ZERO_BLOCK[0])
    b = A8.ZERO_BLOCK[1]
    assert zs["absmax1"][b] == 0 and zs["absmax2"][b] == 0 and zs["absmax1"][b - 1] > 0 and zs["absmax1"][b + 1] > 0
    assert np.all(zs["state1"][b * 256:(b + 1) * 256] == A8.ZERO1) and not zs["state2"][b * 256:(b + 1) * 256].any()
    # the last blocks of 4097 and 4099 hold one and three real elements: their maxima are those elements' alone
    for n, real in (("s4097", 1), ("s4099", 3)):
        m = last_m[NAMES.index(n)]   # the unquantised first moment of the last step
        assert m.size == 4096 + real and state_np(opt, n)["absmax1"][16] == np.abs(m[4096:]).max() > 0
    hs = state_np(opt, A8.HUGE[0])["state2"][A8.HUGE[1] * 256:(A8.HUGE[1] + 1) * 256]
    assert hs[A8.HUGE[2]] == 255 and np.all(np.delete(hs, A8.HUGE[2]) < 64)


def test_padding_never_enters_an_absmax(dev):
    """garbage gradients and parameters in the store's padding change no state and no block maximum"""
    (a, oa), (b, ob) = make(dev, "f32"), make(dev, "f32")
    pad = padding_mask(b, dev)
    for k in range(2):
        set_grads(a, k)
        set_grads(b, k)
        b.grad[pad] = 1.0e6
        oa.step()
        ob.step()
    assert all(torch.equal(x, y) for x, y in zip(all_state(oa), all_state(ob)))
    assert torch.equal(a.data[~pad], b.data[~pad]) and not b.data[pad].any()


@pytest.mark.parametrize("form", ["f32", "bf16"])
def test_pending_clip_equals_prescaled_gradients(dev, form):
    (a, oa), (b, ob) = make(dev, form), make(dev, form)
    for k in range(2):
        set_grads(a, k, 300.0)
        oa.clip_grad_norm_(1.0)
        coef = F(oa.clip_out[0].item())
        assert 0 < coef < 1 and oa._pending_clip
        for n in NAMES:
            g = a.params[n].grad.float().cpu().numpy() * coef            # one fp32 rounding, as the kernel's
            b.params[n].grad.copy_(torch.from_numpy(OA.rbf(g) if form == "bf16" else g))
        oa.step()
        ob.step()
        assert not oa._pending_clip
    assert torch.equal(a.data.view(torch.uint8), b.data.view(torch.uint8))
    assert all(torch.equal(x, y) for x, y in zip(all_state(oa), all_state(ob)))


def _run(dev, form, steps, seed=11, first=0, st_opt=None):
    st, opt = st_opt or make(dev, form, seed=seed)
    for k in range(first, first + steps):
        set_grads(st, k, 300.0)
        set_lr(opt, k)
        opt.clip_grad_norm_(1.0)
        opt.step()
    torch.cuda.synchronize()
    return st, opt


@pytest.mark.parametrize("form", ["master", "bf16_sr"])
def test_save_and_resume_is_bit_identical(dev, form):
    a, oa = _run(dev, form, 4)
    b, ob = _run(dev, form, 2)
    sd = ob.state_dict()
    assert set(sd["state"][NAMES.index("s4096")]) == {"step", "state1", "state2", "absmax1", "absmax2", "qmap1", "qmap2"}
    assert sd["state"][NAMES.index("s4096")]["state1"].shape == (64, 64)
    c, oc = make(dev, form, seed=999)
    for n in NAMES:
        c.write(n, b.value(n))
    oc.load_state_dict(sd)
    assert oc.seed == ob.seed and oc.steps == [2, 2]
    assert all(torch.equal(x, y) for x, y in zip(all_state(ob), all_state(oc)))
    _run(dev, form, 2, first=2, st_opt=(c, oc))
    assert torch.equal(source(a).view(torch.uint8), source(c).view(torch.uint8))
    assert torch.equal(a.data.view(torch.uint8), c.data.view(torch.uint8))
    assert all(torch.equal(x, y) for x, y in zip(all_state(oa), all_state(oc)))


def test_two_runs_give_identical_bits(dev):
    (a, oa), (b, ob), (c, oc) = _run(dev, "bf16_sr", 3), _run(dev, "bf16_sr", 3), _run(dev, "bf16_sr", 3, seed=12)
    assert torch.equal(a.data.view(torch.int16), b.data.view(torch.int16)) and oa.seed == ob.seed
    assert all(torch.equal(x, y) for x, y in zip(all_state(oa), all_state(ob)))
    assert not torch.equal(a.data.view(torch.int16), c.data.view(torch.int16))   # and another seed rounds otherwise


def test_a_broken_table_is_refused_before_any_launch(dev):
    st, opt = make(dev, "f32")
    set_grads(st, 0)
    start = [t.clone() for t in [st.data] + all_state(opt)]
    good = opt._table_host
    t = (_lib.A8Seg * opt._n_segs).from_buffer_copy(bytes(good))
    t[6].blk0 += 1                                           # the blocks are no longer consecutive
    assert K.adamw8bit_check(t, opt._n_segs, st.numel, opt.absmax1.numel(), opt.m32.numel(), 2) == _lib.OTAMD_EINVAL
    opt._table_host = t
    with pytest.raises(RuntimeError, match="invalid arguments"):
        opt.step()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(start, [st.data] + all_state(opt)))   # nothing ran
    opt._table_host = good
    opt.step()
    assert not torch.equal(start[0], st.data)


def test_step_does_not_synchronise_the_host(dev):
    """step() behind a long kernel returns while that kernel's event is incomplete, and raises nothing under torch's
    synchronisation debug mode"""
    st, opt = make(dev, "bf16_sr")
    for k in range(2):   # warm-up: code objects loaded
        set_grads(st, k)
        opt.clip_grad_norm_(1.0)
        opt.step()
    torch.cuda.synchronize()
    set_grads(st, 2)
    x = torch.randn(8192, 8192, device=dev)
    torch.cuda.synchronize()
    ev = torch.cuda.Event()
    for _ in range(40):   # 40 fp32 GEMMs of 1.1 TFLOP: some hundred milliseconds of device work
        x = torch.mm(x, x) * 1e-4
    ev.record()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.clip_grad_norm_(1.0)
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert not ev.query()   # the host is back before the device reached the step
    torch.cuda.synchronize()
    assert opt.steps == [3, 3]


def test_one_training_step_of_the_tiny_sdxl_unet(dev, tmp_path):
    from onetrainer_amd.dataLoader.SyntheticDataLoader import synthetic_sdxl_batch
    from onetrainer_amd.module import unet as U
    from onetrainer_amd.trainer.GenericTrainer import GenericTrainer
    from onetrainer_amd.util import create
    from onetrainer_amd.util.config.TrainConfig import TrainConfig
    cfg = TrainConfig.default_values()
    cfg.batch_size = 2
    cfg.learning_rate = 1e-4
    cfg.learning_rate_warmup_steps = 0
    cfg.workspace_dir = str(tmp_path)
    cfg.optimizer.optimizer = "ADAMW_8BIT"   # every other field None: the reference's fall-backs
    model = create.create_model(cfg, dev, seed=7, unet_config=U.tiny_sdxl_config())
    tr = GenericTrainer(cfg, model=model)
    tr.start()
    opt, st = model.optimizer, model.train_store
    assert isinstance(opt, FusedAdamW8bit) and opt.min_8bit_size == 4096
    kinds = {is8 for is8, _, _ in opt._seg_of.values()}
    assert kinds == {True, False}                            # the tiny UNet has tensors on both paths
    before = source(st).clone()
    tr.train_step(synthetic_sdxl_batch(2, 128, 128, dev, seed=3, te1_dim=48, te2_dim=48, pooled_dim=64))
    torch.cuda.synchronize()
    assert opt.steps[0] == 1 and not torch.equal(before, source(st)) and bool(torch.isfinite(source(st).float()).all())
    assert bool((opt.absmax2 > 0).any()) and bool((opt.code2 != 0).any())
