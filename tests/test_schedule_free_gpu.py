"""Fused schedule-free AdamW (csrc/schedule_free.hip, util/optimizer/schedule_free_fused.py) on the GPU against the
restatement tests/_oracle_schedule_free.py, within the bounds derived there and returned beside its result.  The
schedulefree package, which the reference imports, is not in the reference tree: nothing here is compared with it."""
import os

import numpy as np
import pytest
import torch

import _oracle_adafactor as AF
import _oracle_schedule_free as SF
from onetrainer_amd import kernels as K
from onetrainer_amd.module.param_store import FlatParamStore
from onetrainer_amd.util.optimizer.schedule_free_fused import FusedScheduleFreeAdamW
from oracle import adamw as OA

pytestmark = pytest.mark.gpu

NAMES = [n for n, _ in SF.SHAPES]
FORMS = ["f32", "master", "bf16", "bf16_sr"]
LCG = (6364136223846793005, 1442695040888963407)
GROUP_OF = [0 if i < SF.SPLIT else 1 for i in range(len(NAMES))]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().astype(np.uint16)


def make(dev, form, seed=11, train=True, **kw):
    dtype = torch.float32 if form == "f32" else torch.bfloat16
    st = FlatParamStore([(n, s, "a" if i < SF.SPLIT else "b") for i, (n, s) in enumerate(SF.SHAPES)], dtype, dev,
                        master=form == "master")
    for n, s in SF.SHAPES:
        st.write(n, torch.from_numpy(AF.param0(n, s)))
    groups = [dict(params=[st.params[n] for n in part], **cfg)
              for part, cfg in zip((NAMES[:SF.SPLIT], NAMES[SF.SPLIT:]), SF.GROUP_CFG)]
    opt = FusedScheduleFreeAdamW(st, groups, stochastic_rounding=form == "bf16_sr", seed=seed, **kw)
    if train:
        opt.train()
    return st, opt


def test_the_store_has_the_edges_the_cases_need(dev):
    st, opt = make(dev, "f32")
    (b0, e0), (b1, e1) = opt._ranges
    assert e0 % 8 != 0 and b1 == (e0 + 7) // 8 * 8          # the groups' boundary lies inside an 8-element vector
    assert st.slots["s70001"].numel > 65536 and opt._n_chunks == len(NAMES) + 1   # crosses the norm chunk
    assert [st.slots[n].numel for n in NAMES] == [1, 7, 8, 9, 4099, 70001]


def set_grads(st, k, mult=1.0):
    for n, s in SF.SHAPES:
        st.params[n].grad.copy_(torch.from_numpy(SF.case_grad(n, s, k) * np.float32(mult)))


def set_lr(opt, ogroups, k):
    for g, og, cfg in zip(opt.param_groups, ogroups, SF.GROUP_CFG):
        g["lr"] = og["lr"] = cfg["lr"] * SF.LR_FACTORS[k]


def value(st, n):
    return st.value(n).detach().float().cpu().numpy()


def source(st):
    return st.master if st.master is not None else st.data


def oracle_groups(**kw):
    return [SF.new_group(**dict(cfg, **kw)) for cfg in SF.GROUP_CFG]


def sr_neighbours(x):
    """the bf16 bit patterns below and above (toward larger magnitude) the fp32 values x"""
    u = np.asarray(x, np.float32).view(np.uint32)
    lo = (u >> 16).astype(np.uint16)
    hi = np.where(u & 0xFFFF, lo + np.uint16(1), lo).astype(np.uint16)
    return lo, hi


def check_params(st, opt, form, n, x, tol, seed=None):
    """the store's tensor n against the oracle's fp32 value x (before the output rounding) and its bound"""
    got = value(st, n)
    if form in ("f32", "master"):
        assert np.all(np.abs(got.astype(np.float64) - x) <= tol), n
        if form == "master":   # the working copy is rne(master), bit for bit
            assert np.array_equal(bits(st.params[n]), OA.f32_to_bf16_bits(got)), n
        return bool(np.array_equal(got, x))
    gb = bits(st.params[n]).reshape(-1)
    if form == "bf16_sr":
        lo, hi = sr_neighbours(x.reshape(-1))
        assert np.all((gb == lo) | (gb == hi)), n            # one of the two bf16 neighbours of the fp32 value
        slot = st.slots[n]
        want = OA.copy_stochastic(x.reshape(-1), OA.sr_bits(seed, np.arange(slot.offset, slot.offset + slot.numel)))
    else:
        assert np.all(np.abs(got.astype(np.float64) - x) <= 0.5 * SF.bf16_ulp(got) + tol), n
        want = OA.f32_to_bf16_bits(x).reshape(-1)
    return bool(np.array_equal(gb, want))


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("form", FORMS)
def test_five_steps_against_the_oracle(dev, form, clip):
    is_bf16 = form.startswith("bf16")
    st, opt = make(dev, form, warmup_steps=2)
    ogroups = oracle_groups(warmup_steps=2)
    oz = [None] * len(NAMES)
    ov = [np.zeros(s, np.float32) for _, s in SF.SHAPES]
    tols = [SF.zeros_tol(s) for _, s in SF.SHAPES]
    exact = True
    for k in range(SF.STEPS):
        set_grads(st, k, 300.0 if clip else 1.0)
        set_lr(opt, ogroups, k)
        coef = None
        if clip:
            opt.clip_grad_norm_(1.0)
            coef = np.float32(opt.clip_out[0].item())
            assert 0 < coef < 1
        before = [value(st, n) for n in NAMES]
        seed = (opt.seed * LCG[0] + LCG[1]) & 0xFFFFFFFFFFFFFFFF
        opt.step()
        assert opt.seed == (seed if is_bf16 else 11) and not opt._pending_clip
        scs = [SF.group_scalars(og) for og in ogroups]
        for og, g in zip(ogroups, opt.param_groups):
            assert all(g[key] == og[key] for key in ("k", "weight_sum", "lr_max", "scheduled_lr"))
        for i, (n, s) in enumerate(SF.SHAPES):
            g = st.params[n].grad.float().cpu().numpy()
            if coef is not None:
                g = OA.rbf(g * coef) if is_bf16 else g * coef
            x, oz[i], ov[i], tol_y = SF.sf_step(before[i], g, oz[i], ov[i], scs[GROUP_OF[i]], tol=tols[i], clipped=clip)
            views = {key: v.cpu().numpy() for key, v in opt._views(n).items()}
            assert np.all(np.abs(views["z"].astype(np.float64) - oz[i]) <= tols[i]["z"]), (n, k)
            assert np.all(np.abs(views["exp_avg_sq"].astype(np.float64) - ov[i]) <= tols[i]["v"]), (n, k)
            same = np.array_equal(views["z"], oz[i]) and np.array_equal(views["exp_avg_sq"], ov[i])
            same = check_params(st, opt, form, n, x, tol_y, seed) and same
            print(f"{form} clip={clip} step {k} {n}: bit-equal to the oracle's fp32 path: {same}")
            exact = exact and same
            # the step moved it (a single bf16 element may round back to itself: the large tensors stand for the store)
            assert not np.array_equal(value(st, n), before[i]) or (is_bf16 and x.size < 4096), (n, k)
    # equal host scalars and IEEE arithmetic on both sides: the same bits, states and parameters
    assert exact
    # the padding between and behind the tensors belongs to no group and keeps its zeros
    mask = torch.ones(st.numel, dtype=torch.bool, device=dev)
    for n in NAMES:
        mask[st.slots[n].offset:st.slots[n].offset + st.slots[n].numel] = False
    for buf in (source(st), st.data, opt.z, opt.exp_avg_sq):
        assert mask.any() and not buf[mask].any()


@pytest.mark.parametrize("form", ["master", "bf16_sr"])
def test_window_uses_global_indices(dev, form):
    """a launch over [begin, end) writes those elements as the whole-store launch does and nothing else"""
    (a, oa), (b, ob) = make(dev, form), make(dev, form)
    for st, opt in ((a, oa), (b, ob)):   # one whole step first, so that z is read, not taken
        set_grads(st, 0)
        opt.step()
    set_grads(a, 1)
    set_grads(b, 1)
    start = [t.clone() for t in (source(b), b.data, ob.z, ob.exp_avg_sq)]
    oa.step()
    begin, end = 16, a.slots["s70001"].offset + 4096
    p, w = ob._pw()
    if w is None:
        ob.seed = oa.seed
    K.sf_adamw_step(p, b.grad, w, ob.z, ob.exp_avg_sq, ob._groups_struct(), stochastic_rounding=form == "bf16_sr",
                    seed=ob.seed, begin=begin, end=end)
    torch.cuda.synchronize()
    for full, part, was in zip((source(a), a.data, oa.z, oa.exp_avg_sq), (source(b), b.data, ob.z, ob.exp_avg_sq), start):
        assert torch.equal(part[begin:end], full[begin:end]) and not torch.equal(part[begin:end], was[begin:end])
        assert torch.equal(part[:begin], was[:begin]) and torch.equal(part[end:], was[end:])
    for bad in (dict(begin=4), dict(end=end + 1), dict(begin=end + 8), dict(end=b.numel + 8)):
        with pytest.raises(ValueError, match="range"):
            K.sf_adamw_step(p, b.grad, w, ob.z, ob.exp_avg_sq, ob._groups_struct(), **dict(dict(begin=begin, end=end), **bad))


def _run(dev, form, steps=3, clip=True, seed=11):
    st, opt = make(dev, form, seed=seed)
    for k in range(steps):
        set_grads(st, k, 300.0 if clip else 1.0)
        if clip:
            opt.clip_grad_norm_(1.0)
        opt.step()
    torch.cuda.synchronize()
    return st, opt


def test_stochastic_rounding_repeats_with_one_seed(dev):
    (a, oa), (b, ob), (c, oc) = _run(dev, "bf16_sr"), _run(dev, "bf16_sr"), _run(dev, "bf16_sr", seed=12)
    assert torch.equal(a.data.view(torch.int16), b.data.view(torch.int16))
    assert torch.equal(oa.z, ob.z) and torch.equal(oa.exp_avg_sq, ob.exp_avg_sq) and oa.seed == ob.seed
    assert not torch.equal(a.data.view(torch.int16), c.data.view(torch.int16))   # and another seed rounds otherwise


@pytest.mark.parametrize("form", FORMS)
def test_eval_gives_x_and_train_restores_y(dev, form):
    st, opt = _run(dev, form)
    y_bits, w_bits = source(st).clone(), st.data.clone()
    y = [value(st, n) for n in NAMES]
    with torch.no_grad():
        opt.eval()
    assert not opt.train_mode and all(not g["train_mode"] for g in opt.param_groups)
    exact = True
    for i, n in enumerate(NAMES):
        x, tol = SF.sf_swap(y[i], opt._views(n)["z"].cpu().numpy(), SF.eval_weight(0.9))
        exact = check_params(st, opt, "bf16" if form == "bf16_sr" else form, n, x, tol) and exact   # always RNE
        assert not np.array_equal(value(st, n), y[i]) or (form.startswith("bf16") and x.size < 4096), n
    assert exact
    x_bits = source(st).clone()
    opt.eval()                                               # a second eval() changes nothing
    assert torch.equal(source(st), x_bits)
    with pytest.raises(RuntimeError, match="train mode"):
        opt.step()
    opt.train()
    assert opt.train_mode and opt._y_saved is None
    assert torch.equal(source(st).view(torch.uint8), y_bits.view(torch.uint8))
    assert torch.equal(st.data.view(torch.uint8), w_bits.view(torch.uint8))
    opt.train()                                              # and a second train() changes nothing
    assert torch.equal(source(st).view(torch.uint8), y_bits.view(torch.uint8))


@pytest.mark.parametrize("form", ["f32", "master", "bf16"])
def test_resume_from_a_state_saved_in_eval_mode(dev, form):
    """state_dict() in eval mode, loaded over a store that holds x, then train(): y comes from the lerp, not from saved
    bits.  In fp32 x + (1 - beta1) (z - x) does not give back y's bits (six roundings and two fp32-rounded weights lie
    between), so the resumed run is not bit-identical on any form; it stays within the swap bound carried through the
    oracle's step bounds.  The measured difference is printed; on one MI355X the largest relative difference of a
    parameter over the three further steps was 1.2e-7 (one fp32 ulp) on the fp32 and master forms and 7.8e-3 (two bf16
    ulps) on the bf16 store."""
    a, oa = _run(dev, form, steps=2, clip=False)
    y = [value(a, n) for n in NAMES]
    oa.eval()
    sd = oa.state_dict()
    assert all(not g["train_mode"] and g["k"] == 2 for g in sd["param_groups"])
    b, ob = make(dev, form, seed=999, train=False)
    for n in NAMES:
        b.write(n, a.value(n))
    assert torch.equal(source(b), source(a))
    ob.load_state_dict(sd)
    assert not ob.train_mode and ob.seed == oa.seed and ob._z_set
    ob.train()
    oa.train()
    assert torch.equal(oa.z, ob.z) and torch.equal(oa.exp_avg_sq, ob.exp_avg_sq)
    we, wt = SF.eval_weight(0.9), SF.train_weight(0.9)
    delta = []
    for i, n in enumerate(NAMES):
        z = oa._views(n)["z"].cpu().numpy()
        x, tol_x = SF.sf_swap(y[i], z, we)
        if form == "bf16":
            x = OA.rbf(x)
        back, tol = SF.sf_swap(x, z, wt, tol_p=tol_x)
        # the two weights are rounded to fp32: together they miss the identity by at most 2 U (1 + |we|) |z - y|
        tol = tol + 2 * SF.U * (1 + abs(we)) * np.abs(z.astype(np.float64) - y[i])
        if form == "bf16":
            tol = SF.round_trip_bound(np.maximum(np.abs(y[i]), np.abs(back)), x, 0.9, tol)
        d = np.abs(value(b, n).astype(np.float64) - y[i])
        assert np.all(d <= tol), n
        delta.append(tol)
    ogroups = oracle_groups()
    for og, g in zip(ogroups, oa.param_groups):
        og.update({key: g[key] for key in ("k", "weight_sum", "lr_max")})
    worst = 0.0
    delta_z = [np.zeros(s) for _, s in SF.SHAPES]
    for k in range(2, 5):
        for st, opt in ((a, oa), (b, ob)):
            set_grads(st, k)
        before = [value(a, n) for n in NAMES]
        zs = [oa._views(n)["z"].cpu().numpy() for n in NAMES]
        vs = [oa._views(n)["exp_avg_sq"].cpu().numpy() for n in NAMES]
        oa.step()
        ob.step()
        scs = [SF.group_scalars(og) for og in ogroups]
        for i, (n, s) in enumerate(SF.SHAPES):
            g = a.params[n].grad.float().cpu().numpy()
            tz = {"z": delta_z[i], "v": np.zeros(s)}
            x, _, _, tol_y = SF.sf_step(before[i], g, zs[i], vs[i], scs[GROUP_OF[i]], tol=tz, tol_y=delta[i])
            delta_z[i] = tz["z"]
            delta[i] = tol_y + (SF.bf16_ulp(x) if form == "bf16" else 0.0)   # half an ulp of rounding on either run
            d = np.abs(value(b, n).astype(np.float64) - value(a, n).astype(np.float64))
            worst = max(worst, float((d / np.maximum(np.abs(value(a, n)), 1e-30)).max()))
            assert np.all(d <= delta[i]), (n, k)
            dz = np.abs(ob._views(n)["z"].cpu().numpy().astype(np.float64) - oa._views(n)["z"].cpu().numpy())
            assert np.all(dz <= delta_z[i]), (n, k)
    print(f"{form}: resumed run against the uninterrupted one, largest relative difference {worst:.3e}")
    assert torch.equal(oa.exp_avg_sq, ob.exp_avg_sq)          # v does not see y
    assert all(ga[key] == gb[key] for ga, gb in zip(oa.param_groups, ob.param_groups)
               for key in ("k", "weight_sum", "lr_max", "scheduled_lr", "train_mode"))


@pytest.mark.parametrize("form", ["f32", "bf16_sr"])
def test_lr_zero_keeps_y_and_z_and_updates_v(dev, form):
    st, opt = make(dev, form)
    start = st.data.clone()
    for g in opt.param_groups:
        g["lr"] = 0.0
    set_grads(st, 0)
    opt.step()
    assert all(g["weight_sum"] == 0.0 and g["k"] == 1 for g in opt.param_groups)
    assert torch.equal(st.data.view(torch.uint8), start.view(torch.uint8))
    assert torch.equal(opt.z, start.float())                 # z was taken from y and not moved
    for n in NAMES:
        g = st.params[n].grad.float()
        assert torch.equal(opt._views(n)["exp_avg_sq"] > 0, g != 0) and (g != 0).any()


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
    assert opt.param_groups[0]["k"] == 3


# ---- the trainer -----------------------------------------------------------------------------------------------------
VARIANTS = ["finetune", "lora", "dora"]


def _cfg(tmp, variant):
    from onetrainer_amd.util.config.TrainConfig import TrainConfig
    cfg = TrainConfig.default_values()
    cfg.batch_size = 2
    cfg.learning_rate = 1e-4
    cfg.learning_rate_warmup_steps = 0
    cfg.clip_grad_norm = 0.05
    cfg.workspace_dir = str(tmp)
    cfg.backup_before_save = False
    cfg.optimizer.optimizer = "SCHEDULE_FREE_ADAMW"   # every other field None: the reference's fall-backs
    if variant == "finetune":
        cfg.output_model_format = "DIFFUSERS"
    else:
        cfg.training_method = "LORA"
        cfg.lora_rank, cfg.lora_alpha = 8, 8.0
        cfg.lora_decompose = variant == "dora"
    return cfg


def _trainer(cfg, dev):
    from onetrainer_amd.module import unet as U
    from onetrainer_amd.trainer.GenericTrainer import GenericTrainer
    from onetrainer_amd.util import create
    model = create.create_model(cfg, dev, seed=7, unet_config=U.tiny_sdxl_config())
    tr = GenericTrainer(cfg, model=model)
    tr.start()
    assert isinstance(model.optimizer, FusedScheduleFreeAdamW) and model.optimizer.train_mode
    return tr


def _weights(tr):
    """the model's weights as the savers write them (file layout), read from the store as it stands"""
    lora = tr.model.unet_lora
    sd = lora.state_dict() if lora is not None else tr.model.unet.state_dict()
    return {k: v.detach().float().cpu().contiguous().clone() for k, v in sd.items() if v.is_floating_point()}


def _file_weights(path, variant, backup=False):
    from safetensors.torch import load_file
    if variant != "finetune":
        sd = load_file(os.path.join(path, "lora", "lora.safetensors") if backup else path)
    else:
        sd = load_file(os.path.join(path, "unet", "diffusion_pytorch_model.safetensors"))
    return {k: v.float() for k, v in sd.items() if v.is_floating_point()}


def _same_dict(a, b):
    return set(a) == set(b) and all(a[k].shape == b[k].shape and torch.equal(a[k], b[k]) for k in a)


def _derived(tr):
    """what the setup derives from the adapters: the LoRA bf16 shadows, or the DoRA merged weights and norms"""
    lora = tr.model.unet_lora
    if lora is None:
        return []
    return [lora.shadow] if hasattr(lora, "shadow") else [lora.wp, lora.norms]


@pytest.mark.parametrize("variant", VARIANTS)
def test_trainer_saves_x_and_trains_on(dev, tmp_path, variant):
    from onetrainer_amd.dataLoader.SyntheticDataLoader import synthetic_sdxl_batch
    batch = synthetic_sdxl_batch(2, 128, 128, dev, seed=3, te1_dim=48, te2_dim=48, pooled_dim=64)
    a, b = _trainer(_cfg(tmp_path / "a", variant), dev), _trainer(_cfg(tmp_path / "b", variant), dev)
    opt, st = a.model.optimizer, a.model.train_store
    for k in range(5):
        a.train_step(batch)
        b.train_step(batch)
        if k == 2:   # a backup and a save in the middle of run a (after the first step y = z = x: ckp1 is 1)
            y_bits = source(st).clone()
            y_w = _weights(a)
            derived = [t.clone() for t in _derived(a)]
            a._before_eval()
            assert not opt.train_mode
            x_w = _weights(a)                                 # optimizer.eval() of the live run, in file layout
            assert not _same_dict(x_w, y_w)
            x_at_backup = source(st).clone()
            swapped = [t.clone() for t in _derived(a)]
            if derived:   # the shadows / merged weights follow the swapped adapters: a fresh refresh() gives them
                assert any(not torch.equal(s, d) for s, d in zip(swapped, derived))
                a.model.unet_lora.refresh()
                assert all(torch.equal(s, t) for s, t in zip(swapped, _derived(a)))
            a._after_eval()
            assert opt.train_mode and torch.equal(source(st).view(torch.uint8), y_bits.view(torch.uint8))
            assert all(torch.equal(d, t) for d, t in zip(derived, _derived(a)))
            z_at_backup = opt.z.clone()
            backup = a.backup()
            saved = a.save(print_msg=False)
            assert backup and saved and opt.train_mode
            assert torch.equal(source(st).view(torch.uint8), y_bits.view(torch.uint8))
            assert all(torch.equal(d, t) for d, t in zip(derived, _derived(a)))
            assert _same_dict(_file_weights(saved, variant), x_w)                  # the written model holds x ...
            assert _same_dict(_file_weights(backup, variant, backup=True), x_w)    # ... and so does the backup
            osd = torch.load(os.path.join(backup, "optimizer", "optimizer.pt"), weights_only=False)
            assert all(not g["train_mode"] and g["k"] == 3 for g in osd["param_groups"])
    torch.cuda.synchronize()
    sb = b.model.train_store
    assert torch.equal(source(st).view(torch.uint8), source(sb).view(torch.uint8))   # bit-identical to the plain run
    assert torch.equal(st.data.view(torch.uint8), sb.data.view(torch.uint8))
    assert torch.equal(opt.z, b.model.optimizer.z)

    # resume from the backup: the loaded weights are x, the state says eval mode, start() calls train() once
    cfg_c = _cfg(tmp_path / "a", variant)
    cfg_c.continue_last_backup = True
    c = _trainer(cfg_c, dev)
    oc = c.model.optimizer
    assert c.model.train_progress.global_step == 3 and oc.train_mode and oc._z_set and oc.param_groups[0]["k"] == 3
    assert torch.equal(oc.z, z_at_backup) and not torch.equal(source(c.model.train_store), x_at_backup)   # y, not x
    c.train_step(batch)
    assert oc.param_groups[0]["k"] == 4

    # the final model is x and the optimizer stays in eval mode
    a._before_eval()
    x_w = _weights(a)
    a._after_eval()
    final_cfg = a.config
    final_cfg.output_model_destination = str(tmp_path / ("final" if variant == "finetune" else "final.safetensors"))
    final = a.end()
    assert final and not opt.train_mode and _same_dict(_file_weights(final, variant), x_w)
