"""Fused Prodigy (csrc/prodigy.hip, util/optimizer/prodigy_fused.py) on the GPU against the float64 restatement
tests/_oracle_prodigy.py, within the bounds derived there and returned beside its result.  prodigyopt, which the
reference imports, is not in the reference tree: nothing here is compared with it."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _oracle_adafactor as AF
import _oracle_prodigy as PR
from onetrainer_amd.module.param_store import FlatParamStore
from onetrainer_amd.util.optimizer.prodigy_fused import FusedProdigy
from oracle import adamw as OA

pytestmark = pytest.mark.gpu

SPLIT = 5                   # SHAPES[:SPLIT] -> group 0, the rest -> group 1, one learning rate
NAMES = [n for n, _ in AF.SHAPES]
LCG = (6364136223846793005, 1442695040888963407)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().astype(np.uint16)


def make(dev, form, sr=False, seed=11, lr=1.0, shapes=AF.SHAPES, **cfg):
    dtype = torch.float32 if form == "f32" else torch.bfloat16
    names = [n for n, _ in shapes]
    split = min(SPLIT, len(names) - 1) if len(names) > 1 else 1
    st = FlatParamStore([(n, s, "a" if i < split else "b") for i, (n, s) in enumerate(shapes)], dtype, dev,
                        master=form == "master")
    for n, s in shapes:
        st.write(n, torch.from_numpy(AF.param0(n, s)))
    groups = [{"params": [st.params[n] for n in part], "lr": lr} for part in (names[:split], names[split:]) if part]
    hyper = dict(cfg)
    betas = (hyper.pop("beta1", 0.9), hyper.pop("beta2", 0.999))
    return st, FusedProdigy(st, groups, lr=lr, betas=betas, stochastic_rounding=sr, seed=seed, **hyper)


def set_grads(st, k, mult=1.0):
    for n, s in AF.SHAPES:
        st.params[n].grad.copy_(torch.from_numpy(PR.case_grad(n, s, k) * np.float32(mult)))
    # "zero": case_grad is all zeros for it, as if it had received no gradient and the store had zeroed it


def value(st, n):
    return st.value(n).detach().float().cpu().numpy()


def device_coef(st, opt, form):
    """clip_grad_norm_(1.0) on the device, checked against the host restatement; returns the coefficient it holds"""
    opt.clip_grad_norm_(1.0)
    gl = [st.params[n].grad for n in NAMES]
    got = opt.clip_out[0].item()
    if form == "f32":
        _, coef = OA.clip_grad_norm_f32([g.cpu().numpy().reshape(-1) for g in gl], 1.0)
    elif form == "master":
        _, coef = OA.clip_grad_norm_f32([OA.bf16_to_f32(bits(g).reshape(-1)) for g in gl], 1.0)
    else:
        _, _, coef = OA.clip_grad_norm_bf16([bits(g).reshape(-1) for g in gl], 1.0)
        assert got == coef
    assert abs(got - coef) <= 16 * AF.U * coef and coef < 1.0   # fp32 norms folded in fp32 against float64
    return np.float32(got)


@pytest.mark.parametrize("case", list(PR.GPU_CASES))
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("form", ["f32", "master", "bf16", "bf16_sr"])
def test_three_steps_against_the_oracle(dev, form, clip, case):
    cfg = PR.GPU_CASES[case]
    sr, is_bf16 = form == "bf16_sr", form.startswith("bf16")
    st, opt = make(dev, form, sr=sr, **cfg)
    ost = [PR.new_state(s) for _, s in AF.SHAPES]
    apart = total = 0
    moved = False
    for k in range(PR.GPU_STEPS):
        set_grads(st, k, 300.0 if clip else 1.0)
        coef = device_coef(st, opt, form) if clip else None
        before = [value(st, n) for n in NAMES]
        sc = PR.scalars_from(opt.d_state())
        assert sc["k"] == k
        seed = (opt.seed * LCG[0] + LCG[1]) & 0xFFFFFFFFFFFFFFFF
        opt.step()
        assert opt.seed == (seed if is_bf16 else 11)
        grads = []
        for n in NAMES:
            g = st.params[n].grad.float().cpu().numpy()
            if coef is not None:
                g = OA.rbf(g * coef) if is_bf16 else g * coef
            grads.append(g)
        xs, info = PR.prodigy_step(before, grads, ost, sc, 1.0, **cfg)
        ds = opt.d_state()
        views = {n: {key: v.cpu().numpy().astype(np.float64) for key, v in opt._views(n).items()} for n in NAMES}
        # the two sums (read back from the chunk slots) and the scalars, within the float64 bounds
        num, den = float(opt._chunk_num[:opt._n_chunks].sum()), float(opt._chunk_den[:opt._n_chunks].sum())
        nc = opt._n_chunks
        assert abs(num - info["num"]) <= info["tol_num"] + nc * PR.E * abs(info["num"]), (k, num, info["num"])
        assert abs(den - info["den"]) <= info["tol_den"] + nc * PR.E * abs(info["den"]), (k, den, info["den"])
        assert abs(ds["d_denom"] - info["den"]) <= info["tol_den"]
        assert abs(ds["d_numerator"] - sc["d_numerator"]) <= sc["tol_dnum"], (k, ds, sc)
        assert abs(ds["d"] - sc["d"]) <= sc["tol_d"] and abs(ds["d_max"] - sc["d_max"]) <= sc["tol_dmax"], (k, ds, sc)
        assert ds["k"] == sc["k"] == k + 1 and not ds["skip"]
        moved = moved or ds["d"] != cfg["d0"]
        for i, (n, s) in enumerate(AF.SHAPES):
            o = ost[i]
            for key, okey in (("exp_avg", "m"), ("exp_avg_sq", "v"), ("s", "s")):
                assert np.all(np.abs(views[n][key] - o[okey]) <= o["tol"][okey]), (n, k, key)
            if k == 0:
                assert np.array_equal(views[n]["p0"], before[i].astype(np.float64)), n
            x, got = xs[i], value(st, n)
            if is_bf16:
                slot = st.slots[n]
                if sr:
                    rand = OA.sr_bits(seed, np.arange(slot.offset, slot.offset + slot.numel))
                    want = OA.copy_stochastic(x.reshape(-1), rand)
                else:
                    want = OA.f32_to_bf16_bits(x).reshape(-1)
                dist = AF.bf16_ulps(bits(st.params[n]).reshape(-1), want)
                assert dist.max() <= 1, (n, k, int(dist.max()))
                apart += int((dist != 0).sum())
                total += dist.size
            else:
                assert np.all(np.abs(got.astype(np.float64) - x) <= info["tol_p"][i]), (n, k)
                if form == "master":   # the working copy is rne(master), bit for bit
                    assert np.array_equal(bits(st.params[n]), OA.f32_to_bf16_bits(got))
            if n != "zero":   # ("zero" moves by its decay alone, which a round-to-nearest bf16 value does not show)
                assert not np.array_equal(got, before[i]), (n, k)   # the step moved it
    assert moved                                                    # d left d0 within the three steps
    if is_bf16:
        assert apart <= 1e-3 * total, (apart, total)


def test_free_run_of_d_stays_within_the_compounded_bound(dev):
    """six steps with nothing fed back: the device's d against the oracle's, both free-running, within the bound the
    oracle compounds from its s, num and parameter bounds (sc['tol_d']); the parameters within theirs"""
    cfg = PR.GPU_CASES["decoupled"]
    st, opt = make(dev, "f32", **cfg)
    ost, sc = [PR.new_state(s) for _, s in AF.SHAPES], PR.new_scalars(cfg["d0"])
    params, tol_p = [AF.param0(n, s) for n, s in AF.SHAPES], None
    for k in range(6):
        set_grads(st, k)
        opt.step()
        params, info = PR.prodigy_step(params, [PR.case_grad(n, s, k) for n, s in AF.SHAPES], ost, sc, 1.0,
                                       tol_p=tol_p, **cfg)
        tol_p = info["tol_p"]
        ds = opt.d_state()
        assert abs(ds["d"] - sc["d"]) <= sc["tol_d"], (k, ds["d"], sc["d"], sc["tol_d"])
        assert sc["tol_d"] < sc["d"]   # the compounded bound still says something about d
    assert ds["d"] > 4 * cfg["d0"] and ds["k"] == 6
    for i, n in enumerate(NAMES):
        assert np.all(np.abs(value(st, n).astype(np.float64) - params[i]) <= tol_p[i]), n


def _run(dev, form, sr, steps=PR.GPU_STEPS, clip=True, **cfg):
    st, opt = make(dev, form, sr=sr, **dict(PR.GPU_CASES["decoupled"], **cfg))
    for k in range(steps):
        set_grads(st, k, 300.0)
        if clip:
            opt.clip_grad_norm_(1.0)
        opt.step()
    torch.cuda.synchronize()
    return st, opt


def _same_state(oa, ob):
    names = ("exp_avg", "exp_avg_sq", "s", "p0")
    return (all(torch.equal(getattr(oa, b).view(torch.int32), getattr(ob, b).view(torch.int32)) for b in names)
            and torch.equal(oa._state.view(torch.int64), ob._state.view(torch.int64)))


@pytest.mark.parametrize("form, sr", [("bf16", True), ("master", False)])
def test_second_run_gives_identical_bits(dev, form, sr):
    a, oa = _run(dev, form, sr)
    b, ob = _run(dev, form, sr)
    assert torch.equal(a.data.view(torch.int16), b.data.view(torch.int16))
    assert _same_state(oa, ob)
    assert oa.exp_avg.abs().max() > 0 and oa.s.abs().max() > 0 and oa.d_state()["k"] == PR.GPU_STEPS
    if form == "master":
        assert torch.equal(a.master.view(torch.int32), b.master.view(torch.int32))


def test_lr_zero_is_a_no_op_and_p0_is_captured_by_the_first_real_step(dev):
    st, opt = make(dev, "f32", **PR.GPU_CASES["decoupled"])
    buffers = (st.data, opt.exp_avg, opt.exp_avg_sq, opt.s, opt.p0, opt._state)
    start = [b.clone() for b in buffers]
    for g in opt.param_groups:
        g["lr"] = 0.0
    set_grads(st, 0)
    opt.clip_grad_norm_(1.0)
    opt.step()
    assert all(torch.equal(a, b) for a, b in zip(start, buffers)) and opt.d_state()["k"] == 0
    assert not opt._pending_clip
    st.write("v37", torch.from_numpy(AF.param0("v37", (37,)) * np.float32(2)))   # the parameters move before step one
    now = st.data.clone()
    for g in opt.param_groups:
        g["lr"] = 1.0
    set_grads(st, 0)
    opt.step()
    assert torch.equal(opt.p0, now) and opt.d_state()["k"] == 1
    p0 = opt.p0.clone()
    set_grads(st, 1)
    opt.step()
    assert torch.equal(opt.p0, p0) and not torch.equal(st.data, p0) and opt.d_state()["k"] == 2


@pytest.mark.parametrize("form", ["f32", "bf16_sr"])
def test_zero_gradients_stop_the_step_early(dev, form):
    """all gradients zero: d_denom == 0, the parameters keep their bits (also under stochastic rounding and weight
    decay) and k stays 0"""
    st, opt = make(dev, form, sr=form == "bf16_sr", **PR.GPU_CASES["decoupled"])
    start = st.data.clone()
    st.grad.zero_()
    opt.step()
    ds = opt.d_state()
    assert ds["skip"] and ds["k"] == 0 and ds["d_denom"] == 0.0 and ds["d"] == PR.GPU_CASES["decoupled"]["d0"]
    assert torch.equal(st.data.view(torch.uint8), start.view(torch.uint8))
    set_grads(st, 0)   # and the next step with gradients runs
    opt.step()
    ds = opt.d_state()
    assert not ds["skip"] and ds["k"] == 1 and not torch.equal(st.data, start)


@pytest.mark.parametrize("form, sr, beta1", [("bf16", True, 0.9), ("f32", False, 0.9), ("master", False, 0.0)])
def test_state_dict_resumes_bit_exactly(dev, form, sr, beta1):
    a, oa = _run(dev, form, sr, steps=2, beta1=beta1)
    sd = oa.state_dict()
    assert set(sd) == {"state", "param_groups", "sr_seed"}
    keys = {"step", "s", "p0", "exp_avg", "exp_avg_sq"} - ({"exp_avg"} if beta1 == 0 else set())
    assert len(sd["state"]) == len(NAMES)
    for i, (n, s) in enumerate(AF.SHAPES):
        e = sd["state"][i]
        assert set(e) == keys and e["step"] == 2
        assert all(tuple(e[key].shape) == s and e[key].dtype == torch.float32 for key in keys - {"step"})
    g0 = sd["param_groups"][0]
    assert {"d", "d0", "d_max", "d_numerator", "d_denom", "d_hat", "k", "lr", "betas", "beta3", "eps", "weight_decay",
            "decouple", "use_bias_correction", "safeguard_warmup", "d_coef", "growth_rate", "sr_seed"} <= set(g0)
    ds = oa.d_state()
    assert g0["k"] == 2 and g0["d"] == ds["d"] and g0["d_numerator"] == ds["d_numerator"] and g0["d"] > g0["d0"]
    # upstream saves tensor(0) as the p0 of an all-zero parameter: a scalar is broadcast on load
    zero = NAMES.index("zero")
    sd["state"][zero]["p0"] = torch.tensor(0.0)
    oa.p0[a.slots["zero"].offset:a.slots["zero"].offset + a.slots["zero"].numel].zero_()
    b, ob = make(dev, form, sr=sr, seed=999, **dict(PR.GPU_CASES["decoupled"], beta1=beta1))
    b.data.copy_(a.data)
    if form == "master":
        b.master.copy_(a.master)
    ob.load_state_dict(sd)
    da, db = oa.d_state(), ob.d_state()   # dlr and skip belong to a step in flight and are not saved
    assert ob.seed == oa.seed and all(da[key] == db[key] for key in PR.scalars_from(da) if not key.startswith("tol"))
    for st, opt in ((a, oa), (b, ob)):
        set_grads(st, 2, 300.0)
        opt.clip_grad_norm_(1.0)
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(a.data.view(torch.uint8), b.data.view(torch.uint8))
    assert torch.equal(oa._state.view(torch.int64), ob._state.view(torch.int64)) and oa.d_state()["k"] == 3
    for name in ("exp_avg_sq", "s", "p0") + (("exp_avg",) if beta1 else ()):
        assert torch.equal(getattr(oa, name), getattr(ob, name)), name


def test_step_does_not_synchronise_the_host(dev):
    """step() behind a long kernel returns while that kernel's event is incomplete, and raises nothing under torch's
    synchronisation debug mode; param_groups' d follows at most one step behind without blocking"""
    st, opt = make(dev, "bf16", sr=True, **PR.GPU_CASES["decoupled"])
    for k in range(2):   # warm-up: code objects loaded, pinned copies primed
        set_grads(st, k)
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
        opt.step()
        d_seen = opt.param_groups[0]["d"]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert not ev.query()   # the host is back before the device reached the step
    torch.cuda.synchronize()
    ds = opt.d_state()
    assert ds["k"] == 3 and d_seen > 0
    opt._poll()
    assert opt.param_groups[0]["d"] == opt.param_groups[1]["d"] == ds["d"]   # the copy of the last step has landed


def _trainer_run(dev, method, overlap=True, steps=3):
    from onetrainer_amd.dataLoader.SyntheticDataLoader import synthetic_sdxl_batch
    from onetrainer_amd.module import unet as U
    from onetrainer_amd.trainer.GenericTrainer import GenericTrainer
    from onetrainer_amd.util import create
    from onetrainer_amd.util.config.TrainConfig import TrainConfig
    cfg = TrainConfig.default_values()
    cfg.batch_size = 2
    cfg.learning_rate_warmup_steps = 0
    cfg.clip_grad_norm = 0.05
    cfg.training_method = method
    if method == "LORA":
        cfg.lora_rank, cfg.lora_alpha = 8, 8.0
    cfg.optimizer.optimizer = "PRODIGY"   # every other field None: the reference's fall-backs (create.py:865-880)
    cfg.learning_rate = 1.0
    model = create.create_model(cfg, dev, seed=7, unet_config=U.tiny_sdxl_config())
    tr = GenericTrainer(cfg, model=model)
    tr.start()
    opt = model.optimizer
    assert isinstance(opt, FusedProdigy)
    assert opt.norm_overlap is not None
    if not overlap:
        opt.norm_overlap = None
    scalars = []
    tr.tensorboard = SimpleNamespace(add_scalar=lambda tag, v, step: scalars.append((tag, v)), close=lambda: None)
    batch = synthetic_sdxl_batch(2, 128, 128, dev, seed=3, te1_dim=48, te2_dim=48, pooled_dim=64)
    losses = [float(tr.train_step(batch)) for _ in range(steps)]
    torch.cuda.synchronize()
    return losses, model.train_store.data.clone(), opt, scalars, tr


@pytest.mark.parametrize("method", ["FINE_TUNE", "LORA"])
def test_trainer_steps_with_prodigy(dev, method):
    l1, p1, opt, scalars, tr = _trainer_run(dev, method)
    l2, p2 = _trainer_run(dev, method)[:2]
    l3, p3 = _trainer_run(dev, method, overlap=False)[:2]
    assert all(np.isfinite(l1)) and len(l1) == 3
    assert l1 == l2 and torch.equal(p1.view(torch.uint8), p2.view(torch.uint8))      # bitwise repeatable
    assert torch.equal(p1.view(torch.uint8), p3.view(torch.uint8))                   # overlapped norm = end-of-step norm
    ds = opt.d_state()
    assert ds["k"] == 3 and ds["d"] >= opt.param_groups[0]["d0"] == 1e-6
    assert opt.param_groups[0]["d"] >= opt.param_groups[0]["d0"]
    lrs = [v for tag, v in scalars if tag.startswith("lr/")]
    assert lrs and lrs[-1] == tr.lr_scheduler.get_last_lr()[0] * opt.param_groups[0]["d"]   # lr * d is reported
