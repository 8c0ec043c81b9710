"""Fused CAME (csrc/came.hip, util/optimizer/came_fused.py) on the GPU against the NumPy restatement
tests/_oracle_came.py, which tests/test_came_oracle.py pins to the reference's own run.  The bounds are the ones
derived there and returned beside the oracle's result: second-moment states within ((n - 1) + 8 k) 2^-24 relative,
the first moment within tol_m, the instability states within their S, fp32 parameters within one step's tol_p, bf16
parameters equal or one bf16 ulp apart with at most 1e-3 of them apart."""
import numpy as np
import pytest
import torch

import _oracle_adafactor as AF
import _oracle_came as CM
from onetrainer_amd.module.param_store import FlatParamStore
from onetrainer_amd.util.optimizer.came_fused import FusedCAME
from oracle import adamw as OA

pytestmark = pytest.mark.gpu

CFG = dict(weight_decay=0.01, clip_threshold=1.0, betas=(0.9, 0.999, 0.9999))
LRS = (1e-4, 3e-5)          # two parameter groups
SPLIT = 5                   # SHAPES[:SPLIT] -> group 0, the rest -> group 1
NAMES = [n for n, _ in AF.SHAPES]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().astype(np.uint16)


def make_store(dev, form):
    dtype = torch.float32 if form == "f32" else torch.bfloat16
    st = FlatParamStore([(n, s, "a" if i < SPLIT else "b") for i, (n, s) in enumerate(AF.SHAPES)], dtype, dev,
                        master=form == "master")
    for n, s in AF.SHAPES:
        st.write(n, torch.from_numpy(AF.param0(n, s)))
    return st


def groups_of(st):
    return [{"params": [st.params[n] for n in NAMES[:SPLIT]], "lr": LRS[0]},
            {"params": [st.params[n] for n in NAMES[SPLIT:]], "lr": LRS[1]}]


def make(dev, form, sr=False, seed=11, cfg=CFG):
    st = make_store(dev, form)
    return st, FusedCAME(st, groups_of(st), lr=LRS[0], stochastic_rounding=sr, seed=seed, **cfg)


def set_grads(st, k, mult=1.0):
    for n, s in AF.SHAPES:
        st.params[n].grad.copy_(torch.from_numpy(AF.grad(n, s, k) * np.float32(mult)))
    # "zero" received no gradient: the store zeroes it (finish_backward), the step sees zeros


def value(st, n):
    return st.value(n).detach().float().cpu().numpy()


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("form", ["f32", "master", "bf16", "bf16_sr"])
def test_three_steps_against_the_oracle(dev, form, clip):
    sr = form == "bf16_sr"
    is_bf16 = form.startswith("bf16")
    st, opt = make(dev, form, sr=sr)
    ost = {n: CM.new_state(s) for n, s in AF.SHAPES}
    apart = total = 0
    for k in range(AF.STEPS):
        set_grads(st, k, 3.0 if clip else 1.0)
        coef = None
        if clip:
            opt.clip_grad_norm_(1.0)
            gl = [st.params[n].grad for n in NAMES]
            if form == "f32":
                _, coef = OA.clip_grad_norm_f32([g.cpu().numpy().reshape(-1) for g in gl], 1.0)
            elif form == "master":
                _, coef = OA.clip_grad_norm_f32([OA.bf16_to_f32(bits(g).reshape(-1)) for g in gl], 1.0)
            else:
                _, _, coef = OA.clip_grad_norm_bf16([bits(g).reshape(-1) for g in gl], 1.0)
            got_coef = opt.clip_out[0].item()
            if is_bf16:
                assert got_coef == coef and coef < 1.0
            else:   # fp32 norms: the kernel folds the ten tensors' norms in fp32, the oracle in float64 -> 16 U;
                assert abs(got_coef - coef) <= 16 * AF.U * coef and coef < 1.0   # the step under test gets the
                coef = np.float32(got_coef)                                      # coefficient the device holds
        before = {n: value(st, n) for n in NAMES}
        seed = (opt.seed * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        opt.step()
        if is_bf16:
            assert opt.seed == seed
        for i, (n, s) in enumerate(AF.SHAPES):
            g = st.params[n].grad.float().cpu().numpy()
            if coef is not None:
                g = OA.rbf(g * np.float32(coef)) if is_bf16 else g * np.float32(coef)
            x, info = CM.came_step(before[n], g, ost[n], lr=LRS[0] if i < SPLIT else LRS[1], bf16=form == "bf16",
                                   **CFG)
            got_state = {k2: v.cpu().numpy().astype(np.float64) for k2, v in opt._views(n).items()}
            for key, gkey in CM.SQ_KEYS.items():
                if key in ost[n]:
                    ref = ost[n][key]
                    assert np.all(np.abs(got_state[gkey] - ref) <= CM.sq_bound(s, key, k + 1, ref)), (n, k, gkey)
            for key, gkey in CM.RES_KEYS.items():
                if key in ost[n]:
                    assert np.all(np.abs(got_state[gkey] - ost[n][key]) <= ost[n]["tol"][key]), (n, k, gkey)
            assert np.all(np.abs(got_state["exp_avg"] - ost[n]["m"]) <= info["tol_m"]), (n, k, "exp_avg")
            got = value(st, n)
            if is_bf16:
                slot = st.slots[n]
                if sr:
                    rand = OA.sr_bits(seed, np.arange(slot.offset, slot.offset + slot.numel))
                    want = OA.copy_stochastic(x.reshape(-1), rand)
                else:
                    want = OA.f32_to_bf16_bits(x).reshape(-1)
                d = AF.bf16_ulps(bits(st.params[n]).reshape(-1), want)
                assert d.max() <= 1, (n, k, int(d.max()))
                apart += int((d != 0).sum())
                total += d.size
            else:
                # every step restarts from the GPU's parameters, so the bound is one step's (the states carry on)
                assert np.all(np.abs(got.astype(np.float64) - x) <= info["tol_p"]), (n, k)
                if form == "master":   # the working copy is rne(master), bit for bit
                    assert np.array_equal(bits(st.params[n]), OA.f32_to_bf16_bits(got))
    if is_bf16:
        assert apart <= 1e-3 * total, (apart, total)


def _run(dev, form, sr, steps=AF.STEPS, clip=True):
    st, opt = make(dev, form, sr=sr)
    for k in range(steps):
        set_grads(st, k, 3.0)
        if clip:
            opt.clip_grad_norm_(1.0)
        opt.step()
    torch.cuda.synchronize()
    return st, opt


def _same_moments(oa, ob):
    return all(torch.equal(getattr(oa, b).view(torch.int32), getattr(ob, b).view(torch.int32))
               for b in ("state_buf", "res_buf", "exp_avg"))


@pytest.mark.parametrize("form, sr", [("bf16", True), ("master", False)])
def test_second_run_gives_identical_bits(dev, form, sr):
    a, oa = _run(dev, form, sr)
    b, ob = _run(dev, form, sr)
    assert torch.equal(a.data.view(torch.int16), b.data.view(torch.int16))
    assert _same_moments(oa, ob)
    assert oa.exp_avg.abs().max() > 0 and oa.res_buf.abs().max() > 0
    if form == "master":
        assert torch.equal(a.master.view(torch.int32), b.master.view(torch.int32))


@pytest.mark.parametrize("name", ["m300x1030", "conv3", "v37", "m2x4100"])
def test_step_parameter_is_the_tensors_slice_of_a_store_step(dev, name):
    whole, ow = _run(dev, "bf16", False, steps=1, clip=False)
    st, opt = make(dev, "bf16")
    set_grads(st, 0, 3.0)
    before = st.data.clone()
    gi = 0 if NAMES.index(name) < SPLIT else 1
    opt.step_parameter(st.params[name], opt.param_groups[gi], 0)
    torch.cuda.synchronize()
    s = st.slots[name]
    sl = slice(s.offset, s.offset + s.numel)
    assert torch.equal(st.data[sl].view(torch.int16), whole.data[sl].view(torch.int16))
    # the step ran on this tensor: its first moment is set (an unfactored tensor's update is m = 0.1 u, and lr times
    # that is below half a bf16 ulp of these parameters, so the vectors' bf16 values need not move in one step)
    assert opt.exp_avg[sl].abs().max() > 0
    if len(s.shape) >= 2:
        assert not torch.equal(st.data[sl], before[sl])
    keep = torch.ones(st.numel, dtype=torch.bool, device=st.data.device)
    keep[sl] = False
    assert torch.equal(st.data[keep].view(torch.int16), before[keep].view(torch.int16))   # neighbours untouched
    assert torch.equal(opt.exp_avg[sl], ow.exp_avg[sl]) and not opt.exp_avg[keep].any()
    for key, v in opt._views(name).items():
        assert torch.equal(v, ow._views(name)[key]), key
    other = next(n for n in NAMES if n != name and len(dict(AF.SHAPES)[n]) >= 2)
    assert not any(v.any() for v in opt._views(other).values())


def test_slab_order_is_adafactors(dev):
    """beta2 = 0 makes step one's second-moment states the plain means, as Adafactor's step one (beta2t = 0): the same
    gradients give the same bits, so the partial sums are folded in Adafactor's order"""
    from onetrainer_amd.util.optimizer.adafactor_fused import FusedAdafactor
    st, opt = make(dev, "bf16", cfg=dict(CFG, betas=(0.9, 0.0, 0.9999)))
    sa = make_store(dev, "bf16")
    oa = FusedAdafactor(sa, groups_of(sa), lr=LRS[0], relative_step=False, scale_parameter=False)
    for s_, o in ((st, opt), (sa, oa)):
        set_grads(s_, 0, 3.0)
        o.step()
    torch.cuda.synchronize()
    seen = 0
    for n, s in AF.SHAPES:
        if len(s) >= 2:
            for key in ("exp_avg_sq_row", "exp_avg_sq_col"):
                a, b = opt._views(n)[key], oa._views(n)[key]
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (n, key)
                seen += int(a.abs().max() > 0)
    assert seen >= 14


@pytest.mark.parametrize("form, sr", [("bf16", True), ("f32", False)])
def test_state_dict_resumes_bit_exactly(dev, form, sr):
    a, oa = _run(dev, form, sr, steps=2)
    sd = oa.state_dict()
    assert set(sd) == {"state", "param_groups", "sr_seed"}
    first = sd["state"][0]
    assert set(first) == {"step", "RMS", "exp_avg", "exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_res_row",
                          "exp_avg_res_col"} and first["step"] == 2 and float(first["RMS"]) == 0.0
    assert first["exp_avg"].shape == (64, 70) and first["exp_avg"].dtype == torch.float32
    assert first["exp_avg_sq_row"].shape == first["exp_avg_res_row"].shape == (64,)
    assert first["exp_avg_sq_col"].shape == first["exp_avg_res_col"].shape == (70,)
    assert set(sd["state"][6]) == {"step", "RMS", "exp_avg", "exp_avg_sq"}
    assert tuple(sd["state"][4]["exp_avg_res_row"].shape) == (3, 5, 3)
    assert tuple(sd["state"][4]["exp_avg_res_col"].shape) == (3, 5, 3)
    assert tuple(sd["param_groups"][0]["betas"]) == CFG["betas"]
    b, ob = make(dev, form, sr=sr, seed=999)
    b.data.copy_(a.data)
    ob.load_state_dict(sd)
    for st, opt in ((a, oa), (b, ob)):
        set_grads(st, 2, 3.0)
        opt.clip_grad_norm_(1.0)
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(a.data.view(torch.uint8), b.data.view(torch.uint8))
    assert _same_moments(oa, ob)


def _rms_u(g, row, col):
    """rms(u) in float64 on the host: u = g rsqrt(row / mean(row)) rsqrt(col) with the fresh states"""
    g, row, col = (t.detach().double().cpu() for t in (g, row, col))
    u = g * (row / row.mean(-1, keepdim=True)).rsqrt().unsqueeze(-1) * col.rsqrt().unsqueeze(-2)
    return float(u.pow(2).mean().sqrt())


@pytest.mark.parametrize("form", ["bf16", "f32"])
def test_batched_big_matrices_step_as_separate_matrices(dev, form):
    """mode 2 with batch 2: a (2, 70, 70) tensor (4900 elements a matrix: more than one LDS stage, and the second
    matrix starts off the 8-element alignment) steps bit for bit as two (70, 70) tensors with the same values.  Row
    sums depend on the column index within the tile only, column sums and row-state means on the row order only;
    neither depends on alignment.  clip_threshold=100 keeps the per-tensor rms(u) clip inactive (checked on the
    host): rms(u) is the one per-tensor quantity that differs between the two layouts."""
    dtype = torch.float32 if form == "f32" else torch.bfloat16
    cfg = dict(lr=LRS[0], clip_threshold=100.0)
    a = FlatParamStore([("ab", (2, 70, 70), "a")], dtype, dev)
    b = FlatParamStore([("m0", (70, 70), "a"), ("m1", (70, 70), "a")], dtype, dev)
    p0 = AF.param0("ab", (2, 70, 70))
    a.write("ab", torch.from_numpy(p0))
    for i in range(2):
        b.write(f"m{i}", torch.from_numpy(p0[i]))
    oa = FusedCAME(a, [{"params": [a.params["ab"]]}], **cfg)
    ob = FusedCAME(b, [{"params": [b.params["m0"], b.params["m1"]]}], **cfg)
    assert oa._table[0].mode == 2 and oa._table[0].batch == 2 and a.slots["ab"].offset % 8 == 0
    for k in range(AF.STEPS):
        g = AF.grad("ab", (2, 70, 70), k)
        a.params["ab"].grad.copy_(torch.from_numpy(g))
        for i in range(2):
            b.params[f"m{i}"].grad.copy_(torch.from_numpy(g[i]))
        oa.step()
        ob.step()
        torch.cuda.synchronize()
        va = oa._views("ab")
        # rms(u) / clip_threshold < 1, recomputed on the host: the clip is inactive in both layouts
        rms = [_rms_u(a.params["ab"].grad, va["exp_avg_sq_row"], va["exp_avg_sq_col"])]
        rms += [_rms_u(b.params[f"m{i}"].grad, *(ob._views(f"m{i}")[key] for key in ("exp_avg_sq_row", "exp_avg_sq_col")))
                for i in range(2)]
        assert all(0 < r / cfg["clip_threshold"] < 1 for r in rms), rms
        for i in range(2):
            vb = ob._views(f"m{i}")
            assert set(va) == set(vb) == {"exp_avg", "exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_res_row",
                                          "exp_avg_res_col"}
            for key in va:
                assert torch.equal(va[key][i].view(torch.int32), vb[key].view(torch.int32)), (k, i, key)
                assert va[key][i].abs().max() > 0
            assert torch.equal(a.params["ab"][i].detach().view(torch.uint8),
                               b.params[f"m{i}"].detach().view(torch.uint8)), (k, i)
    assert not torch.equal(a.params["ab"].detach().float().cpu(), torch.from_numpy(p0))   # the steps moved it


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
    cfg.optimizer.optimizer = "CAME"      # every other field None: the reference's fall-backs (create.py:944-949)
    model = create.create_model(cfg, dev, seed=7, unet_config=U.tiny_sdxl_config())
    tr = GenericTrainer(cfg, model=model)
    tr.start()
    opt = model.optimizer
    assert isinstance(opt, FusedCAME)
    assert opt.norm_overlap is not None
    if not overlap:
        opt.norm_overlap = None
    batch = synthetic_sdxl_batch(2, 128, 128, dev, seed=3, te1_dim=48, te2_dim=48, pooled_dim=64)
    losses = [float(tr.train_step(batch)) for _ in range(steps)]
    torch.cuda.synchronize()
    return losses, model.train_store.data.clone()


@pytest.mark.parametrize("method", ["FINE_TUNE", "LORA"])
def test_trainer_steps_with_came(dev, method):
    l1, p1 = _trainer_run(dev, method)
    l2, p2 = _trainer_run(dev, method)
    l3, p3 = _trainer_run(dev, method, overlap=False)
    assert all(np.isfinite(l1)) and len(l1) == 3
    assert l1 == l2 and torch.equal(p1.view(torch.uint8), p2.view(torch.uint8))      # bitwise repeatable
    assert torch.equal(p1.view(torch.uint8), p3.view(torch.uint8))                   # overlapped norm = end-of-step norm
