"""Schedule-free AdamW on the CPU: the restatement tests/_oracle_schedule_free.py against cases worked by hand, the
properties of its scalars, and the wiring (options, refusals, state layout) of util/optimizer/schedule_free_fused.py.
The schedulefree package is not in the reference tree: nothing here is compared with it."""
import numpy as np
import pytest
import torch

import _oracle_schedule_free as SF

F = np.float32


def test_two_steps_by_hand():
    """beta1 = 0.5, beta2 = 0.75, eps = 0, no decay, lr = 0.5, y0 = (1, 2, -4); every number is a dyadic rational, so
    float64 and the fp32 path give exactly these values.
    step 1 (k = 0), g = (1, -2, 4): bc2 = 0.25; lr_max = 0.5, weight = 0.25, weight_sum = 0.25, ckp1 = 1;
        a_y = 0.5 (0.5 * 0 - 1) = -0.5;  v = 0.25 g^2 = (0.25, 1, 4);  v / bc2 = g^2, gn = sign(g) = (1, -1, 1)
        y = y + 1 (z - y) = (1, 2, -4);  y = y - 0.5 gn = (0.5, 2.5, -4.5);  z = z - 0.5 gn = (0.5, 2.5, -4.5)
    step 2 (k = 1), g = (-1, -2, 4): bc2 = 1 - 0.5625 = 0.4375; weight = 0.25, weight_sum = 0.5, ckp1 = 0.5;
        a_y = 0.5 (0.5 * 0.5 - 1) = -0.375;  v = 0.75 v + 0.25 g^2 = 0.4375 g^2 = (0.4375, 1.75, 7);  gn = (-1, -1, 1)
        y = y + 0.5 (z - y) = (0.5, 2.5, -4.5);  y = y - 0.375 gn = (0.875, 2.875, -4.875)
        z = z - 0.5 gn = (1, 3, -5)
    eval: x = y + (1 - 2) (z - y) = 2 y - z = (0.75, 2.75, -4.75), the mean of the two z."""
    grp = SF.new_group(0.5, beta1=0.5, beta2=0.75, eps=0.0, weight_decay=0.0)
    y0 = np.array([1.0, 2.0, -4.0])
    sc = SF.group_scalars(grp)
    assert (sc["ckp1"], sc["a_y"], sc["bc2"], sc["lr"]) == (1.0, -0.5, 0.25, 0.5)
    g1 = np.array([1.0, -2.0, 4.0])
    y, z, v = SF.sf_step_f64(y0, g1, y0, np.zeros(3), sc)
    assert y.tolist() == [0.5, 2.5, -4.5] and z.tolist() == [0.5, 2.5, -4.5] and v.tolist() == [0.25, 1.0, 4.0]
    yf, zf, vf, _ = SF.sf_step(y0, g1, None, np.zeros(3, F), sc)
    assert yf.dtype == F and yf.tolist() == y.tolist() and zf.tolist() == z.tolist() and vf.tolist() == v.tolist()
    sc = SF.group_scalars(grp)
    assert (sc["ckp1"], sc["a_y"], sc["bc2"]) == (0.5, -0.375, 0.4375) and grp["weight_sum"] == 0.5 and grp["k"] == 2
    g2 = np.array([-1.0, -2.0, 4.0])
    y, z, v = SF.sf_step_f64(y, g2, z, v, sc)
    assert y.tolist() == [0.875, 2.875, -4.875] and z.tolist() == [1.0, 3.0, -5.0] and v.tolist() == [0.4375, 1.75, 7.0]
    yf, zf, vf, tol_y = SF.sf_step(yf, g2, zf, vf, sc)
    assert yf.tolist() == y.tolist() and zf.tolist() == z.tolist() and vf.tolist() == v.tolist()
    assert np.all(tol_y > 0) and np.all(tol_y < 32 * SF.U * 5)
    x = SF.swap_f64(y, z, SF.eval_weight(0.5))
    assert x.tolist() == [0.75, 2.75, -4.75]
    xf, _ = SF.sf_swap(yf, zf, SF.eval_weight(0.5))
    assert xf.tolist() == x.tolist()


def test_ckp1_is_one_over_k_plus_one_at_constant_lr():
    grp = SF.new_group(3e-4)
    for k in range(50):
        sc = SF.group_scalars(grp)
        assert abs(sc["ckp1"] - 1 / (k + 1)) <= 4 * 2.0 ** -53 and sc["lr"] == 3e-4
        assert sc["a_y"] == 3e-4 * (0.9 * (1 - sc["ckp1"]) - 1)


def test_weights_follow_lr_max_inside_the_warm_up():
    grp = SF.new_group(1e-3, warmup_steps=4, r=1)
    sums = 0.0
    for k in range(8):
        sc = SF.group_scalars(grp)
        lr = 1e-3 * min(1.0, (k + 1) / 4)
        assert sc["lr"] == lr == grp["scheduled_lr"] and grp["lr_max"] == lr
        assert sc["weight"] == (k + 1) * lr ** 2          # r = 1, weight_lr_power = 2
        sums += sc["weight"]
        assert sc["ckp1"] == sc["weight"] / sums
    grp["lr"] = 1e-4                                        # the scheduler lowers lr: lr_max stays
    sc = SF.group_scalars(grp)
    assert sc["lr"] == 1e-4 and grp["lr_max"] == 1e-3 and sc["weight"] == 9 * 1e-3 ** 2


def test_lr_zero_on_the_first_step():
    grp = SF.new_group(0.0)
    sc = SF.group_scalars(grp)
    assert grp["weight_sum"] == 0.0 and sc["ckp1"] == 0.0 and sc["a_y"] == 0.0 and grp["lr_max"] == 0.0
    y0, g = np.array([0.5, -0.25, 2.0], F), np.array([0.1, 0.2, -0.3], F)
    y, z, v, _ = SF.sf_step(y0, g, None, np.zeros(3, F), sc)
    assert np.array_equal(y, y0) and np.array_equal(z, y0) and np.all(v > 0)


def test_train_undoes_eval_in_float64():
    rng = np.random.default_rng(3)
    y, z = rng.normal(size=64), rng.normal(size=64)
    for beta1 in (0.5, 0.9, 0.95):
        x = SF.swap_f64(y, z, SF.eval_weight(beta1))
        assert np.allclose(x, y + (1 - 1 / beta1) * (z - y), rtol=0, atol=0)
        back = SF.swap_f64(x, z, SF.train_weight(beta1))
        assert np.all(np.abs(back - y) <= 8 * 2.0 ** -53 * (np.abs(y) + np.abs(z)))


def test_fp32_path_stays_within_its_bounds_of_float64():
    """the bounds are forward error bounds of the fp32 path: against float64 arithmetic on the same fp32 scalars, fed
    the fp32 path's y before every step (as the GPU tests feed the device's), z, v and y stay within them"""
    rng = np.random.default_rng(5)
    y = rng.normal(size=256).astype(F)
    grp = SF.new_group(1e-2)
    z, v = None, np.zeros(256, F)
    z64, v64 = y.astype(np.float64), np.zeros(256)
    tol = SF.zeros_tol(y.shape)
    for k in range(4):
        g = rng.normal(size=256).astype(F)
        sc = SF.group_scalars(grp)
        scf = {key: float(F(sc[key])) for key in ("lr", "a_y", "ckp1", "beta2", "eps", "weight_decay")}
        scf.update(one_minus_beta2=float(F(1 - sc["beta2"])), inv_bc2=float(F(1 / sc["bc2"])))
        y64, z64, v64 = SF.sf_step_f64(y, g, z64, v64, scf)
        y, z, v, tol_y = SF.sf_step(y, g, z, v, sc, tol=tol)
        assert np.all(np.abs(v - v64) <= tol["v"]) and np.all(np.abs(z - z64) <= tol["z"])
        assert np.all(np.abs(y - y64) <= tol_y)
        assert np.all(tol_y <= 64 * SF.U * (np.abs(y) + np.abs(z) + 1e-2))   # and they are a few ulps, not a blanket


# ---- wiring ----------------------------------------------------------------------------------------------------------
def _cfg():
    from onetrainer_amd.util.config.TrainConfig import TrainConfig
    cfg = TrainConfig.default_values()
    cfg.optimizer.optimizer = "SCHEDULE_FREE_ADAMW"
    return cfg


def test_schedule_free_options_defaults():
    from onetrainer_amd.util.config.TrainConfig import OptimizerConfig
    from onetrainer_amd.util.create import schedule_free_options
    assert schedule_free_options(OptimizerConfig(optimizer="SCHEDULE_FREE_ADAMW")) == SF.DEFAULTS
    given = dict(beta1=0.8, beta2=0.99, weight_decay=0.1, eps=1e-6, r=1, weight_lr_power=1.0, foreach=True)
    assert schedule_free_options(OptimizerConfig(optimizer="SCHEDULE_FREE_ADAMW", **given)) == given


def test_train_config_reads_the_schedule_free_fields():
    from onetrainer_amd.util.config.TrainConfig import OptimizerConfig, TrainConfig
    cfg = TrainConfig().from_dict({"optimizer": {"optimizer": "SCHEDULE_FREE_ADAMW", "r": 1.0, "weight_lr_power": 0.5}})
    assert (cfg.optimizer.optimizer, cfg.optimizer.r, cfg.optimizer.weight_lr_power) == ("SCHEDULE_FREE_ADAMW", 1.0, 0.5)
    assert OptimizerConfig().r is None and OptimizerConfig().weight_lr_power is None


def test_created_optimizer_is_fused_schedule_free_adamw():
    """on the CPU the construction is intercepted: the class is FusedScheduleFreeAdamW and the arguments are exactly
    the resolved options, the warm-up steps being the raw config value (create.py:763)"""
    from onetrainer_amd.util.create import create_optimizer
    from onetrainer_amd.util.optimizer import schedule_free_fused
    seen = {}

    class Probe(schedule_free_fused.FusedScheduleFreeAdamW):
        def __init__(self, store, groups, **kw):
            seen.update(kw)

    cfg = _cfg()
    cfg.learning_rate = 2e-4
    cfg.learning_rate_warmup_steps = 200
    cfg.gradient_accumulation_steps = 4
    orig, schedule_free_fused.FusedScheduleFreeAdamW = schedule_free_fused.FusedScheduleFreeAdamW, Probe
    try:
        assert isinstance(create_optimizer(None, [], cfg), orig)
    finally:
        schedule_free_fused.FusedScheduleFreeAdamW = orig
    assert seen == dict(lr=2e-4, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8, warmup_steps=200, r=0,
                        weight_lr_power=2.0, foreach=False,
                        stochastic_rounding=bool(cfg.optimizer.stochastic_rounding))


def test_lion_is_still_refused_with_the_old_words():
    from onetrainer_amd.util.create import create_optimizer
    cfg = _cfg()
    cfg.optimizer.optimizer = "LION"
    with pytest.raises(NotImplementedError) as e:
        create_optimizer(None, [], cfg)
    msg = str(e.value)
    assert "LION" in msg and "ADAMW, ADAFACTOR and CAME" in msg and "PRODIGY" in msg and "SCHEDULE_FREE_ADAMW" in msg


def test_fused_back_pass_is_refused_by_name():
    from onetrainer_amd.util.create import create_optimizer
    from onetrainer_amd.util.optimizer.schedule_free_fused import FusedScheduleFreeAdamW
    cfg = _cfg()
    cfg.optimizer.fused_back_pass = True
    with pytest.raises(NotImplementedError, match="fused_back_pass"):
        create_optimizer(None, [{"params": [], "lr": 1e-3}], cfg)
    with pytest.raises(NotImplementedError, match="step_parameter"):
        FusedScheduleFreeAdamW.step_parameter(None, None, None, 0)


def _cpu_optimizer(**kw):
    from onetrainer_amd.module.param_store import FlatParamStore
    from onetrainer_amd.util.optimizer.schedule_free_fused import FusedScheduleFreeAdamW
    st = FlatParamStore([("a", (3,), "g"), ("b", (2, 5), "g")], torch.float32, torch.device("cpu"))
    return st, FusedScheduleFreeAdamW(st, [{"params": [st.params["a"]]}, {"params": [st.params["b"]], "lr": 5e-4}], **kw)


@pytest.mark.parametrize("kw, word", [(dict(betas=(0.0, 0.999)), "beta1"), (dict(betas=(1.0, 0.999)), "beta1"),
                                      (dict(betas=(0.9, 1.0)), "beta2"), (dict(betas=(0.9, -0.1)), "beta2"),
                                      (dict(eps=-1e-8), "eps"), (dict(lr=-1e-3), "lr"),
                                      (dict(warmup_steps=-1), "warmup_steps")])
def test_bad_hyper_parameters_are_refused_by_name(kw, word):
    with pytest.raises(ValueError, match=word):
        _cpu_optimizer(**kw)


def test_state_dict_has_the_package_layout():
    from onetrainer_amd.util.optimizer import schedule_free_fused as M
    st, opt = _cpu_optimizer(lr=1e-3, warmup_steps=10, foreach=True)
    assert opt.state_dict()["state"] == {}                       # no state before the first step
    opt._z_set = True                                            # as the first step leaves it
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups", "sr_seed"}
    keys = {"k", "train_mode", "weight_sum", "lr_max", "scheduled_lr", "warmup_steps", "r", "weight_lr_power", "betas",
            "eps", "weight_decay", "lr", "foreach"}
    assert set(M.GROUP_KEYS) == keys
    for g in sd["param_groups"]:
        assert set(g) == keys | {"params"}
    g0, g1 = sd["param_groups"]
    assert (g0["k"], g0["train_mode"], g0["weight_sum"], g0["lr_max"], g0["scheduled_lr"]) == (0, False, 0.0, -1.0, 0.0)
    assert g0["lr"] == 1e-3 and g1["lr"] == 5e-4 and g0["warmup_steps"] == 10 and g0["foreach"] is True
    assert sorted(sd["state"]) == [0, 1]
    for i, shape in enumerate([(3,), (2, 5)]):
        assert set(sd["state"][i]) == {"z", "exp_avg_sq"}
        assert all(tuple(t.shape) == shape and t.dtype == torch.float32 for t in sd["state"][i].values())


def test_modes_before_the_first_step_and_step_in_eval_mode():
    st, opt = _cpu_optimizer()
    assert not opt.train_mode
    with pytest.raises(RuntimeError, match="train mode"):
        opt.step()
    opt.train()
    assert opt.train_mode and all(g["train_mode"] for g in opt.param_groups)
    opt.eval()
    assert not opt.train_mode and opt._y_saved is None          # x = y = z: nothing to keep


def test_group_scalars_of_the_optimizer_are_the_oracles():
    from onetrainer_amd.util.optimizer.schedule_free_fused import group_scalars
    mine = dict(SF.new_group(1e-3, warmup_steps=3, r=0.5, weight_lr_power=1.5), train_mode=True)
    theirs = SF.new_group(1e-3, warmup_steps=3, r=0.5, weight_lr_power=1.5)
    for k, lr in enumerate([1e-3, 1e-3, 5e-4, 2e-3, 0.0, 1e-3]):
        mine["lr"] = theirs["lr"] = lr
        a, b = group_scalars(mine), SF.group_scalars(theirs)
        mine["k"] += 1
        assert all(a[key] == b[key] for key in ("lr", "ckp1", "a_y", "bc2")), k
        assert all(mine[key] == theirs[key] for key in ("k", "weight_sum", "lr_max", "scheduled_lr"))
