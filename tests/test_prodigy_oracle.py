"""The Prodigy restatement tests/_oracle_prodigy.py on the CPU: cases worked by hand, the convex bound on d, the
configuration defaults and the refusals.  prodigyopt, which the reference imports (modules/util/create.py:863-881), is
not in the reference tree: nothing here is compared with it."""
import math

import numpy as np
import pytest

import _oracle_adafactor as AF
import _oracle_prodigy as PR
from oracle import adamw as OA

F = np.float32
# arithmetic a hand can follow: beta1 = 1/2, beta2 = 3/4, beta3 = 1/2, eps = 1/2, d0 = 1, lr = 1, so at d = 1:
# m = g / 2, v = g^2 / 4, sqrt(v) + d eps = (|g| + 1) / 2, update = g / (|g| + 1)
HAND = dict(beta1=0.5, beta2=0.75, beta3=0.5, eps=0.5, d0=1.0)
P = [4.0, 8.0, -2.0]
G = [1.0, -1.0, 3.0]


def one(p, g, st, sc, lr=1.0, **kw):
    xs, info = PR.prodigy_step([np.array(p, F)], [np.array(g, F)], [st], sc, lr, **dict(HAND, **kw))
    return xs[0], info


def close(a, b):
    return np.allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=1e-6, atol=0)


def test_two_steps_by_hand_d_equals_d0_branch():
    """d_coef = 4.  Step 1: p0 = p, num = 0, m = g / 2 = (.5, -.5, 1.5), v = g^2 / 4 = (.25, .25, 2.25), s = g,
    den = 5, d_numerator = 0, d_hat = 0, d = max(1, 0) = 1, update g / (|g| + 1) = (.5, -.5, .75), p = (3.5, 8.5, -2.75).
    Step 2, same g: p0 - p = (.5, -.5, .75), num = .5 + .5 + 2.25 = 3.25, m = (.75, -.75, 2.25), v = 3/4 v + g^2 / 4 =
    (.4375, .4375, 3.9375), s = s / 2 + g = (1.5, -1.5, 4.5), den = 7.5, d_numerator = 3.25, d_hat = 4 * 3.25 / 7.5 =
    26/15; d == d0 so d = max(1, 26/15) = 26/15 = d_max; update = 1 * m / (sqrt(v) + 26/15 / 2) with the OLD dlr = 1."""
    st, sc = PR.new_state((3,)), PR.new_scalars(1.0)
    x, info = one(P, G, st, sc, d_coef=4.0)
    assert np.array_equal(x, F([3.5, 8.5, -2.75])) and (info["num"], info["den"]) == (0.0, 5.0)
    assert np.array_equal(st["m"], F([.5, -.5, 1.5])) and np.array_equal(st["v"], F([.25, .25, 2.25]))
    assert np.array_equal(st["s"], F(G)) and np.array_equal(st["p0"], F(P))
    assert (sc["d"], sc["d_max"], sc["d_numerator"], sc["d_hat"], sc["k"]) == (1.0, 1.0, 0.0, 0.0, 1)
    x, info = one(x, G, st, sc, d_coef=4.0)
    assert (info["num"], info["den"], info["dlr"]) == (3.25, 7.5, 1.0)
    assert np.array_equal(st["m"], F([.75, -.75, 2.25])) and np.array_equal(st["v"], F([.4375, .4375, 3.9375]))
    assert np.array_equal(st["s"], F([1.5, -1.5, 4.5]))
    assert sc["d_numerator"] == 3.25 and sc["k"] == 2
    assert math.isclose(sc["d_hat"], 26 / 15, rel_tol=1e-15) and sc["d"] == sc["d_max"] == sc["d_hat"]
    want = [3.5 - .75 / (math.sqrt(.4375) + 13 / 15), 8.5 + .75 / (math.sqrt(.4375) + 13 / 15),
            -2.75 - 2.25 / (math.sqrt(3.9375) + 13 / 15)]
    assert close(x, want)


def _loaded():
    """a run in progress: d = 2 (d0 = 1), p0 = p + (1, -1, 1), states zero, one step done"""
    st, sc = PR.new_state((3,)), PR.new_scalars(1.0)
    st["p0"] = F([5.0, 7.0, -1.0])
    sc.update(d=2.0, d_max=2.0, k=1)
    return st, sc


def test_growth_rate_cap_by_hand():
    """lr = 1/2, d = 2: dlr = 1; p0 - p = (1, -1, 1), num = 1 + 1 + 3 = 5; a = (d / d0) dlr = 2, s = 2 g, den = 10;
    d_numerator = 2 * 1 * 5 = 10, d_hat = 8 * 10 / 10 = 8 (d_coef = 8), d != d0, d_max = 8, d = min(8, 2 * 1.5) = 3;
    m = d g / 2 = g, v = d^2 g^2 / 4 = g^2, denominator |g| + 3 / 2 = (2.5, 2.5, 4.5), p -= 1 * g / that"""
    st, sc = _loaded()
    x, info = one(P, G, st, sc, lr=0.5, d_coef=8.0, growth_rate=1.5)
    assert (info["dlr"], info["num"], info["den"]) == (1.0, 5.0, 10.0)
    assert (sc["d_numerator"], sc["d_hat"], sc["d_max"], sc["d"], sc["k"]) == (10.0, 8.0, 8.0, 3.0, 2)
    assert np.array_equal(st["m"], F(G)) and np.array_equal(st["v"], F([1, 1, 9])) and np.array_equal(st["s"], F([2, -2, 6]))
    assert close(x, [4 - 1 / 2.5, 8 + 1 / 2.5, -2 - 3 / 4.5])
    st, sc = _loaded()   # without the cap d follows d_max
    one(P, G, st, sc, lr=0.5, d_coef=8.0)
    assert sc["d"] == 8.0


def test_safeguard_warmup_by_hand():
    """as above with a = (d / d0) d = 4: s = 4 g, den = 20; the numerator keeps dlr: 10; d_hat = 8 * 10 / 20 = 4"""
    st, sc = _loaded()
    x, info = one(P, G, st, sc, lr=0.5, d_coef=8.0, growth_rate=1.5, safeguard_warmup=True)
    assert np.array_equal(st["s"], F([4, -4, 12])) and info["den"] == 20.0
    assert (sc["d_numerator"], sc["d_hat"], sc["d_max"], sc["d"]) == (10.0, 4.0, 4.0, 3.0)
    assert close(x, [4 - 1 / 2.5, 8 + 1 / 2.5, -2 - 3 / 4.5])


def test_bias_correction_by_hand():
    """k = 1: bc = sqrt(1 - (3/4)^2) / (1 - (1/2)^2) = sqrt(7/16) / (3/4) = sqrt(7) / 3; d = 2, lr = 1/2: dlr = bc;
    s = (d / d0) dlr g = 2 bc g, den = 10 bc, d_numerator = 2 bc 5 = 10 bc, d_hat = 1 (d_coef = 1)"""
    bc = math.sqrt(7) / 3
    st, sc = _loaded()
    x, info = one(P, G, st, sc, lr=0.5, use_bias_correction=True)
    assert math.isclose(info["dlr"], bc, rel_tol=1e-15)
    assert close(st["s"], [2 * bc, -2 * bc, 6 * bc]) and math.isclose(info["den"], 10 * bc, rel_tol=1e-6)
    assert math.isclose(sc["d_numerator"], 10 * bc, rel_tol=1e-12) and math.isclose(sc["d_hat"], 1.0, rel_tol=1e-6)
    assert sc["d_max"] == 2.0 and sc["d"] == 2.0   # d_hat below d_max: d = min(2, inf)
    assert close(x, [4 - bc * 1 / 2, 8 + bc * 1 / 2, -2 - bc * 3 / 4])   # denominators |g| + d eps = (2, 2, 4)
    st, sc = _loaded()   # without it bc = 1
    assert one(P, G, st, sc, lr=0.5)[1]["dlr"] == 1.0


def test_weight_decay_by_hand():
    """step 1 of the first case, weight_decay = 1/4.  Decoupled: p <- p - p dlr / 4 = (3, 6, -1.5), then the update
    (.5, -.5, .75): (2.5, 6.5, -2.25), states as without decay.  Coupled: g <- g + p / 4 = (2, 1, 2.5), m = g / 2,
    v = g^2 / 4 = (1, .25, 1.5625), s = g, den = 5.5, denominators (1.5, 1, 1.75), p = (4 - 2/3, 8 - .5, -2 - 5/7)"""
    st, sc = PR.new_state((3,)), PR.new_scalars(1.0)
    x, _ = one(P, G, st, sc, weight_decay=0.25)
    assert np.array_equal(x, F([2.5, 6.5, -2.25])) and np.array_equal(st["m"], F([.5, -.5, 1.5]))
    st, sc = PR.new_state((3,)), PR.new_scalars(1.0)
    x, info = one(P, G, st, sc, weight_decay=0.25, decouple=False)
    assert np.array_equal(st["m"], F([1, .5, 1.25])) and np.array_equal(st["v"], F([1, .25, 1.5625]))
    assert np.array_equal(st["s"], F([2, 1, 2.5])) and info["den"] == 5.5
    assert close(x, [4 - 2 / 3, 7.5, -2 - 5 / 7])


def test_beta1_zero_by_hand():
    """step 1 of the first case with beta1 = 0: d g = g stands for m, the update is g / ((|g| + 1) / 2) =
    (1, -1, 1.5), and m is never written"""
    st, sc = PR.new_state((3,)), PR.new_scalars(1.0)
    x, _ = one(P, G, st, sc, beta1=0.0)
    assert np.array_equal(x, F([3.0, 9.0, -3.5])) and not st["m"].any()
    assert np.array_equal(st["v"], F([.25, .25, 2.25]))


def test_lr_zero_is_a_no_op():
    st, sc = PR.new_state((3,)), PR.new_scalars(1.0)
    x, info = one(P, G, st, sc, lr=0.0)
    assert info["noop"] and np.array_equal(x, F(P)) and st["p0"] is None
    assert not (st["m"].any() or st["v"].any() or st["s"].any()) and sc == PR.new_scalars(1.0)


def test_zero_denominator_stops_after_the_states():
    """g = 0 and s = 0: den = 0.  m = (1, 1, 1) is still halved (step 6 stays); no update, d and k unchanged"""
    st, sc = PR.new_state((3,)), PR.new_scalars(1.0)
    st["m"] = F([1, 1, 1])
    x, info = one(P, [0, 0, 0], st, sc)
    assert info["skipped"] and info["den"] == 0.0 and np.array_equal(x, F(P))
    assert np.array_equal(st["m"], F([.5, .5, .5])) and np.array_equal(st["p0"], F(P))
    assert (sc["d"], sc["d_max"], sc["k"], sc["d_denom"]) == (1.0, 1.0, 0, 0.0)


CONVEX_STEPS = 20


def test_d_stays_below_the_distance_on_a_convex_problem():
    """f(x) = |x - x*|^2 / 2, g = x - x*.  <g_i, x0 - x_i> <= <g_i, x0 - x*> by convexity, so d_numerator <=
    |s|_1 |x0 - x*|_inf and, with d_coef = 1, d_hat and d never exceed |x0 - x*|_inf.  CONVEX_STEPS: the oracle run on
    the CPU with these inputs first holds d >= 1e3 d0 after 9 steps (growth_rate is unbounded) and d settles at 0.327
    against a distance of 2.43 once x has reached x*; 20 steps cover the growth and the plateau."""
    rng = np.random.default_rng(5)
    target = rng.standard_normal(64).astype(F)
    x = np.zeros(64, F)
    dist = float(np.abs(x - target).max())
    st, sc = PR.new_state((64,)), PR.new_scalars()
    for _ in range(CONVEX_STEPS):
        xs, _ = PR.prodigy_step([x], [x - target], [st], sc, 1.0)
        x = xs[0]
        assert sc["d"] <= dist and sc["d_hat"] <= dist
    assert sc["d"] >= 1e3 * PR.DEFAULTS["d0"] and sc["k"] == CONVEX_STEPS


def test_gpu_cases_are_not_near_bf16_rounding_ties():
    """the bf16 comparison of tests/test_prodigy_gpu.py allows 1e-3 of the elements one bf16 ulp away.  For its inputs
    (round-to-nearest store, free run of the oracle) the share of elements whose value before the rounding lies within
    the oracle's own one-step bound of a tie is below a quarter of that: the inputs are not adversarial."""
    for cfg in PR.GPU_CASES.values():
        params = [AF.param0(n, s) for n, s in AF.SHAPES]
        states, sc = [PR.new_state(s) for _, s in AF.SHAPES], PR.new_scalars(cfg["d0"])
        near = total = 0
        for k in range(PR.GPU_STEPS):
            grads = [PR.case_grad(n, s, k) for n, s in AF.SHAPES]
            xs, info = PR.prodigy_step(params, grads, states, sc, 1.0, **cfg)
            for x, tol in zip(xs, info["tol_p"]):
                lo = OA.bf16_to_f32(OA.f32_to_bf16_bits(x)).astype(np.float64)
                ulp = np.ldexp(1.0, np.frexp(np.abs(lo))[1] - 8)              # bf16 spacing at the rounded value
                tie = ulp / 2 - np.abs(x.astype(np.float64) - lo)              # distance to the nearer tie
                near += int((tie <= tol).sum())
                total += x.size
            params = [OA.rbf(x) for x in xs]
            assert all(np.all(np.sign(p) == np.sign(q)) for p, q in zip(params, xs))   # nothing crosses zero
        assert sc["d"] > cfg["d0"] and near <= 0.25e-3 * total, (near, total, sc)


DEFAULT_TABLE = dict(beta1=0.9, beta2=0.999, beta3=None, eps=1e-8, weight_decay=0, decouple=True,
                     use_bias_correction=False, safeguard_warmup=False, d0=1e-6, d_coef=1.0, growth_rate=float("inf"),
                     fsdp_in_use=False, slice_p=1)


def test_prodigy_options_defaults():
    from onetrainer_amd.util.config.TrainConfig import OptimizerConfig
    from onetrainer_amd.util.create import prodigy_options
    assert prodigy_options(OptimizerConfig(optimizer="PRODIGY")) == DEFAULT_TABLE
    assert {k: PR.DEFAULTS[k] for k in PR.DEFAULTS} == {k: DEFAULT_TABLE[k] for k in PR.DEFAULTS}
    given = dict(beta1=0.8, beta2=0.99, beta3=0.9, eps=1e-6, weight_decay=0.1, decouple=False, use_bias_correction=True,
                 safeguard_warmup=True, d0=1e-5, d_coef=2.0, growth_rate=1.02, fsdp_in_use=True, slice_p=2)
    assert prodigy_options(OptimizerConfig(optimizer="PRODIGY", **given)) == given


def test_train_config_reads_the_prodigy_fields():
    from onetrainer_amd.util.config.TrainConfig import TrainConfig
    cfg = TrainConfig().from_dict({"optimizer": {"optimizer": "PRODIGY", "d_coef": 0.5, "safeguard_warmup": True,
                                                 "slice_p": 1, "growth_rate": 1.02}})
    oc = cfg.optimizer
    assert (oc.optimizer, oc.d_coef, oc.safeguard_warmup, oc.slice_p, oc.growth_rate) == ("PRODIGY", 0.5, True, 1, 1.02)
    assert oc.decouple is None and oc.use_bias_correction is None and oc.d0 is None and oc.fsdp_in_use is None


def _cfg():
    from onetrainer_amd.util.config.TrainConfig import TrainConfig
    cfg = TrainConfig.default_values()
    cfg.optimizer.optimizer = "PRODIGY"
    cfg.learning_rate = 1.0
    return cfg


@pytest.mark.parametrize("field, value, word", [("slice_p", 2, "slice_p"), ("fsdp_in_use", True, "fsdp_in_use"),
                                                ("fused_back_pass", True, "fused_back_pass")])
def test_create_optimizer_refuses_by_name(field, value, word):
    from onetrainer_amd.util.create import create_optimizer
    cfg = _cfg()
    setattr(cfg.optimizer, field, value)
    with pytest.raises(NotImplementedError, match=word):
        create_optimizer(None, [{"params": [], "lr": 1.0}], cfg)


def test_create_optimizer_refuses_different_learning_rates():
    from onetrainer_amd.util.create import create_optimizer
    with pytest.raises(NotImplementedError, match="learning_rate"):
        create_optimizer(None, [{"params": [], "lr": 1.0}, {"params": [], "lr": 0.5}], _cfg())


def test_step_parameter_is_refused():
    from onetrainer_amd.util.optimizer.prodigy_fused import FusedProdigy
    with pytest.raises(NotImplementedError, match="step_parameter"):
        FusedProdigy.step_parameter(None, None, None, 0)


def test_created_optimizer_is_fused_prodigy():
    """on the CPU the construction is intercepted: the arguments are the resolved options and the class is
    FusedProdigy; the last refusal names PRODIGY among what is on the hot path"""
    from onetrainer_amd.util.create import create_optimizer
    from onetrainer_amd.util.optimizer import prodigy_fused
    seen = {}

    class Probe(prodigy_fused.FusedProdigy):
        def __init__(self, store, groups, **kw):
            seen.update(kw)

    cfg = _cfg()
    orig, prodigy_fused.FusedProdigy = prodigy_fused.FusedProdigy, Probe
    try:
        assert isinstance(create_optimizer(None, [], cfg), orig)
    finally:
        prodigy_fused.FusedProdigy = orig
    assert seen == dict(lr=1.0, betas=(0.9, 0.999), beta3=None, eps=1e-8, weight_decay=0, decouple=True,
                        use_bias_correction=False, safeguard_warmup=False, d0=1e-6, d_coef=1.0,
                        growth_rate=float("inf"), stochastic_rounding=bool(cfg.optimizer.stochastic_rounding))
    cfg.optimizer.optimizer = "LION"
    with pytest.raises(NotImplementedError, match="PRODIGY"):
        create_optimizer(None, [], cfg)


def test_report_learning_rates_multiplies_by_d():
    from types import SimpleNamespace

    from onetrainer_amd.modelSetup.BaseStableDiffusionXLSetup import report_learning_rates
    from onetrainer_amd.util.NamedParameterGroup import NamedParameterGroup, NamedParameterGroupCollection
    pgc = NamedParameterGroupCollection()
    for name in ("unet", "te/1"):
        pgc.add_group(NamedParameterGroup(name, [], 1.0, display_name=name))
    got = []
    tb = SimpleNamespace(add_scalar=lambda tag, v, step: got.append((tag, v)))
    model = SimpleNamespace(parameters=pgc, train_progress=SimpleNamespace(global_step=1),
                            optimizer=SimpleNamespace(param_groups=[{"d": 0.25}, {"d": 0.25}]))
    report_learning_rates(model, SimpleNamespace(get_last_lr=lambda: [1.0, 0.5]), tb)
    assert got == [("lr/unet", 0.25), ("lr/te", 0.125)]
    model.optimizer = SimpleNamespace(param_groups=[{}, {}])   # an optimizer without d: the identity
    got.clear()
    report_learning_rates(model, SimpleNamespace(get_last_lr=lambda: [1.0, 0.5]), tb)
    assert got == [("lr/unet", 1.0), ("lr/te", 0.5)]
