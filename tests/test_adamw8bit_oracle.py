"""8-bit AdamW on the CPU: the codebooks and the encode rule of tests/_oracle_adamw8bit.py, the oracle against an
unquantised float64 AdamW, and the wiring (options as modules/util/create.py:553-566 resolves them, refusals, state
dict).  bitsandbytes is not in the reference tree: nothing here is compared with it."""
import numpy as np
import pytest
import torch

import _oracle_adamw8bit as A8

F = np.float32


# ---- codebooks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signed", [True, False])
def test_codebook_shape(signed):
    q = A8.dynamic_map(signed)
    assert q.dtype == F and q.shape == (256,) and np.all(np.diff(q) > 0)          # sorted, no duplicates
    assert np.count_nonzero(q == 0) == 1 and q[-1] == 1.0
    if signed:
        # symmetric but for 1: the 127 negatives mirror the 127 positives below 1, 0 sits at code 127
        assert A8.ZERO1 == 127 and np.array_equal(q[:127], -q[128:255][::-1]) and q[0] > -1.0
        assert q[128] == F(0.55e-6) and q[254] == F(1 - 0.45 / 64)
    else:
        assert A8.ZERO2 == 0 and q[0] == 0.0 and q[1] == F((0.1 + 0.45 / 2) * 1e-6) and q[254] == F(1 - 0.45 / 128)


def test_the_package_builds_the_oracles_codebooks():
    from onetrainer_amd.util.optimizer.adamw8bit_fused import dynamic_map
    assert np.array_equal(dynamic_map(True), A8.QMAP1) and np.array_equal(dynamic_map(False), A8.QMAP2)


@pytest.mark.parametrize("qmap, mid", [(A8.QMAP1, A8.MID1), (A8.QMAP2, A8.MID2)])
def test_encode_rule(qmap, mid):
    codes = np.arange(256, dtype=np.uint8)
    assert np.array_equal(A8.encode(mid, qmap), codes)                            # decode(encode(q)) == q
    assert np.array_equal(A8.encode(mid, mid), codes[:255])                       # a midpoint takes the lower code
    assert np.array_equal(A8.encode(mid, np.nextafter(mid, F(2))), codes[1:])     # and the next float the upper one
    lo = -1.0 if qmap[0] < 0 else 0.0
    x = np.random.default_rng(5).uniform(lo, 1.0, 20000).astype(F)
    x = np.concatenate([x, x * F(1e-3), x * F(1e-6), [F(lo), F(1.0), F(0.0)]]).astype(F)
    d = np.abs(qmap[A8.encode(mid, x)].astype(np.float64) - x)
    best = np.abs(qmap.astype(np.float64)[None, :] - x.astype(np.float64)[:, None]).min(axis=1)
    assert np.all(d <= best + 2 * A8.U)                                           # the nearest value (fp32 midpoints)
    assert np.all(d <= A8.half_gap(qmap))


def test_no_operation_is_unpinned():
    """the oracle declares no operation NumPy float32 cannot reproduce, so it flags no element (0 < 0.5 % of any
    tensor) and the GPU test asks for bit equality everywhere"""
    assert A8.UNPINNED == ()


# ---- the oracle is an 8-bit AdamW ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["s4097", "s4099", "s70001"])
def test_oracle_tracks_float64_adamw(name):
    shape = dict(A8.SHAPES)[name]
    n = A8.numel(shape)
    cfg = A8.GROUP_CFG[1]
    beta1, beta2 = cfg["betas"]
    st = A8.new_state(n, True)
    p = np.full(n, F(0.03))
    m64, v64 = np.zeros(n), np.zeros(n)
    e1, e2 = np.zeros(n), np.zeros(n)
    h1, h2 = A8.half_gap(A8.QMAP1), A8.half_gap(A8.QMAP2)
    rep = lambda a: np.repeat(a.astype(np.float64), A8.BLOCK)[:n]
    for k in range(20):
        g = A8.case_grad(name, shape, k).reshape(-1)
        prev1, prev2 = rep(st["absmax1"]), rep(st["absmax2"])
        sc = A8.group_scalars(cfg, k + 1)
        p, m, v = A8.step_8bit(p, g, st, sc)
        m64, v64 = A8.adamw_f64_moments(m64, v64, g, sc)
        e1 = A8.track_bound(e1, prev1, beta1, h1, m)
        e2 = A8.track_bound(e2, prev2, beta2, h2, v)
        assert np.all(np.abs(m - m64) <= e1) and np.all(np.abs(v - v64) <= e2), k
        dm, dv = A8.decode_state(st)
        assert np.all(np.abs(dm - m64) <= e1 + h1 * rep(st["absmax1"])), k
        assert np.all(np.abs(dv - v64) <= e2 + h2 * rep(st["absmax2"])), k
        assert np.array_equal(st["absmax1"], np.abs(np.pad(m, (0, -n % 256))).reshape(-1, 256).max(axis=1))
    # the bound is a fraction of the block's maximum, not a blanket: below 8 % of it after 20 steps
    assert np.all(e1 <= 0.08 * np.maximum(rep(st["absmax1"]), prev1) + 1e-12)
    if name == A8.ZERO_BLOCK[0]:
        b = A8.ZERO_BLOCK[1]
        assert st["absmax1"][b] == 0 and st["absmax2"][b] == 0
        assert np.all(st["code1"][b * 256:(b + 1) * 256] == A8.ZERO1) and np.all(st["code2"][b * 256:(b + 1) * 256] == 0)
    if name == A8.HUGE[0]:
        b = A8.HUGE[1]
        c2 = st["code2"][b * 256:(b + 1) * 256]
        assert c2[A8.HUGE[2]] == 255 and np.all(np.delete(c2, A8.HUGE[2]) < 64)   # the rest: tiny codes


# ---- wiring ----------------------------------------------------------------------------------------------------------
def _cfg():
    from onetrainer_amd.util.config.TrainConfig import TrainConfig
    cfg = TrainConfig.default_values()
    cfg.optimizer.optimizer = "ADAMW_8BIT"
    return cfg


def test_adamw8bit_options_defaults():
    from onetrainer_amd.util.config.TrainConfig import OptimizerConfig
    from onetrainer_amd.util.create import adamw8bit_options
    assert adamw8bit_options(OptimizerConfig(optimizer="ADAMW_8BIT")) == A8.DEFAULTS
    given = dict(beta1=0.8, beta2=0.99, weight_decay=0.1, eps=1e-6, min_8bit_size=1024, percentile_clipping=5,
                 block_wise=False, is_paged=True)
    assert adamw8bit_options(OptimizerConfig(optimizer="ADAMW_8BIT", **given)) == given


def test_train_config_reads_the_8bit_fields():
    from onetrainer_amd.util.config.TrainConfig import OptimizerConfig, TrainConfig
    cfg = TrainConfig().from_dict({"optimizer": {"optimizer": "ADAMW_8BIT", "min_8bit_size": 2048, "block_wise": True,
                                                 "percentile_clipping": 100, "is_paged": False}})
    oc = cfg.optimizer
    assert (oc.optimizer, oc.min_8bit_size, oc.block_wise, oc.percentile_clipping, oc.is_paged) == \
        ("ADAMW_8BIT", 2048, True, 100, False)
    d = OptimizerConfig()
    assert d.min_8bit_size is None and d.block_wise is None and d.percentile_clipping is None and d.is_paged is None


def test_created_optimizer_is_fused_adamw8bit():
    """on the CPU the construction is intercepted: the class is FusedAdamW8bit and the arguments are exactly the
    resolved options (create.py:553-566).  Without the feature ADAMW_8BIT is refused."""
    from onetrainer_amd.util.create import create_optimizer
    from onetrainer_amd.util.optimizer import adamw8bit_fused
    seen = {}

    class Probe(adamw8bit_fused.FusedAdamW8bit):
        def __init__(self, store, groups, **kw):
            seen.update(kw)

    cfg = _cfg()
    cfg.learning_rate = 2e-4
    orig, adamw8bit_fused.FusedAdamW8bit = adamw8bit_fused.FusedAdamW8bit, Probe
    try:
        assert isinstance(create_optimizer(None, [], cfg), orig)
        assert seen == dict(lr=2e-4, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8, min_8bit_size=4096,
                            stochastic_rounding=bool(cfg.optimizer.stochastic_rounding))
        cfg.optimizer.min_8bit_size = 16384
        cfg.optimizer.beta1 = 0.85
        create_optimizer(None, [], cfg)
        assert seen["min_8bit_size"] == 16384 and seen["betas"] == (0.85, 0.999)
    finally:
        adamw8bit_fused.FusedAdamW8bit = orig


@pytest.mark.parametrize("field, value", [("block_wise", False), ("percentile_clipping", 5), ("is_paged", True),
                                          ("fused_back_pass", True)])
def test_create_optimizer_refuses_by_name(field, value):
    from onetrainer_amd.util.create import create_optimizer
    cfg = _cfg()
    setattr(cfg.optimizer, field, value)
    with pytest.raises(NotImplementedError, match=field):
        create_optimizer(None, [{"params": [], "lr": 1e-3}], cfg)


@pytest.mark.parametrize("field, value, word", [("beta1", 1.0, "beta1"), ("beta1", -0.1, "beta1"),
                                                ("beta2", 1.0, "beta2"), ("eps", -1e-8, "eps")])
def test_create_optimizer_refuses_values_out_of_range(field, value, word):
    from onetrainer_amd.util.create import create_optimizer
    cfg = _cfg()
    setattr(cfg.optimizer, field, value)
    with pytest.raises(ValueError, match=word):
        create_optimizer(None, [{"params": [], "lr": 1e-3}], cfg)


def test_create_optimizer_refuses_a_negative_lr():
    from onetrainer_amd.util.create import create_optimizer
    cfg = _cfg()
    with pytest.raises(ValueError, match="lr"):
        create_optimizer(None, [{"params": [], "lr": -1e-3}], cfg)
    cfg.learning_rate = -1.0
    with pytest.raises(ValueError, match="lr"):
        create_optimizer(None, [{"params": []}], cfg)


def test_step_parameter_is_refused():
    from onetrainer_amd.util.optimizer.adamw8bit_fused import FusedAdamW8bit
    with pytest.raises(NotImplementedError, match="step_parameter"):
        FusedAdamW8bit.step_parameter(None, None, None, 0)


def test_lion_is_still_refused_with_the_old_words():
    from onetrainer_amd.util.create import create_optimizer
    cfg = _cfg()
    cfg.optimizer.optimizer = "LION"
    with pytest.raises(NotImplementedError) as e:
        create_optimizer(None, [], cfg)
    msg = str(e.value)
    assert "LION" in msg and "ADAMW, ADAFACTOR and CAME" in msg and "PRODIGY" in msg and "SCHEDULE_FREE_ADAMW" in msg
    assert "ADAMW_8BIT" in msg


def test_group_scalars_of_the_optimizer_are_the_oracles():
    from onetrainer_amd.util.optimizer.adamw8bit_fused import group_scalars
    for cfg in A8.GROUP_CFG:
        for step in (1, 2, 7, 1000):
            assert group_scalars(cfg, step) == A8.group_scalars(cfg, step)


# ---- state dict ------------------------------------------------------------------------------------------------------
def _cpu_optimizer(**kw):
    from onetrainer_amd.module.param_store import FlatParamStore
    from onetrainer_amd.util.optimizer.adamw8bit_fused import FusedAdamW8bit
    st = FlatParamStore([("a", (3,), "g"), ("b", (2, 5), "g"), ("c", (5, 1000), "h"), ("d", (4097,), "h")],
                        torch.float32, torch.device("cpu"))
    groups = [{"params": [st.params["a"], st.params["b"]]}, {"params": [st.params["c"], st.params["d"]], "lr": 5e-4}]
    return st, FusedAdamW8bit(st, groups, **kw)


def test_segment_table_follows_the_slots():
    from onetrainer_amd import _lib
    st, opt = _cpu_optimizer()
    t = opt._table_host
    assert opt._n_segs == 4 and opt._table.numel() == 4 * _lib.C.sizeof(_lib.A8Seg)
    assert [(s.begin, s.end) for s in t] == [(st.slots[n].offset, st.slots[n].offset + st.slots[n].numel) for n in "abcd"]
    assert [s.is8bit for s in t] == [0, 0, 1, 1] and [s.group for s in t] == [0, 0, 1, 1]
    assert [s.blk0 for s in t] == [0, 1, 2, 22] and [s.state_off for s in t] == [0, 8, 0, 20]
    assert opt.absmax1.numel() == 20 + 17 and opt.m32.numel() == 8 + 16
    assert opt.code1.numel() == st.numel and bool((opt.code1 == 127).all()) and not opt.code2.any()
    _, small = _cpu_optimizer(min_8bit_size=10)
    assert [s.is8bit for s in small._table_host] == [0, 1, 1, 1]


def test_state_dict_layout_and_round_trip():
    st, opt = _cpu_optimizer(lr=1e-3, seed=5)
    assert opt.state_dict()["state"] == {}                       # no state before the first step
    g = torch.Generator().manual_seed(3)
    opt.steps = [3, 4]                                           # as three and four steps leave it
    opt.code1.copy_(torch.randint(0, 256, opt.code1.shape, generator=g, dtype=torch.uint8))
    opt.code2.copy_(torch.randint(0, 256, opt.code2.shape, generator=g, dtype=torch.uint8))
    for t in (opt.absmax1, opt.absmax2, opt.m32, opt.v32):
        t.copy_(torch.rand(t.shape, generator=g))
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups", "sr_seed"} and sd["sr_seed"] == 5
    assert sorted(sd["state"]) == [0, 1, 2, 3]
    for i, shape in enumerate([(3,), (2, 5)]):
        s = sd["state"][i]
        assert set(s) == {"step", "state1", "state2"} and float(s["step"]) == 3.0
        assert all(tuple(s[k].shape) == shape and s[k].dtype == torch.float32 for k in ("state1", "state2"))
    for i, (shape, nblk) in enumerate([((5, 1000), 20), ((4097,), 17)], start=2):
        s = sd["state"][i]
        assert set(s) == {"step", "state1", "state2", "absmax1", "absmax2", "qmap1", "qmap2"} and float(s["step"]) == 4.0
        assert all(tuple(s[k].shape) == shape and s[k].dtype == torch.uint8 for k in ("state1", "state2"))
        assert all(tuple(s[k].shape) == (nblk,) and s[k].dtype == torch.float32 for k in ("absmax1", "absmax2"))
        assert np.array_equal(s["qmap1"].numpy(), A8.QMAP1) and np.array_equal(s["qmap2"].numpy(), A8.QMAP2)
    assert sd["param_groups"][0]["lr"] == 1e-3 and sd["param_groups"][1]["lr"] == 5e-4
    assert all(set(g) == {"lr", "betas", "eps", "weight_decay", "params"} for g in sd["param_groups"])

    st2, fresh = _cpu_optimizer(lr=7.0, seed=99)
    del sd["state"][1]                                           # a parameter without saved state starts fresh
    fresh.load_state_dict(sd)
    assert fresh.seed == 5 and fresh.steps == [3, 4] and fresh.param_groups[0]["lr"] == 1e-3
    for name in "acd":
        for k, v in opt._views(name).items():
            assert torch.equal(v, fresh._views(name)[k]), (name, k)
    assert not fresh._views("b")["state1"].any() and not fresh._views("b")["state2"].any()
    # the store's padding keeps the codes of 0
    mask = torch.ones(st2.numel, dtype=torch.bool)
    for n in "abcd":
        mask[st2.slots[n].offset:st2.slots[n].offset + st2.slots[n].numel] = False
    assert mask.any() and bool((fresh.code1[mask] == 127).all()) and not fresh.code2[mask].any()
    bad = opt.state_dict()
    bad["state"][2]["qmap1"] = bad["state"][2]["qmap1"] * 2
    with pytest.raises(ValueError, match="qmap1"):
        fresh.load_state_dict(bad)


@pytest.mark.parametrize("kw, word", [(dict(betas=(1.0, 0.999)), "beta1"), (dict(betas=(0.9, 1.0)), "beta2"),
                                      (dict(eps=-1e-8), "eps"), (dict(lr=-1e-3), "lr"),
                                      (dict(weight_decay=-0.1), "weight_decay"), (dict(min_8bit_size=0), "min_8bit_size")])
def test_bad_hyper_parameters_are_refused_by_name(kw, word):
    with pytest.raises(ValueError, match=word):
        _cpu_optimizer(**kw)


def test_table_check_on_the_host():
    """the library's table check is host code: it needs no device"""
    from onetrainer_amd import _lib
    from onetrainer_amd import kernels as K
    st, opt = _cpu_optimizer()
    n_abs, n_f32 = opt.absmax1.numel(), opt.m32.numel()
    args = lambda t: (t, opt._n_segs, st.numel, n_abs, n_f32, 2)
    assert K.adamw8bit_check(*args(opt._table_host)) == _lib.OTAMD_OK

    def broken(**kw):
        t = (_lib.A8Seg * opt._n_segs).from_buffer_copy(bytes(opt._table_host))
        for k, (i, v) in kw.items():
            setattr(t[i], k, v)
        return t
    for kw in (dict(blk0=(3, 23)), dict(blk0=(0, 1)), dict(end=(3, st.numel + 1)), dict(begin=(1, 4)),
               dict(state_off=(3, 21)), dict(state_off=(2, 1), is8bit=(2, 0)), dict(state_off=(1, 4)),
               dict(group=(0, 2)), dict(begin=(2, 8)), dict(end=(0, 0))):
        assert K.adamw8bit_check(*args(broken(**kw))) == _lib.OTAMD_EINVAL, kw
    assert K.adamw8bit_check(opt._table_host, opt._n_segs, st.numel, n_abs - 1, n_f32, 2) == _lib.OTAMD_EINVAL
    assert K.adamw8bit_check(opt._table_host, opt._n_segs, st.numel, n_abs, n_f32 - 8, 2) == _lib.OTAMD_EINVAL
    assert K.adamw8bit_check(opt._table_host, opt._n_segs, st.numel, n_abs, n_f32, 1) == _lib.OTAMD_EINVAL
