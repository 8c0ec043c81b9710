"""The NumPy restatement of CAME (tests/_oracle_came.py) against the reference's own run recorded in
tests/golden/came_steps.npz (tests/golden/make_came_golden.py), that its bounds have teeth, the resolution of the
configuration fields, the refusals and the fold table.  CPU only.

Bounds are derived, not tuned: tests/_oracle_came.py states them and returns them beside the result.
  bf16:  equal bits or one bf16 ulp apart, none further, at most 1e-3 of all elements apart
"""
from pathlib import Path

import numpy as np
import pytest

import _oracle_adafactor as AF
import _oracle_came as CM
from oracle import adamw as OA

GOLD = np.load(Path(__file__).resolve().parent / "golden" / "came_steps.npz")


def violations(cname, wrong=None, names=None):
    """the fp32 run of one configuration against the golden: [(tensor, step, what)] for every bound missed"""
    cfg, bad = CM.CONFIGS[cname], []
    for n, s in AF.SHAPES:
        if names is not None and n not in names:
            continue
        p, st = AF.param0(n, s), CM.new_state(s)
        tol_p = np.zeros(s, np.float64)
        for k in range(AF.STEPS):
            p, info = CM.came_step(p, CM.grad(cname, n, s, k), st, wrong=wrong, **cfg)
            gold = lambda key: GOLD[f"{cname}/state/{k}/{n}/{key}"]   # noqa: E731
            for key, gkey in CM.SQ_KEYS.items():
                if key in st:
                    ref = gold(gkey)
                    if not np.all(np.abs(CM.sample(st[key]).astype(np.float64) - ref) <= CM.sq_bound(s, key, k + 1, ref)):
                        bad.append((n, k, gkey))
            for key, gkey in CM.RES_KEYS.items():
                if key in st:
                    if not np.all(np.abs(CM.sample(st[key]).astype(np.float64) - gold(gkey)) <= CM.sample(st["tol"][key])):
                        bad.append((n, k, gkey))
            if not np.all(np.abs(CM.sample(st["m"]).astype(np.float64) - gold("exp_avg")) <= CM.sample(info["tol_m"])):
                bad.append((n, k, "exp_avg"))
            tol_p = tol_p + info["tol_p"]   # the run carries its own parameters on: the bounds add up
            if not np.all(np.abs(CM.sample(p).astype(np.float64) - GOLD[f"{cname}/f32/{k}/{n}/p"]) <= CM.sample(tol_p)):
                bad.append((n, k, "p"))
    return bad


# ---- (a) the oracle matches the reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("cname", list(CM.CONFIGS))
def test_oracle_matches_reference_fp32(cname):
    assert violations(cname) == []


def test_clip_threshold_is_active_where_the_cases_say():
    for cname, active in (("clip", True), ("default", True), ("noclip", False)):
        cfg = CM.CONFIGS[cname]
        for n, s in AF.SHAPES[:-1]:   # not the all-zero gradient
            st = CM.new_state(s)
            for k in range(AF.STEPS):
                _, info = CM.came_step(AF.param0(n, s), CM.grad(cname, n, s, k), st, **cfg)
                assert (info["rms_u"] > cfg["clip_threshold"]) == active, (cname, n, k, info["rms_u"])


def test_oracle_matches_reference_bf16():
    apart = total = 0
    for cname, cfg in CM.CONFIGS.items():
        for n, s in AF.SHAPES:
            p, st = AF.param0(n, s), CM.new_state(s)
            for k in range(AF.STEPS):
                x, _ = CM.came_step(p, CM.grad(cname, n, s, k), st, bf16=True, **cfg)
                bits = OA.f32_to_bf16_bits(x)
                p = OA.bf16_to_f32(bits)
                d = AF.bf16_ulps(CM.sample(bits), GOLD[f"{cname}/bf16/{k}/{n}/p"])
                assert d.max() <= 1, (cname, n, k, int(d.max()))
                apart += int((d != 0).sum())
                total += d.size
    assert apart <= 1e-3 * total, (apart, total)


def test_fp32_summation_order_moves_few_bf16_results():
    """the 1e-3 cap on the CPU: the oracle with fp32 (pairwise) sums against the oracle with float64 sums"""
    apart = total = 0
    for cname in ("decay", "clip", "betas"):
        cfg = CM.CONFIGS[cname]
        for n, s in AF.SHAPES:
            p = AF.param0(n, s)
            st = {dt: CM.new_state(s) for dt in (np.float32, np.float64)}
            for k in range(AF.STEPS):
                bits = {dt: OA.f32_to_bf16_bits(CM.came_step(p, CM.grad(cname, n, s, k), st[dt], bf16=True,
                                                             sum_dtype=dt, **cfg)[0]) for dt in st}
                p = OA.bf16_to_f32(bits[np.float64])
                d = AF.bf16_ulps(bits[np.float32], bits[np.float64])
                assert d.max() <= 1
                apart += int((d != 0).sum())
                total += d.size
    assert apart <= 1e-3 * total, (apart, total)


def test_zero_gradient_instability_is_exactly_eps2():
    s = dict(AF.SHAPES)["zero"]
    st = CM.new_state(s)
    CM.came_step(AF.param0("zero", s), np.zeros(s, np.float32), st, **CM.CONFIGS["default"])
    want = OA.fma32(np.float32(1e-16), np.float32(1.0 - 0.9999), np.float32(0.0))   # the EMA of a mean of eps2
    assert np.all(st["res_row"] == want) and np.all(st["res_col"] == want) and not np.any(st["m"])


# ---- (b) the bounds have teeth --------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrong, names", [("old_m", ("m64x70", "conv3", "m2x4100")),
                                          ("beta3", ("m64x70", "conv3", "m2x4100")),
                                          ("eps2", ("zero",))])
def test_a_wrong_restatement_violates_a_bound(wrong, names):
    assert violations("default", names=names) == []
    bad = violations("default", wrong=wrong, names=names)
    assert bad and {b[0] for b in bad} == set(names), bad


# ---- (c) options and configuration ----------------------------------------------------------------------------------
def test_config_none_resolves_as_the_reference():
    """create.py:944-949: None falls back to eps 1e-30, eps2 1e-16, betas 0.9 / 0.999 / 0.9999, weight_decay 0; an
    explicit value wins"""
    from onetrainer_amd.util.config.TrainConfig import OptimizerConfig
    from onetrainer_amd.util.create import came_options
    assert came_options(OptimizerConfig(optimizer="CAME")) == dict(eps=1e-30, eps2=1e-16, beta1=0.9, beta2=0.999,
                                                                   beta3=0.9999, weight_decay=0)
    o = came_options(OptimizerConfig(optimizer="CAME", eps=1e-20, eps2=1e-12, beta1=0.8, beta2=0.99, beta3=0.999,
                                     weight_decay=0.1))
    assert o == dict(eps=1e-20, eps2=1e-12, beta1=0.8, beta2=0.99, beta3=0.999, weight_decay=0.1)


def test_create_optimizer_builds_came_and_refuses_by_name():
    from onetrainer_amd.util.config.TrainConfig import TrainConfig
    from onetrainer_amd.util.create import create_optimizer
    cfg = TrainConfig.default_values()
    cfg.optimizer.optimizer = "CAME"
    cfg.learning_rate = 0.0
    with pytest.raises(ValueError, match="lr"):
        create_optimizer(None, [], cfg)
    cfg.learning_rate = None
    with pytest.raises(ValueError, match="lr"):
        create_optimizer(None, [], cfg)
    cfg.learning_rate = 1e-4
    for name in ("beta1", "beta2", "beta3"):
        setattr(cfg.optimizer, name, 1.5)
        with pytest.raises(ValueError, match="betas"):
            create_optimizer(None, [], cfg)
        setattr(cfg.optimizer, name, None)
    cfg.optimizer.optimizer = "LION"
    with pytest.raises(NotImplementedError, match="ADAMW, ADAFACTOR and CAME"):
        create_optimizer(None, [], cfg)


def test_created_optimizer_is_fused_came():
    """on the CPU the construction goes as far as torch's Optimizer, which refuses the empty parameter list: the
    arguments passed the CAME checks and the class is FusedCAME"""
    from onetrainer_amd.util.config.TrainConfig import TrainConfig
    from onetrainer_amd.util.create import create_optimizer
    from onetrainer_amd.util.optimizer import came_fused
    cfg = TrainConfig.default_values()
    cfg.optimizer.optimizer = "CAME"
    seen = {}

    class Probe(came_fused.FusedCAME):
        def __init__(self, store, groups, **kw):
            seen.update(kw)

    orig, came_fused.FusedCAME = came_fused.FusedCAME, Probe
    try:
        assert isinstance(create_optimizer(None, [], cfg), orig)
    finally:
        came_fused.FusedCAME = orig
    assert seen == dict(lr=cfg.learning_rate, eps=(1e-30, 1e-16), betas=(0.9, 0.999, 0.9999), weight_decay=0,
                        stochastic_rounding=bool(cfg.optimizer.stochastic_rounding))


def test_train_config_round_trips_beta3(tmp_path):
    import json

    from onetrainer_amd.util.config.TrainConfig import TrainConfig
    cfg = TrainConfig.default_values()
    assert cfg.optimizer.beta3 is None
    cfg.optimizer.optimizer, cfg.optimizer.beta3 = "CAME", 0.999
    path = tmp_path / "config.json"
    path.write_text(json.dumps(cfg.to_settings_dict()))
    back = TrainConfig.load(str(path))
    assert back.optimizer.optimizer == "CAME" and back.optimizer.beta3 == 0.999
    assert json.loads(json.dumps(back.to_settings_dict()))["optimizer"]["beta3"] == 0.999


# ---- (d) the fold table ---------------------------------------------------------------------------------------------
def _tables():
    from onetrainer_amd.util.optimizer.adafactor_fused import adafactor_tables
    entries, off = [], 0
    for _, s in AF.SHAPES:
        entries.append((off, s, 0))
        off += (int(np.prod(s)) + 7) // 8 * 8
    tensors, _, nt, *_ = adafactor_tables(entries, off)
    return tensors, nt


def test_fold_table_covers_every_row_and_column_once():
    from onetrainer_amd.util.optimizer.came_fused import FOLD_BLOCK, came_fold_table
    tensors, nt = _tables()
    fold, nf, nm, ranges = came_fold_table(tensors, nt)
    big = [i for i in range(nt) if tensors[i].mode == 2]
    assert len(big) >= 3 and set(ranges) == set(range(nt))
    assert any(tensors[i].batch * tensors[i].rows > FOLD_BLOCK for i in big)       # more than one block of rows
    assert any(tensors[i].batch * tensors[i].cols > FOLD_BLOCK for i in big)       # and of columns
    for i in range(nt):
        t = tensors[i]
        f0, f1, r0, r1 = ranges[i]
        if t.mode != 2:
            assert f0 == f1 and r0 == r1
            continue
        seen = [np.zeros(t.batch * t.rows, np.int32), np.zeros(t.batch * t.cols, np.int32), np.zeros(t.batch, np.int32)]
        assert 0 <= f0 < f1 <= nf <= r0 < r1 <= nf + nm
        for j in list(range(f0, f1)) + list(range(r0, r1)):
            f = fold[j]
            assert f.tensor == i and (f.kind == 2) == (j >= nf)
            seen[f.kind][f.i0:f.i1] += 1
        assert all(np.all(s == 1) for s in seen), i
    # every entry of the table belongs to exactly one tensor's ranges
    assert sum(r[1] - r[0] for r in ranges.values()) == nf and sum(r[3] - r[2] for r in ranges.values()) == nm


@pytest.mark.parametrize("edit", [dict(i1=1 << 40), dict(i0=-1), dict(tensor=99), dict(kind=2), dict(kind=5),
                                  dict(i0=0, i1=1000)])
def test_fold_table_rejects_out_of_range_entries(edit):
    from onetrainer_amd.util.optimizer.came_fused import came_fold_table, check_fold_table
    tensors, nt = _tables()
    fold, nf, nm, _ = came_fold_table(tensors, nt)
    check_fold_table(fold, nf, nm, tensors, nt)
    for k, v in edit.items():
        setattr(fold[0], k, v)
    with pytest.raises(ValueError, match="fold table"):
        check_fold_table(fold, nf, nm, tensors, nt)


def test_fold_table_rejects_a_tensor_that_owns_its_states():
    from onetrainer_amd.util.optimizer.came_fused import came_fold_table, check_fold_table
    tensors, nt = _tables()
    fold, nf, nm, _ = came_fold_table(tensors, nt)
    fold[0].tensor = next(i for i in range(nt) if tensors[i].mode != 2)
    with pytest.raises(ValueError, match="fold table"):
        check_fold_table(fold, nf, nm, tensors, nt)
