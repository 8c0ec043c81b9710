"""The NumPy restatement of Adafactor (tests/_oracle_adafactor.py) against the reference's own run recorded in
tests/golden/adafactor_steps.npz (tests/golden/make_adafactor_golden.py), the option refusals and the resolution of
the configuration fields.  CPU only.

Tolerances are derived, not tuned (tests/_oracle_adafactor.py factor_eps / state_eps): every reduction is a sum of n
non-negative terms, so any fp32 summation order is within (n - 1) 2^-24 relative of the exact sum.
  state:      |s - s_ref| <= ((n - 1) + 8 k) 2^-24 |s_ref| after k steps (n = the length the state's mean reduces)
  parameter:  |p - p_ref| <= sum over the steps of  dmag factor_eps 2^-24 + 4 2^-24 |p|,
              dmag = |lr u| + |weight_decay lr p| of that step
  bf16:       equal bits or one bf16 ulp apart, none further, at most 1e-3 of all elements apart
"""
from pathlib import Path

import numpy as np
import pytest

import _oracle_adafactor as AF
from oracle import adamw as OA

GOLD = np.load(Path(__file__).resolve().parent / "golden" / "adafactor_steps.npz")
STATE_KEYS = {"row": "exp_avg_sq_row", "col": "exp_avg_sq_col", "full": "exp_avg_sq"}


def _reduced(shape, key):
    return {"row": shape[-1], "col": shape[-2] if len(shape) >= 2 else 1, "full": 1}[key]


@pytest.mark.parametrize("cname", list(AF.CONFIGS))
def test_oracle_matches_reference_fp32(cname):
    cfg = AF.CONFIGS[cname]
    for n, s in AF.SHAPES:
        p, st = AF.param0(n, s), AF.new_state(s)
        tol = np.zeros(s, np.float64)
        for k in range(AF.STEPS):
            p, info = AF.adafactor_step(p, AF.grad(n, s, k), st, k + 1, **cfg)
            for key, arr in st.items():
                ref = GOLD[f"state/{k}/{n}/{STATE_KEYS[key]}"]
                bound = AF.state_eps(_reduced(s, key), k + 1) * np.abs(ref)
                assert np.all(np.abs(arr.astype(np.float64) - ref) <= bound), (n, k, key)
            if cfg["scale_parameter"]:
                rms = float(GOLD[f"{cname}/f32/{k}/{n}/rms"])
                assert abs(info["rms_p"] - rms) <= ((p.size - 1) / 2 + 4) * AF.U * rms, (n, k)
            tol += info["dmag"] * AF.factor_eps(s, cfg["scale_parameter"]) * AF.U + 4 * AF.U * np.abs(p)
            ref = GOLD[f"{cname}/f32/{k}/{n}/p"]
            d = np.abs(AF.sample(p).astype(np.float64) - ref)
            assert np.all(d <= AF.sample(tol)), (n, k, float(d.max()))


def test_oracle_matches_reference_bf16():
    apart = total = 0
    for cname, cfg in AF.CONFIGS.items():
        for n, s in AF.SHAPES:
            p, st = AF.param0(n, s), AF.new_state(s)
            for k in range(AF.STEPS):
                x, _ = AF.adafactor_step(p, AF.grad(n, s, k), st, k + 1, **cfg)
                bits = OA.f32_to_bf16_bits(x)
                p = OA.bf16_to_f32(bits)
                d = AF.bf16_ulps(AF.sample(bits), GOLD[f"{cname}/bf16/{k}/{n}/p"])
                assert d.max() <= 1, (cname, n, k, int(d.max()))
                apart += int((d != 0).sum())
                total += d.size
    assert apart <= 1e-3 * total, (apart, total)


def test_fp32_summation_order_moves_few_bf16_results():
    """the 1e-3 cap on the CPU: the oracle with fp32 (pairwise) sums against the oracle with float64 sums"""
    apart = total = 0
    for cname in ("scale_clip", "decay_noclip"):
        cfg = AF.CONFIGS[cname]
        for n, s in AF.SHAPES:
            p = AF.param0(n, s)
            st = {dt: AF.new_state(s) for dt in (np.float32, np.float64)}
            for k in range(AF.STEPS):
                bits = {dt: OA.f32_to_bf16_bits(AF.adafactor_step(p, AF.grad(n, s, k), st[dt], k + 1, sum_dtype=dt,
                                                                  **cfg)[0]) for dt in st}
                p = OA.bf16_to_f32(bits[np.float64])
                d = AF.bf16_ulps(bits[np.float32], bits[np.float64])
                assert d.max() <= 1
                apart += int((d != 0).sum())
                total += d.size
    assert apart <= 1e-3 * total, (apart, total)


# ---- options and configuration ------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts, word", [(dict(relative_step=True), "relative_step"),
                                        (dict(relative_step=False, warmup_init=True), "warmup_init"),
                                        (dict(relative_step=False, beta1=0.9), "beta1")])
def test_refused_options_are_named(opts, word):
    from onetrainer_amd.util.optimizer.adafactor_fused import FusedAdafactor
    with pytest.raises(NotImplementedError, match=word):
        FusedAdafactor(None, [], lr=1e-3, **opts)


def test_config_none_resolves_as_the_reference():
    """create.py:922-934: None falls back to eps 1e-30, eps2 1e-3, clip_threshold 1.0, decay_rate -0.8, beta1 None,
    weight_decay 0.0, scale_parameter True, relative_step True, warmup_init False; an explicit value wins"""
    from onetrainer_amd.util.config.TrainConfig import OptimizerConfig
    from onetrainer_amd.util.create import adafactor_options
    o = adafactor_options(OptimizerConfig(optimizer="ADAFACTOR"))
    assert o == dict(eps=1e-30, eps2=1e-3, clip_threshold=1.0, decay_rate=-0.8, beta1=None, weight_decay=0.0,
                     scale_parameter=True, relative_step=True, warmup_init=False)
    o = adafactor_options(OptimizerConfig(optimizer="ADAFACTOR", eps=1e-20, eps2=1e-2, clip_threshold=2.0,
                                          decay_rate=-0.7, weight_decay=0.1, scale_parameter=False,
                                          relative_step=False, warmup_init=False))
    assert o == dict(eps=1e-20, eps2=1e-2, clip_threshold=2.0, decay_rate=-0.7, beta1=None, weight_decay=0.1,
                     scale_parameter=False, relative_step=False, warmup_init=False)


def test_create_optimizer_refuses_relative_step_and_unknown_optimizers():
    from onetrainer_amd.util.config.TrainConfig import TrainConfig
    from onetrainer_amd.util.create import create_optimizer
    cfg = TrainConfig.default_values()
    cfg.optimizer.optimizer = "ADAFACTOR"          # relative_step None -> True, as in the reference
    with pytest.raises(NotImplementedError, match="relative_step"):
        create_optimizer(None, [], cfg)
    cfg.optimizer.relative_step = False
    cfg.learning_rate_scheduler = "ADAFACTOR"
    with pytest.raises(NotImplementedError, match="ADAFACTOR"):
        create_optimizer(None, [], cfg)
    cfg.optimizer.optimizer = "LION"
    with pytest.raises(NotImplementedError, match="LION"):
        create_optimizer(None, [], cfg)


def test_tables_cover_every_element_once():
    """the slab table the kernels walk: every element of every tensor in exactly one slab, all three modes"""
    from onetrainer_amd.util.optimizer.adafactor_fused import adafactor_tables
    entries, off = [], 0
    for _, s in AF.SHAPES:
        entries.append((off, s, 0))
        off += (int(np.prod(s)) + 7) // 8 * 8
    tensors, slabs, nt, ns, n_state, n_scratch = adafactor_tables(entries, off)
    assert nt == len(AF.SHAPES) and {tensors[i].mode for i in range(nt)} == {0, 1, 2}
    for i in range(nt):
        t = tensors[i]
        seen = np.zeros(t.numel, np.int32)
        for s in (slabs[j] for j in range(t.slab0, t.slab0 + t.n_slabs)):
            if t.mode == 0:
                seen[s.row0:s.row1] += 1
            else:
                seen.reshape(t.batch * t.rows, t.cols)[s.row0:s.row1, s.col0:s.col1] += 1
        assert np.all(seen == 1), i
    with pytest.raises(ValueError):
        adafactor_tables([(4, (8, 8), 0)], 128)
    with pytest.raises(ValueError):
        adafactor_tables([(0, (8, 8), 0)], 32)
