"""CPU checks of the sampler's math: the DDIM timestep table against known answers, the float64 restatement
(tests/_oracle_sampler.py) against a closed form that does not use it, and the rescale factor at cfg_scale = 1."""
import numpy as np
import pytest

import _oracle_sampler as O
from onetrainer_amd.modelSampler import ddim_table


def test_timestep_table_known_answers():
    t = ddim_table(20, 1000)
    assert [a for a, _ in t] == list(range(951, 0, -50)) and len(t) == 20
    assert t[0] == (951, 901) and t[-2] == (51, 1)
    assert t[-1] == (1, 0)          # set_alpha_to_one False: the last alpha_prev is alphas_cumprod[0]
    assert t == O.ddim_table(20, 1000)
    f = ddim_table(20, 1000, force_last_timestep=True)
    assert f[0] == (999, 949) and f[1:] == t
    assert ddim_table(1, 1000) == [(1, 0)]
    assert [a for a, _ in ddim_table(30, 1000)] == [1 + 33 * i for i in range(29, -1, -1)]
    assert ddim_table(999, 1000)[0] == (999, 998)
    for steps in (0, 1000, 1001):   # steps_offset 1 puts the first timestep of N steps at N, outside the table
        with pytest.raises(ValueError):
            ddim_table(steps, 1000)


@pytest.mark.parametrize("v_pred", [False, True])
@pytest.mark.parametrize("cfg,rescale", [(7.0, 0.0), (7.0, 0.7), (1.0, 0.7)])
@pytest.mark.parametrize("force_last", [False, True])
def test_closed_form_loop_reproduces_x0(v_pred, cfg, rescale, force_last):
    """x_t = sqrt(a_t) x0 + sqrt(1 - a_t) e with both halves predicting exactly e (v: sqrt(a_t) e - sqrt(1 - a_t) x0):
    every step recovers x0 and moves to sqrt(a_prev) x0 + sqrt(1 - a_prev) e, whatever the guidance; the loop ends at
    alphas_cumprod[0].  Tolerance: float64 roundoff of a dozen operations on O(1) values, amplified by at most
    1 / sqrt(a_t) <= 15 at t = 999."""
    rng = np.random.default_rng(0)
    acp = O.alphas_cumprod()
    x0 = rng.standard_normal((2, 5, 7, 4))
    e = rng.standard_normal((2, 5, 7, 4))
    table = O.ddim_table(20, 1000, force_last)
    t0 = table[0][0]
    x = np.sqrt(acp[t0]) * x0 + np.sqrt(1 - acp[t0]) * e
    tol = 64 * 15 * 2.0 ** -52 * 8
    for t, tp in table:
        sa, s1 = np.sqrt(acp[t]), np.sqrt(1 - acp[t])
        if force_last and t != t0 and t == table[1][0]:
            # after the forced step the state sits at alpha[949] while the table says 951 (as in the reference's
            # loop): restart the closed form from the timestep the step assumes
            x = sa * x0 + s1 * e
        pred = sa * e - s1 * x0 if v_pred else e
        xp, _ = O.step(pred, pred, x, cfg, rescale, v_pred, sa, s1, np.sqrt(acp[tp]), np.sqrt(1 - acp[tp]))
        want = np.sqrt(acp[tp]) * x0 + np.sqrt(1 - acp[tp]) * e
        assert np.abs(xp - want).max() <= tol, (t, np.abs(xp - want).max())
        x = xp
    assert table[-1][1] == 0
    assert np.abs(x - (np.sqrt(acp[0]) * x0 + np.sqrt(1 - acp[0]) * e)).max() <= tol


def test_cfg_scale_one_gives_factor_exactly_one():
    rng = np.random.default_rng(1)
    neg = rng.standard_normal((3, 9, 4)).astype(np.float32)
    pos = rng.standard_normal((3, 9, 4)).astype(np.float32)
    # bf16-like inputs (the kernel's): p = neg + 1 * (pos - neg) is then exactly pos in float64
    neg = O.bf16_bits_to_f64(O.bf16_round_bits(neg))
    pos = O.bf16_bits_to_f64(O.bf16_round_bits(pos))
    for r in (0.7, 0.3, 1.0):
        f = O.rescale_factor(neg, pos, 1.0, r)
        assert f.shape == (3, 1, 1) and np.all(f == 1.0)
    assert np.all(O.rescale_factor(neg, pos, 7.0, 0.7) != 1.0)


def test_rescale_matches_the_reference_expression():
    """r * (p * std_pos / std_p) + (1 - r) * p, the sampler's own form, against the oracle's factored one"""
    rng = np.random.default_rng(2)
    neg, pos = rng.standard_normal((2, 2, 6, 5, 4))
    p = neg + 7.0 * (pos - neg)
    ax = (1, 2, 3)
    ref = 0.7 * (p * (pos.std(axis=ax, ddof=1, keepdims=True) / p.std(axis=ax, ddof=1, keepdims=True))) + (1 - 0.7) * p
    got = p * O.rescale_factor(neg, pos, 7.0, 0.7)
    assert np.abs(got - ref).max() <= 16 * 2.0 ** -52 * np.abs(ref).max()


def test_bound_is_of_fp32_size():
    """the bound is a few u of the operands, not a tolerance in disguise"""
    rng = np.random.default_rng(3)
    neg, pos, x = rng.standard_normal((3, 1, 16, 16, 4))
    acp = O.alphas_cumprod()
    for v_pred in (False, True):
        xp, b = O.step(neg, pos, x, 7.0, 0.7, v_pred, np.sqrt(acp[501]), np.sqrt(1 - acp[501]), np.sqrt(acp[451]),
                       np.sqrt(1 - acp[451]))
        assert b.shape == xp.shape and np.all(b > 0)
        mag = np.abs(x) + 15.0 * (np.abs(neg) + np.abs(pos))
        assert np.all(b <= 64 * O.U * mag)


def test_rgb8_reference():
    x = np.array([-2.0, -1.0, -1.0 + 2.0 ** -8, 0.0, 1.0 / 255, 1.0, 3.0])
    assert O.rgb8(x).tolist() == [0, 0, 0, 128, 128, 255, 255]   # 127.5 and 128.0 -> 128 (ties to even)
