"""HEAVY_TAIL, COS_MAP and SIGMOID timestep distributions on the host: the bucket weights and the cumulative table
(onetrainer_amd/util/timestep_table.py) against the reference's recorded fp32 tables
(tests/golden/timestep_dists.npz, made by tests/golden/make_timestep_golden.py), the plan ids, and the float64
restatement of the samplers (tests/_timestep_ref.py, whose bounds are derived there) against the reference's
recorded HEAVY_TAIL timesteps."""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import _timestep_ref as R
from onetrainer_amd.modelSetup.BaseStableDiffusionXLSetup import TIMESTEP_DIST, timestep_plan
from onetrainer_amd.util.timestep_table import timestep_cdf, timestep_weights

G = np.load(Path(__file__).parent / "golden" / "timestep_dists.npz")
CASES = sorted({k.rsplit("/", 1)[0] for k in G.files})
TABLE_CASES = [c for c in CASES if not c.startswith("heavy_tail")]
HEAVY_CASES = [c for c in CASES if c.startswith("heavy_tail")]
LEFT_OUT_CAP = 0.02


def case_args(name):
    """(distribution, N, min_t, max_t, shift, bias, weight) of a fixture case"""
    N, mn, mx, shift, bias, weight = G[f"{name}/cfg"]
    N = int(N)
    return name.split("/")[0].upper(), N, int(N * mn), int(N * mx), float(shift), float(bias), float(weight)


def test_fixture_holds_the_cases():
    assert len(TABLE_CASES) == 3 + 3 * 3 * 2 and len(HEAVY_CASES) == 3 * 2
    for c in TABLE_CASES:
        assert G[f"{c}/weights"].dtype == np.float32 and G[f"{c}/t"].size == 64
    for c in HEAVY_CASES:
        assert G[f"{c}/u"].dtype == np.float32 and G[f"{c}/u"].size == 256 and G[f"{c}/t"].size == 256


@pytest.mark.parametrize("name", TABLE_CASES)
def test_weights_match_reference_tables(name):
    """Per bucket, the float64 weight against the reference's fp32 one, relative.  The tolerance is the count of fp32
    roundings of the reference's evaluation times 2^-24, derived in tests/_timestep_ref.py (weights_roundings): 283 at
    COS_MAP shift 1, 507 at shift 3, up to about 2000 for SIGMOID at shift 3 with |noising_weight| 10, where the
    argument of exp carries the error of the doubly shifted linspace times the weight."""
    dist, N, mn, mx, shift, bias, weight = case_args(name)
    ours = timestep_weights(dist, N, mn, mx, shift, bias, weight)
    ref = G[f"{name}/weights"].astype(np.float64)
    assert ours.dtype == np.float64 and ours.shape == ref.shape == (mx - mn,)
    tol = R.weights_roundings(dist, shift, bias, weight) * R.U
    err = np.abs(ours - ref) / np.abs(ours)
    print(name, "worst relative error / tolerance", err.max() / tol, "tolerance", tol)
    assert (err <= tol).all(), (name, err.max(), tol)
    # the reference's own draws land on buckets of positive weight inside [min_t, max_t)
    t = G[f"{name}/t"]
    assert ((t >= mn) & (t < mx)).all() and (ours[t - mn] > 0).all()


def test_sigmoid_applies_the_inverse_shift_twice():
    """at shift 3 the reference's table is the doubly shifted one: a singly shifted table misses it by far more than
    the rounding bound that the doubly shifted one meets"""
    name = "sigmoid/g1_w10_b0"
    dist, N, mn, mx, shift, bias, weight = case_args(name)
    assert shift == 3.0 and weight == 10.0
    ref = G[f"{name}/weights"].astype(np.float64)
    tol = R.weights_roundings(dist, shift, bias, weight) * R.U
    once = R.single_shift_sigmoid(N, mn, mx, shift, bias, weight)
    twice = timestep_weights(dist, N, mn, mx, shift, bias, weight)
    assert (np.abs(twice - ref) <= tol * twice).all()
    assert (np.abs(once - ref) / once).max() > 1000 * tol


def steep_sigmoid():
    """a SIGMOID so steep that exp overflows in float64: exact zero weights on the low buckets"""
    return timestep_weights("SIGMOID", 1000, 0, 1000, 1.0, 0.0, 4000.0)


PLANTED = np.array([0.0, 1.0, 0.0, 0.0, 2.0, 1e-30, 3.0, 0.0, 0.0])


@pytest.mark.parametrize("which", TABLE_CASES + ["steep", "planted"])
def test_cdf_implies_the_bucket_probabilities(which):
    """np.diff of the fp32 table against w / sum(w), per bucket: each edge is rounded to fp32 once at magnitude <= 1,
    an error of at most 2^-25, so a difference of two edges is within 2^-24"""
    if which == "steep":
        w = steep_sigmoid()
        assert (w == 0).sum() > 100 and (w > 0).sum() > 100
    elif which == "planted":
        w = PLANTED
    else:
        w = timestep_weights(*case_args(which))
    cdf = timestep_cdf(w)
    assert cdf.dtype == np.float32 and cdf.shape == w.shape
    assert cdf[-1] == 1.0 and (np.diff(cdf) >= 0).all() and cdf[0] >= 0
    p = np.diff(cdf.astype(np.float64), prepend=0.0)
    err = np.abs(p - w / w.sum())
    print(which, "worst probability error / 2^-24", err.max() / R.U)
    assert (err <= R.U).all()
    assert (p[w == 0] == 0).all()
    last = np.flatnonzero(w > 0)[-1]
    assert (cdf[last:] == 1.0).all() and (last == 0 or cdf[last - 1] < 1.0)


def test_lookup_never_returns_a_zero_weight_bucket():
    for w in (PLANTED, steep_sigmoid()):
        cdf = timestep_cdf(w)
        edges = np.concatenate([cdf, np.nextafter(cdf, np.float32(0)), np.nextafter(cdf, np.float32(2)),
                                np.array([0.0, R.BELOW_ONE, 1.0], dtype=np.float32)])
        u = edges[(edges >= 0) & (edges <= 1)]
        idx = R.table_lookup(cdf, u, 0)
        assert ((idx >= 0) & (idx < w.size)).all() and (w[idx] > 0).all()
        # the strict comparison: a draw of 0 skips the leading buckets of probability 0
        assert R.table_lookup(cdf, np.float32(0), 0) == np.flatnonzero(cdf > 0)[0] >= np.flatnonzero(w > 0)[0]
    assert R.table_lookup(timestep_cdf(PLANTED), timestep_cdf(PLANTED)[1], 0) == 4
    assert R.table_lookup(timestep_cdf(PLANTED), R.BELOW_ONE, 7) == 7 + 6


def test_plan_ids():
    """HEAVY_TAIL's id is new with the samplers (the parent refuses the name)"""
    want = {"UNIFORM": 0, "LOGIT_NORMAL": 1, "HEAVY_TAIL": 2, "COS_MAP": 3, "SIGMOID": 4}
    assert TIMESTEP_DIST == want
    for name, i in want.items():
        assert timestep_plan(SimpleNamespace(timestep_distribution=name)) == i
    with pytest.raises(NotImplementedError, match="INVERSE_SQUARE"):
        timestep_plan(SimpleNamespace(timestep_distribution="INVERSE_SQUARE"))


def test_sd15_and_lora_setups_draw_through_the_sdxl_path():
    from onetrainer_amd.modelSetup.BaseStableDiffusionXLSetup import BaseStableDiffusionXLSetup
    from onetrainer_amd.modelSetup.StableDiffusionFineTuneSetup import StableDiffusionFineTuneSetup
    from onetrainer_amd.modelSetup.StableDiffusionLoRASetup import StableDiffusionLoRASetup
    from onetrainer_amd.modelSetup.StableDiffusionXLLoRASetup import StableDiffusionXLLoRASetup
    for cls in (StableDiffusionFineTuneSetup, StableDiffusionLoRASetup, StableDiffusionXLLoRASetup):
        assert cls.step_inputs is BaseStableDiffusionXLSetup.step_inputs
        assert cls.__init__ is BaseStableDiffusionXLSetup.__init__


@pytest.mark.parametrize("dist", ["COS_MAP", "SIGMOID"])
def test_empty_range_and_bad_weights_are_refused(dist):
    for mn, mx in ((500, 500), (600, 400)):
        with pytest.raises(ValueError, match="min_noising_strength and max_noising_strength"):
            timestep_weights(dist, 1000, mn, mx, 1.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="not finite"):
        timestep_weights(dist, 1000, 0, 1000, float("nan"), 0.0, 0.0)
    with pytest.raises(ValueError, match="no weight table"):
        timestep_weights("HEAVY_TAIL", 1000, 0, 1000, 1.0, 0.0, 0.0)
    for bad in (np.zeros(4), np.array([1.0, np.inf]), np.array([1.0, -1.0]), np.zeros(0)):
        with pytest.raises(ValueError):
            timestep_cdf(bad)


@pytest.mark.parametrize("name", HEAVY_CASES)
def test_heavy_tail_restatement_matches_reference(name):
    """the float64 restatement truncates to the reference's recorded timesteps from the recorded uniforms, except
    where its value lies inside the fp32 error band of an integer (tests/_timestep_ref.py, heavy_tail_band); those
    draws are left out, at most 2 % of them"""
    _, N, mn, mx, shift, bias, weight = case_args(name)
    u, t = G[f"{name}/u"], G[f"{name}/t"]
    want, decided = R.heavy_tail_decided(u, N, mn, mx, shift, weight)
    left_out = 1.0 - decided.mean()
    print(name, "band", R.heavy_tail_band(N, mn, mx, shift, weight), "left out", left_out)
    assert left_out <= LEFT_OUT_CAP
    assert (t[decided] == want[decided]).all()
    assert (np.abs(t - R.heavy_tail_value(u, N, mn, mx, shift, weight)) < 1 + 1e-2).all()   # and nowhere far
