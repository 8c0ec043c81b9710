"""The references and bounds of tests/_diffusion_edges.py, held to account on the CPU: the host Philox reproduces the
Random123 known answers, the u01 corner and the (seed, sample) pairs that hit it; an honest fp32 evaluation of every
formula that is not exact (the Box-Muller normals in numpy fp32, the loss family in the kernels' blocked order) stays
inside every bound on the case tables; the measured floors K_BM and K_LC are what the helper records; planted errors
fall outside, each by the name of its check; and the tables reach the paths they are meant to.  No GPU."""
import math

import numpy as np
import pytest
import torch

import _diffusion_edges as E
from _diffusion_edges import BF, F32, F64, U8, U17, U24

CPU = "cpu:"
TD = [F32, BF]


# ------------------------------------------------------------------------------------------
# 1. the host Philox and u01
def _hex(words):
    return " ".join(format(int(w), "08x") for w in words)


@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_known_answers(ctr, key, out):
    """Random123's kat_vectors for philox4x32-10"""
    assert _hex(E.philox4x32_10(ctr, key)) == out
    # the same through arrays, next to other counters
    w = E.philox4x32_10(tuple(np.array([c, 1, c], dtype=np.uint64) for c in ctr), key)
    assert _hex(x[0] for x in w) == out and _hex(x[2] for x in w) == out


def test_u01_corner():
    assert E.u01(0xFFFFFF00) == np.float32(1.0) and E.u01(0xFFFFFFFF) == np.float32(1.0)
    assert E.u01(0) == np.float32(0.5 * 2.0 ** -24) and E.u01(0xFF) == E.u01(0)
    assert E.u01(0xFFFFFE00) == np.float32(1.0) - np.float32(2.0 ** -23)          # 0xFFFFFE + 0.5 rounds down (even)
    k = np.array([2 ** 23 - 1, 2 ** 23, 2 ** 23 + 1, 2 ** 23 + 2], dtype=np.uint64)
    got = E.u01(k << np.uint64(8)).astype(np.float64) * 2.0 ** 24
    assert got.tolist() == [2 ** 23 - 0.5, 2 ** 23, 2 ** 23 + 2, 2 ** 23 + 2]     # the + 0.5 is lost from 2^23 on
    assert E.BELOW_ONE == np.nextafter(np.float32(1), np.float32(0))


def test_corner_pairs_rederived():
    """stream 2, tag 0x74696d65: word 0 >> 8 = 0xFFFFFF at the listed (seed, sample) pairs, nowhere around them"""
    for seed, sample in E.CORNER_PAIRS:
        w = E.philox_words(seed, 2, E.TAG_TIME, E._idx(max(sample - 3, 0), 8))[0]
        hit = np.flatnonzero((w >> np.uint64(8)) == 0xFFFFFF)
        assert hit.tolist() == [min(sample, 3)], (seed, sample)
        assert E.philox_uniform(seed, sample) == np.float32(1.0) and E.uniform_held(seed, sample) == E.BELOW_ONE
    assert int(E.philox_words(1779877, 2, E.TAG_TIME, 0)[0]) == 0xffffff8e
    # what UNIFORM with the defaults makes of the corner: 1000 from the raw uniform, 999 from the held one
    cfg = {"min_s": 0.0, "max_s": 1.0, "shift": 1.0}
    assert E.uniform_timesteps(np.array([1.0, E.BELOW_ONE], dtype=np.float32), cfg).tolist() == [1000, 999]
    for seed, elem, stream, word in E.NORMAL_CORNERS:
        assert int(E.philox_words(seed, stream, E.TAG_NORMAL, elem >> 1)[0]) == word and word >> 8 == 0xFFFFFF
        z, rad, _ = E.normal_math(seed, stream, E._idx(elem, 2), np.float64)
        assert rad.tolist() == [0.0, 0.0] and not z.any()
        assert not E.normal_math(seed, stream, E._idx(elem, 2), np.float32)[0].any()


# ------------------------------------------------------------------------------------------
# 2. an honest fp32 evaluation is inside every bound
def _normal_draws():
    for n, off in E.NORMAL_CASES:
        big = n > 4096
        for seed in (E.SEEDS[1:2] if big else E.SEEDS):
            for stream in ((1,) if big else E.NORMAL_STREAMS):
                yield seed, stream, off, n


def test_fp32_normals():
    for seed, stream, off, n in _normal_draws():
        z = E.normal_math(seed, stream, E._idx(off, n), np.float32)[0]
        E.check_normals(CPU + "normals", z, seed, stream, off, n, f"normals seed={seed} stream={stream} off={off} n={n}")


def test_normal_floor_measured():
    """the k of the docstring: the worst error of the numpy fp32 Box-Muller beyond the destination's rounding, in units
    of 2^-24 rad (1 + |a|), on the test's own draws.  K_BM is 4 x the recorded k taken one decimal up, and no more;
    numpy's logf / sinf / cosf differ between machines, so what is measured here may be smaller"""
    k = 0.0
    for seed, stream, off, n in _normal_draws():
        idx = E._idx(off, n)
        z64, rad, a = E.normal_math(seed, stream, idx, np.float64)
        z32 = E.normal_math(seed, stream, idx, np.float32)[0].astype(np.float64)
        excess = np.clip(np.abs(z32 - z64) - U24 * np.abs(z64), 0, None)
        unit = U24 * rad * (1 + a)
        k = max(k, float(np.max(np.where(unit > 0, excess / np.where(unit > 0, unit, 1), 0))))
    print(f"box-muller: k = {k:.3f} (K_BM = {E.K_BM})")
    rec = E.K_MEASURED["box-muller"]
    assert k <= E.K_BM / 4 <= rec + 0.1 and E.K_BM / 4 == math.ceil(rec * 10) / 10
    assert E.K_BM * U24 * (1 + 2 * math.pi) < U17          # the project's ceiling 2^-17 rad


def _loss_cases():
    for shape in E.LOSS_SHAPES:
        for td in TD:
            yield E.loss_case(*shape, td)
    yield E.loss_case(*E.LC_SHAPE, F32, "lc")


def test_log_cosh_floor_measured():
    """K_LC as K_BM: the fp32 term (d + softplus(-2 d)) - ln 2 against float64, beyond 2^-24 |term|, in units of
    2^-24 (|d| + softplus(-2 d) + ln 2), on LC_PROBES and the d of every loss case"""
    k = 0.0
    for c in _loss_cases():
        d32 = c.pred[..., :c.C].float() - c.target.float()
        r = E.lc_term(d32.double())
        excess = ((E.lc_term(d32).double() - r).abs() - U24 * r.abs()).clamp_min(0)
        k = max(k, float((excess / (U24 * E.lc_floor_unit(d32))).max()))
    print(f"log-cosh: k = {k:.3f} (K_LC = {E.K_LC})")
    rec = E.K_MEASURED["log-cosh"]
    assert k <= E.K_LC / 4 <= rec + 0.1 and E.K_LC / 4 == math.ceil(rec * 10) / 10


def _r16(t):
    return t.to(BF)


def _fp32_loss_case(c, configs):
    for cfg in configs:
        r, h = E.loss_math(c, cfg, F64), E.loss_math(c, cfg, F32)
        what = f"{c.name} {cfg}"
        E.check_loss(CPU + "diffusion_loss", c, cfg, h, r, what)
        for go in (1.0, 0.5):
            ref, M = E.loss_grad_math(c, cfg, r["coef"], go, F64)
            g = _r16(E.loss_grad_math(c, cfg, h["coef"], go, F32)[0])
            E.check_grad(CPU + "diffusion_loss_grad", c, g, ref, M, what + f" grad go={go}")
    for cfg in E.MSE_CONFIGS:
        r, h = E.mse_math(c, cfg, F64), E.mse_math(c, cfg, F32)
        E.check_loss(CPU + "mse_loss", c, cfg, h, r, f"{c.name} mse {cfg}")
        ref, M = E.mse_grad_math(c, r["coef"], 0.5, F64)
        E.check_grad(CPU + "mse_grad", c, _r16(E.mse_grad_math(c, h["coef"], 0.5, F32)[0]), ref, M, f"{c.name} mse grad")


@pytest.mark.parametrize("td", TD, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", E.LOSS_SHAPES, ids=str)
def test_fp32_losses(shape, td):
    _fp32_loss_case(E.loss_case(*shape, td), E.LOSS_CONFIGS)


def test_fp32_log_cosh_probes():
    """per = 1: losses[b] is the term of one d; sign(0) = 0 and tanh in the gradient"""
    c = E.loss_case(*E.LC_SHAPE, F32, "lc")
    d = c.pred[..., 0].float() - c.target[..., 0]
    assert d.flatten().tolist() == [float(np.float32(v)) for v in E.LC_PROBES]
    _fp32_loss_case(c, E.LOSS_CONFIGS)
    g = E.loss_grad_math(c, E.LOSS_CONFIGS[0], E.loss_math(c, E.LOSS_CONFIGS[0], F64)["coef"], 1.0, F64)[0]
    assert float(g[0, 0, 0]) == 0.0 and bool((g[1:, 0, 0] != 0).all())


def test_velocity_is_the_oracles():
    """E.velocity spells get_velocity's `** 0.5` as the correctly rounded sqrt: the same bits wherever this host's
    pow(x, 0.5) is correctly rounded too (torch's AVX-512 CPU sqrt is an ulp off at alphas_cumprod[500])"""
    acp = E.coeff_tables()[0]
    for dt in TD:
        c = E.pro_case(5, 63, 4, dt)
        x0 = c.lat * E.SF
        a = acp.to(dt)
        same_pow = torch.equal(a ** 0.5, E.sqrt_rn(a)) and torch.equal((1 - a) ** 0.5, E.sqrt_rn(1 - a))
        print(dt, "pow(x, 0.5) is correctly rounded on this host:", same_pow)
        if same_pow:
            E.check_bits(CPU + "velocity", E.velocity(x0, c.eps, c.t.long()),
                         E.OD.get_velocity(x0, c.eps, c.t.long(), E.OD.scaled_linear_betas()), f"velocity {dt}")
        assert E.PRO_T == (0, 1, 500, 998, 999) and c.t.tolist() == list(E.PRO_T)
    x = torch.rand(4096, generator=E._gen(3), dtype=F64).float()
    assert np.array_equal(E.sqrt_rn(x).numpy(), np.sqrt(x.numpy()))
    f = E.flow_reference(E.pro_case(5, 63, 4, BF), 8)[1]
    assert f.dtype == BF and E.FLOW_SHIFT != float(torch.tensor(E.FLOW_SHIFT).to(BF)) and E.FLOW_SHIFT != 0


# ------------------------------------------------------------------------------------------
# 3. planted errors: each is reported as a failure by its check
def _rejected(fn, name):
    saved = dict(E.WORST)
    try:
        fn()
    except AssertionError as e:
        return name in str(e)
    finally:
        E.WORST.clear()
        E.WORST.update(saved)
    return False


@pytest.mark.parametrize("plant", ["sin_cos_swapped", "v1_for_v0", "high_word_dropped"])
def test_planted_normals(plant):
    seed, stream = 1234, 1
    off, n = (2 ** 33 - 3, 8) if plant == "high_word_dropped" else (1, 256)
    z = E.normal_math(seed, stream, E._idx(off, n), np.float32, plant)[0]
    assert _rejected(lambda: E.check_normals("planted", z, seed, stream, off, n, "normals " + plant), "normals " + plant)
    if plant == "high_word_dropped":   # the elements below call 2^32 are still right
        ok = E.normal_math(seed, stream, E._idx(off, 3), np.float32, plant)[0]
        E.check_normals(CPU + "normals", ok, seed, stream, off, 3, "below 2^32 calls")
        u = np.minimum(E.u01(E.philox_words(seed, 2, E.TAG_TIME, E._idx(2 ** 32 - 3, 8), plant)[0]), E.BELOW_ONE)
        assert _rejected(lambda: E.check_bits("planted", u, E.uniform_held(seed, E._idx(2 ** 32 - 3, 8)), "uniforms"), "uniforms")
        assert (u[:3] == E.uniform_held(seed, E._idx(2 ** 32 - 3, 3))).all()


def test_planted_noise_ex_local_sample():
    shape, off, n = E.NOISE_EX_CASES[0]
    seed = 21
    f = lambda st, idx: torch.from_numpy(E.normal_math(seed, st, idx, np.float32)[0])   # noqa: E731
    base, pert = f(1, E._idx(off, n)), f(5, E._idx(off, n))
    good = E.noise_ex_compose(base, f(4, E.noise_ex_index(shape, off, n)), pert, 0.35, 0.05)
    bad = E.noise_ex_compose(base, f(4, E.noise_ex_index(shape, off, n, "local_sample")), pert, 0.35, 0.05)
    E.check_bits(CPU + "noise_ex", good.clone(), good, "noise_ex")
    assert _rejected(lambda: E.check_bits("planted", bad, good, "noise_ex stream 4"), "noise_ex stream 4")


@pytest.mark.parametrize("plant", ["last_element", "neighbour_mask", "nblk_short"])
def test_planted_loss_sums(plant):
    shape = (4, 2049, 1, 8) if plant != "neighbour_mask" else (4, 683, 3, 8)   # sample 1: the outlier is the last element
    c = E.loss_case(*shape, F32)
    cfg = E.LOSS_CONFIGS[10]   # masked, unmasked_weight 0.1, no normalisation, all strengths
    r, h = E.loss_math(c, cfg, F64), E.loss_math(c, cfg, F32, plant)
    assert _rejected(lambda: E.check_loss("planted", c, cfg, h, r, "loss " + plant), "loss " + plant + " losses")
    E.check_loss(CPU + "diffusion_loss", c, cfg, E.loss_math(c, cfg, F32), r, "loss without the plant")


def test_planted_guard_write():
    for dt in (BF, F32, torch.int32):
        buf, v, w = E.gbuf(5, dt)
        v.fill_(1)
        assert E.gbuf_ok(buf, w) and not E.untouched(buf)
        buf[1, 7] = 0.0                      # the element before the destination
        assert not E.gbuf_ok(buf, w)
        buf[1, 7] = math.nan
        buf[1, 8 + w] = 0.0                  # the element after it
        assert not E.gbuf_ok(buf, w)
        buf[1, 8 + w] = math.nan
        buf[2, 0] = 1.0                      # the row below
        assert not E.gbuf_ok(buf, w)
    buf, v, w = E.gbuf(4, F32)
    assert E.untouched(buf) and v.dtype == F32 and bool(torch.isnan(v).all()) and v.data_ptr() % 4 == 0


# ------------------------------------------------------------------------------------------
# 4. the tables reach what they claim
def test_tables_reach_the_counter_words():
    hi = lambda start, n, sh: sorted(set((int(v) >> sh) >> 32 for v in E._idx(start, n)))   # noqa: E731
    assert any(hi(off, n, 1) == [0, 1] for n, off in E.NORMAL_CASES)                 # call >> 32 changes inside a slice
    assert any(off % 2 == 1 for n, off in E.NORMAL_CASES)                            # a pair split across the slice start
    assert any(off >> 33 > 1 for n, off in E.NORMAL_CASES)
    assert any(n > E.GRID for n, _ in E.NORMAL_CASES) and {255, 256, 257} <= {n for n, _ in E.NORMAL_CASES}
    assert any(len(hi(s0, 65, 0)) == 2 for s0 in E.UNIFORM_SAMPLE0)                  # idx >> 32 changes inside a slice
    assert any(s >> 32 for s in E.SEEDS) and {63, 64, 65} <= set(E.UNIFORM_NS)
    for (B, h, w, C), off, n in E.NOISE_EX_CASES:
        hwc = h * w * C
        assert off % C and off % hwc and n % hwc and (off + n) % hwc                  # mid-pixel, mid-sample, ragged end
        idx = E.noise_ex_index((B, h, w, C), off, n)
        assert len(set((idx // np.uint64(C)).tolist())) >= 2                         # more than one sample in the slice
        assert not np.array_equal(idx, E.noise_ex_index((B, h, w, C), off, n, "local_sample"))
    assert any(off > 2 ** 33 for _, off, _ in E.NOISE_EX_CASES)


def test_tables_reach_the_loss_paths():
    pers = {HW * C for _, HW, C, _ in E.LOSS_SHAPES}
    assert {1, 255, 256, 257, 2047, 2048, 2049, 4097} <= pers
    for B, HW, C, cpad in E.LOSS_SHAPES:
        if C == 3:   # a pixel with elements either side of a LOSS_BLK boundary
            assert (E.LOSS_BLK // C) * C < E.LOSS_BLK < (E.LOSS_BLK // C + 1) * C <= HW * C
    assert {B for B, *_ in E.LOSS_SHAPES} >= {1, 3, 257, 1024} and E.LOSS_MAX_B == 1024
    assert any(cpad == C for _, _, C, cpad in E.LOSS_SHAPES) and any(C == 16 for _, _, C, _ in E.LOSS_SHAPES)
    B, HW, C, cpad = E.LOSS_STRIDE
    assert E.GRID < B * HW * cpad < E.GRID + 4096
    B, HW, C, cpad = E.PRO_STRIDE
    assert E.GRID < B * HW * C < E.GRID + 4096
    cf = E.LOSS_CONFIGS
    assert {c[1] for c in cf} == {0.0, 0.1, 1.0} and {c[2] for c in cf} == {True, False} and {c[0] for c in cf} == {True, False}
    assert {c[3] for c in cf} == {E.ALL_S, E.MSE_S, E.MAE_S, E.LC_S} and {c[4] for c in cf} == {0, 1, 2, 3, 4}
    assert {(f, v) for *_, f, v in cf} >= {(1, True), (1, False), (2, True), (2, False), (3, True), (3, False)}
    # the timesteps: 0, 999 and the crossings of 1000 and gamma
    _, sq, s1m = E.coeff_tables()
    snr = ((sq.double() / s1m.double()) ** 2).tolist()
    ts = E.loss_timesteps()
    assert ts[:2] == [0, 999] and snr[ts[2]] >= 1000 > snr[ts[3]] and snr[ts[4]] >= E.GAMMA > snr[ts[5]]
    # the probes: the outlier's square is >= 100 x the rest of its sample, at each of the four positions
    c = E.loss_case(4, 4097, 1, 8, F32)
    assert c.probe == [0, 4096, 2048, 2047]
    d = (c.pred[..., :1].double() - c.target.double()).reshape(4, -1) ** 2
    for b, e in enumerate(c.probe):
        assert d[b, e] >= 100 * (d[b].sum() - d[b, e]) and c.mask[b, e] == 0.5
    m = c.mask
    assert bool((m < 0).any() and (m > 1).any() and (m == 0).any() and (m == 1).any() and ((m > 0) & (m < 0.1)).any())
    assert bool(torch.isnan(c.pred[..., 1:]).all())                                   # pad channels must not be read


def test_worst_ratios_report_cpu():
    rows = {k: v for k, v in E.WORST.items() if k.startswith(CPU)}
    for k in sorted(rows):
        print(f"{k:34s} {rows[k][0]:8.3f}  {rows[k][1]}")
    assert all(v[0] <= 1 for v in rows.values())
