"""csrc/sampler.hip on the GPU: the fused guidance + CFG rescale + DDIM step per element against the float64 oracle's
fp32 bound (tests/_oracle_sampler.py), and the 8-bit conversion exactly."""
import numpy as np
import pytest
import torch

import _oracle_sampler as O
from onetrainer_amd import kernels as K
from onetrainer_amd.model.StableDiffusionXLModel import NoiseScheduler
from onetrainer_amd.modelSampler import ddim_table

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1),       # fewer elements than a wave
          (2, 3, 5),       # not a multiple of any vector width
          (1, 16, 16),     # exactly one workgroup
          (3, 33, 47)]     # several workgroups per sample, ragged tail
TABLE = ddim_table(20, 1000)
FORCED = ddim_table(20, 1000, force_last_timestep=True)
STEPS = {"first": TABLE[0], "middle": TABLE[9], "last": TABLE[-1], "forced": FORCED[0]}


@pytest.fixture(scope="module")
def sched(dev):
    return NoiseScheduler(dev)


@pytest.fixture(scope="module")
def inputs(dev):
    """per shape: pred bf16 [2B, h, w, 8] with zero pads, x fp32 [B, h, w, 4] (host copies as float64 too)"""
    out = {}
    g = torch.Generator().manual_seed(5)
    for B, h, w in SHAPES:
        pred = torch.zeros(2 * B, h, w, 8, dtype=torch.bfloat16)
        pred[..., :4] = (torch.randn(2 * B, h, w, 4, generator=g) * 1.3 + 0.1).bfloat16()
        x = torch.randn(B, h, w, 4, generator=g) * 2.0
        out[(B, h, w)] = (pred.to(dev), x.to(dev), pred[:B, ..., :4].double().numpy(), pred[B:, ..., :4].double().numpy(),
                          x.double().numpy())
    return out


def _coeff(sched, t):
    return float(sched.coeffs[1][t].item()), float(sched.coeffs[2][t].item())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("v_pred", [False, True], ids=["eps", "v"])
@pytest.mark.parametrize("cfg,rescale", [(7.0, 0.0), (7.0, 0.7), (1.0, 0.7), (1.0, 0.0)])
@pytest.mark.parametrize("which", list(STEPS))
def test_step_within_the_oracle_bound(dev, sched, inputs, shape, v_pred, cfg, rescale, which):
    pred, x, neg, pos, x64 = inputs[shape]
    t, tp = STEPS[which]
    got, nxt = K.cfg_ddim_step(pred, x, sched.coeffs, t, tp, cfg, rescale, v_pred)
    sa_t, s1_t = _coeff(sched, t)
    sa_p, s1_p = _coeff(sched, tp)
    want, bound = O.step(neg, pos, x64, cfg, rescale, v_pred, sa_t, s1_t, sa_p, s1_p)
    g = got.double().cpu().numpy()
    err = np.abs(g - want)
    worst = float((err / bound).max())
    print(f"{shape} {which} v={v_pred} cfg={cfg} r={rescale}: max err {err.max():.3e}, worst err/bound {worst:.3f}")
    assert np.all(err <= bound), f"{int((err > bound).sum())} of {err.size} elements outside the bound (worst {worst})"
    # the next UNet input: both halves the bf16 rounding of x_prev, pad channels zero
    B = shape[0]
    bits = nxt.view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(bits[:B, ..., :4], O.bf16_round_bits(got.cpu().numpy()))
    assert np.array_equal(bits[:B], bits[B:]) and not bits[..., 4:].any()
    if which == "last":
        assert tp == 0


@pytest.mark.parametrize("shape", [(2, 3, 5), (3, 33, 47)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("rescale", [0.0, 0.7])
def test_pad_garbage_changes_nothing_and_runs_repeat(dev, sched, inputs, shape, rescale):
    pred, x, *_ = inputs[shape]
    t, tp = STEPS["middle"]
    a, na = K.cfg_ddim_step(pred, x, sched.coeffs, t, tp, 7.0, rescale, False)
    b, nb = K.cfg_ddim_step(pred, x, sched.coeffs, t, tp, 7.0, rescale, False)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(na.view(torch.int16), nb.view(torch.int16))
    dirty = pred.clone()
    dirty[..., 4:6] = 3.0e30
    dirty[..., 6] = float("nan")
    dirty[..., 7] = float("-inf")
    c, nc = K.cfg_ddim_step(dirty, x, sched.coeffs, t, tp, 7.0, rescale, False)
    assert torch.equal(a.view(torch.int32), c.view(torch.int32)) and torch.equal(na.view(torch.int16), nc.view(torch.int16))
    # in place, into given buffers
    xi, ni = x.clone(), torch.full_like(pred, 9.0)
    K.cfg_ddim_step(pred, xi, sched.coeffs, t, tp, 7.0, rescale, False, out=xi, next_in=ni)
    assert torch.equal(a.view(torch.int32), xi.view(torch.int32)) and torch.equal(na.view(torch.int16), ni.view(torch.int16))


def test_constant_prediction_keeps_factor_one(dev, sched):
    """std(p) == 0 (an all-zero or constant guided prediction): the rescale factor is 1, not inf / NaN"""
    t, tp = STEPS["middle"]
    x = torch.randn(2, 5, 7, 4, device=dev)
    for value in (0.0, 0.5):
        pred = torch.zeros(4, 5, 7, 8, dtype=torch.bfloat16, device=dev)
        pred[..., :4] = value
        a, na = K.cfg_ddim_step(pred, x, sched.coeffs, t, tp, 7.0, 0.7, False)
        b, nb = K.cfg_ddim_step(pred, x, sched.coeffs, t, tp, 7.0, 0.0, False)
        assert torch.isfinite(a).all() and torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert torch.equal(na.view(torch.int16), nb.view(torch.int16))


def test_argument_contract(dev, sched, inputs):
    pred, x, *_ = inputs[(2, 3, 5)]
    t, tp = STEPS["middle"]
    bad = [lambda: K.cfg_ddim_step(pred.float(), x, sched.coeffs, t, tp, 7.0),
           lambda: K.cfg_ddim_step(pred[:3], x, sched.coeffs, t, tp, 7.0),
           lambda: K.cfg_ddim_step(pred, x[:1], sched.coeffs, t, tp, 7.0),
           lambda: K.cfg_ddim_step(pred, x.bfloat16(), sched.coeffs, t, tp, 7.0),
           lambda: K.cfg_ddim_step(pred[..., :4].contiguous(), x, sched.coeffs, t, tp, 7.0),
           lambda: K.cfg_ddim_step(pred, x, sched.coeffs, 1000, tp, 7.0),
           lambda: K.cfg_ddim_step(pred, x, sched.coeffs, t, -1, 7.0),
           lambda: K.cfg_ddim_step(pred, x, sched.coeffs, t, tp, 7.0, -0.1),
           lambda: K.cfg_ddim_step(pred, x, sched.coeffs, t, tp, float("nan")),
           lambda: K.cfg_ddim_step(pred, x, sched.coeffs, t, tp, 7.0, next_in=pred),
           lambda: K.cfg_ddim_step(pred, x, (sched.coeffs[0], sched.coeffs[1][:10], sched.coeffs[2]), t, tp, 7.0),
           lambda: K.nhwc_to_rgb8(pred.float()),
           lambda: K.nhwc_to_rgb8(pred[..., :2].contiguous())]
    for f in bad:
        with pytest.raises(ValueError):
            f()


@pytest.mark.parametrize("cpad,n", [(8, 256 * 3 + 96 + 2), (8, 3), (3, 1030)])
def test_nhwc_to_rgb8_exact(dev, cpad, n):
    """every bf16 value at or beside a rounding tie k + 0.5 of the 8-bit grid (x = (2k + 1) / 255 - 1 and its
    neighbours), both clamp edges and their neighbours, values far outside, zeros of both signs"""
    k = np.arange(0, 255, dtype=np.float64)
    ties = (2 * k + 1) / 255.0 - 1.0
    centre = O.bf16_round_bits(ties.astype(np.float32)).astype(np.int32)
    cand = np.concatenate([centre + d for d in (-2, -1, 0, 1, 2)])
    edges = O.bf16_round_bits(np.array([-1.0, 1.0, 0.0, -0.0, -5.0, 5.0, 1e30, -1e30, 2.0 ** -100], dtype=np.float32))
    edge_nb = np.concatenate([edges.astype(np.int32) + d for d in (-1, 0, 1)])
    bits = np.concatenate([cand, edge_nb]).astype(np.uint16)
    bits = bits[np.isfinite(O.bf16_bits_to_f64(bits))]
    vals = np.resize(bits, n * 3).reshape(n, 3)
    full = np.full((n, cpad), 0x7FC0, dtype=np.uint16)      # NaN in every pad channel
    full[:, :3] = vals
    x = torch.from_numpy(full.view(np.int16)).view(torch.bfloat16).to(dev).view(1, 1, n, cpad)
    got = K.nhwc_to_rgb8(x).cpu().numpy().reshape(n, 3)
    want = O.rgb8(O.bf16_bits_to_f64(vals))
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    if vals.size >= bits.size:   # every candidate is in: all 256 levels are reached
        assert set(np.unique(want).tolist()) == set(range(256))


def test_rgb8_inverts_image_to_nhwc(dev):
    img8 = torch.arange(256, dtype=torch.uint8).repeat(3, 4).view(1, 3, 16, 64)
    x = K.image_to_nhwc((img8.float() / 255).to(dev).contiguous())
    back = K.nhwc_to_rgb8(x).cpu()
    # bf16 keeps 8 significant bits: x / 255 * 2 - 1 is held to 2^-8 relative, half a level at most near +-1
    assert (back.permute(0, 3, 1, 2).int() - img8.int()).abs().max() <= 1
