"""NumPy restatement of the Adafactor step the reference runs (modules/util/optimizer/adafactor_extensions.py:16-95
on transformers.Adafactor): fp32 element arithmetic in the order of csrc/adafactor.hip (which is the reference's),
float64 reductions rounded once to fp32.  Pinned to the reference by tests/test_adafactor_oracle.py through
tests/golden/adafactor_steps.npz; the GPU tests compare the kernels with it.

`sum_dtype=np.float32` makes every reduction an fp32 (NumPy pairwise) sum instead: the CPU check of how often an fp32
summation order moves a bf16 result.
"""
import numpy as np

from oracle import adamw as OA

F = np.float32
U = 2.0 ** -24   # fp32 unit roundoff


def new_state(shape):
    if len(shape) >= 2:
        return {"row": np.zeros(shape[:-1], F), "col": np.zeros(shape[:-2] + shape[-1:], F)}
    return {"full": np.zeros(shape, F)}


def _sum(x, axis, dt):
    return np.sum(x, axis=axis, dtype=dt).astype(F)


def _rsqrt(x):
    return F(1) / np.sqrt(x, dtype=F)


def _rms(x, dt):
    """tensor.norm(2) / numel ** 0.5"""
    return F(np.sqrt(np.sum(np.square(x, dtype=dt), dtype=dt))) / F(np.sqrt(float(x.size)))


def adafactor_step(p, g, state, step, lr, eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8, weight_decay=0.0,
                   scale_parameter=False, sum_dtype=np.float64):
    """one step on the fp32 arrays p (parameter value) and g (gradient); `state` (new_state) is updated in place.
    Returns (new fp32 p before any output rounding, info) with info = {"rms_p", "rms_u", "dmag"}: dmag is
    |lr u| + |weight_decay lr p| per element, the magnitude the tolerance formulas scale."""
    p, g = np.asarray(p, F), np.asarray(g, F)
    eps1, eps2 = F(eps[0]), F(eps[1])
    beta2t = 1.0 - float(step) ** decay_rate
    b, omb = F(beta2t), F(1.0 - beta2t)
    upd = g * g + eps1
    if g.ndim >= 2:
        rows, cols = g.shape[-2], g.shape[-1]
        state["row"][...] = OA.fma32(_sum(upd, -1, sum_dtype) / F(cols), omb, state["row"] * b)
        state["col"][...] = OA.fma32(_sum(upd, -2, sum_dtype) / F(rows), omb, state["col"] * b)
        rmean = _sum(state["row"], -1, sum_dtype) / F(rows)
        rf = _rsqrt(state["row"] / rmean[..., None])
        cf = _rsqrt(state["col"])
        u = (rf[..., :, None] * cf[..., None, :]) * g
    else:
        state["full"][...] = OA.fma32(upd, omb, state["full"] * b)
        u = _rsqrt(state["full"]) * g
    rms_u = _rms(u, sum_dtype)
    u = u / np.maximum(rms_u / F(clip_threshold), F(1.0))
    rms_p = _rms(p, sum_dtype) if scale_parameter else F(0)
    lr_eff = np.maximum(eps2, rms_p) * F(lr) if scale_parameter else F(lr)
    u = u * lr_eff
    dmag = np.abs(u).astype(np.float64)
    x = p
    if weight_decay != 0:
        alpha = F(-weight_decay) * lr_eff if scale_parameter else F(-weight_decay * lr)
        dmag = dmag + np.abs(alpha * p)
        x = OA.fma32(p, alpha, p)
    x = x - u
    return x.astype(F), {"rms_p": float(rms_p), "rms_u": float(rms_u), "dmag": dmag}


def factor_eps(shape, scale_parameter):
    """relative error bound (in units of U) of one step's update against any fp32 summation order: every
    reduction is a sum of n non-negative terms, so an fp32 sum in any order is within (n - 1) U of the exact one.
      row state (C - 1), column state (R - 1), mean of the row states (C - 1) + (R - 1);
      u = g rsqrt(row / rmean) rsqrt(col): half of each under the square roots ->  (C - 1) + (R - 1)
      rms(u), when the clip threshold scales: that again + (N - 1) / 2;  rms(p) with scale_parameter: (N - 1) / 2;
      16 for the fp32 roundings of the element ops either side may round differently."""
    n = int(np.prod(shape))
    e = 0.0
    if len(shape) >= 2:
        e = (shape[-1] - 1) + (shape[-2] - 1)
    return e + (e + (n - 1) / 2.0) + ((n - 1) / 2.0 if scale_parameter else 0.0) + 16.0


def state_eps(n_reduced, steps):
    """relative bound of a second-moment state after `steps` steps: the EMA is a convex combination of non-negative
    terms, so the sum's (n - 1) U does not grow; the four fp32 roundings of a step (sum, divide, multiply, fma) on
    either side add 8 U a step."""
    return ((n_reduced - 1) + 8.0 * steps) * U


# ---- the cases tests/golden/make_adafactor_golden.py records and the tests replay --------------------------------
SHAPES = [("m64x70", (64, 70)), ("m300x1030", (300, 1030)), ("m2049x3", (2049, 3)), ("m1x513", (1, 513)),
          ("conv3", (3, 5, 3, 3)), ("conv1", (8, 4, 1, 1)), ("v37", (37,)), ("v5", (5,)), ("m2x4100", (2, 4100)),
          ("zero", (16, 24))]   # "zero": its gradient is all zeros
# Parameters have magnitudes in [0.02, 0.05) and a step moves them by a few bf16 ulps (lr * u of about 1e-3; with
# scale_parameter lr is multiplied by rms(p) of about 0.035): no element comes near zero, where p - lr u cancels and
# one bf16 ulp of the result would be far below the fp32 rounding of the operands.
CONFIGS = {
    "default": dict(lr=1e-3, scale_parameter=False, weight_decay=0.0, clip_threshold=1.0),
    "scale_clip": dict(lr=3e-2, scale_parameter=True, weight_decay=0.0, clip_threshold=0.3),     # clip threshold active
    "decay_noclip": dict(lr=1e-3, scale_parameter=False, weight_decay=0.01, clip_threshold=100.0),   # and not active
    "scale_decay": dict(lr=3e-2, scale_parameter=True, weight_decay=0.01, clip_threshold=1.0),
}
STEPS = 3
SAMPLE = 1024   # the golden keeps at most this many elements of a parameter tensor (evenly strided)


def hashed(shape, seed, scale):
    """deterministic bf16-exact test values in about [-scale, scale): the sum of two 16-bit hashes of the element
    index (oracle.adamw.sr_bits), so the generator and the tests build the same inputs without storing them."""
    n = int(np.prod(shape))
    idx = np.arange(n, dtype=np.uint64)
    h = OA.sr_bits(seed, idx).astype(np.float64) + OA.sr_bits(seed + 7919, idx).astype(np.float64)
    return OA.rbf(((h - 65535.0) / 65536.0 * scale).astype(F)).reshape(shape)


def param0(name, shape):
    h = hashed(shape, 1000 + sum(map(ord, name)), 1.0)
    return OA.rbf((np.where(h < 0, F(-1), F(1)) * (F(0.02) + F(0.03) * np.abs(h))).astype(F))


def grad(name, shape, k):
    """gradient of step k (0-based), scaled 10 ** (-2 + k)"""
    if name == "zero":
        return np.zeros(shape, F)
    return hashed(shape, 2000 + 31 * k + sum(map(ord, name)), 10.0 ** (-2 + k))


def bf16_ulps(a, b):
    """distance in bf16 ulps between two arrays of bf16 bit patterns (sign-magnitude -> ordered integers)"""
    def key(x):
        x = np.asarray(x, np.uint16).astype(np.int64)
        return np.where(x >> 15, -(x & 0x7FFF), x & 0x7FFF)
    return np.abs(key(a) - key(b))


def sample(x):
    x = np.asarray(x).reshape(-1)
    return x[::max(1, -(-x.size // SAMPLE))]
