"""NumPy float64 restatement of the HEAVY_TAIL, COS_MAP and SIGMOID timestep samplers
(modules/modelSetup/mixin/ModelSetupNoiseMixin.py:107-153) given the uniform draw, and the fp32 error bounds the tests
hold the reference's own fp32 run and the kernel (csrc/diffusion.hip, timestep_ex_kernel) to.

U = 2^-24 is the relative error of one fp32 rounding; the bounds are first order in U and count roundings.

HEAVY_TAIL, the value before truncation (heavy_tail_band).  With u the fp32 draw, |w| = |noising_weight|:
  a = fl(pi/2) u            2 roundings, |a| <= pi/2                       |da| <= 3.15 U
  c = cos(a)                |sin| <= 1 carries da; 2 ulp for the library    |dc| <= 5.15 U
  p = c c                   2 |c| dc + 1 rounding                           |dp| <= 11.3 U
  g = (p - 1) + u           two roundings at magnitude <= 1, then <= 0.11   |dg| <= 12.5 U
  s = w g                   w rounded, 1 rounding, |g| <= 0.11              |ds| <= 12.8 |w| U
  v = (1 - u) - s           two roundings, |v| <= 1 + 0.11 |w|              |dv| <= (2 + 13 |w|) U
  t0 = v T + min_t          two roundings at magnitude <= N                 |dt0| <= (T (2 + 13 |w|) + 2 N) U
  t = Ns t0 / (sm1 t0 + N)  slope <= L = max(shift, 1 / shift); its own six roundings act on a result <= N, the three
                            of the denominator amplified by A = (|shift - 1| t0 + N) / (sm1 t0 + N) <= 1 for
                            shift >= 1 and <= (2 - shift) / shift below
  => |dt| <= (L (T (2 + 13 |w|) + 2 N) + N (3 + 3 A)) U.
A draw whose float64 value lies closer than that to an integer may truncate either way in fp32 and is left out of an
exact comparison.  At N = T = 1000, w = 1, shift = 3 the band is 0.0034, so about 0.7 % of the draws fall inside.

COS_MAP / SIGMOID bucket weights, relative (weights_roundings).  lin = linspace(0, 1, T) in fp32 is step * i or
1 - step * (T - 1 - i): relative error <= 4 U.  For z with relative error dz U, D(z) = (shift - shift z) + z has
absolute error <= (shift (dz + 4) + dz) U + D U and D >= min(shift, 1), so
  rel D(z) <= R(dz) = (shift (dz + 4) + dz) / min(shift, 1) + 1.
  x = lin / D(lin):                      dx = 4 + R(4) + 1
  derivative = shift / (D'(lin)) ** 2:   D' = (shift + lin) - lin shift, rel <= R' = (8 shift + 5) / min(shift, 1) + 1;
                                         squared, shift rounded, one division: 2 R' + 3
  COS_MAP:  den = pi - 2 pi x + 2 pi x^2 >= pi / 2; absolute error pi (1 + 2 (dx + 2) + 2 (2 dx + 3) + 6) U, so
            rel den <= (12 dx + 34) U; 2 / den and the product with the derivative add 2:
            total 12 dx + 2 R' + 39
  SIGMOID:  y = x / D(x): dy = dx + R(dx) + 1.  arg = -w (y - b), b = noising_bias + 0.5: absolute error
            E = |w| (dy + |b| + 3 (1 + |b|)) U.  exp carries E and adds 2 for the library; 1 + e, the reciprocal and
            the product with the derivative add 3:
            total E + 2 R' + 8
"""
import math

import numpy as np

U = 2.0 ** -24
BELOW_ONE = np.float32(1.0) - np.float32(2.0 ** -24)        # the largest fp32 below 1


def shift_map(t, N, shift):
    return N * shift * t / ((shift - 1.0) * t + N)


def heavy_tail_value(u, N, min_t, max_t, shift, weight):
    """the timestep before truncation, float64, of the fp32 draws u"""
    u = np.asarray(u, dtype=np.float64)
    v = 1.0 - u - weight * (np.cos(math.pi / 2.0 * u) ** 2.0 - 1.0 + u)
    return shift_map(v * (max_t - min_t) + min_t, N, shift)


def heavy_tail_band(N, min_t, max_t, shift, weight):
    w, T = abs(weight), max_t - min_t
    L = max(shift, 1.0 / shift)
    A = 1.0 if shift >= 1 else (2.0 - shift) / shift
    return (L * (T * (2 + 13 * w) + 2 * N) + N * (3 + 3 * A)) * U


def heavy_tail_decided(u, N, min_t, max_t, shift, weight):
    """(int timesteps of the float64 value, mask of the draws farther than the band from an integer)"""
    t = heavy_tail_value(u, N, min_t, max_t, shift, weight)
    return np.trunc(t).astype(np.int64), np.abs(t - np.rint(t)) > heavy_tail_band(N, min_t, max_t, shift, weight)


def table_lookup(cdf, u, min_t):
    """min_t + the first index with cdf[index] > u, u held below 1.0; fp32 comparisons, exact"""
    cdf = np.asarray(cdf, dtype=np.float32)
    u = np.minimum(np.asarray(u, dtype=np.float32), BELOW_ONE)
    return min_t + np.searchsorted(cdf, u, side="right").astype(np.int64)


def _R(dz, shift):
    return (shift * (dz + 4) + dz) / min(shift, 1.0) + 1


def weights_roundings(dist, shift, bias, weight):
    """relative error of one fp32 bucket weight of the reference, in units of U (derivation above)"""
    dx = 4 + _R(4, shift) + 1
    Rp = (8 * shift + 5) / min(shift, 1.0) + 1
    if dist == "COS_MAP":
        return 12 * dx + 2 * Rp + 39
    dy = dx + _R(dx, shift) + 1
    b = abs(bias + 0.5)
    return abs(weight) * (dy + b + 3 * (1 + b)) + 2 * Rp + 8


def single_shift_sigmoid(N, min_t, max_t, shift, bias, weight):
    """SIGMOID weights with the inverse shift applied once (what the reference does NOT compute)"""
    lin = np.linspace(0.0, 1.0, max_t - min_t)
    x = lin / (shift - shift * lin + lin)
    return 1.0 / (1.0 + np.exp(-weight * (x - (bias + 0.5)))) * (shift / (shift + lin - lin * shift) ** 2.0)
