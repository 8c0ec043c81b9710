"""NumPy float64 restatement of DoRA (modules/module/LoRAModule.py:385-419 and its autograd with the norm detached):
norms, merge, gradient projection, and the fp32 error bounds the tests hold the kernels (and the reference's own fp32
run) to.  Weights are [out, kk, cin] (store layout with the kernel taps flattened; kk = 1 for a Linear), down is
[r, kk, cin], up is [out, r]; axis 0 keeps the input channels (n, dora_scale of length cin), axis 1 the output
channels (length out).

Bounds (u = 2^-24, first order).  A sum of k fp32 terms, in any order, is within (k - 1) u of sum |terms|.
  * Weff = W + s sum_j up_j down_j: r products, r - 1 adds, the scaling and the add of W, so
    |dWeff| <= (r + 2) u mag with mag = |W| + s sum_j |up_j down_j| (cancellation between W and the adapter term is
    covered by mag, not by |Weff|).
  * S = sum of k squares of Weff: non-negative terms, so (k - 1) u S for the sum, u S for the squarings, and
    2 |Weff| |dWeff| per term carried in; n = sqrt(S) + eps adds the rounding of the root and of the add:
    |dn| <= (sum 2 |Weff| dWeff + k u S) / (2 sqrt(S)) + 2 u n.
  * projection: a result that is a sum of `terms` products is within (terms + 4) u sum |terms| -- the sum, the
    product, the two roundings of H = (G dora_scale) / n and the final scaling by s.  For d_scale the products are
    taken apart into G W / n and the r products G s up_j down_j / n per element, since Weff is formed in fp32 first.
"""
import numpy as np

U = 2.0 ** -24


def f64(x):
    return np.asarray(x, dtype=np.float64)


def weff(W, down, up, s):
    return f64(W) + s * np.einsum("oj,jkc->okc", f64(up), f64(down))


def mag(W, down, up, s):
    return np.abs(f64(W)) + s * np.einsum("oj,jkc->okc", np.abs(f64(up)), np.abs(f64(down)))


def _red(x, axis):
    return x.sum(axis=(0, 1)) if axis == 0 else x.sum(axis=(1, 2))


def _bc(v, axis):
    return v[None, None, :] if axis == 0 else v[:, None, None]


def norms(W, down, up, s, axis, eps):
    x = weff(W, down, up, s)
    return np.sqrt(_red(x * x, axis)) + eps


def norm_bound(W, down, up, s, axis, eps):
    x = weff(W, down, up, s)
    r = np.asarray(up).shape[1]
    dx = (r + 2) * U * mag(W, down, up, s)
    S = _red(x * x, axis)
    k = x.size // S.size
    root = np.sqrt(S)
    carried = _red(2 * np.abs(x) * dx, axis) + k * U * S
    return np.where(S > 0, carried / (2 * np.where(S > 0, root, 1.0)), 0.0) + 2 * U * (root + eps)


def merge(W, down, up, scale, s, axis, eps):
    """-> (n, W') in float64; W' is 0 on a line whose n is 0"""
    x = weff(W, down, up, s)
    n = np.sqrt(_red(x * x, axis)) + eps
    safe = np.where(n != 0, n, 1.0)
    wp = np.where(_bc(n, axis) != 0, _bc(f64(scale), axis) * (x / _bc(safe, axis)), 0.0)
    return n, wp


def project(G, W, down, up, scale, n, s, axis):
    """gradients of down, up and dora_scale from G = dL/dW' with n held constant, and their bounds"""
    G, n = f64(G), f64(n)
    x = weff(W, down, up, s)
    r = np.asarray(up).shape[1]
    ok = _bc(n, axis) != 0
    inv = np.where(ok, 1.0 / _bc(np.where(n != 0, n, 1.0), axis), 0.0)
    H = G * _bc(f64(scale), axis) * inv
    d_scale = _red(G * x * inv, axis)
    d_up = s * np.einsum("okc,jkc->oj", H, f64(down))
    d_down = s * np.einsum("oj,okc->jkc", f64(up), H)
    k = x.size // n.size
    b_scale = (k * (r + 1) + 4) * U * _red(np.abs(G) * mag(W, down, up, s) * inv, axis)
    t_up = x.shape[1] * x.shape[2]
    b_up = (t_up + 4) * U * s * np.einsum("okc,jkc->oj", np.abs(H), np.abs(f64(down)))
    b_down = (x.shape[0] + 4) * U * s * np.einsum("oj,okc->jkc", np.abs(f64(up)), np.abs(H))
    return (d_down, d_up, d_scale), (b_down, b_up, b_scale)


def bf16_round(x):
    """float64 -> the nearest bf16 (ties to even), returned as its uint16 bits"""
    f = np.asarray(x, dtype=np.float64).astype(np.float32)   # double rounding is harmless here: checked to one ulp
    b = f.view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    return b.astype(np.uint16)


def bf16_ulps(a_bits, b_bits):
    """distance in bf16 steps between two arrays of bf16 bit patterns (sign-magnitude -> ordered integers)"""
    def key(v):
        v = v.astype(np.int64)
        return np.where(v & 0x8000, -(v & 0x7FFF), v & 0x7FFF)
    return np.abs(key(a_bits) - key(b_bits))


class Bf16Tally:
    """bf16 results against float64 expectations: every element equal bits or one bf16 step apart, none further
    (checked as each tensor is added); the share one step apart over everything added is capped (check)"""

    def __init__(self):
        self.off = self.size = 0

    def add(self, got_bits, want_f64, what=""):
        d = bf16_ulps(np.asarray(got_bits).reshape(-1), bf16_round(want_f64).reshape(-1))
        far = int((d > 1).sum())
        assert far == 0, f"{what}: {far} of {d.size} elements more than one bf16 step off (max {int(d.max())})"
        self.off += int((d == 1).sum())
        self.size += d.size

    def check(self, cap=1e-3):
        print(f"bf16: {self.off} of {self.size} elements one step apart")
        assert self.off <= cap * self.size, f"{self.off} of {self.size} elements one bf16 step off (cap {cap})"
