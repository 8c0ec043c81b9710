"""NumPy restatement of the CAME step the reference runs (modules/util/optimizer/CAME.py:79-178): fp32 element
arithmetic in the order of csrc/came.hip (which is the reference's), float64 reductions rounded once to fp32.  Pinned
to the reference by tests/test_came_oracle.py through tests/golden/came_steps.npz; the GPU tests compare the kernels
with it.  `sum_dtype=np.float32` makes every reduction an fp32 (NumPy pairwise) sum instead: the CPU check of how
often an fp32 summation order moves a bf16 result.

The bounds travel with the result, in float64, per element (U = 2^-24, first-order error propagation with the
second-order term of the square kept).  Both sides compute the same expressions and differ in the order of their
fp32 sums and in a few roundings, so a bound is the distance any two such evaluations can have:
  second-moment states   AF.state_eps unchanged: the EMA is a convex combination of non-negative sums
  clipped u              relative E_u U, E_u = AF.factor_eps(shape, False)
  first moment           tol_m <- beta1 tol_m + (1 - beta1) E_u U |u| + 4 U |m|
  d = u - m              t_d = E_u U |u| + tol_m + U |d|
  res = d^2 + eps2       |delta res| <= 2 |d| t_d + t_d^2 + 2 U res
  instability states     S <- beta3 S + (1 - beta3) (mean(|delta res|) + (n - 1) U mean(res)) + 4 U state, for the row
                         states (n = columns) and the column states (n = rows); the mean of the row states is formed
                         from them each step: S_mean = mean(S_row) + ((rows - 1) + 4) U mean
  update                 relative 0.5 (S_row / row + S_mean / mean + S_col / col) + tol_m / |m| + 8 U; tol_m alone for
                         an unfactored tensor, whose update is m
  parameter              lr |update| times that, plus 4 U |p|, for one step
"""
import numpy as np

import _oracle_adafactor as AF
from oracle import adamw as OA

F = np.float32
U = AF.U

SQ_KEYS = {"row": "exp_avg_sq_row", "col": "exp_avg_sq_col", "full": "exp_avg_sq"}
RES_KEYS = {"res_row": "exp_avg_res_row", "res_col": "exp_avg_res_col"}


def new_state(shape):
    """the moments of one tensor and, under "tol", the bounds that travel with them"""
    st = {"m": np.zeros(shape, F), "steps": 0, "tol": {"m": np.zeros(shape, np.float64)}}
    if len(shape) >= 2:
        r, c = shape[:-1], shape[:-2] + shape[-1:]
        st.update(row=np.zeros(r, F), col=np.zeros(c, F), res_row=np.zeros(r, F), res_col=np.zeros(c, F))
        st["tol"].update(res_row=np.zeros(r, np.float64), res_col=np.zeros(c, np.float64))
    else:
        st["full"] = np.zeros(shape, F)
    return st


def came_step(p, g, state, lr, eps=(1e-30, 1e-16), clip_threshold=1.0, betas=(0.9, 0.999, 0.9999), weight_decay=0.0,
              bf16=False, sum_dtype=np.float64, wrong=None):
    """one step on the fp32 arrays p (parameter value) and g (gradient); `state` (new_state) is updated in place,
    its bounds too.  bf16: the parameter is a bf16 tensor, so the weight-decay add rounds to bf16 before the update
    is subtracted (CAME.py:165-178).  Returns (new fp32 p before the last output rounding, info) with info =
    {"rms_u", "tol_m", "tol_p"}: the bounds of the first moment and of this step's parameter.
    `wrong`: one of the deliberately wrong restatements the bounds must catch: "old_m" (the instability from the
    first moment before its update), "beta3" (beta2 in its place), "eps2" (dropped)."""
    p, g = np.asarray(p, F), np.asarray(g, F)
    eps1, eps2 = F(eps[0]), F(0.0 if wrong == "eps2" else eps[1])
    beta1, beta2, beta3 = betas
    if wrong == "beta3":
        beta3 = beta2
    b1, omb1 = F(beta1), F(1.0 - beta1)
    b2, omb2 = F(beta2), F(1.0 - beta2)
    b3, omb3 = F(beta3), F(1.0 - beta3)
    factored = g.ndim >= 2
    upd = g * g + eps1
    if factored:
        rows, cols = g.shape[-2], g.shape[-1]
        state["row"][...] = OA.fma32(AF._sum(upd, -1, sum_dtype) / F(cols), omb2, state["row"] * b2)
        state["col"][...] = OA.fma32(AF._sum(upd, -2, sum_dtype) / F(rows), omb2, state["col"] * b2)
        rmean = AF._sum(state["row"], -1, sum_dtype) / F(rows)
        u = (AF._rsqrt(state["row"] / rmean[..., None])[..., :, None] * AF._rsqrt(state["col"])[..., None, :]) * g
    else:
        state["full"][...] = OA.fma32(upd, omb2, state["full"] * b2)
        u = AF._rsqrt(state["full"]) * g
    rms_u = AF._rms(u, sum_dtype)
    u = u / np.maximum(rms_u / F(clip_threshold), F(1.0))
    m_old = state["m"].copy()
    state["m"][...] = OA.fma32(u, omb1, m_old * b1)
    m = state["m"]
    d = u - (m_old if wrong == "old_m" else m)
    res = d * d + eps2

    tol = state["tol"]
    e_u = AF.factor_eps(g.shape, False) * U * np.abs(u, dtype=np.float64)
    tol["m"] = float(beta1) * tol["m"] + (1.0 - float(beta1)) * e_u + 4 * U * np.abs(m, dtype=np.float64)
    if factored:
        t_d = e_u + tol["m"] + U * np.abs(d, dtype=np.float64)
        dres = 2 * np.abs(d, dtype=np.float64) * t_d + t_d * t_d + 2 * U * res
        state["res_row"][...] = OA.fma32(AF._sum(res, -1, sum_dtype) / F(cols), omb3, state["res_row"] * b3)
        state["res_col"][...] = OA.fma32(AF._sum(res, -2, sum_dtype) / F(rows), omb3, state["res_col"] * b3)
        for key, ax, n in (("res_row", -1, cols), ("res_col", -2, rows)):
            tol[key] = (float(beta3) * tol[key] + 4 * U * state[key]
                        + (1.0 - float(beta3)) * (dres.mean(ax) + (n - 1) * U * res.mean(ax, dtype=np.float64)))
        res_mean = AF._sum(state["res_row"], -1, sum_dtype) / F(rows)
        s_mean = tol["res_row"].mean(-1) + ((rows - 1) + 4) * U * res_mean
        with np.errstate(invalid="ignore", divide="ignore"):   # the wrong restatement without eps2 divides 0 by 0
            fac = (AF._rsqrt(state["res_row"] / res_mean[..., None])[..., :, None]
                   * AF._rsqrt(state["res_col"])[..., None, :])
            update = fac * m
            rel = 0.5 * ((tol["res_row"] / state["res_row"])[..., :, None] + (s_mean / res_mean)[..., None, None]
                         + (tol["res_col"] / state["res_col"])[..., None, :]) + 8 * U
            tol_update = np.abs(fac, dtype=np.float64) * tol["m"] + np.abs(update, dtype=np.float64) * rel
    else:
        update = m.copy()
        tol_update = tol["m"]
    update = update * F(lr)
    x = p
    if weight_decay != 0:
        x = OA.fma32(p, F(-weight_decay * lr), p)
        if bf16:
            x = OA.rbf(x)
    x = (x - update).astype(F)
    state["steps"] += 1
    tol_p = float(lr) * tol_update + 4 * U * np.abs(x, dtype=np.float64)
    return x, {"rms_u": float(rms_u), "tol_m": tol["m"], "tol_p": tol_p}


def sq_bound(shape, key, steps, ref):
    """bound of a second-moment state (AF.state_eps) around the reference value"""
    n = {"row": shape[-1], "col": shape[-2] if len(shape) >= 2 else 1, "full": 1}[key]
    return AF.state_eps(n, steps) * np.abs(ref)


# ---- the cases tests/golden/make_came_golden.py records and the tests replay ------------------------------------
# The shapes, parameters, gradients and steps are the Adafactor cases' (AF.SHAPES, AF.param0, AF.grad, AF.STEPS).
# CAME has no bias correction: u = g rsqrt(v) with v = (1 - beta2) g^2 in step one has an rms of about
# (1 - beta2)^-0.5 = 32, so clip_threshold 1.0 and 0.3 scale it and 100 does not, whatever the gradient's scale
# (u does not depend on it); the tests assert which.  GSCALE multiplies the gradients all the same.
# lr is 1e-4, not the 1e-3 of a typical run: the update is m rsqrt(res factors), about 0.1 u / (0.9 (1 - beta3)^0.5
# rms(u)) = 11 times the normalised gradient in step one, again whatever the gradient's scale, so lr = 1e-3 moves a
# parameter of magnitude 0.02..0.05 by up to 0.03 a step: elements cross zero, where p - lr u cancels and one bf16
# ulp of the result is far below the fp32 rounding of the operands (measured with lr = 1e-3: fp32-ordered against
# float64 sums up to 128 bf16 ulps apart).  With 1e-4 three steps move an element by at most 0.012 and none comes
# near zero, as _oracle_adafactor.py reasons for its own cases.
CONFIGS = {
    "default": dict(lr=1e-4, weight_decay=0.0, clip_threshold=1.0, betas=(0.9, 0.999, 0.9999)),
    "decay": dict(lr=1e-4, weight_decay=0.01, clip_threshold=1.0, betas=(0.9, 0.999, 0.9999)),   # two roundings
    "clip": dict(lr=1e-4, weight_decay=0.0, clip_threshold=0.3, betas=(0.9, 0.999, 0.9999)),     # clip active
    "noclip": dict(lr=1e-4, weight_decay=0.01, clip_threshold=100.0, betas=(0.9, 0.999, 0.9999)),   # and not
    "betas": dict(lr=1e-4, weight_decay=0.0, clip_threshold=1.0, betas=(0.8, 0.99, 0.999)),
}
GSCALE = {"clip": 4.0}   # gradient multiplier of a configuration (1 otherwise; a power of two keeps bf16 values exact)


SAMPLE = 256   # the golden keeps at most this many elements of an array (evenly strided, as AF.sample strides)


def grad(cname, name, shape, k):
    return AF.grad(name, shape, k) * F(GSCALE.get(cname, 1.0))


def sample(x):
    x = np.asarray(x).reshape(-1)
    return x[::max(1, -(-x.size // SAMPLE))]
