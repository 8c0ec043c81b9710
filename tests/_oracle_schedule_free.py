"""NumPy restatement of schedule-free AdamW in the form the reference asks of schedulefree.AdamWScheduleFree
(modules/util/create.py:752-767, the non-foreach path of step() in 1.4.0) and of its eval() / train() switches.  That
package is not in the reference tree and was not available, so this file IS the contract of csrc/schedule_free.hip and
util/optimizer/schedule_free_fused.py; it is not pinned to any run of the package.

Per group, all scalars in Python floats (float64), k starting at 0 (group_scalars):
    sched = (k + 1) / warmup_steps if k < warmup_steps else 1;   bc2 = 1 - beta2^(k+1)
    lr = group lr * sched;  lr_max = max(lr, lr_max) (starts at -1);  weight = (k + 1)^r lr_max^weight_lr_power
    weight_sum += weight;  ckp1 = weight / weight_sum (0 when weight_sum == 0);  a_y = lr (beta1 (1 - ckp1) - 1)
Per element (sf_step), g after the pending clip, z = y on the first step:
    v = beta2 v + (1 - beta2) g g;  gn = g / (sqrt(v / bc2) + eps) + weight_decay y
    y = y + ckp1 (z - y);  y = y + a_y gn;  z = z - lr gn
eval():  x = y + (1 - 1/beta1) (z - y);   train():  y = x + (1 - beta1) (z - x)         (sf_swap)

`sf_step_f64` and `swap_f64` are these formulas in float64 and nothing else.  `sf_step` and `sf_swap` apply the fp32
roundings of the device path, each named where it happens: the scalars lr, a_y, ckp1, beta2, 1 - beta2, 1 / bc2, eps
and weight_decay are rounded to fp32 once (v / bc2 is the product v * fp32(1 / bc2)); every fp32 operation is one
rounding in the order written (t = a * b, then t + c: no fused multiply-add); sqrt and the division are correctly
rounded; z and v are fp32 whatever the store.

The bounds travel with the result, in float64 (U = 2^-24).  Both sides evaluate the same fp32 expressions from the same
fp32 scalars, so with IEEE arithmetic they agree exactly; the bounds say how far a side may be whose every fp32
operation is within one U (relative) of the exact result of its own operands, and they carry the states' bounds
forward.  With r the result of an operation and tol_a the bound of an operand:
  g (clipped)      tol_g  = U |g|                                    (0 without a clip)
  t1 = beta2 v     tol_t1 = beta2 tol_v + U |t1|
  t2 = (c g) g     tol_t2 = 2 U |t2| + 2 |c g| tol_g
  v  = t1 + t2     tol_v  = tol_t1 + tol_t2 + U |v|
  s  = v ibc       tol_s  = ibc tol_v + U |s|
  root = sqrt(s)   tol_r  = tol_s / (2 sqrt(s))  (sqrt(tol_s) where s = 0)  + U root
  den = root + eps tol_d  = tol_r + U den
  q  = g / den     tol_q  = tol_g / den + |q| tol_d / den + U |q|
  wy = wd y        tol_wy = wd tol_y + U |wy|
  gn = q + wy      tol_gn = tol_q + tol_wy + U |gn|
  dz = z - y       tol_dz = tol_z + tol_y + U |dz|
  t3 = ckp1 dz     tol_t3 = ckp1 tol_dz + U |t3|
  y1 = y + t3      tol_y1 = tol_y + tol_t3 + U |y1|
  t4 = a_y gn      tol_t4 = |a_y| tol_gn + U |t4|
  y2 = y1 + t4     tol_y2 = tol_y1 + tol_t4 + U |y2|
  t5 = lr gn       tol_t5 = lr tol_gn + U |t5|
  z' = z - t5      tol_z' = tol_z + tol_t5 + U |z'|
  swap: d = z - p, t = w d, p' = p + t:   tol_p' = tol_p + |w| (tol_z + tol_p + U |d|) + U |t| + U |p'|
A bf16 store rounds y2 (to nearest, or stochastically to one of its two bf16 neighbours); the tests compare bit
patterns there.  round_trip_bound is the distance train(eval(y)) may have from y on a bf16 store without master.
"""
import numpy as np

F = np.float32
U = 2.0 ** -24

DEFAULTS = dict(beta1=0.9, beta2=0.999, weight_decay=1e-2, eps=1e-8, r=0, weight_lr_power=2.0, foreach=False)


def new_group(lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, warmup_steps=0, r=0, weight_lr_power=2.0):
    return dict(lr=lr, betas=(beta1, beta2), eps=eps, weight_decay=weight_decay, warmup_steps=warmup_steps, r=r,
                weight_lr_power=weight_lr_power, k=0, weight_sum=0.0, lr_max=-1.0, scheduled_lr=0.0)


def group_scalars(g):
    """the host part of one step; updates lr_max, weight_sum, scheduled_lr and k of `g` in place"""
    k = g["k"]
    beta1, beta2 = g["betas"]
    sched = (k + 1) / g["warmup_steps"] if k < g["warmup_steps"] else 1.0
    bc2 = 1 - beta2 ** (k + 1)
    lr = g["lr"] * sched
    g["scheduled_lr"] = lr
    g["lr_max"] = max(lr, g["lr_max"])
    weight = ((k + 1) ** g["r"]) * (g["lr_max"] ** g["weight_lr_power"])
    g["weight_sum"] += weight
    ckp1 = weight / g["weight_sum"] if g["weight_sum"] != 0 else 0.0
    g["k"] = k + 1
    return dict(lr=lr, ckp1=ckp1, a_y=lr * (beta1 * (1 - ckp1) - 1), bc2=bc2, beta2=beta2, eps=g["eps"],
                weight_decay=g["weight_decay"], weight=weight)


def sf_step_f64(y, g, z, v, sc):
    """the step in float64, no rounding anywhere: returns (y, z, v).  sc may carry one_minus_beta2 and inv_bc2 (the
    device's fp32 scalars) in place of the values derived from beta2 and bc2."""
    y, g, z, v = (np.asarray(a, np.float64) for a in (y, g, z, v))
    v = sc["beta2"] * v + sc.get("one_minus_beta2", 1 - sc["beta2"]) * g * g
    scaled = v * sc["inv_bc2"] if "inv_bc2" in sc else v / sc["bc2"]
    gn = g / (np.sqrt(scaled) + sc["eps"]) + sc["weight_decay"] * y
    y = y + sc["ckp1"] * (z - y)
    y = y + sc["a_y"] * gn
    z = z - sc["lr"] * gn
    return y, z, v


def swap_f64(p, z, w):
    p, z = np.asarray(p, np.float64), np.asarray(z, np.float64)
    return p + w * (z - p)


def eval_weight(beta1):
    return 1 - 1 / beta1


def train_weight(beta1):
    return 1 - beta1


def _a(x):
    return np.abs(np.asarray(x, np.float64))


def zeros_tol(shape):
    return {"z": np.zeros(shape), "v": np.zeros(shape)}


def sf_step(y, g, z, v, sc, tol=None, tol_y=None, clipped=False):
    """one step on fp32 arrays with the device's fp32 roundings.  z None: the first step (z = y).  g: the gradient
    after the clip (clipped: it is the fp32 product g * coef, one rounding).  tol: {"z", "v"} bounds of the states
    coming in (zeros_tol), updated in place; tol_y: bound of y coming in.  Returns (y2, z2, v2, tol_y2): fp32 arrays
    before any output rounding of y, and the bound of y2."""
    y, g, v = np.asarray(y, F), np.asarray(g, F), np.asarray(v, F)
    tol = zeros_tol(y.shape) if tol is None else tol
    tol_y = np.zeros(y.shape) if tol_y is None else tol_y
    z = y.copy() if z is None else np.asarray(z, F)
    # the scalars, rounded to fp32 once
    lr, a_y, ckp1 = F(sc["lr"]), F(sc["a_y"]), F(sc["ckp1"])
    b2, omb2, ibc = F(sc["beta2"]), F(1 - sc["beta2"]), F(1 / sc["bc2"])
    eps, wd = F(sc["eps"]), F(sc["weight_decay"])
    tol_g = U * _a(g) if clipped else np.zeros(y.shape)
    t1 = b2 * v                                   # one rounding
    cg = omb2 * g                                 # one rounding
    t2 = cg * g                                   # one rounding
    v2 = t1 + t2                                  # one rounding
    tol_v = float(b2) * tol["v"] + U * _a(t1) + 2 * U * _a(t2) + 2 * _a(cg) * tol_g + U * _a(v2)
    s = v2 * ibc                                  # one rounding
    tol_s = float(ibc) * tol_v + U * _a(s)
    root = np.sqrt(s)                             # correctly rounded
    s64 = s.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        tol_r = np.where(s64 > 0, tol_s / (2 * np.sqrt(s64)), np.sqrt(tol_s)) + U * _a(root)
    den = root + eps                              # one rounding
    tol_d = tol_r + U * _a(den)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = g / den                               # correctly rounded
        tol_q = np.where(_a(den) > 0, tol_g / _a(den) + _a(q) * tol_d / _a(den), 0.0) + U * _a(q)
    wy = wd * y                                   # one rounding
    gn = q + wy                                   # one rounding
    tol_gn = tol_q + float(wd) * tol_y + U * _a(wy) + U * _a(gn)
    dz = z - y                                    # one rounding
    t3 = ckp1 * dz                                # one rounding
    y1 = y + t3                                   # one rounding
    tol_y1 = tol_y + float(ckp1) * (tol["z"] + tol_y + U * _a(dz)) + U * _a(t3) + U * _a(y1)
    t4 = a_y * gn                                 # one rounding
    y2 = y1 + t4                                  # one rounding
    tol_y2 = tol_y1 + abs(float(a_y)) * tol_gn + U * _a(t4) + U * _a(y2)
    t5 = lr * gn                                  # one rounding
    z2 = z - t5                                   # one rounding
    tol["z"] = tol["z"] + float(lr) * tol_gn + U * _a(t5) + U * _a(z2)
    tol["v"] = tol_v
    return y2, z2, v2, tol_y2


def sf_swap(p, z, w, tol_p=None, tol_z=None):
    """p + w (z - p) with the device's fp32 roundings (w rounded to fp32 once); returns (p', tol_p')"""
    p, z = np.asarray(p, F), np.asarray(z, F)
    tol_p = np.zeros(p.shape) if tol_p is None else tol_p
    tol_z = np.zeros(p.shape) if tol_z is None else tol_z
    wf = F(w)
    d = z - p                                     # one rounding
    t = wf * d                                    # one rounding
    out = p + t                                   # one rounding
    return out, tol_p + abs(float(wf)) * (tol_z + tol_p + U * _a(d)) + U * _a(t) + U * _a(out)


def bf16_ulp(x):
    """spacing of bf16 at |x| (normal range)"""
    x = _a(x)
    return np.ldexp(1.0, np.frexp(np.where(x > 0, x, 1e-30))[1] - 8)


def round_trip_bound(y, x, beta1, tol_swap):
    """|train(eval(y)) - y| on a bf16 store rounded to nearest: x carries half a bf16 ulp, train() forms
    beta1 x + (1 - beta1) z, which keeps beta1 of it, and rounds once more; tol_swap: the fp32 bounds of both swaps"""
    return beta1 * 0.5 * bf16_ulp(x) + 0.5 * bf16_ulp(y) + tol_swap


# ---- the store tests/test_schedule_free_gpu.py runs ---------------------------------------------------------------
# sizes 1, 7, 8, 9 (group a: its end, element 33, lies inside the vector [32, 40)), 4099 and 70001 (group b; the last
# crosses the 65536-element norm chunk).  Parameters are _oracle_adafactor.param0 (magnitudes in [0.02, 0.05),
# bf16-exact); the gradient of step k is a hash scaled 10^-2, the same magnitude every step, so that gn is of order one
# and a step moves a parameter by about lr: at the learning rates below several bf16 ulps of 0.02 .. 0.05, and five
# steps stay far from zero.
SHAPES = [("s1", (1,)), ("s7", (7,)), ("s8", (8,)), ("s9", (3, 3)), ("s4099", (4099,)), ("s70001", (70001,))]
SPLIT = 4
GROUP_CFG = [dict(lr=2e-3, weight_decay=0.01), dict(lr=1e-3, weight_decay=0.1)]
LR_FACTORS = [0.25, 0.5, 1.0, 0.8, 0.6]   # a scheduler-like multiplier on both groups' lr, one per step
STEPS = 5


def case_grad(name, shape, k):
    import _oracle_adafactor as AF
    return AF.hashed(shape, 5000 + 17 * k + sum(map(ord, name)), 1e-2)
