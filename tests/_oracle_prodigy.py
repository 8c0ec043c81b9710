"""NumPy float64 restatement of the Prodigy step (Mishchenko and Defazio) in the form the reference asks of
prodigyopt.Prodigy (modules/util/create.py:863-881).  That package is not in the reference tree and was not available,
so this file IS the contract of csrc/prodigy.hip and util/optimizer/prodigy_fused.py; it is not pinned to any run of
the package, and no golden file "from the reference" exists for this optimizer.

One step over the whole store (a list of tensors), g after the pending clip:
   1  lr common to all groups                          2  bc = sqrt(1 - beta2^(k+1)) / (1 - beta1^(k+1)) or 1
   3  dlr = d lr bc (d from before the step)           4  lr == 0: nothing changes, k included
   5  coupled decay: g += weight_decay p
   6  num += g (p0 - p);  m = beta1 m + d (1 - beta1) g (beta1 > 0);  v = beta2 v + d d (1 - beta2) g g
      s = beta3 s + a g, a = (d / d0) dlr or (d / d0) d (safeguard_warmup);  den += |s|
   7  d_numerator = beta3 d_numerator + (d / d0) dlr num;  d_denom = den
   8  d_denom == 0: stop (states of 6 stay, no update, k unchanged)
   9  d_hat = d_coef d_numerator / d_denom;  d == d0: d = max(d, d_hat);  d_max = max(d_max, d_hat)
      d = min(d_max, d growth_rate)
  10  decoupled decay: p += (-weight_decay dlr) p;  p -= dlr m / (sqrt(v) + d eps), new d, old dlr;  beta1 == 0: d g for m
  11  k += 1
Precision: m, v, s, p0 fp32; the scalars and both sums float64; p0 - p is an fp32 difference, its product with g and
the sums are float64; every fp32 operation is one rounding in the order written (t = a * b, then t + c); a
per-element coefficient is formed in float64 and rounded to fp32 once.

The bounds travel with the result, in float64 (U = 2^-24, E = 2^-53).  Both sides evaluate the same fp32 expressions,
so they can differ only where a float64 scalar differs: bc goes through pow() (two libraries), which can move an fp32
coefficient by one ulp (2 U relative); in a free run d itself differs by rel_d = tol_d / d and the parameters by
tol_p.  Counting one U per fp32 rounding of either side on top of that:
  g (coupled decay)      tol_g = weight_decay tol_p + 2 U |g|               (0 in the decoupled form)
  diff = p0 - p          tol_diff = tol_p + U |diff|
  num                    sum(|g| tol_diff + tol_g |diff|) + (n - 1) E sum|g diff|: the products of two fp32 values are
                         exact in float64, so only the order of the n-term sum differs
  m                      tol_m <- beta1 tol_m + U |t1| + (3 U + rel_d) |t2| + U |m| + c_m tol_g    (t1 = beta1 m, t2 = c_m g)
  v                      tol_v <- beta2 tol_v + U |t3| + (4 U + 2 rel_d) |t4| + U |v| + 2 |c_v g| tol_g
  s                      tol_s <- beta3 tol_s + U |t5| + (3 U + 2 rel_d + rel_bc) |t6| + U |s| + a tol_g
  den                    sum(tol_s) + (n - 1) E sum|s|
  bc                     rel_bc = E (b2p / (1 - b2p) + 2 b1p / (1 - b1p) + 4), b.p = beta.^(k+1): pow within 2 ulps on
                         either side, amplified by the subtraction from 1 (half of it under the square root)
  d_numerator            beta3 tol + A (tol_num + (2 rel_d + rel_bc + 4 E) |num|) + 3 E (|beta3 d_numerator| + |A num|),
                         A = (d / d0) dlr
  d_hat                  d_coef (tol_dnum / den + |d_numerator| tol_den / den^2) + 2 E |d_hat|
  d, d_max               max and min move by no more than their arguments do: the largest of the argument bounds
  denom = sqrt(v) + d eps  tol_v / (2 sqrt(v)) (sqrt(tol_v) where v = 0) + U sqrt(v) + U denom + d eps (rel_d' + 2 U)
  u = dlr m / denom      |u| (rel_dlr + 4 U) + dlr tol_m / denom + |u| tol_denom / denom
  x (decoupled decay)    tol_p (1 + |w|) + |w x| (rel_dlr + 3 U) + U |x|,  w = -weight_decay dlr
  p                      tol_x + tol_u + U |p|
Fed the device's parameters and scalars before every step (rel_d = tol_p = 0) these are one step's bounds; in a free
run they compound through `scalars` and the returned tol_p.
"""
import math

import numpy as np

F = np.float32
U = 2.0 ** -24
E = 2.0 ** -53

DEFAULTS = dict(beta1=0.9, beta2=0.999, beta3=None, eps=1e-8, weight_decay=0.0, decouple=True,
                use_bias_correction=False, safeguard_warmup=False, d0=1e-6, d_coef=1.0, growth_rate=float("inf"))


def new_state(shape):
    z = {k: np.zeros(shape, F) for k in ("m", "v", "s")}
    z["p0"] = None
    z["tol"] = {k: np.zeros(shape, np.float64) for k in ("m", "v", "s")}
    return z


def new_scalars(d0=1e-6):
    return dict(d=d0, d_max=d0, d_numerator=0.0, d_denom=0.0, d_hat=d0, k=0, tol_d=0.0, tol_dmax=0.0, tol_dnum=0.0)


def scalars_from(ds):
    """the device's scalars (FusedProdigy.d_state) as the oracle's, with no error carried"""
    sc = {k: ds[k] for k in ("d", "d_max", "d_numerator", "d_denom", "d_hat", "k")}
    sc.update(tol_d=0.0, tol_dmax=0.0, tol_dnum=0.0)
    return sc


def _a64(x):
    return np.abs(np.asarray(x, np.float64))


def prodigy_step(params, grads, states, sc, lr, tol_p=None, **hyper):
    """one step on the lists of fp32 arrays `params` and `grads` (the whole store); `states` (new_state per tensor) and
    the scalars `sc` (new_scalars) are updated in place, their bounds too.  tol_p: per-tensor bounds the parameters
    come with (a free run), or None.  Returns (xs, info): xs the new fp32 parameters before any output rounding (the
    inputs when the step updates nothing), info = {"num", "den", "tol_num", "tol_den", "skipped", "tol_p": [...],
    "dlr", "noop"}."""
    H = dict(DEFAULTS, **hyper)
    beta1, beta2 = float(H["beta1"]), float(H["beta2"])
    beta3 = math.sqrt(beta2) if H["beta3"] is None else float(H["beta3"])
    eps, wd, d0 = float(H["eps"]), float(H["weight_decay"]), float(H["d0"])
    params = [np.asarray(p, F) for p in params]
    grads = [np.asarray(g, F) for g in grads]
    tol_p = [np.zeros(p.shape) for p in params] if tol_p is None else [np.asarray(t, np.float64) for t in tol_p]
    d, k = float(sc["d"]), int(sc["k"])
    rel_d = sc["tol_d"] / d
    bc, rel_bc = 1.0, 0.0
    if H["use_bias_correction"]:
        b1p, b2p = beta1 ** (k + 1), beta2 ** (k + 1)
        bc = math.sqrt(1.0 - b2p) / (1.0 - b1p)
        rel_bc = E * (b2p / (1.0 - b2p) + 2.0 * b1p / (1.0 - b1p) + 4.0)
    dlr = d * lr * bc
    info = {"dlr": dlr, "noop": lr == 0, "skipped": False, "num": 0.0, "den": 0.0, "tol_num": 0.0, "tol_den": 0.0,
            "tol_p": tol_p}
    if lr == 0:
        return params, info
    rel_dlr = rel_d + rel_bc + 2 * E
    r = d / d0
    A = r * dlr
    b1, b2, b3 = F(beta1), F(beta2), F(beta3)
    c_m, c_v = F(d * (1.0 - beta1)), F(d * d * (1.0 - beta2))
    a = F(r * d if H["safeguard_warmup"] else A)
    rel_a = 2 * rel_d + (0.0 if H["safeguard_warmup"] else rel_bc)
    coupled = (not H["decouple"]) and wd != 0
    num = den = abs_num = abs_den = tol_num = tol_den = 0.0
    n = 0
    gs, tol_gs = [], []
    for p, g, st, tp in zip(params, grads, states, tol_p):
        tol_g = np.zeros(p.shape)
        if coupled:
            t = F(wd) * p
            g = g + t
            tol_g = wd * tp + 2 * U * _a64(g)
        gs.append(g)
        tol_gs.append(tol_g)
        if st["p0"] is None:
            st["p0"] = p.copy()
        diff = st["p0"] - p
        term = g.astype(np.float64) * diff.astype(np.float64)
        num += float(term.sum())
        abs_num += float(np.abs(term).sum())
        tol_num += float((_a64(g) * (tp + U * _a64(diff)) + tol_g * _a64(diff)).sum())
        tol = st["tol"]
        if beta1 > 0:
            t1, t2 = b1 * st["m"], c_m * g
            st["m"] = t1 + t2
            tol["m"] = (beta1 * tol["m"] + U * _a64(t1) + (3 * U + rel_d) * _a64(t2) + U * _a64(st["m"])
                        + float(c_m) * tol_g)
        t3, t4 = b2 * st["v"], (c_v * g) * g
        st["v"] = t3 + t4
        tol["v"] = (beta2 * tol["v"] + U * _a64(t3) + (4 * U + 2 * rel_d) * _a64(t4) + U * _a64(st["v"])
                    + 2 * _a64(c_v * g) * tol_g)
        t5, t6 = b3 * st["s"], a * g
        st["s"] = t5 + t6
        tol["s"] = (beta3 * tol["s"] + U * _a64(t5) + (3 * U + rel_a) * _a64(t6) + U * _a64(st["s"])
                    + float(a) * tol_g)
        den += float(_a64(st["s"]).sum())
        abs_den = den
        tol_den += float(tol["s"].sum())
        n += p.size
    tol_num += (n - 1) * E * abs_num
    tol_den += (n - 1) * E * abs_den
    info.update(num=num, den=den, tol_num=tol_num, tol_den=tol_den)
    dn_old = sc["d_numerator"]
    sc["d_numerator"] = beta3 * dn_old + A * num
    sc["tol_dnum"] = (beta3 * sc["tol_dnum"] + A * (tol_num + (2 * rel_d + rel_bc + 4 * E) * abs(num))
                      + 3 * E * (abs(beta3 * dn_old) + abs(A * num)))
    sc["d_denom"] = den
    if den == 0:
        info["skipped"] = True
        return params, info
    d_hat = H["d_coef"] * sc["d_numerator"] / den
    tol_dhat = H["d_coef"] * (sc["tol_dnum"] / den + abs(sc["d_numerator"]) * tol_den / den ** 2) + 2 * E * abs(d_hat)
    tol_d = sc["tol_d"]
    if d == d0:
        d = max(d, d_hat)
        tol_d = max(tol_d, tol_dhat)
    sc["d_max"] = max(sc["d_max"], d_hat)
    sc["tol_dmax"] = max(sc["tol_dmax"], tol_dhat)
    grown = d * H["growth_rate"]
    tol_grown = 0.0 if math.isinf(grown) else tol_d * H["growth_rate"] + E * grown
    d = min(sc["d_max"], grown)
    sc["tol_d"] = max(sc["tol_dmax"], tol_grown)
    sc["d"], sc["d_hat"], sc["k"] = d, d_hat, k + 1
    rel_dn = sc["tol_d"] / d
    # step 10
    dlrf, de, df = F(dlr), F(d * eps), F(d)
    wdd = F(-(wd * dlr)) if H["decouple"] and wd != 0 else F(0)
    xs, tols = [], []
    for p, g, tol_g, st, tp in zip(params, gs, tol_gs, states, tol_p):
        if beta1 > 0:
            m, tol_m = st["m"], st["tol"]["m"]
        else:
            m = df * g
            tol_m = _a64(m) * (rel_dn + 3 * U) + float(df) * tol_g
        v64 = st["v"].astype(np.float64)
        root = np.sqrt(st["v"])
        denom = root + de
        tv = st["tol"]["v"]
        with np.errstate(divide="ignore", invalid="ignore"):
            t_root = np.where(v64 > 0, tv / (2 * np.sqrt(v64)), np.sqrt(tv))
        tol_denom = t_root + U * _a64(root) + U * _a64(denom) + float(de) * (rel_dn + 2 * U)
        u = (dlrf * m) / denom
        tol_u = _a64(u) * (rel_dlr + 4 * U) + float(dlrf) * tol_m / _a64(denom) + _a64(u) * tol_denom / _a64(denom)
        x, tol_x = p, tp
        if wdd != 0:
            t = wdd * x
            x = x + t
            tol_x = tp * (1 + abs(float(wdd))) + _a64(t) * (rel_dlr + 3 * U) + U * _a64(x)
        x = x - u
        xs.append(x.astype(F))
        tols.append(tol_x + tol_u + U * _a64(x))
    info["tol_p"] = tols
    return xs, info


# ---- the cases tests/test_prodigy_gpu.py runs and tests/test_prodigy_oracle.py checks for rounding ties ---------
# The stores are _oracle_adafactor.SHAPES with _oracle_adafactor.param0 (magnitudes in [0.02, 0.05), bf16-exact).
# The gradient of step k is grad(name, shape, 0) * 2^k: one direction, growing, so <g, p0 - p> is positive from the
# second step on and d moves.  lr is 1.0, as Prodigy is run.  d0 = 2e-4, not the default 1e-6: in step one
# m / sqrt(v) = (1 - beta1) / sqrt(1 - beta2) = 3.16 for every element, so a parameter moves by 3.16 d0, which at 1e-6
# is a fiftieth of a bf16 ulp of these values and would leave a round-to-nearest bf16 store untouched; at 2e-4 it is
# 2.6 to 5 ulps.  d leaves d0 in step two through the d == d0 branch (which growth_rate does not cap) and growth_rate
# = 2 binds in step three.  Three steps move an element by less than 4e-3 of its 0.02 or more, so none comes near
# zero, where the one-ulp rule of the bf16 comparison cannot hold (_oracle_came.py has the argument);
# tests/test_prodigy_oracle.py asserts that d moved and that no element changed sign.
GPU_CASES = {
    "decoupled": dict(weight_decay=0.01, d0=2e-4, growth_rate=2.0),
    "coupled_bc_safeguard": dict(weight_decay=0.01, decouple=False, use_bias_correction=True, safeguard_warmup=True,
                                 d0=2e-4, growth_rate=2.0, d_coef=8.0),
}
GPU_STEPS = 3


def case_grad(name, shape, k):
    import _oracle_adafactor as AF
    return AF.grad(name, shape, 0) * F(2.0 ** k)
