"""NumPy float64 restatement of one sampler step -- classifier-free guidance, CFG rescale, a DDIM step at eta = 0
(modules/modelSampler/StableDiffusionXLSampler.py:156-172 with the DDIMScheduler of modules/util/create.py:1255-1266:
leading spacing, steps_offset 1, set_alpha_to_one False, clip_sample False) -- of the DDIM timestep table and of the
decoder output's 8-bit conversion, with the fp32 error bound the tests hold csrc/sampler.hip to.  DDIM and the rescale
(arXiv 2305.08891, section 3.4) are restated from the published formulas; diffusers is not installed here.

    p  = neg + cfg (pos - neg)
    p' = p f,  f = 1 + r (std(pos) / std(p) - 1)        (= r std(pos) / std(p) + (1 - r); r = cfg_rescale, f = 1 at 0)
    epsilon:       x0 = (x - s1_t p') / sa_t            e = p'
    v_prediction:  x0 = sa_t x - s1_t p'                e = sa_t p' + s1_t x
    x_prev = sa_p x0 + s1_p e
sa = sqrt(alphas_cumprod[.]), s1 = sqrt(1 - alphas_cumprod[.]); the caller passes the fp32 table entries the kernel
reads, so the tables carry no error of their own.  std is the unbiased standard deviation over one sample's real
elements; a sample whose guided prediction is constant (std(p) = 0) keeps f = 1.

Bound (u = 2^-24, first order).  The kernel evaluates every line above in fp32 with one rounding per written
operation (no contraction), so a result z = a op b carries |dz| <= (what da and db carry into z) + u |z|:
    d  = pos - neg     E_d  = u |d|
    m  = cfg d         E_m  = |cfg| E_d + u |m|
    p  = neg + m       E_p  = E_m + u |p|
    p' = p f           E_p' = |f| E_p + |p| E_f + u |p'|      (skipped at r = 0: p' = p)
    epsilon:  a = s1_t p'   E_a = s1_t E_p' + u |a| ;  b = x - a   E_b = E_a + u |b| ;  x0 = b / sa_t
              E_x0 = E_b / sa_t + u |x0| ;  E_e = E_p'
    v:        a1 = sa_t x, a2 = s1_t p', x0 = a1 - a2    E_x0 = u |a1| + s1_t E_p' + u |a2| + u |x0|
              e1 = sa_t p', e2 = s1_t x, e = e1 + e2     E_e  = sa_t E_p' + u |e1| + u |e2| + u |e|
    c = sa_p x0, g = s1_p e, x_prev = c + g              E = sa_p E_x0 + u |c| + s1_p E_e + u |g| + u |x_prev|
The factor f.  The kernel forms p in double from the bf16 inputs (products of floats are exact in double) and sums
p, p^2, pos, pos^2 in double, v = 2^-53: a sum of n terms is within (n - 1) v of the sum of their magnitudes, so the
variance (S2 - S1^2 / n) / (n - 1) is within about (n + 3) v k of itself with k = S2 / (S2 - S1^2 / n) the
cancellation between the two terms, a standard deviation within half of that, and the ratio within the sum of the
two; f is then rounded to fp32 once:
    E_f = r ratio ((n + 3) v (k_p + k_pos) / 2 + 4 v) + u |f|
"""
import numpy as np

U = 2.0 ** -24
V = 2.0 ** -53


def f64(x):
    return np.asarray(x, dtype=np.float64)


def alphas_cumprod(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012):
    """scaled_linear betas in float64 (the known-answer tests need the schedule's shape, not its last bits)"""
    betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=np.float64) ** 2
    return np.cumprod(1.0 - betas)


def ddim_table(steps, num_train_timesteps=1000, force_last_timestep=False):
    """[(t, index of alpha_prev)]: leading spacing with steps_offset 1; prev = t - N // steps, and a prev below 0
    takes final_alpha_cumprod = alphas_cumprod[0] (set_alpha_to_one False).  force_last_timestep prepends N - 1."""
    ratio = num_train_timesteps // steps
    ts = [int(round(i * ratio)) + 1 for i in range(steps)][::-1]
    if force_last_timestep:
        ts = [num_train_timesteps - 1] + ts
    return [(t, max(t - ratio, 0)) for t in ts]


def _std(a, axes):
    a = f64(a)
    n = a[0].size
    mean = a.mean(axis=axes, keepdims=True)
    return np.sqrt(((a - mean) ** 2).sum(axis=axes, keepdims=True) / (n - 1))


def _ratio(pos, p, axes):
    """std(pos) / std(p); 1 for a sample whose p is constant (nothing to rescale to: the kernel's guard)"""
    sp = _std(p, axes)
    return np.where(sp > 0, _std(pos, axes) / np.where(sp > 0, sp, 1.0), 1.0)


def _cancel(a, axes):
    """k = S2 / (S2 - S1^2 / n) of the one-pass variance"""
    a = f64(a)
    n = a[0].size
    s2 = (a * a).sum(axis=axes, keepdims=True)
    s1 = a.sum(axis=axes, keepdims=True)
    den = s2 - s1 * s1 / n
    return np.where(den > 0, s2 / np.where(den > 0, den, 1.0), np.inf)


def rescale_factor(neg, pos, cfg_scale, cfg_rescale):
    """f per sample, shaped [B, 1, ..]; exactly 1 when std(pos) == std(p), which cfg_scale = 1 gives"""
    neg, pos = f64(neg), f64(pos)
    axes = tuple(range(1, neg.ndim))
    p = neg + float(cfg_scale) * (pos - neg)
    return 1.0 + float(cfg_rescale) * (_ratio(pos, p, axes) - 1.0)


def step(neg, pos, x, cfg_scale, cfg_rescale, v_pred, sa_t, s1_t, sa_p, s1_p):
    """neg, pos, x: [B, ...] real elements only.  -> (x_prev float64, bound)"""
    neg, pos, x = f64(neg), f64(pos), f64(x)
    cfg, r = float(cfg_scale), float(cfg_rescale)
    sa_t, s1_t, sa_p, s1_p = float(sa_t), float(s1_t), float(sa_p), float(s1_p)
    axes = tuple(range(1, neg.ndim))
    n = neg[0].size
    d = pos - neg
    E = U * np.abs(d)
    m = cfg * d
    E = abs(cfg) * E + U * np.abs(m)
    p = neg + m
    E = E + U * np.abs(p)
    if r > 0:
        ratio = _ratio(pos, p, axes)
        f = 1.0 + r * (ratio - 1.0)
        Ef = r * ratio * ((n + 3) * V * (_cancel(p, axes) + _cancel(pos, axes)) / 2 + 4 * V) + U * np.abs(f)
        pp = p * f
        E = np.abs(f) * E + np.abs(p) * Ef + U * np.abs(pp)
        p = pp
    if v_pred:
        a1, a2 = sa_t * x, s1_t * p
        x0 = a1 - a2
        E0 = U * np.abs(a1) + s1_t * E + U * np.abs(a2) + U * np.abs(x0)
        e1, e2 = sa_t * p, s1_t * x
        e = e1 + e2
        Ee = sa_t * E + U * np.abs(e1) + U * np.abs(e2) + U * np.abs(e)
    else:
        a = s1_t * p
        b = x - a
        x0 = b / sa_t
        E0 = (s1_t * E + U * np.abs(a) + U * np.abs(b)) / sa_t + U * np.abs(x0)
        e, Ee = p, E
    c, g = sa_p * x0, s1_p * e
    xp = c + g
    return xp, sa_p * E0 + U * np.abs(c) + s1_p * Ee + U * np.abs(g) + U * np.abs(xp)


def rgb8(x):
    """round(clamp(x / 2 + 0.5, 0, 1) * 255), ties to even, in float64 like the kernel"""
    return np.rint(np.clip(f64(x) * 0.5 + 0.5, 0.0, 1.0) * 255.0).astype(np.uint8)


def bf16_bits_to_f64(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bf16_round_bits(x32):
    """fp32 -> the nearest bf16 (ties to even) as uint16 bits"""
    b = np.asarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
