"""NumPy restatement of the 8-bit AdamW the reference asks of bnb.optim.AdamW8bit (modules/util/create.py:553-566):
Dettmers et al., "8-bit Optimizers via Block-wise Quantization", the two-state block-wise variant with blocks of 256
and dynamic-tree codebooks.  bitsandbytes is not in the reference tree and was not available, so this file IS the
contract of csrc/adamw8bit.hip and util/optimizer/adamw8bit_fused.py; it is not pinned to any run of the package.

Codebooks (dynamic_map): 256 ascending fp32 values.  Seven levels i = 0 .. 6 of scale 10^(i - 6); level i holds the
centres of 2^i (signed) or 2^(i + 1) (unsigned) equal cells of [0.1, 1] times the scale, the signed map also their
negatives; 0 and 1 complete each map.  Built in float64, rounded to fp32 once.  The signed map is symmetric except
for 1, whose negative is absent.

encode(x) = the number of midpoints mid[i] = (map[i] + map[i + 1]) * 0.5 (fp32, two roundings) strictly below x: the
nearest codebook value, and a value exactly on a midpoint takes the LOWER code.  decode(c) = map[c].

Per group, scalars in Python floats, step from 1, each rounded to fp32 once (group_scalars):
    bc1 = 1 - beta1^step;  bc2 = 1 - beta2^step
    step_size = -lr sqrt(bc2) / bc1;  eps_c = sqrt(bc2) eps;  wd_factor = 1 - lr weight_decay
Per block of 256 elements that starts at the tensor's first element (step_8bit), g after the pending clip:
    m = map1[code1] * absmax1;  v = map2[code2] * absmax2
    t1 = beta1 m; t2 = (1 - beta1) g; m = t1 + t2
    t3 = beta2 v; t4 = ((1 - beta2) g) g; v = t3 + t4
    den = sqrt(v) + eps_c;  q = m / den;  t5 = step_size q;  p = p + t5;  p = p wd_factor
    absmax1 = max |m|;  absmax2 = max v           (over the block's elements; the maximum is exact in any order)
    code1 = encode1(m / absmax1);  code2 = encode2(v / absmax2)        (0 where the absmax is 0: no 0 / 0)
The update uses the unquantised fp32 m and v; the weight decay multiplies after the update, as recalled of the
package's kernel.  A tensor below min_8bit_size takes the same update on fp32 m and v (step_f32).

Every operation is one float32 rounding in the order written (no fused multiply-add); sqrt and the two divisions are
IEEE correctly rounded on both sides.  No operation had to be declared unpinned: UNPINNED is empty, the oracle flags
no element, and the GPU must reproduce codes, absmax and fp32 parameters bit for bit.

track_bound: how far the decoded moments may be from an unquantised float64 AdamW on the same gradients.  With
H = max(map[i + 1] - map[i]) / 2, the largest half gap of the codebook relative to the block's maximum (1 in code
space), re-quantising a block moves an element by at most H absmax (1 + 2^-20) (the slack covers the fp32 midpoints
and the rounding of x / absmax and map * absmax).  The value the update used differs from the exact moment by
E' = beta (E + H absmax_prev) + 4 U |m| (U = 2^-24, the step's own fp32 roundings), E = 0 at the first step.
"""
import numpy as np

F = np.float32
U = 2.0 ** -24
BLOCK = 256
UNPINNED = ()   # operations NumPy float32 cannot reproduce: none

DEFAULTS = dict(beta1=0.9, beta2=0.999, weight_decay=1e-2, eps=1e-8, min_8bit_size=4096, percentile_clipping=100,
                block_wise=True, is_paged=False)


def dynamic_map(signed):
    vals = [0.0, 1.0]
    for level in range(7):
        cells = 2 ** (level if signed else level + 1)
        edges = np.linspace(0.1, 1.0, cells + 1)
        for lo, hi in zip(edges[:-1], edges[1:]):
            c = (lo + hi) / 2.0 * 10.0 ** (level - 6)
            vals.append(c)
            if signed:
                vals.append(-c)
    return np.array(sorted(vals), np.float64).astype(F)


QMAP1, QMAP2 = dynamic_map(True), dynamic_map(False)
ZERO1, ZERO2 = int(np.flatnonzero(QMAP1 == 0)[0]), int(np.flatnonzero(QMAP2 == 0)[0])


def midpoints(qmap):
    s = qmap[:-1] + qmap[1:]          # one rounding
    return s * F(0.5)                 # exact


MID1, MID2 = midpoints(QMAP1), midpoints(QMAP2)


def encode(mid, x):
    """the number of midpoints strictly below x"""
    return np.searchsorted(mid, np.asarray(x, F), side="left").astype(np.uint8)


def half_gap(qmap):
    return float(np.max(np.diff(qmap.astype(np.float64)))) / 2 * (1 + 2.0 ** -20)


def group_scalars(g, step):
    beta1, beta2 = g["betas"]
    lr = float(g["lr"])
    bc1 = 1 - beta1 ** step
    bc2_sqrt = float(np.sqrt(1 - beta2 ** step))
    return dict(beta1=beta1, one_minus_beta1=1 - beta1, beta2=beta2, one_minus_beta2=1 - beta2,
                eps_c=bc2_sqrt * g["eps"], step_size=-(lr * bc2_sqrt / bc1), wd_factor=1 - lr * g["weight_decay"])


def _update(p, g, m, v, sc):
    """the moments and the parameter in fp32, one rounding per line"""
    b1, omb1, b2, omb2 = F(sc["beta1"]), F(sc["one_minus_beta1"]), F(sc["beta2"]), F(sc["one_minus_beta2"])
    eps_c, step_size, wdf = F(sc["eps_c"]), F(sc["step_size"]), F(sc["wd_factor"])
    t1 = b1 * m
    t2 = omb1 * g
    m = t1 + t2
    t3 = b2 * v
    cg = omb2 * g
    t4 = cg * g
    v = t3 + t4
    root = np.sqrt(v)                 # correctly rounded
    den = root + eps_c
    with np.errstate(divide="ignore", invalid="ignore"):
        q = m / den                   # correctly rounded
    t5 = step_size * q
    p = p + t5
    p = p * wdf
    return p, m, v


def new_state(numel, is8bit):
    if not is8bit:
        return dict(m=np.zeros(numel, F), v=np.zeros(numel, F))
    nblk = (numel + BLOCK - 1) // BLOCK
    return dict(code1=np.full(numel, ZERO1, np.uint8), code2=np.full(numel, ZERO2, np.uint8),
                absmax1=np.zeros(nblk, F), absmax2=np.zeros(nblk, F))


def decode_state(st):
    """the fp32 moments an 8-bit state stands for"""
    rep = lambda a: np.repeat(a, BLOCK)[:st["code1"].size]
    return QMAP1[st["code1"]] * rep(st["absmax1"]), QMAP2[st["code2"]] * rep(st["absmax2"])


def _quantise(x, mid, magnitude):
    n = x.size
    nblk = (n + BLOCK - 1) // BLOCK
    pad = np.zeros(nblk * BLOCK, F)
    pad[:n] = np.abs(x) if magnitude else x
    absmax = pad.reshape(nblk, BLOCK).max(axis=1)
    am = np.repeat(absmax, BLOCK)[:n]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(am > 0, x / am, F(0))       # correctly rounded; 0 where the block is all zero
    return encode(mid, q.astype(F)), absmax


def step_8bit(p, g, st, sc):
    """one step of a tensor with 8-bit state (flat fp32 arrays); st is updated in place.  Returns (p', m, v): the fp32
    parameter before any output rounding and the unquantised moments the update used."""
    p, g = np.asarray(p, F).reshape(-1), np.asarray(g, F).reshape(-1)
    m, v = decode_state(st)           # one rounding each
    p2, m, v = _update(p, g, m, v, sc)
    st["code1"], st["absmax1"] = _quantise(m, MID1, True)
    st["code2"], st["absmax2"] = _quantise(v, MID2, False)
    return p2, m, v


def step_f32(p, g, st, sc):
    p, g = np.asarray(p, F).reshape(-1), np.asarray(g, F).reshape(-1)
    p2, st["m"], st["v"] = _update(p, g, st["m"], st["v"], sc)
    return p2, st["m"], st["v"]


def step(p, g, st, sc):
    return (step_8bit if "code1" in st else step_f32)(p, g, st, sc)


def adamw_f64_moments(m, v, g, sc):
    """unquantised AdamW moments in float64, no rounding anywhere, from the four fp32 coefficients the device uses
    (1 - beta is rounded on its own: it is not 1 - fp32(beta))"""
    g = np.asarray(g, np.float64)
    b1, omb1, b2, omb2 = (float(F(sc[k])) for k in ("beta1", "one_minus_beta1", "beta2", "one_minus_beta2"))
    return b1 * m + omb1 * g, b2 * v + omb2 * g * g


def track_bound(err, absmax_prev, beta, half, used):
    """E' = beta (E + H absmax_prev) + 4 U |used|; absmax_prev per element"""
    return beta * (err + half * absmax_prev) + 4 * U * np.abs(used.astype(np.float64))


# ---- the store tests/test_adamw8bit_gpu.py runs -------------------------------------------------------------------
# 1, 7, 8, 9 and 4095 elements take the fp32 path (4095: just under min_8bit_size); 4096 is exactly 16 blocks, 4097
# has a one-element last block, 4099 a three-element one, 70001 has 274 blocks (more than one workgroup sweep at a
# capped grid, and it crosses the 65536-element norm chunk).  Group a ends with s4097 at element 12329, inside the
# vector [12328, 12336); group b begins at 12336.  Both groups hold 8-bit tensors; group a also the fp32 ones.
SHAPES = [("s1", (1,)), ("s7", (7,)), ("s8", (8,)), ("s9", (3, 3)), ("s4095", (4095,)), ("s4096", (64, 64)),
          ("s4097", (4097,)), ("s4099", (4099,)), ("s70001", (70001,))]
SPLIT = 7
GROUP_CFG = [dict(lr=2e-3, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8),
             dict(lr=1e-3, weight_decay=0.1, betas=(0.8, 0.99), eps=1e-6)]
LR_FACTORS = [0.25, 0.5, 1.0, 0.8, 0.6]   # a scheduler-like multiplier on both groups' lr, one per step
STEPS = 5
ZERO_BLOCK = ("s4099", 3)                  # its gradient is zero on every step: absmax stays exactly 0
HUGE = ("s70001", 5, 17, 1.0e4)            # block 5, element 17: gradient scaled 10^4, the rest of the block tiny codes


def numel(shape):
    return int(np.prod(shape))


def case_grad(name, shape, k):
    """gradient of step k: a hash of magnitude 10^-2 (bf16-exact), with the two special blocks"""
    import _oracle_adafactor as AF
    import oracle.adamw as OA
    g = AF.hashed((numel(shape),), 7000 + 17 * k + sum(map(ord, name)), 1e-2).copy()
    if name == ZERO_BLOCK[0]:
        g[ZERO_BLOCK[1] * BLOCK:(ZERO_BLOCK[1] + 1) * BLOCK] = 0
    if name == HUGE[0]:
        i = HUGE[1] * BLOCK + HUGE[2]
        g[i] = OA.rbf(np.array([(abs(g[i]) + F(0.01)) * F(HUGE[3])], F))[0]
    return g.reshape(shape)
