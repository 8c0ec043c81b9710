"""Shared pieces of the attention edge tests (test_attention_edges_gpu.py, test_attention_edges_ref.py):
the float64 reference, its rounding-floor emulation, the per-row metric and the adversarial inputs.
Everything here is plain PyTorch on the CPU; inputs come from seeded CPU generators, so the GPU tests and
the reference-only tests see the same numbers."""
import functools
import math

import torch

BF = torch.bfloat16
LN2 = math.log(2.0)
FWD_CAP, BWD_CAP = 2e-2, 3e-2   # the whole-tensor bounds of tests/test_kernels_gpu.py::test_attention*
FLOOR_FACTOR = 4.0              # kernel <= 4 x the rounding floor: fp32 accumulation order + hardware exp2


def f32(x: float) -> float:
    """the value the C ABI carries for a float argument (AttnArgs.scale, the softmax scale)"""
    return float(torch.tensor(x, dtype=torch.float32))


def rb(t: torch.Tensor) -> torch.Tensor:
    """round to bf16, as float64"""
    return t.to(BF).double()


def heads(t: torch.Tensor, H: int) -> torch.Tensor:
    B, N, C = t.shape
    return t.double().reshape(B, N, H, C // H).permute(0, 2, 1, 3)


def unheads(t: torch.Tensor) -> torch.Tensor:
    B, H, N, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, N, H * D)


def default_scale(D: int) -> float:
    return f32(D ** -0.5)


def reference(q, k, v, do, H, scale):
    """float64 softmax(scale q k^T) v per head, its autograd gradients and lse / ln 2 of bf16 operands"""
    qh, kh, vh = (heads(t, H).requires_grad_(True) for t in (q, k, v))
    s = scale * (qh @ kh.transpose(-1, -2))
    lse = torch.logsumexp(s, dim=-1)
    o = torch.softmax(s, dim=-1) @ vh
    o.backward(heads(do, H))
    return {"o": unheads(o.detach()), "lse2": lse.detach() / LN2, "dq": unheads(qh.grad), "dk": unheads(kh.grad),
            "dv": unheads(vh.grad), "smax2": s.detach().abs().amax(-1) / LN2}


def emulated(q, k, v, do, H, scale, round_=True):
    """The same operation in float64 with only the roundings the flash algorithm is entitled to: P and dS
    rounded to bf16 before their second products (o = P v, dv = P^T do; dq = dS k, dk = dS^T q), o rounded
    to bf16 before delta = rowsum(do o), and bf16 outputs.  round_=False: no rounding (must equal autograd)."""
    r = rb if round_ else (lambda t: t)
    qh, kh, vh, gh = (heads(t, H) for t in (q, k, v, do))
    s = scale * (qh @ kh.transpose(-1, -2))
    p = torch.softmax(s, dim=-1)
    o = r(r(p) @ vh)
    delta = (gh * o).sum(-1, keepdim=True)
    ds = r(p * (gh @ vh.transpose(-1, -2) - delta))
    return {"o": unheads(o), "dq": unheads(r(scale * (ds @ kh))), "dk": unheads(r(scale * (ds.transpose(-1, -2) @ qh))),
            "dv": unheads(r(r(p).transpose(-1, -2) @ gh))}


def row_metric(got, ref, H):
    """max over (b, h, token) rows of max_d |got - ref| / max(max_d |ref|, 2^-6 max_all |ref|): the floor in
    the denominator keeps near-zero rows from dividing by noise.  Returns (worst value, its (b, h, token))."""
    g, r = heads(got.cpu(), H), heads(ref, H)
    err = (g - r).abs().amax(-1)
    den = torch.maximum(r.abs().amax(-1), r.abs().max() * 2.0 ** -6)
    m = torch.where(den > 0, err / den, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    m = torch.where(torch.isnan(err), torch.full_like(err, math.inf), m)
    i = int(m.argmax())
    return float(m.flatten()[i]), tuple(int(x) for x in torch.unravel_index(torch.tensor(i), m.shape))


def ulp32(x: float) -> float:
    """spacing of fp32 at magnitude x (>= 1)"""
    return 2.0 ** (math.floor(math.log2(max(abs(x), 1.0))) - 23)


def lse_bound(ref) -> float:
    """absolute bound on lse (log2 units): the largest value the chain rounds to fp32 is A = max(|lse|,
    |scale log2e s_ij|) (the fp32 score accumulation, the c-multiply, m + log2 l; v_exp / v_log are 1 ulp),
    one fp32 spacing at that magnitude, x 4 -- and never above the existing 2e-2."""
    A = max(float(ref["lse2"].abs().max()), float(ref["smax2"].max()))
    return min(FLOOR_FACTOR * ulp32(A), 2e-2)


class Case:
    """bf16 operands (CPU), the float64 reference and the rounding floor per tensor, computed once per key"""

    def __init__(self, q, k, v, do, H, scale):
        self.q, self.k, self.v, self.do, self.H, self.scale = q, k, v, do, H, scale
        self.ref = reference(q, k, v, do, H, scale)
        emu = emulated(q, k, v, do, H, scale)
        self.floor = {n: row_metric(emu[n], self.ref[n], H)[0] for n in ("o", "dq", "dk", "dv")}

    def tol(self, name):
        """per-row bound: 4 x the rounding floor of this case"""
        return FLOOR_FACTOR * self.floor[name]

    def whole(self, got, name):
        """the metric and bound test_kernels_gpu.py::test_attention* already hold every kernel to: max|d| / max|ref|
        over the whole tensor under 2e-2 (forward) / 3e-2 (backward).  It stays in force beside the per-row bound;
        it is not a cap on the per-row value, because where a row's gradient nearly cancels (softmax close to
        one-hot: dP - delta ~ 0, delta from the bf16 o) the entitled roundings alone put single rows at 0.2 - 0.3
        of their own magnitude while the whole tensor stays at 0.005."""
        r = self.ref[name]
        return float((got.double().cpu() - r).abs().max() / r.abs().max()), (FWD_CAP if name == "o" else BWD_CAP)

    def zero_bound(self, name):
        """Where the reference gradient is identically zero (one key: the softmax is constant) the relative
        metric has no scale; the kernel's dq / dk are then the fp32 noise of dP - delta through one product,
        bounded by one bf16 rounding of dP: 2^-8 scale max|operand| max|do v^T|."""
        gh, vh = heads(self.do, self.H), heads(self.v, self.H)
        dp = (gh @ vh.transpose(-1, -2)).abs().max()
        other = self.k if name == "dq" else self.q
        return float(2.0 ** -8 * self.scale * other.double().abs().max() * dp)


def randn_case(seed, B, H, Nq, Nk, Dv, scale=None):
    g = torch.Generator().manual_seed(seed)
    mk = lambda n: torch.randn(B, n, H * Dv, generator=g).to(BF)   # noqa: E731
    q, k, v, do = mk(Nq), mk(Nk), mk(Nk), mk(Nq)
    return Case(q, k, v, do, H, default_scale(Dv) if scale is None else f32(scale))


@functools.lru_cache(maxsize=None)
def geometry_case(B, H, Nq, Nk, Dv, scale=None):
    return randn_case(1000 * Nq + 7 * Nk + Dv, B, H, Nq, Nk, Dv, scale)


# ------------------------------------------------------------------------------------------
# inputs that make the softmax matter
def _signs(g, n, D):
    """n pairwise distinct vectors of {+-1}^D"""
    while True:
        s = torch.randint(0, 2, (n, D), generator=g) * 2 - 1
        if torch.unique(s, dim=0).shape[0] == n:
            return s.double()


def key_tile_gain(D, order):
    """per-64-key-tile magnitude steps of the 'grow' ordering: doubling per tile up to a = 4 in the last.
    (a = 2 at D = 128 elsewhere; here 4, because with a = 2 the non-matching scores stay under 13 log2 units
    in total and cannot exceed the forward's lazy-max threshold of 8 on more than one tile.)"""
    return 4.0 if order == "grow" or D <= 64 else 2.0


@functools.lru_cache(maxsize=None)
def peaked_case(B, H, Nq, Nk, Dv, order, seed=0):
    """Keys k_j = a_j s_j (s_j in {+-1}^D distinct), queries q_i = k_pi(i): the float64 softmax is one-hot at
    pi(i).  order: 'first' (all matches among the first 32 keys: the max never grows after tile 0), 'last'
    (all in the last partial 32-key tile), 'grow' (a_j doubles per 64-key tile and the matches sit in the last
    tile: the running max grows on every tile).  Returns (Case, pi [B, H, Nq])."""
    g = torch.Generator().manual_seed(100 + seed)
    a = key_tile_gain(Dv, order)
    amp = torch.full((Nk,), a, dtype=torch.float64)
    tail0 = (Nk - 1) // 32 * 32   # first key of the last (partial) 32-key half
    if order == "first":
        lo, hi = 0, min(32, Nk)
    else:
        lo, hi = tail0, Nk
    if order == "grow":
        nt = (Nk + 63) // 64
        amp = a * 2.0 ** -(nt - 1 - torch.arange(Nk) // 64).double()
    k = torch.empty(B, Nk, H, Dv, dtype=torch.float64)
    q = torch.empty(B, Nq, H, Dv, dtype=torch.float64)
    pi = torch.empty(B, H, Nq, dtype=torch.long)
    for b in range(B):
        for h in range(H):
            kk = _signs(g, Nk, Dv) * amp[:, None]
            p = torch.randint(lo, hi, (Nq,), generator=g)
            k[b, :, h], q[b, :, h], pi[b, h] = kk, kk[p], p
    v = torch.randn(B, Nk, H * Dv, generator=g).to(BF)
    do = torch.randn(B, Nq, H * Dv, generator=g).to(BF)
    c = Case(q.reshape(B, Nq, H * Dv).to(BF), k.reshape(B, Nk, H * Dv).to(BF), v, do, H, default_scale(Dv))
    return c, pi


def peaked_margin(c: Case, pi) -> float:
    """smallest gap (nats) between the matching score and the best other score"""
    s = c.scale * (heads(c.q, c.H) @ heads(c.k, c.H).transpose(-1, -2))
    win = s.gather(-1, pi[..., None])
    rest = s.scatter(-1, pi[..., None], -math.inf).amax(-1, keepdim=True)
    return float((win - rest).min())


def peaked_expect(c: Case, pi):
    """what the one-hot softmax gives: o = v[pi], lse = the matching score (log2), dv[j] = sum of do_i over
    pi(i) = j"""
    vh, gh = heads(c.v, c.H), heads(c.do, c.H)
    D = vh.shape[-1]
    o = vh.gather(2, pi[..., None].expand(-1, -1, -1, D))
    dv = torch.zeros_like(vh).scatter_add_(2, pi[..., None].expand(-1, -1, -1, D), gh)
    s = c.scale * (heads(c.q, c.H) @ heads(c.k, c.H).transpose(-1, -2))
    return unheads(o), s.gather(-1, pi[..., None])[..., 0] / LN2, unheads(dv)


def tile_max_growth(c: Case, tile=64):
    """log2-unit growth of the row max from each key tile to the next, max over rows: [ntiles - 1]"""
    s = c.scale / LN2 * (heads(c.q, c.H) @ heads(c.k, c.H).transpose(-1, -2))
    Nk = s.shape[-1]
    run, out = None, []
    for t0 in range(0, Nk, tile):
        m = s[..., t0:t0 + tile].amax(-1)
        if run is not None:
            out.append(float((m - run).max()))
            run = torch.maximum(run, m)
        else:
            run = m
    return out


@functools.lru_cache(maxsize=None)
def negative_case(B, H, Nq, Nk, Dv, seed=0):
    """Every true score <= -20 nats: k_j = -a (u with up to 5 sign flips), q_i = a (u with up to 5 flips), a = 2,
    so score = -a^2 scale (D - 2 hamming) (-32 + hamming nats at D = 64).  A zero-filled key that slipped past the
    mask would score 0 and take essentially all the weight."""
    g = torch.Generator().manual_seed(200 + seed)
    a = 2.0

    def flipped(u, n):
        x = u.repeat(n, 1)
        for i in range(n):
            nf = int(torch.randint(0, 6, (1,), generator=g))
            x[i, torch.randperm(Dv, generator=g)[:nf]] *= -1
        return x
    q = torch.empty(B, Nq, H, Dv, dtype=torch.float64)
    k = torch.empty(B, Nk, H, Dv, dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            u = _signs(g, 1, Dv)[0]
            q[b, :, h], k[b, :, h] = a * flipped(u, Nq), -a * flipped(u, Nk)
    v = torch.randn(B, Nk, H * Dv, generator=g).to(BF)
    do = torch.randn(B, Nq, H * Dv, generator=g).to(BF)
    return Case(q.reshape(B, Nq, H * Dv).to(BF), k.reshape(B, Nk, H * Dv).to(BF), v, do, H, default_scale(Dv))


def with_zero_key(c: Case) -> dict:
    """the float64 reference with one extra all-zero key / value row (what a phantom key computes); dk / dv are
    cut back to the true keys"""
    z = lambda t: torch.cat([t, torch.zeros_like(t[:, :1])], dim=1)   # noqa: E731
    r = reference(c.q, z(c.k), z(c.v), c.do, c.H, c.scale)
    r["dk"], r["dv"] = r["dk"][:, :-1], r["dv"][:, :-1]
    return r


# ------------------------------------------------------------------------------------------
# row softmax references
def softmax_rows_ref(S, ncols, scale, round_scores=False):
    """float64 softmax(scale S[:, :ncols]) and lse (natural log); round_scores: scale * S rounded to fp32 first
    (the kernel's own arithmetic on the scores: matters at |scale S| ~ 1e4, where one fp32 spacing is 1e-3)"""
    x = S[:, :ncols].double() * scale
    if round_scores:
        x = x.float().double()
    return torch.softmax(x, dim=-1), torch.logsumexp(x, dim=-1)


def rows_metric(got, ref):
    """row_metric for a 2-D [rows, cols] pair"""
    return row_metric(got.reshape(1, got.shape[0], -1), ref.reshape(1, ref.shape[0], -1), 1)


def masked_softmax_ref(S, ncols, scale, Nq, H, causal, bias_qch):
    """S [B*H, Nq, >= ncols] fp32; bias_qch: float64 [Nq, ncols, H] or None.  float64 P [B*H, Nq, ncols]"""
    x = S[..., :ncols].double() * scale
    BH = x.shape[0]
    if bias_qch is not None:
        x = x + bias_qch.permute(2, 0, 1).repeat(BH // H, 1, 1)
    if causal:
        qi = torch.arange(Nq)[:, None]
        ci = torch.arange(ncols)[None, :]
        x = x.masked_fill(ci > qi, -math.inf)
    return torch.softmax(x, dim=-1)
