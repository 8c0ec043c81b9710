"""Shared pieces of the gradient-norm / clip edge tests (test_grad_norm_edges_gpu.py, test_grad_norm_edges_ref.py):
the case table, the input families, the float64 reference and the bound of the kernels of csrc/adamw.hip that every
trained step runs through: grad_sqnorm_kernel, tensor_sq_kernel, clip_coef_kernel and scale_bf16_kernel.  Plain
PyTorch and NumPy on the CPU, seeded CPU generators, so both files see the same numbers.

The chunk table (util/optimizer/flat_store.py _init_store, csrc/flat_store.h NormChunk): every tensor starts on a
multiple of ALIGN = 8 elements of the flat store and is cut into chunks of CHUNK = 2^16 elements; the last chunk of a
tensor ends with the tensor, so a chunk never crosses a tensor and only its end can be off a multiple of 8.  One
workgroup of 256 lanes sums a chunk: lane t starts at begin + 8 t and strides 256 x 8; on bf16 gradients a loop with
four loads in flight runs first, while e + 3 x 256 x 8 + 8 <= end (UNROLL = 4 x 256 x 8 elements a trip).  STORES
aims at those numbers; test_grad_norm_edges_ref.py holds its preconditions against the table the optimizer builds.

The bound on tensor_sq (derived, not measured).  A lane turns 8 elements into one fp32 partial by a chain of 8 fmaf
over non-negative terms, s <- fl(g_j^2 + s).  Each fmaf rounds once, so the chain is an 8-term inner product and its
error is at most 8 u sum_j g_j^2 with u = 2^-24 (Jeannerod and Rump 2013: n u bounds an n-term inner product with no
second-order term; with bf16 gradients the first product is exact and 7 u would do).  All terms are non-negative, so
this is 8 u = 2^-21 relative to the partial itself.  Everything after the partial is float64: lane sums, the wave and
block sums, the chunk slots and their sum per tensor in chunk order, at most 2^18 additions below 2^-53 each, which
the never-attained worst case of the chain leaves room for.  So per tensor |got - ref| <= TSQ_BOUND ref = 2^-21 ref,
as long as no square leaves the normal range of fp32 (the families "big66" and "small70" do, on purpose, and are held
to what torch does instead).  tensor_sq_math below is that scheme written once over a dtype: in float64 it is the
reference, in float32 (plain multiply and add, two roundings a term where the kernel has one) the honest evaluation
that the ref file holds to the same bound.

total and coefficient: oracle/adamw.py clip_grad_norm_bf16 / clip_grad_norm_f32, whose rounding points are torch's.
On the bf16 form every stage is rounded to bf16, which swallows the fp32 error: the device must give the oracle's
bits.  On the f32 and master forms the device folds the norms in fp32 and the oracle in float64: FOLD = 16 x 2^-24
relative (test_adafactor_gpu.py).

What torch does at the extremes (recorded by test_grad_norm_edges_ref.py on the CPU), and what the device may do:
  |g| = 2^60   squares are 2^120: finite in fp32 while a tensor holds fewer than 256 elements and the store fewer
               than 256 in all, inf beyond (torch sums squares in fp32).  The device sums a tensor in float64, but
               folds the squares of the fp32 norms in fp32, so its total is inf exactly when torch's is.  Held to
               torch: where torch is finite, as any other case; where torch gives inf, total inf and coefficient 0.
  |g| = 2^66   every square overflows fp32: torch gives total inf and coefficient 0 on all three forms.  The float64
               oracle would give a finite total; torch is the reference, and the device (inf from the first fmaf)
               must give inf and 0.
  |g| = 2^-40  squares are 2^-80, normal: as any other case.
  |g| = 2^-70  squares are 2^-140, subnormal in fp32.  torch on the CPU keeps subnormals: the total is the
               correctly rounded sqrt(n) 2^-70, not 0.  A device may flush subnormal squares to zero, so it is held to
               0 <= total <= torch's total and coefficient == 1 (max_norm 1).
  non-finite   one NaN anywhere: total NaN, coefficient NaN (torch.clamp propagates NaN), every clipped gradient
               NaN.  One +-inf: total inf, coefficient 0, the clipped gradients 0 but inf x 0 = NaN in its place."""
import functools
import math
import unittest.mock

import numpy as np
import torch

from oracle import adamw as OA

BF, F32 = torch.bfloat16, torch.float32
U24 = 2.0 ** -24
TSQ_BOUND = 2.0 ** -21      # the docstring
FOLD = 16 * U24             # f32 / master: total and coefficient, device against the float64-summing oracle
CHUNK, ALIGN = 1 << 16, 8   # flat_store.py _init_store; module/param_store.py (16 bytes, at least 8 elements)
LANES, VEC = 256, 8         # grad_sqnorm_kernel: lanes of a workgroup, elements of a 16-byte bf16 vector
UNROLL = 4 * LANES * VEC    # elements one trip of the bf16 loop with four loads in flight covers
CLIP_BLOCK = 1024           # lanes of clip_coef_kernel's one workgroup
FORMS = ("bf16", "f32", "master")

# chunk lengths the bf16 loop is aimed at: 0, 1 and 2 trips of every lane, with and without a tail; 3 x 256 x 8 and
# one vector more are the lengths at which lane 0 takes no trip / its first
UNROLL_ENDS = (UNROLL - 8, UNROLL, UNROLL + 8, 2 * UNROLL + 8)
STORES = {
    "small": [1, 7, 8, 9, 17],
    "unroll": [3 * LANES * VEC, 3 * LANES * VEC + 8, *UNROLL_ENDS, UNROLL - 1, UNROLL + 9],
    "chunk": [CHUNK, CHUNK + 8, CHUNK - 8, 3 * CHUNK + 24],
    # the same ends in the last chunk of a multi-chunk tensor, and tensors one element off a chunk
    "tails": [CHUNK + UNROLL - 8, 2 * CHUNK + UNROLL + 8, CHUNK + 2 * UNROLL + 8, CHUNK + UNROLL, CHUNK - 1, CHUNK + 1,
              5],
    # more tensors than clip_coef_kernel has lanes: its lane-strided loop takes a second trip
    "many": [(5 * i) % 19 + 1 for i in range(CLIP_BLOCK + 6)],
}
FAMILIES_PARITY = ("normal", "ints")
FAMILIES_NONFINITE = ("inf+", "inf-", "nan_first", "nan_last_vec", "nan_last_chunk")
FAMILIES_EXTREME = ("big60", "big66", "small40", "small70")
EXTREME_STORES = ("small", "unroll")   # a store torch keeps finite at 2^60, and one it does not
NAN_F32_BITS = 0x7FC00000
NAN_BF_BITS = 0x7FC0

CHUNK_DTYPE = np.dtype([("begin", "<i8"), ("end", "<i8"), ("tensor", "<i4"), ("pad", "<i4")])   # NormChunk


def chunk_table(opt) -> np.ndarray:
    """the NormChunk table a FlatStoreOptimizer built, as a structured array"""
    raw = opt._chunks.cpu().numpy().tobytes()
    return np.frombuffer(raw, dtype=CHUNK_DTYPE)[:opt._n_chunks]


def specs(store):
    return [(f"t{i}", (n,), "g") for i, n in enumerate(STORES[store])]


def offsets(store):
    """element offset of every tensor of the store, and the store's padded length (module/param_store.py)"""
    off, out = 0, []
    for n in STORES[store]:
        off = (off + ALIGN - 1) // ALIGN * ALIGN
        out.append(off)
        off += n
    return out, (off + ALIGN - 1) // ALIGN * ALIGN


# ------------------------------------------------------------------------------------------
# inputs
def _seed(*k):
    s = 2468
    for v in k:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return s


def _nan_site(store, fam):
    """(tensor, element) of the planted NaN: the first vector of the first tensor; the last element of the first tensor
    that ends inside a vector (or of the first chunk, where every tensor ends on one); the last element of the tensor
    with the most chunks"""
    sizes = STORES[store]
    if fam == "nan_first":
        return 0, 0
    if fam == "nan_last_vec":
        t = next((i for i, n in enumerate(sizes) if n % VEC), 0)
        return t, min(sizes[t], CHUNK) - 1
    t = max(range(len(sizes)), key=lambda i: sizes[i])
    return t, sizes[t] - 1


@functools.lru_cache(maxsize=8)
def grads(store, fam, form):
    """the gradients of one case: a tuple of 1-D CPU tensors in the gradient dtype of the form (fp32 for "f32", bf16
    for "bf16" and "master")"""
    sizes = STORES[store]
    g = torch.Generator(device="cpu").manual_seed(_seed(list(STORES).index(store), sum(map(ord, fam))))
    T = len(sizes)
    out = []
    for t, n in enumerate(sizes):
        if fam == "ints":
            v = torch.randint(-16, 17, (n,), generator=g).double()
        elif fam == "zeros":
            v = torch.zeros(n, dtype=torch.float64)
        elif fam in FAMILIES_EXTREME:
            k = {"big60": 60, "big66": 66, "small40": -40, "small70": -70}[fam]
            v = (1.0 - 2.0 * (torch.arange(n) % 3 == 1)).double() * 2.0 ** k
        else:
            v = torch.randn(n, generator=g, dtype=torch.float64)
            if fam == "normal":   # 2^k per tensor, k over -30 ... +30
                v = v * 2.0 ** (-30 + (60 * t) // max(T - 1, 1) if T > 1 else 0)
        out.append(v)
    if fam in FAMILIES_NONFINITE:
        if fam.startswith("inf"):
            t = T // 2
            out[t][sizes[t] // 2] = math.inf if fam == "inf+" else -math.inf
        else:
            t, i = _nan_site(store, fam)
            out[t][i] = math.nan
    return tuple(v.to(F32 if form == "f32" else BF) for v in out)


def bits16(t) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int16).numpy().astype(np.uint16).reshape(-1)


def oracle_inputs(gl, form):
    """what oracle.adamw's clip functions take for the form: bf16 bits, or the fp32 values"""
    if form == "bf16":
        return [bits16(g) for g in gl]
    return [g.float().numpy().reshape(-1) for g in gl]


# ------------------------------------------------------------------------------------------
# the reference
def tensor_sq_math(g: np.ndarray, dt) -> float:
    """sum g^2 of one tensor by the kernel's grouping, every operation of the 8-term partials in dt (the vector a
    tensor ends in is filled with zeros); the partials are added in float64"""
    x = np.zeros((g.size + VEC - 1) // VEC * VEC, dtype=dt)
    x[:g.size] = g.astype(dt)
    x = x.reshape(-1, VEC)
    s = np.zeros(x.shape[0], dtype=dt)
    for j in range(VEC):
        s = x[:, j] * x[:, j] + s
    return float(np.sum(s.astype(np.float64)))


def oracle_clip(gl, form, max_norm):
    """(total, coef) by oracle.adamw with the form's rounding points"""
    with np.errstate(all="ignore"):
        if form == "bf16":
            _, total, coef = OA.clip_grad_norm_bf16(oracle_inputs(gl, form), max_norm)
        else:
            total, coef = OA.clip_grad_norm_f32(oracle_inputs(gl, form), max_norm)
    return float(total), float(coef)


class Ref:
    pass


@functools.lru_cache(maxsize=8)
def reference(store, fam, form):
    """float64 per-tensor sum g^2 (sq), the per-tensor norm with the form's rounding (norm: the oracle's total of the
    tensor alone), and the oracle's (total, coef) at a max_norm that bites (total / 4) and one that does not (4 total)"""
    gl = grads(store, fam, form)
    r = Ref()
    with np.errstate(all="ignore"):
        r.sq = np.array([tensor_sq_math(g.double().numpy(), np.float64) for g in gl])
        r.norm = np.array([oracle_clip([g], form, 1.0)[0] for g in gl])
    total = oracle_clip(gl, form, 1.0)[0]
    finite = math.isfinite(total) and total > 0
    r.max_norms = tuple(float(np.float32(total * s)) for s in (0.25, 4.0)) if finite else (1.0,)
    r.clip = {mx: oracle_clip(gl, form, mx) for mx in r.max_norms}
    return r


def torch_clip(gl, form, max_norm):
    """torch.nn.utils.clip_grad_norm_ on CPU tensors of the dtype the reference trainer holds for the form (fp32
    gradients behind fp32 master weights) -> (total, coef, clipped gradients); the coefficient is what the call's
    torch.clamp returned"""
    dt = BF if form == "bf16" else F32
    params = []
    for g in gl:
        p = torch.nn.Parameter(torch.zeros(g.shape, dtype=dt))
        p.grad = g.to(dt).clone()
        params.append(p)
    seen = []
    clamp = torch.clamp

    def spy(*a, **k):
        seen.append(clamp(*a, **k))
        return seen[-1]

    with unittest.mock.patch.object(torch, "clamp", spy):
        total = torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)
    assert len(seen) == 1 and total.dtype == dt and seen[0].dtype == dt
    return float(total), float(seen[0]), [p.grad for p in params]


def same(a: float, b: float) -> bool:
    """equal as numbers; NaN compares as NaN"""
    return (math.isnan(a) and math.isnan(b)) or a == b


# ------------------------------------------------------------------------------------------
# the checks: the worst |err| / bound per kernel path kept for the report
WORST: dict = {}


def note(path, ratio, what):
    if path not in WORST or not ratio <= WORST[path][0]:
        WORST[path] = (ratio, what)


def check_tensor_sq(path, got, ref_sq, what, exact=False):
    """per tensor |got - ref| <= 2^-21 ref (exact: equal bits)"""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - ref_sq)
    tol = np.zeros_like(ref_sq) if exact else TSQ_BOUND * ref_sq
    with np.errstate(all="ignore"):
        ratio = np.where(err == 0, 0.0, np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), math.inf))
    ratio = np.where(np.isnan(ratio), math.inf, ratio)
    note(path, float(ratio.max()), what)
    if not bool((err <= tol).all()):
        i = int(np.argmax(ratio))
        raise AssertionError(f"{what}: {int((~(err <= tol)).sum())} of {err.size} tensors out of bound; worst tensor {i}: "
                             f"got {got[i]!r} ref {ref_sq[i]!r} |d| {err[i]:.3e} bound {tol[i]:.3e}")


def check_scalar(path, got, ref, rel, what):
    """|got - ref| <= rel |ref| (rel 0: the same number)"""
    if rel == 0 or not math.isfinite(ref):
        ok, ratio = same(got, ref), 0.0 if same(got, ref) else math.inf
    else:
        err = abs(got - ref)
        ratio = 0.0 if err == 0 else (err / (rel * abs(ref)) if ref != 0 else math.inf)
        ok = ratio <= 1
    note(path, ratio if not math.isnan(ratio) else math.inf, what)
    assert ok, f"{what}: got {got!r} ref {ref!r} allowed {rel:.3e} relative"


# ------------------------------------------------------------------------------------------
# scale_bf16_by_device_scalar
def all_bf16_patterns() -> np.ndarray:
    return np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)


def scale_reference(bits: np.ndarray, coef: float):
    """(bits of bf16(f32(g) coef), mask of the elements whose exact product is subnormal or underflows: there the
    device may give a zero of the product's sign)"""
    with np.errstate(all="ignore"):
        g = OA.bf16_to_f32(bits)
        ref = OA.f32_to_bf16_bits(g * np.float32(coef))
        exact = g.astype(np.float64) * float(np.float32(coef))
        tiny = (np.abs(exact) < 2.0 ** -126) & (exact != 0)
    return ref, tiny


def check_scaled(got_bits: np.ndarray, bits: np.ndarray, coef: float, what):
    ref, tiny = scale_reference(bits, coef)
    isnan = lambda b: (b & 0x7FFF) > 0x7F80   # noqa: E731
    zero_same_sign = (got_bits & 0x7FFF) == 0
    zero_same_sign &= (got_bits >> 15) == (ref >> 15)
    ok = (got_bits == ref) | (isnan(got_bits) & isnan(ref)) | (tiny & zero_same_sign)
    if not bool(ok.all()):
        i = int(np.flatnonzero(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} elements differ; first at {i}: g {bits[i]:#06x} "
                             f"got {got_bits[i]:#06x} ref {ref[i]:#06x}")
