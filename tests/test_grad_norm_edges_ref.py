"""The truth test_grad_norm_edges_gpu.py is held to, established on the CPU (_grad_norm_edges.py has the derivations):
oracle/adamw.py's clip functions against torch.nn.utils.clip_grad_norm_ on CPU tensors of the same dtype, what torch
does at the extremes, an honest fp32 evaluation of the 8-term partial scheme against the 2^-21 bound, and the case
table against the chunk table the optimizer really builds.

oracle against torch.  bf16: per-tensor norm, total and coefficient are each rounded to bf16, and the oracle claims
torch's bits; so do the clipped gradients (one bf16 product).  f32 / master: torch sums the squares of a tensor in
fp32 in an order of its own, the oracle in float64 rounded once.  Any order of n non-negative fp32 terms is within
(n - 1) 2^-24 of the exact sum, half of that after the square root, so the totals agree within
(n_max / 2 + T / 2 + 4) 2^-24 relative (n_max the largest tensor, T the tensors folded into the total, 4: the two
square roots, the + 1e-6 and the division), and the coefficients likewise.  Non-finite results agree as they are:
NaN with NaN, inf with inf, and the coefficient 0 of an inf total exactly.

Recorded here, required of the device there:
  2^66    torch: total inf, coefficient 0 on every form (the float64 oracle stays finite on f32 / master: torch is the
          reference).
  2^60    torch: finite on the store "small" (42 elements: 42 x 2^120 < 2^128), inf and coefficient 0 on "unroll".
  2^-40   finite, as any other case.
  2^-70   torch keeps the subnormal squares: total = fp32 / bf16 rounding of sqrt(n) 2^-70 > 0, coefficient 1.  A
          device that flushes subnormals gives a smaller total or 0: 0 <= total <= torch's total, coefficient == 1."""
import math

import numpy as np
import pytest
import torch

import _grad_norm_edges as E
from oracle import adamw as OA

ALL_FAMILIES = E.FAMILIES_PARITY + ("zeros",) + E.FAMILIES_NONFINITE


def order_allowance(store):
    sizes = E.STORES[store]
    return (max(sizes) / 2 + len(sizes) / 2 + 4) * E.U24


@pytest.mark.parametrize("form", E.FORMS)
@pytest.mark.parametrize("fam", ALL_FAMILIES)
@pytest.mark.parametrize("store", list(E.STORES))
def test_oracle_matches_torch(store, fam, form):
    gl = E.grads(store, fam, form)
    r = E.reference(store, fam, form)
    rel = 0.0 if form == "bf16" else order_allowance(store)
    for mx in r.max_norms:
        total, coef = r.clip[mx]
        t_total, t_coef, t_clipped = E.torch_clip(gl, form, mx)
        what = f"{store} {fam} {form} max_norm={mx!r}"
        E.check_scalar("cpu:total", total, t_total, rel, what + " total")
        E.check_scalar("cpu:coef", coef, t_coef, rel, what + " coef")
        if fam in ("nan_first", "nan_last_vec", "nan_last_chunk"):
            assert math.isnan(t_total) and math.isnan(t_coef), what
            assert all(bool(torch.isnan(g).all()) for g in t_clipped), what
        elif fam.startswith("inf"):
            assert t_total == math.inf and t_coef == 0.0, what
        elif fam == "zeros":
            assert t_total == 0.0 and t_coef == 1.0, what
        if form == "bf16":   # the clipped gradients: the oracle's bits (NaN as NaN)
            with np.errstate(all="ignore"):
                clipped, _, _ = OA.clip_grad_norm_bf16(E.oracle_inputs(gl, form), mx)
            for i, (a, b) in enumerate(zip(clipped, t_clipped)):
                b = E.bits16(b)
                nan = ((a & 0x7FFF) > 0x7F80) & ((b & 0x7FFF) > 0x7F80)
                assert bool(((a == b) | nan).all()), (what, i)
        elif math.isfinite(t_coef):   # one fp32 product with torch's own coefficient
            for i, (g, b) in enumerate(zip(gl, t_clipped)):
                with np.errstate(all="ignore"):
                    want = g.float().numpy() * np.float32(t_coef)
                assert np.array_equal(want, b.numpy(), equal_nan=True), (what, i)


def test_coefficient_recovered_from_a_clipped_element():
    """the spied torch.clamp result is the factor the gradients were multiplied by: on a power-of-two element
    clipped / original is exact"""
    for form in E.FORMS:
        gl = [g.clone() for g in E.grads("small", "normal", form)]
        gl[2][3] = 2.0 ** -5
        total = E.oracle_clip(gl, form, 1.0)[0]
        _, coef, clipped = E.torch_clip(gl, form, float(np.float32(total / 4)))
        assert 0 < coef < 1 and float(clipped[2][3]) / 2.0 ** -5 == coef, form


@pytest.mark.parametrize("form", E.FORMS)
@pytest.mark.parametrize("store", E.EXTREME_STORES)
def test_extremes_recorded(store, form):
    """what torch does on the CPU at 2^60, 2^66, 2^-40 and 2^-70 (the module docstring)"""
    n_all = sum(E.STORES[store])
    for fam in E.FAMILIES_EXTREME:
        gl = E.grads(store, fam, form)
        total, coef, _ = E.torch_clip(gl, form, 1.0)
        o_total, o_coef = E.oracle_clip(gl, form, 1.0)
        what = f"{store} {fam} {form}"
        if fam == "big66" or (fam == "big60" and store != "small"):
            assert total == math.inf and coef == 0.0, (what, total, coef)
            if form != "bf16" and fam == "big66":   # the float64 oracle is no reference here
                assert math.isfinite(o_total), what
        elif fam == "big60":
            assert math.isfinite(total) and 0 < coef < 1, (what, total, coef)
            E.check_scalar("cpu:total", o_total, total, 0.0 if form == "bf16" else order_allowance(store), what)
        elif fam == "small40":
            assert 0 < total < 1e-9 and coef == 1.0, (what, total, coef)
            E.check_scalar("cpu:total", o_total, total, 0.0 if form == "bf16" else order_allowance(store), what)
            b_total, b_coef, _ = E.torch_clip(gl, form, 2.0 ** -22)   # the + 1e-6 dominates: 2^-22 / 1e-6
            assert 0.2 < b_coef < 0.25, (what, b_coef)
        else:   # small70: a subnormal-derived norm, not 0
            want = math.sqrt(n_all) * 2.0 ** -70
            assert coef == 1.0 and abs(total - want) <= 2.0 ** -7 * want, (what, total, want)


@pytest.mark.parametrize("form", E.FORMS)
@pytest.mark.parametrize("store", list(E.STORES))
def test_honest_fp32_partials_within_bound(store, form):
    """the kernel's grouping in NumPy float32 (multiply, then add: sixteen roundings where the fmaf chain has eight)
    stays inside 2^-21 of the float64 evaluation on every case, and on integer-valued gradients is exact"""
    for fam in E.FAMILIES_PARITY + ("small40",):
        gl = E.grads(store, fam, form)
        ref = np.array([E.tensor_sq_math(g.double().numpy(), np.float64) for g in gl])
        got = np.array([E.tensor_sq_math(g.float().numpy(), np.float32) for g in gl])
        E.check_tensor_sq(f"cpu:tensor_sq {form}", got, ref, f"{store} {fam} {form}", exact=fam == "ints")
        if fam == "ints":
            assert all(float(s).is_integer() for s in ref)
    assert 0 < E.WORST[f"cpu:tensor_sq {form}"][0] <= 1 or form != "f32"   # not vacuous: fp32 operands do round


def test_case_table_preconditions():
    """the chunk table FlatStoreOptimizer builds on a CPU store of every case: the sizes the issue names, every
    targeted chunk length, no chunk across a tensor, begins on multiples of 8"""
    from onetrainer_amd.module.param_store import FlatParamStore
    from onetrainer_amd.util.optimizer.adamw_fused import FusedAdamW

    assert {1, 7, 8, 9, 17} <= set(E.STORES["small"])
    assert {E.CHUNK, E.CHUNK + 8, E.CHUNK - 8, 3 * E.CHUNK + 24} <= set(E.STORES["chunk"])
    assert len(E.STORES["many"]) > E.CLIP_BLOCK
    lengths, last_of_many = set(), set()
    for store, sizes in E.STORES.items():
        for dt in (torch.bfloat16, torch.float32):
            st = FlatParamStore(E.specs(store), dt, torch.device("cpu"))
            opt = FusedAdamW(st, [{"params": [st.params[n] for n in st.order]}], lr=1e-3)
            offs, numel = E.offsets(store)
            assert numel == st.numel <= 2_100_000 and offs == [st.slots[n].offset for n in st.order]
            tab = E.chunk_table(opt)
            covered = [0] * len(sizes)
            for i, c in enumerate(tab):
                b, e, t = int(c["begin"]), int(c["end"]), int(c["tensor"])
                assert b % E.ALIGN == 0 and 0 < e - b <= E.CHUNK
                assert offs[t] <= b and e <= offs[t] + sizes[t]                 # inside its tensor
                assert b == offs[t] + covered[t]                                # in element order, no gap
                covered[t] += e - b
                assert e == offs[t] + sizes[t] or e - b == E.CHUNK              # only a tensor's end cuts a chunk short
                lengths.add(e - b)
                if sizes[t] > E.CHUNK and e == offs[t] + sizes[t]:
                    last_of_many.add(e - b)
            assert covered == sizes
            assert [int(t) for t in tab["tensor"]] == sorted(int(t) for t in tab["tensor"])
    assert set(E.UNROLL_ENDS) <= lengths and set(E.UNROLL_ENDS) <= last_of_many | {E.UNROLL}
    assert {E.UNROLL - 8, E.UNROLL + 8, 2 * E.UNROLL + 8} <= last_of_many
    assert {E.CHUNK, E.CHUNK - 8, 8, 24, 1, 7, 9, 17, 3 * E.LANES * E.VEC, 3 * E.LANES * E.VEC + 8} <= lengths
    assert E.UNROLL == 4 * 256 * 8 and E.CHUNK % E.UNROLL == 0


def test_nan_sites():
    """the planted NaNs sit where the families say: first vector; last, partial vector of a chunk; last chunk of a
    multi-chunk tensor"""
    for store, sizes in E.STORES.items():
        t, i = E._nan_site(store, "nan_last_vec")
        assert i == min(sizes[t], E.CHUNK) - 1 and (sizes[t] % E.VEC or all(n % E.VEC == 0 for n in sizes))
        t, i = E._nan_site(store, "nan_last_chunk")
        assert i // E.CHUNK == (sizes[t] - 1) // E.CHUNK and sizes[t] == max(sizes)
        for fam in ("nan_first", "nan_last_vec", "nan_last_chunk"):
            gl = E.grads(store, fam, "bf16")
            assert sum(int(torch.isnan(g).sum()) for g in gl) == 1
    assert max(E.STORES["tails"]) > 2 * E.CHUNK and max(E.STORES["chunk"]) > 3 * E.CHUNK
    assert any(n % E.VEC for n in E.STORES["tails"]) and any(n % E.VEC for n in E.STORES["small"])


def test_scale_reference_covers_every_pattern():
    bits = E.all_bf16_patterns()
    assert bits.size == 65536 and len(set(bits.tolist())) == 65536
    ref, tiny = E.scale_reference(bits, 1.0)
    nan = (bits & 0x7FFF) > 0x7F80
    assert np.array_equal(ref[~nan], bits[~nan]) and bool((ref[nan] == E.NAN_BF_BITS).all())
    assert int(tiny.sum()) == 2 * 127          # the bf16 subnormals of either sign
    E.check_scaled(np.where(tiny, bits & 0x8000, ref).astype(np.uint16), bits, 1.0, "flushed subnormals pass")
    with pytest.raises(AssertionError):
        E.check_scaled(np.where(tiny, (bits ^ 0x8000) & 0x8000, ref).astype(np.uint16), bits, 1.0, "wrong sign")
    ref0, _ = E.scale_reference(bits, 0.0)
    assert bool((ref0[(bits & 0x7FFF) == 0x7F80] == E.NAN_BF_BITS).all())   # inf x 0
