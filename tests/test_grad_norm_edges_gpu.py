"""The global gradient norm and clip of csrc/adamw.hip (grad_sqnorm_kernel, tensor_sq_kernel, clip_coef_kernel,
otamd_grad_sqnorm_chunks / otamd_grad_clip_finalize / otamd_grad_clip_coef, otamd_scale_bf16_by_device_scalar) against
the float64 reference, the bound and the case table of _grad_norm_edges.py, whose truth test_grad_norm_edges_ref.py
establishes on the CPU: chunk and unroll boundaries, integer-exact sums, range launches, padding, zeros, non-finite
and extreme gradients, and every bf16 bit pattern through the scale kernel."""
import math

import numpy as np
import pytest
import torch

import _grad_norm_edges as E
from onetrainer_amd import _lib
from onetrainer_amd import kernels as K
from onetrainer_amd.module.param_store import FlatParamStore
from onetrainer_amd.util.optimizer.adamw_fused import FusedAdamW
from oracle import adamw as OA

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
PATHS = [f"{k} {f}" for k in ("tensor_sq", "total", "coef") for f in E.FORMS]


def make(dev, store, form):
    st = FlatParamStore(E.specs(store), torch.float32 if form == "f32" else BF, dev, master=form == "master")
    opt = FusedAdamW(st, [{"params": [st.params[n] for n in st.order]}], lr=1e-3, weight_decay=1e-2,
                     stochastic_rounding=False, seed=1)
    assert [st.slots[n].offset for n in st.order] == E.offsets(store)[0]
    return st, opt


def flat(store, tensors, dtype, fill=0.0):
    """the tensors at their offsets of the store's flat buffer (CPU)"""
    offs, numel = E.offsets(store)
    buf = torch.full((numel,), fill, dtype=dtype)
    for o, t in zip(offs, tensors):
        buf[o:o + t.numel()] = t.to(dtype)
    return buf


def valid_mask(store):
    return ~torch.isnan(flat(store, [torch.zeros(n) for n in E.STORES[store]], torch.float32, math.nan))


def load(st, store, gl):
    st.grad.copy_(flat(store, gl, st.grad.dtype))


def clip(opt, max_norm):
    """(total, coef, tensor_sq) of one clip_grad_norm_"""
    opt.clip_grad_norm_(max_norm)
    out = opt.clip_out.cpu()
    return float(out[1]), float(out[0]), opt._tensor_sq.cpu().numpy().copy()


def check_clip(form, got_total, got_coef, ref_total, ref_coef, what):
    rel = 0.0 if form == "bf16" else E.FOLD
    E.check_scalar(f"total {form}", got_total, ref_total, rel, what + " total")
    E.check_scalar(f"coef {form}", got_coef, ref_coef, rel, what + " coef")


@pytest.mark.parametrize("fam", E.FAMILIES_PARITY)
@pytest.mark.parametrize("form", E.FORMS)
@pytest.mark.parametrize("store", list(E.STORES))
def test_per_tensor_parity(dev, store, form, fam):
    st, opt = make(dev, store, form)
    load(st, store, E.grads(store, fam, form))
    r = E.reference(store, fam, form)
    assert len(r.max_norms) == 2
    for mx in r.max_norms:
        total, coef, tsq = clip(opt, mx)
        what = f"{store} {fam} {form} max_norm={mx!r}"
        E.check_tensor_sq(f"tensor_sq {form}", tsq, r.sq, what, exact=fam == "ints")
        check_clip(form, total, coef, *r.clip[mx], what)
    assert r.clip[r.max_norms[0]][1] < 1.0 and r.clip[r.max_norms[1]][1] == 1.0 and coef == 1.0


@pytest.mark.parametrize("form", E.FORMS)
def test_range_launches_match_one_call(dev, form):
    """otamd_grad_sqnorm_chunks over 1, 2 and 5 ranges of the chunk table (cuts inside multi-chunk tensors), then
    otamd_grad_clip_finalize: the bits of the one-call otamd_grad_clip_coef in every chunk slot, tensor and output"""
    store = "tails"
    st, opt = make(dev, store, form)
    load(st, store, E.grads(store, "normal", form))
    mx = E.reference(store, "normal", form).max_norms[0]
    opt.clip_grad_norm_(mx)
    n, nt = opt._n_chunks, len(st.order)
    want = (opt._chunk_sq[:n].clone(), opt._tensor_sq.clone(), opt.clip_out.clone())
    tensor = E.chunk_table(opt)["tensor"]
    inside = [c for c in range(1, n) if tensor[c - 1] == tensor[c]]
    assert n >= 10 and len(inside) >= 4
    lib, dtype = _lib.lib(), opt._norm_dtype
    for cuts in ([], [inside[1]], [inside[0], inside[0] + 1, inside[2], n - 1]):
        assert all(0 < c < n for c in cuts) and any(c in inside for c in cuts) == bool(cuts)
        chunk_sq = torch.full_like(opt._chunk_sq, -12345.0)   # a chunk no range wrote keeps the poison
        tensor_sq = torch.full_like(opt._tensor_sq, -12345.0)
        out = torch.full_like(opt.clip_out, -12345.0)
        edges = [0, *cuts, n]
        for b, e in reversed(list(zip(edges, edges[1:]))):   # backward finishes the last tensors first
            _lib.check(lib.otamd_grad_sqnorm_chunks(st.grad.data_ptr(), dtype, opt._chunks.data_ptr(), b, e,
                                                    chunk_sq.data_ptr(), K.stream_handle()), "otamd_grad_sqnorm_chunks")
        _lib.check(lib.otamd_grad_clip_finalize(opt._chunks.data_ptr(), n, chunk_sq.data_ptr(), tensor_sq.data_ptr(), nt,
                                                float(mx), dtype, out.data_ptr(), K.stream_handle()),
                   "otamd_grad_clip_finalize")
        got = (chunk_sq[:n], tensor_sq, out)
        for g, w, name in zip(got, want, ("chunk_sq", "tensor_sq", "clip_out")):
            assert torch.equal(g.view(torch.int64 if g.dtype == torch.float64 else torch.int32),
                               w.view(torch.int64 if w.dtype == torch.float64 else torch.int32)), (name, len(cuts) + 1)
        assert not bool((chunk_sq[:n] == -12345.0).any())


@pytest.mark.parametrize("form", E.FORMS)
@pytest.mark.parametrize("store", ["small", "tails", "many"])
def test_padding_belongs_to_no_chunk(dev, store, form):
    """NaN bit patterns in the gradient buffer's padding between tensors change nothing, and the norm pass leaves the
    gradient buffer as it found it"""
    st, opt = make(dev, store, form)
    load(st, store, E.grads(store, "normal", form))
    mx = E.reference(store, "normal", form).max_norms[0]
    total, coef, tsq = clip(opt, mx)
    pad = ~valid_mask(store)
    assert 0 < int(pad.sum()) < 8 * len(E.STORES[store])
    st.grad[pad.to(dev)] = math.nan
    ints = torch.int32 if form == "f32" else torch.int16
    before = st.grad.view(ints).clone()
    assert int(torch.isnan(st.grad).sum()) == int(pad.sum())
    total2, coef2, tsq2 = clip(opt, mx)
    assert (total2, coef2) == (total, coef) and np.array_equal(tsq2.view(np.int64), tsq.view(np.int64))
    assert torch.equal(st.grad.view(ints), before)
    E.check_tensor_sq(f"tensor_sq {form}", tsq2, E.reference(store, "normal", form).sq, f"{store} padded {form}")


def set_params(st, store, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    p = [torch.randn(n, generator=g) * 0.05 for n in E.STORES[store]]
    if st.master is not None:
        st.master.copy_(flat(store, p, torch.float32))
        st.data.copy_(st.master.to(BF))
    else:
        st.data.copy_(flat(store, p, st.data.dtype))


@pytest.mark.parametrize("form", E.FORMS)
@pytest.mark.parametrize("store", ["small", "chunk"])
def test_zero_gradients(dev, store, form):
    st, opt = make(dev, store, form)
    set_params(st, store, 3)
    load(st, store, E.grads(store, "zeros", form))
    total, coef, tsq = clip(opt, 1.0)
    assert total == 0.0 and coef == 1.0 and not tsq.any()
    assert E.reference(store, "zeros", form).clip[1.0] == (0.0, 1.0)
    opt.step()
    assert bool(torch.isfinite(st.data).all()) and bool(torch.isfinite(opt.exp_avg).all())
    assert st.master is None or bool(torch.isfinite(st.master).all())


@pytest.mark.parametrize("fam", E.FAMILIES_NONFINITE)
@pytest.mark.parametrize("form", E.FORMS)
@pytest.mark.parametrize("store", list(E.STORES))
def test_non_finite_gradients(dev, store, form, fam):
    """total and coefficient as torch gives them (test_grad_norm_edges_ref.py: the oracle's, NaN as NaN, inf -> 0), and
    one step with that pending coefficient turns exactly the elements non-finite that the oracle step does"""
    st, opt = make(dev, store, form)
    set_params(st, store, 4)
    gl = E.grads(store, fam, form)
    load(st, store, gl)
    r = E.reference(store, fam, form)
    assert r.max_norms == (1.0,)
    total, coef, _ = clip(opt, 1.0)
    ref_total, ref_coef = r.clip[1.0]
    what = f"{store} {fam} {form}"
    if fam.startswith("inf"):
        assert ref_total == math.inf and ref_coef == 0.0
    else:
        assert math.isnan(ref_total) and math.isnan(ref_coef)
    assert E.same(total, ref_total), (what, "total", total, ref_total)
    assert E.same(coef, ref_coef), (what, "coef", coef, ref_coef)
    if form == "f32":
        return
    valid = valid_mask(store).numpy()
    g_bits = E.bits16(st.grad)
    zeros = np.zeros(st.numel, np.float32)
    with np.errstate(all="ignore"):
        if form == "bf16":
            p, _, _ = OA.adamw_step_bf16(E.bits16(st.data), g_bits, np.zeros(st.numel, np.uint16),
                                         np.zeros(st.numel, np.uint16), 1, 1e-3, clip_coef=np.float32(coef))
            want = np.isfinite(OA.bf16_to_f32(p))
        else:
            p, _, _, _ = OA.adamw_step_master(st.master.cpu().numpy(), g_bits, zeros, zeros, 1, 1e-3,
                                              clip_coef=np.float32(coef))
            want = np.isfinite(p)
    opt.step()
    got = torch.isfinite(st.master if form == "master" else st.data).cpu().numpy()
    assert np.array_equal(got[valid], want[valid]), (what, int((got != want)[valid].sum()))
    if form == "master":
        assert np.array_equal(torch.isfinite(st.data).cpu().numpy()[valid], want[valid]), what
    offs, _ = E.offsets(store)
    per_tensor = [bool(want[o:o + n].all()) or not bool(want[o:o + n].any()) for o, n in zip(offs, E.STORES[store])]
    assert fam.startswith("inf") or (all(per_tensor) and not want[valid].any())   # NaN: every parameter is NaN


@pytest.mark.parametrize("fam", E.FAMILIES_EXTREME)
@pytest.mark.parametrize("form", E.FORMS)
@pytest.mark.parametrize("store", E.EXTREME_STORES)
def test_extremes(dev, store, form, fam):
    """the conditions test_grad_norm_edges_ref.py recorded from torch on the CPU"""
    st, opt = make(dev, store, form)
    gl = E.grads(store, fam, form)
    load(st, store, gl)
    total, coef, _ = clip(opt, 1.0)
    t_total, t_coef, _ = E.torch_clip(gl, form, 1.0)
    what = f"{store} {fam} {form}"
    if fam == "small70":
        assert t_total > 0 and t_coef == 1.0
        assert 0.0 <= total <= t_total and coef == 1.0, (what, total, t_total, coef)
    elif not math.isfinite(t_total):
        assert t_total == math.inf and t_coef == 0.0 and (fam == "big66" or store == "unroll")
        assert total == math.inf and coef == 0.0, (what, total, coef)
    else:
        for mx in (1.0, 2.0 ** -22):
            total, coef, _ = clip(opt, mx)
            check_clip(form, total, coef, *E.oracle_clip(gl, form, mx), what + f" max_norm={mx!r}")


def test_scale_bf16_by_device_scalar_every_pattern(dev):
    """all 65 536 bf16 patterns (and three vectors more, so the last workgroup is partial: the entry point takes whole
    16-byte vectors only) 16 bytes into a guarded buffer, times each device scalar"""
    bits = np.concatenate([E.all_bf16_patterns(), E.all_bf16_patterns()[0x3F80:0x3F80 + 24]])
    n, lead, tail = bits.size, 8, 40
    assert n % 8 == 0 and (n // 8) % 256 != 0
    src = torch.from_numpy(bits.astype(np.int16))
    r = E.reference("unroll", "normal", "bf16")
    clip_coef = r.clip[r.max_norms[0]][1]
    assert 0 < clip_coef < 1
    for coef in (1.0, 0.0, 0.37, 2.0 ** -20, clip_coef, math.nan):
        buf = torch.full((lead + n + tail,), E.NAN_BF_BITS, dtype=torch.int16, device=dev)
        buf[lead:lead + n] = src.to(dev)
        c = torch.tensor([coef], dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().otamd_scale_bf16_by_device_scalar(buf[lead:].data_ptr(), n, c.data_ptr(),
                                                                K.stream_handle()), "otamd_scale_bf16_by_device_scalar")
        got = buf.cpu().numpy().astype(np.uint16)
        assert (got[:lead] == E.NAN_BF_BITS).all() and (got[lead + n:] == E.NAN_BF_BITS).all(), coef
        E.check_scaled(got[lead:lead + n], bits, coef, f"scale by {coef!r}")
        E.note("scale_bf16", 0.0, f"coef {coef!r}")


def test_worst_ratios_report():
    """the worst |err| / bound of every path whose tests ran in this process; all at most 1"""
    rows = {k: v for k, v in E.WORST.items() if not k.startswith("cpu:")}
    print()
    for k in sorted(rows):
        print(f"{k:24s} {rows[k][0]:8.3f}  {rows[k][1]}")
    missing = [k for k in PATHS if k not in rows]
    if missing:
        print("not run in this process:", missing)
    assert all(v[0] <= 1 for v in rows.values())
