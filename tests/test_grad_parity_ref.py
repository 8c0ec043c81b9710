"""The network-level gradient bounds of _grad_parity.py, held to the reference alone (no GPU): the measured noise of
the bf16 CPU oracle against the float64 oracle is what the helper records, both bounds stay inside the cap, no case has
a zero reference gradient, and the metrics catch every planted scale or accumulation error."""
import pytest
import torch

import _grad_parity as G


@pytest.mark.parametrize("case", G.CASES)
def test_bounds_measured(case):
    """k_s and k_rel recomputed: the bf16 oracle against the float64 oracle, one backward (A) and two backward passes
    into one .grad (A then B), the larger of the two.  K_MEASURED holds what this shows (within a tenth: torch's CPU
    bf16 routines differ between builds), each bound is 4 x the worst recorded k taken up at its second digit, and no
    more, and neither exceeds the cap.  The unmodified bf16 gradients pass both bounds."""
    ref, b = G.reference(case), G.bf16_oracle(case)
    ws = [G.worst(b[f], ref[f]) for f in ("A", "AB")]
    k_s, k_rel = max(w["s"] for w in ws), max(w["rel"] for w in ws)
    print(f"{case}: k_s {k_s[0]:.4f} ({k_s[1]})  k_rel {k_rel[0]:.4f} ({k_rel[1]})  bounds {G.S_BOUND} {G.REL_BOUND}")
    rec = G.K_MEASURED[case]
    assert abs(k_s[0] - rec["k_s"][0]) <= 0.1 * rec["k_s"][0] + 5e-5, (k_s, rec["k_s"])
    assert abs(k_rel[0] - rec["k_rel"][0]) <= 0.1 * rec["k_rel"][0] + 5e-5, (k_rel, rec["k_rel"])
    assert k_s[0] <= G.S_BOUND / 4 and k_rel[0] <= G.REL_BOUND / 4
    for f in ("A", "B", "AB"):
        assert not G.failures(b[f], ref[f]), f


def test_bounds_are_four_k_inside_the_cap():
    assert set(G.K_MEASURED) == set(G.CASES)
    ks = max(v["k_s"][0] for v in G.K_MEASURED.values())
    kr = max(v["k_rel"][0] for v in G.K_MEASURED.values())
    assert G.S_BOUND == 4 * G.ceil2(ks) and G.REL_BOUND == 4 * G.ceil2(kr)
    assert G.ceil2(ks) - ks < 0.1 * ks and G.ceil2(kr) - kr < 0.1 * kr       # one step up, no more
    assert 0 < G.S_BOUND <= G.CAP and 0 < G.REL_BOUND <= G.CAP
    assert (G.ceil2(0.0143), G.ceil2(0.043), G.ceil2(1.822), G.ceil2(0.02)) == (0.015, 0.043, 1.9, 0.02)


@pytest.mark.parametrize("case", G.CASES)
def test_no_zero_reference_gradients(case):
    """every trained tensor of every case has a float64 gradient that is not identically zero, in each micro-batch
    and in their sum, so every tensor has a scale"""
    ref = G.reference(case)
    c = G.make_case(case)
    want = set(c["lora_sd"]) if c["lora"] else set(c["weights"])
    for f in ("A", "B", "AB"):
        assert set(ref[f]) == want
        zero = [k for k, r in ref[f].items() if torch.count_nonzero(r) == 0]
        assert not zero, (f, zero)
        assert all(torch.isfinite(r).all() for r in ref[f].values())


def test_zero_reference_is_compared_exactly():
    r = {"a": torch.zeros(5, dtype=torch.float64)}
    assert G.metrics(torch.zeros(5), r["a"]) is None
    assert not G.failures({"a": torch.zeros(5)}, r)
    assert G.failures({"a": torch.tensor([0., 0., 1e-30, 0., 0.])}, r)
    assert G.failures({"a": torch.full((3,), float("nan"))}, {"a": torch.ones(3, dtype=torch.float64)})


def _planted_tensors(c):
    """a bias, a norm weight, a conv weight (UNets), an attention projection, and for the adapter cases a LoRA down"""
    names = list(c["lora_sd"] if c["lora"] else c["weights"])
    if c["lora"]:
        pats = ("to_q.lora_down", "to_out.0.lora_up", ".ff.net.2.lora_down", "time_emb_proj.lora_down",
                "linear_1.lora_down", "conv1.lora_down", "proj_mlp.lora_up")
    else:
        pats = ("conv1.bias", "to_out.0.bias", "norm2.weight", "norm_q.weight", "conv2.weight", "conv_in.weight",
                "attn1.to_q.weight", "attn2.to_v.weight", "attn.to_k.weight", "proj_out.weight", "ff.net.2.bias",
                "norm1.linear.weight")
    out = []
    for p in pats:
        hit = [n for n in names if n.endswith(p + ("" if p.endswith(("weight", "bias")) else ".weight"))]
        if hit:
            out.append(hit[len(hit) // 2])
    assert len(out) >= 5, out
    return out


@pytest.mark.parametrize("case", G.CASES)
def test_metrics_catch_planted_errors(case):
    """one tensor at a time: x 2, x 0.5, x (1 + 2 S_BOUND) on the one-pass gradients; only the second micro-batch,
    and the first micro-batch twice, on the two-pass gradients.  Each must leave a bound."""
    c, ref, b = G.make_case(case), G.reference(case), G.bf16_oracle(case)
    for name in _planted_tensors(c):
        one = (lambda g, f: G.failures({name: g}, {name: ref[f][name]}))
        assert not one(b["A"][name], "A") and not one(b["AB"][name], "AB"), name
        for fac in (2.0, 0.5, 1 + 2 * G.S_BOUND, -1.0):
            assert one(b["A"][name] * fac, "A"), (name, fac)
        assert one(b["B"][name], "AB"), (name, "second micro-batch only")
        assert one(b["A"][name], "AB"), (name, "first micro-batch only")
        assert one(b["AB"][name] + b["A"][name], "AB"), (name, "first micro-batch twice")
        assert one(b["B"][name], "A"), (name, "the other micro-batch's gradient")
