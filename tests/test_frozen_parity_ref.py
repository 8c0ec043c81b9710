"""The frozen-network bounds of _frozen_parity.py, held to the reference alone (no GPU): the measured noise of the bf16
CPU oracle against the float64 oracle is what the helper records, the bounds stay inside the cap, the row floor engages
on at most 5 % of a case's rows, an honest fp32 evaluation passes, and every planted glue error leaves a bound by a
factor of two."""
import pytest
import torch

import _frozen_parity as P


@pytest.mark.parametrize("case", P.CASES)
def test_bounds_measured(case):
    """k_rel and k_s recomputed: K_MEASURED holds what this shows (within a tenth: torch's CPU bf16 routines differ
    between builds), on the same output, and the unmodified bf16 outputs pass both bounds."""
    ref, b = P.reference(case), P.bf16_oracle(case)
    w = P.worst(b, ref)
    s_bound, rel_bound = P.BOUNDS[P.family(case)]
    print(f"{case}: k_rel {w['rel'][0]:.4f} ({w['rel'][1]} at {w['rel'][2]})  k_s {w['s'][0]:.5f} ({w['s'][1]})  "
          f"bounds {rel_bound} {s_bound}")
    rec = P.K_MEASURED[case]
    assert abs(w["rel"][0] - rec["k_rel"][0]) <= 0.1 * rec["k_rel"][0] + 5e-5, (w["rel"], rec["k_rel"])
    assert abs(w["s"][0] - rec["k_s"][0]) <= 0.1 * rec["k_s"][0] + 5e-5, (w["s"], rec["k_s"])
    assert w["rel"][0] <= rel_bound / 4 and w["s"][0] <= s_bound / 4
    assert not P.failures(b, ref, P.family(case))


def test_bounds_are_four_k_inside_the_cap():
    assert set(P.K_MEASURED) == set(P.CASES)
    for fam in ("text", "vae"):
        rows = [v for c, v in P.K_MEASURED.items() if P.family(c) == fam]
        ks, kr = max(v["k_s"][0] for v in rows), max(v["k_rel"][0] for v in rows)
        s_bound, rel_bound = P.BOUNDS[fam]
        assert s_bound == 4 * P.ceil2(ks) and rel_bound == 4 * P.ceil2(kr)
        assert P.ceil2(ks) - ks < 0.1 * ks and P.ceil2(kr) - kr < 0.1 * kr       # one step up, no more
        assert 0 < s_bound <= P.CAP and 0 < rel_bound <= P.CAP
        for c, v in P.K_MEASURED.items():
            if P.family(c) == fam:
                assert 4 * P.ceil2(v["k_rel"][0]) <= P.CAP and 4 * P.ceil2(v["k_s"][0]) <= P.CAP, c


@pytest.mark.parametrize("case", P.CASES)
def test_row_floor_share(case):
    """on the float64 reference alone: at most 5 % of the case's rows lie under a quarter of their tensor's rms row
    norm; every output is finite and none is identically zero"""
    ref = P.reference(case)
    w = P.worst(ref, ref)
    print(f"{case}: {w['floored']} of {w['rows']} rows under the floor")
    assert w["floored"] <= P.FLOOR_SHARE * w["rows"]
    assert all(torch.isfinite(r).all() and torch.count_nonzero(r) for r in ref.values())


@pytest.mark.parametrize("case", P.CASES)
def test_fp32_oracle_passes(case):
    """the oracle in its default dtype passes both bounds, and lies under a tenth of the bf16 oracle's own noise: fp32
    rounds 2 ** 16 times finer than bf16, of which the 1 + erf(x) of the deep-tail MLP units (2e-4 at -3.6) gives
    back twelve bits by cancellation (3.5e-4 on clip_g_tiny's last_hidden_state)"""
    got = P.outputs(case, torch.float32)
    w = P.check(got, P.reference(case), f"{case} fp32", P.family(case))
    rec = P.K_MEASURED[case]
    assert w["rel"][0] < 0.1 * rec["k_rel"][0] and w["s"][0] < 0.1 * rec["k_s"][0]


def test_cases_are_the_stated_ones():
    """the token rows and shapes the docstring promises"""
    ids = P.clip_ids()
    assert ids.shape == (P.B, P.T) == (3, 77) and int(ids.max()) == P.EOS_CLIP
    assert ids.argmax(-1).tolist() == [1, 76, 31]
    assert ids[0, 2:].eq(0).all() and ids[2, 31:].eq(P.EOS_CLIP).all() and ids[1].ne(0).all()
    t = P.t5_ids()
    assert [int((row == P.EOS_T5).nonzero()[0]) for row in t] == [2, 32, 76]
    assert t[0, 3:].eq(0).all() and t[1, 33:].eq(0).all()
    # |q - c| on both sides of every bucket boundary up to 76, both signs, and t5_h64 reaches the clamped last bucket
    from oracle import text_encoder as OT
    rel = OT.t5_relative_position(P.T)
    for c in P.T5_CFGS.values():
        bk = OT.t5_bucket(rel, c.relative_attention_num_buckets, c.relative_attention_max_distance)
        first = bk[0]                                   # q = 0: c - q = 0 .. 76
        edges = [n for n in range(1, P.T) if first[n] != first[n - 1]]
        assert len(edges) >= 13 and all(0 < n <= 76 for n in edges)
        assert torch.equal(bk[1:, 0] + 16, first[1:])   # c - q = -1 .. -76: the same buckets on the negative side
    far = OT.t5_bucket(rel, 32, P.T5_CFGS["t5_h64"].relative_attention_max_distance)
    assert int(far.max()) == 31 and int(OT.t5_bucket(rel, 32, 128).max()) == 30
    assert P.CLIP_CFGS["clip_h64"].hidden_size // P.CLIP_CFGS["clip_h64"].num_attention_heads == 64
    assert P.T5_CFGS["t5_h64"].d_kv == 64 and P.T5_CFGS["t5_h64"].num_heads == 8
    assert P.VAE_CFGS["three"].block_out_channels == (64, 96, 160)
    assert {tuple(v.shape[1:3]) for v in P.reference("enc_tiny4").values()} == {(5, 7), (8, 12)}
    assert {tuple(v.shape[1:3]) for v in P.reference("enc_three").values()} == {(5, 7)}
    assert {tuple(v.shape[1:3]) for v in P.reference("dec_tiny16").values()} == {(10, 14), (16, 16)}


def test_default_dtype_oracle_is_unchanged():
    """dtype defaults to fp32: the same bits as an explicit float32, and fp32 outputs"""
    from oracle import text_encoder as OT
    c = P.CLIP_CFGS["clip_g_tiny"]
    a = OT.clip_forward(P.text_weights("clip_g_tiny"), P.clip_ids(), c.num_attention_heads, c.hidden_act)
    b = OT.clip_forward(P.text_weights("clip_g_tiny"), P.clip_ids(), c.num_attention_heads, c.hidden_act,
                        dtype=torch.float32)
    assert a[1].dtype == torch.float32 and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    t = P.T5_CFGS["t5_tiny"]
    h = OT.t5_forward(P.text_weights("t5_tiny"), P.t5_ids(), t.num_heads)
    assert h[-1].dtype == torch.float32


@pytest.mark.parametrize("name", list(P.PLANTED))
def test_planted_error_fails(name):
    """the float64 oracle with one piece of glue wrong: on at least one checked output of at least one case its worst
    rel_row or its |s - 1| is at least twice the bound; outside the block the oracle is whole again."""
    cases, _ = P.PLANTED[name]
    assert cases
    best = 0.0
    for case in cases:
        ref = P.reference(case)
        with P.planted(name):
            got = P.outputs(case, torch.float64)
        s_bound, rel_bound = P.BOUNDS[P.family(case)]
        w = P.worst(got, ref)
        ratio = max(w["rel"][0] / rel_bound, w["s"][0] / s_bound)
        print(f"{name} in {case}: rel_row {w['rel'][0]:.4f} ({w['rel'][1]} at {w['rel'][2]})  |s-1| {w['s'][0]:.5f} "
              f"({w['s'][1]})  = {ratio:.1f} x the bound")
        best = max(best, ratio)
        assert not P.failures(P.outputs(case, torch.float64), ref, P.family(case), 1e-6), "the plant outlived its block"
    assert best >= 2.0, f"{name}: at most {best:.2f} x the bound"
