"""The frozen HIP networks (module/text_encoder.py, module/vae.py) against the float64 table of _frozen_parity.py, per
row: every token of every hidden state and every pixel of every latent and image within REL_BOUND of the oracle, every
tensor's scale within S_BOUND (bounds measured on the CPU, test_frozen_parity_ref.py).  Also: the same bits through the
native host layer and through kernels.python_host(), and the same bits when a case's rows run as B = 1 calls."""
import dataclasses
import functools

import pytest
import torch

import _frozen_parity as P

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _same_fields(mine, oracle_cfg):
    for k in type(oracle_cfg).__dataclass_fields__:      # the oracle's configuration is the HIP model's
        assert getattr(mine, k) == getattr(oracle_cfg, k), k
    return mine


@functools.lru_cache(maxsize=None)
def _text_encoder(name, dev):
    from onetrainer_amd.module import text_encoder as TE
    if name in P.CLIP_CFGS:
        cfg = TE.CLIPTextConfig(**dataclasses.asdict(P.CLIP_CFGS[name]))
        if name == "clip_l_tiny":
            assert cfg == TE.tiny_clip_config(False)
        if name == "clip_g_tiny":
            assert cfg == TE.tiny_clip_config(True)
        enc = TE.CLIPTextEncoder(_same_fields(cfg, P.CLIP_CFGS[name]), dev, seed=0)
    else:
        cfg = TE.T5Config(**dataclasses.asdict(P.T5_CFGS[name]))
        if name == "t5_tiny":
            assert cfg == TE.tiny_t5_config()
        enc = TE.T5TextEncoder(_same_fields(cfg, P.T5_CFGS[name]), dev, seed=0)
    enc.load_state_dict(P.text_weights(name))
    return enc


@functools.lru_cache(maxsize=None)
def _vae(name, half, dev):
    from onetrainer_amd.module import vae as V
    cfg = _same_fields(V.VAEConfig(**dataclasses.asdict(P.VAE_CFGS[name])), P.VAE_CFGS[name])
    if name == "tiny4":
        assert cfg == V.tiny_vae_config()
    if name == "tiny16":
        assert cfg == V.tiny_vae_config(16, False)
    m = (V.AutoencoderKLEncoder if half == "enc" else V.AutoencoderKLDecoder)(cfg, dev, seed=None)
    m.load_state_dict(P.vae_weights(name, half))
    return m


def hip_outputs(case, dev, rows=slice(None)):
    """the outputs of _frozen_parity.outputs from the HIP networks, for the batch rows `rows`, as CPU tensors"""
    from onetrainer_amd.module import text_encoder as TE
    out = {}
    if case in P.CLIP_CFGS:
        enc, ids = _text_encoder(case, dev), P.clip_ids()[rows].to(dev)
        hs, last = enc.forward(ids, set(range(enc.cfg.num_hidden_layers + 1)))
        out = {f"hidden_states[{i}]": hs[i] for i in sorted(hs)}
        out["last_hidden_state"] = last.view(*ids.shape, -1)
        out["pooled"] = enc.pooled(ids, last)
        for dl, skip, ln in P.ENCODE_SELECTIONS:
            out[f"encode({dl},{skip},{ln})"] = enc.encode(ids, default_layer=dl, layer_skip=skip, add_layer_norm=ln)[0]
    elif case in P.T5_CFGS:
        enc, ids = _text_encoder(case, dev), P.t5_ids()[rows].to(dev)
        hs, _ = enc.forward(ids, set(range(enc.cfg.num_layers + 1)))
        out = {f"hidden_states[{i}]": hs[i] for i in sorted(hs)}
        out["encode"] = enc.encode(ids)
        out["encode(skip 1)"] = enc.encode(ids, layer_skip=1)
    elif case in P.FAMILY_CASES:
        l, g, t = (_text_encoder(n, dev) for n in ("clip_l_tiny", "clip_g_tiny", "t5_tiny"))
        i0, i1, it = P.clip_ids()[rows].to(dev), P.clip_ids(1)[rows].to(dev), P.t5_ids()[rows].to(dev)
        out = {"sdxl": lambda: TE.encode_sdxl_text(l, g, i0, i1), "sd15": lambda: TE.encode_sd15_text(l, i0),
               "flux": lambda: TE.encode_flux_text(l, t, i0, it)}[case]()
    else:
        half, name = case.split("_")
        m = _vae(name, half, dev)
        if half == "enc":
            f = 1 << (len(m.cfg.block_out_channels) - 1)
            for h, w in P.ENC_IMAGES[name]:
                lat = m.encode(P.image(h, w)[rows].to(dev))
                assert lat.dtype == torch.float32
                out[f"mean@{h // f}x{w // f}"] = lat
        else:
            for h, w in P.DEC_LATENTS:
                img = m.decode(P.latent(name, h, w)[rows].to(dev))
                assert img.shape[-1] == 8 and img.dtype == BF
                assert torch.count_nonzero(img[..., 3:]) == 0, "the pad channels of the decoder's output are not zero"
                out[f"rgb@{h}x{w}"] = img[..., :3]
    torch.cuda.synchronize()
    return {k: v.detach().float().cpu() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _batched(case, dev):
    return hip_outputs(case, dev)


@pytest.mark.parametrize("case", P.CASES)
def test_matches_float64_oracle(dev, case):
    got = _batched(case, dev)
    assert set(got) == set(P.reference(case))
    P.check(got, P.reference(case), case, P.family(case))


@pytest.mark.parametrize("case", P.CASES)
def test_python_host_same_bits(dev, case):
    """the native host layer and the Python launch path run the same kernels on the same plans"""
    from onetrainer_amd import kernels as K
    got = _batched(case, dev)
    with K.python_host():
        other = hip_outputs(case, dev)
    bad = [k for k in got if not torch.equal(got[k], other[k])]
    assert not bad, bad


@pytest.mark.parametrize("case", P.CASES)
def test_rows_do_not_depend_on_batch_neighbours(dev, case):
    """every batch row run alone (B = 1) gives the bits it has inside the batch of three"""
    got = _batched(case, dev)
    bad = []
    for b in range(P.B):
        one = hip_outputs(case, dev, slice(b, b + 1))
        for k in got:
            if not torch.equal(one[k][0], got[k][b]):
                d = (one[k][0] - got[k][b]).abs()
                bad.append((k, b, int((d > 0).sum()), float(d.max())))
    assert not bad, f"(output, batch row, elements that differ, max |difference|): {bad[:8]}"


def test_report_worst_ratios(dev):
    """the table of DESIGN.md: per network the worst rel_row / REL_BOUND and |s - 1| / S_BOUND over its cases"""
    nets = {"CLIP": tuple(P.CLIP_CFGS), "T5": tuple(P.T5_CFGS), "encode_*_text": tuple(P.FAMILY_CASES),
            "VAE encoder": tuple(c for c in P.VAE_CASES if c.startswith("enc")),
            "VAE decoder": tuple(c for c in P.VAE_CASES if c.startswith("dec"))}
    for net, cases in nets.items():
        rel, s = (0.0, None), (0.0, None)
        for c in cases:
            w = P.worst(_batched(c, dev), P.reference(c))
            s_bound, rel_bound = P.BOUNDS[P.family(c)]
            rel = max(rel, (w["rel"][0] / rel_bound, f"{c} {w['rel'][1]} at {w['rel'][2]}"))
            s = max(s, (w["s"][0] / s_bound, f"{c} {w['s'][1]}"))
        print(f"RATIO {net}: rel_row / REL_BOUND {rel[0]:.3f} ({rel[1]})  |s-1| / S_BOUND {s[0]:.3f} ({s[1]})")
        assert rel[0] <= 1.0 and s[0] <= 1.0
