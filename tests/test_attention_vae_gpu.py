"""Flash attention forward for the VAE's 512-wide head (csrc/attention_vae.hip, kernels.attn_xwide_fwd) against
float64 softmax(scale q k^T) v on the CPU from the same bf16 inputs, at the edges of its tiles (128 queries per
workgroup, 32 keys per tile), and the AutoencoderKL mid block's route to it (module/vae.py)."""
import pytest
import torch

from onetrainer_amd import kernels as K
from onetrainer_amd.module import vae as V
from oracle import vae as OV

D = 512
CASES = [(1, 1, 128, 1), (1, 1, 1, 101),                              # one key; one query
         (1, 1, 127, 101), (1, 1, 128, 101), (1, 1, 129, 101),        # query tile - 1, tile, tile + 1; 3 key tiles + 5
         (1, 1, 128, 31), (1, 1, 128, 32), (1, 1, 128, 33),           # key tile - 1, tile, tile + 1
         (2, 1, 300, 171),                                            # slices of one fused [B, N, 3 D] buffer
         (1, 2, 129, 70)]                                             # two heads (C = 1024)


def _ref(q, k, v, heads, scale):
    """float64 softmax(scale q k^T) v per head, [B, Nq, H, D]"""
    B, Nq, _ = q.shape
    q, k, v = (t.double().cpu().view(B, t.shape[1], heads, -1).transpose(1, 2) for t in (q, k, v))
    return (torch.softmax(scale * q @ k.transpose(-1, -2), -1) @ v).transpose(1, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["normal", "peaked"])
@pytest.mark.parametrize("B,H,Nq,Nk", CASES)
def test_xwide_fwd_rows(dev, B, H, Nq, Nk, family):
    """per output row: max |o - o_ref| <= 2^-9 max |o_ref| (bf16 output rounding) + 2 e_mat, e_mat the same row's
    error of the materialized path (both round P to bf16: the flash form the unnormalised exp, the other the
    normalised p).  Worst measured ratio error / bound: DESIGN.md."""
    g = torch.Generator().manual_seed(Nq * 1000 + Nk)
    C, scale = H * D, D ** -0.5
    q, k, v = (torch.randn(B, n, C, generator=g) for n in (Nq, Nk, Nk))
    if family == "peaked":   # query i points at key (7 i + 3) % Nk: that score leads the row by more than 60
        idx = (7 * torch.arange(Nq) + 3) % Nk
        q = 6.0 * k.view(B, Nk, H, D)[:, idx].reshape(B, Nq, C)
    if B == 2:   # column slices of one buffer, token stride 3 C
        buf = torch.zeros(B, max(Nq, Nk), 3 * C)
        buf[:, :Nq, :C], buf[:, :Nk, C:2 * C], buf[:, :Nk, 2 * C:] = q, k, v
        buf = buf.bfloat16().to(dev)
        q, k, v = buf[:, :Nq, :C], buf[:, :Nk, C:2 * C], buf[:, :Nk, 2 * C:]
    else:
        q, k, v = (t.bfloat16().to(dev) for t in (q, k, v))
    ref = _ref(q, k, v, H, scale)
    if family == "peaked" and Nk > 1:
        s = scale * q.double().cpu().view(B, Nq, H, D).transpose(1, 2) @ k.double().cpu().view(B, Nk, H, D).permute(
            0, 2, 3, 1)
        top = s.topk(2, -1).values
        assert (top[..., 0] - top[..., 1]).min() > 60
    out = torch.full((B, Nq + 3, C), 7.0, dtype=torch.bfloat16, device=dev)
    o = K.attn_xwide_fwd(q, k, v, H, out=out[:, :Nq])
    assert o.data_ptr() == out.data_ptr() and torch.all(out[:, Nq:] == 7.0)
    o_mat, _ = K.attn_mat_fwd(q, k, v, H)
    err = (o.double().cpu().view(B, Nq, H, D) - ref).abs().amax(-1)
    e_mat = (o_mat.double().cpu().view(B, Nq, H, D) - ref).abs().amax(-1)
    bound = 2.0 ** -9 * ref.abs().amax(-1) + 2 * e_mat
    print(f"xwide {family} {(B, H, Nq, Nk)}: worst error / bound {(err / bound).max().item():.3f}")
    assert torch.all(err <= bound), (err / bound).max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("flash", [True, False])
def test_vae_mid_attention_route(dev, monkeypatch, flash):
    """a 512-channel mid block on a 16 x 16 latent (256 tokens), encoder and decoder, against the float64 oracle
    with the bound of tests/test_vae_gpu.py / tests/test_vae_decoder_gpu.py; the flash route (threshold 0) never
    calls attn_mat_fwd, the default threshold keeps these 256 tokens on it"""
    calls = []
    real = K.attn_mat_fwd
    monkeypatch.setattr(K, "attn_mat_fwd", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    if flash:
        monkeypatch.setattr(K, "VAE_FLASH_MIN_TOKENS", 0)
    torch.manual_seed(0)
    cfg = V.VAEConfig(block_out_channels=(64, 512), layers_per_block=1)
    enc, dec = V.AutoencoderKLEncoder(cfg, dev, seed=1), V.AutoencoderKLDecoder(cfg, dev, seed=2)
    img = torch.rand(2, 3, 32, 32)
    lat = torch.randn(2, 16, 16, 4) * cfg.scaling_factor * 1.5
    got_e = enc.encode(img.to(dev)).cpu()
    got_d = dec.decode(lat.to(dev))[..., :3].float().cpu()
    assert len(calls) == (0 if flash else 2)
    oe, od = OV.AutoencoderKLEncoder(cfg, torch.float64), OV.AutoencoderKLDecoder(cfg, torch.float64)
    oe.load_state_dict({k: v.double().cpu() for k, v in enc.state_dict().items()})
    od.load_state_dict({k: v.double().cpu() for k, v in dec.state_dict().items()})
    with torch.no_grad():
        want_e = oe.moments((img * 2 - 1).bfloat16().double())[:, :cfg.latent_channels].permute(0, 2, 3, 1)
        want_d = od((lat / cfg.scaling_factor).bfloat16().double().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    for name, got, want in (("encoder", got_e, want_e), ("decoder", got_d, want_d)):
        err = ((got - want).abs().max() / want.abs().max()).item()
        a, b = got.flatten().double(), want.flatten()
        cos = (a @ b / (a.norm() * b.norm() + 1e-30)).item()
        print(f"{name} flash={flash}: rel err {err:.3e}, cosine {cos:.6f}")
        assert err < 3e-2 and cos > 0.9995, (name, err, cos)


def test_xwide_contract():
    """only the instantiated widths: 500 is none, and 160 belongs to attn_fwd"""
    for d in (500, 160):
        x = torch.zeros(1, 4, d, dtype=torch.bfloat16)
        with pytest.raises(ValueError, match="head dim must be one of"):
            K.attn_xwide_fwd(x, x, x, 1)
