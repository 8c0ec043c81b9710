"""Training the mask-input (inpainting) model types: the 9-channel UNet input through predict, loss, backward, LoRA /
DoRA, backup / resume, the stream-hazard check and the captured step, on tiny UNets with a batch of 2 at 128x128."""
import pytest
import torch

from onetrainer_amd import kernels as K
from onetrainer_amd.dataLoader.SyntheticDataLoader import synthetic_sdxl_batch
from onetrainer_amd.module import unet as U
from onetrainer_amd.module.stream_hazards import StreamHazardCheck
from onetrainer_amd.trainer.GenericTrainer import GenericTrainer
from onetrainer_amd.util import create
from onetrainer_amd.util.config.TrainConfig import TrainConfig

pytestmark = pytest.mark.gpu

SDXL, SD15 = "STABLE_DIFFUSION_XL_10_BASE_INPAINTING", "STABLE_DIFFUSION_15_INPAINTING"


def _ucfg(sdxl=True, in_channels=9):
    u = U.tiny_sdxl_config() if sdxl else U.tiny_sd15_config()
    u.in_channels = in_channels
    return u


def _cfg(sdxl=True, **kw):
    cfg = TrainConfig.default_values()
    cfg.model_type = SDXL if sdxl else SD15
    cfg.batch_size = 2
    cfg.learning_rate = 1e-4
    cfg.learning_rate_warmup_steps = 0
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _trainer(cfg, dev, sdxl=True, in_channels=9):
    model = create.create_model(cfg, dev, seed=3, unet_config=_ucfg(sdxl, in_channels))
    tr = GenericTrainer(cfg, model=model)
    tr.start()
    return tr


def _batch(dev, sdxl=True, seed=1, trivial=False):
    """trivial: mask == 1 and conditioning latent == blank, what a removed mask is replaced by"""
    sf = 0.13025 if sdxl else 0.18215
    if sdxl:
        b = synthetic_sdxl_batch(2, 128, 128, dev, seed=seed, te1_dim=48, te2_dim=48, pooled_dim=64)
    else:
        b = synthetic_sdxl_batch(2, 128, 128, dev, seed=seed, te1_dim=96, sdxl=False, scaling_factor=sf)
    g = torch.Generator().manual_seed(seed + 100)
    blank = torch.randn(16, 16, 4, generator=g) / sf
    mask = (torch.rand(2, 1, 16, 16, generator=g) > 0.5).float()
    cond = torch.randn(2, 16, 16, 4, generator=g) / sf
    if trivial:
        mask, cond = torch.ones_like(mask), blank[None].expand(2, 16, 16, 4).contiguous()
    b["latent_mask"] = mask.to(dev)
    b["latent_conditioning_image"] = cond.to(dev).permute(0, 3, 1, 2)
    b["latent_blank"] = blank.to(dev)
    return b


@pytest.mark.parametrize("sdxl", [True, False], ids=["sdxl", "sd15"])
def test_fine_tune_steps_and_conv_in_gradient(dev, sdxl):
    tr = _trainer(_cfg(sdxl), dev, sdxl)
    model = tr.model
    w = model.unet.store.params["conv_in.weight"]
    assert w.shape[1:] == (3, 3, 16) and not w[..., 9:].any()
    grads, opt_step = [], model.optimizer.step

    def step(*a, **k):
        grads.append(w.grad.clone())
        return opt_step(*a, **k)

    model.optimizer.step = step
    batch = _batch(dev, sdxl)
    losses = [tr.train_step(batch).item() for _ in range(2)]
    torch.cuda.synchronize()
    assert all(l == l and abs(l) < 1e4 for l in losses), losses
    for g in grads:
        assert torch.isfinite(g.float()).all()
        for c in range(4, 9):   # the mask and the conditioning latent reach the weight gradient
            assert g[..., c].any(), c
        assert not g[..., 9:].view(torch.int16).any()   # the pad columns: exactly +0
    assert not w[..., 9:].any()
    assert model.unet.state_dict()["conv_in.weight"].shape[1] == 9


def test_removed_mask_equals_trivial_mask(dev):
    """mask == 1 and conditioning == blank: replacing every mask (probability 1) feeds the bits that replacing none
    (probability 0) feeds"""
    def run(p):
        tr = _trainer(_cfg(unmasked_probability=p), dev)
        batch = _batch(dev, trivial=True)
        out = torch.stack([tr.train_step(batch) for _ in range(2)]).cpu()
        return out, tr.model.unet.store.data.clone()

    (l0, p0), (l1, p1) = run(0.0), run(1.0)
    assert torch.equal(l0, l1), (l0, l1)
    assert torch.equal(p0, p1)


def test_validation_pass_removes_no_mask(dev):
    tr = _trainer(_cfg(unmasked_probability=1.0), dev)
    batch = _batch(dev)
    ins = tr.model_setup.step_inputs(tr.model, batch, tr.config, tr.model.train_progress, deterministic=True)
    assert len(ins) == 3 and not ins[2].any()
    ins = tr.model_setup.step_inputs(tr.model, batch, tr.config, tr.model.train_progress)
    assert ins[2].all()


def test_masked_training_weights_the_loss_by_the_fed_mask(dev):
    """with masked_training the loss mask is the mask the UNet saw: all ones for a sample whose mask was removed"""
    tr = _trainer(_cfg(masked_training=True, unmasked_probability=1.0), dev)
    batch = _batch(dev)
    out = tr.model_setup.predict(tr.model, batch, tr.config, tr.model.train_progress)
    assert torch.equal(out["_loss_mask"], torch.ones_like(batch["latent_mask"]))
    a = tr.model_setup.calculate_loss(tr.model, batch, out, tr.config)
    ones = dict(batch, latent_mask=torch.ones_like(batch["latent_mask"]))
    out.pop("_loss_mask")
    b = tr.model_setup.calculate_loss(tr.model, ones, out, tr.config)
    assert torch.equal(a.detach(), b.detach())


@pytest.mark.parametrize("dora", [False, True], ids=["lora", "dora"])
def test_adapter_on_conv_in_has_nine_reference_channels(dev, dora):
    tr = _trainer(_cfg(training_method="LORA", lora_rank=8, lora_alpha=8.0, lora_decompose=dora), dev)
    loss = tr.train_step(_batch(dev)).item()
    assert loss == loss and abs(loss) < 1e4
    site = next(s for s in tr.model.unet_lora.sites if s.key == "conv_in")
    assert (site.cin, site.cin_ref) == (16, 9)
    sd = tr.model.unet_lora.state_dict()
    assert sd["lora_unet.conv_in.lora_down.weight"].shape[1] == 9


def test_backup_and_resume(dev, tmp_path):
    batch = _batch(dev)
    kw = dict(workspace_dir=str(tmp_path), unmasked_probability=0.5)
    a = _trainer(_cfg(**kw), dev)
    for _ in range(2):
        a.train_step(batch)
    assert a.backup()
    want = a.train_step(batch).item()
    b = _trainer(_cfg(continue_last_backup=True, **kw), dev)
    assert b.model.train_progress.global_step == 2
    assert b.model.unet.cfg.in_channels == 9
    got = b.train_step(batch).item()
    torch.cuda.synchronize()
    assert got == want
    assert torch.equal(a.model.unet.store.data, b.model.unet.store.data)


def test_step_has_no_stream_races(dev):
    tr = _trainer(_cfg(), dev)
    batch = _batch(dev)
    tr.train_step(batch)
    torch.cuda.synchronize()
    with StreamHazardCheck() as chk:
        tr.train_step(batch)
    torch.cuda.synchronize()
    assert chk.regions > 10 and chk.kernel_calls > 100 and chk.checked > 100, chk.report()
    assert not chk.hazards, chk.report()


def test_step_graph_matches_eager(dev, monkeypatch):
    """the captured step reads the step's mask removals from a buffer written before every replay"""
    flags = [tuple(K.inpaint_unmask(2, gs, 0.5, device=dev).tolist()) for gs in range(3)]
    assert len(set(flags)) > 1, flags   # the removals differ between the steps

    def run(graphs):
        monkeypatch.setenv("OTAMD_STEP_GRAPH", "1" if graphs else "0")
        tr = _trainer(_cfg(unmasked_probability=0.5), dev)
        assert (tr.graphs is not None) == graphs
        batch = _batch(dev)
        losses = torch.stack([tr.train_step(batch).clone() for _ in range(3)]).cpu()
        torch.cuda.synchronize()
        return losses, tr.model.unet.store.data.clone(), tr

    l0, p0, _ = run(False)
    l1, p1, tr1 = run(True)
    assert len(tr1.graphs.entries) == 1
    assert torch.equal(l0, l1), (l0, l1)
    assert torch.equal(p0, p1)


def test_four_channel_path_is_unchanged(dev, monkeypatch):
    """a plain SDXL model keeps its 8-wide input and K.ddpm_prologue; the new prologue is never called"""
    calls = []
    ddpm, inpaint = K.ddpm_prologue, K.inpaint_prologue
    monkeypatch.setattr(K, "ddpm_prologue", lambda *a, **k: calls.append("ddpm") or ddpm(*a, **k))
    monkeypatch.setattr(K, "inpaint_prologue", lambda *a, **k: calls.append("inpaint") or inpaint(*a, **k))

    def run():
        cfg = _cfg(model_type="STABLE_DIFFUSION_XL_10_BASE")
        tr = _trainer(cfg, dev, in_channels=4)
        assert tr.model.unet.store.params["conv_in.weight"].shape[1:] == (3, 3, U.PAD_IN)
        batch = synthetic_sdxl_batch(2, 128, 128, dev, seed=1, te1_dim=48, te2_dim=48, pooled_dim=64)
        assert len(tr.model_setup.step_inputs(tr.model, batch, cfg, tr.model.train_progress)) == 2
        out = tr.model_setup.predict(tr.model, batch, cfg, tr.model.train_progress)
        noise, t = tr.model_setup.step_inputs(tr.model, batch, cfg, tr.model.train_progress)
        want = ddpm(tr.model_setup._nhwc_latent(batch["latent_image"]), noise, t, tr.model.noise_scheduler.coeffs,
                    0.13025, 0)
        assert torch.equal(out["_target_nhwc"], want[1]) and "_loss_mask" not in out
        losses = torch.stack([tr.train_step(batch) for _ in range(2)]).cpu()
        return losses, tr.model.unet.store.data.clone()

    (l0, p0), (l1, p1) = run(), run()
    assert calls and set(calls) == {"ddpm"}
    assert torch.equal(l0, l1) and torch.equal(p0, p1)
    with pytest.raises(ValueError, match="conv_in.weight"):
        create.create_model(_cfg(), dev, unet_config=_ucfg(in_channels=4))
    with pytest.raises(ValueError, match="conv_in.weight"):
        create.create_model(_cfg(model_type="STABLE_DIFFUSION_XL_10_BASE"), dev, unet_config=_ucfg(in_channels=9))
