"""Training samples end to end on the GPU: tiny UNet + tiny VAE decoder, ready prompt states, sample_after = 1 STEP,
4 diffusion steps, 64 x 64 images."""
import glob
import os

import numpy as np
import pytest
import torch
from PIL import Image

from onetrainer_amd.dataLoader.SyntheticDataLoader import synthetic_sdxl_batch
from onetrainer_amd.module import unet as U
from onetrainer_amd.module import vae as V
from onetrainer_amd.trainer.GenericTrainer import GenericTrainer
from onetrainer_amd.util import create
from onetrainer_amd.util.config.TrainConfig import TrainConfig
from onetrainer_amd.util.TrainCommands import TrainCommands

pytestmark = pytest.mark.gpu

SAMPLE = {"prompt": "a cat", "negative_prompt": "", "height": 64, "width": 64, "seed": 11, "diffusion_steps": 4,
          "cfg_scale": 5.0}


class _Loader:
    def __init__(self, dev, steps, sdxl=True):
        self.batch = synthetic_sdxl_batch(2, 64, 64, dev, 0, te1_dim=32, te2_dim=64, pooled_dim=64, sdxl=sdxl) if sdxl \
            else synthetic_sdxl_batch(2, 64, 64, dev, 0, te1_dim=96, sdxl=False)
        self.steps = steps

    def get_data_set(self):
        return self

    def approximate_length(self):
        return self.steps

    def start_next_epoch(self):
        pass

    def get_data_loader(self):
        return iter([self.batch] * self.steps)


def _states(dev, sdxl=True):
    g = torch.Generator().manual_seed(3)
    def one():
        return (torch.randn(1, 77, 96, generator=g).bfloat16().to(dev),
                torch.randn(1, 64, generator=g).bfloat16().to(dev) if sdxl else None)
    return {"positive": one(), "negative": one()}


def _trainer(dev, tmp, samples=True, steps=2, method="FINE_TUNE", sd15=False, dora=False, commands=None, **kw):
    cfg = TrainConfig.default_values()
    cfg.batch_size, cfg.epochs = 2, 1
    cfg.learning_rate, cfg.learning_rate_warmup_steps = 1e-3, 0
    cfg.workspace_dir = str(tmp)
    cfg.backup_after_unit = "NEVER"
    cfg.training_method = method
    if method == "LORA":
        cfg.lora_rank, cfg.lora_alpha, cfg.lora_decompose = 8, 8.0, dora
        cfg.dropout_probability = 0.0 if dora else 0.25
    if sd15:
        cfg.model_type = "STABLE_DIFFUSION_15"
    cfg.sample_after, cfg.sample_after_unit, cfg.sample_image_format = 1, "STEP", "PNG"
    cfg.samples = [dict(SAMPLE)] if samples else None
    cfg.sample_definition_file_name = str(tmp / "none.json")
    for k, v in kw.items():
        setattr(cfg, k, v)
    model = create.create_model(cfg, dev, seed=4, unet_config=U.tiny_sd15_config() if sd15 else U.tiny_sdxl_config())
    model.vae_config = V.tiny_vae_config()
    tr = GenericTrainer(cfg, model=model, data_loader=_Loader(dev, steps, sdxl=not sd15), commands=commands)
    tr.sample_prompt_states = _states(dev, sdxl=not sd15)
    tr.start()
    return tr


def _pngs(tmp, sub="0 - a cat"):
    return sorted(glob.glob(os.path.join(str(tmp), "samples", sub, "*.png")))


def test_files_determinism_and_training_untouched(dev, tmp_path):
    runs = []
    for name, samples in (("a", True), ("b", True), ("off", False)):
        tr = _trainer(dev, tmp_path / name, samples=samples)
        losses = []
        step = tr.train_step
        tr.train_step = lambda b, _s=step, _l=losses: (_l.append(_s(b)), _l[-1])[1]
        tr.train(log_every=0)
        torch.cuda.synchronize()
        runs.append((torch.stack(losses).cpu(), tr.model.train_store.data.clone().cpu(), tr))
    files = _pngs(tmp_path / "a")
    assert len(files) == 2 and [os.path.basename(f).split("-training-sample-")[1] for f in files] == [
        "0-0-0.png", "1-0-1.png"]
    assert runs[0][2].sample_paths == files
    img = Image.open(files[0])
    assert img.size == (64, 64) and img.mode == "RGB"
    assert len(np.unique(np.asarray(img).reshape(-1, 3), axis=0)) > 16     # an image, not a constant
    other = _pngs(tmp_path / "b")
    assert [open(f, "rb").read() for f in files] == [open(f, "rb").read() for f in other]
    assert open(files[0], "rb").read() != open(files[1], "rb").read()     # the weights moved between the two
    assert not os.path.exists(tmp_path / "off" / "samples")
    assert getattr(runs[2][2].model, "vae_decoder", None) is None         # nothing attached without samples
    assert torch.equal(runs[0][0].view(torch.int32), runs[2][0].view(torch.int32))          # losses, bit for bit
    assert torch.equal(runs[0][1].view(torch.int16), runs[2][1].view(torch.int16))          # the final store


def test_ema_and_non_ema_images(dev, tmp_path):
    tr = _trainer(dev, tmp_path, steps=4, ema="GPU", ema_decay=0.5, ema_update_step_interval=1, sample_skip_first=3)
    tr.train(log_every=0)
    torch.cuda.synchronize()
    ema, raw = _pngs(tmp_path), _pngs(tmp_path, "0 - a cat - no-ema")
    assert len(ema) == 1 and len(raw) == 1 and os.path.basename(ema[0]).endswith("3-0-3.png")
    assert open(ema[0], "rb").read() != open(raw[0], "rb").read()
    tr2 = _trainer(dev, tmp_path / "only_ema", steps=4, ema="GPU", ema_decay=0.5, ema_update_step_interval=1,
                   sample_skip_first=3, non_ema_sampling=False)
    tr2.train(log_every=0)
    assert len(_pngs(tmp_path / "only_ema")) == 1 and not _pngs(tmp_path / "only_ema", "0 - a cat - no-ema")
    assert open(_pngs(tmp_path / "only_ema")[0], "rb").read() == open(ema[0], "rb").read()


@pytest.mark.parametrize("kind", ["sd15", "lora", "dora"])
def test_plugins_produce_an_image(dev, tmp_path, kind):
    kw = {"sd15": dict(sd15=True), "lora": dict(method="LORA"), "dora": dict(method="LORA", dora=True)}[kind]
    tr = _trainer(dev, tmp_path, steps=1, **kw)
    lora = tr.model.unet_lora
    tr.train(log_every=0)
    files = _pngs(tmp_path)
    assert len(files) == 1 and Image.open(files[0]).size == (64, 64)
    if kind == "lora":
        assert lora.dropout_p == 0.25          # switched off for the sample, back on after it


def test_sample_custom_command_is_served(dev, tmp_path, capsys):
    cmds = TrainCommands()
    tr = _trainer(dev, tmp_path, samples=False, steps=2, commands=cmds)
    assert getattr(tr.model, "vae_decoder", None) is None
    cmds.sample_custom(dict(SAMPLE, prompt="on demand", seed=5))
    tr.train(log_every=0)
    files = _pngs(tmp_path, "custom")
    assert len(files) == 1 and Image.open(files[0]).size == (64, 64)
    assert tr.model.vae_decoder is not None and not cmds.has_sample_commands()
    # a custom sample this build cannot draw is named in a log line and skipped; the rest of the command runs
    got = tr.sample(sample_params=[dict(SAMPLE, noise_scheduler="EULER"), dict(SAMPLE, prompt="second", seed=6)])
    assert len(got) == 1 and "EULER" in capsys.readouterr().out


def test_no_stream_hazards_around_a_sample(dev, tmp_path):
    from onetrainer_amd.module.stream_hazards import StreamHazardCheck
    tr = _trainer(dev, tmp_path, steps=1)
    batch = tr.data_loader.batch
    tr.train_step(batch)
    with StreamHazardCheck() as chk:
        tr.train_step(batch)
        written = tr.sample()
        tr.train_step(batch)
    assert len(written) == 1
    assert not chk.hazards, chk.report()
