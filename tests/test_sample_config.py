"""CPU checks of the sampling configuration, its timers and commands, and the VAE decoder's parameter layout."""
import json
from types import SimpleNamespace

import pytest
import torch

from onetrainer_amd.module import vae as V
from onetrainer_amd.trainer.GenericTrainer import GenericTrainer
from onetrainer_amd.util.config.SampleConfig import SampleConfig, read_sample_configs, safe_filename
from onetrainer_amd.util.config.TrainConfig import TrainConfig
from onetrainer_amd.util.TrainCommands import TrainCommands
from onetrainer_amd.util.TrainProgress import TrainProgress

# one entry of a reference training_samples/samples.json (SampleConfig.to_dict: enums as their value strings)
REF_SAMPLE = {"__version": 0, "enabled": True, "prompt": "a photo of a cat", "negative_prompt": "blurry",
              "height": 1024, "width": 768, "frames": 1, "length": 10.0, "seed": 7, "random_seed": False,
              "diffusion_steps": 30, "cfg_scale": 5.5, "noise_scheduler": "DDIM", "text_encoder_1_layer_skip": 0,
              "text_encoder_2_layer_skip": 0, "text_encoder_3_layer_skip": 0, "text_encoder_4_layer_skip": 0,
              "prior_attention_mask": False, "force_last_timestep": False, "sample_inpainting": False,
              "base_image_path": "", "mask_image_path": ""}


def test_defaults_match_the_reference():
    s = SampleConfig.default_values()
    assert (s.enabled, s.prompt, s.negative_prompt, s.height, s.width, s.frames, s.seed, s.random_seed,
            s.diffusion_steps, s.cfg_scale, s.noise_scheduler, s.force_last_timestep, s.sample_inpainting) == (
        True, "", "", 512, 512, 1, 42, False, 20, 7.0, "DDIM", False, False)
    c = TrainConfig.default_values()
    assert (c.samples, c.sample_definition_file_name, c.sample_after, c.sample_after_unit, c.sample_skip_first,
            c.sample_image_format, c.samples_to_tensorboard, c.non_ema_sampling, c.text_encoder_layer_skip,
            c.text_encoder_2_layer_skip) == (None, "training_samples/samples.json", 10, "MINUTE", 0, "JPG", True,
                                             True, 0, 0)


def test_reference_json_loads(tmp_path):
    s = SampleConfig().from_dict(REF_SAMPLE)
    assert (s.prompt, s.height, s.width, s.seed, s.diffusion_steps, s.cfg_scale) == ("a photo of a cat", 1024, 768,
                                                                                     7, 30, 5.5)
    assert s.extra["text_encoder_3_layer_skip"] == 0 and s.to_dict()["prompt"] == "a photo of a cat"
    cfg = TrainConfig().from_dict({"samples": None, "sample_after": 3, "sample_after_unit": "STEP",
                                   "sample_image_format": "PNG", "text_encoder_2_layer_skip": 1,
                                   "rescale_noise_scheduler_to_zero_terminal_snr": True})
    assert "sample_after" not in cfg.extra and cfg.sample_after == 3 and cfg.sample_image_format == "PNG"
    s.from_train_config(cfg)
    assert s.text_encoder_2_layer_skip == 1 and s.force_last_timestep is True


def test_inline_samples_beat_the_file_and_a_missing_file_gives_none(tmp_path):
    path = tmp_path / "samples.json"
    path.write_text(json.dumps([REF_SAMPLE, dict(REF_SAMPLE, prompt="a dog")]))
    cfg = TrainConfig.default_values()
    cfg.sample_definition_file_name = str(path)
    assert [s.prompt for s in read_sample_configs(cfg)] == ["a photo of a cat", "a dog"]
    cfg.samples = [dict(REF_SAMPLE, prompt="inline")]
    assert [s.prompt for s in read_sample_configs(cfg)] == ["inline"]
    cfg.samples = None
    cfg.sample_definition_file_name = str(tmp_path / "missing.json")
    assert read_sample_configs(cfg) == []
    assert read_sample_configs(TrainConfig.default_values()) == []   # the default path does not exist here


@pytest.mark.parametrize("change,word", [({"noise_scheduler": "EULER_A"}, "EULER_A"),
                                         ({"noise_scheduler": "DPMPP"}, "DPMPP"),
                                         ({"sample_inpainting": True}, "sample_inpainting"),
                                         ({"frames": 9}, "frames")])
def test_unsupported_samples_are_refused_by_name(change, word):
    cfg = TrainConfig.default_values()
    cfg.samples = [dict(REF_SAMPLE, **change)]
    with pytest.raises(NotImplementedError, match=word):
        read_sample_configs(cfg)
    cfg.samples = [dict(REF_SAMPLE, enabled=False, **change)]   # a disabled entry is never sampled
    assert len(read_sample_configs(cfg)) == 1


def test_refusal_happens_when_the_trainer_starts_reading(monkeypatch):
    cfg = TrainConfig.default_values()
    cfg.samples = [dict(REF_SAMPLE, noise_scheduler="UNIPC")]
    tr = GenericTrainer(cfg, model=SimpleNamespace(train_progress=TrainProgress()))
    with pytest.raises(NotImplementedError, match="UNIPC"):
        tr._setup_sampling()


def test_flux_keeps_no_samples(capsys):
    cfg = TrainConfig.default_values()
    cfg.model_type = "FLUX_DEV_1"
    cfg.samples = [dict(REF_SAMPLE)]
    tr = GenericTrainer(cfg, model=SimpleNamespace(train_progress=TrainProgress()))
    tr._setup_sampling()
    assert tr.model_sampler is None and tr.sample_configs == []
    assert capsys.readouterr().out.count("\n") == 1
    assert tr.sample(TrainProgress()) == []


def _timer_trainer(**kw):
    cfg = TrainConfig.default_values()
    for k, v in kw.items():
        setattr(cfg, k, v)
    tr = GenericTrainer(cfg, model=SimpleNamespace(train_progress=TrainProgress()))
    tr.sample_configs = [SampleConfig()]
    return tr


def test_sample_timer_units_and_skip_first():
    tr = _timer_trainer(sample_after=2, sample_after_unit="STEP", sample_skip_first=3)
    hits = [g for g in range(10) if tr._needs_sample(TrainProgress(global_step=g))]
    assert hits == [4, 6, 8]          # every 2 steps (start_at_zero), once global_step + 1 > 3
    tr = _timer_trainer(sample_after=1, sample_after_unit="EPOCH")
    assert tr._needs_sample(TrainProgress(epoch=0, epoch_step=0))
    assert not tr._needs_sample(TrainProgress(epoch=0, epoch_step=1, global_step=1))
    assert tr._needs_sample(TrainProgress(epoch=1, epoch_step=0, global_step=5))
    assert not _timer_trainer(sample_after_unit="NEVER")._needs_sample(TrainProgress())
    assert _timer_trainer(sample_after_unit="ALWAYS")._needs_sample(TrainProgress(global_step=3))
    tr = _timer_trainer(sample_after=1, sample_after_unit="STEP")
    tr.sample_configs = [SampleConfig(enabled=False)]
    assert not tr._needs_sample(TrainProgress())      # nothing enabled: the timer never raises the command


def test_sample_commands_are_taken_once_and_run_at_the_boundary():
    cmds = TrainCommands()
    assert not cmds.has_sample_commands()
    cmds.sample_default()
    cmds.sample_custom({"prompt": "x"})
    assert cmds.has_sample_commands()
    tr = _timer_trainer()
    tr.commands = cmds
    calls = []
    tr.sample = lambda tp, params=None: calls.append(params)
    tr.backup = tr.save = lambda tp=None: calls.append("io")
    tr._run_commands(TrainProgress(), True)
    assert calls == [None, [{"prompt": "x"}]]
    tr._run_commands(TrainProgress(), True)
    assert len(calls) == 2 and not cmds.has_sample_commands()
    cmds.sample_default()
    tr._run_commands(TrainProgress(), False)          # not an agreement point: the sticky command waits
    assert len(calls) == 2 and cmds.has_sample_commands()


def test_safe_filename():
    assert safe_filename("a photo / of: a <cat>, 4k!") == "a photo  of a cat 4k"
    assert safe_filename("x" * 40) == "x" * 32


# ----- decoder parameter layout -------------------------------------------------------------------
def _by_name(cfg):
    return {n: (sh, k) for n, sh, k, _ in V.vae_decoder_specs(cfg)}


@pytest.mark.parametrize("cfgname", ["sd15", "sdxl"])
def test_decoder_specs_full_size(cfgname):
    cfg = {"sd15": V.sd15_vae_config, "sdxl": V.sdxl_vae_config}[cfgname]()
    s = _by_name(cfg)
    assert len(s) == 138 + 2    # diffusers AutoencoderKL: 138 decoder tensors + post_quant_conv weight / bias
    assert s["post_quant_conv.weight"][0] == (4, 4, 1, 1) and s["decoder.conv_in.weight"][0] == (512, 4, 3, 3)
    assert s["decoder.conv_out.weight"][0] == (3, 128, 3, 3) and s["decoder.conv_out.bias"][0] == (3,)
    assert s["decoder.mid_block.attentions.0.to_q.weight"][0] == (512, 512)
    # reversed channels (512, 512, 256, 128), three resnets each, an upsampler on all but the last
    assert s["decoder.up_blocks.0.resnets.2.conv2.weight"][0] == (512, 512, 3, 3)
    assert s["decoder.up_blocks.2.resnets.0.conv1.weight"][0] == (256, 512, 3, 3)
    assert s["decoder.up_blocks.2.resnets.0.conv_shortcut.weight"][0] == (256, 512, 1, 1)
    assert s["decoder.up_blocks.3.resnets.0.conv_shortcut.weight"][0] == (128, 256, 1, 1)
    assert "decoder.up_blocks.1.resnets.0.conv_shortcut.weight" not in s
    assert "decoder.up_blocks.2.upsamplers.0.conv.weight" in s and "decoder.up_blocks.3.upsamplers.0.conv.weight" not in s
    assert "decoder.up_blocks.0.resnets.3.conv1.weight" not in s
    assert s["decoder.conv_norm_out.weight"][0] == (128,)


@pytest.mark.parametrize("quant", [True, False])
def test_decoder_tiny_store_and_round_trip(quant):
    cfg = V.tiny_vae_config(use_quant_conv=quant)
    dec = V.AutoencoderKLDecoder(cfg, "cpu", seed=3)
    s = _by_name(cfg)
    assert ("post_quant_conv.weight" in s) == quant
    assert s["decoder.conv_in.weight"][0] == (160, 4, 3, 3) and s["decoder.up_blocks.1.resnets.1.conv1.weight"][0] == (
        64, 64, 3, 3)
    # store layout: [co, kh, kw, ci]; the latent side and conv_out's outputs zero-padded to 8
    P = dec.store.params
    assert tuple(P["decoder.conv_in.weight"].shape) == (160, 3, 3, 8)
    assert tuple(P["decoder.conv_out.weight"].shape) == (8, 3, 3, 64) and tuple(P["decoder.conv_out.bias"].shape) == (8,)
    assert torch.count_nonzero(P["decoder.conv_out.weight"][3:]) == 0 and torch.count_nonzero(P["decoder.conv_out.bias"][3:]) == 0
    assert torch.count_nonzero(P["decoder.conv_in.weight"][..., 4:]) == 0
    assert torch.count_nonzero(P["decoder.conv_out.weight"][:3]) > 0
    if quant:
        assert tuple(P["post_quant_conv.weight"].shape) == (8, 8)
        assert torch.count_nonzero(P["post_quant_conv.weight"][4:]) == 0
        assert torch.count_nonzero(P["post_quant_conv.weight"][:, 4:]) == 0
    sd = dec.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {n: tuple(sh) for n, (sh, _) in s.items()}
    other = V.AutoencoderKLDecoder(cfg, "cpu", seed=None)
    other.load_state_dict({k: v.float() for k, v in sd.items()})
    assert torch.equal(other.store.data, dec.store.data)
    with pytest.raises(ValueError, match="shape"):
        other.load_state_dict(dict(sd, **{"decoder.conv_out.bias": torch.zeros(8)}))
    assert V.decoder_flops_per_image(cfg, 64, 64) > 0


def test_decoder_ldm_names():
    from onetrainer_amd.modelLoader import ldm_convert as LC
    assert LC.vae_ldm_name("decoder.up_blocks.0.resnets.2.conv_shortcut.weight") == "decoder.up.3.block.2.nin_shortcut.weight"
    assert LC.vae_ldm_name("decoder.up_blocks.2.upsamplers.0.conv.bias") == "decoder.up.1.upsample.conv.bias"
    assert LC.vae_ldm_name("decoder.mid_block.attentions.0.to_out.0.weight") == "decoder.mid.attn_1.proj_out.weight"
    assert LC.vae_ldm_name("decoder.conv_norm_out.bias") == "decoder.norm_out.bias"
    assert LC.vae_ldm_name("post_quant_conv.weight") == "post_quant_conv.weight"
    cfg = V.sdxl_vae_config()
    specs = V.vae_decoder_specs(cfg)
    sd = {LC.VAE_PREFIX + LC.vae_ldm_name(n): torch.zeros(sh) for n, sh, *_ in specs}
    assert set(LC.vae_from_ldm(sd, specs)) == {n for n, *_ in specs}
