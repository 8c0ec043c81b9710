"""CPU checks of sampling beside the rest of the trainer: the sample flag under data parallel, a fine-tune run with
samples configured continuing from its own backup, custom samples this build cannot draw, the image log."""
import json
import os
from types import SimpleNamespace

import torch
from safetensors.torch import save_file

from onetrainer_amd.model.StableDiffusionXLModel import NoiseScheduler, StableDiffusionXLModel
from onetrainer_amd.modelLoader.StableDiffusionModelLoader import StableDiffusionXLModelLoader
from onetrainer_amd.modelSaver import StableDiffusionXLModelSaver, save_sub_module
from onetrainer_amd.module import text_encoder as TE
from onetrainer_amd.module import unet as U
from onetrainer_amd.module import vae as V
from onetrainer_amd.trainer.GenericTrainer import GenericTrainer
from onetrainer_amd.util.config.SampleConfig import SampleConfig
from onetrainer_amd.util.config.TrainConfig import TrainConfig
from onetrainer_amd.util.ModelNames import ModelNames
from onetrainer_amd.util.tensorboard import ScalarLog
from onetrainer_amd.util.TrainCommands import TrainCommands
from onetrainer_amd.util.TrainProgress import TrainProgress

CPU = torch.device("cpu")


# ----- data parallel: which sample flags wait for an agreement point ------------------------------------
def _dp_trainer():
    tr = GenericTrainer(TrainConfig.default_values(), model=SimpleNamespace(train_progress=TrainProgress()))
    tr.world, tr._wallclock_timers = 2, True        # e.g. backup_after_unit MINUTE beside sample_after_unit STEP
    tr.sample_configs = [SampleConfig()]
    calls = []
    tr.sample = lambda tp, params=None: calls.append(("sample", params))
    tr.backup = lambda tp=None: calls.append(("backup", None))
    tr.save = lambda tp=None: calls.append(("save", None))
    tr._agree = lambda flags, step: calls.append(("agree", flags)) or flags
    return tr, calls


def test_step_timer_sample_runs_at_its_exact_step_under_dp():
    tr, calls = _dp_trainer()
    tr._raise_timed(4, "STEP")
    assert tr._det_flags == 4 and not tr.commands.has_sample_commands()   # deterministic: every rank raises it
    tr._run_commands(TrainProgress(global_step=3), False)                 # not an agreement point
    assert calls == [("sample", None)] and tr._det_flags == 0
    tr._det_flags = 4 | 1
    tr._run_commands(TrainProgress(global_step=4), False)
    assert calls[1:] == [("sample", None), ("backup", None)]              # samples first, then the backup


def test_sticky_sample_commands_wait_for_the_agreement_point_under_dp():
    tr, calls = _dp_trainer()
    tr._raise_timed(4, "MINUTE")                   # a wall-clock timer: rank 0's decision, a sticky command
    tr.commands.sample_custom({"prompt": "x"})
    assert tr._det_flags == 0 and tr.commands.has_sample_commands()
    tr._run_commands(TrainProgress(global_step=3), False)
    assert calls == [] and tr.commands.has_sample_commands()
    tr._run_commands(TrainProgress(global_step=16), True)
    assert calls == [("agree", 4 | 8), ("sample", None), ("sample", [{"prompt": "x"}])]
    assert not tr.commands.has_sample_commands()


def test_step_timer_samples_all_run_in_the_loop_under_dp(tmp_path, monkeypatch):
    """the loop itself: world 2, a wall-clock backup timer, sample_after 2 STEP -> a sample at every second step, not
    only where an agreement point falls"""
    monkeypatch.chdir(tmp_path)
    cfg = TrainConfig.default_values()
    cfg.epochs, cfg.sample_after, cfg.sample_after_unit = 1, 2, "STEP"
    tp = TrainProgress()
    loader = SimpleNamespace(get_data_set=lambda: SimpleNamespace(start_next_epoch=lambda: None),
                             get_data_loader=lambda: iter(range(12)))
    tr = GenericTrainer(cfg, model=SimpleNamespace(train_progress=tp), data_loader=loader)
    tr.world, tr.rank = 2, 1                        # a rank that writes no scalars and takes part in no collective here
    tr.sample_configs = [SampleConfig()]
    seen = []
    tr.sample = lambda t, params=None: seen.append(t.global_step)
    tr._agree = lambda flags, step: flags
    tr._report_losses = lambda n, echo=True: None
    tr.abort_distributed = lambda: None

    def step(batch):
        tr._has_gradient = False
        tp.next_step(1)
        return torch.zeros(())

    tr.train_step = step
    tr.train(log_every=0)
    assert tr._wallclock_timers                      # backup_after_unit MINUTE (the default)
    assert seen == [0, 2, 4, 6, 8, 10]


# ----- continuing a fine-tune backup with samples configured -----------------------------------------------
def _tiny_model(seed):
    return StableDiffusionXLModel(U.UNet2DConditionModel(U.tiny_sdxl_config(), CPU, seed=seed), NoiseScheduler(CPU))


def _base_checkpoint(root, seed=5):
    """a diffusers-layout base model: unet/, vae/ (encoder + decoder keys), text_encoder/, tokenizer/"""
    m = _tiny_model(seed)
    StableDiffusionXLModelSaver().save(m, None, "DIFFUSERS", str(root))
    dec = V.AutoencoderKLDecoder(V.tiny_vae_config(), CPU, seed=seed + 1)
    enc = V.AutoencoderKLEncoder(V.tiny_vae_config(), CPU, seed=seed + 2)
    save_sub_module({k: v.contiguous() for k, v in {**enc.state_dict(), **dec.state_dict()}.items()},
                    str(root / "vae"), {"_class_name": "AutoencoderKL"})
    te = TE.CLIPTextEncoder(TE.tiny_clip_config(), CPU, seed=seed + 3)
    os.makedirs(root / "text_encoder")
    save_file({k: v.contiguous() for k, v in te.state_dict().items()}, str(root / "text_encoder" / "model.safetensors"))
    os.makedirs(root / "tokenizer")
    return m, dec, te


def _backup(workspace, seed=9, step=7):
    """what GenericTrainer.backup leaves for a fine-tune: unet/ + meta.json, no decoder, no text encoders"""
    m = _tiny_model(seed)
    path = workspace / "backup" / "2024-01-01_00-00-00-backup-7-0-7"
    StableDiffusionXLModelSaver().save(m, None, "DIFFUSERS", str(path))
    with open(path / "meta.json", "w") as f:
        json.dump({"train_progress": {"epoch": 0, "epoch_step": step, "epoch_sample": step, "global_step": step}}, f)
    return m


def _same(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)


def _resume_trainer(tmp_path, rank=0):
    base, dec, te = _base_checkpoint(tmp_path / "base")
    trained = _backup(tmp_path / "ws")
    cfg = TrainConfig.default_values()
    cfg.base_model_name, cfg.workspace_dir, cfg.continue_last_backup = str(tmp_path / "base"), str(tmp_path / "ws"), True
    cfg.samples = [{"prompt": "a cat", "height": 64, "width": 64}]
    model = _tiny_model(1)
    model.vae_config = V.tiny_vae_config()
    model.text_encoder_1 = TE.CLIPTextEncoder(TE.tiny_clip_config(), CPU, seed=0)   # tiny stand-in for CLIP-L
    tr = GenericTrainer(cfg, model=model)
    tr.device, tr.rank = CPU, rank
    tr._setup_sampling()
    return tr, model, trained, dec, te


def test_fine_tune_with_samples_continues_from_its_backup(tmp_path, capsys):
    tr, model, trained, dec, te = _resume_trainer(tmp_path)
    assert model.vae_decoder is not None and model.keep_text_encoders
    tr._load_weights()
    assert "Continuing training from backup" in capsys.readouterr().out
    assert _same(model.unet, trained.unet)                       # the UNet: from the backup
    assert model.train_progress.global_step == 7
    assert _same(model.vae_decoder, dec)                         # the frozen sampling modules: from the base model
    assert _same(model.text_encoder_1, te)


def test_loader_without_a_sampling_source_is_unchanged(tmp_path):
    """no samples: nothing attached, the backup loads as before and nothing is read from the base model"""
    _base_checkpoint(tmp_path / "base")
    trained = _backup(tmp_path / "ws")
    model = _tiny_model(1)
    path = str(next((tmp_path / "ws" / "backup").iterdir()))
    StableDiffusionXLModelLoader().load(model, ModelNames(base_model=path))
    assert _same(model.unet, trained.unet) and getattr(model, "vae_decoder", None) is None


def test_only_rank_zero_holds_the_sampling_modules(tmp_path):
    tr, model, *_ = _resume_trainer(tmp_path, rank=1)
    assert getattr(model, "vae_decoder", None) is None and not getattr(model, "keep_text_encoders", False)
    assert tr.sample_configs and tr.sample(TrainProgress()) == []


def test_single_file_checkpoint_is_read_once_for_the_decoder(tmp_path, monkeypatch):
    from onetrainer_amd.modelLoader import StableDiffusionModelLoader as L
    from onetrainer_amd.modelLoader import ldm_convert as LC
    src = _tiny_model(3)
    dec = V.AutoencoderKLDecoder(V.tiny_vae_config(), CPU, seed=4)
    f = str(tmp_path / "model.safetensors")
    StableDiffusionXLModelSaver().save(src, None, "SAFETENSORS", f)
    from safetensors.torch import load_file
    sd = load_file(f)
    sd |= {LC.VAE_PREFIX + LC.vae_ldm_name(k, 2): v.contiguous() for k, v in dec.state_dict().items()}
    save_file(sd, f)
    reads = []
    real = L.read_single_file
    monkeypatch.setattr(L, "read_single_file", lambda p: reads.append(p) or real(p))
    dst = _tiny_model(6)
    dst.vae_decoder = V.AutoencoderKLDecoder(V.tiny_vae_config(), CPU, seed=None)
    dst.sampling_source = ModelNames(base_model=f)
    L.StableDiffusionXLModelLoader().load(dst, ModelNames(base_model=f))
    assert _same(dst.unet, src.unet) and _same(dst.vae_decoder, dec) and reads == [f]


# ----- a custom sample that cannot be drawn, the image log ----------------------------------------------------
def test_unsupported_custom_sample_is_logged_and_skipped(capsys):
    tr = GenericTrainer(TrainConfig.default_values(), model=SimpleNamespace(train_progress=TrainProgress()))
    tr.model_sampler = object()
    tr.commands = TrainCommands()
    tr.commands.sample_custom({"prompt": "x", "noise_scheduler": "EULER_A"})
    tr._run_commands(TrainProgress(), True)          # does not raise out of the train loop
    assert "EULER_A" in capsys.readouterr().out and tr.sample_paths == []


def test_image_log_leaves_no_files_without_tensorboard(tmp_path, monkeypatch):
    import builtins
    real = builtins.__import__

    def no_tb(name, *a, **k):
        if name.startswith("torch.utils.tensorboard") or name == "tensorboard":
            raise ImportError(name)
        return real(name, *a, **k)

    monkeypatch.setattr(builtins, "__import__", no_tb)
    monkeypatch.delitem(__import__("sys").modules, "torch.utils.tensorboard", raising=False)
    log = ScalarLog(str(tmp_path / "tb"))
    log.add_image("sample0 - x", torch.zeros(4, 4, 3, dtype=torch.uint8).numpy(), 1)
    log.close()
    assert not os.path.exists(tmp_path / "tb")
