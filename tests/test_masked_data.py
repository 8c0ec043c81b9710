"""Masked training off the GPU (CPU): sample enumeration with <stem>-masklabel.png, the mask's way through the
latent cache (same scale / crop as its image, 0.125x downscale), the loader's latent_mask contract, the loss plan
of the reference's masked preset, and the argument checks of the loss family's C ABI (they return before any
launch).  mgds is not in the image: the mask downscale filter is PARITY UNPINNED."""
import ctypes
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from onetrainer_amd.dataLoader.aspect_bucketing import AspectBucketing
from onetrainer_amd.dataLoader.create import enumerate_samples
from onetrainer_amd.dataLoader.latent_cache import LatentCacheDataLoader, LatentCacheWriter
from onetrainer_amd.modelSetup.BaseStableDiffusionXLSetup import loss_plan
from onetrainer_amd.util.config.plain import plain
from onetrainer_amd.util.config.TrainConfig import TrainConfig

# training_presets/#sd 1.5 masked.json of the reference (settings only)
SD15_MASKED_PRESET = {"base_model_name": "stable-diffusion-v1-5/stable-diffusion-v1-5", "batch_size": 4,
                      "masked_training": True, "max_noising_strength": 0.8, "model_type": "STABLE_DIFFUSION_15",
                      "normalize_masked_area_loss": True, "output_model_destination": "models/model.safetensors",
                      "output_model_format": "SAFETENSORS", "resolution": "512", "training_method": "FINE_TUNE",
                      "vae": {"weight_dtype": "FLOAT_32"}}


def _png(path, size=(16, 16), value=128, mode="RGB"):
    from PIL import Image
    Image.new(mode, size, value if mode == "L" else (value,) * 3).save(path)


def _concept_dir(tmp_path):
    _png(tmp_path / "a.png")
    _png(tmp_path / "a-masklabel.png", value=255, mode="L")
    _png(tmp_path / "b.png")
    (tmp_path / "a.txt").write_text("a photo\n")
    return {"path": str(tmp_path), "enabled": True}


def test_enumerate_pairs_images_with_masklabels(tmp_path):
    concept = _concept_dir(tmp_path)
    cfg = SimpleNamespace(concepts=[concept], concept_file_name="", masked_training=True)
    got = enumerate_samples(cfg)
    assert got == [(str(tmp_path / "a.png"), "a photo", str(tmp_path / "a-masklabel.png")),
                   (str(tmp_path / "b.png"), "", None)]            # no file: the all-ones mask
    cfg.masked_training = False
    assert enumerate_samples(cfg) == [(str(tmp_path / "a.png"), "a photo"), (str(tmp_path / "b.png"), "")]


@pytest.mark.parametrize("knob", ["enable_random_circular_mask_shrink", "enable_random_mask_rotate_crop"])
def test_mask_augmentations_are_refused(tmp_path, knob):
    concept = dict(_concept_dir(tmp_path), image={knob: True})
    with pytest.raises(NotImplementedError, match=knob):
        enumerate_samples(SimpleNamespace(concepts=[concept], concept_file_name="", masked_training=True))
    assert len(enumerate_samples(SimpleNamespace(concepts=[concept], concept_file_name="", masked_training=False))) == 2


def _first_channel_latent(imgs):
    # [B,3,H,W] -> [B,H/8,W/8,1]: the 0.125x antialiased bilinear resize of the first channel (stands in for the VAE)
    x = F.interpolate(imgs[:, :1], size=(imgs.shape[2] // 8, imgs.shape[3] // 8), mode="bilinear", antialias=True,
                      align_corners=False)
    return x.clamp(0.0, 1.0).permute(0, 2, 3, 1)


def _masked_samples(shapes, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for h, w in shapes:
        mask = torch.rand(1, h, w, generator=g)
        mask[:, : h // 3] = 0.0
        mask[:, :, w - w // 4:] = 1.0
        img = torch.cat([mask, torch.rand(2, h, w, generator=g)])
        out.append({"image": img, "mask": mask})
    return out


def test_mask_takes_the_scale_and_crop_of_its_image(tmp_path):
    from safetensors.torch import load_file
    ab = AspectBucketing(128, 64)
    shapes = [(100, 230), (230, 100), (128, 128), (150, 161)]       # non-square: the bucket crops
    assert any(ab.bucket_for(h, w)[0] != ab.bucket_for(h, w)[1] for h, w in shapes)
    LatentCacheWriter(_first_channel_latent, str(tmp_path), ab, "cpu", encode_batch=2).write(_masked_samples(shapes))
    for i, (h, w) in enumerate(shapes):
        rec = load_file(str(tmp_path / f"{i:08d}.safetensors"))
        ch, cw = rec["crop_resolution"].tolist()
        lm = rec["latent_mask"]
        assert lm.shape == (1, ch // 8, cw // 8) and lm.dtype == torch.float32
        assert 0.0 <= lm.min() and lm.max() <= 1.0 and lm.min() < 0.05 and lm.max() > 0.95
        torch.testing.assert_close(rec["latent_image"][..., 0], lm[0], rtol=0, atol=0)


def test_mask_input_forms_agree(tmp_path):
    """PIL 'L' image, HW uint8 and [1, H, W] float masks of the same content cache the same latent mask"""
    from PIL import Image
    from safetensors.torch import load_file
    u8 = (torch.rand(96, 128, generator=torch.Generator().manual_seed(3)) * 255).to(torch.uint8)
    img = torch.rand(3, 96, 128)
    samples = [{"image": img, "mask": Image.fromarray(u8.numpy(), mode="L")}, {"image": img, "mask": u8},
               {"image": img, "mask": (u8.float() / 255.0)[None]}, {"image": img}]
    LatentCacheWriter(_first_channel_latent, str(tmp_path), AspectBucketing(128, 64), "cpu").write(samples)
    recs = [load_file(str(tmp_path / f"{i:08d}.safetensors")) for i in range(4)]
    assert torch.equal(recs[0]["latent_mask"], recs[1]["latent_mask"])
    assert torch.equal(recs[0]["latent_mask"], recs[2]["latent_mask"])
    assert "latent_mask" not in recs[3]
    with pytest.raises(ValueError, match="one channel"):
        LatentCacheWriter(_first_channel_latent, str(tmp_path / "x"), AspectBucketing(128, 64), "cpu").write(
            [{"image": img, "mask": torch.rand(3, 96, 128)}])


def test_loader_emits_latent_mask_only_when_required(tmp_path):
    ab = AspectBucketing(128, 64)
    shapes = [(128, 128)] * 4
    LatentCacheWriter(_first_channel_latent, str(tmp_path), ab, "cpu", encode_batch=2).write(_masked_samples(shapes))
    plain_batches = list(LatentCacheDataLoader(str(tmp_path), 2, "cpu", prefetch=False).get_data_loader())
    assert len(plain_batches) == 2 and all("latent_mask" not in b for b in plain_batches)
    for prefetch in (False, True):
        dl = LatentCacheDataLoader(str(tmp_path), 2, "cpu", prefetch=prefetch, require_mask=True)
        batches = list(dl.get_data_loader())
        assert len(batches) == 2
        for b, p in zip(batches, plain_batches):
            assert set(b) == set(p) | {"latent_mask"}
            m = b["latent_mask"]
            assert m.shape == (2, 1, 16, 16) and m.dtype == torch.float32 and m.is_contiguous()
            assert torch.equal(m[:, 0], b["latent_image"][:, 0])      # each mask rides with its own latent
    # two ranks of a global batch of 4: the mask is sliced with the rest of the batch
    whole = list(LatentCacheDataLoader(str(tmp_path), 4, "cpu", prefetch=False, require_mask=True).get_data_loader())
    r0 = list(LatentCacheDataLoader(str(tmp_path), 2, "cpu", rank=0, world=2, prefetch=False,
                                    require_mask=True).get_data_loader())
    r1 = list(LatentCacheDataLoader(str(tmp_path), 2, "cpu", rank=1, world=2, prefetch=False,
                                    require_mask=True).get_data_loader())
    assert len(whole) == len(r0) == len(r1) == 1
    assert torch.equal(torch.cat([r0[0]["latent_mask"], r1[0]["latent_mask"]]), whole[0]["latent_mask"])
    assert torch.equal(torch.cat([r0[0]["latent_image"], r1[0]["latent_image"]]), whole[0]["latent_image"])
    assert torch.equal(r1[0]["latent_mask"][:, 0], r1[0]["latent_image"][:, 0])


@pytest.mark.parametrize("prefetch", [False, True])
def test_loader_refuses_a_cache_without_masks(tmp_path, prefetch):
    samples = [{"image": torch.rand(3, 128, 128)} for _ in range(2)]
    LatentCacheWriter(_first_channel_latent, str(tmp_path), AspectBucketing(128, 64), "cpu").write(samples)
    dl = LatentCacheDataLoader(str(tmp_path), 2, "cpu", prefetch=prefetch, require_mask=True)
    with pytest.raises(ValueError, match="cache was built without masks; delete cache_dir"):
        list(dl.get_data_loader())


def test_loss_plan_of_the_masked_preset():
    cfg = TrainConfig.reference_defaults().from_dict(SD15_MASKED_PRESET)
    assert (cfg.unmasked_probability, cfg.unmasked_weight, cfg.masked_prior_preservation_weight) == (0.1, 0.1, 0.0)
    assert not cfg.extra.keys() & {"normalize_masked_area_loss", "unmasked_weight", "masked_training"}
    plan = loss_plan(plain(cfg))
    assert plan["masked"] is True and plan["normalize"] is True and plan["unmasked_weight"] == 0.1
    assert (plan["mse_strength"], plan["mae_strength"], plan["log_cosh_strength"]) == (1.0, 0.0, 0.0)
    cfg.mae_strength, cfg.log_cosh_strength, cfg.unmasked_weight = 0.3, 0.2, 0.25
    plan = loss_plan(plain(cfg), flow=True)
    assert (plan["mae_strength"], plan["log_cosh_strength"], plan["unmasked_weight"]) == (0.3, 0.2, 0.25)
    cfg.masked_prior_preservation_weight = 0.5
    with pytest.raises(NotImplementedError, match="masked_prior_preservation_weight"):
        loss_plan(plain(cfg))
    cfg.masked_training = False          # the field is read under masked training only
    assert loss_plan(plain(cfg))["masked"] is False


def test_loss_plan_of_an_unmasked_config_keeps_its_values():
    cfg = TrainConfig.default_values()
    cfg.loss_scaler, cfg.batch_size, cfg.gradient_accumulation_steps, cfg.loss_weight_fn = "BOTH", 4, 3, "P2"
    plan = loss_plan(plain(cfg))
    assert {k: plan[k] for k in ("batch_size_scale", "ga_scale", "loss_fn", "gamma", "mse_strength")} == \
        {"batch_size_scale": 4, "ga_scale": 3, "loss_fn": 3, "gamma": 5.0, "mse_strength": 1.0}
    assert (plan["masked"], plan["mae_strength"], plan["log_cosh_strength"], plan["unmasked_weight"],
            plan["normalize"]) == (False, 0.0, 0.0, 0.1, False)
    # a stand-in config without the mask fields (the reference's defaults apply)
    ns = SimpleNamespace(masked_training=True, mse_strength=1.0, mae_strength=0.0, log_cosh_strength=0.0,
                         loss_scaler="NONE", batch_size=1, gradient_accumulation_steps=1, loss_weight_fn="CONSTANT",
                         loss_weight_strength=5.0)
    plan = loss_plan(plain(ns))
    assert (plan["masked"], plan["unmasked_weight"], plan["normalize"]) == (True, 0.1, False)


def test_loss_family_rejects_bad_arguments():
    """OTAMD_EINVAL before any launch: null pointers, B > 1024, cpad < C, unmasked_weight outside [0, 1], all three
    strengths zero, a workspace too small"""
    from onetrainer_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)

    def fwd(pred=p, cpad=8, B=2, C=4, strengths=(1.0, 0.0, 0.0), uw=0.1, ws_floats=1 << 20, loss_fn=0, coef=p):
        return L.otamd_diffusion_loss(pred, cpad, p, 1, p, B, 64, C, *strengths, uw, 1, 1.0, None, None, None, None,
                                      loss_fn, 5.0, 0, 1000, 1.0, p, ws_floats, p, coef, None, None)

    def bwd(pred=p, cpad=8, B=2, C=4, uw=0.1, coef=p):
        return L.otamd_diffusion_loss_grad(pred, cpad, p, 1, p, B, 64, C, uw, coef, None, p, None)

    for rc in (fwd(pred=None), fwd(coef=None), fwd(B=1025), fwd(B=0), fwd(cpad=3), fwd(uw=-0.01), fwd(uw=1.5),
               fwd(uw=float("nan")), fwd(strengths=(0.0, 0.0, 0.0)), fwd(ws_floats=2 * 4 * 1 - 1), fwd(loss_fn=5),
               fwd(loss_fn=4), fwd(loss_fn=1),
               bwd(pred=None), bwd(coef=None), bwd(B=1025), bwd(cpad=3), bwd(uw=2.0)):
        assert rc == _lib.OTAMD_EINVAL
