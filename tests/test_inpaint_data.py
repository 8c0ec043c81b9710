"""The data side of the mask-input (inpainting) model types off the GPU (CPU): masks are enumerated whether
masked_training is on or off, the cache holds the conditioning latent per sample (and per variation) and one blank
latent per bucket shape, a cache without them is refused, what stays unbuilt is refused by name, and a 9-channel
conv_in goes through the loader and the saver.  A resize of the first channel stands in for the VAE, NumPy
(tests/_oracle_augment.py) for the augmentation kernel."""
import json
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F
from safetensors.torch import load_file

import _oracle_augment as OA
from onetrainer_amd.dataLoader.aspect_bucketing import AspectBucketing
from onetrainer_amd.dataLoader.create import concept_extras, create_data_loader, enumerate_samples
from onetrainer_amd.dataLoader.latent_cache import LatentCacheDataLoader, LatentCacheWriter
from onetrainer_amd.util.config.SampleConfig import read_sample_configs
from onetrainer_amd.util.config.TrainConfig import TrainConfig
from onetrainer_amd.util.model_type import has_mask_input, unet_in_channels

TYPES = ("STABLE_DIFFUSION_15_INPAINTING", "STABLE_DIFFUSION_XL_10_BASE_INPAINTING")


def _png(path, size=(16, 16), value=128, mode="RGB"):
    from PIL import Image
    Image.new(mode, size, value if mode == "L" else (value,) * 3).save(path)


def _latent(x):
    x = F.interpolate(x[:, :1], size=(x.shape[2] // 8, x.shape[3] // 8), mode="bilinear", antialias=True,
                      align_corners=False)
    return x.permute(0, 2, 3, 1)


def _first_channel_latent(imgs):
    """the stand-in encoder: [0, 1] images to the encoder's [-1, 1], then the resize of the first channel"""
    return _latent(imgs * 2 - 1)


def _cond(imgs, masks):
    """the conditioning image in the encoder's range, (2 x - 1) (1 - m), then the stand-in encoder"""
    return _latent((imgs * 2 - 1) * (1 - masks))


def _rows(shapes, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for h, w in shapes:
        mask = (torch.rand(1, h, w, generator=g) > 0.5).float()
        out.append({"image": torch.rand(3, h, w, generator=g), "mask": mask})
    return out


@pytest.mark.parametrize("model_type", TYPES)
def test_mask_input_types(model_type):
    assert has_mask_input(model_type) and unet_in_channels(model_type) == 9
    assert not has_mask_input(model_type[:-len("_INPAINTING")]) and unet_in_channels("STABLE_DIFFUSION_15") == 4


@pytest.mark.parametrize("model_type", TYPES)
def test_enumeration_loads_masks_without_masked_training(tmp_path, model_type):
    _png(tmp_path / "a.png")
    _png(tmp_path / "a-masklabel.png", value=255, mode="L")
    _png(tmp_path / "b.png")
    cfg = SimpleNamespace(concepts=[{"path": str(tmp_path)}], concept_file_name="", masked_training=False,
                          model_type=model_type)
    assert enumerate_samples(cfg) == [(str(tmp_path / "a.png"), "", str(tmp_path / "a-masklabel.png")),
                                      (str(tmp_path / "b.png"), "", None)]
    cfg.model_type = model_type[:-len("_INPAINTING")]
    assert enumerate_samples(cfg) == [(str(tmp_path / "a.png"), ""), (str(tmp_path / "b.png"), "")]


def test_cache_carries_conditioning_latent_and_one_blank_per_bucket(tmp_path):
    ab = AspectBucketing(128, 64)
    shapes = [(128, 128), (100, 230), (128, 128), (230, 100)]
    rows = _rows(shapes)
    rows[2].pop("mask")   # no mask: all ones, the conditioning image is the blank one
    LatentCacheWriter(_first_channel_latent, str(tmp_path), ab, "cpu", encode_batch=2, cond_fn=_cond).write(rows)
    index = json.loads((tmp_path / "index.json").read_text())
    buckets = {"x".join(map(str, s["crop_resolution"])) for s in index["samples"]}
    assert len(buckets) == 3 and set(index["blank"]) == buckets
    for key, fn in index["blank"].items():
        H, W = map(int, key.split("x"))
        blank = load_file(str(tmp_path / fn))["latent_blank"]
        assert blank.shape == (H // 8, W // 8, 1) and not blank.any()   # the encoder's 0 image
    for i, s in enumerate(index["samples"]):
        rec = load_file(str(tmp_path / s["file"]))
        assert rec["latent_conditioning_image"].shape == rec["latent_image"].shape
        assert rec["latent_mask"].shape == (1,) + tuple(rec["latent_image"].shape[:2])
    rec = load_file(str(tmp_path / "00000002.safetensors"))
    assert rec["latent_mask"].min() == 1.0 and not rec["latent_conditioning_image"].any()   # == the blank
    rec = load_file(str(tmp_path / "00000000.safetensors"))   # square, no crop: the stand-in, computed here
    want = _cond(rows[0]["image"][None], rows[0]["mask"][None])[0]
    torch.testing.assert_close(rec["latent_conditioning_image"], want, rtol=0, atol=1e-6)
    # without cond_fn nothing changes: no blank, no conditioning latent
    LatentCacheWriter(_first_channel_latent, str(tmp_path / "p"), ab, "cpu", encode_batch=2).write(_rows(shapes))
    assert "blank" not in json.loads((tmp_path / "p" / "index.json").read_text())
    assert "latent_conditioning_image" not in load_file(str(tmp_path / "p" / "00000000.safetensors"))


def test_loader_contract_and_refusal_of_a_cache_without_conditioning(tmp_path):
    ab = AspectBucketing(128, 64)
    LatentCacheWriter(_first_channel_latent, str(tmp_path / "c"), ab, "cpu", cond_fn=_cond).write(_rows([(128, 128)] * 4))
    for prefetch in (False, True):
        dl = LatentCacheDataLoader(str(tmp_path / "c"), 2, "cpu", prefetch=prefetch, require_mask=True,
                                   require_conditioning=True)
        batches = list(dl.get_data_loader())
        assert len(batches) == 2
        for b in batches:
            assert b["latent_conditioning_image"].shape == b["latent_image"].shape == (2, 1, 16, 16)
            assert b["latent_conditioning_image"].permute(0, 2, 3, 1).is_contiguous()
            assert b["latent_mask"].shape == (2, 1, 16, 16) and b["latent_blank"].shape == (16, 16, 1)
    plain = list(LatentCacheDataLoader(str(tmp_path / "c"), 2, "cpu", prefetch=False).get_data_loader())
    assert all("latent_conditioning_image" not in b and "latent_blank" not in b for b in plain)
    LatentCacheWriter(_first_channel_latent, str(tmp_path / "m"), ab, "cpu").write(_rows([(128, 128)] * 2))
    for prefetch in (False, True):
        dl = LatentCacheDataLoader(str(tmp_path / "m"), 2, "cpu", prefetch=prefetch, require_mask=True,
                                   require_conditioning=True)
        with pytest.raises(ValueError, match="cache was built without conditioning latents; delete cache_dir"):
            list(dl.get_data_loader())


def test_variations_carry_their_own_conditioning_latent_and_mask(tmp_path):
    """image_variations acts on the conditioning latent and the mask as on the image latent: every variation's
    conditioning image is made from that variation's crop of the image and of the mask"""
    rows = _rows([(150, 161), (128, 128)], seed=2)
    concept = {"path": "x", "image_variations": 3, "image": {"enable_crop_jitter": True, "enable_random_flip": True}}
    rows = [dict(r, **concept_extras(concept, i)) for i, r in enumerate(rows)]
    seen = []

    def cond(imgs, masks):
        seen.append((imgs.clone(), masks.clone()))
        return _cond(imgs, masks)

    LatentCacheWriter(_first_channel_latent, str(tmp_path), AspectBucketing(128, 64), "cpu", encode_batch=2,
                      augment_fn=OA.augment_fn, cond_fn=cond).write(rows)
    imgs, masks = torch.cat([s[0] for s in seen]), torch.cat([s[1] for s in seen])
    assert imgs.shape == (6, 3, 128, 128) and masks.shape == (6, 1, 128, 128)
    assert all(len(s[0]) <= 2 for s in seen)   # encode_batch holds for the conditioning images too
    index = json.loads((tmp_path / "index.json").read_text())
    assert list(index["blank"]) == ["128x128"]
    k = 0
    for i, s in enumerate(index["samples"]):
        assert len(s["variations"]) == 2
        for fn in [s["file"]] + s["variations"]:
            rec = load_file(str(tmp_path / fn))
            # the variation's own crop went into both latents: the stand-in encoder of what cond_fn was handed
            torch.testing.assert_close(rec["latent_image"], _first_channel_latent(imgs[k:k + 1])[0], rtol=0, atol=0)
            torch.testing.assert_close(rec["latent_conditioning_image"], _cond(imgs[k:k + 1], masks[k:k + 1])[0],
                                       rtol=0, atol=0)
            assert rec["latent_mask"].shape == (1, 16, 16)
            k += 1
    dl = LatentCacheDataLoader(str(tmp_path), 2, "cpu", prefetch=False, require_mask=True, require_conditioning=True)
    firsts = []
    for _epoch in range(3):
        dl.start_next_epoch()
        firsts.append(next(iter(dl.get_data_loader()))["latent_conditioning_image"].clone())
    assert not torch.equal(firsts[0], firsts[1]) and not torch.equal(firsts[1], firsts[2])


def test_custom_conditioning_image_is_refused(tmp_path):
    _png(tmp_path / "a.png")
    cfg = TrainConfig.default_values()
    assert cfg.custom_conditioning_image is False
    cfg = TrainConfig().from_dict({"model_type": TYPES[1], "custom_conditioning_image": True,
                                   "concepts": [{"path": str(tmp_path)}], "cache_dir": str(tmp_path / "cache")})
    with pytest.raises(NotImplementedError, match="custom_conditioning_image"):
        enumerate_samples(cfg)
    with pytest.raises(NotImplementedError, match="custom_conditioning_image"):
        create_data_loader(cfg, None, "cpu")


@pytest.mark.parametrize("model_type", TYPES)
def test_enabled_samples_are_refused_by_name(model_type):
    cfg = TrainConfig().from_dict({"model_type": model_type, "samples": [{"prompt": "a", "enabled": True}]})
    with pytest.raises(NotImplementedError, match=f"samples for model type {model_type}"):
        read_sample_configs(cfg)
    cfg.samples = [{"prompt": "a", "enabled": False}]
    assert len(read_sample_configs(cfg)) == 1
    cfg.samples = [{"prompt": "a", "sample_inpainting": True}]   # the older refusal keeps its message
    with pytest.raises(NotImplementedError, match="sample_inpainting: inpainting samples are not built"):
        read_sample_configs(cfg)
    cfg.model_type, cfg.samples = model_type[:-len("_INPAINTING")], [{"prompt": "a"}]
    assert len(read_sample_configs(cfg)) == 1


@pytest.mark.parametrize("sdxl", [True, False], ids=["sdxl", "sd15"])
def test_conv_in_round_trip_and_channel_mismatch(tmp_path, sdxl):
    from onetrainer_amd.modelLoader import ldm_convert as LC
    from onetrainer_amd.modelLoader.HFModelLoaderMixin import read_diffusers_sub_module
    from onetrainer_amd.modelLoader.StableDiffusionModelLoader import apply_unet_state_dict
    from onetrainer_amd.modelSaver import save_sub_module, unet_diffusers_config
    from onetrainer_amd.module import unet as U
    from onetrainer_amd.util import create

    def ucfg(c):
        u = U.tiny_sdxl_config() if sdxl else U.tiny_sd15_config()
        u.in_channels = c
        return u

    assert U.pad_in(4) == U.PAD_IN == 8 and U.pad_in(9) == 16
    a = U.UNet2DConditionModel(ucfg(9), "cpu", seed=1)
    c0 = a.cfg.block_out_channels[0]
    assert a.store.params["conv_in.weight"].shape == (c0, 3, 3, 16)
    assert not a.store.params["conv_in.weight"][..., 9:].any() and a.store.params["conv_in.weight"][..., 8].any()
    sd = a.state_dict()
    assert sd["conv_in.weight"].shape == (c0, 9, 3, 3)
    # diffusers directory: saver -> loader, bit for bit, pad columns zero
    save_sub_module({k: v.cpu() for k, v in sd.items()}, str(tmp_path / "unet"), unet_diffusers_config(a.cfg))
    assert json.loads((tmp_path / "unet" / "config.json").read_text())["in_channels"] == 9
    assert U.unet_config_from_diffusers(json.loads((tmp_path / "unet" / "config.json").read_text())).in_channels == 9
    b = U.UNet2DConditionModel(ucfg(9), "cpu", seed=2)
    apply_unet_state_dict(b, read_diffusers_sub_module(str(tmp_path), "unet"))
    assert torch.equal(a.store.data, b.store.data)
    # a 4-channel checkpoint under a 9-channel UNet, and the other way round, names the weight and both shapes
    four = U.UNet2DConditionModel(ucfg(4), "cpu", seed=3)
    assert four.store.params["conv_in.weight"].shape == (c0, 3, 3, 8)
    with pytest.raises(ValueError, match=rf"conv_in.weight: shape \({c0}, 4, 3, 3\) != \({c0}, 9, 3, 3\)"):
        apply_unet_state_dict(b, four.state_dict())
    with pytest.raises(ValueError, match=rf"conv_in.weight: shape \({c0}, 9, 3, 3\) != \({c0}, 4, 3, 3\)"):
        apply_unet_state_dict(four, sd)
    # the model type decides the width create_model admits
    inp, plain = (TYPES[1], "STABLE_DIFFUSION_XL_10_BASE") if sdxl else (TYPES[0], "STABLE_DIFFUSION_15")
    cfg = TrainConfig.default_values()
    cfg.model_type = inp
    with pytest.raises(ValueError, match=rf"conv_in.weight: shape \({c0}, 4, 3, 3\) != \({c0}, 9, 3, 3\)"):
        create.create_model(cfg, "cpu", unet_config=ucfg(4))
    cfg.model_type = plain
    with pytest.raises(ValueError, match=rf"conv_in.weight: shape \({c0}, 9, 3, 3\) != \({c0}, 4, 3, 3\)"):
        create.create_model(cfg, "cpu", unet_config=ucfg(9))
    assert LC is not None
