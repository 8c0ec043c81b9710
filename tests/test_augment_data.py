"""Concept augmentations and cached image variations through the latent cache (CPU): the oracle stands in for the
kernel as augment_fn, a resize of the first channel for the VAE."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from safetensors.torch import load_file

import _oracle_augment as O
from onetrainer_amd.dataLoader import augment as A
from onetrainer_amd.dataLoader.aspect_bucketing import AspectBucketing
from onetrainer_amd.dataLoader.create import concept_extras, enumerate_samples
from onetrainer_amd.dataLoader.latent_cache import (LatentCacheDataLoader, LatentCacheWriter, mask_to_latent_grid,
                                                    scale_only)


def _first_channel_latent(imgs):
    x = F.interpolate(imgs[:, :1], size=(imgs.shape[2] // 8, imgs.shape[3] // 8), mode="bilinear", antialias=True,
                      align_corners=False)
    return x.permute(0, 2, 3, 1)


def _never(*a, **k):
    raise AssertionError("augment_fn called for a row without augmentation")


def _images(shapes, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(3, h, w, generator=g) for h, w in shapes]


SHAPES = [(128, 128), (100, 170), (170, 100), (128, 160), (128, 128)]
TEXT = {"text_encoder_hidden_state": torch.arange(77 * 8, dtype=torch.float32).reshape(77, 8).bfloat16()}


def test_plain_rows_never_reach_augment_fn(tmp_path):
    """no augmentation keys, image_variations absent: today's files, record keys and index, byte for byte the same
    with and without the concept's (empty) settings riding on the rows"""
    imgs = _images(SHAPES)
    plain = [{"image": im, "text": dict(TEXT)} for im in imgs]
    rows = [dict(r, **concept_extras({"path": "x", "image": {"enable_resolution_override": True}}, i))
            for i, r in enumerate(plain)]
    ab = AspectBucketing(128, 64)
    LatentCacheWriter(_first_channel_latent, str(tmp_path / "a"), ab, "cpu", encode_batch=2, augment_fn=_never).write(rows)
    LatentCacheWriter(_first_channel_latent, str(tmp_path / "b"), ab, "cpu", encode_batch=2, augment_fn=_never).write(plain)
    index = json.loads((tmp_path / "a" / "index.json").read_text())
    assert set(index) == {"version", "samples"} and index["version"] == 1
    assert all(set(s) == {"file", "crop_resolution"} for s in index["samples"])
    assert [s["file"] for s in index["samples"]] == [f"{i:08d}.safetensors" for i in range(len(imgs))]
    assert sorted(os.listdir(tmp_path / "a")) == sorted([f"{i:08d}.safetensors" for i in range(len(imgs))] + ["index.json"])
    for name in os.listdir(tmp_path / "a"):
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes(), name
    rec = load_file(str(tmp_path / "a" / "00000001.safetensors"))
    assert set(rec) == {"latent_image", "original_resolution", "crop_offset", "crop_resolution",
                        "text_encoder_hidden_state"}
    batch = next(iter(LatentCacheDataLoader(str(tmp_path / "a"), 2, "cpu", prefetch=False).get_data_loader()))
    assert torch.equal(batch["loss_weight"], torch.ones(2)) and batch["loss_weight"].dtype == torch.float32


JITTER = {"enable_crop_jitter": True, "enable_random_flip": True, "enable_random_hue": True,
          "random_hue_max_strength": 0.2}


def _write_v3(tmp_path, encode_batch=2, order=None, masks=False):
    imgs = _images(SHAPES, seed=1)
    # with masks: geometry only (and a small turn), so the image's first channel stays the mask's twin
    image_cfg = JITTER if not masks else {"enable_crop_jitter": True, "enable_random_flip": True,
                                          "enable_random_rotate": True, "random_rotate_max_angle": 15.0}
    concept = {"path": "x", "seed": 11, "image_variations": 3, "image": image_cfg}
    rows = [dict({"image": im, "text": dict(TEXT)}, **concept_extras(concept, i)) for i, im in enumerate(imgs)]
    if masks:
        for r in rows:
            m = torch.zeros(1, *r["image"].shape[1:])
            m[:, : m.shape[1] // 3, : m.shape[2] // 4] = 1.0        # one corner: neither flip- nor turn-symmetric
            r["mask"] = m
            r["image"] = torch.cat([m, r["image"][1:]])              # the stand-in latent is the image's first channel
    if order is not None:
        rows = [rows[i] for i in order]
    calls = []

    def fn(entries, src, out_numel, H, W):
        calls.append(len(entries))
        return O.augment_fn(entries, src, out_numel, H, W)
    ab = AspectBucketing(128, 64)
    LatentCacheWriter(_first_channel_latent, str(tmp_path), ab, "cpu", encode_batch=encode_batch, augment_fn=fn).write(rows)
    return imgs, ab, calls


def test_three_variations_per_image(tmp_path):
    imgs, ab, calls = _write_v3(tmp_path)
    assert calls and sum(calls) == 3 * len(imgs)
    index = json.loads((tmp_path / "index.json").read_text())["samples"]
    offsets = set()
    for i, (im, s) in enumerate(zip(imgs, index)):
        assert s["file"] == f"{i:08d}.safetensors" and s["variations"] == [f"{i:08d}.v1.safetensors",
                                                                          f"{i:08d}.v2.safetensors"]
        assert "loss_weight" not in s
        scale_res, crop_res = ab.bucket_for(im.shape[1], im.shape[2])
        base = load_file(str(tmp_path / s["file"]))
        assert "text_encoder_hidden_state" in base and "original_resolution" in base
        lat = []
        for v in range(3):
            rec = base if v == 0 else load_file(str(tmp_path / s["variations"][v - 1]))
            if v:
                assert set(rec) == {"latent_image", "crop_offset"}            # the text state is stored once
            p = O.draw(JITTER, 11, i, v, scale_res, crop_res)
            assert rec["crop_offset"].tolist() == [p["y0"], p["x0"]]         # the jitter moves it
            offsets.add((i, p["y0"], p["x0"], p["flip"]))
            e = A.entry(p, 0, 0, 3, scale_res, crop_res)
            want = O.augment(scale_only(im, scale_res).numpy(), e).astype(np.float32)
            want = _first_channel_latent(torch.from_numpy(want)[None])[0]
            torch.testing.assert_close(rec["latent_image"], want, rtol=0, atol=1e-6)
            lat.append(rec["latent_image"])
        assert not torch.equal(lat[0], lat[1]) and not torch.equal(lat[1], lat[2])
    assert len(offsets) > len(imgs)                                         # variations really differ in geometry


def test_draws_do_not_depend_on_grouping(tmp_path):
    """another encode_batch and another sample order (so other chunks) give the same latents per image"""
    _write_v3(tmp_path / "a", encode_batch=2)
    order = [4, 2, 0, 3, 1]
    _write_v3(tmp_path / "b", encode_batch=5, order=order)
    for new, old in enumerate(order):
        for v in range(3):
            a = load_file(str(tmp_path / "a" / (f"{old:08d}.safetensors" if v == 0 else f"{old:08d}.v{v}.safetensors")))
            b = load_file(str(tmp_path / "b" / (f"{new:08d}.safetensors" if v == 0 else f"{new:08d}.v{v}.safetensors")))
            # the image's index within its concept keys the draw, not its place in the write
            assert torch.equal(a["latent_image"], b["latent_image"]) and torch.equal(a["crop_offset"], b["crop_offset"])


def test_reader_cycles_variations_with_the_epoch(tmp_path):
    """variation (epoch mod 3): 0, 1, 2, 0 over four epochs; a resumed run (the trainer hands the restored epoch
    number over) reads the files the uninterrupted run read"""
    imgs, _, _ = _write_v3(tmp_path)
    n = len(imgs)
    recs = [[load_file(str(tmp_path / (f"{i:08d}.safetensors" if v == 0 else f"{i:08d}.v{v}.safetensors")))
             for v in range(3)] for i in range(n)]
    dl = LatentCacheDataLoader(str(tmp_path), 1, "cpu", prefetch=False)
    files = []
    for epoch in range(4):
        dl.start_next_epoch()
        files.append([dl.variation_files(i) for i in range(n)])
        seen = 0
        for batch, idx in zip(dl.get_data_loader(), dl._batches):
            want = recs[idx[0]][epoch % 3]
            assert torch.equal(batch["latent_image"][0].permute(1, 2, 0), want["latent_image"])
            assert [batch["crop_offset"][0].item(), batch["crop_offset"][1].item()] == want["crop_offset"].tolist()
            assert torch.equal(batch["text_encoder_hidden_state"][0], TEXT["text_encoder_hidden_state"])
            seen += 1
        assert seen == n
    assert files[0] == files[3] and files[0] != files[1] != files[2]
    assert all(len(f) == 1 for f in files[0]) and all(f[1].endswith(".v2.safetensors") for f in files[2])
    resumed = LatentCacheDataLoader(str(tmp_path), 1, "cpu", prefetch=False)   # its own count starts over
    resumed.start_next_epoch()
    resumed.set_variation_epoch(2)
    assert [resumed.variation_files(i) for i in range(n)] == files[2]
    batch = next(iter(resumed.get_data_loader()))
    assert torch.equal(batch["latent_image"][0].permute(1, 2, 0), recs[resumed._batches[0][0]][2]["latent_image"])


def test_trainer_hands_the_restored_epoch_to_the_loader():
    """GenericTrainer.train: the loop runs from the restored epoch and tells the data set which one it is"""
    import inspect

    from onetrainer_amd.trainer.GenericTrainer import GenericTrainer
    src = inspect.getsource(GenericTrainer.train)
    assert "for _epoch in range(tp.epoch, cfg.epochs)" in src and "set_variation_epoch(_epoch)" in src


def test_mask_takes_its_images_geometry(tmp_path):
    """fixed flip + a fixed quarter turn, centre crop: the mask (one corner set) lands where the image's does"""
    cfg = {"enable_fixed_flip": True, "enable_fixed_rotate": True, "random_rotate_max_angle": 90.0}
    m = torch.zeros(1, 128, 128)
    m[:, :40, :24] = 1.0
    img = torch.cat([m, torch.rand(2, 128, 128)])
    row = dict({"image": img, "mask": m}, **concept_extras({"path": "x", "image": cfg}, 0))
    LatentCacheWriter(_first_channel_latent, str(tmp_path), AspectBucketing(128, 64), "cpu",
                      augment_fn=O.augment_fn).write([row])
    rec = load_file(str(tmp_path / "00000000.safetensors"))
    lm = rec["latent_mask"]
    assert lm.shape == (1, 16, 16)
    torch.testing.assert_close(lm[0], rec["latent_image"][..., 0].clamp(0, 1), rtol=0, atol=1e-6)
    want = torch.from_numpy(np.rot90(m[0].numpy()[:, ::-1], 1).copy())[None]   # flip, then counter-clockwise
    torch.testing.assert_close(lm, mask_to_latent_grid(want, (16, 16)), rtol=0, atol=1e-5)
    others = [m[0].numpy(), m[0].numpy()[:, ::-1], np.rot90(m[0].numpy(), 1), np.rot90(m[0].numpy()[:, ::-1], -1)]
    for o in others:                       # not where it started, not flipped only, turned only or turned the other way
        assert (lm - mask_to_latent_grid(torch.from_numpy(o.copy())[None], (16, 16))).abs().max() > 0.8


def test_masks_of_variations_are_cached_per_variation(tmp_path):
    imgs, ab, _ = _write_v3(tmp_path, masks=True)
    for i in range(len(imgs)):
        for v in range(3):
            rec = load_file(str(tmp_path / (f"{i:08d}.safetensors" if v == 0 else f"{i:08d}.v{v}.safetensors")))
            if v:
                assert set(rec) == {"latent_image", "crop_offset", "latent_mask"}
            torch.testing.assert_close(rec["latent_mask"][0], rec["latent_image"][..., 0].clamp(0, 1), rtol=0, atol=1e-6)
    dl = LatentCacheDataLoader(str(tmp_path), 1, "cpu", prefetch=False, require_mask=True)
    dl.start_next_epoch()
    dl.start_next_epoch()
    for batch in dl.get_data_loader():
        torch.testing.assert_close(batch["latent_mask"][0, 0], batch["latent_image"][0, 0].clamp(0, 1), rtol=0, atol=1e-6)


def test_concept_loss_weight_reaches_the_batch(tmp_path):
    imgs = _images([(128, 128)] * 4)
    half = {"path": "x", "loss_weight": 0.5}
    rows = [dict({"image": im}, **concept_extras(half if i % 2 else {"path": "y"}, i // 2)) for i, im in enumerate(imgs)]
    LatentCacheWriter(_first_channel_latent, str(tmp_path), AspectBucketing(128, 64), "cpu", augment_fn=_never).write(rows)
    index = json.loads((tmp_path / "index.json").read_text())["samples"]
    assert [s.get("loss_weight") for s in index] == [None, 0.5, None, 0.5]
    for prefetch in (False, True):
        dl = LatentCacheDataLoader(str(tmp_path), 4, "cpu", prefetch=prefetch)
        dl.start_next_epoch()
        (batch,), (idx,) = list(dl.get_data_loader()), dl._batches
        assert batch["loss_weight"].dtype == torch.float32
        assert batch["loss_weight"].tolist() == [0.5 if i % 2 else 1.0 for i in idx]


def test_reference_concept_trains_on_four_cycling_variations_at_half_weight(tmp_path):
    """a concept as the reference's UI writes it: jitter and flip on (its defaults), image_variations 4, loss_weight
    0.5 -- through enumerate / concept_extras / the writer / the reader"""
    from PIL import Image
    d = tmp_path / "concept"
    d.mkdir()
    g = np.random.default_rng(0)
    for name in ("a", "b"):
        Image.fromarray((g.random((96, 140, 3)) * 255).astype(np.uint8)).save(d / f"{name}.png")
    concept = {"path": str(d), "seed": 3, "enabled": True, "image_variations": 4, "loss_weight": 0.5,
               "image": {"enable_crop_jitter": True, "enable_random_flip": True, "enable_fixed_flip": False,
                         "enable_random_rotate": False, "random_rotate_max_angle": 0.0,
                         "enable_random_circular_mask_shrink": False, "enable_random_mask_rotate_crop": False}}
    samples = enumerate_samples(SimpleNamespace(concepts=[concept], concept_file_name="", masked_training=False))
    rows = [dict({"image": Image.open(s[0])}, **concept_extras(concept, i)) for i, s in enumerate(samples)]
    cache = tmp_path / "cache"
    LatentCacheWriter(_first_channel_latent, str(cache), AspectBucketing(128, 64), "cpu",
                      augment_fn=O.augment_fn).write(rows)
    dl = LatentCacheDataLoader(str(cache), 2, "cpu", prefetch=False)
    seen = []
    for _ in range(5):
        dl.start_next_epoch()
        (batch,) = list(dl.get_data_loader())
        assert batch["loss_weight"].tolist() == [0.5, 0.5]
        order = np.argsort(dl._batches[0])
        seen.append(batch["latent_image"][order])
    assert torch.equal(seen[0], seen[4])
    assert all(not torch.equal(seen[a], seen[b]) for a in range(4) for b in range(a + 1, 4))


@pytest.mark.parametrize("knob", ["enable_random_circular_mask_shrink", "enable_random_mask_rotate_crop"])
def test_mask_augmentations_still_raise(tmp_path, knob):
    from PIL import Image
    Image.new("RGB", (16, 16)).save(tmp_path / "a.png")
    concept = {"path": str(tmp_path), "image": {knob: True, "enable_random_flip": True}}
    with pytest.raises(NotImplementedError, match=knob):
        enumerate_samples(SimpleNamespace(concepts=[concept], concept_file_name="", masked_training=True))
