"""Validation loss, host side: the concept split (held-out images never reach the training enumeration), concept
indices and scalar labels, the validate timer, and the three config fields with the reference's defaults."""
import json
import os
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from onetrainer_amd.dataLoader import create as DC
from onetrainer_amd.dataLoader.latent_cache import LatentCacheDataLoader, LatentCacheWriter
from onetrainer_amd.trainer.GenericTrainer import GenericTrainer
from onetrainer_amd.util.config.TrainConfig import TrainConfig
from onetrainer_amd.util.TrainProgress import TrainProgress

GOLDEN = Path(__file__).resolve().parent / "golden" / "reference_trainconfigs.json"


def _concept_dirs(tmp_path):
    from PIL import Image
    spec = {"train": 3, "held": 2, "legacy": 1, "off": 2}
    for name, n in spec.items():
        d = tmp_path / name
        d.mkdir()
        for i in range(n):
            Image.new("RGB", (16, 16), (i * 40, 10, 10)).save(d / f"{name}{i}.png")
            (d / f"{name}{i}.txt").write_text(f"a {name} {i}")
    return [
        {"name": "train", "path": str(tmp_path / "train"), "type": "STANDARD", "seed": 1},
        {"name": "", "path": str(tmp_path / "held"), "type": "VALIDATION", "seed": 2},
        {"name": "old", "path": str(tmp_path / "legacy"), "validation_concept": True, "seed": 3},
        {"name": "off", "path": str(tmp_path / "off"), "type": "VALIDATION", "enabled": False, "seed": 4},
    ]


def _cfg(concepts, **kw):
    cfg = TrainConfig.default_values()
    cfg.concepts = concepts
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_split_keeps_held_out_images_out_of_training(tmp_path):
    cfg = _cfg(_concept_dirs(tmp_path))
    for validation in (False, True):   # the split applies whether or not the pass is on, as in the reference
        cfg.validation = validation
        train = DC.enumerate_samples(cfg)
        assert [os.path.basename(p) for p, _ in train] == ["train0.png", "train1.png", "train2.png"]
        assert [c for _, c in train] == ["a train 0", "a train 1", "a train 2"]
        held = DC.enumerate_validation_samples(cfg)
        assert [os.path.basename(v["sample"][0]) for v in held] == ["held0.png", "held1.png", "legacy0.png"]
        assert [v["concept_index"] for v in held] == [0, 0, 1]
        assert [(v["name"], os.path.basename(v["path"]), v["seed"]) for v in held] == \
            [("", "held", 2), ("", "held", 2), ("old", "legacy", 3)]
    assert DC.validation_labels(DC.validation_concepts(cfg)) == ["held", "old"]


def test_config_without_validation_concepts_enumerates_as_before(tmp_path):
    concepts = [c for c in _concept_dirs(tmp_path) if c["name"] == "train"]
    concepts.append({"path": str(tmp_path / "held")})   # no type at all: a STANDARD concept
    cfg = _cfg(concepts, validation=True)
    assert len(DC.enumerate_samples(cfg)) == 5
    assert DC.enumerate_validation_samples(cfg) == []
    assert not DC.validation_cache_needed(cfg)          # validation on, nothing held out: the pass is skipped
    assert DC.create_validation_data_loader(cfg, "cpu") is None


def test_labels_collisions_and_shared_seeds():
    c = lambda name, path, seed: {"name": name, "path": path, "seed": seed}   # noqa: E731
    assert DC.validation_labels([c("x", "/a", 1), c("x", "/b", 2)]) == ["x", "x(1)"]
    assert DC.validation_labels([c("x", "/a", 1), c("x", "/b", 1)]) == ["x", "x"]
    assert DC.validation_labels([c("x", "/a", 1), c("x", "/b", 2), c("x", "/c", 3)]) == ["x", "x(1)", "x(2)"]
    assert DC.validation_labels([c("", "/data/dogs", 5), c("", "/other/dogs", 6)]) == ["dogs", "dogs(1)"]
    # a concept of a seed that already has a label takes that label, whatever its own name
    assert DC.validation_labels([c("x", "/a", 1), c("y", "/b", 1)]) == ["x", "x"]


def _timer_trainer(**kw):
    cfg = TrainConfig.default_values()
    for k, v in kw.items():
        setattr(cfg, k, v)
    return GenericTrainer(cfg, model=SimpleNamespace(train_progress=TrainProgress()))


def test_validate_timer_units():
    tr = _timer_trainer(validation=True, validate_after=2, validate_after_unit="STEP")
    assert [g for g in range(8) if tr._needs_validate(TrainProgress(global_step=g))] == [0, 2, 4, 6]
    tr = _timer_trainer(validation=True, validate_after=1, validate_after_unit="EPOCH")
    assert tr._needs_validate(TrainProgress(epoch=0, epoch_step=0))
    assert not tr._needs_validate(TrainProgress(epoch=0, epoch_step=1, global_step=1))
    assert tr._needs_validate(TrainProgress(epoch=1, epoch_step=0, global_step=5))
    tr = _timer_trainer(validation=True, validate_after=2, validate_after_unit="EPOCH")
    assert not tr._needs_validate(TrainProgress(epoch=1, epoch_step=0, global_step=5))
    assert tr._needs_validate(TrainProgress(epoch=2, epoch_step=0, global_step=10))
    tr = _timer_trainer(validation=False, validate_after=1, validate_after_unit="STEP")
    assert not any(tr._needs_validate(TrainProgress(global_step=g)) for g in range(4))
    assert not _timer_trainer(validation=False, validate_after_unit="ALWAYS")._needs_validate(TrainProgress())


def test_wall_clock_validate_timer_is_refused_under_data_parallel():
    """the ranks' clocks would not agree on a pass that ends in a collective"""
    for unit in ("SECOND", "MINUTE", "HOUR"):
        tr = _timer_trainer(validation=True, validate_after=1, validate_after_unit=unit)
        tr.world, tr.data_loader = 2, object()
        with pytest.raises(NotImplementedError, match="validate_after_unit"):
            tr.train(log_every=0)


def test_config_fields_round_trip_and_reference_defaults():
    d = TrainConfig.default_values()
    assert (d.validation, d.validate_after, d.validate_after_unit) == (False, 1, "EPOCH")
    ref = json.loads(GOLDEN.read_text())["configs"]
    for name, rec in ref.items():   # the reference's own defaults, as recorded from its TrainConfig
        c = rec["__config__"]
        assert c["validation"] is d.validation, name
        assert c["validate_after"] == d.validate_after, name
        assert c["validate_after_unit"]["name"] == d.validate_after_unit, name
    cfg = TrainConfig().from_dict({"validation": True, "validate_after": 250, "validate_after_unit": "STEP"})
    assert (cfg.validation, cfg.validate_after, cfg.validate_after_unit) == (True, 250, "STEP")
    assert not {"validation", "validate_after", "validate_after_unit"} & set(cfg.extra)   # read, not dropped
    back = TrainConfig().from_dict(cfg.to_settings_dict())
    assert (back.validation, back.validate_after, back.validate_after_unit) == (True, 250, "STEP")


def _write_validation_cache(cache_dir, shapes_and_concepts):
    """a synthetic held-out cache: identity 'VAE' (a strided slice), one record per (H, W, concept index)"""
    enc = lambda im: im[:, :, ::8, ::8].permute(0, 2, 3, 1).repeat(1, 1, 1, 2)[..., :4].contiguous()  # noqa: E731

    class Bucketing:   # every image keeps its own size
        def bucket_for(self, h, w):
            return (h, w), (h, w)

    g = torch.Generator().manual_seed(0)
    rows = [{"image": torch.rand(3, h, w, generator=g), "concept_index": ci,
             "text": {"text_encoder_1_hidden_state": torch.full((2, 4), float(i))}}
            for i, (h, w, ci) in enumerate(shapes_and_concepts)]
    concepts = [{"name": "a", "path": "/a", "seed": 1}, {"name": "b", "path": "/b", "seed": 2}]
    LatentCacheWriter(enc, str(cache_dir), Bucketing(), "cpu", concepts=concepts).write(rows)
    return concepts


def test_validation_loader_every_sample_once_in_fixed_order(tmp_path):
    shapes = [(32, 16, 0), (16, 16, 0), (32, 16, 1), (16, 16, 1), (32, 16, 0)]
    concepts = _write_validation_cache(tmp_path / "validation", shapes)
    meta = json.loads((tmp_path / "validation" / "index.json").read_text())
    assert [s["concept_index"] for s in meta["samples"]] == [0, 0, 1, 1, 0] and meta["concepts"] == concepts

    def run(batch_size, rank=0, world=1):
        ld = LatentCacheDataLoader(str(tmp_path / "validation"), batch_size, "cpu", rank=rank, world=world,
                                   prefetch=False, validation=True)
        out = []
        for _ in range(2):   # two passes: the same order, no shuffle between them
            ld.get_data_set().start_next_epoch()
            got = []
            for b in ld.get_data_loader():
                assert b["concept_index"].dtype == torch.int32 and b["concept_index"].shape == (len(b["loss_weight"]),)
                assert b["concept_index_host"].tolist() == b["concept_index"].tolist()
                assert len({tuple(b["latent_image"].shape[1:])}) == 1
                ids = b["text_encoder_1_hidden_state"][:, 0, 0].int().tolist()   # the sample's cache index
                got.append((ids, b["concept_index"].tolist()))
            out.append(got)
        assert out[0] == out[1]
        return out[0]

    # buckets in ascending resolution, cache index order inside; the short last batch of a bucket is run short
    assert run(2) == [([1, 3], [0, 1]), ([0, 2], [0, 1]), ([4], [0])]
    assert run(1) == [([1], [0]), ([3], [1]), ([0], [0]), ([2], [1]), ([4], [0])]
    assert run(4) == [([1, 3], [0, 1]), ([0, 2, 4], [0, 1, 0])]
    # data parallel: every rank takes a slice, together every sample exactly once
    r0, r1 = run(1, 0, 2), run(1, 1, 2)
    assert sorted(i for ids, _ in r0 + r1 for i in ids) == [0, 1, 2, 3, 4]
    assert r0 == [([1], [0]), ([0], [0]), ([4], [0])] and r1 == [([3], [1]), ([2], [1])]
    assert LatentCacheDataLoader(str(tmp_path / "validation"), 2, "cpu", validation=True).concepts == concepts
