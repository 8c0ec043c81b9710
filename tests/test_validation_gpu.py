"""Validation loss on the GPU: the accumulate kernel against the sequential float64 oracle (exact bits), and the
pass on tiny SDXL / SD 1.5 / FLUX models over a synthetic held-out latent cache: batch-independent per-sample losses,
per-concept means equal to the existing per-sample autograd path, the scalars written, training untouched.

Every comparison is exact by construction (the same kernels, a fixed order, double sums); there is no tolerance.

Measured on an MI355X: the figures of a run are printed before each assertion."""
import json
import os

import numpy as np
import pytest
import torch
from safetensors.torch import save_file

import _oracle_validation as OV
from onetrainer_amd import kernels as K
from onetrainer_amd.dataLoader.latent_cache import LatentCacheDataLoader
from onetrainer_amd.dataLoader.SyntheticDataLoader import synthetic_sdxl_batch
from onetrainer_amd.module import unet as U
from onetrainer_amd.trainer.GenericTrainer import GenericTrainer
from onetrainer_amd.util import create
from onetrainer_amd.util.config.TrainConfig import TrainConfig
from onetrainer_amd.util.tensorboard import ScalarLog, read_scalars

pytestmark = pytest.mark.gpu

CONCEPTS = [{"name": "held", "path": "/data/held", "seed": 11}, {"name": "", "path": "/data/dogs", "seed": 12}]
# (latent h, latent w, concept): two validation concepts of 3 and 2 samples over two bucket shapes
SAMPLES = [(8, 8, 0), (8, 16, 0), (8, 8, 1), (8, 16, 1), (8, 8, 0)]


# ----- the accumulate kernel ----------------------------------------------------------------------
def _losses(n, seed):
    rng = np.random.default_rng(seed)
    return (10.0 ** rng.uniform(-6, 3, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


@pytest.mark.parametrize("host_layer", ["native", "python"])
@pytest.mark.parametrize("n_concepts", [1, 2, 7])
@pytest.mark.parametrize("B", [1, 3, 64, 1024])
def test_accumulate_equals_sequential_float64(dev, B, n_concepts, host_layer):
    used = 5 if n_concepts == 7 else n_concepts   # with 7 concepts two of them receive no sample
    acc = torch.zeros((n_concepts, 2), dtype=torch.float64, device=dev)
    ref = np.zeros((n_concepts, 2))
    for call in range(3):           # three successive calls accumulate into the same buffer
        losses = _losses(B, 100 * B + call)
        idx = np.random.default_rng(7 * B + call).integers(0, used, B).astype(np.int32)
        li, ii = torch.from_numpy(losses).to(dev), torch.from_numpy(idx).to(dev)
        if host_layer == "python":
            with K.python_host():
                K.validation_accumulate(li, ii, n_concepts, acc, index_host=torch.from_numpy(idx))
        else:
            K.validation_accumulate(li, ii, n_concepts, acc, index_host=torch.from_numpy(idx) if call else None)
        OV.accumulate(ref, losses, idx)
    got = acc.cpu().numpy()
    assert got.view(np.int64).tolist() == ref.view(np.int64).tolist()   # the float64 bits
    assert (got[used:] == 0).all()


@pytest.mark.parametrize("host_layer", ["native", "python"])
def test_accumulate_rejects_an_index_out_of_range(dev, host_layer):
    acc = torch.tensor([[1.5, 2.0], [-3.0, 1.0]], dtype=torch.float64, device=dev)
    before = acc.clone()
    losses = torch.tensor([1.0, 2.0, 3.0], device=dev)
    for bad in ([0, 2, 1], [0, -1, 1]):
        idx = torch.tensor(bad, dtype=torch.int32)
        with pytest.raises(RuntimeError, match="invalid arguments"):
            if host_layer == "python":
                with K.python_host():
                    K.validation_accumulate(losses, idx.to(dev), 2, acc, index_host=idx)
            else:
                K.validation_accumulate(losses, idx.to(dev), 2, acc, index_host=idx)
        assert torch.equal(acc, before)
        # without the host copy the launcher cannot know: the kernel skips the sample, nothing out of range is written
        guard = torch.full((4, 2), 7.0, dtype=torch.float64, device=dev)
        K.validation_accumulate(losses, idx.to(dev), 2, guard[1:3], index_host=None)
        assert guard.cpu().tolist() == [[7.0, 7.0], [8.0, 8.0], [10.0, 8.0], [7.0, 7.0]]


def test_noise_per_sample_is_the_batch_of_one(dev):
    for ow, pw, dtype in ((0.0, 0.0, torch.float32), (0.3, 0.2, torch.float32), (0.3, 0.0, torch.bfloat16)):
        one = K.noise_ex((1, 5, 3, 4), seed=0, offset=0, offset_weight=ow, perturbation_weight=pw, dtype=dtype, device=dev)
        many = K.noise_per_sample((3, 5, 3, 4), seed=0, offset_weight=ow, perturbation_weight=pw, dtype=dtype, device=dev)
        assert all(torch.equal(many[b], one[0]) for b in range(3))
    assert torch.equal(K.noise_per_sample((2, 5, 3, 4), seed=9, dtype=torch.float32, device=dev)[1],
                       K.noise((1, 5, 3, 4), seed=9, dtype=torch.float32, device=dev)[0])


def test_lora_dropout_per_sample_rows(dev):
    seed = torch.tensor([0], dtype=torch.int64, device=dev)
    for width in (8, 6):
        one = K.lora_dropout(torch.ones(5, width, dtype=torch.bfloat16, device=dev), seed, 3, 0, 0.5)
        rows = K.lora_dropout(torch.ones(15, width, dtype=torch.bfloat16, device=dev), seed, 3, 0, 0.5, rows_per=5)
        assert torch.equal(rows.view(3, 5, width), one.expand(3, 5, width))          # sample-major rows
        tok = K.lora_dropout(torch.ones(15, width, dtype=torch.bfloat16, device=dev), seed, 3, 0, 0.5, rows_per=-3)
        assert torch.equal(tok.view(5, 3, width), one[:, None].expand(5, 3, width))   # token-major rows (r = t B + b)
        assert 0 < one.float().sum() < 2 * 5 * width


# ----- the pass on tiny models ---------------------------------------------------------------------
def _write_cache(cache_dir, family, masked, C):
    os.makedirs(cache_dir, exist_ok=True)
    g = torch.Generator().manual_seed(5)
    index = []
    for i, (h, w, ci) in enumerate(SAMPLES):
        rec = {"latent_image": (torch.randn(h, w, C, generator=g) / 0.3).contiguous(),
               "original_resolution": torch.tensor([h * 8, w * 8]), "crop_offset": torch.tensor([0, 0]),
               "crop_resolution": torch.tensor([h * 8, w * 8])}
        bf = lambda *s: torch.randn(*s, generator=g).bfloat16()   # noqa: E731
        if family == "sdxl":
            rec.update(text_encoder_1_hidden_state=bf(77, 32), text_encoder_2_hidden_state=bf(77, 64),
                       text_encoder_2_pooled_state=bf(64))
        else:
            rec.update(text_encoder_hidden_state=bf(77, 96))
        if masked:
            rec["latent_mask"] = (torch.rand(1, h, w, generator=g) > 0.4).float()
        fn = f"{i:08d}.safetensors"
        save_file(rec, os.path.join(cache_dir, fn))
        index.append({"file": fn, "crop_resolution": [h * 8, w * 8], "concept_index": ci})
    with open(os.path.join(cache_dir, "index.json"), "w") as f:
        json.dump({"version": 1, "samples": index, "concepts": CONCEPTS}, f)


def _write_flux_cache(cache_dir, fcfg):
    os.makedirs(cache_dir, exist_ok=True)
    g = torch.Generator().manual_seed(5)
    index = []
    for i, (h, w, ci) in enumerate(SAMPLES):
        rec = {"latent_image": (torch.randn(h, w, 16, generator=g) / 0.3611 + 0.1159).contiguous(),
               "original_resolution": torch.tensor([h * 8, w * 8]), "crop_offset": torch.tensor([0, 0]),
               "crop_resolution": torch.tensor([h * 8, w * 8]),
               "text_encoder_1_pooled_state": torch.randn(fcfg.pooled_projection_dim, generator=g).bfloat16(),
               "text_encoder_2_hidden_state": torch.randn(9, fcfg.joint_attention_dim, generator=g).bfloat16()}
        fn = f"{i:08d}.safetensors"
        save_file(rec, os.path.join(cache_dir, fn))
        index.append({"file": fn, "crop_resolution": [h * 8, w * 8], "concept_index": ci})
    with open(os.path.join(cache_dir, "index.json"), "w") as f:
        json.dump({"version": 1, "samples": index, "concepts": CONCEPTS}, f)


class _Loader:
    """the training side: one resident synthetic batch, `steps` times"""

    def __init__(self, batch, steps):
        self.batch, self.steps = batch, steps

    def get_data_set(self):
        return self

    def approximate_length(self):
        return self.steps

    def start_next_epoch(self):
        pass

    def get_data_loader(self):
        return iter([self.batch] * self.steps)


def _trainer(dev, tmp, family, masked=False, validation=True, steps=2, textdrop=False, **kw):
    cfg = TrainConfig.default_values()
    cfg.batch_size, cfg.epochs = 2, 1
    cfg.learning_rate, cfg.learning_rate_warmup_steps = 1e-3, 0
    cfg.workspace_dir, cfg.cache_dir = str(tmp / "ws"), str(tmp / "cache")
    cfg.backup_after_unit = "NEVER"
    cfg.sample_definition_file_name = str(tmp / "none.json")
    cfg.validation, cfg.validate_after, cfg.validate_after_unit = validation, 1, "STEP"
    if masked:
        cfg.masked_training, cfg.mae_strength, cfg.mse_strength = True, 0.5, 0.75
    if textdrop:
        # Random(0) draws 0.844, 0.758, 0.421, ...: as a batch of one every sample keeps both encoders' text (first
        # draw > 0.8, second > 0.5); drawn per batch, the second sample of a batch would lose the first encoder's
        cfg.text_encoder.dropout_probability, cfg.text_encoder_2.dropout_probability = 0.8, 0.5
        cfg.offset_noise_weight, cfg.perturbation_noise_weight = 0.3, 0.2
    for k, v in kw.items():
        setattr(cfg, k, v)
    vdir = os.path.join(cfg.cache_dir, "validation")
    if family == "flux":
        from onetrainer_amd.dataLoader.SyntheticDataLoader import synthetic_flux_batch
        from onetrainer_amd.module import flux as FX
        cfg.model_type = "FLUX_DEV_1"
        fcfg = FX.tiny_flux_config()
        model = create.create_model(cfg, dev, seed=3, flux_config=fcfg)
        _write_flux_cache(vdir, fcfg)
        batch = synthetic_flux_batch(2, 64, 64, dev, seed=1, t5_dim=fcfg.joint_attention_dim,
                                     pooled_dim=fcfg.pooled_projection_dim, text_len=9)
    else:
        sd15 = family == "sd15"
        if sd15:
            cfg.model_type = "STABLE_DIFFUSION_15"
        model = create.create_model(cfg, dev, seed=4, unet_config=U.tiny_sd15_config() if sd15 else U.tiny_sdxl_config())
        _write_cache(vdir, family, masked, 4)
        batch = synthetic_sdxl_batch(2, 64, 64, dev, 0, te1_dim=32, te2_dim=64, pooled_dim=64) if not sd15 \
            else synthetic_sdxl_batch(2, 64, 64, dev, 0, te1_dim=96, sdxl=False)
        if masked:
            batch["latent_mask"] = (torch.rand(2, 1, 8, 8, generator=torch.Generator().manual_seed(1)) > 0.4).float().to(dev)
    tr = GenericTrainer(cfg, model=model, data_loader=_Loader(batch, steps))
    tr.start()
    return tr


def _bits(t):
    return t.contiguous().view(torch.int32).tolist()


LORA = dict(training_method="LORA", lora_rank=8, lora_alpha=8.0, dropout_probability=0.25)


@pytest.mark.parametrize("case", ["sdxl", "sd15", "sdxl-masked-mae", "flux", "sdxl-textdrop-noise",
                                  "sd15-textdrop-noise", "flux-lora-textdrop-noise"])
def test_pass_is_batch_independent_and_equals_the_per_sample_path(dev, tmp_path, case):
    """-textdrop-noise: text dropout on every encoder and offset + perturbation noise, so the per-sample forms of
    all three run through a model; -lora: LoRA dropout, on FLUX the token-major row numbering"""
    family, masked = case.split("-")[0], "masked" in case
    tr = _trainer(dev, tmp_path, family, masked=masked, textdrop="textdrop" in case, **(LORA if "lora" in case else {}))
    if "lora" in case:
        lora = tr.model.transformer_lora
        assert lora.dropout_p == 0.25 and lora.token_major
    cfg, model, setup = tr.config, tr.model, tr.model_setup
    assert tr.validation_data_loader is not None and tr.validation_data_loader.concepts == CONCEPTS
    tr.tensorboard = ScalarLog(str(tmp_path / "tb"))

    res2 = tr.validate(global_step=7, collect=True)            # the training batch size, 2
    tr.validation_data_loader.batch_size = 1
    res1 = tr.validate(global_step=9, collect=True)
    tr.validation_data_loader.batch_size = 2
    idx2, l2 = res2["sample_losses"]
    idx1, l1 = res1["sample_losses"]
    print("per-sample losses, batch 2:", l2.tolist(), "batch 1:", l1.tolist())
    assert idx2 == idx1 == [0, 1, 0, 0, 1]                     # bucket 8x8 (samples 0, 2, 4), then 8x16 (1, 3)
    assert torch.isfinite(l2).all() and (l2 > 0).all()
    # (a) the same per-sample losses bit for bit, whatever batch a sample was in
    assert _bits(l2) == _bits(l1)
    assert torch.equal(res2["acc"], res1["acc"])
    if "lora" in case:
        assert lora.per_sample_batch == 0                      # the row numbering does not outlive the pass

    # (b) / (c) each per-concept mean equals the float64 mean of calculate_loss(predict(deterministic=True)) run per
    # sample through the existing autograd path: what the reference's loop would log
    single = LatentCacheDataLoader(str(tmp_path / "cache" / "validation"), 1, dev, prefetch=False, validation=True,
                                   require_mask=masked)
    single.start_next_epoch()
    sums, counts = {}, {}
    per_sample = []
    for b in single.get_data_loader():
        out = setup.predict(model, b, cfg, model.train_progress, deterministic=True)
        loss = setup.calculate_loss(model, b, out, cfg)
        v = loss.item()
        per_sample.append(v)
        c = int(b["concept_index_host"][0])
        sums[c] = sums.get(c, 0) + v
        counts[c] = counts.get(c, 0) + 1
    print("autograd path per sample:", per_sample)
    assert per_sample == [float(x) for x in l2.tolist()]
    expected = [("loss/validation_step/held", sums[0] / counts[0]), ("loss/validation_step/dogs", sums[1] / counts[1]),
                ("loss/validation_step/total_average", (sums[0] + sums[1]) / 5)]
    print("scalars:", res2["scalars"], "expected:", expected)
    assert res2["scalars"] == expected
    assert counts == {0: 3, 1: 2} and res2["acc"][:, 1].tolist() == [3.0, 2.0]

    # (d) the scalars file holds the expected keys at the expected steps
    tr.tensorboard.close()
    rows = [(r["tag"], r["step"], r["value"]) for r in read_scalars(str(tmp_path / "tb"))]
    assert rows == [(t, 7, v) for t, v in expected] + [(t, 9, v) for t, v in expected]


def _run(dev, tmp, validation, graphs):
    tr = _trainer(dev, tmp, "sdxl", validation=validation, steps=4, **LORA)
    assert tr.model.unet_lora.dropout_p == 0.25 and (tr.graphs is not None) == graphs
    losses = []
    step = tr.train_step
    tr.train_step = lambda b, _s=step, _l=losses: (_l.append(_s(b)), _l[-1])[1]
    tr.train(log_every=0)
    tr.tensorboard.close()
    torch.cuda.synchronize()
    if graphs:   # step 0 ran eagerly, step 1 was captured right after a validation pass, steps 2 and 3 replayed it
        assert len(tr.graphs.entries) == 1
    assert tr.model.unet_lora.per_sample_batch == 0
    return torch.stack(losses).cpu(), tr.model.train_store.data.clone().cpu(), tr


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "step-graph"])
def test_lora_dropout_run_is_untouched_by_validation(dev, tmp_path, monkeypatch, graphs):
    monkeypatch.setenv("OTAMD_STEP_GRAPH", "1" if graphs else "0")   # opt-in
    on = _run(dev, tmp_path / "on", True, graphs)
    off = _run(dev, tmp_path / "off", False, graphs)
    print("training losses with validation:", on[0].tolist(), "without:", off[0].tolist())
    assert _bits(on[0]) == _bits(off[0])                                   # training losses, bit for bit
    assert torch.equal(on[1].view(torch.int32), off[1].view(torch.int32))  # the final adapter store
    assert off[2].validation_data_loader is None
    tb = os.path.join(str(tmp_path / "on" / "ws"), "tensorboard")
    rows = read_scalars(os.path.join(tb, os.listdir(tb)[0]))
    val = [(r["tag"], r["step"]) for r in rows if r["tag"].startswith("loss/validation_step/")]
    assert val == [(f"loss/validation_step/{k}", s) for s in range(4) for k in ("held", "dogs", "total_average")]
    vals = [r["value"] for r in rows if r["tag"] == "loss/validation_step/total_average"]
    assert len(set(vals)) == 4                                             # the adapter moved between the passes
    # with dropout on, the pass is still batch-independent: each sample's mask rows restart at 0
    tr = on[2]
    a = tr.validate(collect=True)["sample_losses"][1]
    tr.validation_data_loader.batch_size = 1
    b = tr.validate(collect=True)["sample_losses"][1]
    print("LoRA dropout per-sample losses, batch 2:", a.tolist(), "batch 1:", b.tolist())
    assert _bits(a) == _bits(b)


def test_no_stream_hazards_around_a_validation_pass(dev, tmp_path):
    from onetrainer_amd.module.stream_hazards import StreamHazardCheck
    tr = _trainer(dev, tmp_path, "sdxl", steps=1, **LORA)
    batch = tr.data_loader.batch
    tr.train_step(batch)
    with StreamHazardCheck() as chk:
        tr.train_step(batch)
        res = tr.validate()
        tr.train_step(batch)
    assert res is not None and len(res["scalars"]) == 3
    assert not chk.hazards, chk.report()
