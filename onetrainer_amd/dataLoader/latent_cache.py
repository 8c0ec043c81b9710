"""Latent cache writer / reader with aspect-ratio buckets.

Replaces what the reference's mgds pipeline does before and around the steps
(modules/dataLoader/StableDiffusionXLBaseDataLoader.py:65-209 + DataLoaderText2ImageMixin.py:139-294):
  CalcAspect -> AspectBucketing -> ScaleCropImage -> RescaleImageChannels -> EncodeVAE ->
  SampleVAEDistribution(mean) -> DiskCache -> AspectBatchSorting -> OutputPipelineModule.
The mgds on-disk cache format is not pinned (mgds is not in this image); this build's format:
  <cache_dir>/index.json            {"version": 1, "samples": [{"file", "crop_resolution"}, ...]}
                                    a sample with image variations adds "variations": [file of variation 1, 2, ...],
                                    a concept loss weight other than 1 adds "loss_weight"
                                    the held-out set's cache (<cache_dir>/validation) adds "concept_index" to every
                                    entry and "concepts": [{"name", "path", "seed"}, ...] to the index
  <cache_dir>/<i:08d>.safetensors   latent_image [h, w, C] fp32 NHWC (VAE latent_dist.mean, unscaled; C = 4, FLUX.1 16),
                                    original_resolution / crop_offset / crop_resolution int64 [2],
                                    optional cached text states (text_encoder_*_hidden_state, pooled),
                                    optional latent_mask [1, h, w] fp32 in [0, 1] (masked training, mask-input models),
                                    optional latent_conditioning_image [h, w, C] fp32 NHWC (mask-input models): the VAE
                                    latent_dist.mean of image * (1 - mask), unscaled.
  <cache_dir>/blank_<H>x<W>.safetensors   mask-input models, once per bucket shape: latent_blank [h, w, C] fp32, the
                                    mean latent of a fully masked H x W image (all zero in the encoder's [-1, 1]);
                                    the index names them: "blank": {"<H>x<W>": file}.
  <cache_dir>/<i:08d>.v<v>.safetensors   variation v >= 1 of sample i (concept.image_variations): only what differs
                                    from variation 0 -- latent_image, crop_offset, latent_mask,
                                    latent_conditioning_image.  Text states are
                                    cached once per image, in the sample's own file.
Images are scaled / cropped on the host (data-loader work, as in mgds' worker threads), encoded on
the GPU by the HIP VAE in same-resolution batches, and written by rank 0 only.
A sample's mask (masked training: <stem>-masklabel.png, one channel) takes the scale and crop of its image, then
the downscale to the latent grid (0.125x for the 8x VAEs, StableDiffusionXLBaseDataLoader.py:70) with the same
antialiased bilinear resize and a clamp to [0, 1].  mgds' exact ScaleImage filter is unpinned (mgds is not in this image).
A sample of a concept with image_variations > 1 or any image augmentation switched on (dataLoader/augment.py) is
scaled on the host, uploaded once uncropped, and cropped / flipped / rotated / colour-shifted into all its variations
on the device (csrc/augment.hip) in front of the encoder; its mask rides through the same launch with the same crop,
flip and rotation.  Every other sample takes the host crop, and its files and index entry are what they always were.
The reader takes variation (epoch mod V) of a sample with V variations (mgds cycles them in order; its exact rule is
unpinned) and emits the concept's loss_weight.
The reader yields the reference batch contract (DataLoaderText2ImageMixin._output_modules_from_out_names),
one resolution per GLOBAL batch, each DP rank taking its slice (aspect_bucketing.rank_slice),
with one batch prefetched on a host thread into pinned memory.
"""
from __future__ import annotations

import json
import os
import queue
import threading

import torch
import torch.nn.functional as F
from safetensors.torch import load_file, save_file

from . import augment as A
from .aspect_bucketing import AspectBucketing, aspect_batches, crop_offset, rank_slice

INDEX = "index.json"


def _to_chw01(img) -> torch.Tensor:
    """PIL image / HWC uint8 tensor / CHW float in [0, 1] -> CHW float32 [0, 1]."""
    if hasattr(img, "convert"):   # PIL
        import numpy as np
        img = torch.from_numpy(np.asarray(img.convert("RGB")).copy())
    if img.dtype == torch.uint8:
        img = img.permute(2, 0, 1).float() / 255.0 if img.shape[-1] == 3 else img.float() / 255.0
    return img.float().contiguous()


def _to_mask01(mask) -> torch.Tensor:
    """PIL image (taken as 'L') / HW uint8 / [1, H, W] float in [0, 1] -> [1, H, W] float32"""
    if hasattr(mask, "convert"):   # PIL
        import numpy as np
        mask = torch.from_numpy(np.asarray(mask.convert("L")).copy())
    mask = torch.as_tensor(mask)
    if mask.dtype == torch.uint8:
        mask = mask.float() / 255.0
    if mask.dim() == 2:
        mask = mask[None]
    if mask.dim() != 3 or mask.shape[0] != 1:
        raise ValueError(f"mask: one channel expected, got shape {tuple(mask.shape)}")
    return mask.float().contiguous()


def latent_mask(mask: torch.Tensor, scale_res, crop_res, offset, size) -> torch.Tensor:
    """[1, H, W] mask -> [1, h, w] latent mask: the image's scale_crop, then the downscale to the latent grid
    `size` -- mgds ScaleImage(factor 0.125) for the 8x VAEs (StableDiffusionXLBaseDataLoader.py:70) -- as the same
    antialiased bilinear resize, clamped to [0, 1]."""
    return mask_to_latent_grid(scale_crop(mask, scale_res, crop_res, offset), size)


def mask_to_latent_grid(m: torch.Tensor, size) -> torch.Tensor:
    """[1, H, W] cropped mask -> [1, h, w] on the latent grid `size`"""
    m = F.interpolate(m[None], size=tuple(size), mode="bilinear", antialias=True, align_corners=False)[0]
    return m.clamp(0.0, 1.0).contiguous()


def scale_only(img: torch.Tensor, scale_res) -> torch.Tensor:
    """the resize of scale_crop without the crop: what the device augmentations crop from"""
    x = F.interpolate(img[None], size=tuple(scale_res), mode="bilinear", antialias=True, align_corners=False)[0]
    return x.clamp(0.0, 1.0).contiguous()


def blank_file(res) -> str:
    return f"blank_{int(res[0])}x{int(res[1])}.safetensors"


def variation_file(i: int, v: int) -> str:
    return f"{i:08d}.safetensors" if v == 0 else f"{i:08d}.v{v}.safetensors"


def scale_crop(img: torch.Tensor, scale_res, crop_res, offset):
    """mgds ScaleCropImage: bilinear (antialiased) resize to scale_res, then crop crop_res at offset."""
    x = F.interpolate(img[None], size=tuple(scale_res), mode="bilinear", antialias=True, align_corners=False)[0]
    y0, x0 = offset
    return x[:, y0:y0 + crop_res[0], x0:x0 + crop_res[1]].clamp(0.0, 1.0).contiguous()


class LatentCacheWriter:
    def __init__(self, encode_fn, cache_dir: str, bucketing, device, encode_batch: int = 8, rank: int = 0,
                 text_fn=None, concepts=None, augment_fn=None, cond_fn=None):
        """encode_fn: [B, 3, H, W] fp32 [0, 1] on `device` -> latent NHWC fp32 [B, H/8, W/8, C]
        (module.vae.AutoencoderKLEncoder.encode).  text_fn (optional): {name: int64 token ids [B, T]}
        on `device` -> {cache key: [B, ...]} (module.text_encoder.encode_sdxl_text & co.), applied to
        samples that carry "tokens" -- the reference's text-encoder caching step.
        augment_fn(entries, src, out_numel, H, W) -> flat fp32 on src's device: the image augmentations of the rows
        that ask for them (default: the HIP kernel, augment.device_augment); never called for the other rows.
        cond_fn (mask-input models): ([B, 3, H, W] fp32 [0, 1], [B, 1, H, W] fp32 mask) on `device` -> the latent of
        the conditioning image image * (1 - mask), NHWC fp32 like encode_fn's.  With it every sample carries a mask
        (all ones when it brings none), every record a latent_conditioning_image, and every bucket shape a blank."""
        self.encode_fn, self.cache_dir, self.bucketing = encode_fn, cache_dir, bucketing
        self.device, self.encode_batch, self.rank = torch.device(device), encode_batch, rank
        self.text_fn = text_fn
        self.concepts = concepts   # the validation cache: {name, path, seed} of the concepts its samples index
        self.augment_fn = augment_fn or A.device_augment
        self.cond_fn = cond_fn

    def _augmented(self, rows, res):
        """rows that carry augmentation parameters (p[10], one dict per variation): each scaled image (and mask) is
        uploaded once, every variation is made by one augment_fn call and encoded.  -> {(sample, variation): latent},
        {(sample, variation): cropped mask [1, H, W]}, {(sample, variation): conditioning latent} (cond_fn only)"""
        H, W = res
        planes, entries, masks, keys, off = [], [], [], [], 0
        for p in rows:
            img = scale_only(p[1], p[3])
            src_off, off = off, off + img.numel()
            planes.append(img.reshape(-1))
            m_off = None
            if p[8] is not None:
                m = scale_only(p[8], p[3])
                m_off, off = off, off + m.numel()
                planes.append(m.reshape(-1))
            for v, prm in enumerate(p[10]):
                keys.append((p[0], v))
                entries.append(A.entry(prm, src_off, len(entries) * 3 * H * W, 3, p[3], res))
                if m_off is not None:   # the image's crop, flip and rotation; no colour stage
                    masks.append(((p[0], v), prm, m_off, p[3]))
        n = len(entries)
        for j, (_, prm, m_off, scale_res) in enumerate(masks):
            entries.append(A.entry(prm, m_off, (n * 3 + j) * H * W, 1, scale_res, res, colour=False))
        out = self.augment_fn(entries, torch.cat(planes).to(self.device), (n * 3 + len(masks)) * H * W, H, W)
        imgs = out[:n * 3 * H * W].view(n, 3, H, W)
        lat = torch.cat([self.encode_fn(imgs[a:a + self.encode_batch]).float().cpu()
                         for a in range(0, n, self.encode_batch)])
        cropped_dev = out[n * 3 * H * W:].view(len(masks), 1, H, W)
        conds = {}
        if self.cond_fn is not None:   # every row has a mask here, so masks and entries share their order
            cl = torch.cat([self.cond_fn(imgs[a:a + self.encode_batch], cropped_dev[a:a + self.encode_batch])
                            .float().cpu() for a in range(0, n, self.encode_batch)])
            conds = dict(zip(keys, cl))
        cropped = cropped_dev.float().cpu()
        return dict(zip(keys, lat)), {m[0]: c for m, c in zip(masks, cropped)}, conds

    def write(self, samples):
        """samples: iterable of dicts {"image": PIL / tensor, optional "text": {name: tensor}, optional "mask":
        PIL 'L' image / HW uint8 / [1, H, W] float in [0, 1], cached as latent_mask, optional "augment": {"image": the
        concept's image dict, "seed": the concept's, "index": the image's within its concept, "variations"}, optional
        "loss_weight": the concept's}.
        Returns the number of cached samples."""
        os.makedirs(self.cache_dir, exist_ok=True)
        prepared = []
        for i, s in enumerate(samples):
            img = _to_chw01(s["image"])
            h, w = img.shape[1], img.shape[2]
            scale_res, crop_res = self.bucketing.bucket_for(h, w)
            off = crop_offset(scale_res, crop_res)
            mask = _to_mask01(s["mask"]) if s.get("mask") is not None else None
            if mask is None and self.cond_fn is not None:
                mask = torch.ones((1, h, w), dtype=torch.float32)
            aug, params = s.get("augment"), None
            if aug and (int(aug.get("variations", 1)) > 1 or A.enabled(aug.get("image"))):
                params = [A.draw(aug.get("image"), aug.get("seed", 0), aug.get("index", i), v, scale_res, crop_res)
                          for v in range(int(aug.get("variations", 1)))]
            prepared.append((i, img, (h, w), scale_res, crop_res, off, dict(s.get("text") or {}), s.get("tokens"),
                             mask, s.get("concept_index"), params, float(s.get("loss_weight", 1.0))))
        by_res: dict = {}
        for p in prepared:
            by_res.setdefault(tuple(p[4]), []).append(p)
        index = [None] * len(prepared)
        blanks = {}
        for res in sorted(by_res):
            group = by_res[res]
            if self.cond_fn is not None:   # the latent of a fully masked image: 0.5 in [0, 1] is 0 in [-1, 1]
                blank = self.encode_fn(torch.full((1, 3) + tuple(res), 0.5, device=self.device)).float().cpu()[0]
                blanks[f"{res[0]}x{res[1]}"] = blank_file(res)
                if self.rank == 0:
                    save_file({"latent_blank": blank.contiguous()}, os.path.join(self.cache_dir, blank_file(res)))
            for k in range(0, len(group), self.encode_batch):
                chunk = group[k:k + self.encode_batch]
                plain = [p for p in chunk if p[10] is None]
                lats, crops, conds = {}, {}, {}
                if plain:
                    imgs = torch.stack([scale_crop(p[1], p[3], p[4], p[5]) for p in plain]).to(self.device)
                    lats = {(p[0], 0): l_ for p, l_ in zip(plain, self.encode_fn(imgs).float().cpu())}
                    if self.cond_fn is not None:
                        ms = torch.stack([scale_crop(p[8], p[3], p[4], p[5]) for p in plain]).to(self.device)
                        conds = {(p[0], 0): c for p, c in zip(plain, self.cond_fn(imgs, ms).float().cpu())}
                if len(plain) < len(chunk):
                    more, crops, more_conds = self._augmented([p for p in chunk if p[10] is not None], res)
                    lats.update(more)
                    conds.update(more_conds)
                tok = [p for p in chunk if p[7] is not None]
                if tok and self.text_fn is not None:
                    names = list(tok[0][7])
                    states = self.text_fn({n: torch.stack([torch.as_tensor(p[7][n], dtype=torch.int64)
                                                           for p in tok]).to(self.device) for n in names})
                    for j, p in enumerate(tok):
                        p[6].update({k2: v[j].to(torch.bfloat16) for k2, v in states.items()})
                for p in chunk:
                    i = p[0]
                    l_ = lats[(i, 0)]
                    offset = p[5] if p[10] is None else (p[10][0]["y0"], p[10][0]["x0"])
                    rec = {"latent_image": l_.contiguous(),
                           "original_resolution": torch.tensor(p[2], dtype=torch.int64),
                           "crop_offset": torch.tensor(offset, dtype=torch.int64),
                           "crop_resolution": torch.tensor(p[4], dtype=torch.int64)}
                    rec.update({k2: v.detach().cpu().contiguous() for k2, v in p[6].items()})
                    if p[8] is not None:   # on the latent's own grid: crop_res / 8 for the 8x VAEs
                        rec["latent_mask"] = (latent_mask(p[8], p[3], p[4], p[5], l_.shape[:2]) if p[10] is None
                                              else mask_to_latent_grid(crops[(i, 0)], l_.shape[:2]))
                    if self.cond_fn is not None:
                        rec["latent_conditioning_image"] = conds[(i, 0)].contiguous()
                    fn = variation_file(i, 0)
                    if self.rank == 0:
                        save_file(rec, os.path.join(self.cache_dir, fn))
                    index[i] = {"file": fn, "crop_resolution": list(p[4])}
                    for v in range(1, len(p[10] or ())):   # only what differs from variation 0
                        lv = lats[(i, v)]
                        var = {"latent_image": lv.contiguous(),
                               "crop_offset": torch.tensor((p[10][v]["y0"], p[10][v]["x0"]), dtype=torch.int64)}
                        if p[8] is not None:
                            var["latent_mask"] = mask_to_latent_grid(crops[(i, v)], lv.shape[:2])
                        if self.cond_fn is not None:
                            var["latent_conditioning_image"] = conds[(i, v)].contiguous()
                        if self.rank == 0:
                            save_file(var, os.path.join(self.cache_dir, variation_file(i, v)))
                        index[i].setdefault("variations", []).append(variation_file(i, v))
                    if p[11] != 1.0:
                        index[i]["loss_weight"] = p[11]
                    if p[9] is not None:
                        index[i]["concept_index"] = int(p[9])
        if self.rank == 0:
            with open(os.path.join(self.cache_dir, INDEX), "w") as f:
                json.dump({"version": 1, "samples": index,
                           **({} if self.concepts is None else {"concepts": self.concepts}),
                           **({"blank": blanks} if self.cond_fn is not None else {})}, f)
        return len(index)


class LatentCacheDataLoader:
    """Reader in the reference's BaseDataLoader shape: get_data_set().start_next_epoch() /
    approximate_length(), get_data_loader() iterable of batches on `device`."""

    def __init__(self, cache_dir: str, batch_size: int, device, seed: int = 0, rank: int = 0, world: int = 1,
                 text_defaults: dict | None = None, prefetch: bool = True, require_mask: bool = False,
                 validation: bool = False, require_conditioning: bool = False):
        """require_mask (masked training, mask-input models): batches carry latent_mask [B, 1, h, w]; a cached record
        without one is an error.  Otherwise a cached mask is not emitted.
        require_conditioning (mask-input models): batches carry latent_conditioning_image [B, C, h, w] (a view of
        NHWC storage, like latent_image) and latent_blank [h, w, C], the blank latent of the batch's bucket shape; a
        cache without either is an error.
        validation (the held-out set's cache): every pass emits every sample exactly once in a fixed order -- the
        buckets in ascending resolution, cache index order within a bucket, no shuffle, nothing dropped, a short
        last batch run short -- and each batch carries concept_index int32 [B] on the device (and
        concept_index_host, the same on the host, for the accumulate launcher's range check)."""
        with open(os.path.join(cache_dir, INDEX)) as f:
            meta = json.load(f)
        self.index = meta["samples"]
        self.validation = validation
        self.concepts = meta.get("concepts", [])   # {name, path, seed} per concept index (validation caches)
        self.cache_dir, self.batch_size, self.device = cache_dir, batch_size, torch.device(device)
        self.seed, self.rank, self.world, self.epoch = seed, rank, world, -1
        self.variation_epoch = None
        self.text_defaults = text_defaults or {}
        self.prefetch = prefetch
        self.require_mask = require_mask
        self.require_conditioning = require_conditioning
        self.blank_files = meta.get("blank") or {}
        self._blanks: dict = {}
        self._batches = []

    # BaseDataLoader.get_data_set() -> MGDS-like
    def get_data_set(self):
        return self

    def _validation_batches(self):
        groups: dict = {}
        for i, s in enumerate(self.index):
            groups.setdefault(tuple(s["crop_resolution"]), []).append(i)
        n = self.batch_size * self.world
        return [idx[k:k + n] for r in sorted(groups) for idx in (groups[r],) for k in range(0, len(idx), n)]

    def start_next_epoch(self):
        self.epoch += 1
        if self.validation:
            self._batches = self._validation_batches()
            return
        res = [tuple(s["crop_resolution"]) for s in self.index]
        self._batches = aspect_batches(res, self.batch_size * self.world, self.seed, self.epoch)

    def approximate_length(self):
        if self.validation:
            return len(self._validation_batches())
        if not self._batches:
            res = [tuple(s["crop_resolution"]) for s in self.index]
            return len(aspect_batches(res, self.batch_size * self.world, self.seed, 0))
        return len(self._batches)

    def set_variation_epoch(self, epoch: int):
        """the trainer's own (restored) epoch number: a resumed run reads the variations the uninterrupted run
        would have read.  Without it the loader's epoch count is used."""
        self.variation_epoch = int(epoch)

    def variation_files(self, i: int, epoch: int | None = None) -> list:
        """the files sample i is read from in `epoch` (default: the current one): its own, then -- for variation
        epoch mod V >= 1 of a sample with V variations -- the variation's, whose keys replace the first's"""
        entry = self.index[i]
        more = entry.get("variations") or []
        if epoch is None:
            epoch = self.epoch if self.variation_epoch is None else self.variation_epoch
        v = max(epoch, 0) % (1 + len(more))
        return [entry["file"]] + ([more[v - 1]] if v else [])

    def _record(self, i: int) -> dict:
        rec = {}
        for fn in self.variation_files(i):
            rec.update(load_file(os.path.join(self.cache_dir, fn)))
        return rec

    def _load(self, idx):
        recs = [self._record(i) for i in idx]
        b = len(recs)
        out = {"latent_image": torch.stack([r["latent_image"] for r in recs])}
        for k in ("original_resolution", "crop_offset", "crop_resolution"):
            v = torch.stack([r[k] for r in recs])
            out[k] = (v[:, 0], v[:, 1])
        text_keys = {k for r in recs for k in r if k.startswith("text_encoder")}
        for k in text_keys:
            out[k] = torch.stack([r[k] for r in recs])
        for k, v in self.text_defaults.items():
            if k not in out:
                out[k] = v.expand(b, *v.shape).contiguous()
        if self.require_mask:
            if any("latent_mask" not in r for r in recs):
                raise ValueError("masked_training: cache was built without masks; delete cache_dir "
                                 f"({self.cache_dir}) so it is rebuilt with them")
            out["latent_mask"] = torch.stack([r["latent_mask"] for r in recs])
        if self.require_conditioning:
            res = "x".join(str(int(v)) for v in self.index[idx[0]]["crop_resolution"])
            if any("latent_conditioning_image" not in r for r in recs) or res not in self.blank_files:
                raise ValueError("mask-input model type: cache was built without conditioning latents; delete "
                                 f"cache_dir ({self.cache_dir}) so it is rebuilt with them")
            out["latent_conditioning_image"] = torch.stack([r["latent_conditioning_image"] for r in recs])
            if res not in self._blanks:
                self._blanks[res] = load_file(os.path.join(self.cache_dir, self.blank_files[res]))["latent_blank"]
            out["latent_blank"] = self._blanks[res].clone()
        # the concept's loss_weight (ConceptConfig.py:197); an index without the key (every older cache) gives 1
        out["loss_weight"] = torch.tensor([float(self.index[i].get("loss_weight", 1.0)) for i in idx],
                                          dtype=torch.float32)
        if self.validation:
            out["concept_index"] = torch.tensor([int(self.index[i]["concept_index"]) for i in idx], dtype=torch.int32)
        if torch.cuda.is_available():
            for k, v in list(out.items()):
                if isinstance(v, torch.Tensor):
                    out[k] = v.pin_memory()
        return out

    def _to_device(self, host):
        dev = {}
        if self.validation:   # before the upload: a pinned host copy stays behind for the launcher's range check
            dev["concept_index_host"] = host["concept_index"]
        for k, v in host.items():
            if isinstance(v, tuple):
                dev[k] = tuple(t.to(self.device, non_blocking=True) for t in v)
            else:
                dev[k] = v.to(self.device, non_blocking=True)
        # the reference's [B, C, h, w] contract, as a view of the cached channels-last (NHWC) storage
        dev["latent_image"] = dev["latent_image"].permute(0, 3, 1, 2)
        if "latent_conditioning_image" in dev:
            dev["latent_conditioning_image"] = dev["latent_conditioning_image"].permute(0, 3, 1, 2)
        dev["concept_type"] = ["VALIDATION" if self.validation else "STANDARD"] * dev["latent_image"].shape[0]
        return dev

    def get_data_loader(self):
        if not self._batches:
            self.start_next_epoch()
        if self.validation:   # a short last batch: the first ranks take whole slices, the rest what is left (or none)
            bs = self.batch_size
            mine = [b[self.rank * bs:(self.rank + 1) * bs] for b in self._batches]
            mine = [b for b in mine if b]
        else:
            mine = [rank_slice(b, self.rank, self.world) for b in self._batches]
        if not self.prefetch:
            for idx in mine:
                yield self._to_device(self._load(idx))
            return
        q: queue.Queue = queue.Queue(maxsize=2)

        def worker():
            try:
                for idx in mine:
                    q.put(self._load(idx))
                q.put(None)
            except Exception as e:   # a failed load (e.g. a mask-less cache) is raised by the consumer
                q.put(e)

        t = threading.Thread(target=worker, daemon=True)
        t.start()
        while True:
            host = q.get()
            if host is None:
                break
            if isinstance(host, Exception):
                t.join()
                raise host
            yield self._to_device(host)
        t.join()


def default_bucketing(config):
    from .aspect_bucketing import SingleAspectCalculation, quantization_for
    target = config.resolution_hw()[0]
    if getattr(config, "aspect_ratio_bucketing", True):
        return AspectBucketing(target, quantization_for(config.model_type))
    return SingleAspectCalculation(target)
