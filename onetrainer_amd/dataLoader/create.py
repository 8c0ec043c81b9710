"""create_data_loader: what modules/util/create.py:391-431 + the family data loaders
(StableDiffusionXLBaseDataLoader.py:33-288, DataLoaderText2ImageMixin.py:139-294) do for the
trainer, on this build's latent cache (dataLoader/latent_cache.py).

  * <cache_dir>/index.json present -> read it (LatentCacheDataLoader, ARB batches, rank slices);
  * otherwise enumerate the concepts' images (config.concepts, else the concept_file_name JSON),
    captions from the sample's .txt next to the image (prompt_source 'sample'), the concept's
    prompt file ('concept') or the file name ('filename'); tokenize with the checkpoint's own
    tokenizers (<base_model>/tokenizer[_2], transformers); encode images with the HIP VAE encoder and
    text with the HIP text encoders the model carries (attach_cache_encoders, loaded by the model
    loader with the base weights), write the cache on rank 0, then read it;
  * under masked_training every image is paired with <stem>-masklabel.png (DataLoaderText2ImageMixin.py:62,
    85-86; all ones when the file is missing), cached as latent_mask and required from the cache.  The
    per-concept mask augmentations (RandomCircularMaskShrink / RandomMaskRotateCrop, :122-135) are refused.
  * for the mask-input (inpainting) model types (util/model_type.py) the mask is loaded whether masked_training is on
    or off (StableDiffusionBaseDataLoader.py:80,99), and the cache also holds latent_conditioning_image -- the VAE
    mean of image * (1 - mask) (mgds GenerateMaskedConditioningImage, :236-246; K.masked_conditioning on the
    encoder's own input) -- and one blank latent per bucket shape; unmasked_probability (:270-276, :287-288) is
    drawn per step by the model setup, not here.  custom_conditioning_image is refused.
  * every training row carries its concept's image dict, seed, index within the concept, image_variations and
    loss_weight (concept_extras): the writer augments on the device and caches the variations (dataLoader/augment.py,
    csrc/augment.hip); the validation cache gets no augmentation and one variation.
mgds itself is not in this image: enumeration and captions follow the reference's
ConceptConfig fields; the bucket list is dataLoader/aspect_bucketing.py (parity unpinned).
"""
from __future__ import annotations

import json
import os

import torch

from ..util.config.plain import plain, value
from ..util.model_type import has_mask_input
from .latent_cache import INDEX, LatentCacheDataLoader, LatentCacheWriter, default_bucketing

IMAGE_EXT = (".png", ".jpg", ".jpeg", ".webp", ".bmp", ".tif", ".tiff")


def cache_ready(config) -> bool:
    return os.path.isfile(os.path.join(plain(config).cache_dir, INDEX))


def has_concepts(config) -> bool:
    cfg = plain(config)
    return bool(cfg.concepts) or bool(cfg.concept_file_name and os.path.isfile(cfg.concept_file_name))


def _family(model_type: str) -> str:
    if model_type.startswith("FLUX"):
        return "flux"
    if model_type.startswith("STABLE_DIFFUSION_XL"):
        return "sdxl"
    return "sd15"


def attach_cache_encoders(model, config, device) -> None:
    """VAE encoder + caching text encoders on the model, before the model loader runs (it fills
    model.vae_encoder / text_encoder_1 / text_encoder_2 from the base checkpoint)."""
    from ..module import text_encoder as TE
    from ..module import vae as V
    cfg = plain(config)
    fam = _family(cfg.model_type)
    vcfg = {"sdxl": V.sdxl_vae_config, "sd15": V.sd15_vae_config, "flux": V.flux_vae_config}[fam]
    model.vae_encoder = V.AutoencoderKLEncoder(vcfg(), device, seed=0)
    model.text_encoder_1 = TE.CLIPTextEncoder(TE.clip_l_config(), device)
    if fam == "sdxl":
        model.text_encoder_2 = TE.CLIPTextEncoder(TE.clip_bigg_config(), device)
    elif fam == "flux":
        model.text_encoder_2 = TE.T5TextEncoder(TE.t5_xxl_config(), device)


VALIDATION_DIR = "validation"   # the held-out set's own latent cache: <cache_dir>/validation


def validation_cache_dir(config) -> str:
    return os.path.join(plain(config).cache_dir, VALIDATION_DIR)


def validation_cache_ready(config) -> bool:
    return os.path.isfile(os.path.join(validation_cache_dir(config), INDEX))


def is_validation_concept(concept: dict) -> bool:
    """ConceptConfig.type == VALIDATION, or the legacy key `validation_concept` that the reference migrates to it
    (modules/util/config/ConceptConfig.py:167-168)"""
    t = concept.get("type")
    if t is not None:
        return str(value(t)) == "VALIDATION"
    return bool(concept.get("validation_concept", False))


def _concepts(cfg, validation: bool = False) -> list:
    """the enabled concepts of one side of the split (DataLoaderMgdsMixin.py:29-30: the validation concepts or all
    the others); the split applies whether or not `validation` is on, so a held-out image is never trained on"""
    concepts = cfg.concepts
    if not concepts:
        path = cfg.concept_file_name
        if not path or not os.path.isfile(path):
            raise FileNotFoundError(f"no concepts: config.concepts is empty and concept file {path!r} is missing")
        with open(path) as f:
            concepts = json.load(f)
    out = []
    for c in concepts:
        c = c.to_dict() if hasattr(c, "to_dict") else dict(c)
        if c.get("enabled", True) and is_validation_concept(c) == validation:
            out.append(c)
    return out


def validation_concepts(config) -> list[dict]:
    """{name, path, seed} of every enabled validation concept; a sample's concept index is its position here.
    Without concepts configured (a run on a ready cache) there are none."""
    cfg = plain(config)
    if not has_concepts(cfg):
        return []
    return [{"name": c.get("name", "") or "", "path": c.get("path", ""), "seed": int(c.get("seed", 0) or 0)}
            for c in _concepts(cfg, validation=True)]


def validation_labels(concepts: list[dict]) -> list[str]:
    """the scalar label of every validation concept (GenericTrainer.py:358-370): its name, else the basename of its
    path; a label already taken by a concept of another seed gets the suffix (1), (2), ...; concepts of one seed
    share the first one's label (the reference accumulates by seed).  Concepts are visited in index order."""
    seed_to_label: dict = {}
    label_to_seed: dict = {}
    for c in concepts:
        seed = c["seed"]
        label = c["name"] if c["name"] else os.path.basename(c["path"])
        if label in label_to_seed and label_to_seed[label] != seed:
            suffix = 1
            new = f"{label}({suffix})"
            while new in label_to_seed and label_to_seed[new] != seed:
                suffix += 1
                new = f"{label}({suffix})"
            label = new
        if seed not in seed_to_label:
            seed_to_label[seed] = label
            label_to_seed[label] = seed
    return [seed_to_label[c["seed"]] for c in concepts]


def _caption(img_path: str, concept: dict) -> str:
    text = concept.get("text") or {}
    src = text.get("prompt_source", "sample")
    if src == "filename":
        return os.path.splitext(os.path.basename(img_path))[0]
    if src == "concept":
        p = text.get("prompt_path", "")
        if p and os.path.isfile(p):
            with open(p) as f:
                return f.readline().strip()
        return ""
    txt = os.path.splitext(img_path)[0] + ".txt"
    if os.path.isfile(txt):
        with open(txt) as f:
            return f.readline().strip()
    return ""


MASK_POSTFIX = "-masklabel.png"
MASK_AUGMENTATIONS = ("enable_random_circular_mask_shrink", "enable_random_mask_rotate_crop")


def mask_path(img_path: str) -> str | None:
    """<stem>-masklabel.png next to the image (DataLoaderText2ImageMixin.py:62), or None when there is none:
    the sample then trains with an all-ones mask (GenerateImageLike color 255, :85)."""
    p = os.path.splitext(img_path)[0] + MASK_POSTFIX
    return p if os.path.isfile(p) else None


def wants_mask(cfg) -> bool:
    """the samples carry a mask: masked training, or a model type that takes the mask as an input"""
    return bool(getattr(cfg, "masked_training", False)) or has_mask_input(getattr(cfg, "model_type", None))


def check_conditioning(cfg) -> None:
    if getattr(cfg, "custom_conditioning_image", False):
        raise NotImplementedError("custom_conditioning_image: conditioning images from <stem>-condlabel files are "
                                  "not built (an inpainting model's conditioning image is image * (1 - mask))")


def enumerate_samples(config) -> list[tuple]:
    """(image path, caption) for every enabled training (non-validation) concept (mgds CollectPaths + caption
    loading); under masked_training or a mask-input model type (image path, caption, mask path or None).  A
    -masklabel.png is never listed as an image."""
    cfg = plain(config)
    return [s for s, _ in _enumerate(cfg, _concepts(cfg))]


def enumerate_validation_samples(config) -> list[dict]:
    """the held-out set: for every image of every enabled validation concept {"sample": the tuple
    enumerate_samples gives, "concept_index": the concept's position among the enabled validation concepts,
    "name" / "path" / "seed": the concept's}"""
    cfg = plain(config)
    concepts = validation_concepts(cfg)
    return [{"sample": s, "concept_index": i, **concepts[i]}
            for s, i in _enumerate(cfg, _concepts(cfg, validation=True))]


def _enumerate(cfg, concepts: list) -> list[tuple]:
    """(sample tuple, position of its concept in `concepts`)"""
    check_conditioning(cfg)
    masked = wants_mask(cfg)
    out = []
    for ci, c in enumerate(concepts):
        if masked:
            on = [k for k in MASK_AUGMENTATIONS if (c.get("image") or {}).get(k)]
            if on:
                raise NotImplementedError(f"concept {c.get('name') or c['path']!r}: mask augmentation {on[0]} is not "
                                          "built (masks are cached as they are)")
        root = c["path"]
        walk = os.walk(root) if c.get("include_subdirectories", False) else [(root, [], os.listdir(root))]
        for d, _, files in walk:
            for fn in sorted(files):
                if fn.lower().endswith(IMAGE_EXT) and not fn.lower().endswith(MASK_POSTFIX):
                    p = os.path.join(d, fn)
                    out.append(((p, _caption(p, c), mask_path(p)) if masked else (p, _caption(p, c)), ci))
    return out


def concept_extras(concept: dict, index: int) -> dict:
    """what a cached row takes from its concept beside the image and the caption: the augmentation switches
    (concept.image), the seed and the image's index within the concept that key the draws, image_variations, and
    loss_weight (ConceptConfig.py:131-138, 189-197).  Absent keys are off / 1 / 1."""
    from . import augment as A
    lw = concept.get("loss_weight")
    return {"augment": {"image": dict(concept.get("image") or {}), "seed": int(concept.get("seed", 0) or 0),
                        "index": int(index), "variations": A.variations(concept)},
            "loss_weight": 1.0 if lw is None else float(lw)}


def _tokenizers(cfg):
    from transformers import CLIPTokenizer
    base = cfg.base_model_name
    fam = _family(cfg.model_type)
    toks = [CLIPTokenizer.from_pretrained(os.path.join(base, "tokenizer"))]
    if fam == "sdxl":
        toks.append(CLIPTokenizer.from_pretrained(os.path.join(base, "tokenizer_2")))
    elif fam == "flux":
        from transformers import AutoTokenizer   # T5TokenizerFast (tokenizer.json) or the sentencepiece T5Tokenizer
        toks.append(AutoTokenizer.from_pretrained(os.path.join(base, "tokenizer_2")))
    return toks


def build_cache(config, model, device, rank: int = 0, validation: bool = False) -> int:
    """the training set into cache_dir, or (validation) the held-out set into <cache_dir>/validation with every
    index entry carrying its concept index and the index the concepts' name / path / seed"""
    from PIL import Image

    from ..module import text_encoder as TE
    cfg = plain(config)
    fam = _family(cfg.model_type)
    concept_of = extras = None
    if validation:   # no augmentation, one variation: held-out losses stay comparable
        held_out = enumerate_validation_samples(cfg)
        samples = [v["sample"] for v in held_out]
        concept_of = [v["concept_index"] for v in held_out]
    else:
        concepts = _concepts(cfg)
        listed = _enumerate(cfg, concepts)
        samples = [s for s, _ in listed]
        extras, seen = [], {}
        for _, ci in listed:   # the image's index within its concept keys its augmentation draws
            extras.append(concept_extras(concepts[ci], seen.get(ci, 0)))
            seen[ci] = seen.get(ci, 0) + 1
    if not samples:
        raise FileNotFoundError(f"no {'validation' if validation else 'training'} images found in the configured "
                                "concepts")
    toks = _tokenizers(cfg)

    def ids(tok, caption):
        return tok(caption, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids[0]

    def row(sample, tokens):
        r = {"image": Image.open(sample[0]), "tokens": tokens}
        if len(sample) > 2:   # masked training / mask input: the -masklabel.png, one channel (missing = all ones)
            r["mask"] = Image.open(sample[2]).convert("L") if sample[2] else Image.new("L", r["image"].size, 255)
        return r

    if fam in ("sdxl", "flux"):
        enc_text = TE.encode_sdxl_text if fam == "sdxl" else TE.encode_flux_text
        text_fn = lambda t: enc_text(model.text_encoder_1, model.text_encoder_2,  # noqa: E731
                                     t["tokens_1"], t["tokens_2"])
        rows = (row(s, {"tokens_1": ids(toks[0], s[1]), "tokens_2": ids(toks[1], s[1])}) for s in samples)
    else:
        text_fn = lambda t: TE.encode_sd15_text(model.text_encoder_1, t["tokens_1"])  # noqa: E731
        rows = (row(s, {"tokens_1": ids(toks[0], s[1])}) for s in samples)
    # a generator: each file is opened (and, once decoded, closed) inside the writer's loop, so a concept
    # folder larger than the open-file limit caches
    if validation:
        rows = ({**r, "concept_index": ci} for r, ci in zip(rows, concept_of))
    else:
        rows = ({**r, **x} for r, x in zip(rows, extras))
    cond_fn = None
    if has_mask_input(cfg.model_type):   # image * (1 - mask) on the encoder's own input, then the same encoder
        from .. import kernels as K
        from ..module.vae import PAD_IN
        cond_fn = lambda im, m: model.vae_encoder.encode_nhwc(  # noqa: E731
            K.masked_conditioning(K.image_to_nhwc(im.contiguous(), 2.0, -1.0, PAD_IN), m.contiguous()))
    writer = LatentCacheWriter(lambda im: model.vae_encoder.encode(im),
                               validation_cache_dir(cfg) if validation else cfg.cache_dir, default_bucketing(cfg),
                               device, rank=rank, text_fn=text_fn,
                               concepts=validation_concepts(cfg) if validation else None, cond_fn=cond_fn)
    return writer.write(rows)


def validation_cache_needed(config) -> bool:
    """`validation` is on, the concepts hold at least one validation concept, and its cache is not written yet"""
    cfg = plain(config)
    return bool(getattr(cfg, "validation", False)) and not validation_cache_ready(cfg) and bool(validation_concepts(cfg))


def create_validation_data_loader(config, device, rank: int = 0, world: int = 1):
    """the held-out set's loader (create_data_loader builds its cache beside the training one), or None when
    `validation` is off or there is no validation concept: the pass is then skipped, as the reference returns early
    on an empty loader (GenericTrainer.py:324-325)"""
    cfg = plain(config)
    if not getattr(cfg, "validation", False) or not validation_cache_ready(cfg):
        return None
    return LatentCacheDataLoader(validation_cache_dir(cfg), cfg.batch_size, device, seed=0, rank=rank, world=world,
                                 require_mask=wants_mask(cfg), validation=True,
                                 require_conditioning=has_mask_input(getattr(cfg, "model_type", None)))


def create_data_loader(config, model, device, rank: int = 0, world: int = 1):
    cfg = plain(config)
    check_conditioning(cfg)
    need_train, need_validation = not cache_ready(cfg), validation_cache_needed(cfg)
    if need_train or need_validation:
        if getattr(model, "vae_encoder", None) is None:
            raise RuntimeError("no latent cache at cache_dir and no VAE encoder on the model "
                               "(GenericTrainer.start attaches one when the cache must be built)")
        if need_train:
            build_cache(cfg, model, device, rank)
        if need_validation:
            build_cache(cfg, model, device, rank, validation=True)
        if world > 1:
            torch.distributed.barrier()
        keep = ("text_encoder_1", "text_encoder_2") if getattr(model, "keep_text_encoders", False) else ()
        for attr in ("vae_encoder", "text_encoder_1", "text_encoder_2"):   # caching done: free the encoders
            if hasattr(model, attr) and attr not in keep:   # (the sampler keeps the text encoders for its prompts)
                setattr(model, attr, None)
        if torch.cuda.is_available():
            torch.cuda.empty_cache()
    return LatentCacheDataLoader(cfg.cache_dir, cfg.batch_size, device, seed=0, rank=rank, world=world,
                                 require_mask=wants_mask(cfg),
                                 require_conditioning=has_mask_input(getattr(cfg, "model_type", None)))
