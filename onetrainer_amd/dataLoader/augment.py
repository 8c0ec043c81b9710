"""Concept image augmentations: drawing the parameters on the host, and the table of the device launch.

The reference puts RandomFlip / RandomRotate / RandomBrightness / RandomContrast / RandomSaturation / RandomHue
between ScaleCropImage (with its crop jitter) and EncodeVAE (modules/dataLoader/mixin/DataLoaderText2ImageMixin.py:
186-212), switched per concept by concept.image.enable_random_* / enable_fixed_* (modules/util/config/
ConceptConfig.py:10-72).  Here every (image, variation) gets its parameters from `draw`, a pure function of the
concept's image dict, the concept's seed, the image's index within the concept and the variation number: they do not
depend on bucket grouping, encode_batch, rank or world size.  The pixels are made by csrc/augment.hip
(kernels.image_augment) from an AugEntry table (`pack_table`).

Readings:
  * a key that is ABSENT from the image dict is OFF (an absent image_variations is 1), so a config without these keys
    caches exactly what it cached before; a concepts file written by the reference's UI carries every key and so gets
    the reference's behaviour (its defaults switch enable_crop_jitter and enable_random_flip on);
  * enable_random_*: flip with probability 1/2; the angle uniform in +-random_rotate_max_angle degrees; brightness /
    contrast / saturation factor uniform in [1 - m, 1 + m], floored at 0; hue shift uniform in +-m / 2 turns;
  * enable_fixed_* replaces the draw by its upper end: always flip, +max_angle, 1 + m, +m / 2.
mgds is not in this image: the enable_fixed_* reading and the hue scale are PARITY UNPINNED.
"""
from __future__ import annotations

import ctypes as C
import math
import random

from .aspect_bucketing import crop_offset

NEUTRAL = {"flip": 0, "angle": 0.0, "cos_a": 1.0, "sin_a": 0.0, "brightness": 1.0, "contrast": 1.0,
           "saturation": 1.0, "hue": 0.0}
# (name, strength key): the draw order is fixed and every value is drawn whether its switch is on or not, so
# switching one augmentation does not move the others
_STRENGTH = (("rotate", "random_rotate_max_angle"), ("brightness", "random_brightness_max_strength"),
             ("contrast", "random_contrast_max_strength"), ("saturation", "random_saturation_max_strength"),
             ("hue", "random_hue_max_strength"))
SWITCHES = ("enable_crop_jitter", "enable_random_flip", "enable_fixed_flip") + tuple(
    f"enable_{kind}_{name}" for name, _ in _STRENGTH for kind in ("random", "fixed"))


def variations(concept: dict) -> int:
    """concept.image_variations (ConceptConfig.py:193); absent = 1"""
    v = int(concept.get("image_variations", 1) or 1)
    if v < 1:
        raise ValueError(f"image_variations must be >= 1, got {v}")
    return v


def enabled(image_cfg: dict | None) -> bool:
    """any augmentation switched on in a concept's image dict"""
    return any(bool((image_cfg or {}).get(k)) for k in SWITCHES)


def draw(image_cfg: dict | None, seed: int, index: int, variation: int, scale_res, crop_res) -> dict:
    """-> {"y0", "x0", "flip", "angle" (degrees), "cos_a", "sin_a", "brightness", "contrast", "saturation", "hue"}:
    the geometry and colour fields of one AugEntry"""
    cfg = image_cfg or {}
    rng = random.Random(f"augment/{int(seed)}/{int(index)}/{int(variation)}")
    u = {name: rng.random() for name in ("flip", "rotate", "brightness", "contrast", "saturation", "hue")}
    y0, x0 = crop_offset(scale_res, crop_res, jitter=bool(cfg.get("enable_crop_jitter")), rng=rng)
    out = dict(NEUTRAL, y0=int(y0), x0=int(x0))
    if cfg.get("enable_fixed_flip"):
        out["flip"] = 1
    elif cfg.get("enable_random_flip"):
        out["flip"] = int(u["flip"] < 0.5)
    span = {}
    for name, key in _STRENGTH:
        m = float(cfg.get(key, 0.0) or 0.0)
        if cfg.get(f"enable_fixed_{name}"):
            span[name] = m
        elif cfg.get(f"enable_random_{name}"):
            span[name] = (2.0 * u[name] - 1.0) * m
    if span.get("rotate"):
        a = math.radians(span["rotate"])
        out.update(angle=span["rotate"], cos_a=math.cos(a), sin_a=math.sin(a))
    for name in ("brightness", "contrast", "saturation"):
        if name in span:
            out[name] = max(0.0, 1.0 + span[name])
    if "hue" in span:
        out["hue"] = 0.5 * span["hue"]
    return out


def is_neutral(p: dict) -> bool:
    return all(p[k] == v for k, v in NEUTRAL.items() if k != "angle")


def entry(params: dict, src_off: int, out_off: int, channels: int, scale_res, crop_res, colour: bool = True) -> dict:
    """one table entry (the fields of _lib.AugEntry by name); colour=False (a mask) keeps the geometry only"""
    e = {"src_off": int(src_off), "out_off": int(out_off), "C": int(channels), "Hs": int(scale_res[0]),
         "Ws": int(scale_res[1]), "y0": params["y0"], "x0": params["x0"], "H": int(crop_res[0]),
         "W": int(crop_res[1]), "flip": params["flip"], "cos_a": params["cos_a"], "sin_a": params["sin_a"]}
    for k in ("brightness", "contrast", "saturation", "hue"):
        e[k] = params[k] if colour else NEUTRAL[k]
    return e


def pack_table(entries: list):
    """list of entry dicts -> ctypes array of _lib.AugEntry"""
    from .. import _lib
    tab = (_lib.AugEntry * len(entries))()
    for t, e in zip(tab, entries):
        for name, _ in _lib.AugEntry._fields_:
            setattr(t, name, e[name])
    return tab


def device_augment(entries: list, src, out_numel: int, H: int, W: int):
    """the writer's default augment_fn: entries + flat fp32 source on the device -> flat fp32 output on the device
    (kernels.image_augment).  No fallback: without the library or a device this raises."""
    import torch

    from .. import kernels as K
    tab = pack_table(entries)
    raw = torch.frombuffer(memoryview(tab).cast("B"), dtype=torch.uint8)   # shares tab's memory
    out = torch.empty(int(out_numel), dtype=torch.float32, device=src.device)
    return K.image_augment(raw.to(src.device), tab, len(entries), src, out, H, W)
