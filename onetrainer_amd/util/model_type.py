"""What the build asks of a model type name (modules/util/enum/ModelType.py)."""
from __future__ import annotations

# ModelType.has_mask_input and has_conditioning_image_input, for the types this build trains: the UNet input is
# [noised latent | mask | conditioning latent], 9 channels
MASK_INPUT_TYPES = ("STABLE_DIFFUSION_15_INPAINTING", "STABLE_DIFFUSION_XL_10_BASE_INPAINTING")


def has_mask_input(model_type) -> bool:
    return str(getattr(model_type, "value", model_type)) in MASK_INPUT_TYPES


def unet_in_channels(model_type) -> int:
    return 9 if has_mask_input(model_type) else 4
