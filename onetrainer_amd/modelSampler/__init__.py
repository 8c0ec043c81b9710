"""Training samples (modules/modelSampler): images drawn from the model while it trains."""
from .StableDiffusionSampler import StableDiffusionSampler, ddim_table  # noqa: F401


def create_model_sampler(model_type: str, model, device):
    """modules/util/create.py create_model_sampler for the families this build samples: SD 1.5 and SDXL.
    None for any other family (FLUX: no samples)."""
    mt = str(model_type)
    if mt.startswith("STABLE_DIFFUSION_XL") or mt.startswith("STABLE_DIFFUSION_15"):
        return StableDiffusionSampler(model, device)
    return None
