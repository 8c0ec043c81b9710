"""SampleConfig subset (modules/util/config/SampleConfig.py:47-69, the reference's defaults) for the training
samples of SD 1.5 / SDXL, loadable from the reference's own sample JSON (`training_samples/samples.json`) or the
inline `samples` list of a train config.  Unknown keys are kept in `extra` and ignored.

What this build's sampler does not do is refused by name when the sample configs are read (check_supported), not in
the middle of a run: schedulers other than DDIM, sample_inpainting, frames > 1, and any enabled sample of a mask-input
(inpainting) model type.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, field, fields

from ..model_type import has_mask_input

IMAGE_FORMATS = {"JPG": (".jpg", "JPEG"), "PNG": (".png", "PNG"), "WEBP": (".webp", "WEBP")}   # ImageFormat.py


@dataclass
class SampleConfig:
    enabled: bool = True
    prompt: str = ""
    negative_prompt: str = ""
    height: int = 512
    width: int = 512
    frames: int = 1
    length: float = 10.0
    seed: int = 42
    random_seed: bool = False
    diffusion_steps: int = 20
    cfg_scale: float = 7.0
    noise_scheduler: str = "DDIM"
    text_encoder_1_layer_skip: int = 0
    text_encoder_2_layer_skip: int = 0
    force_last_timestep: bool = False
    sample_inpainting: bool = False
    base_image_path: str = ""
    mask_image_path: str = ""
    extra: dict = field(default_factory=dict)

    @staticmethod
    def default_values() -> "SampleConfig":
        return SampleConfig()

    def from_dict(self, d: dict) -> "SampleConfig":
        names = {f.name for f in fields(self)} - {"extra"}
        for k, v in d.items():
            if k in names:
                setattr(self, k, getattr(v, "value", v) if k == "noise_scheduler" else v)
            else:
                self.extra[k] = v
        self.noise_scheduler = str(self.noise_scheduler)
        return self

    def to_dict(self) -> dict:
        d = {f.name: getattr(self, f.name) for f in fields(self) if f.name != "extra"}
        d.update(self.extra)
        return d

    def from_train_config(self, train_config) -> "SampleConfig":
        """SampleConfig.from_train_config (SampleConfig.py:34-41): the layer skips and the terminal-SNR switch are
        the train config's"""
        self.text_encoder_1_layer_skip = int(getattr(train_config, "text_encoder_layer_skip", 0) or 0)
        self.text_encoder_2_layer_skip = int(getattr(train_config, "text_encoder_2_layer_skip", 0) or 0)
        extra = getattr(train_config, "extra", None) or {}
        self.force_last_timestep = bool(getattr(train_config, "rescale_noise_scheduler_to_zero_terminal_snr",
                                                extra.get("rescale_noise_scheduler_to_zero_terminal_snr", False)))
        return self

    def check_supported(self) -> "SampleConfig":
        if self.noise_scheduler != "DDIM":
            raise NotImplementedError(f"sample noise_scheduler {self.noise_scheduler}: only DDIM is built")
        if self.sample_inpainting:
            raise NotImplementedError("sample_inpainting: inpainting samples are not built")
        if int(self.frames) > 1:
            raise NotImplementedError(f"sample frames={self.frames}: only single images (frames 1) are built")
        if int(self.diffusion_steps) < 1:
            raise ValueError(f"sample diffusion_steps={self.diffusion_steps}")
        return self


def as_sample_config(s) -> SampleConfig:
    """a SampleConfig of this build, a dict, or the reference's SampleConfig object (to_dict)"""
    if isinstance(s, SampleConfig):
        return s
    d = s.to_dict() if hasattr(s, "to_dict") else dict(s)
    return SampleConfig().from_dict(d)


def read_sample_configs(train_config) -> list[SampleConfig]:
    """the run's sample definitions (GenericTrainer.py:277-285): the inline `samples` list wins, else the JSON file at
    sample_definition_file_name; a missing file means no samples.  Every enabled entry is checked here."""
    samples = getattr(train_config, "samples", None)
    if samples is None:
        path = getattr(train_config, "sample_definition_file_name", "") or ""
        if not os.path.isfile(path):
            return []
        with open(path) as f:
            samples = json.load(f)
    out = [as_sample_config(s) for s in samples]
    for s in out:
        if s.enabled:
            s.check_supported()
    model_type = getattr(train_config, "model_type", None)
    if has_mask_input(model_type) and any(s.enabled for s in out):
        raise NotImplementedError(f"samples for model type {getattr(model_type, 'value', model_type)}: the sampler "
                                  "has no mask and conditioning-image input; disable the sample definitions")
    return out


def safe_filename(text: str, max_length: int | None = 32) -> str:
    """path_util.safe_filename (modules/util/path_util.py:6-21) with spaces allowed"""
    text = "".join(c for c in text if c.isalnum() or c in " ._-#").strip()
    return (text[:max_length] if max_length is not None else text).strip()
