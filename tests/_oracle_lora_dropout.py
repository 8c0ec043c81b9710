"""Host oracle of the LoRA dropout mask (csrc/lora_dropout.hip), on the host Philox4x32-10 of _diffusion_edges.py.

One Philox call per row and per group of 4 consecutive columns: Wq = ceil(width / 4), call index
q = site_id * 2^40 + (row0 + m) * Wq + quad, counter (lo32(q), hi32(q), 6, TAG_DROP), key = the 64-bit seed; word k of
the call belongs to column 4 quad + k.  An element is kept iff word >= thr, thr = floor(p * 2^32) (integers only: p = 0
keeps everything, p = 1 gives thr = 2^32 and keeps nothing); a kept element becomes bf16_rne(float(t) * scale) with
scale = fp32(1 / (1 - p)), a dropped one +0."""
import math

import numpy as np
import torch

from _diffusion_edges import philox4x32_10

STREAM_DROP, TAG_DROP = 6, 0x64726f70
_S32, _M32 = np.uint64(32), np.uint64(0xFFFFFFFF)


def consts(p: float):
    """(thr, scale as the fp32 value the kernel receives)"""
    thr = int(math.floor(float(p) * 4294967296.0))
    scale = float(np.float32(1.0 / (1.0 - p))) if p < 1 else math.inf
    return thr, scale


def words(seed: int, site_id: int, row0: int, M: int, width: int) -> np.ndarray:
    """the 32-bit word of every element, uint64 [M, width]"""
    Wq = (width + 3) // 4
    rows = np.uint64(row0) + np.arange(M, dtype=np.uint64)
    q = (np.uint64(site_id) << np.uint64(40)) + rows[:, None] * np.uint64(Wq) + np.arange(Wq, dtype=np.uint64)[None, :]
    seed = np.array(seed & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    w = philox4x32_10((q & _M32, q >> _S32, STREAM_DROP, TAG_DROP), (seed & _M32, seed >> _S32))
    return np.stack([np.asarray(x, dtype=np.uint64) for x in w], axis=-1).reshape(M, 4 * Wq)[:, :width]


def keep_mask(seed: int, site_id: int, row0: int, M: int, width: int, p: float) -> np.ndarray:
    """bool [M, width]: True where the element is kept"""
    return words(seed, site_id, row0, M, width) >= np.uint64(consts(p)[0])


def apply(t: torch.Tensor, keep, p: float) -> torch.Tensor:
    """the kernel's output for bf16 t (any device) under the mask `keep` (numpy bool of t's shape)"""
    k = torch.from_numpy(np.ascontiguousarray(keep)).to(t.device).reshape(t.shape)
    scaled = (t.float() * consts(p)[1]).to(torch.bfloat16)   # fp32 product, one rne rounding: the kernel's
    return torch.where(k, scaled, torch.zeros_like(scaled))
