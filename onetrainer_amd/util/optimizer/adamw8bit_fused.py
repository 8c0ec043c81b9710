"""Fused 8-bit AdamW (block-wise quantised moments) over a FlatParamStore.

Stands where the reference builds, at modules/util/create.py:553-566,
    bnb.optim.AdamW8bit(params, lr, betas, weight_decay, eps, min_8bit_size, percentile_clipping, block_wise, is_paged)
bitsandbytes (pinned to 0.45.2 by the reference) is not part of the reference tree and was not available to this
build: the contract is the published algorithm (Dettmers et al., "8-bit Optimizers via Block-wise Quantization": two
states, blocks of 256, dynamic-tree codebooks) as restated by tests/_oracle_adamw8bit.py.  No bit- or run-level
comparison with the package was made, and a backup written by it is not claimed to load here, nor the reverse.

Per parameter tensor (a store slot) of at least min_8bit_size elements the state is two uint8 code arrays and two fp32
absmax arrays of ceil(numel / 256) entries; blocks start at the tensor's first element, so none straddles two tensors
or two parameter groups.  A smaller tensor keeps fp32 moments.  `dynamic_map` builds the two codebooks of 256 fp32
values (signed for the first moment, unsigned for the second) once on the host; they are uploaded once and saved with
the state.

One step per group, scalars in Python floats on the host (step counts from 1), each rounded to fp32 once:
    bc1 = 1 - beta1^step;  bc2 = 1 - beta2^step
    step_size = -lr sqrt(bc2) / bc1;  eps_c = sqrt(bc2) eps;  wd_factor = 1 - lr weight_decay
and per block, g after the pending clip:
    m = map1[code1] absmax1;  v = map2[code2] absmax2                  (fp32 tensors read m, v)
    m = beta1 m + (1 - beta1) g;  v = beta2 v + ((1 - beta2) g) g
    p = (p + step_size (m / (sqrt(v) + eps_c))) wd_factor
    absmax1 = max |m|;  absmax2 = max v                                (the block's real elements)
    code = the number of codebook midpoints (map[i] + map[i + 1]) / 2 strictly below m / absmax (v / absmax)
A value on a midpoint takes the lower code; an all-zero block has absmax 0 and the codes of 0.  The first step starts
from the codes of 0 and absmax 0.  One launch (csrc/adamw8bit.hip); step() never synchronises the host.

State dict, per parameter: 'step', 'state1', 'state2' (uint8 codes in the parameter's shape, unpadded), 'absmax1',
'absmax2' (fp32, ceil(numel / 256)), 'qmap1', 'qmap2' (fp32, 256); a tensor below min_8bit_size carries 'step' and
fp32 'state1' / 'state2' only.  The key names are as recalled of bitsandbytes' two-state optimizers and could not be
checked.  Beside 'state' and 'param_groups' the dict holds 'sr_seed'.  load_state_dict restores bit for bit; a
parameter without saved state starts fresh.

Refused by name: beta1 or beta2 outside [0, 1), eps < 0, lr < 0, weight_decay < 0, min_8bit_size < 1 (ValueError);
step_parameter / fused_back_pass (NotImplementedError).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ... import _lib
from ... import kernels as K
from .flat_store import FlatStoreOptimizer

BLOCK = 256


def dynamic_map(signed: bool) -> np.ndarray:
    """The dynamic-tree codebook of 8 bits: 256 ascending fp32 values in [-1, 1] (signed) or [0, 1] (unsigned).
    Seven exponent levels i = 0 .. 6 of scale 10^(i - 6); level i holds the centres of 2^i (signed; 2^(i + 1) unsigned)
    equal cells of [0.1, 1], times the scale, and, signed, their negatives; 0 and 1 complete the set: 2 * 127 + 2 and
    254 + 2 values.  The signed map is symmetric but for 1, which has no negative.  Computed in float64 and rounded to
    fp32 once.  This is bitsandbytes' create_dynamic_map(signed, 7, 8) as recalled; it was not compared with it."""
    data = []
    for i in range(7):
        cells = 2 ** i if signed else 2 ** (i + 1)
        edges = np.linspace(0.1, 1.0, cells + 1, dtype=np.float64)
        means = (edges[:-1] + edges[1:]) / 2.0
        scale = 10.0 ** (i - 6)
        data += (scale * means).tolist()
        if signed:
            data += (-scale * means).tolist()
    data += [0.0, 1.0]
    out = np.sort(np.asarray(data, np.float64)).astype(np.float32)
    assert out.size == 256 and np.all(np.diff(out) > 0)
    return out


def check_hyper(g):
    """the ranges the step takes, refused by name"""
    b1, b2 = (float(b) for b in g["betas"])
    if not 0.0 <= b1 < 1.0:
        raise ValueError(f"ADAMW_8BIT beta1: a coefficient in [0, 1) is required, got {b1!r}")
    if not 0.0 <= b2 < 1.0:
        raise ValueError(f"ADAMW_8BIT beta2: a coefficient in [0, 1) is required, got {b2!r}")
    if not float(g["eps"]) >= 0.0:
        raise ValueError(f"ADAMW_8BIT eps: a non-negative value is required, got {g['eps']!r}")
    if not float(g["lr"]) >= 0.0:
        raise ValueError(f"ADAMW_8BIT lr: a non-negative value is required, got {g['lr']!r}")
    if not float(g["weight_decay"]) >= 0.0:
        raise ValueError(f"ADAMW_8BIT weight_decay: a non-negative value is required, got {g['weight_decay']!r}")


def group_scalars(g, step: int) -> dict:
    """the host part of step `step` (from 1) of group `g`, in Python floats"""
    lr = float(g["lr"])
    beta1, beta2 = (float(b) for b in g["betas"])
    bc1 = 1 - beta1 ** step
    bc2_sqrt = math.sqrt(1 - beta2 ** step)
    return dict(beta1=beta1, one_minus_beta1=1 - beta1, beta2=beta2, one_minus_beta2=1 - beta2,
                eps_c=bc2_sqrt * float(g["eps"]), step_size=-(lr * bc2_sqrt / bc1),
                wd_factor=1 - lr * float(g["weight_decay"]))


class FusedAdamW8bit(FlatStoreOptimizer):
    TUPLE_KEYS = ("betas",)

    def __init__(self, store, param_groups, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 min_8bit_size=4096, stochastic_rounding=True, seed=0):
        if not int(min_8bit_size) >= 1:
            raise ValueError(f"ADAMW_8BIT min_8bit_size: a positive size is required, got {min_8bit_size!r}")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        super().__init__(param_groups, defaults)
        for g in self.param_groups:
            check_hyper(g)
        self._init_store(store)
        self.min_8bit_size = int(min_8bit_size)
        self.stochastic_rounding = bool(stochastic_rounding)
        self.seed = seed
        self.steps = [0 for _ in self.param_groups]
        dev = store.device
        # the segment table: one entry per tensor, in store order
        segs = []
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                s = store.slots[self._name(p)]
                if s.numel > 0:
                    segs.append((s.offset, s.offset + s.numel, gi, s.name))
        segs.sort()
        self._seg_of = {}
        arr = (_lib.A8Seg * max(1, len(segs)))()
        blk = n_abs = n_f32 = 0
        for i, (b, e, gi, name) in enumerate(segs):
            is8 = e - b >= self.min_8bit_size
            nblk = (e - b + BLOCK - 1) // BLOCK
            a = arr[i]
            a.begin, a.end, a.blk0, a.is8bit, a.group = b, e, blk, int(is8), gi
            a.state_off = n_abs if is8 else n_f32
            self._seg_of[name] = (bool(is8), int(a.state_off), nblk)
            blk += nblk
            if is8:
                n_abs += nblk
            else:
                n_f32 += (e - b + 7) // 8 * 8
        self._table_host, self._n_segs = arr, len(segs)
        self._table = self._to_device(arr)
        self.qmap1, self.qmap2 = dynamic_map(True), dynamic_map(False)
        self.zero_code1 = int(np.flatnonzero(self.qmap1 == 0)[0])   # 127; the unsigned map's is 0
        self.zero_code2 = int(np.flatnonzero(self.qmap2 == 0)[0])
        self._qmap = torch.from_numpy(np.concatenate([self.qmap1, self.qmap2])).to(dev)
        self.code1 = torch.full((store.numel,), self.zero_code1, dtype=torch.uint8, device=dev)
        self.code2 = torch.full((store.numel,), self.zero_code2, dtype=torch.uint8, device=dev)
        self.absmax1 = torch.zeros(max(8, n_abs), dtype=torch.float32, device=dev)
        self.absmax2 = torch.zeros_like(self.absmax1)
        self.m32 = torch.zeros(max(8, n_f32), dtype=torch.float32, device=dev)
        self.v32 = torch.zeros_like(self.m32)

    def _groups_struct(self):
        arr = []
        for gi, g in enumerate(self.param_groups):
            check_hyper(g)   # the scheduler and load_state_dict write the groups
            self.steps[gi] += 1
            s = _lib.A8Group()
            for k, v in group_scalars(g, self.steps[gi]).items():
                setattr(s, k, v)
            arr.append(s)
        return arr

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        clip = self._take_clip()
        st = self.store
        st.wait_params()
        if self._n_segs == 0:
            return loss
        p, w = self._pw()
        self._advance_seed()
        K.adamw8bit_step(p, st.grad, w, self.code1, self.code2, self.absmax1, self.absmax2, self.m32, self.v32,
                         self._qmap, self._table, self._table_host, self._n_segs, self._groups_struct(),
                         clip_coef=clip, stochastic_rounding=self.stochastic_rounding and self._bf16_store,
                         seed=self.seed)
        return loss

    def step_parameter(self, p, group, i):
        raise NotImplementedError("ADAMW_8BIT step_parameter (fused_back_pass): the 8-bit step is one launch over the "
                                  "whole store")

    # --- state --------------------------------------------------------------------------------------------------------
    def _views(self, name):
        """the state of one tensor as views of the flat buffers, under the state dict's key names"""
        s = self.store.slots[name]
        if name not in self._seg_of:   # an empty tensor
            return {"state1": self.m32[:0].view(s.shape), "state2": self.v32[:0].view(s.shape)}
        is8, off, nblk = self._seg_of[name]
        if not is8:
            return {"state1": self.m32[off:off + s.numel].view(s.shape), "state2": self.v32[off:off + s.numel].view(s.shape)}
        return {"state1": self._flat(self.code1, name), "state2": self._flat(self.code2, name),
                "absmax1": self.absmax1[off:off + nblk], "absmax2": self.absmax2[off:off + nblk]}

    def _has_state(self, name, gi):
        return self.steps[gi] > 0   # before the first step there is no state, as for any torch optimizer

    def _save_tensor(self, name, gi):
        d = {"step": torch.tensor(float(self.steps[gi])), **super()._save_tensor(name, gi)}
        if "absmax1" in d:
            d["qmap1"], d["qmap2"] = torch.from_numpy(self.qmap1.copy()), torch.from_numpy(self.qmap2.copy())
        return d

    def _group_loaded(self, g):
        check_hyper(g)

    def _load_tensor(self, name, gi, st):
        """bit for bit; a parameter without saved state keeps the codes of 0, absmax 0, fp32 zeros"""
        if ("absmax1" in self._views(name)) != ("absmax1" in st):
            raise ValueError(f"ADAMW_8BIT state of {name}: saved with another min_8bit_size")
        for key in ("qmap1", "qmap2"):
            if key in st and not np.array_equal(torch.as_tensor(st[key]).cpu().numpy(), getattr(self, key)):
                raise ValueError(f"ADAMW_8BIT state of {name}: {key} is not this build's codebook")
        super()._load_tensor(name, gi, st)
        self.steps[gi] = int(float(st["step"]))
