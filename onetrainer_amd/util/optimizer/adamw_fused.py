"""Fused multi-tensor AdamW (+ bf16 stochastic rounding) over a FlatParamStore.

Drop-in for what the reference builds at modules/util/create.py:509-534:
    torch.optim.AdamW(params, lr, betas, weight_decay, eps, foreach=False, fused=False)
    patch_adamw(optimizer, stochastic_rounding)          # modules/util/optimizer/adamw_extensions.py:202-205
plus the global clip the trainer applies before step() (modules/trainer/GenericTrainer.py:712-713).
Same optimizer contract: param_groups with 'lr' (LambdaLR drives it), step(),
zero_grad(set_to_none), state_dict()/load_state_dict() (torch AdamW layout: per-param 'step',
'exp_avg', 'exp_avg_sq'), step_parameter(p, group, i).  The arithmetic is one launch over the
flat store (csrc/adamw.hip) instead of ~8 torch ops per tensor.

Overlap (opt-in, OTAMD_OPT_OVERLAP=1; bf16 stores of >= 64 M elements): step() runs the update on
its own stream in 16 parameter-range chunks (layout = forward order) and records an event per chunk
in the store; the next forward's kernels wait only for the chunk holding their weights
(FlatParamStore.wait_params via PRef.w), so the 36 GB optimizer pass (SDXL: ~6 ms of HBM time)
runs beside the compute-bound forward GEMMs instead of in front of them.  Chunked launches give the
bits of one whole-store launch (global element indices for groups and stochastic rounding).
Readers of the parameters outside the train step call store.wait_params() (state_dict, savers and
backups do).  Measured on the SDXL step (MI355X): no gain (151.1 vs 150.6 ms p50) -- a 256x256 GEMM
workgroup takes a whole CU's register file, so the update only time-slices CUs with the forward.
"""
from __future__ import annotations

import math
import os

import torch

from ... import _lib
from ... import kernels as K
from .flat_store import FlatStoreOptimizer


class FusedAdamW(FlatStoreOptimizer):
    def __init__(self, store, param_groups, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 stochastic_rounding=True, seed=0):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=False, capturable=False, differentiable=False, fused=False)
        super().__init__(param_groups, defaults)
        self._init_store(store)
        self.stochastic_rounding = stochastic_rounding
        self.seed = seed
        self.exp_avg = torch.zeros_like(self.master if self.master is not None else store.data)
        self.exp_avg_sq = torch.zeros_like(self.exp_avg)
        self.steps = [0 for _ in self.param_groups]
        # overlapped update: chunk boundaries on tensor boundaries, ~numel / 16 each
        self.overlap = (store.device.type == "cuda" and store.dtype == torch.bfloat16 and store.numel >= (1 << 26)
                        and self.master is None and os.environ.get("OTAMD_OPT_OVERLAP", "0") == "1")
        self._opt_chunks = []
        if self.overlap:
            # chunk ends at 1/256, 1/128, ..., 1/16 of the store, then every 1/16 (tensor boundaries): the forward's first
            # layers wait only for a small first chunk, the rest of the update runs beside them
            ends = [store.numel >> k for k in range(8, 4, -1)] + [store.numel * i // 16 for i in range(1, 17)]
            b, t = 0, 0
            for n in store.order:
                s = store.slots[n]
                e = (s.offset + s.numel + 7) // 8 * 8
                if t < len(ends) and e >= ends[t]:
                    self._opt_chunks.append((b, e))
                    b = e
                    while t < len(ends) and ends[t] <= e:
                        t += 1
            if b < store.numel:
                self._opt_chunks.append((b, store.numel))
            self._stream = torch.cuda.Stream(device=store.device)

    def _groups_struct(self, idx_list, steps=None):
        arr = []
        for k, gi in enumerate(idx_list):
            g = self.param_groups[gi]
            if steps is None:
                self.steps[gi] += 1
                step = self.steps[gi]
            else:
                step = steps[k]
            lr = float(g["lr"])
            beta1, beta2 = g["betas"]
            bc1 = 1 - beta1 ** step
            bc2 = 1 - beta2 ** step
            s = _lib.AdamwGroup()
            s.begin, s.end = self._ranges[gi]
            s.wd_factor = 1 - lr * g["weight_decay"]
            s.one_minus_beta1 = 1 - beta1
            s.beta2 = beta2
            s.one_minus_beta2 = 1 - beta2
            s.bc2_sqrt = math.sqrt(bc2)
            s.eps = g["eps"]
            s.neg_step_size = -(lr / bc1)
            arr.append(s)
        order = sorted(range(len(arr)), key=lambda i: arr[i].begin)
        return [arr[i] for i in order]

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        groups = self._groups_struct(range(len(self.param_groups)))
        clip = self._take_clip()
        st = self.store
        if self.master is not None:
            K.adamw_master(self.master, st.grad, self.exp_avg, self.exp_avg_sq, st.data, groups, clip_coef=clip)
        elif st.dtype == torch.bfloat16:
            self._advance_seed()
            if self.overlap:
                st.wait_params()                                   # a previous update still in flight
                s = self._stream
                s.wait_stream(torch.cuda.current_stream())         # grads reduced, clip coefficient ready
                events = []
                with torch.cuda.stream(s):
                    for b, e in self._opt_chunks:
                        K.adamw_bf16(st.data, st.grad, self.exp_avg, self.exp_avg_sq, groups, clip_coef=clip,
                                     stochastic_rounding=self.stochastic_rounding, seed=self.seed, begin=b, end=e)
                        ev = torch.cuda.Event()
                        ev.record(s)
                        events.append((e, ev))
                st.set_update_events(events)
            else:
                K.adamw_bf16(st.data, st.grad, self.exp_avg, self.exp_avg_sq, groups, clip_coef=clip,
                             stochastic_rounding=self.stochastic_rounding, seed=self.seed)
        else:
            K.adamw_f32(st.data, st.grad, self.exp_avg, self.exp_avg_sq, groups, clip_coef=clip)
        return loss

    def step_parameter(self, p, group, i):
        """fused-back-pass API (adamw_extensions.py:202-205): update one parameter tensor."""
        self.store.wait_params()
        gi = self.param_groups.index(group)
        name = self._name(p)
        s = self.store.slots[name]
        if not hasattr(self, "_pstep"):
            self._pstep = {}
        self._pstep[name] = self._pstep.get(name, self.steps[gi]) + 1
        saved = self._ranges[gi]
        self._ranges[gi] = (s.offset, s.offset + s.numel)
        try:
            groups = self._groups_struct([gi], steps=[self._pstep[name]])
        finally:
            self._ranges[gi] = saved
        st = self.store
        b, e = s.offset // 8 * 8, (s.offset + s.numel + 7) // 8 * 8   # this tensor only (the store pads to 8)
        if self.master is not None:
            K.adamw_master(self.master, st.grad, self.exp_avg, self.exp_avg_sq, st.data, groups, begin=b, end=e)
            return
        K.adamw_bf16(st.data, st.grad, self.exp_avg, self.exp_avg_sq, groups, clip_coef=None,
                     stochastic_rounding=self.stochastic_rounding, seed=self.seed, begin=b, end=e)

    # --- torch AdamW-compatible state: written from the start, as step() needs no first-step flag -----------------
    def _views(self, name):
        return {"exp_avg": self._flat(self.exp_avg, name), "exp_avg_sq": self._flat(self.exp_avg_sq, name)}

    def _save_tensor(self, name, gi):
        return {"step": torch.tensor(float(self.steps[gi])), **super()._save_tensor(name, gi)}

    def _load_tensor(self, name, gi, st):
        super()._load_tensor(name, gi, st)
        self.steps[gi] = int(float(st["step"]))
