"""Fused Prodigy (Mishchenko and Defazio: the learning rate is estimated, configurations run it at lr 1.0) over a
FlatParamStore.

Stands where the reference builds, at modules/util/create.py:863-881,
    prodigyopt.Prodigy(params, lr, betas, beta3, eps, weight_decay, decouple, use_bias_correction, safeguard_warmup,
                       d0, d_coef, growth_rate, fsdp_in_use, slice_p)
The prodigyopt package is imported there but is not part of the reference tree and was not available to this build:
the contract is the published Prodigy step, restated in float64 with the fp32 roundings named by
tests/_oracle_prodigy.py.  No bit- or run-level comparison with prodigyopt was made.

One step, with g the gradient after the pending clip, the scalars d, d_max, d_numerator, k and the per-element states
m (exp_avg), v (exp_avg_sq), s and p0 (the parameters at the first step):
    dlr = d lr bc,  bc = sqrt(1 - beta2^(k+1)) / (1 - beta1^(k+1)) under use_bias_correction, else 1
    lr == 0: nothing changes
    g += weight_decay p                                  (coupled form: decouple False)
    num = sum g (p0 - p);  m = beta1 m + d (1 - beta1) g;  v = beta2 v + d^2 (1 - beta2) g g
    s = beta3 s + (d / d0) dlr g   ((d / d0) d under safeguard_warmup);  den = sum |s|
    d_numerator = beta3 d_numerator + (d / d0) dlr num;  d_denom = den;  den == 0: stop (no update, k stays)
    d_hat = d_coef d_numerator / d_denom;  d == d0: d = max(d, d_hat);  d_max = max(d_max, d_hat)
    d = min(d_max, d growth_rate)
    p += (-weight_decay dlr) p  (decoupled form);  p -= dlr m / (sqrt(v) + d eps)   (new d, old dlr; beta1 == 0: d g for m)
    k += 1
It is three launches (csrc/prodigy.hip: accumulate over the grad-norm chunk table, finalize, apply) with the scalars
in a device block: step() never synchronises the host with the device.  d_state() reads the block (blocking);
param_groups[i]["d"] is refreshed from an asynchronous copy to pinned memory and is at most one step old.

Same optimizer contract as the siblings (param_groups with 'lr', step, zero_grad, clip_grad_norm_ of the base class;
state_dict / load_state_dict: per parameter 'step', 's', 'p0', 'exp_avg' (absent when beta1 == 0), 'exp_avg_sq'; the
groups carry d, d0, d_max, d_numerator, d_denom, d_hat, k and the hyper-parameters; 'sr_seed').

This build's choices, recorded in DESIGN.md:
  * m, v, s and p0 are fp32 whatever the parameter dtype.
  * a tensor that received no gradient is stepped with a zero gradient (the store zeroes it), as the siblings do.
  * under data parallel the gradients in the store are already all-reduced, so every rank computes the same d with
    no further collective.
Refused by name: parameter groups whose learning rates or hyper-parameters differ, slice_p != 1, fsdp_in_use,
fused_back_pass and step_parameter (NotImplementedError: the step needs sums over the whole store); eps <= 0,
d0 <= 0, a beta outside [0, 1) (ValueError).
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from ... import _lib
from ... import kernels as K
from .flat_store import FlatStoreOptimizer

CHUNK = 1 << 16   # elements of a NormChunk at most (FlatStoreOptimizer._init_store)
HYPER_KEYS = ("betas", "beta3", "eps", "weight_decay", "decouple", "use_bias_correction", "safeguard_warmup", "d0",
              "d_coef", "growth_rate")
STATE_KEYS = ("d", "d_max", "d_numerator", "d_denom", "d_hat", "k")


def resolve_beta3(beta3, beta2) -> float:
    return math.sqrt(beta2) if beta3 is None else float(beta3)


def check_hyper(g):
    """the ranges csrc/prodigy.hip takes, refused by name"""
    b1, b2 = (float(b) for b in g["betas"])
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"PRODIGY betas: two coefficients in [0, 1) are required, got {g['betas']!r}")
    if g["beta3"] is not None and not 0.0 <= float(g["beta3"]) <= 1.0:
        raise ValueError(f"PRODIGY beta3: a coefficient in [0, 1] is required, got {g['beta3']!r}")
    if not float(g["eps"]) > 0.0:
        raise ValueError(f"PRODIGY eps: a positive value is required, got {g['eps']!r}")
    if not float(g["d0"]) > 0.0:
        raise ValueError(f"PRODIGY d0: a positive value is required, got {g['d0']!r}")


def check_chunks(chunks, n_chunks, numel):
    """every range of the chunk table the accumulate kernel walks (it trusts the table)"""
    for i in range(n_chunks):
        c = chunks[i]
        if not (0 <= c.begin < c.end <= numel and c.begin % 8 == 0 and c.end - c.begin <= CHUNK):
            raise ValueError("prodigy chunk table: a chunk outside the store, unaligned or too long")


class FusedProdigy(FlatStoreOptimizer):
    TUPLE_KEYS = ("betas",)

    def __init__(self, store, param_groups, lr=1.0, betas=(0.9, 0.999), beta3=None, eps=1e-8, weight_decay=0.0,
                 decouple=True, use_bias_correction=False, safeguard_warmup=False, d0=1e-6, d_coef=1.0,
                 growth_rate=float("inf"), stochastic_rounding=False, seed=0):
        defaults = dict(lr=lr, betas=tuple(betas), beta3=beta3, eps=eps, weight_decay=weight_decay,
                        decouple=bool(decouple), use_bias_correction=bool(use_bias_correction),
                        safeguard_warmup=bool(safeguard_warmup), d=d0, d0=d0, d_max=d0, d_numerator=0.0, d_denom=0.0,
                        d_hat=d0, d_coef=d_coef, growth_rate=growth_rate, k=0)
        super().__init__(param_groups, defaults)
        first = self.param_groups[0]
        for g in self.param_groups:
            check_hyper(g)
            for key in HYPER_KEYS:
                if g[key] != first[key]:
                    raise NotImplementedError(f"PRODIGY {key}: parameter groups that differ in it are not supported "
                                              "(d is one estimate for the whole store)")
        self._common_lr()
        self._init_store(store)
        if sum(len(g["params"]) for g in self.param_groups) != len(store.order):
            raise ValueError("PRODIGY: the parameter groups must hold every tensor of the store")
        raw = bytes(self._chunks.cpu().numpy().tobytes())
        check_chunks((_lib.NormChunk * self._n_chunks).from_buffer_copy(raw[:self._n_chunks * C.sizeof(_lib.NormChunk)]),
                     self._n_chunks, store.numel)
        self.stochastic_rounding = bool(stochastic_rounding)
        self.seed = seed
        dev = store.device

        def f32():
            return torch.zeros(store.numel, dtype=torch.float32, device=dev)

        self.exp_avg = f32() if float(first["betas"][0]) > 0.0 else None
        self.exp_avg_sq, self.s, self.p0 = f32(), f32(), f32()
        self._p0_set = False   # p0 is captured by the first step that runs
        self._chunk_num = torch.zeros(max(1, self._n_chunks), dtype=torch.float64, device=dev)
        self._chunk_den = torch.zeros(max(1, self._n_chunks), dtype=torch.float64, device=dev)
        self._state = torch.zeros(C.sizeof(_lib.ProdigyState) // 8, dtype=torch.float64, device=dev)
        self._write_state(first)
        # the asynchronous read-back of d: two pinned blocks, each with the event recorded after its copy
        self._host = [[torch.zeros(self._state.numel(), dtype=torch.float64).pin_memory(), torch.cuda.Event(), False]
                      for _ in range(2)]
        self._next_host = 0

    # --- the device scalars -------------------------------------------------------------------------------------------
    def _write_state(self, g):
        vals = [float(g[k]) for k in ("d", "d_max", "d_numerator", "d_denom", "d_hat")] + [0.0, float(g["k"]), 0.0]
        self._state.copy_(torch.tensor(vals, dtype=torch.float64))

    def d_state(self) -> dict:
        """the device scalars, read back now (blocks until the enqueued steps have run)"""
        vals = self._state.cpu().tolist()
        s = _lib.ProdigyState(*vals)
        out = {k: getattr(s, k) for k in ("d", "d_max", "d_numerator", "d_denom", "d_hat", "dlr")}
        out["k"], out["skip"] = int(s.k), bool(s.skip)
        return out

    def _poll(self):
        """param_groups[i]['d'] <- the newest d whose copy has completed; never blocks"""
        for i in (self._next_host, 1 - self._next_host):   # oldest first
            slot = self._host[i]
            if slot[2] and slot[1].query():
                slot[2] = False
                d = float(slot[0][0])
                for g in self.param_groups:
                    g["d"] = d

    def _enqueue_d_copy(self):
        self._poll()
        slot = self._host[self._next_host]
        if slot[2]:   # its last copy is still in flight: this step's d is picked up by a later copy
            return
        slot[0].copy_(self._state, non_blocking=True)
        slot[1].record()
        slot[2] = True
        self._next_host = 1 - self._next_host

    # --- the optimizer ------------------------------------------------------------------------------------------------
    def _common_lr(self) -> float:
        lrs = {float(g["lr"]) for g in self.param_groups}
        if len(lrs) != 1:
            raise NotImplementedError(f"PRODIGY lr: parameter groups with different learning rates {sorted(lrs)} are "
                                      "not supported (d is one estimate for the whole store)")
        return lrs.pop()

    def _hyper(self, lr) -> _lib.ProdigyHyper:
        g = self.param_groups[0]
        h = _lib.ProdigyHyper()
        h.lr = lr
        h.beta1, h.beta2 = (float(b) for b in g["betas"])
        h.beta3 = resolve_beta3(g["beta3"], h.beta2)
        h.eps, h.weight_decay, h.d0 = float(g["eps"]), float(g["weight_decay"]), float(g["d0"])
        h.d_coef, h.growth_rate = float(g["d_coef"]), float(g["growth_rate"])
        h.decouple, h.use_bias_correction = int(bool(g["decouple"])), int(bool(g["use_bias_correction"]))
        h.safeguard_warmup = int(bool(g["safeguard_warmup"]))
        return h

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        self._poll()
        lr = self._common_lr()
        clip = self._take_clip()
        if lr == 0.0:   # a complete no-op: no state, no k, no p0
            return loss
        st = self.store
        st.wait_params()
        p, w = self._pw()
        self._advance_seed()
        h = self._hyper(lr)
        K.prodigy_accumulate(p, st.grad, w, self.p0, self.exp_avg, self.exp_avg_sq, self.s, self._chunks,
                             self._n_chunks, self._chunk_num, self._chunk_den, self._state, h, clip_coef=clip,
                             capture_p0=not self._p0_set)
        self._p0_set = True
        K.prodigy_finalize(self._chunk_num, self._chunk_den, self._n_chunks, self._state, h)
        K.prodigy_apply(p, st.grad, w, self.exp_avg, self.exp_avg_sq, self._state, h, clip_coef=clip,
                        stochastic_rounding=self.stochastic_rounding and self._bf16_store, seed=self.seed)
        self._enqueue_d_copy()
        return loss

    def step_parameter(self, p, group, i):
        raise NotImplementedError("PRODIGY step_parameter (fused_back_pass): the step needs sums over the whole store")

    # --- state: nothing before the first step, as for any torch optimizer --------------------------------------------
    def _views(self, name):
        v = {"s": self._flat(self.s, name), "p0": self._flat(self.p0, name),
             "exp_avg_sq": self._flat(self.exp_avg_sq, name)}
        if self.exp_avg is not None:
            v["exp_avg"] = self._flat(self.exp_avg, name)
        return v

    def _has_state(self, name, gi):
        return self._p0_set

    def _save_tensor(self, name, gi):
        return {"step": self.param_groups[gi]["k"], **super()._save_tensor(name, gi)}

    def state_dict(self):
        self.store.wait_params()
        ds = self.d_state()
        for g in self.param_groups:
            g.update({k: ds[k] for k in STATE_KEYS})
        sd = super().state_dict()
        for gd in sd["param_groups"]:
            gd["sr_seed"] = sd["sr_seed"]   # the groups carry the seed too
        return sd

    def _saved_seed(self, sd):
        """the top-level seed, else the first group's that has one"""
        seeds = [sd.get("sr_seed")] + [g.get("sr_seed") for g in sd["param_groups"]]
        return next((seed for seed in seeds if seed is not None), None)

    def _load_tensor(self, name, gi, st):
        super()._load_tensor(name, gi, st)
        self._p0_set = True

    def _loaded(self, fresh):
        if self._p0_set:   # a tensor without saved state starts here: its p0 is its current value
            for name in fresh:
                self._views(name)["p0"].copy_(self.store.value(name))
        self._write_state(self.param_groups[0])
