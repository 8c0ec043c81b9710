"""Fused schedule-free AdamW (Defazio et al., "The Road Less Scheduled") over a FlatParamStore.

Stands where the reference builds, at modules/util/create.py:752-767,
    schedulefree.AdamWScheduleFree(params, lr, betas, weight_decay, eps, warmup_steps, r, weight_lr_power, foreach)
The schedulefree package (pinned to 1.4.0 by the reference) is not part of the reference tree and was not available to
this build: the contract is the non-foreach path of AdamWScheduleFree.step as restated, in float64 with the fp32
roundings named, by tests/_oracle_schedule_free.py.  No bit- or run-level comparison with the package was made.

The store holds the gradient point y while training; z (the base iterate) and v (exp_avg_sq) are fp32 states.  The
weights to save are the average x, which is not stored: eval() turns the store into x, train() back into y.

One step per group, all scalars in Python floats on the host (k starts at 0):
    sched = (k + 1) / warmup_steps if k < warmup_steps else 1;  bc2 = 1 - beta2^(k+1)
    lr = group lr * sched;  lr_max = max(lr, lr_max);  weight = (k + 1)^r lr_max^weight_lr_power
    weight_sum += weight;  ckp1 = weight / weight_sum (0 when weight_sum == 0);  a_y = lr (beta1 (1 - ckp1) - 1)
and per element, g after the pending clip:
    v = beta2 v + (1 - beta2) g g;  gn = g / (sqrt(v / bc2) + eps) + weight_decay y
    y = y + ckp1 (z - y);  y = y + a_y gn;  z = z - lr gn;        then k += 1
One launch (csrc/schedule_free.hip); z = y is taken inside the first step's launch.  step() never synchronises the host.

eval():  p = p + (1 - 1/beta1) (z - p), after keeping the bits of y in a buffer; train() puts those bits back, so a
backup or a save in the middle of a run leaves the rest of the run bit-identical to an uninterrupted one.  Without
saved bits (after load_state_dict of a state saved in eval mode, which is what a backup holds) train() computes
p = p + (1 - beta1) (z - p).  Each is a no-op in its own mode; step() in eval mode raises RuntimeError, as the package
does.  Like the package's, a new optimizer starts with train_mode False: call train() before the first step (the
trainer does).

State dict in the package's layout: per parameter 'z', 'exp_avg_sq' (after the first step); per group k, train_mode,
weight_sum, lr_max, scheduled_lr, warmup_steps, r, weight_lr_power, betas, eps, weight_decay, lr, foreach; 'sr_seed'.

Refused by name: beta1 outside (0, 1), beta2 outside [0, 1), eps < 0, lr < 0, warmup_steps < 0 (ValueError);
step_parameter / fused_back_pass (NotImplementedError).  foreach=True is accepted: one launch either way.
"""
from __future__ import annotations

import torch

from ... import _lib
from ... import kernels as K
from .flat_store import FlatStoreOptimizer

GROUP_KEYS = ("k", "train_mode", "weight_sum", "lr_max", "scheduled_lr", "warmup_steps", "r", "weight_lr_power", "betas",
              "eps", "weight_decay", "lr", "foreach")


def check_hyper(g):
    """the ranges the step and the mode switches take, refused by name"""
    b1, b2 = (float(b) for b in g["betas"])
    if not 0.0 < b1 < 1.0:
        raise ValueError(f"SCHEDULE_FREE_ADAMW beta1: a coefficient in (0, 1) is required (eval() divides by it), "
                         f"got {b1!r}")
    if not 0.0 <= b2 < 1.0:
        raise ValueError(f"SCHEDULE_FREE_ADAMW beta2: a coefficient in [0, 1) is required, got {b2!r}")
    if not float(g["eps"]) >= 0.0:
        raise ValueError(f"SCHEDULE_FREE_ADAMW eps: a non-negative value is required, got {g['eps']!r}")
    if not float(g["lr"]) >= 0.0:
        raise ValueError(f"SCHEDULE_FREE_ADAMW lr: a non-negative value is required, got {g['lr']!r}")
    if not g["warmup_steps"] >= 0:
        raise ValueError(f"SCHEDULE_FREE_ADAMW warmup_steps: a non-negative value is required, "
                         f"got {g['warmup_steps']!r}")


def group_scalars(g) -> dict:
    """the host part of one step of group `g` (a param_group dict, updated in place except k): returns lr, ckp1, a_y,
    bc2 of the step in Python floats"""
    k = int(g["k"])
    beta1, beta2 = (float(b) for b in g["betas"])
    warmup = g["warmup_steps"]
    sched = (k + 1) / warmup if k < warmup else 1.0
    bc2 = 1 - beta2 ** (k + 1)
    lr = float(g["lr"]) * sched
    g["scheduled_lr"] = lr
    lr_max = g["lr_max"] = max(lr, g["lr_max"])
    weight = ((k + 1) ** g["r"]) * (lr_max ** g["weight_lr_power"])
    weight_sum = g["weight_sum"] = g["weight_sum"] + weight
    ckp1 = weight / weight_sum if weight_sum != 0 else 0.0
    return dict(lr=lr, ckp1=ckp1, a_y=lr * (beta1 * (1 - ckp1) - 1), bc2=bc2)


class FusedScheduleFreeAdamW(FlatStoreOptimizer):
    TUPLE_KEYS = ("betas",)

    def __init__(self, store, param_groups, lr=0.0025, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, warmup_steps=0,
                 r=0.0, weight_lr_power=2.0, foreach=False, stochastic_rounding=True, seed=0):
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, r=r, k=0, warmup_steps=warmup_steps, train_mode=False,
                        weight_sum=0.0, lr_max=-1.0, scheduled_lr=0.0, weight_lr_power=weight_lr_power,
                        weight_decay=weight_decay, foreach=bool(foreach))
        super().__init__(param_groups, defaults)
        for g in self.param_groups:
            check_hyper(g)
        self._init_store(store)
        self.stochastic_rounding = bool(stochastic_rounding)
        self.seed = seed
        self.z = torch.zeros(store.numel, dtype=torch.float32, device=store.device)
        self.exp_avg_sq = torch.zeros_like(self.z)
        self._z_set = False    # z = y is taken by the first step that runs
        self._y_saved = None   # eval(): the bits of y (the master, or the store data), for train()

    # --- the two modes' flag ------------------------------------------------------------------------------------------
    @property
    def train_mode(self) -> bool:
        return bool(self.param_groups[0]["train_mode"])

    def _set_mode(self, mode: bool):
        for g in self.param_groups:
            g["train_mode"] = mode

    # --- the optimizer ------------------------------------------------------------------------------------------------
    def _groups_struct(self):
        arr = []
        for gi, g in enumerate(self.param_groups):
            check_hyper(g)   # the scheduler and load_state_dict write the groups
            sc = group_scalars(g)
            beta2 = float(g["betas"][1])
            s = _lib.SfGroup()
            s.begin, s.end = self._ranges[gi]
            s.lr, s.a_y, s.ckp1 = sc["lr"], sc["a_y"], sc["ckp1"]
            s.beta2, s.one_minus_beta2, s.inv_bc2 = beta2, 1 - beta2, 1 / sc["bc2"]
            s.eps, s.weight_decay = float(g["eps"]), float(g["weight_decay"])
            s.first = int(not self._z_set)
            g["k"] = int(g["k"]) + 1
            arr.append(s)
        return sorted(arr, key=lambda s: s.begin)

    @torch.no_grad()
    def step(self, closure=None):
        if not self.train_mode:
            raise RuntimeError("Optimizer was not in train mode when step is called. Please insert .train() and "
                               ".eval() calls on the optimizer. See documentation for details.")
        loss = closure() if closure is not None else None
        clip = self._take_clip()
        st = self.store
        st.wait_params()
        p, w = self._pw()
        self._advance_seed()
        K.sf_adamw_step(p, st.grad, w, self.z, self.exp_avg_sq, self._groups_struct(), clip_coef=clip,
                        stochastic_rounding=self.stochastic_rounding and self._bf16_store, seed=self.seed)
        self._z_set = True
        return loss

    def step_parameter(self, p, group, i):
        raise NotImplementedError("SCHEDULE_FREE_ADAMW step_parameter (fused_back_pass): the reference offers the fused "
                                  "back pass for other optimizers only")

    # --- the two modes ------------------------------------------------------------------------------------------------
    def _swap(self, weight_of):
        p, w = self._pw()
        groups = []
        for gi, g in enumerate(self.param_groups):
            s = _lib.SfSwapGroup()
            s.begin, s.end = self._ranges[gi]
            s.w = weight_of(float(g["betas"][0]))
            groups.append(s)
        K.sf_swap(p, w, self.z, sorted(groups, key=lambda s: s.begin))

    @torch.no_grad()
    def eval(self):
        """y -> x: the store holds the averaged weights, the ones to save.  The bits of y wait in a buffer."""
        if not self.train_mode:
            return
        if self._z_set:   # before the first step x = y = z
            self.store.wait_params()
            self._y_saved = self._pw()[0].detach().clone()
            self._swap(lambda beta1: 1 - 1 / beta1)
        self._set_mode(False)

    @torch.no_grad()
    def train(self):
        """x -> y: the saved bits when eval() of this object made x, else y = x + (1 - beta1) (z - x)."""
        if self.train_mode:
            return
        if self._z_set:
            st = self.store
            st.wait_params()
            if self._y_saved is not None:
                p, w = self._pw()
                p.copy_(self._y_saved)
                if w is not None:
                    w.copy_(p)   # the working copy is rne(master), as the step leaves it
            else:
                self._swap(lambda beta1: 1 - beta1)
        self._y_saved = None
        self._set_mode(True)

    # --- state: nothing before the first step, as for any torch optimizer --------------------------------------------
    def _views(self, name):
        return {"z": self._flat(self.z, name), "exp_avg_sq": self._flat(self.exp_avg_sq, name)}

    def _has_state(self, name, gi):
        return self._z_set

    def _group_loaded(self, g):
        check_hyper(g)

    def _load_tensor(self, name, gi, st):
        super()._load_tensor(name, gi, st)
        self._z_set = True

    def _loaded(self, fresh):
        self._y_saved = None   # the store now holds what the state says, not what eval() of this object left
        if self._z_set:   # a tensor without saved state starts here: x = y = z is its current value
            for name in fresh:
                self._views(name)["z"].copy_(self.store.value(name))
        self._set_mode(self.train_mode)   # one mode for the whole store
