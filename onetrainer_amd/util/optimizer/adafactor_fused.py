"""Fused Adafactor (factored second moments) over a FlatParamStore.

Drop-in for what the reference builds at modules/util/create.py:914-936:
    transformers.Adafactor(params, lr, eps=(eps, eps2), clip_threshold, decay_rate, beta1, weight_decay,
                           scale_parameter, relative_step, warmup_init)
    patch_adafactor(optimizer, stochastic_rounding)      # modules/util/optimizer/adafactor_extensions.py:118-121
Same optimizer contract as FusedAdamW (param_groups with 'lr', step, zero_grad, clip_grad_norm_, step_parameter,
state_dict / load_state_dict in transformers' Adafactor layout: per parameter 'step', 'RMS' and
'exp_avg_sq_row' + 'exp_avg_sq_col' or 'exp_avg_sq'; 'sr_seed' at the top level).  A step is five launches over the
whole store (csrc/adafactor.hip) driven by a tensor table and a slab table built once (factored_store.py, which
also holds step, step_parameter and the state dict: FactoredStoreOptimizer, shared with FusedCAME).

States are fp32 whatever the parameter dtype: one row vector and one column vector per matrix (the last two
dimensions of a tensor of ndim >= 2; the leading ones are a batch, so a (cout, cin, 3, 3) conv weight keeps
cout * cin 3x3 factorisations, as the reference's grad_shape[:-1] / grad_shape[:-2] + grad_shape[-1:] do).

Deviations from the reference, recorded in DESIGN.md:
  * stochastic_rounding is honoured for bf16 parameters.  In the reference the stochastic copy is followed by an
    unconditional p.copy_(p_data_fp32) (adafactor_extensions.py:92-95), so the flag has no effect there and bf16
    weights are rounded to nearest; stochastic_rounding=False reproduces that bit for bit.
  * a tensor that received no gradient is stepped with a zero gradient (the store zeroes it), as FusedAdamW does;
    the reference skips it.
  * 'RMS' is tracked only with scale_parameter (nothing else reads it); it is 0 otherwise.
Refused (NotImplementedError naming the option): relative_step, warmup_init (and with them the ADAFACTOR LR
scheduler), beta1 (a full-size first moment is what this optimizer exists to avoid).
"""
from __future__ import annotations

import torch

from ... import _lib
from ... import kernels as K
from .factored_store import AF_CT, AF_STAGE, AF_STAGES, FactoredStoreOptimizer, adafactor_tables  # noqa: F401


class FusedAdafactor(FactoredStoreOptimizer):
    def __init__(self, store, param_groups, lr=None, eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8,
                 beta1=None, weight_decay=0.0, scale_parameter=True, relative_step=True, warmup_init=False,
                 stochastic_rounding=False, seed=0):
        if relative_step:
            raise NotImplementedError("Adafactor relative_step=True (and the ADAFACTOR LR scheduler) is not on the hot "
                                      "path: set relative_step=False and a learning rate")
        if warmup_init:
            raise NotImplementedError("Adafactor warmup_init=True needs relative_step, which is not on the hot path")
        if beta1 is not None:
            raise NotImplementedError("Adafactor beta1: a full-size first moment is not on the hot path")
        if lr is None:
            raise ValueError("Adafactor without relative_step needs a learning rate")
        defaults = dict(lr=lr, eps=tuple(eps), clip_threshold=clip_threshold, decay_rate=decay_rate, beta1=None,
                        weight_decay=weight_decay, scale_parameter=scale_parameter, relative_step=False,
                        warmup_init=False)
        super().__init__(param_groups, defaults)
        self._init_factored(store, stochastic_rounding, seed)
        self._pstep = {}   # step_parameter's per-tensor step counts

    def _alloc(self, tensors, n_state, n_scratch):
        dev = self.store.device
        self.state_buf = torch.zeros(n_state, dtype=torch.float32, device=dev)     # row / column / full second moments
        self._scratch = torch.zeros(n_scratch, dtype=torch.float32, device=dev)
        self._slab_sq = torch.zeros(2 * max(1, self._ns), dtype=torch.float64, device=dev)
        self._scal = torch.zeros(4 * max(1, self._nt), dtype=torch.float32, device=dev)   # rms(p), rms(u) per tensor

    def _groups_struct(self, steps):
        arr = []
        for g, step in zip(self.param_groups, steps):
            lr = float(g["lr"])
            beta2t = 1.0 - float(max(step, 1)) ** g["decay_rate"]   # step 0: a group step_parameter does not touch
            s = _lib.AdafactorGroup()
            s.lr = lr
            s.neg_wd = -g["weight_decay"]
            s.alpha_wd = -g["weight_decay"] * lr
            s.eps1, s.eps2 = g["eps"]
            s.clip_threshold = g["clip_threshold"]
            s.beta2t = beta2t
            s.one_minus_beta2t = 1.0 - beta2t
            s.scale_parameter = int(bool(g["scale_parameter"]))
            arr.append(s)
        return arr

    def _launch(self, p, g, w, groups, ranges, clip, sr):
        K.adafactor_step(p, g, w, self.state_buf, self._scratch, self._slab_sq, self._scal, self._tensors, ranges[0],
                         self._slabs, ranges[1], groups, clip_coef=clip, stochastic_rounding=sr, seed=self.seed)

    def _parameter_steps(self, name, group):
        """fused-back-pass API (adafactor_extensions.py:118-121): the tensor's own step count in its group's place"""
        gi = next(i for i, g in enumerate(self.param_groups) if g is group)
        self._pstep[name] = self._pstep.get(name, self.steps[gi]) + 1
        steps = list(self.steps)
        steps[gi] = self._pstep[name]
        return steps

    # --- transformers Adafactor-compatible state ------------------------------------------------------------------
    def _views(self, name):
        """{state key: view of the state buffer} of one tensor's second moments"""
        s = self.store.slots[name]
        t = self._table[self._tindex[name]]
        if t.mode == 0:
            return {"exp_avg_sq": self.state_buf[t.full_off:t.full_off + t.numel].view(s.shape)}
        return {"exp_avg_sq_row": self.state_buf[t.row_off:t.row_off + t.batch * t.rows].view(s.shape[:-1]),
                "exp_avg_sq_col": self.state_buf[t.col_off:t.col_off + t.batch * t.cols]
                .view(s.shape[:-2] + s.shape[-1:])}

    def _rms(self):
        return self._scal.cpu()[::4]

    def _load_rms(self, ti, value):
        self._scal[4 * ti] = value
