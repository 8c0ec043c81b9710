"""Fused CAME (confidence-guided adaptive memory-efficient optimization) over a FlatParamStore.

Drop-in for what the reference builds at modules/util/create.py:938-951:
    CAME(params, lr, betas=(beta1, beta2, beta3), weight_decay, eps=(eps, eps2), stochastic_rounding)
        # modules/util/optimizer/CAME.py
Same optimizer contract as FusedAdafactor (param_groups with 'lr', 'betas', 'eps', 'clip_threshold' and
'weight_decay'; step, zero_grad, clip_grad_norm_, step_parameter; state_dict / load_state_dict in the reference's
layout: per parameter 'step', 'RMS', 'exp_avg' and 'exp_avg_sq_row' + 'exp_avg_sq_col' + 'exp_avg_res_row' +
'exp_avg_res_col' or 'exp_avg_sq'; 'sr_seed' at the top level).  A step is nine launches over the whole store
(csrc/came.hip) driven by the Adafactor tensor and slab tables (factored_store.adafactor_tables) and a fold table
built once here; the optimizer around them is factored_store.FactoredStoreOptimizer, shared with FusedAdafactor.

States are fp32 whatever the parameter dtype, as the reference allocates them from the float gradient
(CAME.py:84-109): the first moment is full-size, the second moment and the instability keep one row vector and one
column vector per matrix (the last two dimensions of a tensor of ndim >= 2; the leading ones are a batch).  So the
optimizer state is about AdamW's size (4 B a parameter against two bf16 moments): CAME is here for parity with the
reference, not to save memory.

Deviations from the reference, recorded in DESIGN.md:
  * 'RMS' is saved as 0.  The reference stores rms(p) there each step (CAME.py:114) and nothing reads it.
  * a tensor that received no gradient is stepped with a zero gradient (the store zeroes it), as FusedAdamW and
    FusedAdafactor do; the reference skips it.
  * under stochastic rounding a bf16 parameter is rounded once, from the fp32 fma(p, alpha, p) - lr * update.  The
    reference rounds twice stochastically when weight_decay != 0 (CAME.py:165-176); one unbiased rounding has the
    same expectation.  stochastic_rounding=False reproduces the reference's two round-to-nearest adds bit for bit.
Refused by name (ValueError): a missing or non-positive lr, a beta outside [0, 1] (the reference's assertions,
CAME.py:41-42).
"""
from __future__ import annotations

import torch

from ... import _lib
from ... import kernels as K
from .factored_store import FactoredStoreOptimizer

FOLD_BLOCK = 256   # csrc/came.hip: AF_THREADS rows, or columns, per fold workgroup (a thread each)


def check_fold_table(fold, n_fold, n_mean, tensors, n_tensors):
    """every range the fold table names, against the tensor table (the kernels trust the tables): entries
    [0, n_fold) are blocks of rows (kind 0) or columns (kind 1) of a mode 2 tensor, entries [n_fold, n_fold + n_mean)
    one of its matrices (kind 2)."""
    for i in range(n_fold + n_mean):
        f = fold[i]
        ok = 0 <= f.tensor < n_tensors and tensors[f.tensor].mode == 2 and f.kind in ((0, 1) if i < n_fold else (2,))
        if ok:
            t = tensors[f.tensor]
            limit = t.batch * (t.rows, t.cols, 1)[f.kind]
            ok = 0 <= f.i0 < f.i1 <= limit and f.i1 - f.i0 <= (1 if f.kind == 2 else FOLD_BLOCK)
        if not ok:
            raise ValueError("came fold table: an entry outside its tensor")


def came_fold_table(tensors, n_tensors):
    """the fold table of csrc/came.hip for an Adafactor tensor table: for every mode 2 tensor (a matrix that spans
    slabs) blocks of FOLD_BLOCK rows and of FOLD_BLOCK columns, then one entry per matrix for the row-state mean.
    Returns (fold, n_fold, n_mean, ranges) with ranges[ti] = (f0, f1, r0, r1): tensor ti's entries [f0, f1) of the
    row / column blocks and [r0, r1) of the means (indices into the one table, the means after the blocks)."""
    blocks, means, spans = [], [], {}

    def entry(dst, ti, kind, i0, i1):
        f = _lib.CameFold()
        f.i0, f.i1, f.tensor, f.kind = i0, i1, ti, kind
        dst.append(f)

    for ti in range(n_tensors):
        t = tensors[ti]
        f0, r0 = len(blocks), len(means)
        if t.mode == 2:
            for kind, n in ((0, t.batch * t.rows), (1, t.batch * t.cols)):
                for i0 in range(0, n, FOLD_BLOCK):
                    entry(blocks, ti, kind, i0, min(n, i0 + FOLD_BLOCK))
            for b in range(t.batch):
                entry(means, ti, 2, b, b + 1)
        spans[ti] = (f0, len(blocks), r0, len(means))
    nf, nm = len(blocks), len(means)
    ranges = {ti: (f0, f1, nf + r0, nf + r1) for ti, (f0, f1, r0, r1) in spans.items()}
    fold = (_lib.CameFold * max(1, nf + nm))(*(blocks + means))
    check_fold_table(fold, nf, nm, tensors, n_tensors)
    return fold, nf, nm, ranges


def _check_hyper(lr, betas):
    """the reference's assertions (CAME.py:41-42), refused by name"""
    if lr is None or not float(lr) > 0.0:
        raise ValueError(f"CAME lr: a positive learning rate is required, got {lr!r}")
    if len(tuple(betas)) != 3 or not all(0.0 <= float(b) <= 1.0 for b in betas):
        raise ValueError(f"CAME betas: three coefficients in [0, 1] are required, got {betas!r}")


class FusedCAME(FactoredStoreOptimizer):
    TUPLE_KEYS = ("eps", "betas")

    def __init__(self, store, param_groups, lr=None, eps=(1e-30, 1e-16), clip_threshold=1.0,
                 betas=(0.9, 0.999, 0.9999), weight_decay=0.0, stochastic_rounding=False, seed=0):
        _check_hyper(lr, betas)
        defaults = dict(lr=lr, eps=tuple(eps), clip_threshold=clip_threshold, betas=tuple(betas),
                        weight_decay=weight_decay)
        super().__init__(param_groups, defaults)
        for g in self.param_groups:
            _check_hyper(g["lr"], g["betas"])
        self._init_factored(store, stochastic_rounding, seed)

    def _alloc(self, tensors, n_state, n_scratch):
        dev = self.store.device
        fold, self._nf, self._nm, self._fold_ranges = came_fold_table(tensors, self._nt)
        self._fold = self._to_device(fold)
        self.exp_avg = torch.zeros(self.store.numel, dtype=torch.float32, device=dev)   # first moment, store layout
        self.state_buf = torch.zeros(n_state, dtype=torch.float32, device=dev)       # row / column / full second moments
        self.res_buf = torch.zeros(n_state, dtype=torch.float32, device=dev)         # row / column instability
        self._scratch = torch.zeros(n_scratch, dtype=torch.float32, device=dev)
        self._scratch_res = torch.zeros(n_scratch, dtype=torch.float32, device=dev)
        self._slab_sq = torch.zeros(max(1, self._ns), dtype=torch.float64, device=dev)
        self._scal = torch.zeros(max(8, self._nt), dtype=torch.float32, device=dev)   # rms(u) per tensor

    def _groups_struct(self, steps=None):
        arr = []
        for g in self.param_groups:
            lr = float(g["lr"])
            b1, b2, b3 = (float(b) for b in g["betas"])
            s = _lib.CameGroup()
            s.lr = lr
            s.alpha_wd = -g["weight_decay"] * lr
            s.eps1, s.eps2 = g["eps"]
            s.clip_threshold = g["clip_threshold"]
            s.beta1, s.one_minus_beta1 = b1, 1.0 - b1
            s.beta2, s.one_minus_beta2 = b2, 1.0 - b2
            s.beta3, s.one_minus_beta3 = b3, 1.0 - b3
            arr.append(s)
        return arr

    def _ranges_all(self):
        return super()._ranges_all() + ((0, self._nf), (self._nf, self._nf + self._nm))

    def _ranges_of(self, ti):
        f0, f1, r0, r1 = self._fold_ranges[ti]
        return super()._ranges_of(ti) + ((f0, f1), (r0, r1))

    def _launch(self, p, g, w, groups, ranges, clip, sr):
        K.came_step(p, g, w, self.exp_avg, self.state_buf, self.res_buf, self._scratch, self._scratch_res,
                    self._slab_sq, self._scal, self._tensors, ranges[0], self._slabs, ranges[1], self._fold, ranges[2],
                    ranges[3], groups, clip_coef=clip, stochastic_rounding=sr, seed=self.seed)

    # --- the reference's CAME state layout (CAME.py:79-178) ---------------------------------------------------------
    def _views(self, name):
        """{state key: view of its buffer} of one tensor's moments"""
        s = self.store.slots[name]
        t = self._table[self._tindex[name]]
        v = {"exp_avg": self._flat(self.exp_avg, name)}
        if t.mode == 0:
            v["exp_avg_sq"] = self.state_buf[t.full_off:t.full_off + t.numel].view(s.shape)
            return v
        for key, buf in (("sq", self.state_buf), ("res", self.res_buf)):
            v[f"exp_avg_{key}_row"] = buf[t.row_off:t.row_off + t.batch * t.rows].view(s.shape[:-1])
            v[f"exp_avg_{key}_col"] = buf[t.col_off:t.col_off + t.batch * t.cols].view(s.shape[:-2] + s.shape[-1:])
        return v
