"""Fused Adafactor (factored second moments) over a FlatParamStore.

Drop-in for what the reference builds at modules/util/create.py:914-936:
    transformers.Adafactor(params, lr, eps=(eps, eps2), clip_threshold, decay_rate, beta1, weight_decay,
                           scale_parameter, relative_step, warmup_init)
    patch_adafactor(optimizer, stochastic_rounding)      # modules/util/optimizer/adafactor_extensions.py:118-121
Same optimizer contract as FusedAdamW (param_groups with 'lr', step, zero_grad, clip_grad_norm_, step_parameter,
state_dict / load_state_dict in transformers' Adafactor layout: per parameter 'step', 'RMS' and
'exp_avg_sq_row' + 'exp_avg_sq_col' or 'exp_avg_sq'; 'sr_seed' at the top level).  A step is five launches over the
whole store (csrc/adafactor.hip) driven by a tensor table and a slab table built once here.

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
from .adamw_fused import FlatStoreOptimizer

# csrc/adafactor.hip: AF_STAGE floats per LDS stage, column tiles of at most AF_CT, AF_STAGES stages per slab
AF_STAGE, AF_CT, AF_STAGES = 4096, 4080, 8


def _up8(n: int) -> int:
    return (n + 7) // 8 * 8


def adafactor_tables(entries, store_numel: int):
    """entries: [(offset, shape, group)] of the tensors to step, in store order.  Returns (tensors, slabs,
    n_tensors, n_slabs, state_numel, scratch_numel): the ctypes AdafactorTensor / AdafactorSlab arrays
    csrc/adafactor.hip walks, their lengths, and the sizes of the fp32 state and scratch buffers their offsets index.  Every range a table names is checked here
    against the buffers (the kernels trust the tables)."""
    T, S = [], []
    state = scratch = 0
    for offset, shape, group in entries:
        numel = 1
        for d in shape:
            numel *= int(d)
        if numel == 0:
            continue
        if offset % 8 or offset < 0 or offset + numel > store_numel:
            raise ValueError("adafactor table: tensor outside the store or not 8-element aligned")
        t = _lib.AdafactorTensor()
        t.offset, t.numel, t.group = offset, numel, group
        t.row_off = t.col_off = t.full_off = t.rpart_off = t.cpart_off = t.rmean_off = -1
        t.slab0 = len(S)
        ti = len(T)

        def slab(row0, row1, col0, col1):
            s = _lib.AdafactorSlab()
            s.row0, s.row1, s.tensor, s.col0, s.col1 = row0, row1, ti, col0, col1
            S.append(s)

        if len(shape) < 2:
            t.mode, t.batch, t.rows, t.cols = 0, 1, 1, numel
            t.full_off = state
            state += _up8(numel)
            for e0 in range(0, numel, AF_STAGE * AF_STAGES):
                slab(e0, min(numel, e0 + AF_STAGE * AF_STAGES), 0, 0)
        else:
            rows, cols = int(shape[-2]), int(shape[-1])
            batch = numel // (rows * cols)
            if max(batch, rows, cols) >= 1 << 31:
                raise ValueError("adafactor table: a dimension of 2^31 or more")
            t.batch, t.rows, t.cols = batch, rows, cols
            t.row_off = state
            state += _up8(batch * rows)
            t.col_off = state
            state += _up8(batch * cols)
            t.rmean_off = scratch
            scratch += _up8(batch)
            if rows * cols <= AF_STAGE:
                mps = AF_STAGE // (rows * cols)            # whole matrices per LDS stage
                t.mode, t.slab_rows, t.row_slabs, t.col_tiles = 1, mps, 1, 1
                for m0 in range(0, batch, mps * AF_STAGES):
                    slab(m0 * rows, min(batch, m0 + mps * AF_STAGES) * rows, 0, cols)
            else:
                tiles = [(c0, min(cols, c0 + AF_CT)) for c0 in range(0, cols, AF_CT)]
                w8 = ((tiles[0][1] - tiles[0][0] + 7) // 8 + 1) * 8     # the widest tile's padded stage row
                slab_rows = min(rows, AF_STAGES * max(1, AF_STAGE // w8))
                row_slabs = (rows + slab_rows - 1) // slab_rows
                assert w8 <= AF_STAGE and slab_rows <= AF_STAGE
                t.mode, t.slab_rows, t.row_slabs, t.col_tiles = 2, slab_rows, row_slabs, len(tiles)
                t.rpart_off = scratch
                scratch += _up8(batch * rows * len(tiles))
                t.cpart_off = scratch
                scratch += _up8(batch * row_slabs * cols)
                for b in range(batch):
                    for r0 in range(0, rows, slab_rows):
                        for c0, c1 in tiles:
                            slab(b * rows + r0, b * rows + min(rows, r0 + slab_rows), c0, c1)
        t.n_slabs = len(S) - t.slab0
        T.append(t)
    for t in T:   # what the kernels index: slabs inside their tensor, states and partials inside their buffers
        for s in S[t.slab0:t.slab0 + t.n_slabs]:
            if t.mode == 0:
                ok = 0 <= s.row0 < s.row1 <= t.numel
            else:
                ok = (0 <= s.row0 < s.row1 <= t.batch * t.rows and 0 <= s.col0 < s.col1 <= t.cols
                      and s.col1 - s.col0 <= AF_CT)
                if t.mode == 1:
                    ok = ok and s.row0 % t.rows == 0 and s.row1 % t.rows == 0 and s.col1 - s.col0 == t.cols
                else:
                    ok = ok and s.row0 // t.rows == (s.row1 - 1) // t.rows and s.row1 - s.row0 <= t.slab_rows
            if not ok:
                raise ValueError("adafactor table: a slab outside its tensor")
        ends = [t.full_off + t.numel] if t.mode == 0 else [t.row_off + t.batch * t.rows, t.col_off + t.batch * t.cols]
        if max(ends) > state or (t.mode and t.rmean_off + t.batch > scratch) or (
                t.mode == 2 and max(t.rpart_off + t.batch * t.rows * t.col_tiles,
                                    t.cpart_off + t.batch * t.row_slabs * t.cols) > scratch):
            raise ValueError("adafactor table: a state or partial range outside its buffer")
    tensors = (_lib.AdafactorTensor * max(1, len(T)))(*T)
    slabs = (_lib.AdafactorSlab * max(1, len(S)))(*S)
    return tensors, slabs, len(T), len(S), max(8, state), max(8, scratch)


def _to_device(arr, device):
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)


class FusedAdafactor(FlatStoreOptimizer):
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
        if len(self.param_groups) > 8:
            raise ValueError("FusedAdafactor: at most 8 parameter groups")
        self._init_store(store)
        self.stochastic_rounding = bool(stochastic_rounding)
        self.seed = seed
        self.steps = [0 for _ in self.param_groups]
        entries = []
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                s = store.slots[self._ptr2name[p.data_ptr()]]
                entries.append((s.offset, s.shape, gi, s.name))
        entries.sort(key=lambda e: e[0])
        tensors, slabs, self._nt, self._ns, n_state, n_scratch = adafactor_tables([e[:3] for e in entries],
                                                                                 store.numel)
        self._table = [tensors[i] for i in range(self._nt)]          # host copies (state_dict, step_parameter)
        names = [e[3] for e in entries if store.slots[e[3]].numel > 0]
        self._tindex = {n: i for i, n in enumerate(names)}
        dev = store.device
        self._tensors, self._slabs = _to_device(tensors, dev), _to_device(slabs, dev)
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

    def _launch(self, groups, t_range, s_range, clip):
        st = self.store
        p = self.master if self.master is not None else st.data
        w = st.data if self.master is not None else None
        K.adafactor_step(p, st.grad, w, self.state_buf, self._scratch, self._slab_sq, self._scal, self._tensors,
                         t_range, self._slabs, s_range, groups, clip_coef=clip,
                         stochastic_rounding=self.stochastic_rounding and w is None and st.dtype == torch.bfloat16,
                         seed=self.seed)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        self.store.wait_params()
        for gi in range(len(self.param_groups)):
            self.steps[gi] += 1
        clip = self.clip_out if self._pending_clip else None
        self._pending_clip = False
        if self.master is None and self.store.dtype == torch.bfloat16:
            self.seed = (self.seed * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        self._launch(self._groups_struct(self.steps), (0, self._nt), (0, self._ns), clip)
        return loss

    def step_parameter(self, p, group, i):
        """fused-back-pass API (adafactor_extensions.py:118-121): update one parameter tensor."""
        self.store.wait_params()
        gi = next(i for i, g in enumerate(self.param_groups) if g is group)
        name = self._ptr2name[p.data_ptr()]
        if name not in self._tindex:
            return
        if not hasattr(self, "_pstep"):
            self._pstep = {}
        self._pstep[name] = self._pstep.get(name, self.steps[gi]) + 1
        steps = list(self.steps)
        steps[gi] = self._pstep[name]
        ti = self._tindex[name]
        t = self._table[ti]
        self._launch(self._groups_struct(steps), (ti, ti + 1), (t.slab0, t.slab0 + t.n_slabs), None)

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

    def state_dict(self):
        self.store.wait_params()
        state, groups, idx = {}, [], 0
        scal = self._scal.cpu()
        for gi, g in enumerate(self.param_groups):
            ids = []
            for p in g["params"]:
                name = self._ptr2name[p.data_ptr()]
                if name in self._tindex:
                    d = {"step": self.steps[gi], "RMS": scal[4 * self._tindex[name]].clone()}
                    d.update({k: v.clone() for k, v in self._views(name).items()})
                    state[idx] = d
                ids.append(idx)
                idx += 1
            gd = {k: v for k, v in g.items() if k != "params"}
            gd["params"] = ids
            groups.append(gd)
        # the stochastic-rounding stream position, so that a resumed run rounds like an uninterrupted one
        return {"state": state, "param_groups": groups, "sr_seed": int(self.seed)}

    def load_state_dict(self, sd):
        self.store.wait_params()
        if "sr_seed" in sd:
            self.seed = int(sd["sr_seed"])
        for gi, (g, gsd) in enumerate(zip(self.param_groups, sd["param_groups"])):
            for k, v in gsd.items():
                if k != "params":
                    g[k] = tuple(v) if k == "eps" else v
            for p, pid in zip(g["params"], gsd["params"]):
                name = self._ptr2name[p.data_ptr()]
                st = sd["state"].get(pid)
                if st and name in self._tindex:
                    for k, v in self._views(name).items():
                        v.copy_(st[k].reshape(v.shape))
                    self._scal[4 * self._tindex[name]] = float(st.get("RMS", 0.0))
                    self.steps[gi] = int(float(st["step"]))
