"""What the factored optimizers over a FlatParamStore share (FusedAdafactor, adafactor_fused.py; FusedCAME,
came_fused.py): the tensor and slab tables that csrc/adafactor_walk.h walks, and the optimizer around them: the
8-group limit, the step counters, step(), step_parameter() and the 'step' / 'RMS' entries of the state dict (the
walk is flat_store.FlatStoreOptimizer's).  A subclass supplies its buffers (_alloc), its group structs
(_groups_struct), its launch (_launch), the views of one tensor's states (_views), and where it differs: the saved
'RMS' (_rms, _load_rms), the group keys that load as tuples (TUPLE_KEYS), further per-tensor table ranges
(_ranges_all, _ranges_of) and the step counts step_parameter uses (_parameter_steps)."""
from __future__ import annotations

import torch

from ... import _lib
from .flat_store import FlatStoreOptimizer

# csrc/adafactor_walk.h: AF_STAGE floats per LDS stage, column tiles of at most AF_CT, AF_STAGES stages per slab
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


class FactoredStoreOptimizer(FlatStoreOptimizer):
    TUPLE_KEYS = ("eps",)   # group keys that load_state_dict restores as tuples

    def _init_factored(self, store, stochastic_rounding, seed):
        """after torch's Optimizer.__init__: the store, the tables and the subclass's buffers"""
        if len(self.param_groups) > 8:
            raise ValueError(f"{type(self).__name__}: at most 8 parameter groups")
        self._init_store(store)
        self.stochastic_rounding = bool(stochastic_rounding)
        self.seed = seed
        self.steps = [0 for _ in self.param_groups]
        entries = []
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                s = store.slots[self._name(p)]
                entries.append((s.offset, s.shape, gi, s.name))
        entries.sort(key=lambda e: e[0])
        tensors, slabs, self._nt, self._ns, n_state, n_scratch = adafactor_tables([e[:3] for e in entries],
                                                                                 store.numel)
        self._table = [tensors[i] for i in range(self._nt)]          # host copies (state_dict, step_parameter)
        names = [e[3] for e in entries if store.slots[e[3]].numel > 0]
        self._tindex = {n: i for i, n in enumerate(names)}
        self._tensors, self._slabs = self._to_device(tensors), self._to_device(slabs)
        self._alloc(tensors, n_state, n_scratch)

    # --- what a subclass may extend ---------------------------------------------------------------------------------
    def _ranges_all(self):
        """the table ranges of a store step: (tensors, slabs, ...)"""
        return (0, self._nt), (0, self._ns)

    def _ranges_of(self, ti):
        """the table ranges of tensor ti alone (step_parameter)"""
        t = self._table[ti]
        return (ti, ti + 1), (t.slab0, t.slab0 + t.n_slabs)

    def _parameter_steps(self, name, group):
        """the per-group step counts of a step_parameter call on one tensor of `group`"""
        return self.steps

    def _rms(self):
        """per table entry, the value saved as 'RMS' (a CPU tensor)"""
        return torch.zeros(max(1, self._nt))

    def _load_rms(self, ti, value):
        pass

    # --- the optimizer ------------------------------------------------------------------------------------------------
    def _call(self, steps, ranges, clip):
        p, w = self._pw()
        self._launch(p, self.store.grad, w, self._groups_struct(steps), ranges, clip,
                     self.stochastic_rounding and self._bf16_store)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        self.store.wait_params()
        for gi in range(len(self.param_groups)):
            self.steps[gi] += 1
        clip = self._take_clip()
        self._advance_seed()
        self._call(self.steps, self._ranges_all(), clip)
        return loss

    def step_parameter(self, p, group, i):
        """fused-back-pass API: update one parameter tensor."""
        self.store.wait_params()
        name = self._name(p)
        if name in self._tindex:
            self._call(self._parameter_steps(name, group), self._ranges_of(self._tindex[name]), None)

    # --- state in the reference optimizer's layout: every tensor of the table, from the start ------------------------
    def _has_state(self, name, gi):
        return name in self._tindex   # an empty tensor has no table entry

    def state_dict(self):
        self.store.wait_params()
        self._rms_saved = self._rms()   # one read-back for the whole dict
        return super().state_dict()

    def _save_tensor(self, name, gi):
        return {"step": self.steps[gi], "RMS": self._rms_saved[self._tindex[name]].clone(),
                **super()._save_tensor(name, gi)}

    def _load_tensor(self, name, gi, st):
        if name in self._tindex:
            super()._load_tensor(name, gi, st)
            self._load_rms(self._tindex[name], float(st.get("RMS", 0.0)))
            self.steps[gi] = int(float(st["step"]))
