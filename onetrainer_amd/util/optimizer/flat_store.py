"""What every fused optimizer over a FlatParamStore shares: FlatStoreOptimizer (the parameter groups as element
ranges, the global grad norm and its clip, the store forms, the stochastic-rounding seed and one state_dict /
load_state_dict walk with hooks for what differs) and OverlappedGradNorm (the norm pass spread over the backward)."""
from __future__ import annotations

import os

import torch

from ... import _lib
from ... import kernels as K

_NORM_CHECK = os.environ.get("OTAMD_NORM_CHECK") == "1"

# the stochastic-rounding seed advances by one step of this 64-bit LCG (Knuth's MMIX constants) per optimizer step
SR_LCG_MUL, SR_LCG_ADD = 6364136223846793005, 1442695040888963407


class FlatStoreOptimizer(torch.optim.Optimizer):
    """What every fused optimizer over a FlatParamStore shares: the parameter groups as contiguous element ranges,
    the per-tensor chunk table of the global grad norm, clip_grad_norm_ (whose coefficient stays on the device and is
    applied inside the next step()), the hook OverlappedGradNorm attaches to, the store form of a launch, the
    stochastic-rounding seed and the walk of state_dict / load_state_dict.  FusedAdamW (adamw_fused.py), FusedAdafactor
    and FusedCAME (through factored_store.py), FusedProdigy (prodigy_fused.py), FusedScheduleFreeAdamW
    (schedule_free_fused.py) and FusedAdamW8bit (adamw8bit_fused.py) derive from it and supply, for the state dict,
    _views and whichever of the hooks below differ for them."""

    TUPLE_KEYS = ()   # group keys that load_state_dict restores as tuples

    def _init_store(self, store):
        self.store = store
        # fp32 master weights (module/param_store.py `master`): fp32 moments, the reference's fp32 AdamW path
        # (adamw_extensions.py:125-148 without stochastic rounding, which applies to bf16 parameters only)
        self.master = getattr(store, "master", None)
        self._norm_dtype = K.grad_norm_dtype(store.grad, self.master is not None) if store.grad is not None else 0
        self._ptr2name = {store.params[n].data_ptr(): n for n in store.order}
        self._ranges = []
        for g in self.param_groups:
            offs = []
            for p in g["params"]:
                s = store.slots[self._name(p)]
                offs.append((s.offset, s.offset + s.numel))
            b, e = min(o[0] for o in offs), max(o[1] for o in offs)
            span = [s for s in store.order if b <= store.slots[s].offset < e]
            if len(span) != len(offs):
                raise ValueError("each optimizer param group must be a contiguous range of the flat store")
            self._ranges.append((b, e))
        # per-tensor chunk table for the global grad norm
        chunks = []
        for ti, n in enumerate(store.order):
            s = store.slots[n]
            for c0 in range(s.offset, s.offset + s.numel, 1 << 16):
                chunks.append((c0, min(s.offset + s.numel, c0 + (1 << 16)), ti))
        arr = (_lib.NormChunk * len(chunks))()
        for i, (b, e, t) in enumerate(chunks):
            arr[i].begin, arr[i].end, arr[i].tensor = b, e, t
        self._chunks = self._to_device(arr)
        self._n_chunks = len(chunks)
        self._tensor_sq = torch.zeros(len(store.order), dtype=torch.float64, device=store.device)
        self._chunk_sq = torch.zeros(max(1, len(chunks)), dtype=torch.float64, device=store.device)   # one slot per chunk
        self.clip_out = torch.zeros(2, dtype=torch.float32, device=store.device)   # [coef, total norm]
        self._chunk_tensor = [c[2] for c in chunks]
        self.norm_overlap = None   # OverlappedGradNorm, attached by the trainer (single process, clip on)
        self._pending_clip = False

    # --- clip_grad_norm_ (GenericTrainer.py:712-713) ----------------------------------------------
    def clip_grad_norm_(self, max_norm: float) -> torch.Tensor:
        """computes the clip coefficient on device; it is applied inside the next step()."""
        self.store.wait_params()   # the previous (overlapped) update still reads grads / clip_out
        nt = len(self.store.order)
        if self.norm_overlap is not None and self.norm_overlap.take():   # sums accumulated during backward
            if _NORM_CHECK:   # debug: every overlapped chunk sum against the same pass over the final gradients
                ref = torch.empty_like(self._chunk_sq)
                _lib.check(_lib.lib().otamd_grad_sqnorm_chunks(self.store.grad.data_ptr(), self._norm_dtype,
                                                               self._chunks.data_ptr(), 0, self._n_chunks,
                                                               ref.data_ptr(), K.stream_handle()), "norm check")
                bad = (ref != self._chunk_sq[:self._n_chunks]).nonzero().flatten().tolist()
                if bad:
                    names = sorted({self.store.order[self._chunk_tensor[c]] for c in bad})
                    print(f"[norm check] {len(bad)} of {self._n_chunks} overlapped chunk sums differ from the final "
                          f"gradients': {names[:12]}", flush=True)
            _lib.check(_lib.lib().otamd_grad_clip_finalize(self._chunks.data_ptr(), self._n_chunks,
                                                           self._chunk_sq.data_ptr(), self._tensor_sq.data_ptr(), nt,
                                                           float(max_norm), self._norm_dtype,
                                                           self.clip_out.data_ptr(), K.stream_handle()),
                       "otamd_grad_clip_finalize")
        else:
            K.grad_clip_coef(self.store.grad, self._chunks, self._n_chunks, self._chunk_sq, self._tensor_sq, nt,
                             max_norm, self.clip_out, fp32_semantics=self.master is not None)
        self._pending_clip = True
        return self.clip_out[1]

    def _take_clip(self):
        """the device clip coefficient a clip_grad_norm_ since the last step left for this one, or None"""
        clip = self.clip_out if self._pending_clip else None
        self._pending_clip = False
        return clip

    def zero_grad(self, set_to_none: bool = True):
        """grads are views of the flat store that the next backward overwrites; nothing to clear."""
        self.store.accumulating = False

    # --- the store and its forms ------------------------------------------------------------------------------------
    def _to_device(self, arr) -> torch.Tensor:
        """a ctypes struct array as uint8 bytes on the store's device (the tables the kernels walk)"""
        return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.store.device)

    def _pw(self):
        """(the buffer that holds the trained values, the bf16 working copy of a master store or None)"""
        if self.master is not None:
            return self.master, self.store.data
        return self.store.data, None

    @property
    def _bf16_store(self) -> bool:
        """a bf16 store without a master: the one form whose parameter write rounds, stochastically on request"""
        return self.master is None and self.store.dtype == torch.bfloat16

    def _advance_seed(self):
        """one LCG step per optimizer step of a bf16 store (the other forms draw no rounding bits)"""
        if self._bf16_store:
            self.seed = (self.seed * SR_LCG_MUL + SR_LCG_ADD) & 0xFFFFFFFFFFFFFFFF

    def _name(self, p) -> str:
        return self._ptr2name[p.data_ptr()]

    def _flat(self, buf, name):
        """the elements of tensor `name` in a buffer indexed as the store, in the tensor's shape"""
        s = self.store.slots[name]
        return buf[s.offset:s.offset + s.numel].view(s.shape)

    # --- state_dict / load_state_dict: one walk over groups and parameters ------------------------------------------
    def _views(self, name) -> dict:
        """{state key: view of its buffer} of one tensor"""
        raise NotImplementedError

    def _has_state(self, name, gi) -> bool:
        """whether state_dict holds an entry for this tensor yet"""
        return True

    def _save_tensor(self, name, gi) -> dict:
        """the saved entry of one tensor: clones of its views; a subclass adds 'step' and the like"""
        return {k: v.clone() for k, v in self._views(name).items()}

    def _load_tensor(self, name, gi, st):
        """one tensor's saved entry into its views; a scalar stands for a constant tensor (tensor(0) for zeros)"""
        for k, v in self._views(name).items():
            src = torch.as_tensor(st[k]).to(device=v.device, dtype=v.dtype)
            v.copy_(src.expand(v.shape) if src.numel() == 1 else src.reshape(v.shape))

    def _saved_seed(self, sd):
        return sd.get("sr_seed")

    def _group_loaded(self, g):
        """checks after the keys of one group are restored"""

    def _loaded(self, fresh):
        """after the walk; fresh: the names of the tensors that had no saved state"""

    def state_dict(self):
        self.store.wait_params()
        state, groups, idx = {}, [], 0
        for gi, g in enumerate(self.param_groups):
            ids = []
            for p in g["params"]:
                name = self._name(p)
                if self._has_state(name, gi):
                    state[idx] = self._save_tensor(name, gi)
                ids.append(idx)
                idx += 1
            gd = {k: v for k, v in g.items() if k != "params"}
            gd["params"] = ids
            groups.append(gd)
        # the stochastic-rounding stream position, so that a resumed run rounds like an uninterrupted one
        return {"state": state, "param_groups": groups, "sr_seed": int(self.seed)}

    def load_state_dict(self, sd):
        self.store.wait_params()
        seed = self._saved_seed(sd)
        if seed is not None:
            self.seed = int(seed)
        fresh = []
        for gi, (g, gsd) in enumerate(zip(self.param_groups, sd["param_groups"])):
            for k, v in gsd.items():
                if k not in ("params", "sr_seed"):   # sr_seed: FusedProdigy's per-group copy of the top-level one
                    g[k] = tuple(v) if k in self.TUPLE_KEYS else v
            self._group_loaded(g)
            for p, pid in zip(g["params"], gsd["params"]):
                st = sd["state"].get(pid)
                if st:
                    self._load_tensor(self._name(p), gi, st)
                else:
                    fresh.append(self._name(p))
        self._loaded(fresh)


class OverlappedGradNorm:
    """clip_grad_norm_'s squared-norm pass spread over the backward.  Single process: gradient ranges of about
    `bucket_bytes` (whole tensors, reverse layout order = the order backward finishes them) are summed on the
    weight-gradient stream as soon as every tensor in the range has its gradient -- the stream then waits for
    the dgrad chain's position, so both streams' writes are ordered before the read.  clip_grad_norm_ then only
    folds the per-chunk sums into per-tensor ones in chunk order (otamd_grad_clip_finalize) instead of reading
    the whole gradient buffer (SDXL: 5.1 GB, ~0.9 ms) after backward.  The sums are fp64, one slot per chunk
    (no atomics: the same bits every run), and the coefficient is formed with torch's bf16 roundings exactly as
    otamd_grad_clip_coef does.  Ranges with a tensor that received no gradient are
    summed after finish_backward has zeroed it.  Data parallel (`reducer`): the norm must see the all-reduced
    gradients, so the ranges are the reducer's buckets and each is summed on the reducer's post stream right after
    its collective completes (trainer/ddp.py reduced_hooks); only the last bucket's sums follow the backward.
    OTAMD_NORM_OVERLAP=0 disables it."""

    def __init__(self, opt: FlatStoreOptimizer, bucket_bytes: int = 64 << 20, reducer=None):
        self.opt = opt
        self.dp = reducer is not None
        store = opt.store
        limit = max(1, bucket_bytes // store.grad.element_size())
        t_chunks: dict = {}
        for ci, ti in enumerate(opt._chunk_tensor):
            b, e = t_chunks.get(ti, (ci, ci))
            t_chunks[ti] = (min(b, ci), max(e, ci + 1))
        self.buckets = []   # (first chunk, end chunk, names)
        if self.dp:
            t_index = {n: ti for ti, n in enumerate(store.order)}
            for _, _, names in reducer.buckets:
                spans = [t_chunks[t_index[n]] for n in names if t_index[n] in t_chunks]
                self.buckets.append((min(b for b, _ in spans) if spans else None,
                                     max(e for _, e in spans) if spans else None, list(names)))
            self.armed = False
            self.ready = False
            reducer.reduced_hooks.append(self._on_reduced)
            return
        cur, c_lo, c_hi, size = [], None, None, 0
        for ti in reversed(range(len(store.order))):
            name = store.order[ti]
            n = store.slots[name].numel
            if cur and size + n > limit:
                self.buckets.append((c_lo, c_hi, cur))
                cur, size = [], 0
            if not cur:
                c_lo, c_hi = None, None
            if ti in t_chunks:   # a tensor with no norm chunks (numel 0) must not stretch the bucket's range
                b, e = t_chunks[ti]
                c_lo = b if c_lo is None else min(c_lo, b)
                c_hi = e if c_hi is None else max(c_hi, e)
            cur.append(name)
            size += n
        if cur:
            self.buckets.append((c_lo, c_hi, cur))
        self.bucket_of = {n: bi for bi, (_, _, names) in enumerate(self.buckets) for n in names}
        self.armed = False
        self.ready = False
        self._ev = torch.cuda.Event()
        store.ready_hooks.append(self._on_ready)

    def arm(self, update_step: bool):
        """before the backward of a step: only the update step's gradients are final."""
        self.armed = update_step
        self.ready = False
        self.pending = [len(b[2]) for b in self.buckets]
        self._seen = set()
        self.launched = [False] * len(self.buckets)   # every bucket's chunk slots are rewritten each armed step

    def _launch(self, bi, side):
        self.launched[bi] = True
        c0, c1, _ = self.buckets[bi]
        if c0 is None:   # only empty tensors: nothing to sum
            return
        opt = self.opt
        g = opt.store.grad
        dtype = opt._norm_dtype
        if side is not None:
            from ...module import streams as S
            S.defer_flush()   # the bucket's deferred split-K reduces (module/streams.py) before its norms
            self._ev.record(torch.cuda.current_stream())
            side.wait_event(self._ev)
            with torch.cuda.stream(side):
                _lib.check(_lib.lib().otamd_grad_sqnorm_chunks(g.data_ptr(), dtype, opt._chunks.data_ptr(), c0, c1,
                                                               opt._chunk_sq.data_ptr(), K.stream_handle()),
                           "otamd_grad_sqnorm_chunks")
        else:
            _lib.check(_lib.lib().otamd_grad_sqnorm_chunks(g.data_ptr(), dtype, opt._chunks.data_ptr(), c0, c1,
                                                           opt._chunk_sq.data_ptr(), K.stream_handle()),
                       "otamd_grad_sqnorm_chunks")

    def _on_reduced(self, bi):
        """data parallel: bucket bi holds the global sum (on the reducer's post stream, the current stream here)."""
        if self.armed:
            self._launch(bi, None)

    def _on_ready(self, names):
        if not self.armed:
            return
        pending, bucket_of = self.pending, self.bucket_of
        if _NORM_CHECK:   # debug: a gradient marked twice, or after its range was summed, would race the norm pass
            for n in names:
                if n in self._seen:
                    raise RuntimeError(f"overlapped grad norm: {n} marked ready twice in one step")
                if self.launched[bucket_of[n]]:
                    raise RuntimeError(f"overlapped grad norm: {n} marked ready after its range was summed")
                self._seen.add(n)
        for n in names:
            bi = bucket_of[n]
            pending[bi] -= 1
            if pending[bi] == 0 and not self.launched[bi]:
                from ...module import streams as S
                self._launch(bi, S.side_stream())

    def finish(self):
        """after finish_backward (streams joined, grads of untouched tensors zeroed): sum what is left."""
        if not self.armed:
            return
        for bi in range(len(self.buckets)):
            if not self.launched[bi]:
                if self.dp:   # every reducer bucket goes out in reducer.finish(), which runs before this
                    raise RuntimeError("overlapped grad norm: bucket %d was not all-reduced this step" % bi)
                self._launch(bi, None)
        # every chunk slot is rewritten on an armed step: the finalize never sees an earlier step's sums
        assert all(self.launched), "overlapped grad norm: a bucket was not summed this step"
        self.ready = True

    def take(self) -> bool:
        """True once per armed step whose sums are complete (consumed by clip_grad_norm_)."""
        r = self.ready
        self.ready = False
        self.armed = False
        return r
