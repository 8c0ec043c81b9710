"""Flat parameter / gradient store.

All trainable tensors of a model live as views of ONE flat buffer (params) with a twin flat
buffer for gradients, each tensor at a 16-byte aligned offset.  Consequences:
  * the fused AdamW (csrc/adamw.hip) is a single pass over the flat buffers (14 B/param bf16);
  * data-parallel gradient buckets are contiguous slices of the flat grad buffer (trainer/ddp.py);
  * weights that one GEMM consumes together (to_q|to_k|to_v, to_k|to_v) are adjacent, so the
    fused projection weight and its gradient are plain views -- no concat, no split.
Backward kernels write weight gradients straight into `grad` views (overwrite on the first
micro-step of an accumulation window, accumulate afterwards) and call `mark_ready`, which feeds
the DP reducer; autograd never materialises or accumulates parameter gradients.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch


class W8Ref:
    """A frozen e4m3 Linear weight (weight_dtype FLOAT_8, LinearFp8.py): `w8` uint8 [N, K] of e4m3 bytes and `scale`
    fp32 [N], one entry per row, so the weights one GEMM consumes together (to_q|to_k|to_v) are one W8Ref whose rows
    carry their member's scalar.  Never trainable: there is no weight gradient."""
    __slots__ = ("w8", "scale")

    def __init__(self, w8: torch.Tensor, scale: torch.Tensor):
        self.w8, self.scale = w8, scale

    @property
    def shape(self):
        return self.w8.shape

    @classmethod
    def quantize(cls, members) -> "W8Ref":
        """members: the bf16 / fp32 [n_i, K] weights of one (fused) GEMM, quantised on the device one by one
        (kernels.quantize_fp8: each with its own per-tensor scale) into one buffer"""
        from .. import kernels as K
        rows, k = sum(m.shape[0] for m in members), members[0].shape[1]
        w8 = torch.empty((rows, k), dtype=torch.uint8, device=members[0].device)
        scale = torch.empty(rows, dtype=torch.float32, device=members[0].device)
        r0 = 0
        for m in members:
            K.quantize_fp8(m.contiguous(), out=w8[r0:r0 + m.shape[0]], scale_rows=scale[r0:r0 + m.shape[0]])
            r0 += m.shape[0]
        return cls(w8, scale)

    def dequantized(self) -> torch.Tensor:
        """the bf16 weight the kernels multiply by: weight.to(bf16).mul_(scale) of LinearFp8.forward"""
        return self.w8.view(torch.float8_e4m3fn).to(torch.bfloat16) * self.scale.to(torch.bfloat16)[:, None]


def fp8_eligible(shape) -> bool:
    """a Linear weight [N, K] the e4m3 GEMMs take (csrc/gemm_w8.hip): K in 16-groups, N in 8-groups"""
    return len(shape) == 2 and shape[1] % 16 == 0 and shape[0] % 8 == 0


@dataclass
class Slot:
    name: str
    shape: tuple
    offset: int
    numel: int
    group: str


class FlatParamStore:
    def __init__(self, specs, dtype, device, align_bytes=16, trainable=True, master=False, fp8=()):
        """specs: iterable of (name, shape, group) in layout order.  trainable=False: a frozen base
        (LoRA training, unet.requires_grad_(False) in StableDiffusionXLLoRASetup.py:78-86): no grad
        buffer, parameters do not require grad, backward kernels skip its weight gradients.
        master=True: fp32 master weights (weight_dtype FLOAT_32, TrainConfig.py:782) behind the bf16 working copy
        `data` the kernels read -- `master` holds the trained values, `data` their round-to-nearest bf16 cast (what
        autocast feeds every GEMM, dtype_util.py:28-49); gradients stay bf16 (autocast's weight gradients are bf16
        GEMM results cast to fp32, so bf16 holds them exactly)."""
        esz = torch.tensor([], dtype=dtype).element_size()
        al = max(8, align_bytes // esz)   # >= 8 elements: the grad-norm kernel reads 8-wide chunks
        self.dtype, self.device = dtype, device
        self.slots: dict[str, Slot] = {}
        self.order: list[str] = []
        self.fp8_rows: dict[str, int] = {}   # fp8 weight -> its first row in scale_rows
        fp8 = set(fp8)
        if fp8 and trainable:
            raise ValueError("fp8 weights belong to a frozen store")
        off = off8 = rows8 = 0
        for name, shape, group in specs:
            n = 1
            for s in shape:
                n *= int(s)
            if name in fp8:   # n is a multiple of 16 bytes (fp8_eligible): adjacent weights stay adjacent
                if not fp8_eligible(shape):
                    raise ValueError(f"{name} {tuple(shape)}: not a Linear weight the e4m3 GEMMs take")
                self.slots[name] = Slot(name, tuple(int(s) for s in shape), off8, n, group)
                self.fp8_rows[name] = rows8
                off8, rows8 = off8 + n, rows8 + int(shape[0])
            else:
                off = (off + al - 1) // al * al
                self.slots[name] = Slot(name, tuple(int(s) for s in shape), off, n, group)
                off += n
            self.order.append(name)
        self.numel = (off + al - 1) // al * al
        self.trainable = trainable
        self.data8 = torch.zeros(off8, dtype=torch.uint8, device=device) if fp8 else None
        self.scale_rows = torch.zeros(rows8, dtype=torch.float32, device=device) if fp8 else None
        self.data = torch.zeros(self.numel, dtype=dtype, device=device)
        if master and (not trainable or dtype != torch.bfloat16):
            raise ValueError("fp32 master weights back a trainable bf16 store")
        self.master = torch.zeros(self.numel, dtype=torch.float32, device=device) if master else None
        self.grad = torch.zeros(self.numel, dtype=dtype, device=device) if trainable else None
        self._params: dict[str, torch.nn.Parameter] = {}
        for name in self.order:
            s = self.slots[name]
            buf = self.data8 if name in self.fp8_rows else self.data
            p = torch.nn.Parameter(buf[s.offset:s.offset + s.numel].view(s.shape), requires_grad=trainable)
            if trainable:
                p.grad = self.grad[s.offset:s.offset + s.numel].view(s.shape)
            self._params[name] = p
        self._written: set[str] = set()
        self.accumulating = False          # True on micro-steps after the first of a GA window
        self.ready_hooks = []              # callables(names) -> None (DP reducer)
        # optimizer update in flight on another stream (util/optimizer/adamw_fused.py): [(end element,
        # event)] in layout order; a consumer of element range [.., end) waits for the events up to it
        self.update_events: list | None = None
        self._waited = 0

    # ----- views -------------------------------------------------------------------------------
    @property
    def params(self) -> dict:
        """name -> parameter view.  A reader that takes weights from here (or from view()) rather than
        through PRef.w is ordered after an optimizer update still in flight on its own stream
        (util/optimizer/adamw_fused.py overlap): it waits for every pending chunk."""
        if self.update_events is not None:
            self.wait_params()
        return self._params

    def view(self, names, shape=None, grad=False):
        """contiguous view spanning `names` (which must be adjacent without padding); a weight view
        waits for the optimizer chunks covering it when an update is in flight."""
        if isinstance(names, str):
            names = [names]
        first = self.slots[names[0]]
        end = first.offset
        for n in names:
            s = self.slots[n]
            if s.offset != end:
                raise ValueError(f"parameters {names} are not adjacent in the flat store")
            end += s.numel
        n8 = sum(n in self.fp8_rows for n in names)
        if n8 and n8 != len(names):
            raise ValueError(f"parameters {names} mix fp8 and bf16 weights")
        buf = self.grad if grad else self.data
        if buf is None:
            return None
        if n8:
            w8 = self.data8[first.offset:end].view(shape if shape is not None else first.shape)
            r0 = self.fp8_rows[names[0]]
            return W8Ref(w8, self.scale_rows[r0:r0 + w8.shape[0]])
        if not grad and self.update_events is not None:
            self.wait_params(end)
        v = buf[first.offset:end]
        if shape is not None:
            v = v.view(shape)
        elif len(names) == 1:
            v = v.view(first.shape)
        return v

    def value(self, name):
        """the trained value of one tensor (store layout): the fp32 master view, else the parameter view."""
        s = self.slots[name]
        if name in self.fp8_rows:   # what the kernels multiply by (bf16)
            return self.view(name).dequantized()
        if self.master is not None:
            return self.master[s.offset:s.offset + s.numel].view(s.shape)
        return self.params[name].detach()

    @torch.no_grad()
    def write(self, name, value):
        """set one tensor (store layout); with master weights the fp32 value goes to the master and the working
        copy takes its bf16 cast."""
        s = self.slots[name]
        if name in self.fp8_rows:   # LinearFp8.quantize, on the device, as the weight is loaded
            from .. import kernels as K
            v = value.to(self.device)
            v = v if v.dtype in (torch.bfloat16, torch.float32) else v.float()
            ref = self.view(name)
            K.quantize_fp8(v.reshape(s.shape).contiguous(), out=ref.w8, scale_rows=ref.scale)
            return
        if self.master is not None:
            self.wait_params()
            mv = self.master[s.offset:s.offset + s.numel].view(s.shape)
            mv.copy_(value)
            self.data[s.offset:s.offset + s.numel].view(s.shape).copy_(mv)
        else:
            self.params[name].copy_(value)

    def range_of(self, names):
        first = self.slots[names[0]]
        last = self.slots[names[-1]]
        return first.offset, last.offset + last.numel

    # ----- asynchronous optimizer updates ------------------------------------------------------------
    def set_update_events(self, events):
        self.update_events = events or None
        self._waited = 0

    def wait_params(self, end: int | None = None):
        """make the current stream wait for the optimizer chunks covering elements [0, end) (all when
        end is None).  Forward order = layout order, so a forward that reaches layer L waits only for the
        chunks up to L's weights; the rest of the update keeps running beside it."""
        ev = self.update_events
        if ev is None:
            return
        cur = torch.cuda.current_stream(self.device)
        while self._waited < len(ev):
            e_end, e = ev[self._waited]
            cur.wait_event(e)
            self._waited += 1
            if end is not None and e_end >= end:
                break
        if self._waited >= len(ev):
            self.update_events = None

    # ----- gradient bookkeeping -----------------------------------------------------------------
    def accumulate_into(self, names) -> bool:
        """True if a backward kernel must add into the grad view (GA window), else overwrite."""
        return self.accumulating

    def mark_ready(self, names):
        self._written.update(names)
        for h in self.ready_hooks:
            h(names)

    def begin_backward(self):
        self.wait_params()   # backward overwrites the gradients the optimizer chunks read
        self._written.clear()
        if self.device.type == "cuda":
            from .streams import defer_begin
            defer_begin(self.grad if self.trainable else None)   # the gradient GEMMs' split-K reduces go out grouped

    def finish_backward(self):
        """join the weight-gradient stream, then zero the grads of parameters that received none
        this micro-step (overwrite semantics)."""
        if self.device.type == "cuda":
            from .streams import defer_end, join
            defer_end()      # the pending grouped split-K reduces, before anything reads the gradients
            join()
        if self.trainable and not self.accumulating:
            for n in self.order:
                if n not in self._written:
                    s = self.slots[n]
                    self.grad[s.offset:s.offset + s.numel].zero_()

    def named_parameters(self):
        return [(n, self._params[n]) for n in self.order]

    def group_ranges(self):
        """{group: (begin, end)} element ranges; groups must be contiguous in layout order."""
        out = {}
        for n in self.order:
            s = self.slots[n]
            b, e = out.get(s.group, (s.offset, s.offset + s.numel))
            out[s.group] = (min(b, s.offset), max(e, s.offset + s.numel))
        return out
