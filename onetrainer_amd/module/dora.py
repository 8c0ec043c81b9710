"""DoRA (weight-decomposed LoRA, `lora_decompose`) for the HIP UNet.

Semantics of modules/module/LoRAModule.py:334-419 (DoRAModule), per adapted Linear / Conv2d, all fp32:
    Weff = W + (alpha / rank) * up.view(out, -1) @ down.view(r, -1)
    n    = ||Weff|| over every axis but the kept one (detached) + eps
    W'   = dora_scale * (Weff / n)
    y    = op(x, W', bias)               # bf16 autocast rounds W' once
The kept axis is the input-channel axis (dora_scale [1, in, 1, 1] / [1, in]) or, with `decompose_output_axis`, the
output-channel axis ([out, 1, 1, 1] / [out, 1]); eps = finfo(float32).eps with `norm_epsilon`, else 0; dora_scale is a
trained parameter initialised to the same norm of the base weight, key "<prefix>.<module>.dora_scale".

MI355X layout (not a translation): merge once per step, run the base graph, project the gradient.
  * one fp32 FlatParamStore holds lora_down, lora_up and dora_scale of every adapted module (the fused optimizers,
    the grad-norm, the DP buckets and EMA run over it as over the LoRA store);
  * W' of every adapted base GEMM lives in one bf16 buffer in base-store order (a fused q|k|v group is one span, the
    rows of members the layer filter leaves out are a copy of W), refreshed by ONE launch (kernels.dora_merge) at
    construction, after load_state_dict and after every optimizer step;
  * the model runs its plain base graph on W' (LinearFn / ConvFn, the attention paths unchanged): `DoraRef` has the
    functional.PRef duck type, its weight-gradient GEMM overwrites the matching span of a second bf16 buffer G, and
    `done()` queues the projection of G onto the adapter gradients; neighbouring sites go out together on the
    weight-gradient stream (kernels.dora_project), then their adapter slots are marked ready.
G is not inside the gradient buffer the split-K deferral is opened on (module/streams.defer_begin: the adapter
store's), so a split-K weight-gradient GEMM into G launches its reduce with the GEMM, in stream order before the
projection that reads it.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from .. import _lib
from .. import kernels as K
from . import streams as S
from .lora import discover_sites
from .param_store import FlatParamStore


class DoraRef:
    """functional.PRef duck type over one adapted base GEMM: `w` is its W' span, `g` the span of G that receives
    dL/dW', `params` the site's adapter parameters (so autograd sees a trainable input)."""
    __slots__ = ("wrapper", "site", "names", "w", "g", "params", "e0", "e1")
    trainable = True

    def __init__(self, wrapper, site, w, g, names, e0, e1):
        self.wrapper, self.site, self.w, self.g, self.names, self.e0, self.e1 = wrapper, site, w, g, names, e0, e1
        self.params = tuple(wrapper.store.params[n] for n in names)

    def acc(self) -> bool:
        return False   # G is overwritten every micro-step; accumulation happens in the projection's outputs

    def done(self):
        self.wrapper.project(self)


class AdapterStore(FlatParamStore):
    """the DoRA adapter store: projections still queued (DoRAWrapper.project) go out before the weight-gradient
    stream is joined and the unwritten gradients are zeroed"""
    flush_pending = None

    def finish_backward(self):
        if self.flush_pending is not None:
            self.flush_pending()
        super().finish_backward()


class DoRAWrapper:
    """LoRAModuleWrapper(model, prefix, config with lora_decompose, module_filter) for the HIP UNet."""
    # a projection launch serves the queued neighbouring sites together once they fill the part: one site alone is
    # 1-20 workgroups of 64 lines each on 256 CUs (measured: 794 per-site launch pairs took 613 ms of an SDXL step)
    PROJECT_BLOCKS = 1024

    def __init__(self, model, rank: int = 16, alpha: float = 1.0, module_filter=None, prefix: str = "lora_unet",
                 seed: int = 0, dtype=torch.float32, norm_epsilon: bool = True, decompose_output_axis: bool = False):
        if dtype != torch.float32:
            raise NotImplementedError("DoRA adapters are fp32 (lora_weight_dtype FLOAT_32)")
        self.model = self.unet = model
        self.rank, self.alpha, self.prefix = rank, float(alpha), prefix
        self.scale = self.alpha / rank
        self.norm_epsilon, self.output_axis = bool(norm_epsilon), bool(decompose_output_axis)
        self.eps = float(torch.finfo(torch.float32).eps) if norm_epsilon else 0.0
        base = model.store
        dev = torch.device(model.device)
        self.sites = sites = discover_sites(model, rank, self.scale, module_filter)
        self.site_of = {}
        for s in sites:
            for mname in s.group:
                self.site_of[mname] = s
            self.site_of[s.key] = s
        # fp32 store: per site the downs, the ups, then the scales (the LoRA store's order plus dora_scale)
        specs = []
        for s in sites:
            for mname in s.modules:
                dshape = (rank, s.cin) if s.kind == "linear" else (rank, s.k, s.k, s.cin)
                specs.append((f"{prefix}.{mname}.lora_down.weight", dshape, prefix))
            for mname, co in zip(s.modules, s.couts):
                specs.append((f"{prefix}.{mname}.lora_up.weight", (co, rank), prefix))
            for mname, co in zip(s.modules, s.couts):
                specs.append((f"{prefix}.{mname}.dora_scale", self._scale_shape(s, s.cin, co), prefix))
        self.store = AdapterStore(specs, dtype, dev)
        self.store.flush_pending = self.flush
        self._pending = None    # [e0, e1, slot names]: table entries whose G spans are written, projection not launched
        # W' and G: the sites' base spans, in base-store order, each at an 8-element boundary
        total, span_of = 0, {}
        for s in sites:
            wn = [g + ".weight" for g in s.group]
            base.view(wn)                                   # raises unless the group is adjacent in the base store
            b0, b1 = base.range_of(wn)
            span_of[s.key] = (total, b0, b1)
            total = (total + (b1 - b0) + 7) // 8 * 8
        self.wp = torch.zeros(max(total, 8), dtype=torch.bfloat16, device=dev)
        self.g = torch.zeros(max(total, 8), dtype=torch.bfloat16, device=dev)
        entries, self.refs, noff, cblk, rblk = [], {}, 0, 0, 0
        with torch.no_grad():
            for s in sites:
                off, b0, b1 = span_of[s.key]
                self.wp[off:off + b1 - b0].copy_(base.data[b0:b1])   # members without an adapter stay a copy of W
                e0 = len(entries)
                for mname, co in zip(s.modules, s.couts):
                    ws = base.slots[mname + ".weight"]
                    kept = co if self.output_axis else s.cin
                    entries.append(dict(w_off=ws.offset, wp_off=off + ws.offset - b0,
                                        down_off=self.store.slots[f"{prefix}.{mname}.lora_down.weight"].offset,
                                        up_off=self.store.slots[f"{prefix}.{mname}.lora_up.weight"].offset,
                                        scale_off=self.store.slots[f"{prefix}.{mname}.dora_scale"].offset,
                                        norm_off=noff, out=co, cin=s.cin, kk=s.k * s.k, rank=rank, cblk0=cblk,
                                        rblk0=rblk, s=self.scale))
                    noff += kept
                    cblk += (s.cin + 63) // 64
                    rblk += (co + 63) // 64
                names = [f"{prefix}.{m}.{leaf}" for leaf in ("lora_down.weight", "lora_up.weight", "dora_scale")
                         for m in s.modules]
                s.store, s.names = self.store, names
                s.params = tuple(self.store.params[n] for n in names)
                s.e0, s.e1, s.span = e0, len(entries), (off, b1 - b0)
        self.norms = torch.zeros(max(noff, 8), dtype=torch.float32, device=dev)
        self._host_table = (_lib.DoraEntry * max(len(entries), 1))()
        for i, e in enumerate(entries):
            for k, v in e.items():
                setattr(self._host_table[i], k, v)
        self._n_entries = len(entries)
        self._entry_of = {}
        i = 0
        for s in sites:
            for mname in s.modules:
                self._entry_of[mname] = i
                i += 1
        self._table = torch.frombuffer(bytearray(bytes(self._host_table)), dtype=torch.uint8).to(dev)
        if seed is not None:
            self.init_weights(seed)
        self.refresh()

    # ----- layout ---------------------------------------------------------------------------------
    def _scale_shape(self, s, cin, cout):
        """the reference's dora_scale shape with this store's channel counts (conv_in's input channels padded)"""
        tail = (1, 1) if (s.kind == "conv" or s.conv1x1) else ()
        return ((cout, 1) if self.output_axis else (1, cin)) + tail

    def ref_for(self, names, shape=None):
        """the DoraRef of the base GEMM over the weights `names` (a name or the list of a fused group), None when it
        carries no adapter"""
        names = [names] if isinstance(names, str) else list(names)
        if not names[0].endswith(".weight"):
            return None
        s = self.site_of.get(names[0][:-len(".weight")])
        if s is None:
            return None
        if tuple(n[:-len(".weight")] for n in names) != s.group:
            raise NotImplementedError(f"base GEMM {names} does not match the DoRA fusion group {s.group}")
        key = (s.key, shape)
        r = self.refs.get(key)
        if r is None:
            off, n = s.span
            if shape is None:   # the slot's shape; a fused group of Linears as one [sum out, in] matrix
                shape = self.model.store.slots[names[0]].shape
                if len(names) > 1:
                    shape = (n // shape[-1], shape[-1])
            r = self.refs[key] = DoraRef(self, s, self.wp[off:off + n].view(shape), self.g[off:off + n].view(shape),
                                         s.names, s.e0, s.e1)
        return r

    def module_views(self, module: str):
        """(W', G, n) views of one adapted module, in store layout (tests, tools)"""
        e = self._host_table[self._entry_of[module]]
        shape = self.model.store.slots[module + ".weight"].shape
        numel = math.prod(shape)
        kept = e.out if self.output_axis else e.cin
        return (self.wp[e.wp_off:e.wp_off + numel].view(shape), self.g[e.wp_off:e.wp_off + numel].view(shape),
                self.norms[e.norm_off:e.norm_off + kept])

    # ----- parameters -----------------------------------------------------------------------------
    def base_norm(self, module: str) -> torch.Tensor:
        """the norm of the base weight the reference initialises dora_scale to (DoRAModule.initialize_weights), in the
        store's scale shape"""
        s = self.site_of[module]
        w = self.model.store.params[module + ".weight"].detach().float()
        if self.output_axis:
            n = w.reshape(w.shape[0], -1).norm(dim=1)
        else:
            n = w.reshape(-1, w.shape[-1]).norm(dim=0)
        return n.reshape(self.store.slots[f"{self.prefix}.{module}.dora_scale"].shape)

    def init_weights(self, seed: int):
        """LoRAModule.initialize_weights (down ~ U(+-1/sqrt(fan_in)) with the LoRA wrapper's draws, up = 0; padded
        input channels stay zero) + DoRAModule.initialize_weights (dora_scale = the norm of the base weight)."""
        g = torch.Generator(device=self.unet.device).manual_seed(seed)
        with torch.no_grad():
            for s in self.sites:
                for m in s.modules:
                    p = self.store.params[f"{self.prefix}.{m}.lora_down.weight"]
                    bound = 1.0 / math.sqrt(s.cin_ref * s.k * s.k)
                    v = (torch.rand(p.shape, generator=g, device=p.device) * 2 - 1) * bound
                    if s.cin != s.cin_ref:
                        v[..., s.cin_ref:] = 0
                    p.copy_(v)
                    self.store.params[f"{self.prefix}.{m}.lora_up.weight"].zero_()
                    self.store.params[f"{self.prefix}.{m}.dora_scale"].copy_(self.base_norm(m))

    def refresh(self):
        """fp32 adapters -> n and bf16 W' of every adapted module: one launch; call after every update."""
        if self.store.device.type != "cuda" or not self._n_entries:
            return   # structure-only use on a CPU host (tests); the kernels need the GPU
        self.store.wait_params()
        K.dora_merge(self._table, self._host_table, self._n_entries, int(self.output_axis), self.eps,
                     self.model.store.data, self.store.data, self.norms, out=self.wp)

    def project(self, ref: DoraRef):
        """queue the projection of one base GEMM's G span (its weight-gradient GEMM is already on the weight-gradient
        stream).  Backward reaches the sites in reverse table order, so neighbours extend one entry range; the range
        is launched once it holds PROJECT_BLOCKS workgroups, when a site does not adjoin it, and at the end of the
        backward (AdapterStore.finish_backward)."""
        p = self._pending
        if p is not None and ref.e1 != p[0] and ref.e0 != p[1]:
            self.flush()
            p = None
        if p is None:
            p = self._pending = [ref.e0, ref.e1, []]
        p[0], p[1] = min(p[0], ref.e0), max(p[1], ref.e1)
        p[2].extend(ref.names)
        t = self._host_table
        if t[p[1] - 1].cblk0 + (t[p[1] - 1].cin + 63) // 64 - t[p[0]].cblk0 >= self.PROJECT_BLOCKS:
            self.flush()

    def flush(self):
        """G spans of the queued entries -> the fp32 gradients of their adapters, on the weight-gradient stream behind
        the GEMMs that wrote the spans; then the slots are ready (grad-norm chunks, DP buckets)."""
        p, self._pending = self._pending, None
        if p is None:
            return
        with S.wgrad_region(()):
            K.dora_project(self._table, self._host_table, self._n_entries, p[0], p[1], int(self.output_axis),
                           self.model.store.data, self.store.data, self.norms, self.g, out=self.store.grad,
                           accumulate=self.store.accumulate_into(p[2]))
        self.store.mark_ready(p[2])

    def parameters(self):
        return [p for _, p in self.store.named_parameters()]

    def num_parameters(self, reference_shapes: bool = True) -> int:
        n = 0
        for s in self.sites:
            cin = s.cin_ref if reference_shapes else s.cin
            for co in (s.couts_ref if reference_shapes else s.couts):
                n += self.rank * cin * s.k * s.k + co * self.rank + (co if self.output_axis else cin)
        return n

    def state_dict(self, grads: bool = False) -> dict:
        """reference key layout (LoRAModuleWrapper.state_dict with DoRAModule): NCHW conv weights, unpadded,
        + dora_scale in the reference's shape + alpha."""
        out = {}
        r = self.rank
        for s in self.sites:
            for m, co_ref in zip(s.modules, s.couts_ref):
                d = self.store.params[f"{self.prefix}.{m}.lora_down.weight"]
                u = self.store.params[f"{self.prefix}.{m}.lora_up.weight"]
                sc = self.store.params[f"{self.prefix}.{m}.dora_scale"]
                d, u, sc = (d.grad, u.grad, sc.grad) if grads else (d.detach(), u.detach(), sc.detach())
                if s.kind == "conv":
                    d = d[..., :s.cin_ref].permute(0, 3, 1, 2)
                    u = u[:co_ref].reshape(co_ref, r, 1, 1)
                elif s.conv1x1:
                    d = d.reshape(r, s.cin_ref, 1, 1)
                    u = u.reshape(co_ref, r, 1, 1)
                sc = sc[:co_ref] if self.output_axis else sc[:, :s.cin_ref]
                out[f"{self.prefix}.{m}.lora_down.weight"] = d.contiguous()
                out[f"{self.prefix}.{m}.lora_up.weight"] = u.contiguous()
                out[f"{self.prefix}.{m}.dora_scale"] = sc.contiguous()
                out[f"{self.prefix}.{m}.alpha"] = torch.tensor(self.alpha)
        return out

    def load_state_dict(self, sd: dict):
        """missing keys keep their init (LoRAModuleWrapper.load_state_dict): a plain-LoRA file leaves dora_scale at the
        norm of the base weight"""
        r = self.rank
        with torch.no_grad():
            for s in self.sites:
                for m, co_ref in zip(s.modules, s.couts_ref):
                    dk, uk = f"{self.prefix}.{m}.lora_down.weight", f"{self.prefix}.{m}.lora_up.weight"
                    sk = f"{self.prefix}.{m}.dora_scale"
                    if dk in sd:
                        d = sd[dk].to(self.store.device, torch.float32).clone()   # sd may hold views of this store
                        u = sd[uk].to(self.store.device, torch.float32).clone()
                        pd, pu = self.store.params[dk], self.store.params[uk]
                        if d.dim() == 4 and d.shape[2] > 1:
                            pd.zero_()
                            pd[..., :s.cin_ref].copy_(d.permute(0, 2, 3, 1))
                        else:
                            pd.copy_(d.reshape(pd.shape))
                        pu.zero_()
                        pu[:co_ref].copy_(u.reshape(co_ref, r))
                    if sk in sd:
                        ps = self.store.params[sk]
                        v = sd[sk].to(self.store.device, torch.float32).clone()
                        ps.zero_()
                        if self.output_axis:
                            ps[:co_ref].copy_(v.reshape((co_ref,) + tuple(ps.shape[1:])))
                        else:
                            ps[:, :s.cin_ref].copy_(v.reshape((1, s.cin_ref) + tuple(ps.shape[2:])))
        self.refresh()
