"""Exponential moving average of the trained weights on one flat shadow buffer.

Carries the contract of the reference's EMAModuleWrapper (modules/module/EMAModule.py:6-86) for a FlatParamStore:
the warm-up decay schedule and the update-interval gate (:31-43), the update `ema += (1 - decay) * (p - ema)` with
each torch op's rounding (:44-54), the swap of the averaged weights into the model around a save (:63-75) and the
state dict (:77-86).  The reference keeps one tensor per parameter and runs three torch ops per tensor in a Python
loop; here the shadow is one flat buffer with the store's layout and the update is one launch (csrc/ema.hip).

Shadow dtype.  The reference clones the parameters, so a bf16 store gets a bf16 shadow; that is the default here, with
identical bits.  `fp32_shadow` keeps an fp32 shadow of a bf16 store instead (what the reference computes after
`ema.to(device, dtype=torch.float32)`): at decay 0.9999 most increments of a bf16 shadow are below half an ulp and
round away.  An fp32 store (LoRA) and a master store (the shadow follows `store.master`) are fp32 either way.

EMAMode.CPU keeps the shadow on the host and updates it with the reference's own sequence on a host copy of the flat
parameters (sub_, mul_, add_): off the hot path, the same bits.

State.  `state_dict()` is {"decay", "ema_parameters": [one tensor per parameter]} like the reference's, but the
tensors are in this build's parameter order (model.parameters.parameters(), the store's layout order) and in the
store's shapes (NHWC convolution weights, padded channels): like optimizer.pt, ema.pt round-trips within this build
and is not the reference's file.
"""
from __future__ import annotations

import torch

from .. import kernels as K


class FlatStoreEMA:
    def __init__(self, store, decay: float = 0.9999, update_step_interval: int = 1, device=None,
                 fp32_shadow: bool = False):
        self.store = store
        self.decay = decay
        self.update_step_interval = update_step_interval
        self.device = torch.device(device) if device is not None else store.device
        store.wait_params()
        shadow = self._source().detach().clone().to(self.device)
        if fp32_shadow:
            shadow = shadow.float()
        self.shadow = shadow
        self.temp_stored_parameters = None

    def _source(self) -> torch.Tensor:
        """the flat buffer that holds the trained values: the fp32 master if the store has one, else `data`."""
        return self.store.master if self.store.master is not None else self.store.data

    # ----- schedule (EMAModule.py:31-43) --------------------------------------------------------------------
    def get_current_decay(self, optimization_step) -> float:
        return min((1 + optimization_step) / (10 + optimization_step), self.decay)

    def updates_at(self, optimization_step) -> bool:
        return (optimization_step + 1) % self.update_step_interval == 0

    @torch.no_grad()
    def step(self, optimization_step, begin: int = 0, end: int | None = None) -> bool:
        """the update of optimizer step `optimization_step` (0-based), if the interval lets it through; [begin, end)
        restricts it to an element range of the store (multiples of 8).  Returns whether the shadow was updated."""
        one_minus_decay = 1 - self.get_current_decay(optimization_step)
        if not self.updates_at(optimization_step):
            return False
        self.store.wait_params()
        p = self._source()
        if self.shadow.is_cuda:
            K.ema_update(self.shadow, p, one_minus_decay, begin, end)
            return True
        # host shadow: in-place on a host copy of the parameters, as the reference does across devices; an fp32
        # shadow of bf16 parameters widens the copy first (exact), which is what torch's promotion computes
        end = p.numel() if end is None else end
        copy = p[begin:end].detach().to(self.shadow.device, self.shadow.dtype, copy=True)
        e = self.shadow[begin:end]
        copy.sub_(e)
        copy.mul_(one_minus_decay)
        e.add_(copy)
        return True

    # ----- swapping weights (EMAModule.py:63-75) ------------------------------------------------------------
    @torch.no_grad()
    def _write_store(self, flat: torch.Tensor):
        st = self.store
        if st.master is not None:   # as FlatParamStore.write: the working copy is the master's bf16 cast
            st.master.copy_(flat)
            st.data.copy_(st.master)
        else:
            st.data.copy_(flat)

    def copy_ema_to(self, store_temp: bool = True) -> None:
        """the averaged weights into the store; store_temp keeps the trained ones on the host for copy_temp_to."""
        self.store.wait_params()
        if store_temp:
            self.temp_stored_parameters = self._source().detach().to("cpu", copy=True)
        self._write_store(self.shadow)

    def copy_temp_to(self) -> None:
        self.store.wait_params()
        self._write_store(self.temp_stored_parameters)
        self.temp_stored_parameters = None

    # ----- state (EMAModule.py:77-86) -----------------------------------------------------------------------
    def _views(self):
        st = self.store
        for n in st.order:
            s = st.slots[n]
            yield n, self.shadow[s.offset:s.offset + s.numel].view(s.shape)

    def state_dict(self) -> dict:
        return {"decay": self.decay, "ema_parameters": [v.clone() for _, v in self._views()]}

    @torch.no_grad()
    def load_state_dict(self, state_dict: dict) -> None:
        self.decay = self.decay if self.decay else state_dict.get("decay", self.decay)   # a configured decay wins
        saved = state_dict.get("ema_parameters")
        views = list(self._views())
        if saved is None or len(saved) != len(views):
            raise ValueError(f"ema state: {0 if saved is None else len(saved)} tensors for {len(views)} parameters")
        for (n, v), t in zip(views, saved):
            if tuple(t.shape) != tuple(v.shape):
                raise ValueError(f"ema state: {n} has shape {tuple(t.shape)}, the store's is {tuple(v.shape)}")
            v.copy_(t)
