"""NumPy restatement of the EMA update the reference runs (modules/module/EMAModule.py:31-54) and the hashed inputs of
the EMA tests.  Pinned to the reference by tests/test_ema_oracle.py through tests/golden/ema_steps.npz (written by
tests/golden/make_ema_golden.py from the reference's own EMAModuleWrapper); the GPU tests compare the kernels of
csrc/ema.hip with it, bit for bit: the update has no reductions and no reassociation.

Three forms.  "f32": fp32 shadow of fp32 parameters, three fp32 roundings.  "bf16": bf16 shadow of bf16 parameters,
every torch op's result rounded to bf16.  "mixed": fp32 shadow of bf16 parameters (the reference after
ema.to(device, dtype=torch.float32)): the parameters widen exactly, then as "f32".  Arrays are fp32 throughout;
bf16 tensors are fp32 arrays of bf16-exact values.
"""
import numpy as np
import torch

from onetrainer_amd.module.param_store import FlatParamStore
from oracle import adamw as OA

F = np.float32

FORMS = ("f32", "bf16", "mixed")
# 1, 7, 8, 9: around the kernels' 8-element granule; 4099: several granules and a ragged end; one 2-D tensor
SHAPES = [("one", (1,)), ("seven", (7,)), ("eight", (8,)), ("nine", (9,)), ("vec", (4099,)), ("mat", (5, 13))]
# "warm": the warm-up term (1 + s) / (10 + s) crosses the cap 0.75 at s = 27; "gate": the interval lets steps 2, 5, 8
# through, each with its warm-up decay
SCHEDULES = {"warm": dict(decay=0.75, interval=1, steps=32), "gate": dict(decay=0.9999, interval=3, steps=9)}
SAMPLE = 1024   # the golden keeps at most this many elements of a tensor (evenly strided)


def shadow_is_bf16(form):
    return form == "bf16"


def params_are_bf16(form):
    return form != "f32"


def current_decay(step, decay):
    return min((1 + step) / (10 + step), decay)


def updates_at(step, interval):
    return (step + 1) % interval == 0


def one_minus_decay(step, decay):
    """Python's double 1 - decay, narrowed to fp32 as torch applies a Python scalar to a float tensor"""
    return F(1 - current_decay(step, decay))


def ema_update(form, e, p, omd):
    """e + omd * (p - e) with the roundings of the three torch ops sub, mul (by a scalar), add_"""
    e, p, omd = np.asarray(e, F), np.asarray(p, F), F(omd)
    if form == "bf16":
        d = OA.rbf(p - e)
        d = OA.rbf(omd * d)
        return OA.rbf(e + d)
    d = p - e
    d = omd * d
    return (e + d).astype(F)


def _hash16(seed, n, offset=0):
    return OA.sr_bits(seed, np.arange(offset, offset + n, dtype=np.uint64)).astype(np.int64)


def values(seed, n, k, bf16):
    """n deterministic test values of trajectory point k (hashed, not stored; IEEE basic operations only, so every
    host builds the same bits): magnitudes 2^-20 .. 2^10 (1e-6 .. 1e3) of either sign moving by up to 12.5 % from
    point to point, and per 16 elements one +0, one -0 and one value that never moves (p == e at every step)."""
    h = _hash16(seed, n)
    expo = (h % 31) - 20
    mant = F(1) + (_hash16(seed + 101, n) / 65536.0).astype(F)
    sign = np.where(_hash16(seed + 211, n) & 1, F(-1), F(1))
    base = (sign * np.ldexp(mant, expo.astype(np.int32))).astype(F)
    wobble = ((_hash16(seed + 307 + 13 * k, n) - 32768) / 65536.0).astype(F) * F(0.25)
    x = (base * (F(1) + wobble)).astype(F)
    kind = (np.arange(n) + seed) % 16
    x = np.where(kind == 5, base, x)
    x = np.where(kind == 3, F(0.0), x)
    x = np.where(kind == 11, F(-0.0), x)
    return OA.rbf(x) if bf16 else x.astype(F)


def _seed(name):
    return 3000 + sum(map(ord, name))


def param(name, shape, k, bf16):
    """the parameters at trajectory point k: k = 0 initialises the shadow, optimizer step s sees point s + 1"""
    return values(_seed(name), int(np.prod(shape)), k, bf16).reshape(shape)


def run(form, sched, params=None):
    """the shadow after every step of a schedule: [{name: fp32 array}] (unchanged on a gated-out step)"""
    s = SCHEDULES[sched]
    bf = params_are_bf16(form)
    params = params or (lambda n, sh, k: param(n, sh, k, bf))
    e = {n: params(n, sh, 0).copy() for n, sh in SHAPES}
    out = []
    for k in range(s["steps"]):
        if updates_at(k, s["interval"]):
            omd = one_minus_decay(k, s["decay"])
            e = {n: ema_update(form, e[n], params(n, sh, k + 1), omd) for n, sh in SHAPES}
        out.append({n: v.copy() for n, v in e.items()})
    return out


def sample(x):
    x = np.asarray(x).reshape(-1)
    return x[::max(1, -(-x.size // SAMPLE))]


def bits(form, x):
    """what the golden stores and the tests compare: fp32 values as uint32 patterns, bf16 as uint16 patterns"""
    x = np.ascontiguousarray(x, F)
    return OA.f32_to_bf16_bits(x) if shadow_is_bf16(form) else x.view(np.uint32)


# ----- torch-side helpers shared by the CPU and GPU tests ----------------------------------------------------------
def build_store(form, k=0, device="cpu"):
    """a FlatParamStore with SHAPES holding trajectory point k: fp32 ("f32"), bf16, or ("master") bf16 behind an
    fp32 master"""
    master = form == "master"
    dtype = torch.float32 if form == "f32" else torch.bfloat16
    store = FlatParamStore([(n, sh, "g") for n, sh in SHAPES], dtype, torch.device(device), master=master)
    write_point(store, form, k)
    return store


def write_point(store, form, k):
    for n, sh in SHAPES:
        store.write(n, torch.from_numpy(param(n, sh, k, form not in ("f32", "master"))).to(store.device))


def shadow_bits(ema, form):
    """{name: bit patterns of the tensor's shadow} in the golden's encoding"""
    out = {}
    for n, v in ema._views():
        v = v.detach().cpu().contiguous()
        out[n] = (v.view(torch.int16).numpy().astype(np.uint16) if v.dtype == torch.bfloat16
                  else v.numpy().view(np.uint32)).reshape(-1)
    return out
