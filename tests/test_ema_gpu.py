"""The EMA of the trained weights on the GPU: the three kernel forms of csrc/ema.hip against the reference's own
EMAModuleWrapper (tests/golden/ema_steps.npz) and the NumPy restatement (tests/_oracle_ema.py), the argument contract
of the C ABI, and the trainer: step, scalar, backup, resume, periodic and final save.  Every comparison is bit
equality: the update has no reductions and no reassociation."""
import os
from pathlib import Path

import numpy as np
import pytest
import torch
from safetensors.torch import load_file

import _oracle_ema as OE
from _oracle_ema import build_store, shadow_bits, write_point
from onetrainer_amd import _lib
from onetrainer_amd import kernels as K
from onetrainer_amd.dataLoader.SyntheticDataLoader import synthetic_sdxl_batch
from onetrainer_amd.module import unet as U
from onetrainer_amd.module.ema import FlatStoreEMA
from onetrainer_amd.trainer.GenericTrainer import GenericTrainer
from onetrainer_amd.util import create
from onetrainer_amd.util.config.TrainConfig import TrainConfig
from onetrainer_amd.util.tensorboard import read_scalars

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "ema_steps.npz"
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _dtypes(form):
    """(shadow, parameters) torch dtypes of a kernel form"""
    return (BF16 if OE.shadow_is_bf16(form) else F32), (BF16 if OE.params_are_bf16(form) else F32)


def _dev(x, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(dtype)


def _host(t):
    """a flat device tensor as an fp32 array (bf16 widens exactly)"""
    return t.detach().float().cpu().numpy()


def _same_bits(form, got, want):
    return np.array_equal(OE.bits(form, got), OE.bits(form, want))


# ----- kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", list(OE.SCHEDULES))
@pytest.mark.parametrize("form", OE.FORMS)
def test_kernel_equals_reference(dev, golden, form, sched):
    """FlatStoreEMA on a device store, every step of both schedules against the reference's recorded shadow"""
    s = OE.SCHEDULES[sched]
    st = build_store("f32" if form == "f32" else "bf16", device=dev)
    ema = FlatStoreEMA(st, decay=s["decay"], update_step_interval=s["interval"], device=dev,
                       fp32_shadow=form == "mixed")
    assert ema.shadow.is_cuda and ema.shadow.dtype == _dtypes(form)[0]
    for k in range(s["steps"]):
        write_point(st, form, k + 1)
        assert ema.step(k) == OE.updates_at(k, s["interval"])
        got = shadow_bits(ema, form)
        for n, _ in OE.SHAPES:
            want = golden[f"{sched}/{form}/{k}/{n}"]
            want = want if want.dtype == np.uint16 else want.view(np.uint32)
            assert np.array_equal(OE.sample(got[n]), want), (sched, form, k, n)
    assert not ema.shadow[st.slots["one"].offset + 1:st.slots["seven"].offset].any()   # padding stays 0


@pytest.mark.parametrize("form", OE.FORMS)
def test_grid_stride_partial_second_sweep(dev, form):
    """about 1.1 sweeps of the capped grid: the grid-stride loop and its prefetch run a partial second pass"""
    et, pt = _dtypes(form)
    code = K.ema_form(torch.empty(0, dtype=et), torch.empty(0, dtype=pt))
    n = K.ema_sweep_elems(code) + 8 * 1000 + 8
    assert n % 8 == 0 and 1 << 20 < n < 1 << 26
    e0 = OE.values(11, n, 0, et == BF16)
    p = OE.values(11, n, 1, pt == BF16)
    e, pd = _dev(e0, et, dev), _dev(p, pt, dev)
    omd = OE.one_minus_decay(3, 0.9999)
    K.ema_update(e, pd, float(omd))
    want = OE.ema_update(form, e0, p, omd)
    got = _host(e)
    bad = np.flatnonzero(OE.bits(form, got) != OE.bits(form, want))
    assert bad.size == 0, (form, bad.size, bad[:8])
    assert torch.equal(pd, _dev(p, pt, dev))      # the parameters are only read


@pytest.mark.parametrize("form", OE.FORMS)
def test_sub_range_leaves_the_rest_untouched(dev, form):
    n, begin, end = 8 * 700, 8 * 3, 8 * 613
    et, pt = _dtypes(form)
    e0 = OE.values(23, n, 0, et == BF16)
    p = OE.values(23, n, 1, pt == BF16)
    e, pd = _dev(e0, et, dev), _dev(p, pt, dev)
    omd = OE.one_minus_decay(0, 0.75)
    K.ema_update(e, pd, float(omd), begin, end)
    got = _host(e)
    assert _same_bits(form, got[:begin], e0[:begin]) and _same_bits(form, got[end:], e0[end:])
    assert _same_bits(form, got[begin:end], OE.ema_update(form, e0[begin:end], p[begin:end], omd))
    assert not _same_bits(form, got[begin:end], e0[begin:end])


def test_argument_contract(dev):
    L = _lib.lib()
    e = torch.zeros(64, dtype=BF16, device=dev)
    p = torch.ones(64, dtype=BF16, device=dev)
    s = K.stream_handle()
    call = L.otamd_ema_range
    assert call(e.data_ptr(), p.data_ptr(), 0, 0, 0, 0.5, s) == _lib.OTAMD_OK           # empty: no launch
    assert call(e.data_ptr(), p.data_ptr(), 0, 16, 16, 0.5, s) == _lib.OTAMD_OK
    assert call(e.data_ptr() + 2, p.data_ptr(), 0, 0, 8, 0.5, s) == _lib.OTAMD_EINVAL   # misaligned pointers
    assert call(e.data_ptr(), p.data_ptr() + 8, 0, 0, 8, 0.5, s) == _lib.OTAMD_EINVAL
    assert call(e.data_ptr(), p.data_ptr(), 0, 0, 12, 0.5, s) == _lib.OTAMD_EINVAL      # not multiples of 8
    assert call(e.data_ptr(), p.data_ptr(), 0, 4, 16, 0.5, s) == _lib.OTAMD_EINVAL
    assert call(None, p.data_ptr(), 0, 0, 8, 0.5, s) == _lib.OTAMD_EINVAL               # null pointers
    assert call(e.data_ptr(), None, 0, 0, 8, 0.5, s) == _lib.OTAMD_EINVAL
    assert call(e.data_ptr(), p.data_ptr(), 3, 0, 8, 0.5, s) == _lib.OTAMD_EINVAL       # no such form
    assert call(e.data_ptr(), p.data_ptr(), 0, 16, 8, 0.5, s) == _lib.OTAMD_EINVAL      # end < begin
    assert call(e.data_ptr(), p.data_ptr(), 0, -8, 8, 0.5, s) == _lib.OTAMD_EINVAL
    torch.cuda.synchronize()
    assert not e.any() and bool((p == 1).all())                                          # nothing was launched
    with pytest.raises(ValueError):
        K.ema_update(e, p.float(), 0.5)                                                  # bf16 shadow of fp32 parameters
    with pytest.raises(ValueError):
        K.ema_update(e, p, 0.5, 0, 72)                                                   # past the buffers


# ----- trainer ---------------------------------------------------------------------------------------------------
VARIANTS = {"finetune_bf16": "bf16", "finetune_master": "f32", "lora": "f32"}   # variant -> kernel form
DECAY, INTERVAL, GA = 0.9999, 2, 2


def _cfg(tmp, variant, ema="GPU"):
    cfg = TrainConfig.default_values()
    cfg.batch_size = 2
    cfg.learning_rate = 1e-4
    cfg.learning_rate_warmup_steps = 4
    cfg.gradient_accumulation_steps = GA
    cfg.workspace_dir = str(tmp)
    cfg.backup_before_save = False
    if variant == "lora":
        cfg.training_method = "LORA"
        cfg.lora_rank, cfg.lora_alpha = 8, 8.0
        cfg.output_model_destination = str(Path(tmp) / "final.safetensors")
    else:
        cfg.output_model_format = "DIFFUSERS"
        cfg.output_model_destination = str(Path(tmp) / "final")
        if variant == "finetune_master":
            cfg.weight_dtype = "FLOAT_32"
    if ema is not None:
        cfg.ema, cfg.ema_decay, cfg.ema_update_step_interval = ema, DECAY, INTERVAL
    return cfg


def _trainer(cfg, dev, seed):
    model = create.create_model(cfg, dev, seed=seed, unet_config=U.tiny_sdxl_config())
    tr = GenericTrainer(cfg, model=model)
    tr.start()
    return tr


def _source(tr):
    """the flat buffer of trained values (what the EMA averages)"""
    st = tr.model.train_store
    return st.master if st.master is not None else st.data


def _weights(tr, dtype=None):
    """the model's weights as the savers write them (file layout), read from the store as it stands"""
    lora = tr.model.unet_lora
    sd = lora.state_dict() if lora is not None else tr.model.unet.state_dict()
    return {k: (v.to(dtype) if dtype is not None and v.is_floating_point() else v).detach().cpu().contiguous().clone()
            for k, v in sd.items()}


def _file_weights(path, variant, backup=False):
    if variant == "lora":
        return load_file(os.path.join(path, "lora", "lora.safetensors") if backup else path)
    return load_file(os.path.join(path, "unet", "diffusion_pytorch_model.safetensors"))


def _same_dict(a, b):
    if set(a) != set(b):
        return False
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape
               and torch.equal(a[k].reshape(-1).view(torch.uint8), b[k].reshape(-1).view(torch.uint8)) for k in a)


def _averaged_weights(tr, dtype):
    """the file-layout weights of the shadow: swapped into the store by hand, read, and swapped back"""
    ema = tr.model.ema
    ema.copy_ema_to(store_temp=True)
    assert torch.equal(_source(tr), ema.shadow)
    out = _weights(tr, dtype)
    ema.copy_temp_to()
    return out


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_trainer_ema(dev, tmp_path, variant):
    form = VARIANTS[variant]
    lora = variant == "lora"
    torch.manual_seed(0)
    batch = synthetic_sdxl_batch(2, 128, 128, dev, seed=1, te1_dim=48, te2_dim=48, pooled_dim=64)
    a = _trainer(_cfg(tmp_path, variant), dev, seed=3)
    ema, st = a.model.ema, a.model.train_store
    assert isinstance(ema, FlatStoreEMA) and ema.store is st and ema.shadow.is_cuda
    assert (st.master is not None) == (variant == "finetune_master")
    assert ema.shadow.dtype == _dtypes(form)[0] and _source(a).dtype == _dtypes(form)[1]
    a.tensorboard = a._open_scalar_log()
    want = _host(_source(a))                       # a fresh shadow is the parameters
    assert _same_bits(form, _host(ema.shadow), want)
    at_backup = None
    for g in range(8):
        a.train_step(batch)
        if (g + 1) % GA == 0 and OE.updates_at(g // GA, INTERVAL):     # micro-steps 3 and 7: update steps 1 and 3
            before = want
            want = OE.ema_update(form, want, _host(_source(a)), OE.one_minus_decay(g // GA, DECAY))
            assert not _same_bits(form, want, before)
        assert _same_bits(form, _host(ema.shadow), want), (variant, g)   # unchanged on every other micro-step
        if g == 3:
            path = a.backup()
            assert path and os.path.isfile(os.path.join(path, "ema", "ema.pt"))
            trained = _weights(a)
            assert _same_dict(_file_weights(path, variant, backup=True), trained)   # a backup holds the trained weights
            at_backup = ema.shadow.clone()
            # a periodic save holds the averaged weights and leaves the store as it was
            data, src = st.data.clone(), _source(a).clone()
            averaged = _averaged_weights(a, F32)
            assert not _same_dict(averaged, _weights(a, F32))
            saved = a.save(print_msg=False)
            assert saved and _same_dict(_file_weights(saved, variant), averaged)
            assert torch.equal(st.data.view(torch.uint8), data.view(torch.uint8))
            assert torch.equal(_source(a).view(torch.uint8), src.view(torch.uint8))
            assert ema.temp_stored_parameters is None
    a.tensorboard.flush()
    decays = [(r["step"], r["value"]) for r in read_scalars(a.tensorboard.log_dir) if r["tag"] == "ema_decay"]
    assert decays == [(g, OE.current_decay(g // GA, DECAY)) for g in (1, 3, 5, 7)]
    shadow_a, params_a = ema.shadow.clone(), _source(a).clone()

    # resume from the backup taken after micro-step 3 and run on: the same shadow, bit for bit
    cfg_b = _cfg(tmp_path, variant)
    cfg_b.continue_last_backup = True
    b = _trainer(cfg_b, dev, seed=3 if lora else 7)
    assert b.model.train_progress.global_step == 4 and getattr(b.model, "ema_state_dict", None) is None
    assert torch.equal(b.model.ema.shadow.view(torch.uint8), at_backup.view(torch.uint8))
    for _ in range(4):
        b.train_step(batch)
    assert torch.equal(_source(b).view(torch.uint8), params_a.view(torch.uint8))
    assert torch.equal(b.model.ema.shadow.view(torch.uint8), shadow_a.view(torch.uint8))

    # the final model is the averaged one
    averaged = _averaged_weights(a, F32)
    final = a.end()
    assert final and _same_dict(_file_weights(final, variant), averaged)
    assert torch.equal(_source(a), ema.shadow)


def test_ema_off_is_the_run_without_the_fields(dev, tmp_path):
    """`ema: OFF` against a config that never names the EMA fields: no EMA object, no ema/ directory, the same
    trained bits"""
    batch = synthetic_sdxl_batch(2, 128, 128, dev, seed=1, te1_dim=48, te2_dim=48, pooled_dim=64)
    base = {"batch_size": 2, "learning_rate": 1e-4, "learning_rate_warmup_steps": 4, "gradient_accumulation_steps": GA}
    runs = []
    for name, extra in (("off", {"ema": "OFF", "ema_decay": DECAY, "ema_update_step_interval": 1}), ("absent", {})):
        cfg = TrainConfig.default_values().from_dict({**base, **extra, "workspace_dir": str(tmp_path / name)})
        tr = _trainer(cfg, dev, seed=3)
        assert tr.model.ema is None
        for _ in range(4):
            tr.train_step(batch)
        path = tr.backup()
        assert path and not os.path.exists(os.path.join(path, "ema"))
        runs.append(tr.model.train_store.data.clone())
    assert torch.equal(runs[0].view(torch.uint8), runs[1].view(torch.uint8))
