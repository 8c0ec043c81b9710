"""CPU checks of the EMA of the trained weights (module/ema.py): the NumPy restatement of the three roundings
(tests/_oracle_ema.py) and FlatStoreEMA's host path against the reference's own EMAModuleWrapper recorded in
tests/golden/ema_steps.npz, bit for bit; the decay schedule and the interval gate; the state dict; the weight swap
around a save; the config fields and the factory.  No tolerance anywhere: the update has no reductions."""
from pathlib import Path

import numpy as np
import pytest
import torch

import _oracle_ema as OE
from _oracle_ema import build_store, shadow_bits, write_point
from onetrainer_amd.module.ema import FlatStoreEMA
from onetrainer_amd.util import create
from onetrainer_amd.util.config.TrainConfig import TrainConfig

GOLDEN = Path(__file__).resolve().parent / "golden" / "ema_steps.npz"
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("sched", list(OE.SCHEDULES))
@pytest.mark.parametrize("form", OE.FORMS)
def test_restatement_equals_reference(golden, form, sched):
    steps = OE.run(form, sched)
    assert len(steps) == OE.SCHEDULES[sched]["steps"]
    for k, rec in enumerate(steps):
        for n, _ in OE.SHAPES:
            want = golden[f"{sched}/{form}/{k}/{n}"]
            want = want if want.dtype == np.uint16 else want.view(np.uint32)
            assert np.array_equal(OE.sample(OE.bits(form, rec[n])), want), (sched, form, k, n)


def test_inputs_cover_the_hard_values():
    for bf in (False, True):
        x = np.concatenate([OE.param(n, sh, 1, bf).reshape(-1) for n, sh in OE.SHAPES])
        x0 = np.concatenate([OE.param(n, sh, 0, bf).reshape(-1) for n, sh in OE.SHAPES])
        assert np.any((x == 0) & ~np.signbit(x)) and np.any((x == 0) & np.signbit(x))      # +0 and -0
        assert np.any((x == x0) & (x != 0)) and np.any(x != x0)                              # p == e, and not
        a = np.abs(x[x != 0])
        assert a.min() < 2e-6 and a.max() > 1e3 / 2 and np.all(a > 1e-30) and np.all(np.isfinite(x))


def test_decay_schedule_and_gate():
    st = build_store("f32")
    ema = FlatStoreEMA(st, decay=0.75, update_step_interval=1, device=CPU)
    for s in (0, 1, 26, 27, 28, 1000):
        assert ema.get_current_decay(s) == min((1 + s) / (10 + s), 0.75)
    assert ema.get_current_decay(26) == 27 / 36 and ema.get_current_decay(27) == 0.75   # the cap, reached at s = 27
    gated = FlatStoreEMA(st, decay=0.9999, update_step_interval=3, device=CPU)
    write_point(st, "f32", 1)
    before = gated.shadow.clone()
    ran = [gated.step(s) for s in range(9)]
    assert ran == [False, False, True] * 3
    assert not torch.equal(before, gated.shadow)
    idle = FlatStoreEMA(st, decay=0.9999, update_step_interval=3, device=CPU)
    write_point(st, "f32", 2)
    before = idle.shadow.clone()
    assert not idle.step(0) and not idle.step(1) and torch.equal(before, idle.shadow)


@pytest.mark.parametrize("sched", list(OE.SCHEDULES))
@pytest.mark.parametrize("form", OE.FORMS)
def test_cpu_mode_equals_reference(golden, form, sched):
    s = OE.SCHEDULES[sched]
    st = build_store("f32" if form == "f32" else "bf16")
    ema = FlatStoreEMA(st, decay=s["decay"], update_step_interval=s["interval"], device=CPU,
                       fp32_shadow=form == "mixed")
    assert ema.shadow.dtype == (torch.bfloat16 if form == "bf16" else torch.float32)
    for k in range(s["steps"]):
        write_point(st, form, k + 1)
        ema.step(k)
        got = shadow_bits(ema, form)
        for n, _ in OE.SHAPES:
            want = golden[f"{sched}/{form}/{k}/{n}"]
            want = want if want.dtype == np.uint16 else want.view(np.uint32)
            assert np.array_equal(OE.sample(got[n]), want), (sched, form, k, n)
    assert not ema.shadow[st.slots["one"].offset + 1:st.slots["seven"].offset].any()   # padding stays 0


def test_master_store_cpu_mode_follows_the_master():
    st = build_store("master")
    ema = FlatStoreEMA(st, decay=0.75, update_step_interval=1, device=CPU)
    assert ema.shadow.dtype == torch.float32 and torch.equal(ema.shadow, st.master)
    want = {n: OE.param(n, sh, 0, False) for n, sh in OE.SHAPES}
    for k in range(3):
        write_point(st, "master", k + 1)
        ema.step(k)
        want = {n: OE.ema_update("f32", want[n], OE.param(n, sh, k + 1, False), OE.one_minus_decay(k, 0.75))
                for n, sh in OE.SHAPES}
    got = shadow_bits(ema, "f32")
    for n, _ in OE.SHAPES:
        assert np.array_equal(got[n], OE.bits("f32", want[n]).reshape(-1)), n


def test_state_dict_round_trip_and_configured_decay_wins():
    st = build_store("bf16")
    a = FlatStoreEMA(st, decay=0.75, update_step_interval=1, device=CPU)
    write_point(st, "bf16", 1)
    a.step(0)
    sd = a.state_dict()
    assert sd["decay"] == 0.75 and len(sd["ema_parameters"]) == len(OE.SHAPES)
    assert [tuple(t.shape) for t in sd["ema_parameters"]] == [sh for _, sh in OE.SHAPES]
    b = FlatStoreEMA(st, decay=0.5, update_step_interval=1, device=CPU)
    assert not torch.equal(a.shadow, b.shadow)
    b.load_state_dict(sd)
    assert torch.equal(a.shadow.view(torch.int16), b.shadow.view(torch.int16))
    assert b.decay == 0.5                      # the configured decay wins over the saved one
    c = FlatStoreEMA(st, decay=0, update_step_interval=1, device=CPU)
    c.load_state_dict(sd)
    assert c.decay == 0.75                     # none configured: the saved one
    with pytest.raises(ValueError):
        b.load_state_dict({"decay": 0.75, "ema_parameters": sd["ema_parameters"][:-1]})


@pytest.mark.parametrize("kind", ["bf16", "f32", "master"])
def test_swap_restores_the_parameters(kind):
    st = build_store(kind)
    ema = FlatStoreEMA(st, decay=0.75, update_step_interval=1, device=CPU)
    write_point(st, kind, 1)
    ema.step(0)
    data, master = st.data.clone(), None if st.master is None else st.master.clone()
    ema.copy_ema_to(store_temp=True)
    if st.master is not None:
        assert torch.equal(st.master, ema.shadow)
        assert torch.equal(st.data.view(torch.int16), ema.shadow.to(torch.bfloat16).view(torch.int16))   # rne(master)
    else:
        assert torch.equal(st.data, ema.shadow)
    assert not torch.equal(st.data, data) and ema.temp_stored_parameters.device.type == "cpu"
    ema.copy_temp_to()
    assert ema.temp_stored_parameters is None
    assert torch.equal(st.data.view(torch.int32 if kind == "f32" else torch.int16),
                       data.view(torch.int32 if kind == "f32" else torch.int16))
    if master is not None:
        assert torch.equal(st.master.view(torch.int32), master.view(torch.int32))


def test_config_fields_and_factory():
    d = TrainConfig()
    assert (d.ema, d.ema_decay, d.ema_update_step_interval, d.ema_fp32) == ("OFF", 0.999, 5, False)
    cfg = TrainConfig().from_dict({"ema": "GPU", "ema_decay": 0.9, "ema_update_step_interval": 2})
    assert (cfg.ema, cfg.ema_decay, cfg.ema_update_step_interval) == ("GPU", 0.9, 2)
    assert not any(k.startswith("ema") for k in cfg.extra)
    st = build_store("bf16")
    assert create.create_ema(st, None, TrainConfig()) is None
    cfg.ema = "CPU"
    ema = create.create_ema(st, None, cfg)
    assert isinstance(ema, FlatStoreEMA) and ema.shadow.device.type == "cpu"
    assert (ema.decay, ema.update_step_interval, ema.shadow.dtype) == (0.9, 2, torch.bfloat16)
    cfg.ema_fp32 = True
    assert create.create_ema(st, None, cfg).shadow.dtype == torch.float32
    sd = ema.state_dict()
    sd["ema_parameters"] = [t + 1 for t in sd["ema_parameters"]]
    cfg.ema_fp32 = False
    loaded = create.create_ema(st, sd, cfg)
    assert torch.equal(loaded.state_dict()["ema_parameters"][4], sd["ema_parameters"][4])
    cfg.ema = "DISK"
    with pytest.raises(NotImplementedError, match="DISK"):
        create.create_ema(st, None, cfg)
