"""The saved format of the fused optimizers is a contract: state_dict / load_state_dict of every class over one
four-tensor CPU store (util/optimizer/flat_store.py holds the walk, each class its hooks).  What the oracle tests of
schedule-free and 8-bit AdamW already pin (their key sets, 'no state before the first step') is not repeated here.
FusedProdigy keeps pinned host memory and device events for its read-back of d, so it is built here with those two
stubbed; its resume on the device is test_prodigy_gpu.py's."""
import copy

import pytest
import torch

from onetrainer_amd.module.param_store import FlatParamStore

SPEC = [("a", (3,), "g"), ("b", (2, 5), "g"), ("c", (5, 1000), "h"), ("d", (4097,), "h")]
SHAPES = {n: s for n, s, _ in SPEC}
TOP = {"state", "param_groups", "sr_seed"}


def _store():
    st = FlatParamStore(SPEC, torch.float32, torch.device("cpu"))
    st.data.copy_(torch.randn(st.data.shape, generator=torch.Generator().manual_seed(11)))
    return st


def _groups(st, second=None):
    return [{"params": [st.params["a"], st.params["b"]]}, dict({"params": [st.params["c"], st.params["d"]]}, **(second or {}))]


def _make(name, seed=5, monkeypatch=None):
    st = _store()
    if name == "adamw":
        from onetrainer_amd.util.optimizer.adamw_fused import FusedAdamW
        return st, FusedAdamW(st, _groups(st, {"lr": 5e-4}), lr=1e-3, seed=seed)
    if name == "adafactor":
        from onetrainer_amd.util.optimizer.adafactor_fused import FusedAdafactor
        return st, FusedAdafactor(st, _groups(st, {"lr": 5e-4}), lr=1e-3, relative_step=False, seed=seed)
    if name == "came":
        from onetrainer_amd.util.optimizer.came_fused import FusedCAME
        return st, FusedCAME(st, _groups(st, {"lr": 5e-4}), lr=1e-3, seed=seed)
    if name == "schedule_free":
        from onetrainer_amd.util.optimizer.schedule_free_fused import FusedScheduleFreeAdamW
        return st, FusedScheduleFreeAdamW(st, _groups(st, {"lr": 5e-4}), lr=1e-3, seed=seed)
    if name == "adamw8bit":
        from onetrainer_amd.util.optimizer.adamw8bit_fused import FusedAdamW8bit
        return st, FusedAdamW8bit(st, _groups(st, {"lr": 5e-4}), lr=1e-3, seed=seed)
    from onetrainer_amd.util.optimizer.prodigy_fused import FusedProdigy

    class Event:
        def record(self, *a):
            pass

        def query(self):
            return True
    monkeypatch.setattr(torch.cuda, "Event", Event)
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    return st, FusedProdigy(st, _groups(st), seed=seed)


def _fill(opt):
    """every state buffer from one generator, the counters as three and four steps leave them"""
    g = torch.Generator().manual_seed(3)
    for k, v in sorted(vars(opt).items()):
        if isinstance(v, torch.Tensor) and not k.startswith("_") and k != "clip_out":
            v.copy_(torch.randint(0, 256, v.shape, generator=g, dtype=torch.uint8) if v.dtype == torch.uint8
                    else torch.rand(v.shape, generator=g))
    if hasattr(opt, "steps"):
        opt.steps = [3, 4]
    for flag in ("_z_set", "_p0_set"):
        if hasattr(opt, flag):
            setattr(opt, flag, True)


def _views(opt, n):
    """{state key: view of its buffer} of tensor n; AdamW's moments are indexed as the store"""
    if type(opt).__name__ == "FusedAdamW":
        s = opt.store.slots[n]
        return {k: getattr(opt, k)[s.offset:s.offset + s.numel].view(s.shape) for k in ("exp_avg", "exp_avg_sq")}
    return opt._views(n)


FACTORED = {"step", "RMS", "exp_avg_sq_row", "exp_avg_sq_col"}
CAME_FACTORED = FACTORED | {"exp_avg", "exp_avg_res_row", "exp_avg_res_col"}
KEYS = {   # per class: the entry of a vector ("a", "d") and of a matrix ("b", "c")
    "adamw": ({"step", "exp_avg", "exp_avg_sq"},) * 2,
    "adafactor": ({"step", "RMS", "exp_avg_sq"}, FACTORED),
    "came": ({"step", "RMS", "exp_avg", "exp_avg_sq"}, CAME_FACTORED),
    "prodigy": ({"step", "s", "p0", "exp_avg", "exp_avg_sq"},) * 2,
}
TUPLES = {"adamw": set(), "adafactor": {"eps"}, "came": {"eps", "betas"}, "schedule_free": {"betas"},
          "adamw8bit": {"betas"}, "prodigy": {"betas"}}


@pytest.mark.parametrize("name", sorted(KEYS))
def test_key_sets_types_and_shapes(name, monkeypatch):
    st, opt = _make(name, monkeypatch=monkeypatch)
    _fill(opt)
    sd = opt.state_dict()
    assert set(sd) == TOP and sd["sr_seed"] == 5 and type(sd["sr_seed"]) is int
    assert sorted(sd["state"]) == [0, 1, 2, 3] and [g["params"] for g in sd["param_groups"]] == [[0, 1], [2, 3]]
    vec, mat = KEYS[name]
    for i, n in enumerate("abcd"):
        s = sd["state"][i]
        assert set(s) == (mat if len(SHAPES[n]) == 2 else vec), n
        for k, v in s.items():
            if k in ("step", "RMS"):
                continue
            assert v.dtype == torch.float32 and v.data_ptr() != _views(opt, n)[k].data_ptr(), (n, k)   # a clone
            want = {"_row": SHAPES[n][:-1], "_col": SHAPES[n][:-2] + SHAPES[n][-1:]}.get(k[-4:], SHAPES[n])
            assert tuple(v.shape) == tuple(want) and torch.equal(v, _views(opt, n)[k]), (n, k)
    step = [sd["state"][i]["step"] for i in range(4)]
    if name == "adamw":     # torch's AdamW layout: a float tensor
        assert all(isinstance(x, torch.Tensor) and x.dtype == torch.float32 for x in step) and [float(x) for x in step] == [3, 3, 4, 4]
    elif name == "prodigy":  # the device's k, one for the whole store
        assert step == [0, 0, 0, 0] and all(type(x) is int for x in step)
    else:
        assert step == [3, 3, 4, 4] and all(type(x) is int for x in step)
        assert all(isinstance(sd["state"][i]["RMS"], torch.Tensor) and sd["state"][i]["RMS"].shape == () for i in range(4))


def test_group_keys():
    _, opt = _make("adamw")
    sd = opt.state_dict()
    assert all(set(g) == {"lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach", "capturable",
                          "differentiable", "fused", "params"} for g in sd["param_groups"])
    assert [g["lr"] for g in sd["param_groups"]] == [1e-3, 5e-4]
    _, opt = _make("adafactor")
    assert all(set(g) == {"lr", "eps", "clip_threshold", "decay_rate", "beta1", "weight_decay", "scale_parameter",
                          "relative_step", "warmup_init", "params"} for g in opt.state_dict()["param_groups"])
    _, opt = _make("came")
    assert all(set(g) == {"lr", "eps", "clip_threshold", "betas", "weight_decay", "params"}
               for g in opt.state_dict()["param_groups"])


@pytest.mark.parametrize("name", ["adamw", "adafactor", "came"])
def test_state_is_written_before_the_first_step(name):
    """AdamW and the factored optimizers keep no first-step flag: their (zero) state is there from the start"""
    _, opt = _make(name)
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 1, 2, 3]
    assert all(float(sd["state"][i]["step"]) == 0 for i in range(4))
    assert all(not v.any() for s in sd["state"].values() for k, v in s.items() if k != "step")


def test_prodigy_has_no_state_before_the_first_step_and_carries_the_seed_in_its_groups(monkeypatch):
    from onetrainer_amd.util.optimizer import prodigy_fused as P
    _, opt = _make("prodigy", monkeypatch=monkeypatch)
    sd = opt.state_dict()
    assert sd["state"] == {} and sd["sr_seed"] == 5
    keys = {"lr", "d", "d_max", "k", "d_coef", "growth_rate", "sr_seed", "params"} | set(P.HYPER_KEYS) | set(P.STATE_KEYS)
    assert all(set(g) == keys and g["sr_seed"] == 5 for g in sd["param_groups"])
    assert "sr_seed" not in opt.param_groups[0]                  # the live groups do not grow the key
    assert list(sd["param_groups"][0])[-2:] == ["params", "sr_seed"]


def test_prodigy_seed_falls_back_to_the_first_group_that_has_one(monkeypatch):
    _, opt = _make("prodigy", monkeypatch=monkeypatch)
    _fill(opt)
    sd = opt.state_dict()

    def load(change):
        d = copy.deepcopy(sd)
        change(d)
        _, fresh = _make("prodigy", seed=99, monkeypatch=monkeypatch)
        fresh.load_state_dict(d)
        assert all("sr_seed" not in g for g in fresh.param_groups)
        return fresh.seed

    def groups_only(d):
        del d["sr_seed"]
        d["param_groups"][0]["sr_seed"], d["param_groups"][1]["sr_seed"] = None, 8

    def none_anywhere(d):
        d["sr_seed"] = None
        for g in d["param_groups"]:
            del g["sr_seed"]
    assert load(lambda d: None) == 5
    assert load(lambda d: d["param_groups"][0].update(sr_seed=7)) == 5      # the top level wins
    assert load(lambda d: d.update(sr_seed=None) or d["param_groups"][0].update(sr_seed=7)) == 7
    assert load(groups_only) == 8
    assert load(none_anywhere) == 99                                         # nothing saved: the seed stays


@pytest.mark.parametrize("name", ["adamw", "adafactor", "came", "schedule_free", "adamw8bit", "prodigy"])
def test_round_trip_and_a_parameter_without_saved_state(name, monkeypatch):
    st, opt = _make(name, monkeypatch=monkeypatch)
    _fill(opt)
    sd = opt.state_dict()
    sd["param_groups"][0]["lr"] = 0.25 if name != "prodigy" else sd["param_groups"][0]["lr"]
    for g in sd["param_groups"]:                                 # as a JSON or safetensors round trip leaves tuples
        for k in ("betas", "eps"):
            if isinstance(g.get(k), tuple):
                g[k] = list(g[k])
    part = copy.deepcopy(sd)
    del part["state"][1]
    del part["sr_seed"]
    st2, full = _make(name, seed=99, monkeypatch=monkeypatch)
    full.load_state_dict(sd)
    assert full.seed == 5 and getattr(full, "steps", [3, 4]) == [3, 4]
    assert all(torch.equal(v, _views(full, n)[k]) for n in "abcd" for k, v in _views(opt, n).items())
    assert full.param_groups[0]["lr"] == sd["param_groups"][0]["lr"]
    for g in full.param_groups:                                  # the keys the class restores as tuples, and no others
        assert {k for k in ("betas", "eps") if isinstance(g.get(k), tuple)} == TUPLES[name]
    st3, fresh = _make(name, seed=99, monkeypatch=monkeypatch)
    fresh.load_state_dict(part)
    # Prodigy's groups carry the seed; every other class keeps its own without the top-level key
    assert fresh.seed == (5 if name == "prodigy" else 99)
    for n in "acd":
        assert all(torch.equal(v, _views(fresh, n)[k]) for k, v in _views(opt, n).items()), n
    start = {"schedule_free": {"z": st3.value("b")}, "prodigy": {"p0": st3.value("b")}}.get(name, {})
    for k, v in _views(fresh, "b").items():                   # "b" starts fresh: zeros, or the current value
        assert torch.equal(v, start[k].reshape(v.shape)) if k in start else not v.any(), k


def test_schedule_free_forgets_saved_bits_and_keeps_one_mode():
    _, opt = _make("schedule_free")
    _fill(opt)
    sd = opt.state_dict()
    sd["param_groups"][0]["train_mode"] = True                    # the first group's mode is the store's
    _, fresh = _make("schedule_free", seed=99)
    fresh._y_saved = torch.zeros(1)
    fresh.load_state_dict(sd)
    assert fresh._y_saved is None and fresh._z_set and all(g["train_mode"] for g in fresh.param_groups)
    sd["param_groups"][1]["betas"] = (1.0, 0.999)
    with pytest.raises(ValueError, match="beta1"):
        fresh.load_state_dict(sd)
