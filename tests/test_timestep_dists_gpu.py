"""HEAVY_TAIL, COS_MAP and SIGMOID timesteps on the GPU (csrc/diffusion.hip timestep_ex_kernel, otamd_timesteps_ex):
the table lookup exactly against the host lookup on hand-picked uniforms, HEAVY_TAIL against the float64 restatement
(tests/_timestep_ref.py) on the reference's recorded uniforms, the shared Philox uniform, DP slices, the drawn
distribution, the untouched old entry point, and the setups end to end."""
from pathlib import Path

import numpy as np
import pytest
import torch

import _timestep_ref as R
from onetrainer_amd import _lib
from onetrainer_amd import kernels as K
from onetrainer_amd.util.timestep_table import timestep_cdf, timestep_weights

pytestmark = pytest.mark.gpu
G = np.load(Path(__file__).parent / "golden" / "timestep_dists.npz")
HEAVY_CASES = sorted({k.rsplit("/", 1)[0] for k in G.files if k.startswith("heavy_tail")})
LEFT_OUT_CAP = 0.02
# (distribution, N, min strength, max strength, shift, bias, weight): the fixture's geometries, SIGMOID steep enough
# at N = 1000 that buckets of probability 0 lead the table
TABLES = [("COS_MAP", 1000, 0.0, 1.0, 1.0, 0.0, 0.0), ("SIGMOID", 1000, 0.1, 0.9, 3.0, 0.0, 4000.0),
          ("SIGMOID", 10, 0.0, 1.0, 0.5, 0.3, 10.0), ("COS_MAP", 10, 0.0, 1.0, 0.5, 0.0, 0.0)]
PLANTED = np.array([0.0, 1.0, 0.0, 0.0, 2.0, 1e-30, 3.0, 0.0, 0.0, 0.0])      # N = 10: zeros in front, inside, behind


def table(case):
    dist, N, mn, mx, shift, bias, weight = case
    return timestep_cdf(timestep_weights(dist, N, int(N * mn), int(N * mx), shift, bias, weight))


def draw(dev, case, cdf, n, seed=0, sample0=0, draws=None):
    dist, N, mn, mx, shift, bias, weight = case
    return K.timesteps(n, seed=seed, sample0=sample0, dist={"HEAVY_TAIL": 2, "COS_MAP": 3, "SIGMOID": 4}[dist],
                       num_train_timesteps=N, min_s=mn, max_s=mx, shift=shift, bias=bias, weight=weight, device=dev,
                       draws=None if draws is None else torch.from_numpy(np.ascontiguousarray(draws)).to(dev),
                       cdf=None if cdf is None else torch.from_numpy(cdf).to(dev))


def picked_uniforms(cdf):
    """0, the largest fp32 below 1, every table entry and its two fp32 neighbours (those inside [0, 1))"""
    u = np.concatenate([np.array([0.0, R.BELOW_ONE], dtype=np.float32), cdf, np.nextafter(cdf, np.float32(0)),
                        np.nextafter(cdf, np.float32(2))]).astype(np.float32)
    return np.unique(u[(u >= 0) & (u < 1)])


def philox_uniforms(dev, n, seed, sample0=0):
    """the uniforms of samples [sample0, sample0 + n), recovered exactly from UNIFORM at N = 2^24 over the whole range
    with shift 1: there t0 = 2^24 u and the shift map (2^24 t0) / (0 t0 + 2^24) are exact, u = (k + 0.5) / 2^24 with
    k < 2^24 truncates to k below 2^23, and from 2^23 on k + 0.5 is rounded to the integer t itself (ties to even: k
    or k + 1).  k = 0xFFFFFF is the exception: its k + 0.5 rounds to 2^24, u01 is exactly 1.0, and every timestep
    kernel holds that uniform at the largest fp32 below 1, so t = 2^24 - 1 and what is returned is that held value,
    the u the kernels use"""
    t = K.timesteps(n, seed=seed, sample0=sample0, dist=0, num_train_timesteps=1 << 24, device=dev).cpu().numpy()
    return (np.where(t < (1 << 23), t + 0.5, t.astype(np.float64)) / 2.0 ** 24).astype(np.float32)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("which", list(range(len(TABLES))) + ["planted"])
def test_table_lookup_exact_on_picked_uniforms(dev, which, n):
    """the launch uses 64-thread blocks: one thread, one short of a block, a full block, a block and one thread"""
    if which == "planted":
        case, cdf = ("COS_MAP", 10, 0.0, 1.0, 1.0, 0.0, 0.0), timestep_cdf(PLANTED)
        weights = PLANTED
    else:
        case = TABLES[which]
        weights = timestep_weights(case[0], case[1], int(case[1] * case[2]), int(case[1] * case[3]), *case[4:])
        cdf = timestep_cdf(weights)
    N, mn, mx = case[1], int(case[1] * case[2]), int(case[1] * case[3])
    u_all = picked_uniforms(cdf)
    p = np.diff(cdf.astype(np.float64), prepend=0.0)
    seen = []
    # chunks of n uniforms (n = 1: sixteen of them, spread over the list); a short last chunk repeats itself
    for start in range(0, len(u_all), n if n > 1 else max(1, len(u_all) // 16)):
        u = np.resize(u_all[start:start + n], n)
        got = draw(dev, case, cdf, n, draws=u).cpu().numpy()
        want = R.table_lookup(cdf, u, mn)
        assert (got == want).all(), (which, n, start)
        seen.append(got)
    got = np.concatenate(seen)
    assert ((got >= mn) & (got < mx)).all()
    assert (p[got - mn] > 0).all() and (weights[got - mn] > 0).all()
    if which in (1, "planted"):
        assert (weights == 0).sum() >= 6 and (p == 0).sum() >= 6    # these tables do hold zero-weight buckets
    if n > 1:
        assert set(np.flatnonzero(p > 0) + mn) == set(got)          # every reachable bucket was reached


@pytest.mark.parametrize("name", HEAVY_CASES)
def test_heavy_tail_on_reference_uniforms(dev, name):
    """equality with the float64 restatement outside the fp32 error band of an integer (heavy_tail_band); the same
    draws agree with the reference's recorded timesteps"""
    N, mn, mx, shift, bias, weight = (float(v) for v in G[f"{name}/cfg"])
    N = int(N)
    u = G[f"{name}/u"]
    got = draw(dev, ("HEAVY_TAIL", N, mn, mx, shift, bias, weight), None, u.size, draws=u).cpu().numpy()
    want, decided = R.heavy_tail_decided(u, N, int(N * mn), int(N * mx), shift, weight)
    left_out = 1.0 - decided.mean()
    print(name, "left out", left_out, "differ from the reference's fp32", int((got != G[f"{name}/t"]).sum()))
    assert left_out <= LEFT_OUT_CAP
    assert (got[decided] == want[decided]).all()
    assert (got[decided] == G[f"{name}/t"][decided]).all()
    assert (np.abs(got - want) <= 1).all() and ((got >= 0) & (got < N)).all()


@pytest.mark.parametrize("which", [1, 2])
def test_table_draws_use_the_uniform_stream(dev, which):
    """with the same (seed, sample0), the Philox path of the table kernel is the host lookup of the uniforms UNIFORM
    draws, and the same again when they come back through draws="""
    case, cdf = TABLES[which], table(TABLES[which])
    mn = int(case[1] * case[2])
    n, seed, sample0 = 257, 1234, 77
    u = philox_uniforms(dev, n, seed, sample0)
    assert ((u > 0) & (u <= 1)).all() and len(np.unique(u)) > 250
    got = draw(dev, case, cdf, n, seed=seed, sample0=sample0).cpu().numpy()
    assert (got == R.table_lookup(cdf, u, mn)).all()
    assert (got == draw(dev, case, cdf, n, draws=u).cpu().numpy()).all()
    # HEAVY_TAIL reads the same uniform
    hcase = ("HEAVY_TAIL", 1000, 0.0, 1.0, 3.0, 0.0, 1.0)
    assert torch.equal(draw(dev, hcase, None, n, seed=seed, sample0=sample0), draw(dev, hcase, None, n, draws=u))


@pytest.mark.parametrize("case", [("HEAVY_TAIL", 1000, 0.0, 1.0, 3.0, 0.0, 0.5), TABLES[0], TABLES[1]],
                         ids=["HEAVY_TAIL", "COS_MAP", "SIGMOID"])
def test_dp_slices_match_global(dev, case):
    cdf = None if case[0] == "HEAVY_TAIL" else table(case)
    whole = draw(dev, case, cdf, 8, seed=5)
    parts = torch.cat([draw(dev, case, cdf, 4, seed=5), draw(dev, case, cdf, 4, seed=5, sample0=4)])
    assert torch.equal(whole, parts)
    assert len(set(whole.tolist())) > 1 and not torch.equal(whole, draw(dev, case, cdf, 8, seed=6))


@pytest.mark.parametrize("case", [("COS_MAP", 1000, 0.0, 1.0, 3.0, 0.0, 0.0), ("SIGMOID", 1000, 0.0, 1.0, 3.0, 0.0, 10.0)],
                         ids=["COS_MAP", "SIGMOID"])
def test_drawn_distribution_follows_the_table(dev, case):
    """n = 65536 draws: the largest gap between the empirical CDF and the table is at most
    sqrt(ln(2 / 1e-9) / (2 n)) (Dvoretzky-Kiefer-Wolfowitz: a larger gap has probability below 1e-9)"""
    n = 65536
    cdf = table(case)
    t = draw(dev, case, cdf, n, seed=2024).cpu().numpy()
    emp = np.cumsum(np.bincount(t, minlength=cdf.size)) / n
    gap = np.abs(emp - cdf.astype(np.float64)).max()
    bound = np.sqrt(np.log(2 / 1e-9) / (2 * n))
    print(case[0], "largest CDF gap", gap, "bound", bound)
    assert gap <= bound


def _raw(entry, out, n, dist, N, mn, mx, draws=None, cdf=None, n_cdf=None):
    args = [out.data_ptr() if out is not None else None, n, 0, 11, dist, N, mn, mx, 1.0, 0.0, 0.0,
            None if draws is None else draws.data_ptr()]
    if entry == "otamd_timesteps_ex":
        args += [None if cdf is None else cdf.data_ptr(), (0 if cdf is None else cdf.numel()) if n_cdf is None else n_cdf]
    return getattr(_lib.lib(), entry)(*args, K.stream_handle())


def test_old_ids_untouched_and_argument_checks(dev):
    n = 300
    for dist, kw in ((0, {}), (0, {"shift": 3.0, "min_s": 0.1, "max_s": 0.9}), (1, {"bias": 0.5, "weight": 0.3})):
        direct = torch.empty(n, dtype=torch.int32, device=dev)
        N = 1000
        mn, mx = int(N * kw.get("min_s", 0.0)), int(N * kw.get("max_s", 1.0))
        rc = _lib.lib().otamd_timesteps(direct.data_ptr(), n, 3, 99, dist, N, mn, mx, float(kw.get("shift", 1.0)),
                                        float(kw.get("bias", 0.0)), float(kw.get("weight", 0.0)), None,
                                        K.stream_handle())
        assert rc == _lib.OTAMD_OK
        assert torch.equal(K.timesteps(n, seed=99, sample0=3, dist=dist, device=dev, **kw), direct)
    out = torch.full((8,), -7, dtype=torch.int32, device=dev)
    cdf = torch.from_numpy(timestep_cdf(np.ones(10))).to(dev)
    E = _lib.OTAMD_EINVAL
    assert _raw("otamd_timesteps", out, 8, 2, 10, 0, 10) == E                      # the old entry point still refuses 2
    assert _raw("otamd_timesteps", out, 8, 3, 10, 0, 10) == E
    ex = "otamd_timesteps_ex"
    assert _raw(ex, out, 8, 3, 10, 0, 10, cdf=None) == E                           # table without a table
    assert _raw(ex, out, 8, 3, 10, 0, 9, cdf=cdf) == E                             # n_cdf != max_t - min_t
    assert _raw(ex, out, 8, 3, 10, 2, 10, cdf=cdf) == E
    assert _raw(ex, out, 8, 3, 10, 5, 5, cdf=cdf, n_cdf=0) == E                    # n_cdf <= 0
    assert _raw(ex, out, 8, 3, 10, 0, 10, cdf=cdf, n_cdf=-1) == E
    assert _raw(ex, out, 8, 4, 10, 0, 10, cdf=cdf) == E                            # dist outside {0, 1, 2, 3}
    assert _raw(ex, out, 8, -1, 10, 0, 10, cdf=cdf) == E
    for dist in (0, 1, 2, 3):                                                      # the existing range checks
        assert _raw(ex, None, 8, dist, 10, 0, 10, cdf=cdf) == E
        assert _raw(ex, out, 0, dist, 10, 0, 10, cdf=cdf) == E
        assert _raw(ex, out, 8, dist, 0, 0, 0, cdf=cdf) == E
        assert _raw(ex, out, 8, dist, 10, -1, 9, cdf=cdf) == E
        assert _raw(ex, out, 8, dist, 10, 6, 5, cdf=cdf) == E
        assert _raw(ex, out, 8, dist, 10, 1, 11, cdf=cdf) == E
    torch.cuda.synchronize()
    assert (out == -7).all()                                                       # a refused call writes nothing
    assert _raw(ex, out, 8, 3, 10, 0, 10, cdf=cdf) == _lib.OTAMD_OK
    assert ((out >= 0) & (out < 10)).all()
    # the wrapper's own checks
    with pytest.raises(ValueError, match="timestep cdf"):
        K.timesteps(8, seed=0, dist=3, num_train_timesteps=10, device=dev)
    with pytest.raises(ValueError, match="timestep cdf"):
        K.timesteps(8, seed=0, dist=4, num_train_timesteps=12, device=dev, cdf=cdf)
    with pytest.raises(ValueError, match="timestep cdf"):
        K.timesteps(8, seed=0, dist=0, num_train_timesteps=10, device=dev, cdf=cdf)
    with pytest.raises(ValueError, match="distribution id"):
        K.timesteps(8, seed=0, dist=5, num_train_timesteps=10, device=dev)


def _sdxl_trainer(dev, dist, **kw):
    from onetrainer_amd.module import unet as U
    from onetrainer_amd.trainer.GenericTrainer import GenericTrainer
    from onetrainer_amd.util import create
    from onetrainer_amd.util.config.TrainConfig import TrainConfig
    cfg = TrainConfig.default_values()
    cfg.batch_size = 2
    cfg.learning_rate = 1e-4
    cfg.learning_rate_warmup_steps = 0
    cfg.timestep_distribution = dist
    cfg.min_noising_strength, cfg.max_noising_strength = 0.2, 0.8
    cfg.timestep_shift, cfg.noising_weight, cfg.noising_bias = 3.0, 1.0, 0.1
    for k, v in kw.items():
        setattr(cfg, k, v)
    tr = GenericTrainer(cfg, model=create.create_model(cfg, dev, seed=3, unet_config=U.tiny_sdxl_config()))
    tr.start()
    return tr, cfg


def _sdxl_batch(dev):
    from onetrainer_amd.dataLoader.SyntheticDataLoader import synthetic_sdxl_batch
    return synthetic_sdxl_batch(2, 128, 128, dev, seed=1, te1_dim=48, te2_dim=48, pooled_dim=64)


def _expected(dev, cfg, dist, seed, B, N=1000, shift=None):
    case = (dist, N, cfg.min_noising_strength, cfg.max_noising_strength, cfg.timestep_shift if shift is None else shift,
            cfg.noising_bias, cfg.noising_weight)
    return draw(dev, case, None if dist == "HEAVY_TAIL" else table(case), B, seed=seed)


@pytest.mark.parametrize("dist", ["HEAVY_TAIL", "COS_MAP", "SIGMOID"])
def test_sdxl_steps_train(dev, dist):
    """strengths 0.2..0.8: the timesteps stay inside [200, 800).  HEAVY_TAIL runs at shift 1 here, since its shift
    map acts after the range is applied and moves timesteps past max_t, as the reference's does"""
    tr, cfg = _sdxl_trainer(dev, dist, **({"timestep_shift": 1.0} if dist == "HEAVY_TAIL" else {}))
    batch = _sdxl_batch(dev)
    model, setup = tr.model, tr.model_setup
    for step in range(2):
        gs = model.train_progress.global_step
        _, t = setup.step_inputs(model, batch, cfg, model.train_progress)
        assert t.dtype == torch.int32 and ((t >= 200) & (t < 800)).all(), t
        assert torch.equal(t, _expected(dev, cfg, dist, gs, 2))
        loss = tr.train_step(batch).item()
        assert np.isfinite(loss) and abs(loss) < 1e4, loss
    assert len(setup.timestep_tables.tables) == (0 if dist == "HEAVY_TAIL" else 1)
    _, t = setup.step_inputs(model, batch, cfg, model.train_progress, deterministic=True)
    assert (t == 499).all()


def test_captured_step_draws_from_the_table(dev, monkeypatch):
    """the captured step (trainer/step_graph.py) draws (noise, timestep) outside the graph through
    step_inputs(out=...): the table is built on the eager first step and the replays read it"""
    monkeypatch.setenv("OTAMD_STEP_GRAPH", "1")
    tr, cfg = _sdxl_trainer(dev, "SIGMOID")
    assert tr.graphs is not None
    batch = _sdxl_batch(dev)
    losses = []
    for step in range(3):
        gs = tr.model.train_progress.global_step
        losses.append(tr.train_step(batch).item())
    torch.cuda.synchronize()
    assert len(tr.graphs.entries) == 1 and all(np.isfinite(losses))
    (entry,) = tr.graphs.entries.values()
    assert torch.equal(entry.timestep, _expected(dev, cfg, "SIGMOID", gs, 2))
    assert len(tr.model_setup.timestep_tables.tables) == 1


def test_flux_step_inputs_cos_map(dev):
    from onetrainer_amd.dataLoader.SyntheticDataLoader import synthetic_flux_batch
    from onetrainer_amd.module import flux as FX
    from onetrainer_amd.trainer.GenericTrainer import GenericTrainer
    from onetrainer_amd.util import create
    from onetrainer_amd.util.config.TrainConfig import TrainConfig
    cfg = TrainConfig.default_values()
    cfg.model_type = "FLUX_DEV_1"
    cfg.training_method = "LORA"
    cfg.timestep_distribution = "COS_MAP"
    cfg.dynamic_timestep_shifting = True
    cfg.min_noising_strength, cfg.max_noising_strength = 0.2, 0.8
    cfg.batch_size = 2
    cfg.lora_rank, cfg.lora_alpha = 8, 8.0
    fcfg = FX.tiny_flux_config()
    tr = GenericTrainer(cfg, model=create.create_model(cfg, dev, seed=3, flux_config=fcfg))
    tr.start()
    model, setup = tr.model, tr.model_setup
    batch = synthetic_flux_batch(2, 128, 128, dev, seed=1, t5_dim=fcfg.joint_attention_dim,
                                 pooled_dim=fcfg.pooled_projection_dim, text_len=9)
    N = model.noise_scheduler.config["num_train_timesteps"]
    noise, t = setup.step_inputs(model, batch, cfg, model.train_progress)
    assert tuple(noise.shape) == (2, 16, 16, 16)
    assert t.dtype == torch.int32 and ((t >= int(N * 0.2)) & (t < int(N * 0.8))).all(), t
    shift = setup._shift(cfg, 16, 16)
    assert shift != 1.0
    assert torch.equal(t, _expected(dev, cfg, "COS_MAP", model.train_progress.global_step, 2, N=N, shift=shift))
    out = setup.predict(model, batch, cfg, model.train_progress)
    assert torch.equal(out["timestep"], t)
    assert len(setup.timestep_tables.tables) == 1
