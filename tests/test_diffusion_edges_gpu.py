"""The 13 kernels of csrc/diffusion.hip at their edges (GPU): the Philox generator bit for bit against a host Philox, the
normals per element against float64 Box-Muller, UNIFORM / LOGIT_NORMAL and noise_ex exactly, the u01 = 1 corner, both
prologues bit for bit against the oracle, and the loss family against float64 per sample and per element, on the
smallest shapes that reach each path, every output inside a guarded NaN-filled buffer.  References, bounds and case
tables: tests/_diffusion_edges.py; tests/test_diffusion_edges_ref.py holds them to account on the CPU.  The last test
prints the worst |err| / bound per kernel."""
import numpy as np
import pytest
import torch

import _diffusion_edges as E
from _diffusion_edges import BF, F32, F64
from onetrainer_amd import _lib
from onetrainer_amd import kernels as K
from test_timestep_dists_gpu import philox_uniforms

pytestmark = pytest.mark.gpu
I32 = torch.int32
M64 = 0xFFFFFFFFFFFFFFFF


def status(name, *args):
    return getattr(K.lib(), name)(*[K._p(a) if isinstance(a, torch.Tensor) else a for a in args], K.stream_handle())


def raw(name, *args):
    K.check(status(name, *args), name)


def isf32(dt):
    return int(dt == F32)


# ------------------------------------------------------------------------------------------
# generator
def stream_draw(dev, n, seed, stream, offset, dtype=F32):
    buf, v, w = E.gbuf(n, dtype, dev)
    raw("otamd_noise_stream", v, isf32(dtype), n, offset, seed & M64, stream)
    assert E.gbuf_ok(buf, w), "noise_stream guards"
    return v.cpu()


def timestep_draw(dev, n, seed, sample0, dist, N=1000, draws=None, min_s=0.0, max_s=1.0, shift=1.0, bias=0.0, weight=0.0):
    buf, v, w = E.gbuf(n, I32, dev)
    K.timesteps(n, seed=seed, sample0=sample0, dist=dist, num_train_timesteps=N, min_s=min_s, max_s=max_s, shift=shift,
                bias=bias, weight=weight, out=v, draws=None if draws is None else draws.to(dev))
    assert E.gbuf_ok(buf, w), "timesteps guards"
    return v.cpu()


@pytest.mark.parametrize("seed", E.SEEDS)
@pytest.mark.parametrize("sample0", E.UNIFORM_SAMPLE0)
def test_uniforms_exact(dev, seed, sample0):
    for n in E.UNIFORM_NS:
        u = philox_uniforms(dev, n, seed, sample0)
        E.check_bits("philox uniform", u, E.uniform_held(seed, E._idx(sample0, n)), f"uniforms seed={seed} sample0={sample0} n={n}")


@pytest.mark.parametrize("name", E.TS_UNIFORM)
def test_uniform_timesteps_through_philox(dev, name):
    cfg = E.ts_cfg(name)
    for seed, sample0, n in ((1234, 77, 257), (2 ** 32 + 5, 2 ** 32 - 3, 65)):
        got = timestep_draw(dev, n, seed, sample0, 0, min_s=cfg["min_s"], max_s=cfg["max_s"], shift=cfg["shift"])
        want = E.uniform_timesteps(E.uniform_held(seed, E._idx(sample0, n)), cfg)
        E.check_bits("timesteps UNIFORM", got, want, f"UNIFORM {name} seed={seed} sample0={sample0}")


@pytest.mark.parametrize("name", E.TS_LOGIT)
def test_logit_normal_timesteps_through_philox(dev, name):
    cfg = E.ts_cfg(name)
    for seed, sample0, n in ((1234, 77, 257), (5, 2 ** 33 + 11, 65)):
        kw = dict(min_s=cfg["min_s"], max_s=cfg["max_s"], shift=cfg["shift"], bias=cfg["bias"], weight=cfg["weight"])
        got = timestep_draw(dev, n, seed, sample0, 1, **kw)
        z = stream_draw(dev, n, seed, 3, sample0)
        E.check_normals("noise_stream", z, seed, 3, sample0, n, f"stream 3 seed={seed} off={sample0}")
        want = timestep_draw(dev, n, 0, 0, 1, draws=E.logit_draws(z, cfg), **kw)
        E.check_bits("timesteps LOGIT_NORMAL", got, want, f"LOGIT_NORMAL {name} seed={seed} sample0={sample0}")
        assert int(got.min()) >= 0 and int(got.max()) <= 999


def test_logit_normal_held_inside_the_tables(dev):
    """1 / (1 + expf(-x)) is exactly 1.0 from x ~ 17.4 on: the result is held at N - 1"""
    d = torch.tensor([17.4, 40.0, -200.0, 0.0], dtype=F32)
    assert timestep_draw(dev, 4, 0, 0, 1, draws=d, max_s=1.0).tolist() == [999, 999, 0, 500]


@pytest.mark.parametrize("n,offset", E.NORMAL_CASES)
def test_normals_per_element(dev, n, offset):
    big = n > 4096
    drawn = {}
    for seed in (E.SEEDS[1:2] if big else E.SEEDS):
        for stream in ((1,) if big else E.NORMAL_STREAMS):
            z = stream_draw(dev, n, seed, stream, offset)
            what = f"normals seed={seed} stream={stream} off={offset} n={n}"
            E.check_normals("noise_stream", z, seed, stream, offset, n, what)
            if not big:
                E.check_bits("noise_stream bf16", stream_draw(dev, n, seed, stream, offset, BF), E.rne_bf16(z), what + " bf16")
            drawn[(seed, stream)] = z
            if stream == 1:
                for dt in (F32,) if big else (F32, BF):
                    buf, v, w = E.gbuf(n, dt, dev)
                    K.noise((n,), seed, offset=offset, dtype=dt, out=v)
                    assert E.gbuf_ok(buf, w), what + " noise guards"
                    E.check_bits("noise", v, z.to(dt), what + " noise()")
    if n >= 255 and not big:   # the streams, and the seeds, draw different values
        keys = list(drawn)
        for i, a in enumerate(keys):
            for b in keys[i + 1:]:
                assert float((drawn[a] == drawn[b]).float().mean()) < 0.02, (a, b)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", range(len(E.NOISE_EX_CASES)))
def test_noise_ex_exact(dev, case, dtype):
    shape, off, n = E.NOISE_EX_CASES[case]
    (B, h, w_, C), seed = shape, 21
    idx4 = E.noise_ex_index(shape, off, n)
    lo, hi = int(idx4.min()), int(idx4.max())
    base, pert = stream_draw(dev, n, seed, 1, off, dtype), stream_draw(dev, n, seed, 5, off, dtype)
    o4 = stream_draw(dev, hi - lo + 1, seed, 4, lo, dtype)[torch.from_numpy((idx4 - np.uint64(lo)).astype(np.int64))]
    for ow, pw in E.NOISE_EX_WEIGHTS:
        buf, v, w = E.gbuf(n, dtype, dev)
        raw("otamd_noise_ex", v, isf32(dtype), n, off, seed, C, h * w_ * C, float(ow), float(pw))
        assert E.gbuf_ok(buf, w), "noise_ex guards"
        E.check_bits("noise_ex", v, E.noise_ex_compose(base, o4, pert, ow, pw), f"noise_ex {shape} off={off} n={n} {ow, pw}")


@pytest.mark.parametrize("seed,sample", E.CORNER_PAIRS)
def test_uniform_corner_stays_inside_the_tables(dev, seed, sample):
    """word 0 >> 8 = 0xFFFFFF: u01 is exactly 1.0 there, and UNIFORM with the defaults returned 1000, one past the
    1000-entry tables (observed before timestep_kernel held the uniform below 1: t = 1000 at (1779877, 0))"""
    s0 = max(sample - 3, 0)
    got = timestep_draw(dev, 8, seed, s0, 0)
    u = E.uniform_held(seed, E._idx(s0, 8))
    cfg = {"min_s": 0.0, "max_s": 1.0, "shift": 1.0}
    print("corner", seed, sample, "returned", got.tolist())
    assert 0 <= int(got[sample - s0]) <= 999
    assert int(got[sample - s0]) == int(E.uniform_timesteps(np.array([E.BELOW_ONE]), cfg)[0]) == 999
    E.check_bits("timesteps UNIFORM", got, E.uniform_timesteps(u, cfg), f"corner {seed, sample} and its neighbours")
    E.check_bits("philox uniform", philox_uniforms(dev, 8, seed, s0), u, f"corner {seed, sample} uniforms")


@pytest.mark.parametrize("seed,elem,stream,word", E.NORMAL_CORNERS)
def test_normal_corner_is_zero(dev, seed, elem, stream, word):
    """u1 = 1.0: rad = 0, both elements of the pair +-0, the neighbours as the host predicts"""
    z = stream_draw(dev, 8, seed, stream, elem - 3)
    E.check_normals("noise_stream", z, seed, stream, elem - 3, 8, f"normal corner {seed, elem, stream}")
    assert z[3:5].tolist() == [0.0, 0.0] and bool((z[:3] != 0).all() and (z[5:] != 0).all())


# ------------------------------------------------------------------------------------------
# prologues
def pro_run(dev, c, cpad, dtype, kind=None):
    """ddpm (kind 0 / 1 / 2) or flow (kind None) into guarded buffers -> (model_in, target, scaled or None)"""
    n = c.B * c.HW
    bi, vi, wi = E.gbuf(n * cpad, BF, dev)
    bt, vt, wt = E.gbuf(n * c.C, dtype, dev)
    lat, eps, t = c.lat.to(dev), c.eps.to(dev), c.t.to(dev)
    vs = None
    if kind is None:
        raw("otamd_flow_prologue", lat, eps, isf32(dtype), t, float(E.FLOW_SF), float(E.FLOW_SHIFT), 1000, c.B, c.HW, c.C,
            cpad, vi, vt)
    else:
        bs, vs, ws = E.gbuf(n * c.C, F32, dev)
        acp, sq, s1m = (x.to(dev) for x in E.coeff_tables())
        raw("otamd_ddpm_prologue", lat, eps, isf32(dtype), t, acp, sq, s1m, float(E.SF), c.B, c.HW, c.C, cpad, vi, vt, kind, vs)
        assert E.gbuf_ok(bs, ws), "scaled guards"
    assert E.gbuf_ok(bi, wi) and E.gbuf_ok(bt, wt), "prologue guards"
    shp = (c.B, c.HW, 1)
    return vi.view(*shp, cpad), vt.view(*shp, c.C), None if vs is None else vs.view(*shp, c.C)


def ddpm_check(dev, c, cpad, dtype, kind, what):
    xi, tg, sc = pro_run(dev, c, cpad, dtype, kind)
    ri, rt, rs = E.ddpm_reference(c, cpad, kind)
    E.check_bits("ddpm_prologue unet_in", xi, ri, what + " unet_in (pad +0)")
    E.check_bits("ddpm_prologue target", tg, rt, what + " target")
    E.check_bits("ddpm_prologue scaled", sc, rs, what + " scaled")


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("HW", E.PRO_HW)
@pytest.mark.parametrize("C,cpad", E.DDPM_CC)
def test_ddpm_prologue_exact(dev, C, cpad, HW, dtype):
    c = E.pro_case(5, HW, C, dtype)
    for kind in (0, 1, 2):
        ddpm_check(dev, c, cpad, dtype, kind, f"ddpm C={C} cpad={cpad} HW={HW} kind={kind}")


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("C,cpad", E.FLOW_CC)
def test_flow_prologue_exact(dev, C, cpad, dtype):
    for HW in E.PRO_HW:
        c = E.pro_case(5, HW, C, dtype)
        assert 0 in c.t.tolist() and 999 in c.t.tolist()
        xi, tg, _ = pro_run(dev, c, cpad, dtype)
        ri, rt = E.flow_reference(c, cpad)
        E.check_bits("flow_prologue model_in", xi, ri, f"flow C={C} cpad={cpad} HW={HW} model_in (pad +0)")
        E.check_bits("flow_prologue target", tg, rt, f"flow C={C} cpad={cpad} HW={HW} target")


def test_prologues_grid_stride(dev):
    B, HW, C, cpad = E.PRO_STRIDE
    c = E.pro_case(B, HW, C, F32)
    ddpm_check(dev, c, cpad, F32, 1, "ddpm grid stride")
    xi, tg, _ = pro_run(dev, c, cpad, F32)
    ri, rt = E.flow_reference(c, cpad)
    E.check_bits("flow_prologue model_in", xi, ri, "flow grid stride model_in")
    E.check_bits("flow_prologue target", tg, rt, "flow grid stride target")


# ------------------------------------------------------------------------------------------
# losses
class Dev:
    """the operands of a loss case on the device, and the guarded outputs of one call"""

    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        self.pred, self.target, self.mask, self.lw, self.t = (x.to(dev) for x in (c.pred, c.target, c.mask, c.lw, c.t))
        self.sq, self.s1m = c.sq.to(dev), c.s1m.to(dev)
        self.ws = torch.full((4 * c.B * c.nblk + 8,), float("nan"), dtype=F32, device=dev)

    def outs(self, ncoef):
        c = self.c
        self.o = [E.gbuf(1, F32, self.dev), E.gbuf(c.B * ncoef, F32, self.dev), E.gbuf(c.B, F32, self.dev)]
        return [v for _, v, _ in self.o]

    def got(self):
        assert all(E.gbuf_ok(b, w) for b, _, w in self.o), self.c.name + " loss guards"
        return {"loss": self.o[0][1].cpu(), "coef": self.o[1][1].cpu(), "losses": self.o[2][1].cpu()}

    def loss(self, cfg, B=None):
        c = self.c
        masked, uw, normalize, (s2, s1, sl), fn, vp = cfg
        lo, co, ls = self.outs(3)
        return status("otamd_diffusion_loss", self.pred, c.cpad, self.target, isf32(c.target.dtype),
                      self.mask if masked else None, c.B if B is None else B, c.HW, c.C, float(s2), float(s1), float(sl),
                      float(uw), int(normalize), float(E.SCALE), self.lw, self.t, self.sq, self.s1m, fn, float(E.GAMMA),
                      int(vp), 1000, float(E.GA), self.ws, 4 * c.B * c.nblk, lo, co, ls)

    def mse(self, cfg, B=None):
        c = self.c
        fn, vp = cfg
        lo, co, ls = self.outs(1)
        return status("otamd_mse_loss", self.pred, c.cpad, self.target, isf32(c.target.dtype), c.B if B is None else B, c.HW,
                      c.C, float(E.MSE_STRENGTH), float(E.SCALE), self.lw, self.t, self.sq, self.s1m, fn, float(E.GAMMA),
                      int(vp), 1000, float(E.GA), self.ws, c.B * c.nblk, lo, co, ls)

    def grad(self, cfg, coef, go):
        """cfg None: mse_grad"""
        c = self.c
        buf, v, w = E.gbuf(c.B * c.HW * c.cpad, BF, self.dev)
        g = None if go is None else torch.tensor([go], dtype=F32, device=self.dev)
        if cfg is None:
            raw("otamd_mse_grad", self.pred, c.cpad, self.target, isf32(c.target.dtype), c.B, c.HW, c.C, coef, g, v)
        else:
            raw("otamd_diffusion_loss_grad", self.pred, c.cpad, self.target, isf32(c.target.dtype),
                self.mask if cfg[0] else None, c.B, c.HW, c.C, float(cfg[1]), coef, g, v)
        assert E.gbuf_ok(buf, w), c.name + " grad guards"
        return v.cpu().view(c.B, c.HW, c.cpad)


def loss_case_check(dev, c, configs, mse_configs):
    d = Dev(c, dev)
    for cfg in configs:
        what = f"{c.name} {cfg}"
        assert d.loss(cfg) == _lib.OTAMD_OK
        coef_dev = d.o[1][1]
        r = E.loss_math(c, cfg, F64)
        E.check_loss("diffusion_loss", c, cfg, d.got(), r, what)
        g1 = d.grad(cfg, coef_dev, None)
        ref, M = E.loss_grad_math(c, cfg, r["coef"], 1.0, F64)
        E.check_grad("diffusion_loss_grad", c, g1, ref, M, what + " grad")
        gh = d.grad(cfg, coef_dev, 0.5)
        E.check_bits("diffusion_loss_grad", gh, (g1.float() * 0.5).to(BF), what + " grad_out 0.5 scales exactly")
    for cfg in mse_configs:
        what = f"{c.name} mse {cfg}"
        assert d.mse(cfg) == _lib.OTAMD_OK
        coef_dev = d.o[1][1]
        r = E.mse_math(c, cfg, F64)
        E.check_loss("mse_loss", c, cfg, d.got(), r, what)
        ref, M = E.mse_grad_math(c, r["coef"], 0.5, F64)
        E.check_grad("mse_grad", c, d.grad(None, coef_dev, 0.5), ref, M, what + " grad")


@pytest.mark.parametrize("td", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", E.LOSS_SHAPES, ids=str)
def test_losses(dev, shape, td):
    loss_case_check(dev, E.loss_case(*shape, td), E.LOSS_CONFIGS, E.MSE_CONFIGS)


def test_log_cosh_probes(dev):
    """per = 1, d = LC_PROBES exactly: the softplus threshold at d = -10, the cancellation at small d, sign(0) = 0"""
    c = E.loss_case(*E.LC_SHAPE, F32, "lc")
    loss_case_check(dev, c, E.LOSS_CONFIGS, E.MSE_CONFIGS[:1])
    d = Dev(c, dev)
    cfg = E.LOSS_CONFIGS[10]
    assert d.loss(cfg) == _lib.OTAMD_OK
    g = d.grad(cfg, d.o[1][1], None)
    assert float(g[0, 0, 0]) == 0.0 and bool((g[1:, 0, 0] != 0).all())


def test_loss_batch_limit(dev):
    """B = 1025 is refused and nothing is written"""
    c = E.loss_case(1024, 2, 4, 8, F32)
    d = Dev(c, dev)
    for call, cfg in ((d.loss, E.LOSS_CONFIGS[0]), (d.mse, E.MSE_CONFIGS[0])):
        assert call(cfg, B=E.LOSS_MAX_B + 1) == _lib.OTAMD_EINVAL
        torch.cuda.synchronize()
        assert all(E.untouched(b) for b, _, _ in d.o) and bool(torch.isnan(d.ws).all())
    buf, v, w = E.gbuf(16, BF, dev)
    assert status("otamd_diffusion_loss_grad", d.pred, c.cpad, d.target, 1, None, E.LOSS_MAX_B + 1, c.HW, c.C, 0.1,
                  torch.zeros(3 * 1025, device=dev), None, v) == _lib.OTAMD_EINVAL
    torch.cuda.synchronize()
    assert E.untouched(buf)


def test_loss_grads_grid_stride(dev):
    """B HW cpad a little over 8192 x 256: the second sweep of both gradient kernels, and 257 blocks per sample"""
    c = E.loss_case(*E.LOSS_STRIDE, F32, False)
    loss_case_check(dev, c, [E.LOSS_CONFIGS[0]], [E.MSE_CONFIGS[1]])


def test_worst_ratios_report():
    rows = {k: v for k, v in E.WORST.items() if not k.startswith("cpu:")}
    for k in sorted(rows):
        print(f"{k:34s} {rows[k][0]:8.3f}  {rows[k][1]}")
    assert rows and all(v[0] <= 1 for v in rows.values())
