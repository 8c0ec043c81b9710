"""DoRA on the GPU (csrc/dora.hip, module/dora.py): the merge and the gradient projection per element against the
float64 oracle (tests/_oracle_dora.py, whose bounds are derived there), the wiring against a plain UNet that holds
W' as its weights, and training / save / backup through the setup and GenericTrainer."""
import os

import numpy as np
import pytest
import torch

import _oracle_dora as O
from onetrainer_amd.dataLoader.SyntheticDataLoader import synthetic_sdxl_batch
from onetrainer_amd.module import streams as S
from onetrainer_amd.module import unet as U
from onetrainer_amd.module.dora import DoRAWrapper
from onetrainer_amd.module.param_store import FlatParamStore
from onetrainer_amd.module.stream_hazards import StreamHazardCheck
from onetrainer_amd.trainer.GenericTrainer import GenericTrainer
from onetrainer_amd.util import create
from onetrainer_amd.util.config.TrainConfig import TrainConfig

pytestmark = pytest.mark.gpu

# the smallest shapes that reach every edge: a Linear smaller than one tile with odd tile remainders (24 x 40), one of
# several tiles per side (320 x 320), a 3x3 conv (kernel taps folded into the input-axis norm), the conv_in form (4
# real input channels padded to the store's 8), a 1x1 conv held as a linear, and a q|k|v group whose to_k the layer
# filter leaves out
SPECS = [("lin_a.weight", (24, 40), "linear", 40), ("lin_b.weight", (320, 320), "linear", 320),
         ("conv.weight", (24, 16, 3, 3), "conv", 144), ("conv_in.weight", (16, 4, 3, 3), "conv", 36),
         ("pw.weight", (24, 16, 1, 1), "conv", 16), ("blk.attn1.to_q.weight", (64, 64), "linear", 64),
         ("blk.attn1.to_k.weight", (64, 64), "linear", 64), ("blk.attn1.to_v.weight", (64, 64), "linear", 64)]
FILTER = ["lin_a", "lin_b", "conv", "pw", "to_q", "to_v"]
ADAPTED = ["lin_a", "lin_b", "conv", "conv_in", "pw", "blk.attn1.to_q", "blk.attn1.to_v"]
QKV = ["blk.attn1.to_q.weight", "blk.attn1.to_k.weight", "blk.attn1.to_v.weight"]


class Net:
    """the model surface DoRAWrapper reads (specs, store, device) over a frozen bf16 store of the shapes above"""

    def __init__(self, dev, output_axis):
        self.device, self.specs = dev, SPECS
        self.store = FlatParamStore([(n, U._store_shape(n, sh, k, None), "net") for n, sh, k, _ in SPECS],
                                    torch.bfloat16, dev, trainable=False)
        g = torch.Generator(device=dev).manual_seed(5)
        with torch.no_grad():
            for n, _, _, fan in SPECS:
                p = self.store.params[n]
                p.copy_((torch.rand(p.shape, generator=g, device=dev) * 2 - 1) / fan ** 0.5)
            self.store.params["conv_in.weight"][..., 4:] = 0      # the padded input channels: all-zero input lines
            w = self.store.params["lin_a.weight"]
            if output_axis:
                w[3, :] = 0                                       # an all-zero reduced line on the output axis
            else:
                w[:, 8] = 0
            self.store.params["lin_b.weight"][5, 7] = 320.0       # one element ~1e4 x the rest of its row and column


def _wrapper(dev, rank, output_axis, eps, seed=0):
    net = Net(dev, output_axis)
    w = DoRAWrapper(net, rank=rank, alpha=2.0, module_filter=FILTER, seed=seed, norm_epsilon=eps,
                    decompose_output_axis=output_axis)
    g = torch.Generator(device=dev).manual_seed(7 + rank)
    with torch.no_grad():
        for m in ADAPTED:
            up = w.store.params[f"lora_unet.{m}.lora_up.weight"]
            up.copy_(torch.randn(up.shape, generator=g, device=dev) * 0.05)
            sc = w.store.params[f"lora_unet.{m}.dora_scale"]
            sc.mul_(1 + 0.1 * torch.randn(sc.shape, generator=g, device=dev))
        if output_axis:
            w.store.params["lora_unet.lin_a.lora_up.weight"][3, :] = 0
        else:
            w.store.params["lora_unet.lin_a.lora_down.weight"][:, 8] = 0
    w.refresh()
    torch.cuda.synchronize()
    return net, w


def _mats(net, w, m):
    """(W, down, up, scale) of one module as float64 [out, kk, cin] / [r, kk, cin] / [out, r] / [kept]"""
    W = net.store.params[m + ".weight"].detach().float().cpu().numpy().astype(np.float64)
    out, cin = W.shape[0], W.shape[-1]
    W = W.reshape(out, -1, cin)
    d = w.store.params[f"lora_unet.{m}.lora_down.weight"].detach().cpu().numpy().astype(np.float64)
    u = w.store.params[f"lora_unet.{m}.lora_up.weight"].detach().cpu().numpy().astype(np.float64)
    sc = w.store.params[f"lora_unet.{m}.dora_scale"].detach().cpu().numpy().astype(np.float64).reshape(-1)
    return W, d.reshape(d.shape[0], -1, cin), u, sc


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("eps", [True, False])
@pytest.mark.parametrize("output_axis", [False, True])
@pytest.mark.parametrize("rank", [1, 4, 16, 32])
def test_merge_matches_oracle(dev, rank, output_axis, eps):
    net, w = _wrapper(dev, rank, output_axis, eps)
    axis = int(output_axis)
    tally = O.Bf16Tally()
    zero_lines = 0
    for m in ADAPTED:
        W, d, u, sc = _mats(net, w, m)
        wp, _, n = w.module_views(m)
        n_ref, wp_ref = O.merge(W, d, u, sc, w.scale, axis, w.eps)
        bound = O.norm_bound(W, d, u, w.scale, axis, w.eps)
        err = np.abs(n.cpu().numpy().astype(np.float64) - n_ref)
        print(m, "n: worst error / bound", float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (m, float(err.max()))
        assert torch.isfinite(wp.float()).all()
        tally.add(_bits(wp).reshape(-1), wp_ref.reshape(-1), m)
        zero = n_ref == w.eps                      # an all-zero reduced line: zeros, no NaN
        zero_lines += int(zero.sum())
        lines = wp.float().cpu().numpy().reshape(W.shape)
        assert not (lines[:, :, zero] if axis == 0 else lines[zero]).any()
    assert zero_lines >= (1 if output_axis else 5)  # lin_a's planted line (+ conv_in's padded channels, input axis)
    tally.check()
    # the member the filter leaves out: its rows of the fused q|k|v weight are the base weight, bit for bit
    ref = w.ref_for(QKV, (192, 64))
    assert torch.equal(ref.w[64:128], net.store.params[QKV[1]])
    assert not torch.equal(ref.w[:64], net.store.params[QKV[0]])
    # two runs give the same bits
    wp0, n0 = w.wp.clone(), w.norms.clone()
    w.norms.fill_(-1.0)
    w.refresh()
    torch.cuda.synchronize()
    assert torch.equal(wp0.view(torch.int16), w.wp.view(torch.int16)) and torch.equal(n0, w.norms)


def _project_all(w):
    for s in w.sites:
        w.ref_for([g + ".weight" for g in s.group]).done()
    w.flush()
    S.join()
    torch.cuda.synchronize()


@pytest.mark.parametrize("eps", [True, False])
@pytest.mark.parametrize("output_axis", [False, True])
@pytest.mark.parametrize("rank", [1, 4, 16, 32])
def test_projection_matches_oracle(dev, rank, output_axis, eps):
    net, w = _wrapper(dev, rank, output_axis, eps)
    axis = int(output_axis)
    g = torch.Generator(device=dev).manual_seed(11)
    G1 = torch.randn(w.g.shape, generator=g, device=dev).bfloat16()
    G2 = torch.randn(w.g.shape, generator=g, device=dev).bfloat16()
    w.g.copy_(G1)
    w.store.grad.fill_(7.0)                        # overwritten, not added to
    w.store.accumulating = False
    _project_all(w)
    first = w.store.grad.clone()
    w.store.grad.fill_(7.0)
    _project_all(w)
    assert torch.equal(first, w.store.grad)        # bit-repeatable
    w.g.copy_(G2)
    w.store.accumulating = True                    # the second micro-step of an accumulation window adds
    _project_all(w)
    w.store.accumulating = False
    leaves = ("lora_down.weight", "lora_up.weight", "dora_scale")
    for m in ADAPTED:
        W, d, u, sc = _mats(net, w, m)
        n = w.module_views(m)[2].cpu().numpy().astype(np.float64)    # the kernel's own fp32 n, as the projection reads it
        res = []
        for Gx in (G1, G2):
            w.g.copy_(Gx)
            Gm = w.module_views(m)[1].float().cpu().numpy().astype(np.float64).reshape(W.shape)
            res.append(O.project(Gm, W, d, u, sc, n, w.scale, axis))
        for i, leaf in enumerate(leaves):
            slot = w.store.slots[f"lora_unet.{m}.{leaf}"]
            one = first[slot.offset:slot.offset + slot.numel].cpu().numpy().astype(np.float64)
            two = w.store.grad[slot.offset:slot.offset + slot.numel].cpu().numpy().astype(np.float64)
            want1, b1 = res[0][0][i].reshape(-1), res[0][1][i].reshape(-1)
            want2, b2 = res[1][0][i].reshape(-1), res[1][1][i].reshape(-1)
            e1 = np.abs(one - want1)
            assert (e1 <= b1).all(), (m, leaf, float(e1.max()), float(b1[e1.argmax()]))
            e2 = np.abs(two - (want1 + want2))
            b12 = b1 + b2 + O.U * np.abs(want1 + want2)            # the add of the two micro-steps rounds once more
            assert (e2 <= b12).all(), (m, leaf, "accumulated", float(e2.max()))
            assert np.isfinite(two).all()
            assert np.abs(want1).max() > 0


def _dora_unet(dev, output_axis=False):
    a = U.UNet2DConditionModel(U.tiny_sdxl_config(), dev, seed=3, trainable=False)
    w = DoRAWrapper(a, rank=4, alpha=4.0, seed=1, decompose_output_axis=output_axis)
    g = torch.Generator(device=dev).manual_seed(2)
    with torch.no_grad():
        for n, p in w.store.named_parameters():
            if n.endswith("lora_up.weight"):
                p.copy_(torch.randn(p.shape, generator=g, device=dev) * 0.02)
    w.refresh()
    a.dora = w
    return a, w


def _inputs(dev):
    g = torch.Generator(device=dev).manual_seed(9)
    x = torch.zeros(2, 16, 16, 8, device=dev, dtype=torch.bfloat16)
    x[..., :4] = torch.randn(2, 16, 16, 4, generator=g, device=dev).bfloat16()
    t = torch.tensor([100, 700], device=dev)
    ehs = torch.randn(2, 77, 96, generator=g, device=dev).bfloat16()
    te = torch.randn(2, 64, generator=g, device=dev).bfloat16()
    ids = torch.tensor([[128, 128, 0, 0, 128, 128]] * 2, device=dev, dtype=torch.float32)
    return x, t, ehs, te, ids


def test_forward_and_weight_gradients_are_the_base_graphs(dev):
    a, w = _dora_unet(dev)
    b = U.UNet2DConditionModel(U.tiny_sdxl_config(), dev, seed=3, trainable=True)
    b._kv_batched = lambda *args: None     # the per-block K|V projection, as an adapted UNet runs it
    with torch.no_grad():
        b.store.data.copy_(a.store.data)
        for s in w.sites:
            off, n = s.span
            b0, b1 = a.store.range_of([g + ".weight" for g in s.group])
            b.store.data[b0:b1].copy_(w.wp[off:off + n])
    inp = _inputs(dev)
    target = torch.randn(2, 16, 16, 8, generator=torch.Generator(device=dev).manual_seed(4), device=dev)
    outs = []
    for net, store in ((a, w.store), (b, b.store)):
        y = net(*inp)
        loss = (y.float() - target).square().mean()
        store.begin_backward()
        loss.backward()
        store.finish_backward()
        torch.cuda.synchronize()
        outs.append(y.detach())
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    assert len(w.sites) > 40
    for s in w.sites:
        off, n = s.span
        b0, b1 = a.store.range_of([g + ".weight" for g in s.group])
        assert torch.equal(w.g[off:off + n].view(torch.int16), b.store.grad[b0:b1].view(torch.int16)), s.key
    assert w.store.grad.abs().sum() > 0 and torch.isfinite(w.store.grad).all()


def _cfg(tmp, **kw):
    cfg = TrainConfig.default_values()
    cfg.batch_size = 2
    cfg.learning_rate = 1e-3
    cfg.learning_rate_warmup_steps = 4
    cfg.workspace_dir = str(tmp)
    cfg.training_method = "LORA"
    cfg.lora_rank, cfg.lora_alpha = 8, 8.0
    cfg.lora_decompose = True
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _trainer(cfg, dev, seed=3):
    model = create.create_model(cfg, dev, seed=seed, unet_config=U.tiny_sdxl_config())
    tr = GenericTrainer(cfg, model=model)
    tr.start()
    return tr


def _batch(dev):
    return synthetic_sdxl_batch(2, 128, 128, dev, seed=1, te1_dim=48, te2_dim=48, pooled_dim=64)


def _leaf_moved(w, before, leaf):
    return any(not torch.equal(before[s.offset:s.offset + s.numel], w.store.data[s.offset:s.offset + s.numel])
               for n, s in w.store.slots.items() if n.endswith(leaf))


def test_training_save_and_backup(dev, tmp_path):
    batch = _batch(dev)
    tr = _trainer(_cfg(tmp_path), dev)
    w = tr.model.unet_lora
    assert isinstance(w, DoRAWrapper) and tr.model.unet.dora is w and tr.model.unet.lora is None
    before = w.store.data.clone()
    losses = [tr.train_step(batch).item() for _ in range(2)]
    path = tr.backup()
    losses.append(tr.train_step(batch).item())
    torch.cuda.synchronize()
    assert all(np.isfinite(losses))
    for leaf in ("dora_scale", "lora_down.weight", "lora_up.weight"):
        assert _leaf_moved(w, before, leaf), leaf
    # W' after the step is the merge of the stored parameters
    tally = O.Bf16Tally()
    base = tr.model.unet
    for m in ("conv_in", "down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_k",
              "down_blocks.1.attentions.0.proj_in", "mid_block.resnets.0.conv1", "up_blocks.0.resnets.0.conv_shortcut"):
        W, d, u, sc = _mats(base, w, m)
        wp, _, n = w.module_views(m)
        n_ref, wp_ref = O.merge(W, d, u, sc, w.scale, 0, w.eps)
        assert (np.abs(n.cpu().numpy() - n_ref) <= O.norm_bound(W, d, u, w.scale, 0, w.eps)).all(), m
        tally.add(_bits(wp).reshape(-1), wp_ref.reshape(-1), m)
    tally.check()
    # save -> load: the state comes back bit for bit, dora_scale in the reference's key and shape
    sd = {k: v.clone() for k, v in w.state_dict().items()}
    assert sd["lora_unet.conv_in.dora_scale"].shape == (1, 4, 1, 1)
    assert sd["lora_unet.time_embedding.linear_1.dora_scale"].shape == (1, 64)
    dest = os.path.join(tmp_path, "out", "dora.safetensors")
    from onetrainer_amd.modelSaver import create_model_saver
    create_model_saver(tr.config.model_type, "LORA").save(tr.model, tr.config, "SAFETENSORS", dest)
    from safetensors.torch import load_file
    loaded = load_file(dest)
    assert set(loaded) == set(sd)
    fresh = DoRAWrapper(U.UNet2DConditionModel(U.tiny_sdxl_config(), dev, seed=3, trainable=False), rank=8, alpha=8.0,
                        seed=5)
    fresh.load_state_dict(loaded)
    torch.cuda.synchronize()
    assert torch.equal(fresh.store.data, w.store.data)
    assert torch.equal(fresh.wp.view(torch.int16), w.wp.view(torch.int16))
    # a plain-LoRA file leaves dora_scale at its init
    plain = {k: v for k, v in loaded.items() if not k.endswith("dora_scale")}
    fresh2 = DoRAWrapper(U.UNet2DConditionModel(U.tiny_sdxl_config(), dev, seed=3, trainable=False), rank=8, alpha=8.0,
                         seed=5)
    init_scale = fresh2.store.params["lora_unet.conv_in.dora_scale"].clone()
    fresh2.load_state_dict(plain)
    assert torch.equal(fresh2.store.params["lora_unet.conv_in.dora_scale"], init_scale)
    assert torch.equal(fresh2.store.params["lora_unet.conv_in.lora_up.weight"],
                       w.store.params["lora_unet.conv_in.lora_up.weight"])
    # INTERNAL backup -> resume: the next step is bit-identical to the uninterrupted run
    assert path and os.path.isfile(os.path.join(path, "lora", "lora.safetensors"))
    cfg_b = _cfg(tmp_path, continue_last_backup=True)
    b = _trainer(cfg_b, dev)
    assert b.model.train_progress.global_step == 2
    loss_b = b.train_step(batch).item()
    torch.cuda.synchronize()
    assert loss_b == losses[2]
    assert torch.equal(b.model.train_store.data, w.store.data)
    assert torch.equal(b.model.unet_lora.wp.view(torch.int16), w.wp.view(torch.int16))


def test_gradient_accumulation_adds(dev, tmp_path):
    """two micro-steps of one accumulation window: G is overwritten, the adapter gradients add up"""
    batch = _batch(dev)
    tr = _trainer(_cfg(tmp_path, gradient_accumulation_steps=2, learning_rate_warmup_steps=0), dev)
    w = tr.model.unet_lora
    tr.train_step(batch)
    torch.cuda.synchronize()
    g1 = w.store.grad.clone()
    assert w.store.accumulating and g1.abs().sum() > 0
    before = w.store.data.clone()
    tr.train_step(batch)                           # the update step: the window's sum reaches the optimizer
    torch.cuda.synchronize()
    assert not w.store.accumulating
    assert not torch.equal(before, w.store.data) and torch.isfinite(w.store.data).all()


@pytest.mark.parametrize("variant", ["ema", "adafactor", "output_axis_no_eps", "sd15"])
def test_one_step_with_pointwise_users(dev, tmp_path, variant):
    """EMA and Adafactor over the adapter store, the output axis without the epsilon, and the SD 1.5 plugin (1x1 conv
    projections held as linears): two steps run, stay finite and move dora_scale"""
    kw = {}
    if variant == "ema":
        kw = dict(ema="GPU", ema_decay=0.9, ema_update_step_interval=1)
    if variant == "output_axis_no_eps":
        kw = dict(lora_decompose_output_axis=True, lora_decompose_norm_epsilon=False)
    cfg = _cfg(tmp_path, **kw)
    if variant == "adafactor":
        cfg.optimizer.optimizer = "ADAFACTOR"
        cfg.optimizer.scale_parameter = False
        cfg.optimizer.relative_step = False
        cfg.optimizer.warmup_init = False
    batch = _batch(dev)
    if variant == "sd15":
        cfg.model_type = "STABLE_DIFFUSION_15"
        tr = GenericTrainer(cfg, model=create.create_model(cfg, dev, seed=3, unet_config=U.tiny_sd15_config()))
        tr.start()
        assert type(tr.model_setup).__name__ == "StableDiffusionLoRASetup"
        batch = synthetic_sdxl_batch(2, 128, 128, dev, seed=1, te1_dim=96, sdxl=False, scaling_factor=0.18215)
    else:
        tr = _trainer(cfg, dev)
    w = tr.model.unet_lora
    assert isinstance(w, DoRAWrapper)
    assert w.output_axis == (variant == "output_axis_no_eps") and (w.eps == 0.0) == (variant == "output_axis_no_eps")
    before = w.store.data.clone()
    losses = [tr.train_step(batch).item() for _ in range(2)]
    torch.cuda.synchronize()
    assert all(np.isfinite(losses))
    assert _leaf_moved(w, before, "dora_scale")
    assert torch.isfinite(w.store.data).all() and torch.isfinite(w.wp.float()).all()
    if variant == "ema":
        assert tr.model.ema is not None


def test_step_has_no_stream_races(dev, tmp_path):
    cfg = _cfg(tmp_path)
    cfg.batch_size = 1
    tr = _trainer(cfg, dev)
    batch = synthetic_sdxl_batch(1, 128, 128, dev, seed=0, te1_dim=48, te2_dim=48, pooled_dim=64)
    tr.train_step(batch)
    torch.cuda.synchronize()
    with StreamHazardCheck() as chk:
        tr.train_step(batch)
    torch.cuda.synchronize()
    assert chk.regions > 10 and chk.kernel_calls > 100 and chk.checked > 100, chk.report()
    assert not chk.hazards, chk.report()
