"""csrc/augment.hip (K.image_augment) against the float64 oracle on every output pixel, and the augmented latent
cache end to end on the device.

Tolerance: an entry's bound is 4 x _oracle_augment.STAGE_ERR_F32 of the last stage it runs -- the float32 oracle's
own error against float64 on these very inputs (recomputed by test_augment_oracle.py); the 4 covers the kernel's
different, fixed summation order in the mean and its coordinate arithmetic.  Measured kernel errors:
_oracle_augment.KERNEL_ERR and DESIGN.md."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _oracle_augment as O
from onetrainer_amd import _lib
from onetrainer_amd import kernels as K
from onetrainer_amd.dataLoader import augment as A

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _cases():
    return O.gpu_cases()


@functools.lru_cache(maxsize=None)
def _reference(name):
    """float64 oracle output of every entry of a case (computed once, never written to)"""
    return tuple(O.augment(plane, e) for e, plane in O.case_planes(_cases()[name]))


def _run(dev, name):
    flat, ents, H, W, out_numel = _cases()[name]
    out = A.device_augment(ents, torch.from_numpy(flat).to(dev), out_numel, H, W)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("name", ["odd", "square", "wide"])
def test_kernel_matches_oracle_on_every_pixel(dev, name):
    flat, ents, H, W, out_numel = _cases()[name]
    got = _run(dev, name)
    assert got.shape == (out_numel,) and np.isfinite(got).all()
    for e, ref in zip(ents, _reference(name)):
        g = got[e["out_off"]:e["out_off"] + e["C"] * H * W].reshape(e["C"], H, W).astype(np.float64)
        err = np.abs(g - ref).max()
        stage = O.last_stage(e)
        print(f"{name} entry C={e['C']} angle={e['angle']} last stage {stage}: max err {err:.3e} "
              f"(bound {4 * O.STAGE_ERR_F32[stage]:.3e})")
        assert err <= 4 * O.STAGE_ERR_F32[stage], (name, stage, err)
        assert g.min() >= 0.0 and g.max() <= 1.0 + 1e-6


def test_contrast_zero_leaves_the_mean(dev):
    """256 x 320 at contrast 0: the gray sum spans 2 x 16 workgroups, and every output pixel is the one constant m"""
    flat, ents, H, W, _ = _cases()["wide"]
    got = _run(dev, "wide")
    assert np.ptp(got) == 0.0
    m = float(_reference("wide")[0][0, 0, 0])
    assert abs(float(got[0]) - m) <= 4 * O.STAGE_ERR_F32["contrast"]


def test_crop_and_flip_are_bit_exact(dev):
    flat, ents, H, W, _ = _cases()["copy"]
    got = _run(dev, "copy")
    for e, ref in zip(ents, _reference("copy")):
        g = got[e["out_off"]:e["out_off"] + 3 * H * W].reshape(3, H, W)
        assert np.array_equal(g, ref.astype(np.float32)), (e["y0"], e["x0"], e["flip"])
    # the odd-sized mask-free path: entry 0 of "odd" without its colour factors and turn is a flip-only copy
    flat, ents, H, W, out_numel = _cases()["odd"]
    plain = [dict(e, cos_a=1.0, sin_a=0.0, angle=0.0, brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0)
             for e in ents]
    out = A.device_augment(plain, torch.from_numpy(flat).to(dev), out_numel, H, W).cpu().numpy()
    for e, (_, plane) in zip(plain, O.case_planes(_cases()["odd"])):
        g = out[e["out_off"]:e["out_off"] + e["C"] * H * W].reshape(e["C"], H, W)
        assert np.array_equal(g, O.geometry(plane, e, np.float32))


def test_two_runs_give_equal_bits(dev):
    for name in ("odd", "wide"):
        assert np.array_equal(_run(dev, name).view(np.uint32), _run(dev, name).view(np.uint32))


def test_launcher_refuses_entries_outside_the_buffers(dev):
    """an argument check on the host copy of the table, before any launch"""
    flat, ents, H, W, out_numel = _cases()["copy"]
    src = torch.from_numpy(flat).to(dev)
    out = torch.full((out_numel,), -1.0, device=dev)

    def call(entries, out_t=out, src_t=src):
        tab = A.pack_table(entries)
        raw = torch.frombuffer(memoryview(tab).cast("B"), dtype=torch.uint8).to(dev)
        return K.image_augment(raw, tab, len(entries), src_t, out_t, H, W)

    bad = [dict(ents[0], src_off=flat.size - 10),                    # the source plane runs past the buffer
           dict(ents[0], src_off=-4), dict(ents[0], out_off=out_numel - 5), dict(ents[0], out_off=-1),
           dict(ents[0], y0=ents[0]["Hs"] - H + 1), dict(ents[0], x0=ents[0]["Ws"] - W + 1), dict(ents[0], x0=-1),
           dict(ents[0], Hs=4000), dict(ents[0], C=2), dict(ents[0], H=H + 1), dict(ents[0], flip=2),
           dict(ents[0], cos_a=float("nan")), dict(ents[0], cos_a=0.5, sin_a=0.5), dict(ents[0], contrast=-0.1),
           dict(ents[0], hue=float("inf"))]
    for e in bad:
        with pytest.raises(RuntimeError, match="invalid arguments"):
            call([ents[1], e])
    with pytest.raises(RuntimeError, match="invalid arguments"):
        call(ents[:1], out_t=out[:3 * H * W - 4])
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())                                  # nothing was launched
    ws = _lib.lib().otamd_image_augment_ws_floats(2, H, W)
    tab = A.pack_table(ents[:2])
    small = torch.empty(ws - 1, device=dev)
    rc = _lib.lib().otamd_image_augment(out.data_ptr(), C.cast(tab, C.c_void_p), 2, H, W, src.data_ptr(), src.numel(),
                                        out.data_ptr(), out.numel(), small.data_ptr(), small.numel(), None)
    assert rc == _lib.OTAMD_EINVAL
    call(ents)                                                        # and the good table runs
    torch.cuda.synchronize()
    assert bool((out >= 0.0).all())


def test_cache_end_to_end_on_the_device(dev, tmp_path):
    """tiny SD 1.5 VAE, two 64 x 64 images (70 x 64 sources, so the jitter has room), V = 3, flip + jitter + hue: the
    cache is built on the device and read for four epochs; variation v's latent is the encoder applied to the
    oracle's image (the VAE test's tolerance: 3e-2 of the latent range); an unaugmented build gives the bytes of a
    writer whose augment_fn raises"""
    from safetensors.torch import load_file

    from onetrainer_amd.dataLoader.aspect_bucketing import SingleAspectCalculation
    from onetrainer_amd.dataLoader.create import concept_extras
    from onetrainer_amd.dataLoader.latent_cache import LatentCacheDataLoader, LatentCacheWriter, scale_only
    from onetrainer_amd.module import vae as V
    enc = V.AutoencoderKLEncoder(V.tiny_vae_config(), dev, seed=1)
    encode = lambda im: enc.encode(im)  # noqa: E731
    g = torch.Generator().manual_seed(5)
    imgs = [torch.rand(3, 70, 64, generator=g), torch.rand(3, 64, 72, generator=g)]
    image_cfg = {"enable_crop_jitter": True, "enable_random_flip": True, "enable_random_hue": True,
                 "random_hue_max_strength": 0.3}
    concept = {"path": "x", "seed": 4, "image_variations": 3, "image": image_cfg}
    rows = [dict({"image": im}, **concept_extras(concept, i)) for i, im in enumerate(imgs)]
    bucket = SingleAspectCalculation(64)
    LatentCacheWriter(encode, str(tmp_path / "aug"), bucket, dev).write(rows)
    for i, im in enumerate(imgs):
        scale_res, crop_res = bucket.bucket_for(im.shape[1], im.shape[2])
        assert crop_res == (64, 64) and scale_res != crop_res
        src = scale_only(im, scale_res).numpy()
        oracle = np.stack([O.augment(src, A.entry(O.draw(image_cfg, 4, i, v, scale_res, crop_res), 0, 0, 3, scale_res,
                                                  crop_res)) for v in range(3)]).astype(np.float32)
        want = enc.encode(torch.from_numpy(oracle).to(dev)).float().cpu()
        for v in range(3):
            rec = load_file(str(tmp_path / "aug" / (f"{i:08d}.safetensors" if v == 0 else f"{i:08d}.v{v}.safetensors")))
            err = (rec["latent_image"] - want[v]).abs().max() / want[v].abs().max()
            assert err < 3e-2, (i, v, err)
        assert (want[0] - want[1]).abs().max() / want[0].abs().max() > 3e-2     # the variations are different pictures
    dl = LatentCacheDataLoader(str(tmp_path / "aug"), 2, dev, prefetch=False)
    seen = []
    for epoch in range(4):
        dl.start_next_epoch()
        (batch,) = list(dl.get_data_loader())
        order = np.argsort(dl._batches[0])
        seen.append(batch["latent_image"][torch.as_tensor(order, device=dev)].cpu())
        for k, i in enumerate(dl._batches[0]):
            v = epoch % 3
            rec = load_file(str(tmp_path / "aug" / (f"{i:08d}.safetensors" if v == 0 else f"{i:08d}.v{v}.safetensors")))
            assert torch.equal(batch["latent_image"][k].permute(1, 2, 0).cpu(), rec["latent_image"])
    assert torch.equal(seen[0], seen[3]) and not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])

    def never(*a, **k):
        raise AssertionError("augment_fn called")
    plain = [{"image": im} for im in imgs]
    LatentCacheWriter(encode, str(tmp_path / "p1"), bucket, dev).write(
        [dict(r, **concept_extras({"path": "x"}, i)) for i, r in enumerate(plain)])
    LatentCacheWriter(encode, str(tmp_path / "p2"), bucket, dev, augment_fn=never).write(plain)
    names = sorted(p.name for p in (tmp_path / "p1").iterdir())
    assert names == ["00000000.safetensors", "00000001.safetensors", "index.json"]
    for n in names:
        assert (tmp_path / "p1" / n).read_bytes() == (tmp_path / "p2" / n).read_bytes(), n
