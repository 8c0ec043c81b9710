"""The augmentation oracle (_oracle_augment.py), pinned against things it did not come from (CPU): hue against the
standard library's colorsys, brightness / saturation / contrast against PIL's ImageEnhance, rotation against
np.rot90 and PIL's Image.rotate; the parameter draws of dataLoader/augment.py; and the float32-against-float64
figures the kernel's tolerance is taken from."""
import colorsys
import math

import numpy as np
import pytest

import _oracle_augment as O
from onetrainer_amd.dataLoader import augment as A


def _rgb(seed=0, H=24, W=31):
    rng = np.random.default_rng(seed)
    img = rng.random((3, H, W))
    img[:, 0, :6] = np.array([[0.0] * 3, [1.0] * 3, [0.5] * 3, [0.2] * 3, [1.0, 0.0, 0.0], [0.3, 0.3, 0.9]]).T
    return img


@pytest.mark.parametrize("f", [0.0 + 1e-9, 0.2, 0.5, -0.45, -0.3, 0.999, -0.999])
def test_hue_matches_colorsys(f):
    """pixel by pixel, gray and black pixels included; the shifts wrap through 0 (negative) and through 1"""
    img = _rgb()
    got = O.hue(img, f)
    wrapped_low = wrapped_high = 0
    for i in range(img.shape[1]):
        for j in range(img.shape[2]):
            h, s, v = colorsys.rgb_to_hsv(*img[:, i, j])
            wrapped_low += h + f < 0
            wrapped_high += h + f >= 1
            want = colorsys.hsv_to_rgb((h + f) % 1.0, s, v)
            assert np.abs(got[:, i, j] - want).max() < 1e-12, (i, j, img[:, i, j])
    assert np.array_equal(got[:, 0, :4], img[:, 0, :4])             # black, white, grays: untouched
    if f < 0:
        assert wrapped_low > 0
    if f > 0.1:
        assert wrapped_high > 0


def _u8(img):
    return np.round(img * 255.0).astype(np.uint8)


@pytest.mark.parametrize("name,factor", [("Brightness", 0.6), ("Brightness", 1.4), ("Color", 0.3), ("Color", 1.7),
                                         ("Contrast", 0.5), ("Contrast", 1.5)])
def test_colour_stages_match_pil(name, factor):
    """PIL's ImageEnhance blends the 8-bit image with a degenerate one (black; its 'L' conversion; the rounded mean of
    that) and rounds to 8 bits.  Against the oracle on the same 8-bit image, in units of 1/255:
      * the blend's own rounding / truncation to 8 bits: 1;
      * the degenerate image is itself 8-bit: PIL's 'L' uses the ITU-R 601 weights (0.299, 0.587, 0.114) in 16-bit
        fixed point, the oracle (0.2989, 0.587, 0.114) -- a difference of at most 0.0001 * 255 < 0.03 -- plus the
        rounding of L to 8 bits, 0.5, and for contrast the rounding of the mean, another 0.5: at most 1.03 units,
        weighted by |1 - factor| <= 0.7: 0.73.
    Together below 2 units of 1/255."""
    from PIL import Image, ImageEnhance
    img8 = _u8(_rgb(1))
    pil = Image.fromarray(np.ascontiguousarray(img8.transpose(1, 2, 0)), mode="RGB")
    want = np.asarray(getattr(ImageEnhance, name)(pil).enhance(factor)).transpose(2, 0, 1).astype(np.float64)
    x = img8.astype(np.float64) / 255.0
    got = {"Brightness": O.brightness, "Color": O.saturation, "Contrast": O.contrast}[name](x, factor) * 255.0
    assert np.abs(got - want).max() <= 2.0, np.abs(got - want).max()
    assert np.abs(got - x * 255.0).max() > 20.0                      # the stage did something


def _rot_entry(H, W, angle):
    a = math.radians(angle)
    return {"C": 3, "y0": 0, "x0": 0, "H": H, "W": W, "flip": 0, "cos_a": math.cos(a) if angle else 1.0,
            "sin_a": math.sin(a) if angle else 0.0}


def test_rotation_identity_and_quarter_turn():
    img = _rgb(2, 32, 32)
    assert np.array_equal(O.geometry(img, _rot_entry(32, 32, 0.0)), img)
    got = O.geometry(img, _rot_entry(32, 32, 90.0))
    want = np.stack([np.rot90(c, 1) for c in img])                 # counter-clockwise
    assert np.abs(got - want).max() < 1e-6                          # cos 90 degrees is 6e-17 (and 4e-8 as float32)


def test_rotation_turns_counter_clockwise_like_pil():
    from PIL import Image
    y, x = np.mgrid[0:48, 0:48]
    plane = (0.5 + 0.5 * np.sin(0.3 * x) * np.cos(0.2 * y + 0.05 * x)).astype(np.float32)
    got = O.geometry(np.stack([plane] * 3), _rot_entry(48, 48, 17.0))[0]
    pil = Image.fromarray(plane, mode="F")
    plus = np.asarray(pil.rotate(17.0, resample=Image.BILINEAR))
    minus = np.asarray(pil.rotate(-17.0, resample=Image.BILINEAR))
    inner = (slice(12, 36), slice(12, 36))                           # away from the corners that leave the picture
    e_plus, e_minus = np.abs(got - plus)[inner].max(), np.abs(got - minus)[inner].max()
    assert e_plus < 0.02 and e_minus > 10 * e_plus, (e_plus, e_minus)


def test_flip_and_crop_are_slices():
    img = _rgb(3, 20, 30)
    e = dict(_rot_entry(11, 13, 0.0), y0=4, x0=9, flip=1)
    assert np.array_equal(O.geometry(img, e), img[:, 4:15, 9:22][:, :, ::-1])


def test_taps_outside_the_crop_are_zero():
    """the source is all ones, the crop strictly inside it: a rotated crop still fades to 0 at its corners"""
    e = dict(_rot_entry(16, 16, 45.0), y0=8, x0=8)
    got = O.geometry(np.ones((3, 32, 32)), e)
    assert got[0, 0, 0] == 0.0 and got[0, 8, 8] == 1.0


# ---- the draws --------------------------------------------------------------------------------------------------------
ALL_ON = {"enable_crop_jitter": True, "enable_random_flip": True, "enable_random_rotate": True,
          "random_rotate_max_angle": 10.0, "enable_random_brightness": True, "random_brightness_max_strength": 0.2,
          "enable_random_contrast": True, "random_contrast_max_strength": 0.3, "enable_random_saturation": True,
          "random_saturation_max_strength": 0.4, "enable_random_hue": True, "random_hue_max_strength": 0.1}


def test_draws_match_the_oracle_and_their_ranges():
    seen_flip = set()
    for index in range(40):
        for v in range(3):
            p = A.draw(ALL_ON, 7, index, v, (80, 64), (64, 64))
            assert p == O.draw(ALL_ON, 7, index, v, (80, 64), (64, 64))
            assert 0 <= p["y0"] <= 16 and p["x0"] == 0
            assert abs(p["angle"]) <= 10.0 and abs(p["cos_a"] - math.cos(math.radians(p["angle"]))) < 1e-15
            assert 0.8 <= p["brightness"] <= 1.2 and 0.7 <= p["contrast"] <= 1.3 and 0.6 <= p["saturation"] <= 1.4
            assert abs(p["hue"]) <= 0.05
            seen_flip.add(p["flip"])
    assert seen_flip == {0, 1}
    assert A.draw({"enable_random_brightness": True, "random_brightness_max_strength": 3.0}, 0, 0, 0, (8, 8), (8, 8)
                  )["brightness"] >= 0.0


def test_draws_depend_only_on_seed_index_variation():
    """the same for any bucket grouping and batch size (neither is an argument), different across variations,
    images and seeds"""
    p = A.draw(ALL_ON, 7, 3, 1, (80, 64), (64, 64))
    assert p == A.draw(dict(ALL_ON), 7, 3, 1, (80, 64), (64, 64))
    others = [A.draw(ALL_ON, 7, 3, 0, (80, 64), (64, 64)), A.draw(ALL_ON, 7, 3, 2, (80, 64), (64, 64)),
              A.draw(ALL_ON, 7, 4, 1, (80, 64), (64, 64)), A.draw(ALL_ON, 8, 3, 1, (80, 64), (64, 64))]
    for o in others:
        assert o != p and o["angle"] != p["angle"] and o["hue"] != p["hue"]
    # switching one augmentation off leaves the others where they were
    fewer = {k: v for k, v in ALL_ON.items() if k != "enable_random_rotate"}
    q = A.draw(fewer, 7, 3, 1, (80, 64), (64, 64))
    assert q["angle"] == 0.0 and {k: q[k] for k in ("flip", "brightness", "hue", "y0")} == \
        {k: p[k] for k in ("flip", "brightness", "hue", "y0")}


def test_fixed_switches_give_the_upper_ends():
    cfg = {k.replace("enable_random_", "enable_fixed_"): v for k, v in ALL_ON.items()}
    cfg["enable_random_flip"] = cfg["enable_random_rotate"] = True      # fixed wins over random
    for index in range(5):
        p = A.draw(cfg, 1, index, 0, (64, 64), (64, 64))
        assert p["flip"] == 1 and p["angle"] == 10.0
        assert (p["brightness"], p["contrast"], p["saturation"], p["hue"]) == (1.2, 1.3, 1.4, 0.05)
        assert p == O.draw(cfg, 1, index, 0, (64, 64), (64, 64))


def test_absent_keys_are_off():
    for cfg in (None, {}, {"random_rotate_max_angle": 30.0, "random_hue_max_strength": 0.5,
                           "enable_resolution_override": True}):
        p = A.draw(cfg, 5, 2, 1, (80, 70), (64, 64))
        assert A.is_neutral(p) and (p["y0"], p["x0"]) == (8, 3)          # the centre crop
        assert not A.enabled(cfg)
    assert A.enabled({"enable_crop_jitter": True}) and A.enabled({"enable_fixed_hue": True})
    assert A.variations({}) == 1 and A.variations({"image_variations": 4}) == 4
    with pytest.raises(ValueError):
        A.variations({"image_variations": -1})


# ---- the kernel's tolerance -------------------------------------------------------------------------------------------
def test_stage_errors_measured():
    """STAGE_ERR_F32 recomputed: the float32 oracle against the float64 oracle on the GPU test's own inputs
    (within a tenth: NumPy's float32 sum order differs between builds); the float32 oracle passes the 4 x bound it
    sets for the kernel, and the bound is far below one 8-bit step"""
    got = O.measure_stage_errors()
    print(got)
    for s in O.STAGES:
        assert abs(got[s] - O.STAGE_ERR_F32[s]) <= 0.1 * O.STAGE_ERR_F32[s], (s, got[s], O.STAGE_ERR_F32[s])
        assert got[s] <= 4 * O.STAGE_ERR_F32[s]
        assert 0 < 4 * O.STAGE_ERR_F32[s] < 0.01 / 255


def test_gpu_cases_cover_what_they_claim():
    cases = O.gpu_cases()
    odd = cases["odd"][1]
    assert len(odd) == 5 and {(e["H"], e["W"], e["Hs"], e["Ws"]) for e in odd} == {(37, 53, 41, 64)}
    assert {(e["y0"], e["x0"]) for e in odd[:4]} == {(0, 0), (4, 11), (0, 11), (4, 0)}
    assert sorted(e["angle"] for e in odd[:4]) == [-7.5, 0.0, 7.5, 45.0] and odd[4]["C"] == 1
    assert {O.last_stage(e) for e in odd} == {"hue", "contrast", "geometry"}
    assert cases["square"][1][0]["angle"] == 90.0 and cases["wide"][1][0]["contrast"] == 0.0
    for name, (flat, ents, H, W, out_numel) in cases.items():
        spans = sorted((e["out_off"], e["out_off"] + e["C"] * H * W) for e in ents)
        assert spans[0][0] == 0 and spans[-1][1] == out_numel
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])), name      # disjoint, no gaps
        for e in ents:
            assert e["src_off"] + e["C"] * e["Hs"] * e["Ws"] <= flat.size and flat.dtype == np.float32
            assert 0 <= e["y0"] <= e["Hs"] - H and 0 <= e["x0"] <= e["Ws"] - W
    # a contrast of 0 leaves the constant mean
    e, plane = O.case_planes(cases["wide"])[0]
    out = O.augment(plane, e)
    assert np.ptp(out) == 0.0 and 0.2 < out[0, 0, 0] < 0.8
