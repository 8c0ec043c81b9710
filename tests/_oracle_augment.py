"""NumPy restatement of csrc/augment.hip and of dataLoader/augment.py's parameter draws (test-side oracle).

`augment` runs the five stages in float64 (the reference) or, with dtype=np.float32, in the kernel's own precision
and operation order -- the float32 run is what the kernel's tolerance is measured from.  A stage whose factor is
neutral (no rotation, 1, 1, 1, 0) is not run, as in the kernel.  The oracle itself is pinned by
test_augment_oracle.py against colorsys, PIL's ImageEnhance / Image.rotate and np.rot90.

Tolerance of the kernel (tests/test_augment_gpu.py): STAGE_ERR_F32[s] is the worst absolute error, over every
pixel of every entry of `gpu_cases()`, of the float32 oracle against the float64 oracle with the pipeline cut after
stage s (errors are cumulative: a stage carries what the stages before it left).  An entry's bound is 4 x the figure
of the last stage it runs; the 4 covers the kernel's different (fixed) summation order in the mean and its coordinate
arithmetic.  test_augment_oracle.py recomputes the figures.  KERNEL_ERR holds what the kernel showed on an MI355X.
"""
import math
import random

import numpy as np

STAGES = ("geometry", "brightness", "contrast", "saturation", "hue")

# worst |float32 oracle - float64 oracle| with the pipeline cut after each stage, over gpu_cases()
STAGE_ERR_F32 = {"geometry": 2.57e-6, "brightness": 2.84e-6, "contrast": 3.51e-6, "saturation": 3.51e-6,
                 "hue": 3.51e-6}
# worst |kernel - float64 oracle| per last stage run, measured on an MI355X
KERNEL_ERR = {"geometry": 1.37e-6, "contrast": 3.57e-6, "hue": 2.46e-6}   # bounds: 1.03e-5, 1.40e-5, 1.40e-5


def _clamp01(x):
    return np.minimum(np.maximum(x, x.dtype.type(0)), x.dtype.type(1))


def gray(img):
    t = img.dtype.type
    return (t(0.2989) * img[0] + t(0.587) * img[1]) + t(0.114) * img[2]


def geometry(src, e, dtype=np.float64):
    """crop at (y0, x0), flip, rotate: [C, Hs, Ws] -> [C, H, W]"""
    t = np.dtype(dtype).type
    H, W = e["H"], e["W"]
    crop = np.asarray(src)[:, e["y0"]:e["y0"] + H, e["x0"]:e["x0"] + W]
    if e["flip"]:
        crop = crop[:, :, ::-1]
    cos_a, sin_a = np.float32(e["cos_a"]), np.float32(e["sin_a"])   # the table holds float32
    if cos_a == 1 and sin_a == 0:
        return np.ascontiguousarray(crop).astype(dtype)
    crop = crop.astype(dtype)
    cos_a, sin_a = t(cos_a), t(sin_a)
    cx, cy = t(W - 1) * t(0.5), t(H - 1) * t(0.5)
    yo = (np.arange(H, dtype=dtype) - cy)[:, None]
    xo = (np.arange(W, dtype=dtype) - cx)[None, :]
    xs = (cos_a * xo - sin_a * yo) + cx
    ys = (sin_a * xo + cos_a * yo) + cy
    fx, fy = np.floor(xs), np.floor(ys)
    ax, ay = xs - fx, ys - fy
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    one = t(1)

    def tap(y, x):
        inside = (y >= 0) & (y < H) & (x >= 0) & (x < W)
        v = crop[:, np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)]
        return np.where(inside[None], v, t(0))

    w00, w01, w10, w11 = (one - ax) * (one - ay), ax * (one - ay), (one - ax) * ay, ax * ay
    return ((w00 * tap(iy, ix) + w01 * tap(iy, ix + 1)) + w10 * tap(iy + 1, ix)) + w11 * tap(iy + 1, ix + 1)


def brightness(img, b):
    return _clamp01(img * img.dtype.type(b))


def contrast(img, c, mean=None):
    """mean: the image mean of gray (computed here when None)"""
    t = img.dtype.type
    if mean is None:
        mean = gray(img).sum(dtype=img.dtype) / t(img.shape[1] * img.shape[2])
    cm = (t(1) - t(c)) * t(mean)
    return _clamp01(t(c) * img + cm)


def saturation(img, s):
    t = img.dtype.type
    sg = (t(1) - t(s)) * gray(img)
    return _clamp01(t(s) * img + sg[None])


def hue(img, f):
    t = img.dtype.type
    r, g, b = img[0], img[1], img[2]
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    d = mx - mn
    chroma = d != 0
    ds, ms = np.where(chroma, d, t(1)), np.where(chroma, mx, t(1))
    sat = d / ms
    h = np.where(r == mx, (g - b) / ds, np.where(g == mx, t(2) + (b - r) / ds, t(4) + (r - g) / ds))
    h = h / t(6) + t(f)
    h = h - np.floor(h)
    h6 = h * t(6)
    fi = np.floor(h6)
    fr = h6 - fi
    one = t(1)
    p, q, tt = mx * (one - sat), mx * (one - sat * fr), mx * (one - sat * (one - fr))
    i = fi.astype(np.int64) % 6
    out_r = np.choose(i, [mx, q, p, p, tt, mx])
    out_g = np.choose(i, [tt, mx, mx, q, p, p])
    out_b = np.choose(i, [p, p, tt, mx, mx, q])
    return np.stack([np.where(chroma, out_r, r), np.where(chroma, out_g, g), np.where(chroma, out_b, b)])


def last_stage(e):
    """the last stage the entry runs (its error class)"""
    f32 = np.float32
    last = "geometry"
    if f32(e["brightness"]) != 1:
        last = "brightness"
    if e["C"] == 3:
        for name, neutral in (("contrast", 1), ("saturation", 1), ("hue", 0)):
            if f32(e[name]) != neutral:
                last = name
    return last


def augment(src, e, dtype=np.float64, upto="hue"):
    """one entry: src [C, Hs, Ws] in [0, 1] -> [C, H, W]; the factors are read as the float32 the table holds;
    the pipeline stops after stage `upto`"""
    f32 = np.float32
    stop = STAGES.index(upto)
    x = geometry(src, e, dtype)
    if stop >= 1 and f32(e["brightness"]) != 1:
        x = brightness(x, f32(e["brightness"]))
    if e["C"] == 3:
        if stop >= 2 and f32(e["contrast"]) != 1:
            x = contrast(x, f32(e["contrast"]))
        if stop >= 3 and f32(e["saturation"]) != 1:
            x = saturation(x, f32(e["saturation"]))
        if stop >= 4 and f32(e["hue"]) != 0:
            x = hue(x, f32(e["hue"]))
    return x


def augment_fn(entries, src, out_numel, H, W):
    """LatentCacheWriter's augment_fn on the oracle (float64, returned as the float32 the kernel writes)"""
    import torch
    flat = src.detach().cpu().numpy()
    out = np.zeros(int(out_numel), dtype=np.float32)
    for e in entries:
        assert (e["H"], e["W"]) == (H, W)
        n = e["C"] * e["Hs"] * e["Ws"]
        plane = flat[e["src_off"]:e["src_off"] + n].reshape(e["C"], e["Hs"], e["Ws"])
        out[e["out_off"]:e["out_off"] + e["C"] * H * W] = augment(plane, e).astype(np.float32).reshape(-1)
    return torch.from_numpy(out).to(src.device)


# ---- the draws --------------------------------------------------------------------------------------------------------
def draw(image_cfg, seed, index, variation, scale_res, crop_res):
    """dataLoader/augment.py:draw restated"""
    cfg = image_cfg or {}
    rng = random.Random(f"augment/{int(seed)}/{int(index)}/{int(variation)}")
    u = [rng.random() for _ in range(6)]   # flip, rotate, brightness, contrast, saturation, hue
    dy, dx = scale_res[0] - crop_res[0], scale_res[1] - crop_res[1]
    if cfg.get("enable_crop_jitter"):
        y0, x0 = rng.randint(0, max(dy, 0)), rng.randint(0, max(dx, 0))
    else:
        y0, x0 = dy // 2, dx // 2
    out = {"y0": y0, "x0": x0, "flip": 0, "angle": 0.0, "cos_a": 1.0, "sin_a": 0.0, "brightness": 1.0,
           "contrast": 1.0, "saturation": 1.0, "hue": 0.0}
    if cfg.get("enable_fixed_flip"):
        out["flip"] = 1
    elif cfg.get("enable_random_flip"):
        out["flip"] = int(u[0] < 0.5)

    def span(name, key, ui):
        m = float(cfg.get(key, 0.0) or 0.0)
        if cfg.get(f"enable_fixed_{name}"):
            return m
        if cfg.get(f"enable_random_{name}"):
            return (2.0 * ui - 1.0) * m
        return None
    a = span("rotate", "random_rotate_max_angle", u[1])
    if a:
        out.update(angle=a, cos_a=math.cos(math.radians(a)), sin_a=math.sin(math.radians(a)))
    for k, name in enumerate(("brightness", "contrast", "saturation")):
        s = span(name, f"random_{name}_max_strength", u[2 + k])
        if s is not None:
            out[name] = max(0.0, 1.0 + s)
    s = span("hue", "random_hue_max_strength", u[5])
    if s is not None:
        out["hue"] = 0.5 * s
    return out


# ---- the GPU test's inputs (shared with the CPU test that measures the tolerance) ------------------------------------
def _entry(src_off, out_off, C, Hs, Ws, y0, x0, H, W, flip=0, angle=0.0, b=1.0, c=1.0, s=1.0, h=0.0):
    a = math.radians(angle)
    return {"src_off": src_off, "out_off": out_off, "C": C, "Hs": Hs, "Ws": Ws, "y0": y0, "x0": x0, "H": H, "W": W,
            "flip": flip, "angle": angle, "cos_a": math.cos(a) if angle else 1.0, "sin_a": math.sin(a) if angle else 0.0,
            "brightness": b, "contrast": c, "saturation": s, "hue": h}


def _images(rng, C, H, W):
    """smooth structure + noise in [0, 1], with black, white, gray and saturated patches (the hue stage's edges)"""
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([0.5 + 0.5 * np.sin(0.21 * x + 0.13 * y + c) * np.cos(0.17 * y - 0.05 * x * c) for c in range(C)])
    img = np.clip(0.7 * img + 0.3 * rng.random((C, H, W)), 0.0, 1.0)
    if C == 3 and H >= 16 and W >= 16:
        img[:, 0:4, 0:4] = 0.0
        img[:, 0:4, W - 4:W] = 1.0
        img[:, H - 4:H, 0:4] = 0.5
        img[:, H - 4:H, W - 4:W] = np.array([1.0, 0.0, 0.0])[:, None, None]
        img[:, H // 2:H // 2 + 2, 0:6] = np.array([0.25, 0.25, 0.75])[:, None, None]
    return img.astype(np.float32)


def gpu_cases():
    """{name: (src flat float32, [entries], H, W, out_numel)}: the launches of test_augment_gpu.py.
    "odd": five 37 x 53 entries from 41 x 64 sources -- offsets at 0 and at their maximum (the crop touches every
    source edge), angles 0, +-7.5, 45, one mask; "square": 64 x 64 at 90 degrees; "wide": 256 x 320 at contrast 0
    (the mean spans 32 workgroups); "copy": crop-only and flip-only entries, aligned (vector path) and not."""
    rng = np.random.default_rng(20240607)
    cases = {}
    Hs, Ws, H, W = 41, 64, 37, 53
    srcs = [_images(rng, 3, Hs, Ws) for _ in range(4)] + [_images(rng, 1, Hs, Ws)]
    offs = np.cumsum([0] + [s.size for s in srcs]).tolist()
    n = 3 * H * W
    ents = [_entry(offs[0], 0 * n, 3, Hs, Ws, 0, 0, H, W, flip=1, angle=0.0, b=1.2, c=0.7, s=1.3, h=0.2),
            _entry(offs[1], 1 * n, 3, Hs, Ws, Hs - H, Ws - W, H, W, flip=0, angle=7.5, b=0.8, c=1.4, s=0.5, h=-0.45),
            _entry(offs[2], 2 * n, 3, Hs, Ws, 0, Ws - W, H, W, flip=1, angle=-7.5, s=1.6, h=0.5),
            _entry(offs[3], 3 * n, 3, Hs, Ws, Hs - H, 0, H, W, flip=0, angle=45.0, b=1.1, c=1.25),
            _entry(offs[4], 4 * n, 1, Hs, Ws, 2, 5, H, W, flip=1, angle=7.5)]
    cases["odd"] = (np.concatenate([s.reshape(-1) for s in srcs]), ents, H, W, 4 * n + H * W)
    sq = _images(rng, 3, 64, 64)
    cases["square"] = (sq.reshape(-1), [_entry(0, 0, 3, 64, 64, 0, 0, 64, 64, angle=90.0)], 64, 64, 3 * 64 * 64)
    wide = _images(rng, 3, 260, 328)
    cases["wide"] = (wide.reshape(-1), [_entry(0, 0, 3, 260, 328, 3, 4, 256, 320, c=0.0)], 256, 320, 3 * 256 * 320)
    a = _images(rng, 3, 40, 72)
    m = 3 * 32 * 64
    cases["copy"] = (a.reshape(-1), [_entry(0, 0 * m, 3, 40, 72, 4, 8, 32, 64),            # aligned: vector path
                                     _entry(0, 1 * m, 3, 40, 72, 8, 4, 32, 64, flip=1),
                                     _entry(0, 2 * m, 3, 40, 72, 3, 5, 32, 64),            # x0 off the 16-byte grid
                                     _entry(0, 3 * m, 3, 40, 72, 0, 7, 32, 64, flip=1)], 32, 64, 4 * m)
    return cases


def case_planes(case):
    """[(entry, its source plane [C, Hs, Ws])] of one case"""
    flat, ents = case[0], case[1]
    return [(e, flat[e["src_off"]:e["src_off"] + e["C"] * e["Hs"] * e["Ws"]].reshape(e["C"], e["Hs"], e["Ws"]))
            for e in ents]


def measure_stage_errors():
    """{stage: worst |float32 oracle - float64 oracle| after that stage} over gpu_cases()"""
    worst = dict.fromkeys(STAGES, 0.0)
    for case in gpu_cases().values():
        for e, plane in case_planes(case):
            for s in STAGES:
                lo = augment(plane, e, np.float32, upto=s).astype(np.float64)
                worst[s] = max(worst[s], float(np.abs(lo - augment(plane, e, np.float64, upto=s)).max()))
    return worst
