"""Numpy restatement (TEST INFRASTRUCTURE, not product code) of the training augmentations the device path implements:
crop + bilinear resize and colour jitter, as Pillow 12.2.0 computes them.

What it restates
----------------
    PIL.ImageEnhance.Brightness / Contrast / Color      blend(degenerate, image, factor), src/libImaging/Blend.c
    Image.convert('L')                                  L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16
    Image.convert('HSV') / convert('RGB') of HSV        src/libImaging/Convert.c rgb2hsv_row / hsv2rgb_row
    Image.crop(box).resize((S, S), BILINEAR)            src/libImaging/Resample.c, triangle filter, support 1.0
The jitter is the sequence torchvision's PIL backend runs (adjust_brightness / _contrast / _saturation / _hue), which
albumentations' ColorJitter is documented to follow.  tests/test_augment_ref.py pins every function here to the live
Pillow; tests/test_augment_gpu.py pins the kernels to this file bit for bit.

Per-frame jitter parameters: `order` is a permutation of (BRIGHTNESS, CONTRAST, SATURATION, HUE), `factors` the three
blend factors (float32), `hue` the shift in turns (float32)."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
F32 = np.float32


# ------------------------------------------------------------------------------------------------------------ colour
def grey(img):
    """convert('L') of uint8 [..., 3] -> uint8 [...]"""
    x = img.astype(np.int64)
    return ((19595 * x[..., 0] + 38470 * x[..., 1] + 7471 * x[..., 2] + 0x8000) >> 16).astype(np.uint8)


def blend(deg, img, f):
    """Image.blend(deg, img, f): deg + f * (img - deg) in float32; truncated for 0 <= f <= 1, clipped first otherwise"""
    f = F32(f)
    d = np.asarray(deg).astype(F32)
    t = d + f * (img.astype(F32) - d)            # two float32 roundings: product, then sum
    if 0.0 <= f <= 1.0:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def contrast_mean(img):
    """int(mean(L) + 0.5) in integers: (2 sum + N) // (2 N)"""
    L = grey(img).astype(np.int64)
    return int((2 * int(L.sum()) + L.size) // (2 * L.size))


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def contrast(img, f, m=None):
    m = contrast_mean(img) if m is None else m
    return blend(np.full_like(img, m), img, f)


def saturation(img, f):
    return blend(np.repeat(grey(img)[..., None], 3, -1), img, f)


def rgb_to_hsv(img):
    """Convert.c rgb2hsv_row: float32 ratios, the sums and the fmod in double, the result stored as float32"""
    r, g, b = (img[..., i].astype(np.int32) for i in range(3))
    mx = np.maximum(r, np.maximum(g, b))
    mn = np.minimum(r, np.minimum(g, b))
    flat = mx == mn
    cr = np.where(flat, 1, mx - mn).astype(F32)
    s = cr / np.where(flat, 1, mx).astype(F32)
    rc = ((mx - r).astype(F32) / cr).astype(np.float64)
    gc = ((mx - g).astype(F32) / cr).astype(np.float64)
    bc = ((mx - b).astype(F32) / cr).astype(np.float64)
    h = np.where(r == mx, bc - gc, np.where(g == mx, 2.0 + rc - bc, 4.0 + gc - rc))
    h = _h_to_level(h)
    sv = (s.astype(np.float64) * 255.0).astype(np.int32)
    out = np.stack([np.where(flat, 0, h), np.where(flat, 0, sv), mx], -1)
    return out.astype(np.uint8)


def _h_to_level(h):
    h = h.astype(F32).astype(np.float64)
    x = np.fmod(h / 6.0 + 1.0, 1.0).astype(F32)
    return (x.astype(np.float64) * 255.0).astype(np.int32)


def hsv_to_rgb(hsv):
    """Convert.c hsv2rgb_row, all in float32"""
    h, s, v = (hsv[..., i] for i in range(3))
    vf = v.astype(F32)
    fs = s.astype(F32) / F32(255.0)
    f0 = h.astype(F32) * F32(6.0) / F32(255.0)
    i = np.floor(f0)
    f = f0 - i

    def rnd(x):
        return np.clip(np.floor(x + F32(0.5)), 0, 255).astype(np.uint8)

    one = F32(1.0)
    p = rnd(vf * (one - fs))
    q = rnd(vf * (one - fs * f))
    t = rnd(vf * (one - fs * (one - f)))
    sel = i.astype(np.int32) % 6
    table = ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))
    out = np.empty(hsv.shape, np.uint8)
    for c in range(3):
        out[..., c] = np.select([sel == k for k in range(6)], [table[k][c] for k in range(6)])
        out[..., c] = np.where(s == 0, v, out[..., c])
    return out


def hue_levels(hue):
    """trunc(hue * 255) in float32"""
    return int(F32(hue) * F32(255.0))


def hue_shift(img, hue):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + hue_levels(hue)) % 256).astype(np.uint8)
    return hsv_to_rgb(hsv)


def color_jitter(img, order, factors, hue):
    """the four ops in `order` on one frame; contrast takes the mean L of the frame as it is when its turn comes"""
    for op in order:
        if op == BRIGHTNESS:
            img = brightness(img, factors[0])
        elif op == CONTRAST:
            img = contrast(img, factors[1])
        elif op == SATURATION:
            img = saturation(img, factors[2])
        elif op == HUE:
            img = hue_shift(img, hue)
        else:
            raise ValueError(op)
    return img


def jitter_pixels(pix, order, factors, hue, m):
    """the four ops on loose pixels [k, 3] with a given contrast mean (what dxa_color_jitter_pixels_host computes)"""
    for op in order:
        if op == BRIGHTNESS:
            pix = brightness(pix, factors[0])
        elif op == CONTRAST:
            pix = contrast(pix, factors[1], m)
        elif op == SATURATION:
            pix = saturation(pix, factors[2])
        else:
            pix = hue_shift(pix, hue)
    return pix


# ------------------------------------------------------------------------------------------------------ crop / resize
def bilinear_coeffs(in_size, out_size):
    """Resample.c precompute_coeffs + normalize_coeffs_8bpc with the triangle filter (support 1.0) over the full box.
    Returns ksize, bounds [out, 2] (first index, count), taps [out, ksize] int32."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = []
        for x in range(xmax):
            a = abs((x + xmin - center + 0.5) * ss)
            w.append(1.0 - a if a < 1.0 else 0.0)
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            f = v * (1 << PRECISION_BITS)
            kk[xx, x] = int(-0.5 + f) if v < 0 else int(0.5 + f)
        bounds[xx] = (xmin, xmax)
    return ksize, bounds, kk


def _resample_axis(img, out_size, axis):
    img = np.moveaxis(img, axis, 0)
    _, bounds, kk = bilinear_coeffs(img.shape[0], out_size)
    out = np.empty((out_size,) + img.shape[1:], np.uint8)
    src = img.astype(np.int64)
    for xx in range(out_size):
        xmin, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = np.full(img.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        acc += np.tensordot(kk[xx, :n].astype(np.int64), src[xmin:xmin + n], axes=(0, 0))
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_bilinear(img, out_h, out_w):
    """Image.resize((out_w, out_h), BILINEAR): horizontal pass, then vertical; an unchanged axis is skipped"""
    h, w = img.shape[:2]
    if w != out_w:
        img = _resample_axis(img, out_w, 1)
    if h != out_h:
        img = _resample_axis(img, out_h, 0)
    return img


def crop_resize(img, x0, y0, c, S):
    """crop((x0, y0, x0 + c, y0 + c)) then resize((S, S), BILINEAR): the taps never read outside the box"""
    return resize_bilinear(np.ascontiguousarray(img[y0:y0 + c, x0:x0 + c]), S, S)


def pad_square(img, fill):
    """expand2square / PadToSquare on a uint8 HWC array: centred, (side - size) // 2 before"""
    h, w = img.shape[:2]
    if h == w:
        return img
    p = max(h, w)
    out = np.empty((p, p, 3), np.uint8)
    out[:] = np.asarray(fill, np.uint8)
    y0, x0 = (p - h) // 2, (p - w) // 2
    out[y0:y0 + h, x0:x0 + w] = img
    return out


# ---------------------------------------------------------------------------------------------------- Pillow helpers
def pil_grey(img):
    from PIL import Image
    return np.asarray(Image.fromarray(img, "RGB").convert("L"))


def pil_enhance(img, op, f):
    from PIL import Image, ImageEnhance
    cls = {BRIGHTNESS: ImageEnhance.Brightness, CONTRAST: ImageEnhance.Contrast, SATURATION: ImageEnhance.Color}[op]
    return np.asarray(cls(Image.fromarray(img, "RGB")).enhance(float(F32(f))))


def pil_hue_shift(img, hue):
    """torchvision's PIL adjust_hue: the H plane of convert('HSV') shifted with uint8 wrap-around, back to RGB"""
    from PIL import Image
    hsv = np.asarray(Image.fromarray(img, "RGB").convert("HSV")).copy()
    hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + hue_levels(hue)) % 256).astype(np.uint8)
    return np.asarray(Image.fromarray(hsv, "HSV").convert("RGB"))


def pil_color_jitter(img, order, factors, hue):
    for op in order:
        img = pil_hue_shift(img, hue) if op == HUE else pil_enhance(img, op, factors[op])
    return img


def pil_crop_resize(img, x0, y0, c, S):
    from PIL import Image
    return np.asarray(Image.fromarray(img, "RGB").crop((x0, y0, x0 + c, y0 + c)).resize((S, S), Image.BILINEAR))


def pil_pad_square(img, fill):
    from PIL import Image
    h, w = img.shape[:2]
    if h == w:
        return img
    p = max(h, w)
    sq = Image.new("RGB", (p, p), tuple(int(v) for v in fill))
    sq.paste(Image.fromarray(img, "RGB"), ((p - w) // 2, (p - h) // 2))
    return np.asarray(sq)
