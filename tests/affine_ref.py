"""Numpy restatement (TEST INFRASTRUCTURE, not product code) of the bilinear affine warp the device path implements, as
Pillow 12.2.0 computes it.

What it restates
----------------
    Image.transform(size, AFFINE, m, BILINEAR, fillcolor)   src/libImaging/Geometry.c affine_transform +
                                                            bilinear_filter32RGB (BILINEAR_HEAD / BILINEAR_BODY)
    Image.rotate(angle, BILINEAR)                           PIL/Image.py: the matrix it hands to transform()
Everything is float64 and every numpy operation rounds once, as the C code does (Pillow is built without fused
multiply-add).  tests/test_affine_ref.py pins both functions to the live Pillow and dxa_image_affine_host to them;
tests/test_affine_gpu.py pins the kernel to this file bit for bit."""
import math

import numpy as np

# the cases both test files run
ANGLES = (-5, -3.217, -0.01, 0, 0.4, 4.99999, 5)
GENERAL = {                                                   # inverse matrices: output pixel -> source position
    "shear": (1.0, 0.25, -1.5, -0.1, 1.0, 0.75),
    "zoom 2x": (0.5, 0.0, 0.0, 0.0, 0.5, 0.0),
    "shrink 0.5x": (2.0, 0.0, 0.0, 0.0, 2.0, 0.0),
    "half-pixel shift": (1.0, 0.0, 0.5, 0.0, 1.0, 0.5),
}
FILL = (122, 116, 104)                                        # int(CLIP mean * 255)


def rotate_matrix(angle, h, w):
    """the inverse matrix Image.rotate(angle) of a w x h image passes to transform(): 6 Python floats"""
    angle = angle % 360.0
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = w / 2, h / 2
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def affine(img, m, fill=(0, 0, 0)):
    """uint8 [h, w, 3] -> the same shape: output pixel (x, y) reads the source at m applied to (x + 0.5, y + 0.5)"""
    h, w = img.shape[:2]
    m = [np.float64(v) for v in m]
    xc = (np.arange(w, dtype=np.float64) + 0.5)[None, :]
    yc = (np.arange(h, dtype=np.float64) + 0.5)[:, None]
    with np.errstate(invalid="ignore"):
        xin = (m[0] * xc + m[1] * yc) + m[2]
        yin = (m[3] * xc + m[4] * yc) + m[5]
        inside = (xin >= 0.0) & (xin < w) & (yin >= 0.0) & (yin < h)
    xin = np.where(inside, xin, 0.5) - 0.5
    yin = np.where(inside, yin, 0.5) - 0.5
    xf, yf = np.floor(xin), np.floor(yin)
    dx, dy = (xin - xf)[..., None], (yin - yf)[..., None]
    xi, yi = xf.astype(np.int64), yf.astype(np.int64)
    x0, x1 = np.clip(xi, 0, w - 1), np.clip(xi + 1, 0, w - 1)
    src = img.astype(np.float64)

    def row(y):
        a, b = src[y, x0], src[y, x1]
        return a + (b - a) * dx

    v1 = row(np.clip(yi, 0, h - 1))
    below = ((yi + 1 >= 0) & (yi + 1 < h))[..., None]
    v2 = np.where(below, row(np.clip(yi + 1, 0, h - 1)), v1)
    v = v1 + (v2 - v1) * dy
    out = v.astype(np.int32).astype(np.uint8)                 # (UINT8)v: truncation
    return np.where(inside[..., None], out, np.asarray(fill, np.uint8)).astype(np.uint8)


def rotate(img, angle, fill=(0, 0, 0)):
    return affine(img, rotate_matrix(angle, *img.shape[:2]), fill)


# ---------------------------------------------------------------------------------------------------- Pillow helpers
def pil_affine(img, m, fill=(0, 0, 0)):
    from PIL import Image
    h, w = img.shape[:2]
    out = Image.fromarray(img, "RGB").transform((w, h), Image.AFFINE, tuple(float(v) for v in m), resample=Image.BILINEAR,
                                                fillcolor=tuple(int(v) for v in fill))
    return np.asarray(out)


def pil_rotate(img, angle, fill=(0, 0, 0)):
    from PIL import Image
    return np.asarray(Image.fromarray(img, "RGB").rotate(angle, resample=Image.BILINEAR, fillcolor=tuple(int(v) for v in fill)))
