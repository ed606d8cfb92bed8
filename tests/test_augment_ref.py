"""Training augmentations, CPU side: tests/augment_ref.py (the numpy restatement the GPU tests compare with) against the
live Pillow; the library's host routines (dxa_color_jitter_pixels_host: the very per-pixel code the kernels run;
dxa_resample_coeffs with DXA_FILTER_BILINEAR) against the restatement; PixelAug's draws; argument checks."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from . import augment_ref as R

ORDERS = list(itertools.permutations(range(4)))


def frame(h, w, seed):
    from oracle import image_oracle as IO
    return IO.synthetic_image(h, w, seed)


def all_colours():
    idx = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(idx >> 16) & 255, (idx >> 8) & 255, idx & 255], -1).astype(np.uint8)


def host_jitter(pix, order, factors, hue, m):
    from dexbotic_amd import _lib as L
    q = L.JitterParams()
    q.apply = 1
    for i in range(4):
        q.order[i] = order[i]
    q.brightness, q.contrast, q.saturation, q.hue = factors[0], factors[1], factors[2], hue
    out = np.ascontiguousarray(pix.reshape(-1, 3)).copy()
    L.check(L.lib.dxa_color_jitter_pixels_host(out.ctypes.data_as(C.c_void_p), out.shape[0], C.byref(q), m))
    return out.reshape(pix.shape)


# ------------------------------------------------------------------------------------ the restatement against Pillow
def test_enhancers_match_pillow():
    pytest.importorskip("PIL.Image")
    img = frame(37, 53, 1)
    assert np.array_equal(R.grey(img), R.pil_grey(img))
    for f in (0.0, 0.5, 0.7, 0.83, 1.0, 1.17, 1.3, 1.5):
        assert np.array_equal(R.brightness(img, f), R.pil_enhance(img, R.BRIGHTNESS, f)), f
        assert np.array_equal(R.contrast(img, f), R.pil_enhance(img, R.CONTRAST, f)), f
        assert np.array_equal(R.saturation(img, f), R.pil_enhance(img, R.SATURATION, f)), f


def test_hsv_round_trip_matches_pillow_on_a_colour_sample():
    """every 16th level of each channel plus the extremes both ways (the exhaustive run is the host-function test below)"""
    Image = pytest.importorskip("PIL.Image")
    lv = np.unique(np.r_[0:256:5, 1, 254, 255]).astype(np.uint8)
    img = np.stack(np.meshgrid(lv, lv, lv, indexing="ij"), -1).reshape(lv.size, -1, 3)
    assert np.array_equal(R.rgb_to_hsv(img), np.asarray(Image.fromarray(img, "RGB").convert("HSV")))
    assert np.array_equal(R.hsv_to_rgb(img), np.asarray(Image.fromarray(img, "HSV").convert("RGB")))
    for hue in (0.1, -0.1, 0.08, -0.03, 0.0, 0.5, -0.5):
        assert np.array_equal(R.hue_shift(img, hue), R.pil_hue_shift(img, hue)), hue


def test_crop_resize_matches_pillow():
    pytest.importorskip("PIL.Image")
    img = frame(37, 53, 2)
    big = frame(201, 233, 3)
    cases = [(img, 0, 0, 37, 48), (img, 16, 0, 37, 48), (img, 5, 7, 29, 48), (img, 50, 34, 3, 48), (img, 11, 3, 31, 17),
             (img, 3, 1, 33, 33), (big, 0, 0, 201, 48), (big, 32, 0, 201, 384), (big, 13, 9, 191, 97), (big, 7, 0, 199, 200)]
    for src, x0, y0, c, S in cases:
        assert np.array_equal(R.crop_resize(src, x0, y0, c, S), R.pil_crop_resize(src, x0, y0, c, S)), (x0, y0, c, S)
    sq = R.pad_square(img, (122, 116, 104))
    assert np.array_equal(sq, R.pil_pad_square(img, (122, 116, 104))) and sq.shape == (53, 53, 3)


def test_composed_jitter_matches_pillow_in_all_24_orders():
    pytest.importorskip("PIL.Image")
    img = frame(37, 53, 4)
    rs = np.random.RandomState(0)
    for n, order in enumerate(ORDERS):
        factors = np.float32([rs.uniform(0.7, 1.3), rs.uniform(0.6, 1.4), rs.uniform(0.5, 1.5)])
        hue = np.float32(rs.uniform(-0.1, 0.1))
        assert np.array_equal(R.color_jitter(img, order, factors, hue), R.pil_color_jitter(img, order, factors, hue)), order


def test_contrast_mean_rounds_half_up():
    ImageStat = pytest.importorskip("PIL.ImageStat")
    from PIL import Image
    for n101, want in ((12, 101), (11, 100)):                   # mean L = 100.5 exactly, and 100 + 11/24
        img = np.full((4, 6, 3), 100, np.uint8)
        img.reshape(-1, 3)[:n101] = 101
        assert R.contrast_mean(img) == want
        assert int(ImageStat.Stat(Image.fromarray(img, "RGB").convert("L")).mean[0] + 0.5) == want
        assert np.array_equal(R.contrast(img, 0.0), np.full_like(img, want))
        assert np.array_equal(R.contrast(img, 0.0), R.pil_enhance(img, R.CONTRAST, 0.0))


# --------------------------------------------------------------------------------- the library's host code
def test_host_pixels_match_restatement_on_all_colours():
    """dxa_color_jitter_pixels_host runs the __host__ __device__ header the kernels run.  All 2^24 colours through one
    order with factors either side of 1 and both hue signs; with Pillow present, the hue op alone against Pillow too."""
    pix = all_colours()
    order, factors, m = (2, 3, 0, 1), np.float32([1.17, 0.7, 1.3]), 117
    for hue in (np.float32(-0.1), np.float32(0.08)):
        got = host_jitter(pix, order, factors, hue, m)
        assert np.array_equal(got, R.jitter_pixels(pix, order, factors, hue, m)), hue
    got = host_jitter(pix, (0, 1, 2, 3), np.float32([1, 1, 1]), np.float32(0.1), 0)     # unit factors: the hue op alone
    try:
        import PIL.Image  # noqa: F401
    except ImportError:
        return
    img = pix.reshape(4096, 4096, 3)
    assert np.array_equal(got.reshape(img.shape), R.pil_hue_shift(img, np.float32(0.1)))


def test_host_pixels_match_restatement_in_all_24_orders():
    rs = np.random.RandomState(1)
    pix = np.ascontiguousarray(all_colours()[rs.choice(1 << 24, 4096, replace=False)])
    for order in ORDERS:
        factors = np.float32([rs.uniform(0.0, 1.3), rs.uniform(0.6, 1.4), rs.uniform(0.5, 1.5)])
        hue, m = np.float32(rs.uniform(-0.1, 0.1)), int(rs.randint(0, 256))
        assert np.array_equal(host_jitter(pix, order, factors, hue, m), R.jitter_pixels(pix, order, factors, hue, m)), order


def test_bilinear_tables_match_restatement():
    from dexbotic_amd import _lib as L
    for n_in, n_out in ((37, 48), (53, 48), (3, 48), (64, 48), (48, 48), (373, 384), (728, 728), (1280, 728), (200, 17)):
        ks, bounds, kk = R.bilinear_coeffs(n_in, n_out)
        assert L.lib.dxa_resample_ksize_filter(n_in, n_out, L.FILTER_BILINEAR) == ks
        b = np.zeros((n_out, 2), np.int32)
        k = np.zeros((n_out, ks), np.int32)
        L.check(L.lib.dxa_resample_coeffs(n_in, n_out, L.FILTER_BILINEAR, b.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p)))
        assert np.array_equal(b, bounds) and np.array_equal(k, kk), (n_in, n_out)
    assert L.lib.dxa_resample_ksize_filter(640, 224, L.FILTER_BICUBIC) == L.lib.dxa_resample_ksize(640, 224)
    assert L.lib.dxa_resample_ksize_filter(640, 224, 1) == 0
    assert L.lib.dxa_resample_coeffs(8, 8, 1, b.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p)) != 0
    assert "DXA_FILTER_BILINEAR" in L.last_error()


# ------------------------------------------------------------------------------------------------------ the draws
def test_pixel_aug_sample():
    from dexbotic_amd.data.dataset.augmentations import PixelAug
    a, b = PixelAug("v3", p=0.5, seed=7).sample(64, 200, 200), PixelAug("v3", p=0.5, seed=7).sample(64, 200, 200)
    for name in ("apply_crop", "box", "apply_jitter", "order", "factors", "hue"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert not np.array_equal(a.hue, PixelAug("v3", p=0.5, seed=8).sample(64, 200, 200).hue)
    assert 0 < a.apply_crop.sum() < 64 and 0 < a.apply_jitter.sum() < 64
    x0, y0, c = a.box.T
    assert (c >= 195).all() and (c <= 200).all() and (x0 >= 0).all() and (y0 >= 0).all()
    assert (x0 + c <= 200).all() and (y0 + c <= 200).all() and len(np.unique(c)) > 1
    assert all(sorted(o) == [0, 1, 2, 3] for o in a.order.tolist()) and len({tuple(o) for o in a.order.tolist()}) > 4
    lo, hi = np.float32([0.7, 0.6, 0.5]), np.float32([1.3, 1.4, 1.5])
    assert (a.factors >= lo).all() and (a.factors <= hi).all() and (np.abs(a.hue) <= np.float32(0.08)).all()
    assert a.factors.dtype == np.float32 and a.hue.dtype == np.float32
    rect = PixelAug("v3", p=1.0, seed=1).sample(5, 10, 400)             # sqrt(0.95 * 4000) > 10: always the fallback
    assert rect.apply_crop.all() and (rect.box == (195, 0, 10)).all()
    tall = PixelAug("v3", p=1.0, seed=1).sample(3, 401, 10)
    assert (tall.box == (0, 195, 10)).all()
    col = PixelAug("color_dm0", p=0.0, seed=1).sample(4, 64, 64)
    assert not col.apply_crop.any() and not col.apply_jitter.any() and (col.box == (0, 0, 64)).all()
    ident = PixelAug("identity", seed=5)
    state = ident.rng.bit_generator.state
    par = ident.sample(6, 30, 40)
    assert ident.rng.bit_generator.state == state                       # nothing drawn
    assert not par.apply_crop.any() and not par.apply_jitter.any() and len(par) == 6
    assert len(par.take(np.asarray([1, 4]))) == 2


def test_pixel_aug_names():
    from dexbotic_amd.data.dataset.augmentations import PixelAug
    for name in ("pi0", "dm0", "v1", "v2"):
        with pytest.raises(NotImplementedError, match=name):
            PixelAug(policy=name)
    for name in ("dm0_color", "v4", ""):                                # "dm0_color" is not a key of the reference's table
        with pytest.raises(KeyError):
            PixelAug(policy=name)
    assert (PixelAug("v3").crop_size, PixelAug("color_dm0").resize, PixelAug("color").pads_to_square) == (384, 728, True)


# ------------------------------------------------------------------------------------------------- argument checks
def test_entry_points_reject_bad_arguments_with_a_message():
    from dexbotic_amd import _lib as L
    from dexbotic_amd import kernels as K
    lib, fake = L.lib, 4096                                             # (never dereferenced: the checks come first)
    box = np.asarray([[0, 0, 8, 0]], np.int32)
    sides = np.asarray([8], np.int32)
    bp, sp = box.ctypes.data_as(C.c_void_p), sides.ctypes.data_as(C.c_void_p)
    assert lib.dxa_image_crop_resize(None, 1, 8, 8, 0, 0, fake, bp, 8, fake, fake, sp, 1, 3, fake, 8, fake, None) == -1
    assert "null buffer" in L.last_error()
    assert lib.dxa_image_crop_resize(fake, 1, 8, 8, 0, 0, None, None, 8, fake, fake, sp, 1, 3, fake, 8, fake, None) == -1
    assert "null box table" in L.last_error()
    for bad in ([1, 0, 8, 0], [0, 1, 8, 0], [-1, 0, 8, 0], [0, 0, 9, 0], [0, 0, 0, 0]):
        b = np.asarray([bad], np.int32)
        assert lib.dxa_image_crop_resize(fake, 1, 8, 8, 0, 0, fake, b.ctypes.data_as(C.c_void_p), 8, fake, fake, sp, 1, 3, fake, 8,
                                         fake, None) == -1
        assert "outside the 8x8 frame" in L.last_error(), bad
    wide = np.asarray([[2, 0, 8, 0]], np.int32)                         # a fine box, but 7 scratch rows for 8 box rows
    assert lib.dxa_image_crop_resize(fake, 1, 8, 12, 0, 0, fake, wide.ctypes.data_as(C.c_void_p), 8, fake, fake, sp, 1, 3, fake,
                                     7, fake, None) == -1 and "scratch" in L.last_error()
    tall = np.asarray([[0, 4, 8, 0]], np.int32)
    assert lib.dxa_image_crop_resize(fake, 1, 8, 12, 0, 0, fake, tall.ctypes.data_as(C.c_void_p), 8, fake, fake, sp, 1, 3, fake,
                                     8, fake, None) == -1 and "outside the 8x12 frame" in L.last_error()
    other = np.asarray([[0, 0, 7, 0]], np.int32)
    assert lib.dxa_image_crop_resize(fake, 1, 8, 8, 0, 0, fake, other.ctypes.data_as(C.c_void_p), 8, fake, fake, sp, 1, 3, fake,
                                     8, fake, None) == -1 and "another side" in L.last_error()
    assert lib.dxa_image_crop_resize(fake, 1, 8, 8, 0, 0, fake, bp, 4, fake, fake, sp, 1, 3, fake, 8, fake, None) == -1
    assert "tap stride" in L.last_error()                               # 8 -> 4 needs 5 taps
    q = L.JitterParams()
    q.apply = 1
    for i in range(4):
        q.order[i] = (0, 1, 2, 2)[i]
    q.brightness = q.contrast = q.saturation = 1.0
    assert lib.dxa_color_jitter(None, 1, 8, 8, fake, C.byref(q), fake, None) == -1 and "null buffer" in L.last_error()
    assert lib.dxa_color_jitter(fake, 1, 8, 8, fake, None, fake, None) == -1 and "null parameter table" in L.last_error()
    assert lib.dxa_color_jitter(fake, 1, 8, 8, fake, C.byref(q), fake, None) == -1 and "permutation" in L.last_error()
    px = np.zeros((2, 3), np.uint8)
    assert lib.dxa_color_jitter_pixels_host(px.ctypes.data_as(C.c_void_p), 2, C.byref(q), 0) == -1 and "permutation" in L.last_error()
    q.order[3] = 3
    q.hue = 0.75
    assert lib.dxa_color_jitter_pixels_host(px.ctypes.data_as(C.c_void_p), 2, C.byref(q), 0) == -1 and "hue" in L.last_error()
    q.hue = 0.0
    assert lib.dxa_color_jitter_pixels_host(None, 2, C.byref(q), 0) == -1 and "null buffer" in L.last_error()
    assert lib.dxa_color_jitter_pixels_host(px.ctypes.data_as(C.c_void_p), 2, C.byref(q), 256) == -1 and "mean" in L.last_error()
    assert lib.dxa_color_jitter_pixels_host(px.ctypes.data_as(C.c_void_p), 2, C.byref(q), 7) == 0
    # the Python wrappers refuse what is not a contiguous uint8 [n, h, w, 3] before anything else
    for bad in (torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 8, 4, dtype=torch.uint8), torch.zeros(8, 8, 3, dtype=torch.uint8)):
        with pytest.raises(L.DxaError, match="uint8"):
            K.image_crop_resize(bad, [[0, 0, 8]], 8)
        with pytest.raises(L.DxaError, match="uint8"):
            K.image_color_jitter(bad, [1], [[0, 1, 2, 3]], [[1, 1, 1]], [0.0])
