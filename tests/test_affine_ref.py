"""The affine warp and the DeviceAug compositions, CPU side: tests/affine_ref.py (the numpy restatement the GPU tests compare
with) against the live Pillow; dxa_image_affine_host (the very per-pixel code the kernel runs) against the restatement;
AugSpec / DeviceAug names, validation and draws; argument checks of both entry points.  Every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

from . import affine_ref as A

ROT_SIZES = ((7, 7), (16, 16), (33, 33), (20, 31))
GEN_SIZES = ((9, 9), (33, 48), (64, 64))


def frames_for(h, w, seed):
    """one frame of random bytes and one synthetic camera frame"""
    from oracle import image_oracle as IO
    return (np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8), IO.synthetic_image(h, w, seed))


def cases():
    """(label, frame, inverse matrix, fill) of every case the restatement was compared with Pillow on"""
    for h, w in ROT_SIZES:
        for k, img in enumerate(frames_for(h, w, 3 * h + w)):
            for angle in A.ANGLES + ((90,) if h == w else ()):
                yield f"{h}x{w} frame {k} at {angle} deg", img, A.rotate_matrix(angle, h, w), (0, 0, 0)
    for h, w in GEN_SIZES:
        for k, img in enumerate(frames_for(h, w, 5 * h + w)):
            for name, m in A.GENERAL.items():
                yield f"{h}x{w} frame {k}, {name}", img, m, A.FILL


def host_affine(frames, mats, fill=(0, 0, 0)):
    from dexbotic_amd import _lib as L
    frames = np.ascontiguousarray(frames)
    n, h, w, _ = frames.shape
    mats = np.ascontiguousarray(np.asarray(mats, np.float64).reshape(n, 6))
    out = np.full_like(frames, 77)
    L.check(L.lib.dxa_image_affine_host(frames.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), n, h, w,
                                        mats.ctypes.data_as(C.c_void_p), fill[0] | (fill[1] << 8) | (fill[2] << 16)))
    return out


# ------------------------------------------------------------------------------------ the restatement against Pillow
def test_restatement_matches_pillow():
    pytest.importorskip("PIL.Image")
    count = 0
    for label, img, m, fill in cases():
        assert np.array_equal(A.affine(img, m, fill), A.pil_affine(img, m, fill)), label
        count += 1
    assert count == 2 * (4 * 7 + 3 + 3 * 4)


def test_rotate_matches_pillow_rotate():
    """Image.rotate itself: the matrix (angle mod 360, 15 places, the centre) and the transposes it takes at 0 and 90 degrees"""
    pytest.importorskip("PIL.Image")
    from dexbotic_amd import kernels as K
    for h, w in ROT_SIZES:
        img = frames_for(h, w, h + w)[0]
        for angle in A.ANGLES + ((90,) if h == w else ()) + (355.0, 725.5):
            assert np.array_equal(A.rotate(img, angle), A.pil_rotate(img, angle)), (h, w, angle)
            assert K.rotate_matrix(angle, h, w) == A.rotate_matrix(angle, h, w)
    assert not np.array_equal(A.rotate(img, 3.0), A.rotate(img, -3.0))


# ------------------------------------------------------------------------------ the host routine against the restatement
def test_host_function_matches_restatement():
    for label, img, m, fill in cases():
        assert np.array_equal(host_affine(img[None], m, fill)[0], A.affine(img, m, fill)), label


def test_host_function_edge_shapes():
    one = np.asarray([[[[9, 200, 31]]]], np.uint8)                                      # 1 x 1: every in-range position is that pixel
    assert np.array_equal(host_affine(one, A.rotate_matrix(3.3, 1, 1))[0], A.affine(one[0], A.rotate_matrix(3.3, 1, 1)))
    assert np.array_equal(host_affine(one, (1, 0, 0, 0, 1, 0)), one)
    col = frames_for(13, 1, 4)[0]                                                       # w = 1: x0 = x1 = 0
    for m in (A.rotate_matrix(-5, 13, 1), A.GENERAL["half-pixel shift"], (1.0, 0.0, 0.0, 0.0, 0.7, 0.2)):
        assert np.array_equal(host_affine(col[None], m, A.FILL)[0], A.affine(col, m, A.FILL))
    img = frames_for(12, 10, 5)[1]
    away = (1.0, 0.0, 100.0, 0.0, 1.0, 0.0)                                             # every source position is outside
    got = host_affine(img[None], away, A.FILL)[0]
    assert (got == np.asarray(A.FILL, np.uint8)).all() and np.array_equal(got, A.affine(img, away, A.FILL))
    big = frames_for(224, 224, 6)[1]
    assert np.array_equal(host_affine(big[None], A.rotate_matrix(3.3, 224, 224))[0], A.rotate(big, 3.3))
    pair = np.stack(frames_for(20, 31, 7))                                              # each frame its own matrix
    mats = [A.rotate_matrix(-5, 20, 31), A.GENERAL["shear"]]
    got = host_affine(pair, mats, A.FILL)
    assert all(np.array_equal(got[i], A.affine(pair[i], mats[i], A.FILL)) for i in range(2))
    from dexbotic_amd import _lib as L
    assert L.lib.dxa_image_affine_host(None, None, 0, 8, 8, None, 0) == 0               # n = 0: nothing to do, nothing read


# ------------------------------------------------------------------------------------------------- argument checks
def test_affine_entry_points_reject_bad_arguments_with_a_message():
    from dexbotic_amd import _lib as L
    lib, fake, other = L.lib, 4096, 1 << 20                             # (never dereferenced: the checks come first)
    eye = np.asarray([[1, 0, 0, 0, 1, 0]], np.float64)
    mp = eye.ctypes.data_as(C.c_void_p)
    assert lib.dxa_image_affine(fake, other, 0, 8, 8, None, None, 0, None) == 0
    assert lib.dxa_image_affine(fake, other, 1, 0, 8, fake, mp, 0, None) == -1 and "bad frame size" in L.last_error()
    assert lib.dxa_image_affine(fake, other, -1, 8, 8, fake, mp, 0, None) == -1 and "bad frame size" in L.last_error()
    assert lib.dxa_image_affine(None, other, 1, 8, 8, fake, mp, 0, None) == -1 and "null buffer" in L.last_error()
    assert lib.dxa_image_affine(fake, None, 1, 8, 8, fake, mp, 0, None) == -1 and "null buffer" in L.last_error()
    assert lib.dxa_image_affine(fake, other, 1, 8, 8, None, mp, 0, None) == -1 and "null matrix table" in L.last_error()
    assert lib.dxa_image_affine(fake, other, 1, 8, 8, fake, None, 0, None) == -1 and "null matrix table" in L.last_error()
    assert lib.dxa_image_affine(fake, fake, 1, 8, 8, fake, mp, 0, None) == -1 and "out of place" in L.last_error()
    assert lib.dxa_image_affine(fake, fake + 100, 1, 8, 8, fake, mp, 0, None) == -1 and "overlap" in L.last_error()
    assert lib.dxa_image_affine(fake, other, 65536, 1, 1, fake, mp, 0, None) == -1 and "too many frames" in L.last_error()
    for bad in (np.nan, np.inf, -np.inf):
        mats = np.tile(eye, (3, 1))
        mats[2, 4] = bad
        assert lib.dxa_image_affine(fake, other, 3, 8, 8, fake, mats.ctypes.data_as(C.c_void_p), 0, None) == -1
        assert "frame 2: matrix is not finite" in L.last_error()
    src = np.zeros((1, 8, 8, 3), np.uint8)
    dst = np.zeros_like(src)
    sp, dp = src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p)
    assert lib.dxa_image_affine_host(sp, dp, 1, 8, 0, mp, 0) == -1 and "bad frame size" in L.last_error()
    assert lib.dxa_image_affine_host(None, dp, 1, 8, 8, mp, 0) == -1 and "null buffer" in L.last_error()
    assert lib.dxa_image_affine_host(sp, dp, 1, 8, 8, None, 0) == -1 and "null matrix table" in L.last_error()
    assert lib.dxa_image_affine_host(sp, sp, 1, 8, 8, mp, 0) == -1 and "out of place" in L.last_error()
    nan = np.asarray([[1, 0, np.nan, 0, 1, 0]], np.float64)
    assert lib.dxa_image_affine_host(sp, dp, 1, 8, 8, nan.ctypes.data_as(C.c_void_p), 0) == -1 and "not finite" in L.last_error()
    assert lib.dxa_image_affine_host(sp, dp, 1, 8, 8, mp, 0) == 0


# ------------------------------------------------------------------------------------------------ names and specs
def test_aug_spec_names():
    from dexbotic_amd.data.dataset.augmentations import AugSpec, DeviceAug
    jit = (0.3, 0.4, 0.5)
    assert AugSpec.of("v3") == AugSpec(crop_size=384, crop_scale=(0.95, 1.0), jitter=jit + (0.08,))
    assert AugSpec.of("color") == AugSpec(pad_to_square=True, jitter=jit + (0.1,))
    assert AugSpec.of("color_dm0") == AugSpec(pad_to_square=True, resize=728, jitter=jit + (0.1,))
    assert AugSpec.of("identity") == AugSpec() and AugSpec().identity and not AugSpec.of("color").identity
    for name, side in (("pi0", 224), ("dm0", 728)):
        assert AugSpec.of(name) == AugSpec(pad_to_square=True, crop_size=side, crop_scale=(0.95, 0.95), crop_p=1.0,
                                           rotate_limit=(-5, 5), rotate_p=1.0, jitter=jit + (0.1,), jitter_p=None)
    for name in ("v1", "v2"):
        with pytest.raises(NotImplementedError, match=name):
            AugSpec.of(name)
        with pytest.raises(NotImplementedError, match=name):
            DeviceAug(name)
    for name in ("dm0_color", "v4", ""):
        with pytest.raises(KeyError):
            AugSpec.of(name)
        with pytest.raises(KeyError):
            DeviceAug(name)
    d = DeviceAug("dm0", p=0.25)
    assert (d.crop_size, d.resize, d.pads_to_square, d.identity) == (728, None, True, False)
    assert (d.crop_p, d.rotate_p, d.jitter_p) == (1.0, 1.0, 0.25)                 # an omitted probability is the policy's p
    assert DeviceAug("identity").identity and DeviceAug(AugSpec(rotate_limit=(-10, 10))).rotate_p == 0.5
    with pytest.raises(TypeError):
        DeviceAug(3)


def test_pixel_aug_points_to_device_aug_for_the_rotating_policies():
    from dexbotic_amd.data.dataset.augmentations import PixelAug
    for name in ("pi0", "dm0"):
        with pytest.raises(NotImplementedError, match=f"{name}.*DeviceAug"):
            PixelAug(name)


def test_aug_spec_validation():
    from dexbotic_amd.data.dataset.augmentations import AugSpec
    with pytest.raises(ValueError, match="at most one of crop_size and resize"):
        AugSpec(crop_size=224, resize=728)
    for bad in (dict(crop_size=0), dict(resize=-1), dict(crop_size=8, crop_scale=(1.0, 0.9)), dict(crop_size=8, crop_scale=(0.0, 1.0)),
                dict(rotate_limit=(5, -5)), dict(rotate_limit=(0, float("nan"))), dict(jitter=(0.3, 0.4, 0.5)),
                dict(jitter=(0.3, 0.4, 0.5, 0.6)), dict(jitter=(-0.1, 0.4, 0.5, 0.1)), dict(rotate_limit=(-5, 5), rotate_p=1.5),
                dict(crop_size=8, crop_p=-0.1), dict(jitter=(0.3, 0.4, 0.5, 0.1), jitter_p=2)):
        with pytest.raises(ValueError):
            AugSpec(**bad)


# ------------------------------------------------------------------------------------------------------ the draws
NAMES6 = ("apply_crop", "box", "apply_jitter", "order", "factors", "hue")


def test_device_aug_draws_what_pixel_aug_draws():
    from dexbotic_amd.data.dataset.augmentations import DeviceAug, PixelAug
    for name in ("v3", "color", "color_dm0", "identity"):
        for p, seed in ((0.5, 7), (1.0, 2), (0.0, 3)):
            a, b = DeviceAug(name, p=p, seed=seed).sample(32, 200, 200), PixelAug(name, p=p, seed=seed).sample(32, 200, 200)
            for col in NAMES6:
                assert np.array_equal(getattr(a, col), getattr(b, col)) and getattr(a, col).dtype == getattr(b, col).dtype, (name, col)
            assert not a.apply_rotate.any() and not a.angle.any()
    rect = DeviceAug("v3", p=1.0, seed=1).sample(5, 10, 400)             # the fallback box, as PixelAug
    assert (rect.box == (195, 0, 10)).all()


def test_device_aug_sample():
    from dexbotic_amd.data.dataset.augmentations import AugSpec, DeviceAug
    a, b = DeviceAug("pi0", p=0.5, seed=7).sample(64, 200, 200), DeviceAug("pi0", p=0.5, seed=7).sample(64, 200, 200)
    for col in NAMES6 + ("apply_rotate", "angle"):
        assert np.array_equal(getattr(a, col), getattr(b, col)), col
    other = DeviceAug("pi0", p=0.5, seed=8).sample(64, 200, 200)
    assert not np.array_equal(a.angle, other.angle)
    assert a.apply_rotate.dtype == np.int32 and a.angle.dtype == np.float64
    assert a.apply_crop.all() and a.apply_rotate.all() and 0 < a.apply_jitter.sum() < 64
    assert (np.abs(a.angle) <= 5).all() and a.angle.min() < -2 and a.angle.max() > 2 and len(np.unique(a.angle)) == 64
    assert (a.box[:, 2] == 195).all()                                    # round(sqrt(0.95) * 200)
    z = DeviceAug("pi0", p=0.0, seed=3).sample(40, 160, 160)            # crop and rotate have p = 1 of their own
    assert z.apply_crop.all() and z.apply_rotate.all() and not z.apply_jitter.any() and (np.abs(z.angle) <= 5).all()
    assert (DeviceAug("dm0", p=0.0, seed=3).sample(40, 160, 160).angle == z.angle).all()   # the same blocks in the same order
    sub = a.take(np.asarray([1, 4]))
    assert len(sub) == 2 and np.array_equal(sub.angle, a.angle[[1, 4]]) and np.array_equal(sub.apply_rotate, a.apply_rotate[[1, 4]])
    # a custom composition: only a rotation, wider than the reference's, on half of the frames
    c = DeviceAug(AugSpec(rotate_limit=(-10, 10), rotate_p=0.5), seed=11).sample(64, 30, 40)
    assert 0 < c.apply_rotate.sum() < 64 and (np.abs(c.angle) <= 10).all() and np.abs(c.angle).max() > 5
    assert not c.apply_crop.any() and not c.apply_jitter.any() and (c.box == (0, 0, 30)).all()
    ident = DeviceAug("identity", seed=5)
    state = ident.rng.bit_generator.state
    ident.sample(6, 30, 40)
    assert ident.rng.bit_generator.state == state                       # nothing drawn


def test_for_cameras():
    from dexbotic_amd.data.dataset.augmentations import AugSpec, DeviceAug
    cams = DeviceAug.for_cameras(["pi0", "color", "color"], 3, p=0.5, seed=4)
    assert [c.policy for c in cams] == ["pi0", "color", "color"] and all(c.p == 0.5 for c in cams)
    h1, h2 = cams[1].sample(8, 64, 64).hue, cams[2].sample(8, 64, 64).hue
    assert not np.array_equal(h1, h2)                                    # the same policy, generators of their own
    again = DeviceAug.for_cameras(["pi0", "color", "color"], 3, p=0.5, seed=4)
    assert np.array_equal(again[1].sample(8, 64, 64).hue, h1) and np.array_equal(again[2].sample(8, 64, 64).hue, h2)
    assert not np.array_equal(DeviceAug.for_cameras(["pi0", "color", "color"], 3, seed=5)[1].sample(8, 64, 64).hue, h1)
    same = DeviceAug.for_cameras("dm0", 2, p=0.3, seed=1)
    assert len(same) == 2 and all(c.policy == "dm0" and c.crop_size == 728 and c.p == 0.3 for c in same)
    assert not np.array_equal(same[0].sample(4, 800, 800).angle, same[1].sample(4, 800, 800).angle)
    assert DeviceAug.for_cameras("", 2) == [None, None]
    mixed = DeviceAug.for_cameras(["pi0", None, "", AugSpec(rotate_limit=(-10, 10))], 4, seed=0)
    assert mixed[1] is None and mixed[2] is None and mixed[0].policy == "pi0" and mixed[3].spec.rotate_limit == (-10, 10)
    with pytest.raises(AssertionError, match="The length of aug_policy 2 must be equal to num_images 3"):
        DeviceAug.for_cameras(["pi0", "color"], 3)
    for bad in (None, ("pi0", "color"), 3):
        with pytest.raises(ValueError, match="must be str or list"):
            DeviceAug.for_cameras(bad, 2)
    with pytest.raises(KeyError):
        DeviceAug.for_cameras(["pi0", "dm0_color"], 2)
