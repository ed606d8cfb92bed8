"""The affine warp on the GPU: dxa_image_affine (through dexbotic_amd.kernels) and the DeviceAug route of PreprocessRGB against
tests/affine_ref.py and tests/augment_ref.py, which tests/test_affine_ref.py and tests/test_augment_ref.py pin to Pillow.
Every comparison is bit for bit."""
import numpy as np
import pytest
import torch

from . import affine_ref as A
from . import augment_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BG = (122, 116, 104)                                          # int(CLIP mean * 255)
NAMES6 = ("apply_crop", "box", "apply_jitter", "order", "factors", "hue")


def frames_of(n, h, w, seed):
    from oracle import image_oracle as IO
    return np.stack([IO.synthetic_image(h, w, seed + i) for i in range(n)])


def affine_dev(frames, mats, fill):
    from dexbotic_amd import kernels as K
    t = torch.from_numpy(frames).to(DEV)
    keep = t.clone()
    out = K.image_affine(t, mats, fill)
    assert out.shape == t.shape and out.dtype == torch.uint8 and out.data_ptr() != t.data_ptr()
    assert torch.equal(t, keep)                               # out of place: the source is as it was
    return out.cpu().numpy()


# 33 x 33: 3267 bytes a frame, so frame 0 takes the dword path across row ends and frames 1, 2 start off a dword (byte path);
# 48 x 48: every frame on the dword path; 20 x 31: rectangular, 3 * w no multiple of 4 but the frames are (dword path).
# 1024 pixels to a workgroup: 33 x 33 and 48 x 48 take more than one, the last one partly filled.
@pytest.mark.parametrize("h,w", [(33, 33), (48, 48), (20, 31)])
def test_affine_matches_restatement(h, w):
    frames = frames_of(3, h, w, 10 * h + w)
    rot = [A.rotate_matrix(a, h, w) for a in (-5, 0, 3.217)]
    sets = [rot] + [[m, rot[0], A.GENERAL["half-pixel shift"]] for m in A.GENERAL.values()]
    for mats in sets:
        got = affine_dev(frames, mats, A.FILL)
        for i in range(3):
            assert np.array_equal(got[i], A.affine(frames[i], mats[i], A.FILL)), (mats[i], i)


def test_affine_odd_tail_and_empty_batch():
    from dexbotic_amd import kernels as K
    frames = frames_of(2, 7, 5, 3)                            # 35 pixels: a lane with three pixels left on either path
    mats = [A.rotate_matrix(4.99999, 7, 5), A.GENERAL["shear"]]
    got = affine_dev(frames, mats, A.FILL)
    assert all(np.array_equal(got[i], A.affine(frames[i], mats[i], A.FILL)) for i in range(2))
    empty = K.image_affine(torch.empty(0, 8, 8, 3, dtype=torch.uint8, device=DEV), np.zeros((0, 6)))
    assert empty.shape == (0, 8, 8, 3)
    assert K.image_rotate(torch.empty(0, 8, 8, 3, dtype=torch.uint8, device=DEV), []).shape == (0, 8, 8, 3)
    with pytest.raises(Exception, match="2 frames but 1 matrices"):
        K.image_affine(torch.from_numpy(frames).to(DEV), np.zeros((1, 6)))
    with pytest.raises(Exception, match="not finite"):
        K.image_affine(torch.from_numpy(frames).to(DEV), np.full((2, 6), np.nan))


def test_rotate_one_224_frame():
    from dexbotic_amd import kernels as K
    frame = frames_of(1, 224, 224, 77)
    t = torch.from_numpy(frame).to(DEV)
    assert np.array_equal(K.image_rotate(t, [3.3])[0].cpu().numpy(), A.rotate(frame[0], 3.3))
    assert np.array_equal(K.image_rotate(t, [-725.5], fill=BG)[0].cpu().numpy(), A.rotate(frame[0], -725.5, BG))


# -------------------------------------------------------------------------------------------------------- end to end
def processor(aug=None, aspect="pad"):
    from dexbotic_amd.data.dataset.rgb_preprocess import ImageProcessorSpec, PreprocessRGB
    return PreprocessRGB(ImageProcessorSpec(), image_aspect_ratio=aspect, augmentations=aug, device=DEV)


def augment_ref_frame(frame, spec, aspect, par, i):
    """what the composition does to one frame, with row i of the drawn table: uint8 HWC"""
    if aspect == "pad":
        frame = R.pad_square(frame, BG)
    if spec.pad_to_square:
        frame = R.pad_square(frame, (0, 0, 0))
    if par.apply_crop[i]:
        frame = R.crop_resize(frame, *par.box[i], spec.crop_size)
    elif spec.resize is not None:
        frame = R.resize_bilinear(frame, spec.resize, spec.resize)
    if par.apply_rotate[i]:
        frame = A.rotate(frame, float(par.angle[i]))          # albumentations' Rotate fills with 0
    if par.apply_jitter[i]:
        frame = R.color_jitter(frame, par.order[i], par.factors[i], par.hue[i])
    return frame


def check_against_ref(spec, aspect, frames, p, seed):
    from dexbotic_amd.data.dataset.augmentations import DeviceAug
    from oracle import image_oracle as IO
    pre = processor(DeviceAug(spec, p=p, seed=seed), aspect)
    t = torch.from_numpy(frames).to(DEV)
    keep = t.clone()
    out, u8 = pre.batch(t, augment=True, want_u8=True)
    assert torch.equal(t, keep)                               # the caller's frames are never written
    h, w = frames.shape[1:3]
    side = (max(h, w), max(h, w)) if aspect == "pad" or pre.augmentations.pads_to_square else (h, w)
    fresh = DeviceAug(spec, p=p, seed=seed)
    par = fresh.sample(len(frames), *side)
    plain = processor(None, aspect)
    for i, f in enumerate(frames):
        a = augment_ref_frame(f, fresh.spec, aspect, par, i)
        assert np.array_equal(u8[i].cpu().numpy(), IO.preprocess_u8(a, aspect=aspect)), (spec, i)
        assert torch.equal(out[i], plain.batch(torch.from_numpy(a)[None])[0]), (spec, i)    # the same normalise launch
    return pre, par, out, u8


def test_pi0_end_to_end():
    frames = frames_of(3, 120, 160, 200)
    pre, par, out, u8 = check_against_ref("pi0", "pad", frames, 1.0, 3)
    assert par.apply_crop.all() and par.apply_rotate.all() and par.apply_jitter.all() and out.shape == (3, 3, 224, 224)
    assert len(np.unique(par.angle)) == 3 and (np.abs(par.angle) <= 5).all()
    # __call__ on a PIL frame is a batch of one: the first row of a fresh table
    from PIL import Image
    from dexbotic_amd.data.dataset.augmentations import DeviceAug
    one = processor(DeviceAug("pi0", p=1.0, seed=3), "pad")(Image.fromarray(frames[0]))
    assert torch.equal(one, out[0])
    # (above, the expand2square pad has the processor's colour while the rotation fills its corners with 0)
    check_against_ref("pi0", None, frames_of(2, 37, 53, 210), 1.0, 5)       # no expand2square: the policy's own zero pad is real
    _, par0, _, _ = check_against_ref("pi0", "pad", frames[:2], 0.0, 5)     # p = 0: cropped and rotated all the same, no jitter
    assert par0.apply_crop.all() and par0.apply_rotate.all() and not par0.apply_jitter.any()


def test_dm0_end_to_end():
    _, par, out, _ = check_against_ref("dm0", "pad", frames_of(2, 96, 128, 220), 1.0, 6)     # cropped to 728 x 728, then rotated
    assert par.apply_crop.all() and par.apply_rotate.all() and out.shape == (2, 3, 224, 224)


def test_custom_spec_rotates_some_uncropped_frames():
    """rotate_limit (-10, 10) at p = 0.5 and nothing else but a jitter: the frames keep their 40 x 56 and some of them turn"""
    from dexbotic_amd.data.dataset.augmentations import AugSpec, DeviceAug
    spec = AugSpec(rotate_limit=(-10, 10), rotate_p=0.5, jitter=(0.3, 0.4, 0.5, 0.1))
    seed = next(s for s in range(50) if 0 < DeviceAug(spec, p=1.0, seed=s).sample(5, 40, 56).apply_rotate.sum() < 5)
    _, par, _, _ = check_against_ref(spec, None, frames_of(5, 40, 56, 230), 1.0, seed)
    assert 0 < par.apply_rotate.sum() < 5 and not par.apply_crop.any() and par.apply_jitter.all()
    assert np.abs(par.angle[par.apply_rotate == 1]).max() > 5
    only = AugSpec(rotate_limit=(-10, 10), rotate_p=1.0)      # every frame turns and nothing else happens: no clone needed
    check_against_ref(only, None, frames_of(2, 40, 56, 240), 0.5, 1)


def test_device_aug_v3_is_pixel_aug_v3():
    from dexbotic_amd.data.dataset.augmentations import DeviceAug, PixelAug
    frames = torch.from_numpy(frames_of(6, 90, 120, 110))
    seed = next(s for s in range(50) if 0 < PixelAug("v3", p=0.5, seed=s).sample(6, 120, 120).apply_crop.sum() < 6)
    a, a8 = processor(DeviceAug("v3", p=0.5, seed=seed)).batch(frames, augment=True, want_u8=True)
    b, b8 = processor(PixelAug("v3", p=0.5, seed=seed)).batch(frames, augment=True, want_u8=True)
    assert torch.equal(a, b) and torch.equal(a8, b8)
    plain = processor(None).batch(frames)
    assert not torch.equal(a, plain)
    assert torch.equal(processor(DeviceAug("identity")).batch(frames, augment=True), plain)
    assert torch.equal(processor(DeviceAug("pi0", seed=1)).batch(frames), plain)          # augment defaults to False
