"""Training augmentations on the GPU: dxa_image_crop_resize and dxa_color_jitter (through dexbotic_amd.kernels) and the
PixelAug route of PreprocessRGB against tests/augment_ref.py, which tests/test_augment_ref.py pins to Pillow.  Every
comparison is bit for bit."""
import itertools

import numpy as np
import pytest
import torch

from . import augment_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ORDERS = list(itertools.permutations(range(4)))
BG = (122, 116, 104)                                          # int(CLIP mean * 255)


def frames_of(n, h, w, seed):
    from oracle import image_oracle as IO
    return np.stack([IO.synthetic_image(h, w, seed + i) for i in range(n)])


def crop_resize_dev(frames, boxes, S, pad):
    from dexbotic_amd import kernels as K
    out = K.image_crop_resize(torch.from_numpy(frames).to(DEV), boxes, S, pad=pad, bg=BG)
    assert out.shape == (len(frames), S, S, 3) and out.dtype == torch.uint8
    return out.cpu().numpy()


def crop_resize_ref(frames, boxes, S, pad):
    return np.stack([R.crop_resize(R.pad_square(f, BG) if pad else f, x0, y0, c, S) for f, (x0, y0, c) in zip(frames, boxes)])


def jitter_dev(frames, apply, order, factors, hue):
    from dexbotic_amd import kernels as K
    t = torch.from_numpy(frames).to(DEV)
    assert K.image_color_jitter(t, apply, order, factors, hue) is t
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------------ crop + resize
@pytest.mark.parametrize("S", [48, 17])                      # 48: dword path, up- and down-scaling; 17: the byte path
def test_crop_resize_padded_frames(S):
    frames = frames_of(5, 37, 53, 10)                        # padded to 53 x 53: 8 rows of background above and below
    boxes = [(0, 0, 53), (50, 50, 3), (5, 7, 29), (16, 0, 37), (2, 3, 48)]
    assert np.array_equal(crop_resize_dev(frames, boxes, S, True), crop_resize_ref(frames, boxes, S, True))


def test_crop_resize_unpadded_frames():
    frames = frames_of(5, 64, 64, 20)
    boxes = [(0, 0, 64), (61, 0, 3), (1, 2, 62), (10, 16, 48), (7, 5, 51)]
    assert np.array_equal(crop_resize_dev(frames, boxes, 48, False), crop_resize_ref(frames, boxes, 48, False))
    rect = frames_of(5, 37, 53, 30)                          # rectangular, no pad: boxes that touch two and three borders
    boxes = [(0, 0, 37), (16, 0, 37), (8, 0, 37), (50, 34, 3), (1, 1, 35)]
    assert np.array_equal(crop_resize_dev(rect, boxes, 48, False), crop_resize_ref(rect, boxes, 48, False))


def test_crop_resize_to_384():
    frames = frames_of(1, 64, 64, 40)
    assert np.array_equal(crop_resize_dev(frames, [(1, 2, 61)], 384, False), crop_resize_ref(frames, [(1, 2, 61)], 384, False))


# ------------------------------------------------------------------------------------------------------------- jitter
def test_jitter_all_orders():
    """24 frames of 37 x 53, one per order: 5883 bytes a frame, so the frames start at every byte alignment"""
    frames = frames_of(24, 37, 53, 50)
    rs = np.random.RandomState(2)
    factors = np.float32([[rs.uniform(0.7, 1.3), rs.uniform(0.6, 1.4), rs.uniform(0.5, 1.5)] for _ in ORDERS])
    factors[0], factors[1] = (0.7, 1.4, 0.5), (1.3, 0.6, 1.5)
    hue = np.float32([(0.1, -0.1, 0.0)[i % 3] for i in range(24)])
    got = jitter_dev(frames, np.ones(24, np.int32), ORDERS, factors, hue)
    for i, order in enumerate(ORDERS):
        assert np.array_equal(got[i], R.color_jitter(frames[i], order, factors[i], hue[i])), order


def test_jitter_mixed_batch_leaves_the_others_alone():
    frames = frames_of(6, 64, 64, 80)
    apply = np.int32([1, 0, 0, 1, 0, 1])
    order = [ORDERS[5], ORDERS[0], ORDERS[0], ORDERS[17], ORDERS[0], ORDERS[22]]
    factors = np.float32([[1.2, 0.8, 1.1], [9, 9, 9], [9, 9, 9], [0.75, 1.35, 0.6], [9, 9, 9], [1.0, 1.0, 1.0]])
    hue = np.float32([0.1, 0.3, 0.3, -0.1, 0.3, 0.0])
    got = jitter_dev(frames, apply, order, factors, hue)
    for i in range(6):
        want = R.color_jitter(frames[i], order[i], factors[i], hue[i]) if apply[i] else frames[i]
        assert np.array_equal(got[i], want), i


def test_jitter_contrast_mean_rounding():
    """mean L exactly 100.5 rounds up to 101, 100 + 11/24 does not"""
    frames = np.full((2, 4, 6, 3), 100, np.uint8)
    frames[0].reshape(-1, 3)[:12] = 101
    frames[1].reshape(-1, 3)[:11] = 101
    ones = np.float32([[1.0, 0.0, 1.0]] * 2)
    got = jitter_dev(frames, [1, 1], [ORDERS[0]] * 2, ones, np.float32([0, 0]))
    assert (got[0] == 101).all() and (got[1] == 100).all()
    order, factors = (2, 1, 3, 0), np.float32([[1.1, 0.5, 0.9]] * 2)
    got = jitter_dev(frames, [1, 1], [order] * 2, factors, np.float32([0.1, 0.1]))
    for i in range(2):
        assert np.array_equal(got[i], R.color_jitter(frames[i], order, factors[i], np.float32(0.1)))


def test_jitter_sum_of_a_large_frame_needs_64_bits():
    """4104 x 4104 white pixels: 2 * sum(L) + N is past 2^32, so a 32-bit sum would give a darker mean"""
    from dexbotic_amd import kernels as K
    t = torch.full((1, 4104, 4104, 3), 255, dtype=torch.uint8, device=DEV)
    K.image_color_jitter(t, [1], [(1, 0, 2, 3)], np.float32([[1.0, 0.5, 1.0]]), np.float32([0.0]))
    assert int(t.min()) == 255


# -------------------------------------------------------------------------------------------------------- end to end
def processor(policy=None, aspect="pad", **kw):
    from dexbotic_amd.data.dataset.augmentations import PixelAug
    from dexbotic_amd.data.dataset.rgb_preprocess import ImageProcessorSpec, PreprocessRGB
    aug = PixelAug(policy, **kw) if policy else None
    return PreprocessRGB(ImageProcessorSpec(), image_aspect_ratio=aspect, augmentations=aug, device=DEV)


def augment_ref_frame(frame, policy, aspect, par, i):
    """what the policy does to one frame, with row i of the drawn table: uint8 HWC"""
    from dexbotic_amd.data.dataset.augmentations import PixelAug
    aug = PixelAug(policy)
    if aspect == "pad":
        frame = R.pad_square(frame, BG)
    if aug.pads_to_square:
        frame = R.pad_square(frame, (0, 0, 0))
    if par.apply_crop[i]:
        frame = R.crop_resize(frame, *par.box[i], aug.crop_size)
    elif aug.resize is not None:
        frame = R.resize_bilinear(frame, aug.resize, aug.resize)
    if par.apply_jitter[i]:
        frame = R.color_jitter(frame, par.order[i], par.factors[i], par.hue[i])
    return frame


def check_against_ref(policy, aspect, frames, p, seed):
    from dexbotic_amd.data.dataset.augmentations import PixelAug
    from oracle import image_oracle as IO
    pre = processor(policy, aspect, p=p, seed=seed)
    out, u8 = pre.batch(torch.from_numpy(frames), augment=True, want_u8=True)
    h, w = frames.shape[1:3]
    side = (max(h, w), max(h, w)) if aspect == "pad" or pre.augmentations.pads_to_square else (h, w)
    par = PixelAug(policy, p=p, seed=seed).sample(len(frames), *side)
    plain = processor(None, aspect)
    for i, f in enumerate(frames):
        a = augment_ref_frame(f, policy, aspect, par, i)
        assert np.array_equal(u8[i].cpu().numpy(), IO.preprocess_u8(a, aspect=aspect)), (policy, i)
        assert torch.equal(out[i], plain.batch(torch.from_numpy(a)[None])[0]), (policy, i)   # the same normalise launch
    return pre, par, out, u8


def test_v3_end_to_end():
    frames = frames_of(3, 120, 160, 100)
    pre, par, out, u8 = check_against_ref("v3", "pad", frames, 1.0, 3)
    assert par.apply_crop.all() and par.apply_jitter.all() and out.shape == (3, 3, 224, 224)
    again, again8 = processor("v3", "pad", p=1.0, seed=3).batch(torch.from_numpy(frames), augment=True, want_u8=True)
    assert torch.equal(again, out) and torch.equal(again8, u8)              # same seed, same bytes
    other = processor("v3", "pad", p=1.0, seed=4).batch(torch.from_numpy(frames), augment=True)
    assert not torch.equal(other, out)
    # __call__ on a PIL frame is a batch of one: the first row of a fresh table
    from PIL import Image
    one = processor("v3", "pad", p=1.0, seed=3)(Image.fromarray(frames[0]))
    assert torch.equal(one, out[0])


def test_v3_mixed_draws_go_through_two_groups():
    from dexbotic_amd.data.dataset.augmentations import PixelAug
    frames = frames_of(6, 90, 120, 110)
    seed = next(s for s in range(50) if 0 < PixelAug("v3", p=0.5, seed=s).sample(6, 120, 120).apply_crop.sum() < 6)
    _, par, _, _ = check_against_ref("v3", "pad", frames, 0.5, seed)
    assert 0 < par.apply_crop.sum() < 6
    check_against_ref("v3", None, frames_of(3, 64, 64, 115), 0.5, seed)     # square frames, nothing padded, no-crop frames cloned


def test_color_policies_end_to_end():
    frames = frames_of(2, 37, 53, 120)
    check_against_ref("color", None, frames, 1.0, 5)                        # the policy's own zero pad is real here
    check_against_ref("color", "pad", frames, 1.0, 5)                       # ... and a no-op after expand2square
    check_against_ref("color_dm0", None, frames, 1.0, 6)


def test_without_a_device_policy_nothing_changes():
    from oracle import image_oracle as IO
    frames = frames_of(2, 120, 160, 130)
    t = torch.from_numpy(frames)
    out, u8 = processor(None).batch(t, want_u8=True)
    for i in range(2):
        assert np.array_equal(u8[i].cpu().numpy(), IO.preprocess_u8(frames[i]))
    assert torch.equal(processor("v3", p=1.0, seed=1).batch(t), out)         # augment defaults to False
    assert torch.equal(processor("identity").batch(t, augment=True), out)
    with pytest.raises(ValueError):
        processor(None).batch(t, augment=True)
    from PIL import Image
    from dexbotic_amd.data.dataset.rgb_preprocess import ImageProcessorSpec, PreprocessRGB
    seen = []

    def host_aug(image):                                                     # a host callable keeps the host path
        seen.append(image.size)
        return image

    pre = PreprocessRGB(ImageProcessorSpec(), image_aspect_ratio="pad", augmentations=host_aug, device=DEV)
    assert torch.equal(pre(Image.fromarray(frames[0])), out[0]) and seen == [(160, 160)]
    # the jitter works in place, but never on the caller's frames ('color' on square frames: no pad, no resize)
    d = torch.from_numpy(frames_of(2, 64, 64, 140)).to(DEV)
    keep = d.clone()
    jit = processor("color", None, p=1.0, seed=2).batch(d, augment=True)
    assert torch.equal(d, keep) and not torch.equal(jit, processor(None, None).batch(d))
