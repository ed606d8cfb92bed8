"""Device-side PixelAug — mirror of dexbotic/data/dataset/augmentations.py:12-20 for the policies that are crops, pads,
resizes, rotations and colour jitter only.

The reference builds an albumentations pipeline per policy and runs it on the host, one PIL frame at a time.  Here the
objects only DRAW: ``sample(n, h, w)`` returns one row of parameters per frame, and PreprocessRGB hands the rows to
libdexbotic_amd's dxa_image_crop_resize / dxa_image_affine / dxa_color_jitter together with the frames.

``PixelAug(name)`` covers the four policies without a rotation:

    'v3'         RandomResizedCrop(384, scale (0.95, 1.0), ratio 1, p) -> ColorJitter(0.3, 0.4, 0.5, 0.08, p)
    'color'      PadToSquare(fill 0) -> ColorJitter(0.3, 0.4, 0.5, 0.1, p)
    'color_dm0'  PadToSquare(fill 0) -> Resize(728, 728) -> ColorJitter(0.3, 0.4, 0.5, 0.1, p)
    'identity'   nothing

``DeviceAug(spec_or_name)`` takes a composition (``AugSpec``) of the five operations the reference's policies are made of
— PadToSquare, RandomResizedCrop, Resize, Rotate, ColorJitter — or the name of one: the four above and

    'pi0'        PadToSquare(fill 0) -> RandomResizedCrop(224, scale (0.95, 0.95), ratio 1, p=1) -> Rotate((-5, 5), p=1)
                 -> ColorJitter(0.3, 0.4, 0.5, 0.1, p)
    'dm0'        the same with RandomResizedCrop(728)

'v1' and 'v2' are noise / blur / dropout families: NotImplementedError.  Any other name is a KeyError, as in the
reference's NAME2AUG.  The pixel arithmetic is Pillow's (crop + BILINEAR resize, transform(AFFINE, BILINEAR),
ImageEnhance + HSV), not cv2's: see the README."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3

# crop: RandomResizedCrop output side; resize: Resize side; pad: PadToSquare(fill=0) first; hue: ColorJitter's hue range
_POLICIES = {
    "v3": dict(crop=384, resize=None, pad=False, hue=0.08),
    "color": dict(crop=None, resize=None, pad=True, hue=0.1),
    "color_dm0": dict(crop=None, resize=728, pad=True, hue=0.1),
    "identity": None,
}
_NOT_ON_DEVICE = {"pi0": "Rotate", "dm0": "Rotate", "v1": "CoarseDropout", "v2": "noise, blur and dropout families"}
_CROP_SCALE = (0.95, 1.0)
_JITTER = (0.3, 0.4, 0.5)                                     # brightness, contrast, saturation


@dataclass
class AugParams:
    """one row per frame"""
    apply_crop: np.ndarray      # int32 [n]
    box: np.ndarray             # int32 [n, 3]: x0, y0, c of the square crop in the (padded) frame
    apply_jitter: np.ndarray    # int32 [n]
    order: np.ndarray           # int32 [n, 4]: permutation of BRIGHTNESS, CONTRAST, SATURATION, HUE
    factors: np.ndarray         # float32 [n, 3]: brightness, contrast, saturation blend factors
    hue: np.ndarray             # float32 [n]: hue shift in turns

    def __len__(self):
        return len(self.apply_crop)

    def take(self, idx) -> "AugParams":
        return AugParams(self.apply_crop[idx], self.box[idx], self.apply_jitter[idx], self.order[idx], self.factors[idx],
                         self.hue[idx])


def _draw_box(rng, scale, h: int, w: int):
    """RandomResizedCrop with ratio 1: side round(sqrt(u * h * w)), redrawn up to 10 times while it does not fit, then
    the central min(h, w) square"""
    for _ in range(10):
        c = int(round(float(np.sqrt(rng.uniform(*scale) * h * w))))
        if 0 < c <= min(h, w):
            return int(rng.integers(0, w - c + 1)), int(rng.integers(0, h - c + 1)), c
    c = min(h, w)
    return (w - c) // 2, (h - c) // 2, c


class PixelAug:
    def __init__(self, policy: str = "v3", p: float = 0.5, seed: Optional[int] = None):
        if policy in _NOT_ON_DEVICE:
            where = f"DeviceAug({policy!r}) runs it on the device" if _NOT_ON_DEVICE[policy] == "Rotate" else "which has no device kernel"
            raise NotImplementedError(f"PixelAug policy {policy!r} needs {_NOT_ON_DEVICE[policy]}: {where}; "
                                      f"PixelAug on the device: {sorted(_POLICIES)}")
        if policy not in _POLICIES:
            raise KeyError(policy)
        self.policy, self.p = policy, float(p)
        spec = _POLICIES[policy]
        self.identity = spec is None
        self.crop_size = None if self.identity else spec["crop"]
        self.resize = None if self.identity else spec["resize"]
        self.pads_to_square = False if self.identity else spec["pad"]
        self.hue_range = 0.0 if self.identity else spec["hue"]
        self.rng = np.random.default_rng(seed)

    def sample(self, n: int, h: int, w: int) -> AugParams:
        """the draws for n frames of h x w (the size after any padding to a square).  Per frame, in this order: whether
        to crop, the crop, whether to jitter, the jitter."""
        par = AugParams(np.zeros(n, np.int32), np.zeros((n, 3), np.int32), np.zeros(n, np.int32),
                        np.tile(np.arange(4, dtype=np.int32), (n, 1)), np.ones((n, 3), np.float32), np.zeros(n, np.float32))
        par.box[:] = (0, 0, min(h, w))
        if self.identity:
            return par
        rng = self.rng
        for i in range(n):
            if self.crop_size is not None:
                par.apply_crop[i] = rng.random() < self.p
                par.box[i] = self._draw_box(h, w)
            par.apply_jitter[i] = rng.random() < self.p
            par.order[i] = rng.permutation(4)
            par.factors[i] = [rng.uniform(max(0.0, 1.0 - a), 1.0 + a) for a in _JITTER]
            par.hue[i] = rng.uniform(-self.hue_range, self.hue_range)
        return par

    def _draw_box(self, h: int, w: int):
        return _draw_box(self.rng, _CROP_SCALE, h, w)


# ------------------------------------------------------------------------------------------- compositions with a rotation
@dataclass(frozen=True)
class AugSpec:
    """A composition of the reference's five operations, in pipeline order: PadToSquare(fill 0) -> RandomResizedCrop(crop_size,
    crop_scale, ratio 1) or Resize(resize) -> Rotate(rotate_limit, bilinear, fill 0) -> ColorJitter(*jitter).  An operation
    whose field is None (False for the pad) is absent; a probability left at None is the policy's p."""
    pad_to_square: bool = False
    crop_size: Optional[int] = None
    crop_scale: Tuple[float, float] = _CROP_SCALE
    crop_p: Optional[float] = None
    resize: Optional[int] = None
    rotate_limit: Optional[Tuple[float, float]] = None          # degrees, counter-clockwise
    rotate_p: Optional[float] = None
    jitter: Optional[Tuple[float, float, float, float]] = None  # brightness, contrast, saturation, hue ranges
    jitter_p: Optional[float] = None

    def __post_init__(self):
        if self.crop_size is not None and self.resize is not None:
            raise ValueError("AugSpec: at most one of crop_size and resize may be set")
        for name in ("crop_size", "resize"):
            v = getattr(self, name)
            if v is not None and int(v) <= 0:
                raise ValueError(f"AugSpec: {name} must be positive, got {v}")
        lo, hi = self.crop_scale
        if not 0.0 < lo <= hi:
            raise ValueError(f"AugSpec: crop_scale must be 0 < lo <= hi, got {self.crop_scale}")
        if self.rotate_limit is not None:
            lo, hi = self.rotate_limit
            if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
                raise ValueError(f"AugSpec: rotate_limit must be finite with lo <= hi, got {self.rotate_limit}")
        if self.jitter is not None:
            if len(self.jitter) != 4 or min(self.jitter) < 0 or self.jitter[3] > 0.5:
                raise ValueError(f"AugSpec: jitter is (brightness, contrast, saturation, hue), all >= 0 and hue <= 0.5, got {self.jitter}")
        for name in ("crop_p", "rotate_p", "jitter_p"):
            v = getattr(self, name)
            if v is not None and not 0.0 <= v <= 1.0:
                raise ValueError(f"AugSpec: {name} must be a probability, got {v}")

    @property
    def identity(self) -> bool:
        return not (self.pad_to_square or self.crop_size is not None or self.resize is not None
                    or self.rotate_limit is not None or self.jitter is not None)

    @staticmethod
    def of(name: str) -> "AugSpec":
        """the reference's composition of that name (NAME2AUG)"""
        if name in ("pi0", "dm0"):
            return AugSpec(pad_to_square=True, crop_size=224 if name == "pi0" else 728, crop_scale=(0.95, 0.95), crop_p=1.0,
                           rotate_limit=(-5.0, 5.0), rotate_p=1.0, jitter=_JITTER + (0.1,))
        if name in _NOT_ON_DEVICE:
            raise NotImplementedError(f"policy {name!r} needs {_NOT_ON_DEVICE[name]}, which has no device kernel; "
                                      f"on the device: {sorted(list(_POLICIES) + ['pi0', 'dm0'])}")
        if name not in _POLICIES:
            raise KeyError(name)
        pol = _POLICIES[name]
        if pol is None:
            return AugSpec()
        return AugSpec(pad_to_square=pol["pad"], crop_size=pol["crop"], resize=pol["resize"], jitter=_JITTER + (pol["hue"],))


@dataclass
class DeviceAugParams(AugParams):
    """AugParams and the rotation's two columns"""
    apply_rotate: np.ndarray    # int32 [n]
    angle: np.ndarray           # float64 [n]: degrees, counter-clockwise as Pillow's Image.rotate

    def take(self, idx) -> "DeviceAugParams":
        return DeviceAugParams(self.apply_crop[idx], self.box[idx], self.apply_jitter[idx], self.order[idx], self.factors[idx],
                               self.hue[idx], self.apply_rotate[idx], self.angle[idx])


class DeviceAug:
    """draws for an AugSpec (or the name of one of the reference's).  `seed` is whatever numpy.random.default_rng takes."""

    def __init__(self, spec="v3", p: float = 0.5, seed=None):
        self.policy = spec if isinstance(spec, str) else None
        self.spec = AugSpec.of(spec) if isinstance(spec, str) else spec
        if not isinstance(self.spec, AugSpec):
            raise TypeError(f"DeviceAug takes an AugSpec or a policy name, got {type(spec).__name__}")
        self.p = float(p)
        s = self.spec
        self.identity = s.identity
        self.crop_size, self.resize, self.pads_to_square = s.crop_size, s.resize, bool(s.pad_to_square)
        self.crop_p, self.rotate_p, self.jitter_p = (self.p if v is None else float(v) for v in (s.crop_p, s.rotate_p, s.jitter_p))
        self.rng = np.random.default_rng(seed)

    def sample(self, n: int, h: int, w: int) -> DeviceAugParams:
        """the draws for n frames of h x w (the size after any padding to a square).  Per frame one block per operation
        the spec has, in pipeline order: crop (whether, then the box), rotate (whether, then the angle), jitter (whether,
        then the order, the three factors and the hue).  A block is drawn even when its probability is 1."""
        par = DeviceAugParams(np.zeros(n, np.int32), np.zeros((n, 3), np.int32), np.zeros(n, np.int32),
                              np.tile(np.arange(4, dtype=np.int32), (n, 1)), np.ones((n, 3), np.float32), np.zeros(n, np.float32),
                              np.zeros(n, np.int32), np.zeros(n, np.float64))
        par.box[:] = (0, 0, min(h, w))
        s, rng = self.spec, self.rng
        for i in range(n):
            if s.crop_size is not None:
                par.apply_crop[i] = rng.random() < self.crop_p
                par.box[i] = _draw_box(rng, s.crop_scale, h, w)
            if s.rotate_limit is not None:
                par.apply_rotate[i] = rng.random() < self.rotate_p
                par.angle[i] = rng.uniform(*s.rotate_limit)
            if s.jitter is not None:
                par.apply_jitter[i] = rng.random() < self.jitter_p
                par.order[i] = rng.permutation(4)
                par.factors[i] = [rng.uniform(max(0.0, 1.0 - a), 1.0 + a) for a in s.jitter[:3]]
                par.hue[i] = rng.uniform(-s.jitter[3], s.jitter[3])
        return par

    @staticmethod
    def for_cameras(aug_policy, num_images: int, p: float = 0.5, seed=None):
        """one DeviceAug (or None) per camera, as dex_dataset.py:49-76 builds its PreprocessRGB list: a string gives every
        camera that policy, a list names each camera's (a falsy entry: no augmentation).  The cameras' generators are
        spawned from one numpy.random.SeedSequence(seed), so they are independent and the whole set is reproducible."""
        if isinstance(aug_policy, str):
            policies = [aug_policy] * num_images
        elif isinstance(aug_policy, list):
            assert len(aug_policy) == num_images, \
                f"The length of aug_policy {len(aug_policy)} must be equal to num_images {num_images}"
            policies = aug_policy
        else:
            raise ValueError(f"Invalid aug_policy: {aug_policy}, must be str or list")
        seeds = np.random.SeedSequence(seed).spawn(num_images)
        return [DeviceAug(pol, p=p, seed=s) if pol else None for pol, s in zip(policies, seeds)]
