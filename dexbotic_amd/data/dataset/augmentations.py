"""Device-side PixelAug — mirror of dexbotic/data/dataset/augmentations.py:12-20 for the policies that are crops, pads,
resizes and colour jitter only.

The reference builds an albumentations pipeline per policy and runs it on the host, one PIL frame at a time.  Here the
object only DRAWS: ``sample(n, h, w)`` returns one row of parameters per frame, and PreprocessRGB hands the rows to
libdexbotic_amd's dxa_image_crop_resize / dxa_color_jitter together with the frames.  Covered:

    'v3'         RandomResizedCrop(384, scale (0.95, 1.0), ratio 1, p) -> ColorJitter(0.3, 0.4, 0.5, 0.08, p)
    'color'      PadToSquare(fill 0) -> ColorJitter(0.3, 0.4, 0.5, 0.1, p)
    'color_dm0'  PadToSquare(fill 0) -> Resize(728, 728) -> ColorJitter(0.3, 0.4, 0.5, 0.1, p)
    'identity'   nothing

'pi0' and 'dm0' rotate (a non-separable warp), 'v1' and 'v2' are noise / blur / dropout families: NotImplementedError.
Any other name is a KeyError, as in the reference's NAME2AUG.  The pixel arithmetic is Pillow's (crop + BILINEAR resize,
ImageEnhance + HSV), not cv2's: see the README."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

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


class PixelAug:
    def __init__(self, policy: str = "v3", p: float = 0.5, seed: Optional[int] = None):
        if policy in _NOT_ON_DEVICE:
            raise NotImplementedError(f"PixelAug policy {policy!r} needs {_NOT_ON_DEVICE[policy]}, which has no device kernel; "
                                      f"on the device: {sorted(_POLICIES)}")
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
        """RandomResizedCrop with ratio 1: side round(sqrt(u * h * w)), redrawn up to 10 times while it does not fit, then
        the central min(h, w) square"""
        for _ in range(10):
            c = int(round(float(np.sqrt(self.rng.uniform(*_CROP_SCALE) * h * w))))
            if 0 < c <= min(h, w):
                return int(self.rng.integers(0, w - c + 1)), int(self.rng.integers(0, h - c + 1)), c
        c = min(h, w)
        return (w - c) // 2, (h - c) // 2, c
