"""Device-side PreprocessRGB — drop-in for dexbotic/data/dataset/rgb_preprocess.py:5-44.

The reference pads the PIL frame to a square, then lets the HF CLIP image processor resize (Pillow bicubic), crop,
rescale and normalise it on the host, one frame at a time.  Here the uint8 frame goes to the MI355X as it is
(h*w*3 bytes over PCIe instead of 3*224*224 floats) and libdexbotic_amd's dxa_image_preprocess does all of that in two
launches, bit-exact with Pillow's 8-bit resampler (tests/test_image_gpu.py).  Same constructor, same call."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from ... import kernels as K
from .augmentations import DeviceAug, PixelAug


def _edge(v, key):
    """one entry of the size / crop_size of an HF image processor (dict, SizeDict or a bare int)"""
    if isinstance(v, int):
        return v
    if isinstance(v, dict):
        return v.get(key)
    return getattr(v, key, None)


class ImageProcessorSpec:
    """the fields of an HF CLIPImageProcessor this path reads (defaults: openai/clip-vit-large-patch14)"""

    def __init__(self, size: int = 224, crop_size: int = 224, image_mean: Sequence[float] = (0.48145466, 0.4578275, 0.40821073),
                 image_std: Sequence[float] = (0.26862954, 0.26130258, 0.27577711), rescale_factor: float = 1 / 255):
        self.size = {"shortest_edge": size}
        self.crop_size = {"height": crop_size, "width": crop_size}
        self.image_mean, self.image_std, self.rescale_factor = tuple(image_mean), tuple(image_std), rescale_factor


def to_uint8_hwc(image) -> torch.Tensor:
    """PIL.Image / numpy / torch frame -> contiguous uint8 [h, w, 3] tensor (host or device, unchanged)"""
    if isinstance(image, torch.Tensor):
        t = image
    elif isinstance(image, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(image))
    else:                                               # PIL image: the reference feeds .convert('RGB') frames
        t = torch.from_numpy(np.asarray(image.convert("RGB") if getattr(image, "mode", "RGB") != "RGB" else image).copy())
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[-1] != 3:
        raise ValueError(f"expected a uint8 RGB frame [h, w, 3], got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


class PreprocessRGB:
    def __init__(self, image_processor, image_aspect_ratio=None, augmentations=None, image_pad_mode="mean",
                 device: Optional[torch.device] = None, dtype: torch.dtype = torch.float32):
        self.image_processor = image_processor
        self.image_aspect_ratio = image_aspect_ratio
        self.augmentations = augmentations
        self.image_pad_mode = image_pad_mode
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.dtype = dtype

    # ---- geometry / constants read off the processor exactly where the reference reads them
    def _crop(self):
        cs = getattr(self.image_processor, "crop_size", None) or self.image_processor.size
        return int(_edge(cs, "height")), int(_edge(cs, "width"))

    def _short(self):
        s = self.image_processor.size
        v = _edge(s, "shortest_edge")
        return int(v if v is not None else _edge(s, "height"))

    def _bg(self):
        if self.image_pad_mode == "zero":                                   # rgb_preprocess.py:20-21
            return (0, 0, 0)
        return tuple(int(x * 255) for x in self.image_processor.image_mean)  # rgb_preprocess.py:23

    def batch(self, frames: torch.Tensor, want_u8: bool = False, augment: bool = False):
        """frames: uint8 [n, h, w, 3] (host or device) -> [n, 3, H, W] on the device.  With `augment` the frames first go
        through the PixelAug or DeviceAug policy given as `augmentations`, on the device, each frame with its own draw."""
        frames = frames.to(self.device, non_blocking=True)
        if augment:
            if not isinstance(self.augmentations, (PixelAug, DeviceAug)):
                raise ValueError("batch(augment=True) needs augmentations=PixelAug(...) or DeviceAug(...); a host callable works per "
                                 "frame through __call__")
            if not self.augmentations.identity:
                return self._augmented(frames, want_u8)
        return self._preprocess(frames, want_u8)

    def process(self, images):
        """the ``process_images`` of the policies: PIL / numpy / torch uint8 frames [h, w, 3] -> [n, 3, H, W].  Frames of equal size
        share one launch pair; frames of unequal sizes go one by one and the result is stacked when all outputs have one shape
        (a list otherwise), as in the reference."""
        frames = [to_uint8_hwc(im) for im in images]
        if frames and all(f.shape == frames[0].shape for f in frames):
            if all(f.device.type == "cpu" for f in frames):
                # host frames are stacked by numpy (one memcpy per frame): torch.stack above ATen's parallel grain wakes the whole
                # OpenMP pool for 393 KB, and its spinning workers cost a serving process its cgroup CPU quota (hostcpu.py)
                return self.batch(torch.from_numpy(np.stack([f.numpy() for f in frames])))
            return self.batch(torch.stack(frames))
        out = [self.batch(f[None])[0] for f in frames]
        if out and all(x.shape == out[0].shape for x in out):
            out = torch.stack(out, dim=0)
        return out

    def _preprocess(self, frames, want_u8):
        p = self.image_processor
        return K.image_preprocess(frames, pad=self.image_aspect_ratio == "pad", bg=self._bg(), size=self._short(),
                                  crop=self._crop(), mean=p.image_mean, std=p.image_std,
                                  rescale=getattr(p, "rescale_factor", 1 / 255), out_dtype=self.dtype, want_u8=want_u8)

    def _augmented(self, frames, want_u8):
        """expand2square with the processor's colour where the reference has it (before the augmentation), then the policy:
        its own PadToSquare(fill=0) is a no-op on a square frame and a real zero pad otherwise.  A batch stays rectangular,
        so the frames 'v3' crops (-> 384 x 384) and the ones it leaves at their size go through the launches as two groups.
        A DeviceAug's rotation comes after the crop or resize of its group and before the jitter, at whatever size the frames
        then have; it fills with 0 whatever image_pad_mode is, as albumentations' Rotate does."""
        aug = self.augmentations
        K._check_u8_frames(frames, "PreprocessRGB.batch")
        n, h, w, _ = frames.shape
        expand = self.image_aspect_ratio == "pad"
        padded = (expand or aug.pads_to_square) and h != w
        ph, pw = (max(h, w), max(h, w)) if padded else (h, w)
        bg = self._bg() if expand else (0, 0, 0)
        if aug.resize is not None and ph != pw:                  # an AugSpec can ask for this; the named policies pad first
            raise ValueError(f"the Resize of an augmentation policy takes square frames, got {ph} x {pw}: pad them to a square first")
        par = aug.sample(n, ph, pw)
        groups = []                                              # (frame indices, boxes or None, output side)
        cropped = np.flatnonzero(par.apply_crop)
        whole = np.flatnonzero(par.apply_crop == 0)
        if len(cropped):
            groups.append((cropped, par.box[cropped], aug.crop_size))
        if len(whole):
            if aug.resize is not None or padded:                 # both only ever see square frames
                box = np.tile(np.asarray([0, 0, ph], np.int32), (len(whole), 1))
                groups.append((whole, box, aug.resize if aug.resize is not None else ph))
            else:
                groups.append((whole, None, None))
        ch, cw = self._crop()
        out = torch.empty(n, 3, ch, cw, device=self.device, dtype=self.dtype)
        u8 = torch.empty(n, ch, cw, 3, device=self.device, dtype=torch.uint8) if want_u8 else None
        for idx, box, side in groups:
            everything = len(idx) == n
            sel = None if everything else torch.from_numpy(idx).to(self.device)
            sub = frames if everything else frames.index_select(0, sel)
            own = not everything                                 # index_select copied them
            if box is not None:
                sub, own = K.image_crop_resize(sub, box, side, pad=padded, bg=bg), True
            q = par.take(idx)
            turn = np.flatnonzero(getattr(q, "apply_rotate", ()))
            if len(turn) == len(idx):
                sub, own = K.image_rotate(sub, q.angle), True
            elif len(turn):
                tsel = torch.from_numpy(turn).to(self.device)
                sub = sub if own else sub.clone()
                sub.index_copy_(0, tsel, K.image_rotate(sub.index_select(0, tsel), q.angle[turn]))
                own = True
            if not own:
                sub = sub.clone()                                # the jitter works in place: never on the caller's frames
            K.image_color_jitter(sub, q.apply_jitter, q.order, q.factors, q.hue)
            res = self._preprocess(sub, want_u8)
            o, o8 = res if want_u8 else (res, None)
            if everything:
                out, u8 = o, o8
            else:
                out.index_copy_(0, sel, o)
                if want_u8:
                    u8.index_copy_(0, sel, o8)
        return (out, u8) if want_u8 else out

    def __call__(self, image) -> torch.Tensor:
        if image is None:                                                   # rgb_preprocess.py:14-19
            ch, cw = self._crop()
            return torch.zeros(3, ch, cw, device=self.device, dtype=self.dtype)
        if isinstance(self.augmentations, (PixelAug, DeviceAug)):           # the device policies: one frame is a batch of one
            return self.batch(to_uint8_hwc(image)[None], augment=True)[0]
        if self.augmentations:                                              # any other callable works on PIL frames on the host
            if self.image_aspect_ratio == "pad":
                from PIL import Image
                w, h = image.size
                if w != h:
                    side = max(w, h)
                    sq = Image.new(image.mode, (side, side), self._bg())
                    sq.paste(image, (0, (w - h) // 2) if w > h else ((h - w) // 2, 0))
                    image = sq
            image = self.augmentations(image=image)
        return self.batch(to_uint8_hwc(image)[None])[0]


class DummyRGBProcessor:
    def __call__(self, image) -> torch.Tensor:
        return torch.zeros(1)
