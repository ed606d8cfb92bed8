#!/usr/bin/env python
"""Training-augmentation micro-benchmark: the device route of PreprocessRGB with a PixelAug or DeviceAug policy (crop-resize,
affine warp, colour jitter and preprocess launches; uint8 frames already in HBM) next to the same operations with Pillow on one
host core (tests/augment_ref's and tests/affine_ref's Pillow helpers + a bicubic resize and the normalise in numpy), on the same
frames, every frame cropped, rotated where the policy rotates, and jittered (p = 1).  Four workloads: 32 frames of 256 x 256
under 'v3' and under 'pi0', 48 frames of 728 x 728 under 'color_dm0' and under 'dm0'; the device and the host legs alternate
round by round inside one run, so both see the same machine.  For the rotating policies the affine launch is timed on the
output of the crop-resize launch, so the two rows are launches over the same number of output bytes.
    python scripts/augment_bench.py [--rounds 7] [--reps 20] [--out report.txt]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dexbotic_amd import kernels as K  # noqa: E402
from dexbotic_amd.data.dataset.augmentations import DeviceAug, PixelAug  # noqa: E402
from dexbotic_amd.data.dataset.rgb_preprocess import ImageProcessorSpec, PreprocessRGB  # noqa: E402
from tests import affine_ref as A  # noqa: E402
from tests import augment_ref as R  # noqa: E402

WORKLOADS = (("v3", 32, 256), ("color_dm0", 48, 728), ("pi0", 32, 256), ("dm0", 48, 728))


def policy_of(name, **kw):
    """the rotating policies are DeviceAug's; the others stay on PixelAug, as they were measured before"""
    return DeviceAug(name, **kw) if name in ("pi0", "dm0") else PixelAug(name, **kw)


def quartiles(x):
    q1, med, q3 = np.percentile(np.asarray(x, np.float64), [25, 50, 75])
    return {"q1": round(float(q1), 4), "median": round(float(med), 4), "q3": round(float(q3), 4), "samples": len(x)}


def timed(fn, reps, prepare=None):
    """per-call device-event and wall times (ms) of fn, each call ended by a synchronise; `prepare` runs untimed before each"""
    ev, wall = [], []
    for _ in range(reps):
        if prepare is not None:
            prepare()
            torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        ev.append(e0.elapsed_time(e1))
    return ev, wall


def host_batch(frames, policy, par, spec):
    """the reference's order of work per frame with Pillow: [pad] -> crop / resize -> [rotate] -> jitter -> bicubic resize ->
    normalise"""
    from PIL import Image
    aug = policy_of(policy)
    mean, std = np.asarray(spec.image_mean, np.float32), np.asarray(spec.image_std, np.float32)
    size = spec.size["shortest_edge"]
    out = []
    for i, f in enumerate(frames):
        if aug.pads_to_square:
            f = R.pil_pad_square(f, (0, 0, 0))
        if par.apply_crop[i]:
            f = R.pil_crop_resize(f, *(int(v) for v in par.box[i]), aug.crop_size)
        elif aug.resize is not None:
            f = np.asarray(Image.fromarray(f, "RGB").resize((aug.resize, aug.resize), Image.BILINEAR))
        if getattr(par, "apply_rotate", None) is not None and par.apply_rotate[i]:
            f = A.pil_rotate(f, float(par.angle[i]))
        if par.apply_jitter[i]:
            f = R.pil_color_jitter(f, par.order[i], par.factors[i], par.hue[i])
        u8 = np.asarray(Image.fromarray(f, "RGB").resize((size, size), Image.BICUBIC))
        x = (u8.astype(np.float64) * spec.rescale_factor).astype(np.float32)
        out.append(np.ascontiguousarray(((x - mean) / std).transpose(2, 0, 1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs the GPU: there is no host fallback to time")
    torch.set_num_threads(1)
    spec = ImageProcessorSpec()
    res = {"rounds": a.rounds, "reps_per_round": a.reps, "p": 1.0, "workloads": {}}
    state = []
    for policy, n, side in WORKLOADS:
        frames = np.random.RandomState(side).randint(0, 256, (n, side, side, 3)).astype(np.uint8)
        dev = torch.from_numpy(frames).cuda()
        pre = PreprocessRGB(spec, image_aspect_ratio="pad", augmentations=policy_of(policy, p=1.0, seed=0), device="cuda")
        par = policy_of(policy, p=1.0, seed=1).sample(n, side, side)
        aug = pre.augmentations
        out_side = aug.crop_size or aug.resize
        boxes = par.box if aug.crop_size else np.tile(np.asarray([0, 0, side], np.int32), (n, 1))
        resized = K.image_crop_resize(dev, boxes, out_side)
        work = resized.clone()                                   # the jitter works in place: every timed call starts from `resized`
        stages = {
            "crop_resize": lambda dev=dev, boxes=boxes, out_side=out_side: K.image_crop_resize(dev, boxes, out_side),
            "color_jitter": lambda work=work, par=par: K.image_color_jitter(work, par.apply_jitter, par.order, par.factors, par.hue),
            "preprocess": lambda resized=resized, pre=pre: pre.batch(resized),
            "batch": lambda dev=dev, pre=pre: pre.batch(dev, augment=True),
        }
        if isinstance(aug, DeviceAug):                           # the warp over what the crop-resize launch wrote: the same bytes out
            stages["affine"] = lambda resized=resized, par=par: K.image_rotate(resized, par.angle)
        for fn in stages.values():                               # warm every shape the timed window uses
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        host_batch(frames[:2], policy, par, spec)
        prepare = {"color_jitter": lambda work=work, resized=resized: work.copy_(resized)}
        state.append((policy, n, side, frames, par, stages, prepare, {k: ([], []) for k in stages}, []))
    for _ in range(a.rounds):                                    # device and host legs alternate, workload by workload
        for policy, n, side, frames, par, stages, prepare, dev_t, host_t in state:
            for k, fn in stages.items():
                ev, wall = timed(fn, a.reps, prepare.get(k))
                dev_t[k][0].extend(ev)
                dev_t[k][1].extend(wall)
            t0 = time.perf_counter()
            host_batch(frames, policy, par, spec)
            host_t.append(1e3 * (time.perf_counter() - t0))
    for policy, n, side, frames, par, stages, prepare, dev_t, host_t in state:
        w = {"policy": policy, "frames": n, "frame": f"{side}x{side}",
             "device_event_ms": {k: quartiles(v[0]) for k, v in dev_t.items()},
             "device_wall_ms": {k: quartiles(v[1]) for k, v in dev_t.items()},
             "host_pillow_1core_ms_per_batch": quartiles(host_t)}
        w["host_pillow_1core_ms_per_frame"] = round(w["host_pillow_1core_ms_per_batch"]["median"] / n, 4)
        w["device_batch_cheaper_than_host"] = bool(w["device_wall_ms"]["batch"]["q3"] < w["host_pillow_1core_ms_per_batch"]["q1"])
        res["workloads"][f"{policy}_{n}x{side}"] = w
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
