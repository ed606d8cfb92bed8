"""Generate tests/golden/flow_serve_t1.npz by running the REFERENCE's request transforms, prompt tokenisers and pi0 ``process_images``
on the CPU.

TEST INFRASTRUCTURE, CPU only.  Needs the reference tree next to this repository's build container (oracle/gen_golden.py: REF); the
fixture it writes is committed, so no test reads the reference.  Inputs and results only are recorded.

    python scripts/gen_golden_flow_serve.py            # from the repository root

What is run: tests/flow_serve_cases.py (the cases, stated once for this script and for tests/test_flow_serve_ref.py) over
``dexbotic.data.dataset.transform.{action,output,common}`` and ``dexbotic.tokenization.process``, the tokenisers over the stand-in
tokenizers of tests/flow_serve_tokenizers.py.  The ``transform`` package's ``__init__`` may pull in storage / video libraries that are
not installed; the three files are then loaded by path — they import numpy, torch, math and copy only.

pi0's frames: the reference's ``Pi0ForCausalLM.process_images`` (pi0_arch.py:493-511) on the tiny model of oracle/gen_golden_pi0.py
(SigLIP processor at 28 px) over two uint8 noise frames of unequal sides, 30 x 44 and 44 x 30 — padded with black to 44 x 44, then
resized 44 -> 28 by the processor's bicubic, so the pad colour and the resampler both show in the recorded pixel tensors."""
from __future__ import annotations

import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

FRAME_SHAPES = ((30, 44), (44, 30))


def reference_transforms(ref: str) -> types.SimpleNamespace:
    names = ("action", "output", "common")
    try:
        mods = [importlib.import_module(f"dexbotic.data.dataset.transform.{n}") for n in names]
        how = "imported"
    except Exception as e:                                       # noqa: BLE001  (reported below)
        mods = []
        for n in names:
            spec = importlib.util.spec_from_file_location(f"_ref_transform_{n}",
                                                          os.path.join(ref, "dexbotic/data/dataset/transform", n + ".py"))
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            mods.append(mod)
        how = f"loaded by path ({type(e).__name__}: {e})"
    ns = types.SimpleNamespace(how=how)
    for mod in mods:
        for k, v in vars(mod).items():
            if isinstance(v, type):
                setattr(ns, k, v)
    return ns


def main():
    from oracle.gen_golden import GOLD, REF, install_timm_shim
    from tests import flow_serve_cases as C
    sys.path.insert(0, REF)
    install_timm_shim()
    torch.set_num_threads(8)
    T = reference_transforms(REF)
    P = importlib.import_module("dexbotic.tokenization.process")

    inputs = C.make_inputs()
    res = {"in/" + k: v for k, v in inputs.items()}
    res["prompts"] = np.array(C.PROMPTS)
    res.update({"ref/" + k: np.asarray(v) for k, v in C.run_transforms(T, inputs).items()})
    res.update({"ref/" + k: np.asarray(v) for k, v in C.run_tokenizers(P).items()})

    # ---- pi0: raw frames through the reference's own process_images
    from PIL import Image
    from oracle.gen_golden_pi0 import build_reference
    from oracle.pi0_oracle import Pi0OracleConfig, pi0_shapes
    from oracle.weights import make_weights
    cfg = Pi0OracleConfig()
    m = build_reference(cfg, make_weights(pi0_shapes(cfg), 2468))
    rs = np.random.RandomState(C.SEED + 1)
    frames = [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in FRAME_SHAPES]
    pix = m.process_images([Image.fromarray(f) for f in frames])
    assert torch.is_tensor(pix) and tuple(pix.shape) == (2, 3, cfg.v_image, cfg.v_image) and pix.dtype == torch.float32
    for i, f in enumerate(frames):
        res[f"pix/frame{i}"] = f
    res["pix/out"] = pix.numpy()

    path = os.path.join(GOLD, "flow_serve_t1.npz")
    np.savez_compressed(path, **res)
    print(f"[gen_golden_flow_serve] transforms {T.how}; {len(res)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
