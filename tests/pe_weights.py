"""The Perception Encoder fixtures' weights and images, regenerated instead of stored: the recipe of tests/muvla_weights.py over the
fixture's ordered (key, shape) list, with one change — every LayerScale ``gamma`` g becomes 1 + 10 g (1 + 0.5 N(0, 1), on the bf16
grid).  At the recipe's own 0.05 N(0, 1) the two branches of a block would hardly reach the output, and a wrong block would pass.

Imported by scripts/gen_golden_pe.py (which loads the result into the reference's classes) and by the tests (native classes);
tests/golden/pe_t1.npz and dm0_pe_t1.npz store the list, the seed and per-tensor checksums of the result."""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np

from . import muvla_weights as MW


def make_weights(keys: Sequence[str], shapes: Sequence[Tuple[int, ...]], seed: int) -> Dict[str, np.ndarray]:
    w = MW.make_weights(keys, shapes, seed)
    for k in w:
        if k.endswith(".gamma"):
            w[k] = MW.bf16_grid(1.0 + 10.0 * w[k])
    return w


def from_fixture(g) -> Tuple[Dict[str, np.ndarray], np.ndarray]:
    """(weights, images) of an opened pe_t1.npz / dm0_pe_t1.npz"""
    keys = [str(k) for k in g["w_keys"]]
    return make_weights(keys, MW.unpack_shapes(g["w_shapes"]), int(g["seed"])), MW.make_images(g["image_shape"], int(g["seed"]))
