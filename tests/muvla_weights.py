"""The MuVLA fixture's weights and images, regenerated instead of stored: 36.9 M parameters do not fit a committed file.

One recipe, imported by scripts/gen_golden_muvla.py (which loads the result into the reference's class) and by the tests (which
load it into the native class): ``numpy.random.RandomState(seed)`` walked over the fixture's ordered (key, shape) list — N(0, 0.05)
matrices and biases, 1-D ``weight`` tensors (norm gains) 1 + 0.1 N(0, 1) — every value rounded to the bf16 grid, so the bf16 model
starts from exactly the same weights.  tests/golden/muvla_t1.npz stores the list, the seed and per-tensor checksums (sum and sum of
squares, float64): a recipe that drifts is caught by tests/test_muvla_config.py before any GPU test looks at a number."""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np
import torch


def bf16_grid(a: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def make_weights(keys: Sequence[str], shapes: Sequence[Tuple[int, ...]], seed: int) -> Dict[str, np.ndarray]:
    """state dict (fp32 arrays on the bf16 grid) for the ordered keys; the order is part of the recipe"""
    rs = np.random.RandomState(int(seed))
    w = {}
    for k, shape in zip(keys, shapes):
        shape = tuple(int(s) for s in shape)
        leaf = str(k).rsplit(".", 1)[-1]
        if leaf == "weight" and len(shape) == 1:
            a = 1.0 + 0.1 * rs.standard_normal(shape)
        else:
            a = 0.05 * rs.standard_normal(shape)
        w[str(k)] = bf16_grid(a)
    return w


def make_images(shape: Sequence[int], seed: int) -> np.ndarray:
    """the fixture's images: clipped standard normals on the bf16 grid, from a stream of their own (seed + 1)"""
    rs = np.random.RandomState(int(seed) + 1)
    return bf16_grid(np.clip(rs.standard_normal(tuple(int(s) for s in shape)), -2.5, 2.5))


def checksums(keys: Sequence[str], w: Dict[str, np.ndarray]) -> np.ndarray:
    """[len(keys), 2] float64: (sum, sum of squares) per tensor, in key order"""
    return np.array([[w[str(k)].astype(np.float64).sum(), np.square(w[str(k)].astype(np.float64)).sum()] for k in keys])


def pack_shapes(shapes: Sequence[Tuple[int, ...]]) -> np.ndarray:
    """[n, 4] int64, unused trailing dimensions 0 (npz files hold no ragged lists)"""
    out = np.zeros((len(shapes), 4), dtype=np.int64)
    for i, s in enumerate(shapes):
        out[i, :len(s)] = s
    return out


def unpack_shapes(packed: np.ndarray):
    return [tuple(int(v) for v in row if v > 0) for row in packed]


def from_fixture(g) -> Tuple[Dict[str, np.ndarray], np.ndarray]:
    """(weights, images) of an opened muvla_t1.npz"""
    keys = [str(k) for k in g["w_keys"]]
    w = make_weights(keys, unpack_shapes(g["w_shapes"]), int(g["seed"]))
    return w, make_images(g["image_shape"], int(g["seed"]))
