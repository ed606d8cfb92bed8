"""Container transforms of a serving request (dexbotic/data/dataset/transform/common.py: ``ToNumpy``, ``ToTensor``, ``Pipeline``):
same constructors, same episode-dict contract.  Host code on purpose — a request's state row is a few dozen numbers, and what the
reference answers is defined by numpy's dtype promotion (float64 statistics against float32 data), kept here as it is."""
from __future__ import annotations

import numpy as np
import torch

_NUMBER = (int, float, bool, complex, np.number)


class ToNumpy:
    """numbers and (nested) lists of numbers -> numpy arrays, dicts walked, strings and everything else left as they are; a list whose
    converted items are all arrays is stacked"""

    def __call__(self, episode_data_dict, **kwargs):
        x = episode_data_dict
        if isinstance(x, dict):
            return {k: self(v) for k, v in x.items()}
        if isinstance(x, list):
            if all(isinstance(v, _NUMBER) for v in x):
                return np.array(x)
            items = [self(v) for v in x]
            return np.stack(items) if all(isinstance(v, np.ndarray) for v in items) else items
        if isinstance(x, _NUMBER):
            return np.array(x)
        return x


class ToTensor:
    """every leaf through ``torch.as_tensor`` (dicts and lists walked)"""

    def __call__(self, data, **kwargs):
        if isinstance(data, dict):
            return {k: self(v) for k, v in data.items()}
        if isinstance(data, list):
            return [self(v) for v in data]
        return torch.as_tensor(data)


class Pipeline:
    """transforms applied in order; like the reference it remembers the last ``predict_length`` / ``statistic_mapping`` it was given"""

    def __init__(self, transforms: list):
        self.transforms = []
        for t in transforms:
            self.add(t)

    def add(self, transform) -> None:
        if isinstance(transform, list):
            self.transforms.extend(transform)
            return
        self.transforms.append(transform)
        for attr in ("predict_length", "statistic_mapping"):
            if hasattr(transform, attr):
                setattr(self, attr, getattr(transform, attr))

    def __call__(self, episode_data_dict, **kwargs):
        for t in self.transforms:
            episode_data_dict = t(episode_data_dict, **kwargs)
        return episode_data_dict
