"""Answer-side transforms of a serving request (dexbotic/data/dataset/transform/output.py: ``ActionDenorm``, ``AbsoluteAction``):
the sampled chunk in normalised units -> physical units -> absolute actions.  Host numpy, evaluated in the reference's order and
with its dtype promotion: the statistics are float64 arrays, the chunk float32, so both results are float64."""
from __future__ import annotations

import math

import numpy as np


class ActionDenorm:
    """inverse of ActionNorm for every key of ``statistic_mapping`` (``strict=False``: the keys present only — the request's
    normalised ``state`` is brought back as well, before AbsoluteAction adds it).  Statistics shorter than the data's last axis are
    padded — mean 0 / std 1, min -1 / max 1 — IN the mapping, as the reference does: the padded arrays serve the next request."""

    def __init__(self, statistic_mapping: dict = {"default": {"min": -1, "max": 1}}, strict: bool = True,
                 use_quantiles: bool = False):
        self.statistic_mapping = statistic_mapping
        self.strict = strict
        self.use_quantiles = use_quantiles

    def __call__(self, episode_data_dict: dict, **kwargs) -> dict:
        for key, stats in self.statistic_mapping.items():
            if key in episode_data_dict:
                episode_data_dict[key] = self._denormalize(episode_data_dict[key], stats)
            elif self.strict:
                raise KeyError(f"{key} is not in the episode_data_dict, please check the statistic_mapping")
        return episode_data_dict

    @staticmethod
    def _pad(stats: dict, name: str, width: int, fill: float) -> None:
        have = stats[name].shape[-1]
        stats[name] = np.concatenate([stats[name], np.full(width - have, fill)], axis=-1)

    def _denormalize(self, data, stats):
        width = data.shape[-1]
        if self.use_quantiles:
            if stats["max"].shape[-1] != width:
                self._pad(stats, "max", width, 1.0)
                self._pad(stats, "min", width, -1.0)
            return (data + 1) / 2 * (stats["max"] - stats["min"] + 1e-6) + stats["min"]
        if stats["mean"].shape[-1] != width:
            self._pad(stats, "mean", width, 0.0)
            self._pad(stats, "std", width, 1.0)
        return data * (stats["std"] + 1e-6) + stats["mean"]


class AbsoluteAction:
    """``action`` (deltas against the request's ``state``) -> absolute actions: state + action, the ``non_delta_mask`` components
    (default the last) taken from the action as they are, the ``periodic_mask`` components wrapped once into
    [-periodic_range, periodic_range].  The action has the state's rank or one more (a chunk per state row)."""

    def __call__(self, episode_data_dict: dict, **kwargs) -> dict:
        if "state" not in episode_data_dict or "action" not in episode_data_dict:
            return episode_data_dict
        meta = episode_data_dict["meta_data"]
        keep = meta.get("non_delta_mask", [-1])
        periodic = meta.get("periodic_mask", None)
        span = meta.get("periodic_range", math.pi)
        state, action = episode_data_dict["state"], episode_data_dict["action"]
        if action.ndim == state.ndim:
            out = state + action
        elif action.ndim == state.ndim + 1:
            out = state[..., None, :] + action
        else:
            raise ValueError(f"The dim of action {action.ndim} should be equal to or one more than the dim of state {state.ndim}")
        out[..., keep] = action[..., keep]
        if periodic is not None:
            for d in periodic:
                out[..., d] = np.where(out[..., d] > span, out[..., d] - span * 2, out[..., d])
                out[..., d] = np.where(out[..., d] < -span, out[..., d] + span * 2, out[..., d])
        episode_data_dict["abs_action"] = out
        episode_data_dict["action"] = out
        return episode_data_dict
