"""The DDIM schedule of the OFT diffusion head, as host arithmetic.

The reference builds ``diffusers.DDIMScheduler(num_train_timesteps=100, beta_schedule="squaredcos_cap_v2")`` and uses its defaults
(oft/action_model/model.py:220).  What that scheduler contributes is three closed-form formulas (Song et al., "Denoising Diffusion
Implicit Models"; Nichol & Dhariwal's cosine schedule), written down here so that nothing depends on the package:

* ``ab(s) = cos((s + 0.008) / 1.008 * pi / 2) ** 2``, ``beta_i = min(1 - ab((i + 1) / N) / ab(i / N), 0.999)`` in float64, stored as
  fp32; ``alphas_cumprod = cumprod(1 - beta)`` in fp32; ``final_alpha_cumprod = 1``;
* ``add_noise``: ``sqrt(a_t) x0 + sqrt(1 - a_t) noise``;
* ``set_timesteps(n)``, "leading" spacing, offset 0: ``t_k = (n - 1 - k) (N // n)``; ``step`` with eta = 0, epsilon prediction,
  ``clip_sample`` at 1: ``x0 = clamp((x - sqrt(1 - a_t) eps) / sqrt(a_t), -1, 1)``, ``x_prev = sqrt(a_prev) x0 + sqrt(1 - a_prev) eps``
  with ``a_prev = alphas_cumprod[t - N // n]``, 1 below zero; the model's own eps goes into the second term.

These are pinned to the formulas, NOT checked against the ``diffusers`` package.
"""
from __future__ import annotations

import math
from typing import List, Tuple

import numpy as np
import torch

CLIP_SAMPLE_RANGE = 1.0


def _alpha_bar(s: float) -> float:
    return math.cos((s + 0.008) / 1.008 * math.pi / 2) ** 2


class DDIMSchedule:
    def __init__(self, num_train_timesteps: int = 100):
        N = int(num_train_timesteps)
        if N < 1:
            raise ValueError(f"DDIMSchedule: num_train_timesteps = {N}")
        self.num_train_timesteps = N
        betas = np.array([min(1.0 - _alpha_bar((i + 1) / N) / _alpha_bar(i / N), 0.999) for i in range(N)], dtype=np.float64)
        self.betas = torch.from_numpy(betas.astype(np.float32))
        self.alphas_cumprod = torch.cumprod(1.0 - self.betas, dim=0)            # fp32, as the scheduler keeps it
        self.final_alpha_cumprod = 1.0
        self.timesteps: List[int] = list(range(N - 1, -1, -1))
        self.num_inference_steps = N
        self._dev = {}

    def tables(self, device) -> Tuple[torch.Tensor, torch.Tensor]:
        """(sqrt(a_t), sqrt(1 - a_t)) [N] fp32 on ``device``, uploaded once"""
        key = str(device)
        if key not in self._dev:
            a = self.alphas_cumprod
            self._dev[key] = ((a ** 0.5).to(device), ((1 - a) ** 0.5).to(device))
        return self._dev[key]

    def add_noise(self, original: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor) -> torch.Tensor:
        """``timesteps`` [B] int64 on the device of ``original`` [B, ...]"""
        sa, sb = self.tables(original.device)
        shape = (-1,) + (1,) * (original.dim() - 1)
        return sa[timesteps].view(shape) * original + sb[timesteps].view(shape) * noise

    def set_timesteps(self, n: int) -> List[int]:
        n, N = int(n), self.num_train_timesteps
        if not 1 <= n <= N:
            raise ValueError(f"DDIMSchedule: {n} inference steps outside [1, {N}]")
        ratio = N // n
        self.num_inference_steps = n
        self.timesteps = [(n - 1 - k) * ratio for k in range(n)]
        return self.timesteps

    def step_coefficients(self, k: int) -> Tuple[float, float, float, float]:
        """(c0, c1, c2, c3) of step k of the current timesteps: x0 = clamp(c0 x - c1 eps), x_prev = c2 x0 + c3 eps"""
        t = self.timesteps[k]
        prev = t - self.num_train_timesteps // self.num_inference_steps
        a_t = float(self.alphas_cumprod[t])
        a_prev = float(self.alphas_cumprod[prev]) if prev >= 0 else self.final_alpha_cumprod
        return 1.0 / math.sqrt(a_t), math.sqrt(1.0 - a_t) / math.sqrt(a_t), math.sqrt(a_prev), math.sqrt(1.0 - a_prev)

    def step(self, eps: torch.Tensor, k: int, x: torch.Tensor) -> torch.Tensor:
        """one step on host / torch tensors (the sampler runs dxa_ddim_step_embed; this is the statement the tests compare it with)"""
        c0, c1, c2, c3 = self.step_coefficients(k)
        x0 = (c0 * x - c1 * eps).clamp(-CLIP_SAMPLE_RANGE, CLIP_SAMPLE_RANGE)
        return c2 * x0 + c3 * eps
