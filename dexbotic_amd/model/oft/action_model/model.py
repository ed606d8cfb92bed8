"""Action heads of the OFT policy: host-side mirror of dexbotic/model/oft/action_model/model.py on libdexbotic_amd kernels.

``L1RegressionActionHead`` (:129-160): ``action_query`` [1, T A, d], the learned rows placed behind every sample's prompt, and an
``MLPResNet`` (:104-126) that reads the A hidden rows of one time step as ONE row of A d columns: layer_norm1 -> fc1 -> ReLU -> two
``MLPResNetBlock`` (:83-101, LayerNorm -> Linear -> ReLU, plus the skip) -> layer_norm2 -> fc2.  ``ProprioProjector`` (:12-30):
fc1 -> GELU(erf) -> fc2.  ``DiscreteActionHead`` (:273-347): no trunk at all — the LLM's vocabulary is the head; it carries the bin
<-> action helpers and the optional projector.  ``DiffusionActionHead`` (:197-271): ``NoisyActionProjector`` (:33-55), the
sinusoidal time row (:57-80) and the same ``MLPResNet`` under ``noise_predictor.mlp_resnet`` (:163-194); its scheduler is
ddim.DDIMSchedule.  Parameter names as in the reference's modules.  The products run in the compute dtype (the reference runs
them under autocast), the LayerNorm statistics in fp32.
"""
from __future__ import annotations

import math
import re
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from .... import _lib as L
from .... import functional as Fn
from ....engine import ParamStore
from .ddim import DDIMSchedule

LN_EPS = 1e-5           # nn.LayerNorm's default, which the reference's MLPResNet uses throughout
NUM_BLOCKS = 2          # L1RegressionActionHead builds MLPResNet(num_blocks=2, ...) (:143-145)


class ProprioProjector(nn.Module):
    """proprio state [B, proprio_dim] -> one row of the LLM's width per sample"""

    def __init__(self, store: ParamStore, prefix: str, llm_dim: int, proprio_dim: int):
        super().__init__()
        self.store, self.p, self.llm_dim, self.proprio_dim = store, prefix, llm_dim, proprio_dim
        store.register([(prefix + "fc1.weight", (llm_dim, proprio_dim)), (prefix + "fc1.bias", (llm_dim,))])
        store.register([(prefix + "fc2.weight", (llm_dim, llm_dim)), (prefix + "fc2.bias", (llm_dim,))])

    def forward(self, proprio: torch.Tensor) -> torch.Tensor:
        st, p = self.store, self.p
        x = proprio.to(device=st.device, dtype=st.compute_dtype).reshape(-1, self.proprio_dim).contiguous()
        return Fn.MlpFn.apply(x, st.params[p + "fc1.weight"], st, p + "fc1.weight", p + "fc1.bias", p + "fc2.weight", p + "fc2.bias",
                              L.ACT_GELU_ERF)


class MLPResNet(nn.Module):
    """the head's trunk.  ``forward`` takes the decoder output and the per-sample offsets: layer_norm1 reads its rows in place"""

    def __init__(self, store: ParamStore, prefix: str, num_blocks: int, input_dim: int, hidden_dim: int, output_dim: int):
        super().__init__()
        self.store, self.p, self.num_blocks = store, prefix, num_blocks
        self.input_dim, self.hidden_dim, self.output_dim = input_dim, hidden_dim, output_dim
        store.register([(prefix + "layer_norm1.weight", (input_dim,)), (prefix + "layer_norm1.bias", (input_dim,))], layernorm=True)
        store.register([(prefix + "fc1.weight", (hidden_dim, input_dim)), (prefix + "fc1.bias", (hidden_dim,))])
        for i in range(num_blocks):
            b = f"{prefix}mlp_resnet_blocks.{i}.ffn."
            store.register([(b + "0.weight", (hidden_dim,)), (b + "0.bias", (hidden_dim,))], layernorm=True)
            store.register([(b + "1.weight", (hidden_dim, hidden_dim)), (b + "1.bias", (hidden_dim,))])
        store.register([(prefix + "layer_norm2.weight", (hidden_dim,)), (prefix + "layer_norm2.bias", (hidden_dim,))], layernorm=True)
        store.register([(prefix + "fc2.weight", (output_dim, hidden_dim)), (prefix + "fc2.bias", (output_dim,))])

    def forward(self, hidden: torch.Tensor, off: torch.Tensor, T: int, A: int, skip: bool) -> torch.Tensor:
        """hidden [B, Sq, d], off [B] int64 (first row of each sample's block) -> [B T, output_dim]"""
        st, p = self.store, self.p
        anchor = st.params[p + "fc1.weight"]
        x = Fn.ActionNormFn.apply(hidden, anchor, st, p + "layer_norm1.weight", p + "layer_norm1.bias", off, T, A, skip, LN_EPS)
        x = Fn.LinearFn.apply(x, anchor, st, p + "fc1.weight", p + "fc1.bias", L.ACT_RELU, None)
        for i in range(self.num_blocks):
            b = f"{p}mlp_resnet_blocks.{i}.ffn."
            x = Fn.ResidualLinearFn.apply(x, anchor, st, b + "0.weight", b + "0.bias", b + "1.weight", b + "1.bias", L.ACT_RELU, LN_EPS)
        x = Fn.NormFn.apply(x, anchor, st, "ln", p + "layer_norm2.weight", p + "layer_norm2.bias", LN_EPS)
        return Fn.LinearFn.apply(x, anchor, st, p + "fc2.weight", p + "fc2.bias", L.ACT_NONE, None)


class DiscreteActionHead(nn.Module):
    """discrete actions read off the LLM's own vocabulary (model.py:273-347): no parameters except the optional
    ``proprio_projector``.  ``action_query`` is ``torch.ones(1, T A)`` — token ids, not a parameter and not in the state dict: every
    query row is the embedding row of token ``QUERY_TOKEN``.  Bin b of ``num_bins`` stands for the action b / (num_bins - 1) * 2 - 1;
    the decoders read the LAST num_bins - 1 vocabulary logits (oft_discrete_arch.py:222-224)."""

    QUERY_TOKEN = 1

    def __init__(self, store: ParamStore, prefix: str, input_dim: int, vocab_size: int, action_dim: int, action_chunk: int,
                 num_bins: int = 256, use_proprio: bool = False, proprio_dim: Optional[int] = None):
        super().__init__()
        self.store, self.p = store, prefix
        self.input_dim, self.vocab_size, self.action_dim, self.action_chunk = input_dim, vocab_size, action_dim, action_chunk
        self.num_bins, self.use_proprio = int(num_bins), bool(use_proprio)
        self.action_query = torch.ones(1, action_chunk * action_dim)
        self.proprio_projector = None
        if use_proprio:
            if not proprio_dim:
                raise ValueError("OFT: use_proprio=True needs config.proprio_dim")
            store.new_bucket()
            self.proprio_projector = ProprioProjector(store, prefix + "proprio_projector.", input_dim, int(proprio_dim))

    @property
    def num_query_rows(self) -> int:
        return self.action_chunk * self.action_dim

    def discretize_actions(self, actions: torch.Tensor) -> torch.Tensor:
        """[B, T, A] in [-1, 1] (clipped) -> bin indices in [0, num_bins - 1]"""
        actions = torch.clamp(actions, -1, 1)
        return ((actions + 1) / 2 * (self.num_bins - 1)).round().long()

    def continuous_to_discrete_tokens(self, actions: torch.Tensor) -> torch.Tensor:
        """[B, T, A] -> [B, T A] bin indices"""
        discrete = self.discretize_actions(actions)
        return discrete.reshape(discrete.size(0), -1)

    def discrete_tokens_to_continuous(self, token_ids) -> torch.Tensor:
        """[B, T A] bin indices, or a text string holding them -> [B, T, A] actions in [-1, 1]"""
        if isinstance(token_ids, str):
            found = re.findall(r"\d+", token_ids)[: self.action_chunk * self.action_dim]
            actions = np.array([int(a) for a in found], dtype=np.float32).reshape(1, self.action_chunk, self.action_dim)
            actions = torch.from_numpy(actions)
        else:
            actions = token_ids.reshape(token_ids.size(0), self.action_chunk, self.action_dim).float()
        return (actions / (self.num_bins - 1)) * 2 - 1


class NoisePredictionModel(nn.Module):
    """the diffusion head's trunk (model.py:163-194): the same ``MLPResNet``, under ``mlp_resnet``"""

    def __init__(self, store: ParamStore, prefix: str, transformer_hidden_dim: int, hidden_dim: int, action_dim: int):
        super().__init__()
        self.mlp_resnet = MLPResNet(store, prefix + "mlp_resnet.", NUM_BLOCKS, transformer_hidden_dim, hidden_dim, action_dim)


class DiffusionActionHead(nn.Module):
    """continuous actions by conditional denoising diffusion (model.py:197-271): every noisy action component becomes one row
    (``noisy_action_projector``: Linear(1, d) -> GELU(erf) -> Linear(d, d)), a sinusoidal time row stands in front of them, and the
    MLP-ResNet reads the T A hidden rows behind the time row as T rows of A d columns and predicts the noise.  No ``action_query``;
    the scheduler (ddim.DDIMSchedule) and the time encoder hold no parameters."""

    def __init__(self, store: ParamStore, prefix: str, input_dim: int, hidden_dim: int, action_dim: int, action_chunk: int,
                 num_diffusion_steps: int = 100, use_proprio: bool = False, proprio_dim: Optional[int] = None):
        super().__init__()
        if hidden_dim % 2 != 0 or hidden_dim < 4:
            raise ValueError(f"OFT: the time encoder needs an even width of at least 4, got {hidden_dim}")
        if input_dim % 8 != 0 or input_dim != hidden_dim:
            raise ValueError(f"OFT: the diffusion head's row kernels need the LLM width as a multiple of 8 (and the time row is as wide "
                             f"as the LLM), got {input_dim} / {hidden_dim}")
        self.store, self.p = store, prefix
        self.input_dim, self.action_dim, self.action_chunk = input_dim, action_dim, action_chunk
        self.num_diffusion_steps = int(num_diffusion_steps)
        self.noise_scheduler = DDIMSchedule(self.num_diffusion_steps)
        store.new_bucket()
        # registration order = the order the forward first uses them (the DP reducer walks the buckets backwards)
        pp = prefix + "noisy_action_projector."
        store.register([(pp + "fc1.weight", (input_dim, 1)), (pp + "fc1.bias", (input_dim,))])
        store.register([(pp + "fc2.weight", (input_dim, input_dim)), (pp + "fc2.bias", (input_dim,))])
        self.proprio_projector = None
        if use_proprio:
            if not proprio_dim:
                raise ValueError("OFT: use_proprio=True needs config.proprio_dim")
            self.proprio_projector = ProprioProjector(store, prefix + "proprio_projector.", input_dim, int(proprio_dim))
        self.noise_predictor = NoisePredictionModel(store, prefix + "noise_predictor.", input_dim * action_dim, hidden_dim, action_dim)
        self._time_tables = {}
        # the state dict lists the head in the reference's module order: trunk, projector, proprio projector
        self.noisy_action_projector = nn.Module()            # parameter container (engine.attach_parameters fills it)
        for k in ("noise_predictor", "noisy_action_projector", "proprio_projector"):
            if k in self._modules:
                self._modules[k] = self._modules.pop(k)

    @property
    def num_query_rows(self) -> int:
        """rows of a sample's block behind the optional state row: the time row and the T A noisy-action rows"""
        return self.action_chunk * self.action_dim + 1

    def time_table(self, device) -> torch.Tensor:
        """``SinusoidalPositionalEncoding`` (model.py:57-80) of every training timestep 0 ... N - 1, [N, d] fp32: built once with
        the reference's own torch ops on the host (so row t has the bits the reference computes for timestep t), kept per device"""
        key = str(device)
        if key not in self._time_tables:
            half = self.input_dim // 2
            exponent = torch.arange(half) * -math.log(10000) / (half - 1)
            emb = torch.arange(self.num_diffusion_steps)[:, None] * torch.exp(exponent)[None, :]
            self._time_tables[key] = torch.cat((emb.sin(), emb.cos()), dim=-1).to(device)
        return self._time_tables[key]

    def time_encoder(self, timesteps) -> torch.Tensor:
        """timesteps [B] (integers in [0, N), tensor or list) -> [B, d] fp32 on the model's device: rows of ``time_table``"""
        dev = self.store.device
        idx = torch.as_tensor(timesteps).to(device=dev, dtype=torch.int64).reshape(-1)
        return self.time_table(dev).index_select(0, idx)

    def sample_noisy_actions(self, actions: torch.Tensor, generator: Optional[torch.Generator] = None) -> dict:
        """the reference's draw (model.py:227-257): ``noise`` ~ N(0, 1) [B, T, A], one timestep in [0, N) per sample,
        ``noisy_actions`` = add_noise, ``diffusion_timestep_embeddings`` [B, 1, d]; all fp32 on the model's device.  ``generator``
        (on its own device) makes the draw reproducible."""
        dev = self.store.device
        actions = actions.to(device=dev, dtype=torch.float32)
        B = actions.shape[0]
        gdev = generator.device if generator is not None else dev
        noise = torch.randn((B, self.action_chunk, self.action_dim), generator=generator, device=gdev, dtype=torch.float32).to(dev)
        timesteps = torch.randint(0, self.num_diffusion_steps, (B,), generator=generator, device=gdev).to(dev)
        noisy = self.noise_scheduler.add_noise(actions.reshape(B, self.action_chunk, self.action_dim), noise, timesteps)
        return dict(noise=noise, noisy_actions=noisy, diffusion_timestep_embeddings=self.time_encoder(timesteps).unsqueeze(1))

    def project_noisy_actions(self, noisy_actions: torch.Tensor) -> torch.Tensor:
        """[B, T, A] fp32 -> the [B T A, d] projected rows: fc1 + GELU in one launch, fc2 as a product with a bias epilogue"""
        st, p = self.store, self.p + "noisy_action_projector."
        anchor = st.params[p + "fc2.weight"]
        h = Fn.NoisyEmbedFn.apply(noisy_actions.to(device=st.device, dtype=torch.float32), anchor, st, p + "fc1.weight", p + "fc1.bias")
        return Fn.LinearFn.apply(h, anchor, st, p + "fc2.weight", p + "fc2.bias", L.ACT_NONE, None)

    def predict_noise(self, hidden: torch.Tensor, off: torch.Tensor, skip: int = 1) -> torch.Tensor:
        """decoder output [B, Sq, d] -> predicted noise [B, T, A].  ``off`` [B]: the row ``skip`` rows in front of each sample's
        noisy-action rows, ``skip`` in {0, 1}: the head's LayerNorm kernel takes no more, so with a state row the caller hands in the
        TIME row's offset and skip = 1 (``OFTDiffusionModel.time_offsets``), not the block's first row and skip = 2."""
        B = hidden.shape[0]
        out = self.noise_predictor.mlp_resnet(hidden, off, self.action_chunk, self.action_dim, bool(skip))
        return out.view(B, self.action_chunk, self.action_dim)


class L1RegressionActionHead(nn.Module):
    """continuous actions by L1 regression: T A learned query rows in, one MLP-ResNet row per time step out"""

    def __init__(self, store: ParamStore, prefix: str, input_dim: int, hidden_dim: int, action_dim: int, action_chunk: int,
                 use_proprio: bool = False, proprio_dim: Optional[int] = None):
        super().__init__()
        self.store, self.p = store, prefix
        self.input_dim, self.action_dim, self.action_chunk = input_dim, action_dim, action_chunk
        store.new_bucket()
        # registration order = the order the forward first uses them (the DP reducer walks the buckets backwards)
        store.register([(prefix + "action_query", (1, action_chunk * action_dim, input_dim))])
        self.proprio_projector = None
        if use_proprio:
            if not proprio_dim:
                raise ValueError("OFT: use_proprio=True needs config.proprio_dim")
            self.proprio_projector = ProprioProjector(store, prefix + "proprio_projector.", input_dim, int(proprio_dim))
        self.model = MLPResNet(store, prefix + "model.", NUM_BLOCKS, input_dim * action_dim, hidden_dim, action_dim)

    @property
    def query_name(self) -> str:
        return self.p + "action_query"

    @property
    def num_query_rows(self) -> int:
        return self.action_chunk * self.action_dim

    def predict_action(self, hidden: torch.Tensor, off: torch.Tensor, skip: bool) -> torch.Tensor:
        """decoder output [B, Sq, d] + block offsets -> predicted actions [B, T, A] (model.py:151-160 on the rows in place)"""
        B = hidden.shape[0]
        out = self.model(hidden, off, self.action_chunk, self.action_dim, skip)
        return out.view(B, self.action_chunk, self.action_dim)
