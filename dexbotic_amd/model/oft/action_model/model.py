"""Action heads of the OFT policy: host-side mirror of dexbotic/model/oft/action_model/model.py on libdexbotic_amd kernels.

``L1RegressionActionHead`` (:129-160): ``action_query`` [1, T A, d], the learned rows placed behind every sample's prompt, and an
``MLPResNet`` (:104-126) that reads the A hidden rows of one time step as ONE row of A d columns: layer_norm1 -> fc1 -> ReLU -> two
``MLPResNetBlock`` (:83-101, LayerNorm -> Linear -> ReLU, plus the skip) -> layer_norm2 -> fc2.  ``ProprioProjector`` (:12-30):
fc1 -> GELU(erf) -> fc2.  ``DiscreteActionHead`` (:273-347): no trunk at all — the LLM's vocabulary is the head; it carries the bin
<-> action helpers and the optional projector.  Parameter names as in the reference's modules.  The products run in the compute dtype (the reference runs
them under autocast), the LayerNorm statistics in fp32.
"""
from __future__ import annotations

import re
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from .... import _lib as L
from .... import functional as Fn
from ....engine import ParamStore

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
