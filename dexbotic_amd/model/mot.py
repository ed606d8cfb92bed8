"""What the dual-expert policies (pi0, pi0.5, DM0) share around ``functional.MotLayerFn``: the block mask as the kernels take it, the
loop over the layers, and the sampler's scaffolding (per-layer key / value buffers, the float32 time schedule, the graph-or-eager
tail).  What differs between the policies — the masks' cumulative sums, the final norm, where the schedule stops, pi0's state token
— stays with each policy."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib as L
from .. import functional as Fn
from .. import hostcpu


def mask_tensors(q_cum: np.ndarray, q_valid: np.ndarray, k_cum: np.ndarray, k_valid: np.ndarray, device):
    """block mask (pi0_arch.py:22-28) as the kernels take it: q_limit[b,i] = #keys with cumsum <= the query's
    (keys are ordered, cumsum non-decreasing), key_valid[b,j] = input_mask.  Invalid queries get limit 0."""
    lim = (k_cum[:, None, :] <= q_cum[:, :, None]).sum(-1).astype(np.int32)
    lim[~q_valid] = 0
    return hostcpu.upload(lim, device), hostcpu.upload(k_valid.astype(np.uint8), device)


def flow_times(dt: float):
    """the references' float32 time accumulation 1, 1 + dt, 1 + dt + dt, ... (pi0_arch.py:470-489); where it stops is the caller's"""
    time = np.float32(1.0)
    while True:
        yield time
        time = np.float32(time + np.float32(dt))


class MotPolicy:
    """mixin of a policy with ``self.store``, ``self.config.llm_config`` and the two experts ``self.model.llm`` /
    ``self.model.action_expert`` (``layer_specs`` per layer, the llm's ``rope_tables``)"""

    def _lin(self, x, n: str, act=L.ACT_NONE):
        """one of the policy's small linears ``model.<n>``"""
        st = self.store
        return Fn.LinearFn.apply(x, st.params[f"model.{n}.weight"], st, f"model.{n}.weight", f"model.{n}.bias", act, None)

    def _v_t(self, suf: torch.Tensor) -> torch.Tensor:
        """action_out_proj of the last ``chunk_size`` suffix outputs -> the flow's velocity [B, chunk, A] fp32"""
        B, n = suf.shape[0], self.config.chunk_size
        return self._lin(suf[:, -n:].reshape(B * n, -1).contiguous(), "action_out_proj").view(B, n, -1).float()

    def _geom(self, B: int, S0: int, S1: int):
        c = self.config.llm_config
        return (B, S0, S1, c.num_attention_heads, c.num_key_value_heads, c.head_dim)

    def _mot_layers(self, geom, x0, x1, mods, cos_t, sin_t, pos0, pos1, q_limit, key_valid, kv=None, kv0: int = 0):
        """every layer of the mixture on the experts' rows x0 [B * S0, d] / x1 [B * S1, d_a] -> (x0, x1): one MotLayerFn per layer,
        through autograd when gradients are on, its ``_run`` alone otherwise (the same launches: the same bits).  An expert whose
        rows are None is left out (the sampler's prefix pass: the llm alone; its Euler steps: the action expert alone, with the
        per-layer buffers ``kv`` written from slot ``kv0``).  ``mods`` [2 L + 1, B, 3 d_a]: pi0.5's modulations.  The last layer's
        llm half after attention is never computed (nothing reads prefix_out): x0 comes back without it."""
        llm, exp = self.model.llm, self.model.action_expert
        n = llm.config.num_hidden_layers
        for li in range(n):
            sps = (llm.layer_specs[li] if x0 is not None else None, exp.layer_specs[li] if x1 is not None else None)
            mod1, mod2 = (None, None) if mods is None else (mods[2 * li], mods[2 * li + 1])
            x0, x1 = Fn.mot_layer(self.store, sps, geom, li == n - 1, x0, x1, mod1, mod2, cos_t, sin_t, pos0, pos1, q_limit,
                                  key_valid, kv=None if kv is None else kv[li], kv0=kv0)
        return x0, x1

    def _mot_rows(self, ptok, stok, positions: np.ndarray, q_limit, key_valid, mods=None) -> torch.Tensor:
        """the mixture over both experts, prefix tokens ptok [B, P, d] and suffix tokens stok [B, Sx, d_a] at the RoPE rows
        ``positions`` [B, P + Sx] -> the action expert's rows [B * Sx, d_a] BEFORE its final norm (the policy's own)"""
        B, P, Sx = ptok.shape[0], ptok.shape[1], stok.shape[1]
        dev = self.store.device
        cos_t, sin_t = self.model.llm.rope_tables(int(positions.max()) + 1, dev)
        pos0 = hostcpu.upload(positions[:, :P].astype(np.int32), dev).reshape(-1)
        pos1 = hostcpu.upload(positions[:, P:].astype(np.int32), dev).reshape(-1)
        x0 = ptok.reshape(B * P, -1).contiguous()
        x1 = stok.reshape(B * Sx, -1).contiguous()
        return self._mot_layers(self._geom(B, P, Sx), x0, x1, mods, cos_t, sin_t, pos0, pos1, q_limit, key_valid)[1]

    def sampler_kv_buffers(self, B: int, cap: int):
        """the sampler's per-layer (k, v) [B, Hkv, cap = P + suffix, D] buffers for this shape: allocated once and kept (a captured
        graph holds their addresses), filled by the prefix pass and by every Euler step"""
        c, st = self.config.llm_config, self.store
        pool = self.__dict__.setdefault("_sampler_kv", {})
        key = (B, cap, st.compute_dtype)
        if key not in pool:
            if len(pool) >= 8:
                pool.pop(next(iter(pool)))
            shape = (B, c.num_key_value_heads, cap, c.head_dim)
            pool[key] = [(torch.empty(shape, device=st.device, dtype=st.compute_dtype),
                          torch.empty(shape, device=st.device, dtype=st.compute_dtype)) for _ in range(c.num_hidden_layers)]
        return pool[key]

    def _run_sampler(self, euler, inputs: dict, key: tuple, use_graph=None) -> torch.Tensor:
        """the Euler loop ``euler(**inputs)``, tensors in / tensors out: replayed as ONE HIP graph per ``key`` (graphs.GraphCache)
        or run launch by launch.  The key / value buffers are not inputs (inputs are copied into the graph's own memory): the graph
        reads and writes them where they are, so their address belongs in ``key``.  A weight change needs no new capture: the graph
        reads the arena in place and the prefix pass — host code — has already brought the bf16 shadows up to date; only the fp32
        (1 + w) of Gemma norms are tensors of their own, refreshed here."""
        from .. import graphs
        dev = self.store.device
        if dev.type == "cuda" and (graphs.enabled() if use_graph is None else use_graph):
            cache = self.__dict__.setdefault("_sampler_graphs", graphs.GraphCache(dev))
            Fn.gemma_norm_refresh(self.store)
            return cache.run(key, euler, inputs).clone()
        return euler(**inputs)
