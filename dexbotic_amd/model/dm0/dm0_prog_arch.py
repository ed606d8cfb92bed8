"""DM0-prog policy: DM0 at inference time with one extra suffix token that carries the task progress; host-side mirror of
dexbotic/model/dm0/dm0_prog_arch.py on libdexbotic_amd kernels.

``DM0ProgConfig`` (:35-60), ``DM0ProgModel`` (:63-97: DM0's modules + ``progress_in_proj`` Linear(1, d_a) / ``progress_out_proj``
Linear(d_a, 1)), ``DM0ProgForCausalLM.inference_action`` (:418-576).  What differs from model/dm0/dm0_arch.py:

* with ``progress`` the suffix is ``1 + chunk_size`` rows: the embedded progress in front of the action rows.  The reference's
  ``attn_mask`` is still [1, 0, 0, ...], so the whole suffix is one bidirectional block (cumsum P + 1) whose positions follow the
  prefix; the key / value buffers are [B, Hkv, P + 1 + chunk, D];
* every Euler step also reads ``progress_out_proj`` of the progress row's output; the request returns the action chunk and the
  minimum of those predictions over the steps, [B, 1, 1];
* the two ends of a step are ONE launch each: ``dxa_flow_suffix_in`` (action_in_proj, progress_in_proj and the time-embedding half of
  the input of ``action_time_mlp_in``) and ``dxa_flow_euler_tail`` (final norm, action_out_proj, the Euler update in place,
  progress_out_proj and the running minimum), with p = 0 progress rows when no progress is given.  The tail keeps the normalised row
  and the velocity in fp32, one rounding fewer than DM0's composed sequence;
* the sampler state is ONE fp32 tensor [B, chunk * A + 1] (the sample, then the running minimum): ``MotPolicy._run_sampler`` and
  ``graphs.GraphCache`` carry one tensor, and ``progress`` is an input of the looped function, so a replay takes a new value
  without a new capture;
* no ``forward``: the reference class is inference-only (it defines no flow-matching step, and its progress projections never see a
  gradient), so training raises ``NotImplementedError`` here instead of silently inheriting DM0's step.
"""
from __future__ import annotations

import torch

from ... import kernels as K
from ... import _lib as L
from ..dexbotic_arch import register_model_with_hf, register_with_hf
from .dm0_arch import DM0Config, DM0ForCausalLM, DM0Model


class DM0ProgConfig(DM0Config):
    """dm0_prog_arch.py:35-60: DM0's fields under the reference's ``model_type``"""
    model_type = "dexbotic_dm0_prog"

    def __init__(self, **kwargs):          # (transformers generates an empty __init__ for a config class that defines none)
        super().__init__(**kwargs)


register_with_hf(DM0ProgConfig)


class DM0ProgModel(DM0Model):
    """DM0's registration order, then the two progress projections (the reference's module order)"""

    def __init__(self, config: DM0ProgConfig, store):
        super().__init__(config, store)
        da = config.action_config.hidden_size
        store.new_bucket()
        for name, shape in (("progress_in_proj", (da, 1)), ("progress_out_proj", (1, da))):
            store.register([(f"model.{name}.weight", shape), (f"model.{name}.bias", (shape[0],))])


def _begin_progress(progress, B: int):
    """``progress`` [B, 1] or [B, 1, 1] -> fp32 [B, 1] on the host side of the call; the reference unsqueezes a 2-D tensor and leaves
    ``begin_progress`` None for any other rank, which then dies on an empty ``torch.stack`` (:436-441, :503)"""
    if not torch.is_tensor(progress):
        progress = torch.as_tensor(progress)
    if progress.dim() not in (2, 3) or progress.numel() != B:
        raise ValueError(f"DM0-prog: progress must be [B, 1] or [B, 1, 1] with B = {B}, got shape {tuple(progress.shape)}")
    return progress.reshape(B, 1)


class DM0ProgForCausalLM(DM0ForCausalLM):
    config_class = DM0ProgConfig

    def _real_init(self, config):
        self.model = DM0ProgModel(config, self.store)
        self.store.new_bucket()
        self.store.register([("lm_head.weight", (config.llm_config.vocab_size, config.llm_config.hidden_size))])

    def forward(self, *args, **kwargs):
        raise NotImplementedError("DM0ProgForCausalLM is inference-only, as the reference class is: it defines no flow-matching "
                                  "forward and its progress projections never see a gradient; train a DM0ForCausalLM")

    @torch.no_grad()
    def inference_action(self, input_ids=None, attention_mask=None, states=None, images=None, image_masks=None, progress=None,
                         diffusion_steps: int = 10, **kwargs):
        """dm0_prog_arch.py:418-576.  ``progress`` [B, 1] or [B, 1, 1]: the task progress the caller believes it is at.  kwarg
        ``noise`` [B, chunk, A] injects the initial sample, ``use_graph`` overrides the graph switch.  Returns the [B, chunk, A]
        tensor, or with ``progress`` the pair (actions, end_progress [B, 1, 1] fp32: the minimum over the Euler steps of the
        predicted end-of-chunk progress)."""
        c, st = self.config, self.store
        dev = st.device
        B, n, A = states.shape[0], c.chunk_size, c.action_dim
        p = 0 if progress is None else 1
        if p:
            progress = _begin_progress(progress, B)
        noise = kwargs.get("noise")
        state = torch.empty((B, n * A + 1), device=dev, dtype=torch.float32)        # the sample, then the running minimum
        state[:, :n * A] = (torch.randn(B, n * A, device=dev) if noise is None else noise.to(dev).float().reshape(B, n * A))
        pl =self._sampler_plan(attention_mask, image_masks, B, p + n, diffusion_steps)
        self._prefix_pass(pl, input_ids, images)
        P, dt, kv, cos_t, sin_t = pl.P, pl.dt, pl.kv, pl.cos_t, pl.sin_t
        exp = self.model.action_expert
        eps = exp.config.rms_norm_eps

        def w(name):
            return st.w(f"model.{name}.weight"), st.w(f"model.{name}.bias")

        # ---- the Euler loop: tensors in / tensors out; the suffix keys / values go to [P, P + p + chunk) of the buffers
        def euler(state, te_table, q_limit, key_valid, pos, progress=None):
            x, pm = state[:, :n * A], state[:, n * A:]
            w_in, b_in = w("action_in_proj")
            w_out, b_out = w("action_out_proj")
            w_p, b_p = w("progress_in_proj") if p else (None, None)
            w_q, b_q = w("progress_out_proj") if p else (None, None)
            g = st.w(exp.p + "norm.weight")
            pm.fill_(float("inf"))
            for s in range(pl.steps):
                h = K.flow_suffix_in(x, te_table[s], w_in, b_in, n, A, progress, w_p, b_p)
                h = self._lin(self._lin(h, "action_time_mlp_in", L.ACT_SILU), "action_time_mlp_out")
                _, h = self._mot_layers(pl.geom_s, None, h, None, cos_t, sin_t, None, pos, q_limit, key_valid, kv=kv, kv0=P)
                K.flow_euler_tail_(h.contiguous(), g, w_out, b_out, x, n, eps, dt, pm if p else None, w_q, b_q)
            return state
        inputs = dict(state=state, te_table=pl.te_table, q_limit=pl.q_limit, key_valid=pl.key_valid, pos=pl.pos)
        if p:
            inputs["progress"] = progress.to(device=dev, dtype=torch.float32).contiguous()
        key = ("euler-prog", p, int(diffusion_steps), P, cos_t.data_ptr(), kv[0][0].data_ptr())
        out = self._run_sampler(euler, inputs, key, kwargs.get("use_graph"))
        acts = out[:, :n * A].reshape(B, n, A).contiguous()
        return (acts, out[:, n * A:].reshape(B, 1, 1).clone()) if p else acts


register_model_with_hf(DM0ProgForCausalLM)
