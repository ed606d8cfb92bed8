"""Generate tests/golden/dm0_t1.npz by running the REFERENCE's DM0ForCausalLM on the CPU.

TEST INFRASTRUCTURE, CPU only.  Needs the reference tree next to this repository's build container (oracle/gen_golden.py: REF); the
fixture it writes is committed, so no test reads the reference.

    python scripts/gen_golden_dm0.py            # from the repository root

Pinned: a tiny DM0 — CLIP tower 64 wide, 2 layers, 28 px / patch 14 (4 tokens per camera); Qwen3 llm d 96, F 128, 4 q / 2 kv heads
x 32, 3 layers (so one llm layer both receives and passes on gradient); action expert d 64, F 80, the same attention geometry;
``bf16=False`` — on a batch of 2 samples x 3 cameras, camera 1 of sample 1 masked out, 7 text tokens, sample 1 right-padded by 2,
chunk_size 6, action_dim 8.  Recorded: the inputs, the injected ``noise`` / ``time``, ``loss``, ``v_t``, every gradient norm
(``gradN/``; the two that are exactly zero included), a handful of gradients in full (``grad/``), the parameters whose gradient is
None, the ordered key / shape list of the state dict, and ``init_noise`` / ``infer_actions`` of the 10-step Euler sampler.
The weights and the images are NOT stored: tests/muvla_weights.py regenerates them from the seed and the ordered key / shape list,
and the archive keeps per-tensor checksums.

How the draws are pinned without editing the reference: ``forward`` and ``inference_action`` draw their noise / time with the global
torch generator; the script seeds it, makes the same calls itself, seeds it again and calls the reference.  The forward's pair is
verified through ``mse(v_t, noise - actions) == loss``, the sampler's through the recompute loop below.

The sampler: the reference's ``inference_action`` does not run under this transformers — ``_compute_merged_layer`` reads
``past_key_values.key_cache`` / ``.value_cache``, which ``DynamicCache`` no longer has, so the cached prefix is silently not
concatenated and the mask shapes clash.  ``dm0_arch.DynamicCache`` is replaced FROM HERE by a ten-line object with those two lists
and an ``update`` that appends and returns its arguments; with it the reference's own sampler runs.  Its result is asserted equal
(max abs difference 0.0) to a full-recompute loop built from the reference's own pieces (``get_prefix_hidden_states``,
``get_suffix_hidden_states``, ``make_attn_mask_2d`` / ``_4d``, ``_merged_attention_forward(past_key_values=None, use_cache=False)``
per step).

bf16: the reference is also built with ``bf16=True`` (llm / expert / tower / projector in bf16, the norm gains kept fp32) and run on
the same batch on the CPU.  It runs (loss 1.38688 against 1.38766 in fp32); its ``loss`` / ``v_t`` are recorded as ``bf16/loss`` /
``bf16/v_t``.  Should it stop running under another transformers, the script prints the exception and records nothing under ``bf16/``.
Shims: the timm stub of oracle/gen_golden.py (imported, not edited), locally saved tiny CLIP / Qwen3 directories.
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

SEED = 41
VOCAB, HIDDEN, INTER, LAYERS, HEADS, KV_HEADS, HEAD_DIM = 264, 96, 128, 3, 4, 2, 32
A_HIDDEN, A_INTER = 64, 80
V_HIDDEN, V_INTER, V_LAYERS, V_HEADS, V_IMAGE, V_PATCH = 64, 128, 2, 2, 28, 14
B, CAMS, L_TXT, CHUNK, ADIM, STEPS = 2, 3, 7, 6, 8, 10
FULL_GRADS = ("model.llm.layers.1.self_attn.q_norm.weight", "model.llm.layers.2.self_attn.k_norm.weight",
              "model.action_expert.model.layers.0.self_attn.q_norm.weight", "model.action_expert.model.layers.2.self_attn.k_norm.weight",
              "model.llm.layers.1.self_attn.k_proj.weight", "model.action_expert.model.layers.1.self_attn.q_proj.weight",
              "model.action_time_mlp_in.weight", "model.llm.layers.0.input_layernorm.weight")


class ListCache:
    """what dm0_arch._compute_merged_layer expects of its cache (module docstring)"""

    def __init__(self):
        self.key_cache, self.value_cache = [], []

    def update(self, k, v, layer_idx, *a, **kw):
        self.key_cache.append(k)
        self.value_cache.append(v)
        return k, v


def recompute_sampler(m, U, ids, mask, images, image_masks, x, steps):
    """the Euler loop without a cache, from the reference's own pieces"""
    dt = -1.0 / steps
    time = torch.tensor(1.0, dtype=x.dtype)
    ph, ppad, patt = m.get_prefix_hidden_states(ids, mask, images, image_masks)
    mods = [m.model.llm, m.model.action_expert.model]
    while time >= -dt / 2:
        sh, spad, satt = m.get_suffix_hidden_states(x, time.broadcast_to(x.shape[0]))
        pad, att = torch.cat([ppad, spad], dim=1), torch.cat([patt, satt], dim=1)
        m4 = U.make_attn_mask_4d(U.make_attn_mask_2d(padding_mask=pad, attn_mask=att), dtype=ph.dtype)
        ppos = torch.cumsum(ppad, dim=1) - 1
        spos = torch.sum(ppad, dim=-1)[:, None] + torch.cumsum(spad, dim=1) - 1
        (_, so), _ = m._merged_attention_forward(module_list=mods, attention_mask=m4, position_ids=torch.cat([ppos, spos], dim=1),
                                                 past_key_values=None, input_embeds_list=[ph, sh], use_cache=False)
        v_t = m.model.action_out_proj(so[:, -m.model.config.chunk_size:])
        x, time = x + v_t * dt, time + dt
    return x


def tiny_dirs():
    """locally saved tiny CLIP / Qwen3 llm / Qwen3 action-expert directories (module docstring: Pinned) -> their three paths"""
    from transformers import CLIPImageProcessor, CLIPVisionConfig, CLIPVisionModel, Qwen3Config
    tmp = tempfile.mkdtemp()
    d_clip, d_llm, d_act = (os.path.join(tmp, n) for n in ("tiny_clip", "tiny_qwen3", "tiny_qwen3_action"))
    vcfg = CLIPVisionConfig(hidden_size=V_HIDDEN, intermediate_size=V_INTER, num_hidden_layers=V_LAYERS,
                            num_attention_heads=V_HEADS, image_size=V_IMAGE, patch_size=V_PATCH)
    CLIPVisionModel(vcfg).save_pretrained(d_clip)
    CLIPImageProcessor(size={"shortest_edge": V_IMAGE}, crop_size={"height": V_IMAGE, "width": V_IMAGE}).save_pretrained(d_clip)
    q3 = dict(vocab_size=VOCAB, num_hidden_layers=LAYERS, num_attention_heads=HEADS, num_key_value_heads=KV_HEADS,
              head_dim=HEAD_DIM, max_position_embeddings=4096, rope_theta=1e6, rms_norm_eps=1e-6, tie_word_embeddings=False,
              attention_bias=False)
    Qwen3Config(hidden_size=HIDDEN, intermediate_size=INTER, **q3).save_pretrained(d_llm)
    Qwen3Config(hidden_size=A_HIDDEN, intermediate_size=A_INTER, **q3).save_pretrained(d_act)
    return d_clip, d_llm, d_act


def main():
    from oracle.gen_golden import GOLD, REF, install_timm_shim
    from tests.muvla_weights import checksums, make_images, make_weights, pack_shapes
    sys.path.insert(0, REF)
    install_timm_shim()
    from dexbotic.model.dm0 import dm0_arch as arch
    from dexbotic.model.dm0 import dm0_utils as U

    torch.manual_seed(SEED)
    d_clip, d_llm, d_act = tiny_dirs()

    def build(bf16):
        cfg = arch.DM0Config(llm_config=d_llm, action_config=d_act, mm_vision_tower=d_clip, mm_projector_type="mlp2x_gelu",
                             action_dim=ADIM, chunk_size=CHUNK, bf16=bf16)
        return arch.DM0ForCausalLM(cfg)

    m = build(False)
    keys = list(m.state_dict().keys())
    shapes = [tuple(v.shape) for v in m.state_dict().values()]
    w = make_weights(keys, shapes, SEED)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    for p_ in m.parameters():
        p_.requires_grad = True
    n_par = sum(int(np.prod(s)) for s in shapes)

    rs = np.random.RandomState(SEED + 2)
    ids = rs.randint(10, 250, size=(B, L_TXT)).astype(np.int64)
    mask = np.ones((B, L_TXT), dtype=bool)
    mask[1, L_TXT - 2:] = False                  # sample 1: right-padded by 2
    image_masks = np.ones((B, CAMS), dtype=bool)
    image_masks[1, 1] = False                    # camera 1 of sample 1 masked out: a hole in the middle of the prefix
    image_shape = (B, CAMS, 3, V_IMAGE, V_IMAGE)
    images = make_images(image_shape, SEED)
    actions = rs.uniform(-1, 1, size=(B, CHUNK, ADIM)).astype(np.float32)
    states = rs.uniform(-1, 1, size=(B, ADIM)).astype(np.float32)
    t = torch.from_numpy
    kw = dict(input_ids=t(ids), attention_mask=t(mask), images=t(images), image_masks=t(image_masks))

    # ---- training step: the draws the reference will make
    def draws():
        a = t(actions)
        noise = torch.normal(mean=torch.zeros_like(a), std=torch.ones_like(a))
        time = torch.distributions.Beta(1.5, 1.0).sample((B,)) * 0.999 + 0.001
        return noise, time.to(a.dtype)
    torch.manual_seed(SEED + 3)
    noise, time = draws()
    torch.manual_seed(SEED + 3)
    m.train()
    out = m(actions=t(actions), states=t(states), **kw)
    chk = torch.nn.functional.mse_loss(out.logits, noise - t(actions))
    assert torch.equal(chk, out.loss), "the replicated noise is not the reference's"
    out.loss.backward()
    sd = dict(m.named_parameters())
    res = dict(seed=np.int64(SEED), w_keys=np.array(keys), w_shapes=pack_shapes(shapes), w_checksums=checksums(keys, w),
               image_shape=np.array(image_shape, dtype=np.int64), image_checksum=checksums(["images"], {"images": images}),
               input_ids=ids, attention_mask=mask, image_masks=image_masks, actions=actions, states=states,
               noise=noise.numpy().astype(np.float32), time=time.numpy().astype(np.float32),
               loss=np.float32(out.loss.item()), v_t=out.logits.detach().numpy().astype(np.float32),
               cfg=np.array([VOCAB, HIDDEN, INTER, LAYERS, HEADS, KV_HEADS, HEAD_DIM, A_HIDDEN, A_INTER, V_HIDDEN, V_INTER, V_LAYERS,
                             V_HEADS, V_IMAGE, V_PATCH, CHUNK, ADIM, STEPS], dtype=np.int64))
    gsq, no_grad, zero = 0.0, [], []
    for n, p_ in sd.items():
        if p_.grad is None:
            no_grad.append(n)
            continue
        gn = p_.grad.double().norm().item()
        gsq += gn * gn
        res["gradN/" + n] = np.float64(gn)
        if gn == 0.0:
            zero.append(n)
    res["grad_norm"] = np.float64(gsq ** 0.5)
    res["no_grad"] = np.array(sorted(no_grad))
    res["zero_grad"] = np.array(sorted(zero))
    for n in FULL_GRADS:
        res["grad/" + n] = sd[n].grad.numpy().astype(np.float32)

    # ---- sampler: the reference's own with the list cache, and the recompute loop
    m.eval()
    arch.DynamicCache = ListCache
    shape = (B, CHUNK, ADIM)
    torch.manual_seed(SEED + 4)
    init = torch.normal(0, 1, size=shape, dtype=torch.float32)
    torch.manual_seed(SEED + 4)
    with torch.no_grad():
        got = m.inference_action(states=t(states), diffusion_steps=STEPS, **kw)
        want = recompute_sampler(m, U, t(ids), t(mask), t(images), t(image_masks), init, STEPS)
    diff = float((got - want).abs().max())
    assert diff == 0.0, f"cached sampler and recompute loop differ by {diff}"
    res["init_noise"] = init.numpy().astype(np.float32)
    res["infer_actions"] = got.numpy().astype(np.float32)

    # ---- the reference's own bf16 arithmetic on the same batch
    bf16_note = "not run"
    try:
        mb = build(True)
        mb.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
        mb.model.to_bfloat16_for_selected_params()
        mb.train()
        torch.manual_seed(SEED + 3)
        with torch.no_grad():
            ob = mb(actions=t(actions), states=t(states), **kw)
        res["bf16/loss"] = np.float32(ob.loss.float().item())
        res["bf16/v_t"] = ob.logits.float().numpy().astype(np.float32)
        bf16_note = f"loss {res['bf16/loss']:.5f}"
    except Exception as e:                                       # noqa: BLE001  (reported, nothing recorded)
        bf16_note = f"did not run: {type(e).__name__}: {e}"
    path = os.path.join(GOLD, "dm0_t1.npz")
    np.savez_compressed(path, **res)
    print(f"[gen_golden_dm0] params {n_par} loss {res['loss']:.5f} |g| {res['grad_norm']:.4f} no_grad {len(no_grad)} zero {zero} "
          f"sampler diff {diff} bf16 {bf16_note} {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
