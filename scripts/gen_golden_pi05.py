"""Generate tests/golden/pi05_t1.npz by running the REFERENCE's Pi05ForCausalLM on the CPU.

TEST INFRASTRUCTURE, CPU only.  Needs the reference tree next to this repository's build container (oracle/gen_golden.py: REF); the
fixture it writes is committed, so no test reads the reference.

    python scripts/gen_golden_pi05.py            # from the repository root

Pinned: a tiny pi0.5 — SigLIP tower 64 wide, 2 layers, 28 px / patch 14 (4 tokens per camera), linear projector; Gemma llm
(``adarms_gemma`` with ``use_adarms=False``: a plain ``gemma`` llm fails in the reference, HF's GemmaRMSNorm.forward takes no
``cond``) d 96, F 128, 4 q / 1 kv heads x 32, 3 layers; action expert ``adarms_gemma`` with ``use_adarms=True``, d 64, F 80,
``width`` = ``adarms_cond_dim`` = 64 — on a batch of 2 samples x 3 cameras, camera 1 of sample 1 masked out, 7 text tokens, sample 1
right-padded by 2, chunk_size 6, action_dim 8.  Every weight is random, the ``dense`` ones of the adaptive norms included (the
reference zero-initialises them, which would hide the scale and the gate).  Recorded: the inputs, the injected ``noise`` / ``time``,
``loss``, ``v_t``, every gradient norm (``gradN/``), eight gradients in full (``grad/``), the parameters whose gradient is None
(``no_grad``), the ordered key / shape list of the state dict, and ``init_noise`` / ``infer_actions`` of the 10-step Euler sampler.
The weights and the images are NOT stored: tests/muvla_weights.py regenerates them from the seed and the ordered key / shape list,
and the archive keeps per-tensor checksums.

How the draws are pinned without editing the reference: ``forward`` and ``inference_action`` draw their noise / time with the global
torch generator; the script seeds it, makes the same calls itself, seeds it again and calls the reference.  The forward's pair is
verified through ``mse(v_t, noise - actions) == loss``.

Shims, none of which edits the reference: (1) a stub ``loguru`` module (``logger`` = a logging.Logger; the package is not installed);
(2) placeholder classes on ``transformers.models.gemma.modeling_gemma`` for the five names the reference's modeling file imports and
this transformers no longer exports; (3) ``rope_parameters`` in both Gemma config dicts; (4) the ``DynamicCache.key_cache`` /
``value_cache`` views of oracle/gen_golden_pi0.py (pi05_arch.py:192-197 reads them); and the timm stub of oracle/gen_golden.py.

bf16: the reference is also converted to bf16 (``.to(torch.bfloat16)``) and run on the same batch on the CPU, every floating-point
input in bf16 and the same draws rounded to bf16 (``inject`` of oracle/gen_golden_pi0.py); its ``loss`` / ``v_t`` are recorded as
``bf16/loss`` / ``bf16/v_t``.  Should it not run, the script prints the exception and records nothing under ``bf16/``.
"""
from __future__ import annotations

import logging
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

SEED = 53
VOCAB, HIDDEN, INTER, LAYERS, HEADS, KV_HEADS, HEAD_DIM = 264, 96, 128, 3, 4, 1, 32
A_HIDDEN, A_INTER = 64, 80
V_HIDDEN, V_INTER, V_LAYERS, V_HEADS, V_IMAGE, V_PATCH = 64, 128, 2, 2, 28, 14
B, CAMS, L_TXT, CHUNK, ADIM, STEPS = 2, 3, 7, 6, 8, 10
ROPE_THETA = 10000.0
FULL_GRADS = ("model.action_expert.layers.1.input_layernorm.dense.weight", "model.action_expert.norm.dense.weight",
              "model.time_mlp_in.weight", "model.llm.layers.0.input_layernorm.weight",
              "model.action_expert.layers.2.post_attention_layernorm.dense.bias", "model.action_expert.layers.0.self_attn.q_proj.weight",
              "model.llm.layers.1.self_attn.k_proj.weight", "model.action_in_proj.weight")
GEMMA_NAMES = ("AttentionMaskConverter", "KwargsForCausalLM", "SequenceClassifierOutputWithPast", "StaticCache", "TokenClassifierOutput")


def install_shims():
    """shims (1), (2) and (4) of the module docstring"""
    if "loguru" not in sys.modules:
        mod = types.ModuleType("loguru")
        mod.logger = logging.getLogger("loguru")
        sys.modules["loguru"] = mod
    import transformers.models.gemma.modeling_gemma as hf_gemma
    for name in GEMMA_NAMES:
        if not hasattr(hf_gemma, name):
            setattr(hf_gemma, name, type(name, (), {}))
    import oracle.gen_golden_pi0  # noqa: F401  (the module whose DynamicCache views these are)
    from transformers import DynamicCache
    if not hasattr(DynamicCache, "key_cache"):
        DynamicCache.key_cache = property(lambda self: [l.keys for l in self.layers])
        DynamicCache.value_cache = property(lambda self: [l.values for l in self.layers])


def gemma_dict(hidden, inter, **over):
    d = dict(model_type="adarms_gemma", vocab_size=VOCAB, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=LAYERS,
             num_attention_heads=HEADS, num_key_value_heads=KV_HEADS, head_dim=HEAD_DIM, max_position_embeddings=512,
             rope_theta=ROPE_THETA, rms_norm_eps=1e-6, rope_parameters=dict(rope_type="default", rope_theta=ROPE_THETA),
             use_adarms=False)
    d.update(over)
    return d


def main():
    from oracle.gen_golden import GOLD, REF, install_timm_shim
    from oracle.gen_golden_pi0 import inject
    from tests.muvla_weights import checksums, make_images, make_weights, pack_shapes
    sys.path.insert(0, REF)
    install_timm_shim()
    install_shims()
    from transformers import SiglipImageProcessor
    import dexbotic.model.pi05  # noqa: F401  (registers adarms_gemma)
    from dexbotic.model.pi05 import pi05_arch as arch

    torch.manual_seed(SEED)
    torch.set_num_threads(8)
    d_proc = os.path.join(tempfile.mkdtemp(), "tiny_siglip")
    SiglipImageProcessor(size={"height": V_IMAGE, "width": V_IMAGE}).save_pretrained(d_proc)
    vc = dict(model_type="siglip_vision_model", hidden_size=V_HIDDEN, intermediate_size=V_INTER, num_hidden_layers=V_LAYERS,
              num_attention_heads=V_HEADS, image_size=V_IMAGE, patch_size=V_PATCH, layer_norm_eps=1e-6)
    llm = gemma_dict(HIDDEN, INTER)
    act = gemma_dict(A_HIDDEN, A_INTER, use_adarms=True, adarms_cond_dim=A_HIDDEN, width=A_HIDDEN)

    def build():
        cfg = arch.Pi05Config(vision_config=dict(vc), processor_config=d_proc, action_config=dict(act), llm_config=dict(llm),
                              mm_projector_type="linear", action_dim=ADIM, chunk_size=CHUNK)
        return arch.Pi05ForCausalLM(cfg)

    m = build()
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

    # ---- training step: the draws the reference will make (pi05_arch.py:355-368)
    def draws():
        a = t(actions)
        noise = torch.normal(mean=torch.zeros_like(a), std=torch.ones_like(a))
        time = torch.distributions.Beta(1.5, 1).sample((B,)) * 0.999 + 0.001
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
    gsq, no_grad = 0.0, []
    for n, p_ in sd.items():
        if p_.grad is None:
            no_grad.append(n)
            continue
        gn = p_.grad.double().norm().item()
        gsq += gn * gn
        res["gradN/" + n] = np.float64(gn)
    res["grad_norm"] = np.float64(gsq ** 0.5)
    res["no_grad"] = np.array(sorted(no_grad))
    for n in FULL_GRADS:
        res["grad/" + n] = sd[n].grad.numpy().astype(np.float32)

    # ---- sampler: the reference's own (pi05_arch.py:423-515), its initial noise pinned by the seed
    m.eval()
    shape = (B, CHUNK, ADIM)
    torch.manual_seed(SEED + 4)
    init = torch.normal(0, 1, size=shape, dtype=torch.float32)
    torch.manual_seed(SEED + 4)
    with torch.no_grad():
        got = m.inference_action(states=t(states), diffusion_steps=STEPS, **kw)
    res["init_noise"] = init.numpy().astype(np.float32)
    res["infer_actions"] = got.numpy().astype(np.float32)

    # ---- the reference's own bf16 arithmetic on the same batch
    bf16_note = "not run"
    try:
        mb = build()
        mb.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
        mb = mb.to(torch.bfloat16)
        mb.train()
        # every floating-point input in bf16 (the reference takes the dtype of noise, time and x_t from ``actions``); the same draws,
        # rounded to bf16, handed in through oracle/gen_golden_pi0.py's ``inject``
        bf = torch.bfloat16
        with torch.no_grad(), inject(noise.to(bf), time.to(bf).float()):
            ob = mb(actions=t(actions).to(bf), states=t(states).to(bf), input_ids=t(ids), attention_mask=t(mask),
                    images=t(images).to(bf), image_masks=t(image_masks))
        res["bf16/loss"] = np.float32(ob.loss.float().item())
        res["bf16/v_t"] = ob.logits.float().numpy().astype(np.float32)
        bf16_note = f"loss {res['bf16/loss']:.5f}"
    except Exception as e:                                       # noqa: BLE001  (reported, nothing recorded)
        bf16_note = f"did not run: {type(e).__name__}: {e}"
    path = os.path.join(GOLD, "pi05_t1.npz")
    np.savez_compressed(path, **res)
    print(f"[gen_golden_pi05] params {n_par} loss {res['loss']:.5f} |g| {res['grad_norm']:.4f} no_grad {sorted(no_grad)} "
          f"bf16 {bf16_note} {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
