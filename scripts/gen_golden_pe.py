"""Generate tests/golden/pe_t1.npz (and dm0_pe_t1.npz) by running the REFERENCE's Perception Encoder tower on the CPU.

TEST INFRASTRUCTURE, CPU only.  Needs the reference tree next to this repository's build container (oracle/gen_golden.py: REF); the
fixtures it writes are committed, so no test reads the reference.

    python scripts/gen_golden_pe.py            # from the repository root

pe_t1.npz.  Pinned: a tiny tower — patch 4, width 64, 2 layers, 2 heads (head width 32), mlp_ratio 2, image_size 24, CLS token, no
ln_post, LayerScale, pool "none" — built with ``PerceptionEncoderConfig(...).build_model()`` (the reference's ``get_config`` knows
one name only).  EVERY tensor is overwritten: ``attn.in_proj_weight`` / ``in_proj_bias`` are ``torch.empty`` in the reference and a
freshly built tower yields NaN; the LayerScale gammas are of order 1 (tests/pe_weights.py).  Runs:
  * 2 images at 24 px (grid 6, 37 tokens; 6 -> 3 -> 2 exercises the padded border of the second convolution at an odd grid):
    ``out`` [2, 4, 256], ``loss`` = sum(out * R) for the stored ``R``, every gradient norm (``gradN/``), five gradients in full
    (``grad/``) and every fourth output channel of ``vit_downsampler2.weight``'s (``grad_rows4/``: the whole tensor, 1.2 MB of
    floats, is more than a committed file may hold; its norm is under ``gradN/`` like the others);
  * the same weights on 1 image at 16 px (grid 4, not the native 6: resampled positions, picked RoPE rows): ``out16`` [1, 1, 256],
    ``loss16`` = sum(out16 * R16), and the gradients of ``positional_embedding`` / ``class_embedding`` in full (``grad16/``);
  * the reference's own bf16 run (``.to(torch.bfloat16)``) of the 24-px batch: ``bf16/out``.
The weights and the images are NOT stored: tests/pe_weights.py regenerates them from the seed and the ordered key / shape list, and
the archive keeps per-tensor checksums.

dm0_pe_t1.npz.  The tiny DM0 of scripts/gen_golden_dm0.py (its constants, list cache and recompute sampler are imported from there)
with this tower instead of CLIP — ``mm_vision_tower="pe_lang_l14_728"`` while ``pe_encoder.get_config`` is replaced FROM HERE by a
function that returns the tiny config, ``mm_projector_type="linear4x"`` — recorded as gen_golden_dm0.py records dm0_t1.npz.  Should
the reference's DM0 class not build or run that way, the script prints the exception and writes no dm0_pe_t1.npz.

Shims, none of which edits the reference: the timm stub of oracle/gen_golden.py and a stub ``loguru`` module where the package is not
installed (as scripts/gen_golden_pi05.py).
"""
from __future__ import annotations

import logging
import os
import sys
import tempfile
import traceback
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

SEED = 67
PATCH, WIDTH, LAYERS, HEADS, MLP_RATIO, IMAGE, LS_INIT = 4, 64, 2, 2, 2.0, 24, 0.1
N_IMG, IMAGE_SMALL = 2, 16
P = "model.mm_vision_tower.vision_tower."
FULL_GRADS = ("conv1.weight", "positional_embedding", "transformer.resblocks.1.attn.in_proj_weight", "transformer.resblocks.0.ls_1.gamma",
              "vit_downsampler1.weight")
DM0_FULL_GRADS = (P + "conv1.weight", P + "transformer.resblocks.0.ls_1.gamma", P + "vit_downsampler2.bias",
                  "model.mm_projector.weight", "model.llm.layers.1.self_attn.k_proj.weight", "model.action_time_mlp_in.weight")


def install_loguru_stub():
    try:
        import loguru  # noqa: F401
    except ImportError:
        mod = types.ModuleType("loguru")
        mod.logger = logging.getLogger("loguru")
        sys.modules["loguru"] = mod


def tiny_config(pe_cfg):
    return pe_cfg.PerceptionEncoderConfig(patch_size=PATCH, width=WIDTH, layers=LAYERS, heads=HEADS, mlp_ratio=MLP_RATIO, output_dim=None,
                                          ls_init_value=LS_INIT, image_size=IMAGE, use_cls_token=True, pool_type="none",
                                          use_ln_pre=True, use_ln_post=False)


def grads_into(res, named, full, prefix=""):
    gsq, no_grad = 0.0, []
    for n, p_ in named.items():
        if p_.grad is None:
            no_grad.append(n)
            continue
        gn = p_.grad.double().norm().item()
        gsq += gn * gn
        res[prefix + "gradN/" + n] = np.float64(gn)
    for n in full:
        res[prefix + "grad/" + n] = named[n].grad.numpy().astype(np.float32)
    return gsq ** 0.5, sorted(no_grad)


def tower_fixture(pe_cfg, GOLD):
    from tests.muvla_weights import checksums, make_images, pack_shapes
    from tests.pe_weights import make_weights
    t = torch.from_numpy
    m = tiny_config(pe_cfg).build_model()
    keys = list(m.state_dict().keys())
    shapes = [tuple(v.shape) for v in m.state_dict().values()]
    w = make_weights(keys, shapes, SEED)
    m.load_state_dict({k: t(v) for k, v in w.items()}, strict=True)
    image_shape = (N_IMG, 3, IMAGE, IMAGE)
    images = make_images(image_shape, SEED)
    rs = np.random.RandomState(SEED + 5)

    out = m(t(images))
    R = rs.standard_normal(tuple(out.shape)).astype(np.float32)
    loss = (out * t(R)).sum()
    loss.backward()
    res = dict(seed=np.int64(SEED), w_keys=np.array(keys), w_shapes=pack_shapes(shapes), w_checksums=checksums(keys, w),
               image_shape=np.array(image_shape, dtype=np.int64), image_checksum=checksums(["images"], {"images": images}),
               cfg=np.array([PATCH, WIDTH, LAYERS, HEADS, int(MLP_RATIO), IMAGE, IMAGE_SMALL], dtype=np.int64), ls_init=np.float64(LS_INIT),
               out=out.detach().numpy().astype(np.float32), R=R, loss=np.float64(loss.item()))
    gnorm, no_grad = grads_into(res, dict(m.named_parameters()), FULL_GRADS)
    assert not no_grad, no_grad
    res["grad_norm"] = np.float64(gnorm)
    res["grad_rows4/vit_downsampler2.weight"] = m.vit_downsampler2.weight.grad[::4].numpy().astype(np.float32)

    # ---- the same weights at 16 px: grid 4 on a tower whose native grid is 6
    m.zero_grad(set_to_none=True)
    images16 = make_images((1, 3, IMAGE_SMALL, IMAGE_SMALL), SEED + 7)
    out16 = m(t(images16))
    R16 = rs.standard_normal(tuple(out16.shape)).astype(np.float32)
    loss16 = (out16 * t(R16)).sum()
    loss16.backward()
    named = dict(m.named_parameters())
    res.update(image16_seed=np.int64(SEED + 7), image16_checksum=checksums(["images"], {"images": images16}),
               out16=out16.detach().numpy().astype(np.float32), R16=R16, loss16=np.float64(loss16.item()))
    for n in ("positional_embedding", "class_embedding"):
        res["grad16/" + n] = named[n].grad.numpy().astype(np.float32)
    for n, p_ in named.items():
        res["grad16N/" + n] = np.float64(p_.grad.double().norm().item())

    # ---- the reference's own bf16 arithmetic on the 24-px batch
    bf16_note = "not run"
    try:
        mb = tiny_config(pe_cfg).build_model()
        mb.load_state_dict({k: t(v) for k, v in w.items()}, strict=True)
        mb = mb.to(torch.bfloat16)
        with torch.no_grad():
            ob = mb(t(images).to(torch.bfloat16))
        res["bf16/out"] = ob.float().numpy().astype(np.float32)
        d = float(np.abs(res["bf16/out"] - res["out"]).max() / np.abs(res["out"]).max())
        bf16_note = f"rel distance to fp32 {d:.3e}"
    except Exception as e:                                       # noqa: BLE001  (reported, nothing recorded)
        bf16_note = f"did not run: {type(e).__name__}: {e}"
    path = os.path.join(GOLD, "pe_t1.npz")
    np.savez_compressed(path, **res)
    print(f"[gen_golden_pe] tower params {sum(int(np.prod(s)) for s in shapes)} out {tuple(out.shape)} loss {loss.item():.5f} "
          f"|g| {gnorm:.4f} out16 {tuple(out16.shape)} loss16 {loss16.item():.5f} bf16 {bf16_note} {os.path.getsize(path)} bytes")


def dm0_fixture(pe_cfg, GOLD):
    import gen_golden_dm0 as D                                   # constants, ListCache, recompute_sampler (this directory)
    from tests.muvla_weights import checksums, make_images, pack_shapes
    from tests.pe_weights import make_weights
    from transformers import Qwen3Config
    from dexbotic.model.dm0 import dm0_arch as arch
    from dexbotic.model.dm0 import dm0_utils as U
    from dexbotic.model.modules.mm_vision.pe import pe_encoder
    pe_encoder.get_config = lambda name: tiny_config(pe_cfg)     # the shim: the registered name, the tiny tower
    t = torch.from_numpy
    tmp = tempfile.mkdtemp()
    d_llm, d_act = (os.path.join(tmp, n) for n in ("tiny_qwen3", "tiny_qwen3_action"))
    q3 = dict(vocab_size=D.VOCAB, num_hidden_layers=D.LAYERS, num_attention_heads=D.HEADS, num_key_value_heads=D.KV_HEADS,
              head_dim=D.HEAD_DIM, max_position_embeddings=4096, rope_theta=1e6, rms_norm_eps=1e-6, tie_word_embeddings=False,
              attention_bias=False)
    Qwen3Config(hidden_size=D.HIDDEN, intermediate_size=D.INTER, **q3).save_pretrained(d_llm)
    Qwen3Config(hidden_size=D.A_HIDDEN, intermediate_size=D.A_INTER, **q3).save_pretrained(d_act)

    def build(bf16):
        cfg = arch.DM0Config(llm_config=d_llm, action_config=d_act, mm_vision_tower="pe_lang_l14_728", mm_projector_type="linear4x",
                             action_dim=D.ADIM, chunk_size=D.CHUNK, bf16=bf16)
        return arch.DM0ForCausalLM(cfg)

    m = build(False)
    keys = list(m.state_dict().keys())
    shapes = [tuple(v.shape) for v in m.state_dict().values()]
    w = make_weights(keys, shapes, SEED)
    m.load_state_dict({k: t(v) for k, v in w.items()}, strict=True)
    for p_ in m.parameters():
        p_.requires_grad = True
    B, CAMS, L_TXT, CHUNK, ADIM, STEPS = D.B, D.CAMS, D.L_TXT, D.CHUNK, D.ADIM, D.STEPS
    rs = np.random.RandomState(SEED + 2)
    ids = rs.randint(10, 250, size=(B, L_TXT)).astype(np.int64)
    mask = np.ones((B, L_TXT), dtype=bool)
    mask[1, L_TXT - 2:] = False
    image_masks = np.ones((B, CAMS), dtype=bool)
    image_masks[1, 1] = False
    image_shape = (B, CAMS, 3, IMAGE, IMAGE)
    images = make_images(image_shape, SEED)
    actions = rs.uniform(-1, 1, size=(B, CHUNK, ADIM)).astype(np.float32)
    states = rs.uniform(-1, 1, size=(B, ADIM)).astype(np.float32)
    kw = dict(input_ids=t(ids), attention_mask=t(mask), images=t(images), image_masks=t(image_masks))

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
    res = dict(seed=np.int64(SEED), w_keys=np.array(keys), w_shapes=pack_shapes(shapes), w_checksums=checksums(keys, w),
               image_shape=np.array(image_shape, dtype=np.int64), image_checksum=checksums(["images"], {"images": images}),
               input_ids=ids, attention_mask=mask, image_masks=image_masks, actions=actions, states=states,
               noise=noise.numpy().astype(np.float32), time=time.numpy().astype(np.float32),
               loss=np.float32(out.loss.item()), v_t=out.logits.detach().numpy().astype(np.float32),
               cfg=np.array([D.VOCAB, D.HIDDEN, D.INTER, D.LAYERS, D.HEADS, D.KV_HEADS, D.HEAD_DIM, D.A_HIDDEN, D.A_INTER, CHUNK, ADIM,
                             STEPS], dtype=np.int64),
               pe_cfg=np.array([PATCH, WIDTH, LAYERS, HEADS, int(MLP_RATIO), IMAGE], dtype=np.int64), ls_init=np.float64(LS_INIT))
    gnorm, no_grad = grads_into(res, dict(m.named_parameters()), DM0_FULL_GRADS)
    res["grad_norm"] = np.float64(gnorm)
    res["no_grad"] = np.array(no_grad)

    m.eval()
    arch.DynamicCache = D.ListCache
    torch.manual_seed(SEED + 4)
    init = torch.normal(0, 1, size=(B, CHUNK, ADIM), dtype=torch.float32)
    torch.manual_seed(SEED + 4)
    with torch.no_grad():
        got = m.inference_action(states=t(states), diffusion_steps=STEPS, **kw)
        want = D.recompute_sampler(m, U, t(ids), t(mask), t(images), t(image_masks), init, STEPS)
    diff = float((got - want).abs().max())
    assert diff == 0.0, f"cached sampler and recompute loop differ by {diff}"
    res["init_noise"] = init.numpy().astype(np.float32)
    res["infer_actions"] = got.numpy().astype(np.float32)
    path = os.path.join(GOLD, "dm0_pe_t1.npz")
    np.savez_compressed(path, **res)
    print(f"[gen_golden_pe] dm0 params {sum(int(np.prod(s)) for s in shapes)} loss {res['loss']:.5f} |g| {gnorm:.4f} "
          f"no_grad {len(no_grad)} sampler diff {diff} {os.path.getsize(path)} bytes")


def main():
    from oracle.gen_golden import GOLD, REF, install_timm_shim
    sys.path.insert(0, REF)
    sys.path.insert(0, HERE)
    install_timm_shim()
    install_loguru_stub()
    from dexbotic.model.modules.mm_vision.pe import pe_configuration as pe_cfg
    torch.manual_seed(SEED)
    torch.set_num_threads(8)
    tower_fixture(pe_cfg, GOLD)
    try:
        dm0_fixture(pe_cfg, GOLD)
    except Exception as e:                                           # noqa: BLE001  (reported, no DM0 fixture written)
        traceback.print_exc()
        print(f"[gen_golden_pe] the reference's DM0 with this tower did not run: {type(e).__name__}: {e}")


if __name__ == "__main__":
    main()
