"""Generate tests/golden/oft_dit_t1.npz by running the REFERENCE's OFTForCausalLM with ``action_model_type="DiT"`` on the CPU.

TEST INFRASTRUCTURE, CPU only.  Needs the reference tree next to this repository's build container (oracle/gen_golden.py: REF); the
fixture it writes is committed, so no test reads the reference.

    python scripts/gen_golden_oft_dit.py        # from the repository root

The tiny model, the batch and the shims are those of scripts/gen_golden_oft.py (imported, not edited), built TWICE: ``use_proprio``
False (keys under ``np/``) and True (``pp/``).  The one thing the reference takes from the ``diffusers`` package, which is not
installed, is ``DDIMScheduler``: a stand-in of OUR OWN is injected under that name before the reference is imported.  It is written
from the DDIM formulas (cosine schedule ``squaredcos_cap_v2``, "leading" timestep spacing, eta 0, epsilon prediction, clip_sample at
1) in the package's order of operations; it was NOT checked against the package.  dexbotic_amd/model/oft/action_model/ddim.py states
the same formulas independently, so a test of one against the other is a test of consistency only.

Stored at top level: ``alphas_cumprod`` [100], the 10 inference timesteps, the training timesteps (7 and 93: both ends of the
schedule), the batch.  Per build: the training ``noise`` / ``noisy_actions`` / time embeddings (a deterministic ``noisy_dict``), the
predicted noise, the MSE loss, every gradient norm (``gradN/``), six gradients in full (``grad/``), the parameters without a gradient,
the ordered key / shape list, and the reference's bf16 run with its distance from the fp32 run (``bf16_gap_*``, as in oft_t1.npz).
For the sampler of sample 0 (``inference_action``, 10 steps): the start noise, ``eps_k`` and ``x_k`` after each step, the
de-normalised actions; the same from the bf16 model with its gaps.  ``torch.randn`` is replaced for the length of that call by a
function that returns the stored start noise (on the bf16 grid, so both precisions start from the same point).

The bf16 loss gap bounds the GPU test's bf16 loss, and a loss is a mean: the reference's two runs can agree by cancellation while
their predictions are a bf16 rounding apart.  The training noise comes from the first seeded stream whose loss gap is at least 2^-10
(a quarter of bf16's spacing) in both builds; the script asserts it.

A final element with |x| = 1 was saturated by the clamp and says nothing about the arithmetic before it: the start noise comes from
the first seeded stream for which at most one final element in four is saturated, in both builds; the script asserts it.
"""
from __future__ import annotations

import importlib.machinery
import math
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

SEED = 67
TRAIN_TIMESTEPS = (7, 93)
DDIM_STEPS = 10
FULL_GRADS = ("model.action_head.noisy_action_projector.fc1.weight", "model.action_head.noisy_action_projector.fc1.bias",
              "model.action_head.noisy_action_projector.fc2.weight", "model.action_head.noise_predictor.mlp_resnet.layer_norm1.weight",
              "model.llm.layers.0.self_attn.q_proj.weight", "model.action_head.proprio_projector.fc1.weight")
MIN_LOSS_GAP = 2.0 ** -10     # smallest bf16-against-fp32 loss gap of the reference that is taken as a measure of bf16 (main())
STEP_LOG = []           # (model_output, sample, prev_sample) of every scheduler step, in call order


class DDIMScheduler:
    """stand-in for diffusers.schedulers.scheduling_ddim.DDIMScheduler: what the reference's OFT calls, nothing else"""

    def __init__(self, num_train_timesteps: int = 1000, beta_schedule: str = "linear", **kw):
        assert beta_schedule == "squaredcos_cap_v2" and not kw, (beta_schedule, kw)
        N = num_train_timesteps

        def ab(s):
            return math.cos((s + 0.008) / 1.008 * math.pi / 2) ** 2

        self.betas = torch.tensor([min(1 - ab((i + 1) / N) / ab(i / N), 0.999) for i in range(N)], dtype=torch.float32)
        self.alphas_cumprod = torch.cumprod(1.0 - self.betas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0)
        self.config = types.SimpleNamespace(num_train_timesteps=N, clip_sample=True, clip_sample_range=1.0, prediction_type="epsilon",
                                            timestep_spacing="leading", steps_offset=0)
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, N)[::-1].copy().astype(np.int64))

    def add_noise(self, original_samples, noise, timesteps):
        a = self.alphas_cumprod.to(dtype=original_samples.dtype)
        sa, sb = a[timesteps] ** 0.5, (1 - a[timesteps]) ** 0.5
        while sa.dim() < original_samples.dim():
            sa, sb = sa.unsqueeze(-1), sb.unsqueeze(-1)
        return sa * original_samples + sb * noise

    def set_timesteps(self, num_inference_steps: int, device=None):
        self.num_inference_steps = num_inference_steps
        ratio = self.config.num_train_timesteps // num_inference_steps
        self.timesteps = torch.from_numpy((np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64))

    def step(self, model_output, timestep, sample, eta: float = 0.0):
        assert eta == 0.0
        t = int(timestep)
        prev = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev] if prev >= 0 else self.final_alpha_cumprod
        x0 = (sample - (1 - a_t) ** 0.5 * model_output) / a_t ** 0.5
        x0 = x0.clamp(-self.config.clip_sample_range, self.config.clip_sample_range)
        prev_sample = a_prev ** 0.5 * x0 + (1 - a_prev) ** 0.5 * model_output      # the model's own eps, not re-derived after the clamp
        STEP_LOG.append((model_output.detach().clone(), sample.detach().clone(), prev_sample.detach().clone()))
        return types.SimpleNamespace(prev_sample=prev_sample, pred_original_sample=x0)


def install_ddim_stand_in():
    assert "diffusers" not in sys.modules, "install the stand-in before anything imports diffusers"
    names = ("diffusers", "diffusers.schedulers", "diffusers.schedulers.scheduling_ddim")
    mods = {n: types.ModuleType(n) for n in names}
    mods[names[2]].DDIMScheduler = DDIMScheduler
    mods[names[1]].scheduling_ddim = mods[names[2]]
    mods[names[0]].schedulers = mods[names[1]]
    for n, m in mods.items():
        m.__spec__ = importlib.machinery.ModuleSpec(n, None)
        sys.modules[n] = m


def main():
    import gen_golden_oft as G
    from oracle.gen_golden import GOLD, REF, install_timm_shim
    from tests.muvla_weights import checksums, make_images, make_weights, pack_shapes
    sys.path.insert(0, REF)
    install_timm_shim()
    install_ddim_stand_in()
    G.install_diffusers_stub()                                   # (finds the stand-in and leaves it)
    from transformers import CLIPImageProcessor, CLIPVisionConfig, CLIPVisionModel, Qwen2Config
    from dexbotic.model.oft.oft_arch import OFTConfig, OFTForCausalLM
    rel_err = G.rel_err
    B, ADIM, CHUNK, PDIM, HIDDEN = G.B, G.ADIM, G.CHUNK, G.PDIM, G.HIDDEN

    torch.manual_seed(SEED)
    torch.set_num_threads(8)
    d = os.path.join(tempfile.mkdtemp(), "tiny_clip")
    vcfg = CLIPVisionConfig(hidden_size=G.V_HIDDEN, intermediate_size=G.V_INTER, num_hidden_layers=G.V_LAYERS,
                            num_attention_heads=G.V_HEADS, image_size=G.V_IMAGE, patch_size=G.V_PATCH, layer_norm_eps=1e-5)
    CLIPVisionModel(vcfg).save_pretrained(d)
    CLIPImageProcessor(size={"shortest_edge": G.V_IMAGE}, crop_size={"height": G.V_IMAGE, "width": G.V_IMAGE}).save_pretrained(d)

    def build(use_proprio: bool):
        llm = Qwen2Config(vocab_size=G.VOCAB, hidden_size=HIDDEN, intermediate_size=G.INTER, num_hidden_layers=G.LAYERS,
                          num_attention_heads=G.HEADS, num_key_value_heads=G.KV_HEADS, max_position_embeddings=4096,
                          rope_theta=1e6, rms_norm_eps=1e-6)
        cfg = OFTConfig(llm_config=llm, mm_vision_tower=d, mm_projector_type="mlp2x_gelu", action_model_type="DiT",
                        action_dim=ADIM, chunk_size=CHUNK, use_proprio=use_proprio, proprio_dim=PDIM)
        m = OFTForCausalLM(cfg)
        for p_ in m.parameters():
            p_.requires_grad = True
        return m

    rs = np.random.RandomState(SEED + 2)
    ids = rs.randint(10, 250, size=(B, G.L_TXT)).astype(np.int64)
    ids[:, 2] = G.IMG
    mask = np.ones((B, G.L_TXT), dtype=bool)
    mask[1, G.L_TXT - 3:] = False                    # sample 1: three tokens shorter (right padding)
    image_shape = (B, 3, G.V_IMAGE, G.V_IMAGE)
    images = make_images(image_shape, SEED)
    states = rs.uniform(-1, 1, size=(B, PDIM)).astype(np.float32)
    actions = rs.uniform(-1, 1, size=(B, CHUNK, ADIM)).astype(np.float32)
    t = torch.from_numpy
    bf = torch.bfloat16
    timesteps = torch.tensor(TRAIN_TIMESTEPS, dtype=torch.int64)

    builds = {}
    for tag, use_proprio in (("np", False), ("pp", True)):
        m = build(use_proprio)
        keys = list(m.state_dict().keys())
        shapes = [tuple(v.shape) for v in m.state_dict().values()]
        w = make_weights(keys, shapes, SEED)
        m.load_state_dict({k: t(v) for k, v in w.items()}, strict=True)
        m.train()
        mb = build(use_proprio)
        mb.load_state_dict({k: t(v) for k, v in w.items()}, strict=True)
        mb = mb.to(bf)
        mb.train()
        builds[tag] = dict(m=m, mb=mb, keys=keys, shapes=shapes, w=w, kw=dict(states=t(states)) if use_proprio else {})

    def noisy_dict(m, noise, dtype=torch.float32):
        """the deterministic ``noisy_dict`` of the batch, as sample_noisy_actions forms it; the noise (the target) stays fp32"""
        head = m.model.action_head
        noisy = head.noise_scheduler.add_noise(t(actions), t(noise), timesteps)
        temb = head.time_encoder(timesteps).to(noisy.dtype).unsqueeze(1)
        return dict(noise=t(noise), noisy_actions=noisy.to(dtype), diffusion_timestep_embeddings=temb.to(dtype))

    def run(model, nd, kw, dtype=torch.float32):
        return model(input_ids=t(ids), attention_mask=t(mask), images=t(images).to(dtype), actions=t(actions), noisy_dict=nd,
                     **{k: v.to(dtype) for k, v in kw.items()})

    # the training noise.  A loss is a mean: the bf16 run's loss can land on the fp32 run's by cancellation while its predictions
    # are a bf16 rounding away, and twice such a gap bounds nothing.  bf16 keeps 8 bits: a relative gap below 2^-10, a quarter of
    # its spacing, is agreement by cancellation.  The noise comes from the first seeded stream whose loss gap is at least that, in
    # both builds (a condition on the reference's two runs alone)
    train_seed = None
    for ts in range(100):
        noise = np.random.RandomState(SEED + 300 + ts).standard_normal((B, CHUNK, ADIM)).astype(np.float32)
        gaps = []
        for bd in builds.values():
            with torch.no_grad():
                l32 = run(bd["m"], noisy_dict(bd["m"], noise), bd["kw"]).loss.item()
                lbf = run(bd["mb"], noisy_dict(bd["m"], noise, bf), bd["kw"], bf).loss.float().item()
            gaps.append(abs(lbf - l32) / abs(l32))
        if min(gaps) >= MIN_LOSS_GAP:
            train_seed = ts
            break
    assert train_seed is not None, "no noise stream gives a bf16 loss gap of 2^-10 in both builds"

    sched = builds["np"]["m"].model.action_head.noise_scheduler
    assert isinstance(sched, DDIMScheduler)
    sched.set_timesteps(DDIM_STEPS)
    ddim_timesteps = sched.timesteps.numpy().astype(np.int64)
    assert ddim_timesteps.tolist() == [90, 80, 70, 60, 50, 40, 30, 20, 10, 0]

    def sample(model, kw0, start, dtype):
        """the reference's inference_action on sample 0 from the given start noise -> (eps [n, T, A], x [n, T, A], actions)"""
        real_randn = torch.randn

        def fixed_randn(*size, **k):
            assert tuple(size) == (1, CHUNK, ADIM) and k.get("dtype") == dtype, (size, k)
            return t(start).to(dtype)

        del STEP_LOG[:]
        torch.randn = fixed_randn
        try:
            got = model.inference_action(t(ids[:1]), t(images[:1]).to(dtype), dict(action_norms=G.ACTION_NORMS, num_ddim_steps=DDIM_STEPS,
                                                                                 **{k: v.to(dtype) for k, v in kw0.items()}))
        finally:
            torch.randn = real_randn
        assert len(STEP_LOG) == DDIM_STEPS and torch.equal(STEP_LOG[0][1].float(), t(start))
        eps = np.stack([e.float().numpy()[0] for e, _, _ in STEP_LOG]).astype(np.float32)
        xs = np.stack([x.float().numpy()[0] for _, _, x in STEP_LOG]).astype(np.float32)
        return eps, xs, np.array(got, dtype=np.float64)

    # the start noise of the sampler: on the bf16 grid, and at most one final element in four saturated by the clamp, in both builds
    for bd in builds.values():
        bd["m"].eval()
    noise_seed = None
    for ns in range(200):
        start = t(np.random.RandomState(SEED + 500 + ns).standard_normal((1, CHUNK, ADIM)).astype(np.float32)).to(bf).float().numpy()
        sat = []
        for bd in builds.values():
            _, xs, _ = sample(bd["m"], {k: v[:1] for k, v in bd["kw"].items()}, start, torch.float32)
            sat.append(int((np.abs(xs[-1]) >= 1.0).sum()))
        if all(4 * s <= CHUNK * ADIM for s in sat):
            noise_seed = ns
            break
    assert noise_seed is not None, "no start noise leaves three final elements in four unsaturated"
    for bd in builds.values():
        bd["m"].train()

    res = dict(seed=np.int64(SEED), noise_seed=np.int64(noise_seed), train_seed=np.int64(train_seed), input_ids=ids, attention_mask=mask, actions=actions, states=states,
               image_shape=np.array(image_shape, dtype=np.int64), image_checksum=checksums(["images"], {"images": images}),
               action_norm_min=np.array(G.ACTION_NORMS["min"], dtype=np.float64),
               action_norm_max=np.array(G.ACTION_NORMS["max"], dtype=np.float64),
               alphas_cumprod=sched.alphas_cumprod.numpy().astype(np.float32), ddim_timesteps=ddim_timesteps,
               train_timesteps=np.array(TRAIN_TIMESTEPS, dtype=np.int64), sampler_start=start.astype(np.float32),
               cfg=np.array([G.VOCAB, HIDDEN, G.INTER, G.LAYERS, G.HEADS, G.KV_HEADS, G.V_HIDDEN, G.V_INTER, G.V_LAYERS, G.V_HEADS,
                             G.V_IMAGE, G.V_PATCH, ADIM, CHUNK, PDIM], dtype=np.int64))
    notes = []
    for tag, bd in builds.items():
        m, mb, kw, keys, shapes, w = bd["m"], bd["mb"], bd["kw"], bd["keys"], bd["shapes"], bd["w"]
        P = tag + "/"
        nd = noisy_dict(m, noise)
        noisy, temb = nd["noisy_actions"], nd["diffusion_timestep_embeddings"]
        m.zero_grad(set_to_none=True)
        out = run(m, nd, kw)
        out.loss.backward()
        pred = out.logits.detach().float().numpy()
        sd = dict(m.named_parameters())
        res.update({P + "w_keys": np.array(keys), P + "w_shapes": pack_shapes(shapes), P + "w_checksums": checksums(keys, w),
                    P + "noise": noise, P + "noisy_actions": noisy.numpy().astype(np.float32),
                    P + "time_embeddings": temb.numpy().astype(np.float32),
                    P + "pred": pred.astype(np.float32), P + "loss": np.float32(out.loss.item())})
        gsq, no_grad = 0.0, []
        for n, p_ in sd.items():
            if p_.grad is None:
                no_grad.append(n)
                continue
            gn = p_.grad.double().norm().item()
            gsq += gn * gn
            res[P + "gradN/" + n] = np.float64(gn)
        res[P + "grad_norm"] = np.float64(gsq ** 0.5)
        res[P + "no_grad"] = np.array(sorted(no_grad))
        for n in FULL_GRADS:
            if n in sd:
                res[P + "grad/" + n] = sd[n].grad.numpy().astype(np.float32)
        # the reference's own bf16 arithmetic on the same batch: noisy actions and time rows in bf16, the noise (the target) in fp32
        with torch.no_grad():
            ob = run(mb, noisy_dict(m, noise, bf), kw, bf)
        pbf = ob.logits.float().numpy()
        res[P + "bf16/loss"] = np.float32(ob.loss.float().item())
        res[P + "bf16/pred"] = pbf.astype(np.float32)
        res[P + "bf16_gap_loss"] = np.float64(abs(float(res[P + "bf16/loss"]) - float(res[P + "loss"])) / abs(float(res[P + "loss"])))
        res[P + "bf16_gap_pred"] = np.float64(rel_err(pbf, pred))
        # the sampler on sample 0, fp32 and bf16, from the same start
        m.eval()
        mb.eval()
        kw0 = {k: v[:1] for k, v in kw.items()}
        eps, xs, acts = sample(m, kw0, start, torch.float32)
        eps_b, xs_b, acts_b = sample(mb, kw0, start, bf)
        sat = int((np.abs(xs[-1]) >= 1.0).sum())
        assert 4 * sat <= CHUNK * ADIM, (tag, xs[-1])
        assert float(res[P + "bf16_gap_loss"]) >= MIN_LOSS_GAP, (tag, res[P + "bf16_gap_loss"])
        res.update({P + "sampler/eps": eps, P + "sampler/x": xs, P + "sampler/actions": acts, P + "sampler/bf16/eps": eps_b,
                    P + "sampler/bf16/x": xs_b, P + "sampler/bf16/actions": acts_b,
                    P + "bf16_gap_x": np.float64(rel_err(xs_b, xs)), P + "bf16_gap_actions": np.float64(rel_err(acts_b, acts))})
        notes.append(f"{tag}: loss {res[P + 'loss']:.5f} |g| {res[P + 'grad_norm']:.4f} no_grad {len(no_grad)} bf16 loss "
                     f"{res[P + 'bf16/loss']:.5f} gaps {res[P + 'bf16_gap_loss']:.3e}/{res[P + 'bf16_gap_pred']:.3e}; sampler final |x| "
                     f"{np.abs(xs[-1]).min():.2f}-{np.abs(xs[-1]).max():.2f} ({sat} saturated) bf16 gaps "
                     f"{res[P + 'bf16_gap_x']:.3e}/{res[P + 'bf16_gap_actions']:.3e}")
    path = os.path.join(GOLD, "oft_dit_t1.npz")
    np.savez_compressed(path, **res)
    print(f"[gen_golden_oft_dit] training noise stream {train_seed}, sampler noise stream {noise_seed}; " + "; ".join(notes) + f"; {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
