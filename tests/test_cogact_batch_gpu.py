"""CogACTForCausalLM.inference_action_batch: B requests through one prefill and — for a model served in bfloat16 — ONE launch of the
persistent DiT sampler with B request groups (csrc/dit_fused.hip).  Toy CogACT of the golden fixtures (t2: DiT 192 wide, 3 heads of
64, 3 blocks — the fused kernels' shapes), injected noise."""
import numpy as np
import pytest
import torch

from tests.helpers import build_product, load_golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
B = 3
# A chunk of the batch against the same request served alone.  The sampler contributes nothing to that distance (it is held to the
# single sampler's bits below); what differs is the bf16 prefill, whose products at 3 x S rows are not the kernels' choices at S rows,
# so the cognition feature moves by bf16 rounding — and this toy head's random weights amplify operand-level rounding to 3.2e-2 of
# the largest de-normalised action (tests/test_parity_gpu.py::test_whole_sampler_in_one_launch_equals_the_per_step_sampler, which
# bounds that at 1.5 x = 5e-2).  The per-component bound of the fp32 chunks (assert_chunk_close: atol 1e-5, rtol 1e-3) does not hold
# between two bf16 prefills: measured 1.4e-2, 2.5e-2 and 3.6e-2 for the three requests.  Bound: the same 5e-2.
BF16_CHUNK_TOL = 5e-2


@pytest.fixture(scope="module")
def setup(golden_dir):
    g, cfg, w = load_golden(golden_dir, "t2")
    m = build_product(cfg, w, "bfloat16", DEV, train=False)
    m.eval()
    norms = {"min": g["norm_min"].tolist(), "max": g["norm_max"].tolist()}
    args = {"cfg_scale": 1.5, "num_ddim_steps": 10, "action_norms": norms}
    return m, cfg, g, args


def _inputs(g, cfg, n):
    """n requests of the fixture's shape: the prompt with another last token each, n different frames, scaled noise"""
    ids = T(g["infer_ids"]).repeat(n, 1)
    ids[:, -1] = (ids[:, -1] + torch.arange(n, device=DEV)) % cfg.vocab_size
    frames = T(g["images"])
    img = torch.stack([frames[b % frames.shape[0]] * (1.0 - 0.05 * (b // frames.shape[0])) for b in range(n)], 0)
    noise = torch.cat([T(g["init_noise"]) * (1.0 - 0.1 * (b % 7)) for b in range(n)], 0)
    return ids, img, noise


def test_batch_of_three_takes_the_one_launch_sampler_and_matches_single_requests(setup):
    m, cfg, g, args = setup
    head = m.model.action_head.net
    ids, img, noise = _inputs(g, cfg, B)
    eager = m.inference_action_batch(ids, img, dict(args, use_graph=False), noise=noise)
    assert head.used_fused, "B = 3 in bf16 did not take the batched one-launch sampler"
    assert isinstance(eager, list) and len(eager) == B
    assert all(len(c) == cfg.chunk_size and len(c[0]) == cfg.action_dim for c in eager)
    assert eager[0] != eager[1] and eager[1] != eager[2]

    # (1) the sampler: the batched prefill's cognition rows, fed ONE AT A TIME to the single-request sampler, give each chunk exactly
    with torch.no_grad():
        plan = m.model._plans.get(ids, None, None, m.model.num_image_tokens(img.to(m.store.compute_dtype)),
                                  getattr(m.config, "tokenizer_model_max_length", None),
                                  getattr(m.config, "tokenizer_padding_side", "right"))
        S = plan.plan.shape[1]
        from dexbotic_amd import functional as Fn
        feats = m.model._extract_vision_features(img.to(m.store.compute_dtype))
        embeds = Fn.SpliceFn.apply(feats, m.store.params[m.model.llm.embed_name], m.store, m.model.llm.embed_name,
                                   plan.dev(m.store.device)["plan"]).view(B, S, -1)
        cognition = m.model.llm(embeds, None, None)[:, -1, :].float().unsqueeze(1)
        unc = m.store.w32("model.action_head.net.z_embedder.uncondition")
        for b in range(B):
            z = torch.cat([cognition[b:b + 1], unc.unsqueeze(0)], 0)
            assert head.fused_sampler_ok(2, cfg.chunk_size + 1)
            x = head.ddim_sample_fused(noise[b:b + 1], z, m.model.action_head.ddim_diffusion, 1.5)
            one = m._denorm(x[0].cpu().numpy(), args["action_norms"]).tolist()
            assert one == eager[b], f"request {b}: batched launch differs from the single sampler on the same cognition row by " \
                f"{rel_err(eager[b], one):.3e}"

    # (2) the whole request: each chunk against inference_action on that request alone (BF16_CHUNK_TOL above)
    singles = [m.inference_action(ids[b:b + 1], img[b:b + 1], dict(args, use_graph=False), noise=noise[b:b + 1]) for b in range(B)]
    for b in range(B):
        print(f"request {b}: B = 3 against B = 1, max-norm ratio {rel_err(eager[b], singles[b]):.3e}")
    for b in range(B):
        assert rel_err(eager[b], singles[b]) < BF16_CHUNK_TOL, (b, rel_err(eager[b], singles[b]))

    # (3) inference_action on the batch: still the reference's contract, sample 0's chunk
    assert m.inference_action(ids, img, dict(args, use_graph=False), noise=noise) == eager[0]


def test_second_call_of_a_batch_size_replays_its_graph_and_another_size_captures_anew(setup):
    m, cfg, g, args = setup
    m.__dict__.pop("_infer_graphs", None)
    ids, img, noise = _inputs(g, cfg, B)
    want = m.inference_action_batch(ids, img, dict(args, use_graph=False), noise=noise)
    for call in range(3):                                   # 1: eager warm-up on the private stream, 2: capture + replay, 3: replay
        assert m.inference_action_batch(ids, img, dict(args, use_graph=True), noise=noise) == want, call
        assert m.model.action_head.net.used_fused
    keys = list(m._infer_graphs)
    assert len(keys) == 1 and keys[0][1] == B and m._infer_graphs[keys[0]]["graph"] is not None
    ids2, img2, noise2 = _inputs(g, cfg, 2)
    want2 = m.inference_action_batch(ids2, img2, dict(args, use_graph=False), noise=noise2)
    for call in range(2):
        assert m.inference_action_batch(ids2, img2, dict(args, use_graph=True), noise=noise2) == want2
    assert sorted(k[1] for k in m._infer_graphs) == [2, B]
    assert all(e["graph"] is not None for e in m._infer_graphs.values())
    # the B = 3 graph is still there and still right
    assert m.inference_action_batch(ids, img, dict(args, use_graph=True), noise=noise) == want


def test_more_requests_than_a_launch_takes_are_still_answered(setup, monkeypatch):
    """above the group cap the batch runs on the per-step path: the same answers as that path gives request by request"""
    from dexbotic_amd import kernels as K
    m, cfg, g, args = setup
    n = K.DIT_SAMPLE_MAX_GROUPS + 1
    ids, img, noise = _inputs(g, cfg, n)
    got = m.inference_action_batch(ids, img, dict(args, use_graph=False), noise=noise)
    assert not m.model.action_head.net.used_fused
    assert len(got) == n and all(len(c) == cfg.chunk_size for c in got)
    monkeypatch.setenv("DXA_DIT_SAMPLER", "0")              # the single requests on the same (per-step) sampler
    for b in (0, 1, n - 1):
        one = m.inference_action(ids[b:b + 1], img[b:b + 1], dict(args, use_graph=False), noise=noise[b:b + 1])
        print(f"request {b} of {n}: per-step path at B = {n} against B = 1, max-norm ratio {rel_err(got[b], one):.3e}")
        assert rel_err(got[b], one) < BF16_CHUNK_TOL, (b, rel_err(got[b], one))
