"""The flow policies' serving route on the GPU: pi0's ``process_images`` against the reference's pixel tensors
(tests/golden/flow_serve_t1.npz), and FlowInferenceServer for pi0 / pi0.5 / DM0 at the tiny configurations of pi0_t1.npz /
pi05_t1.npz / dm0_t1.npz — the answer against the fixture-pinned formulas (tests/test_flow_serve_ref.py: answer_formulas) applied
to the request's own raw chunk, the Flask route, absent views padded (bit for bit a direct ``inference_action`` with a zero pixel
tensor) and left out (``views="present"``: the same chunk within the project's chunk tolerance), and the captured sampler's replay.

One model and one set of statistics per policy, built once and shared; every test that needs a fresh request shape has its own."""
import io
import json
import os

import numpy as np
import pytest
import torch

from . import muvla_weights as MW
from .flow_serve_tokenizers import dm0_tokenizer, pi0_tokenizer
from .helpers import assert_chunk_close
from .test_flow_serve_ref import answer_formulas, load

pytestmark = pytest.mark.gpu
DEV = "cuda"
POLICIES = ("pi0", "pi05", "dm0")
QUANTILES = {"pi0": False, "pi05": True, "dm0": True}
PROMPT = "pick up the red_block\nand place it"

_MODELS = {}


def build_pi0(golden_dir):
    from oracle import pi0_oracle as P
    from oracle.weights import make_weights, weights_crc
    from dexbotic_amd.model.pi0.pi0_arch import Pi0Config, Pi0ForCausalLM
    g = np.load(os.path.join(golden_dir, "pi0_t1.npz"), allow_pickle=False)
    c = P.Pi0OracleConfig()
    w = make_weights(P.pi0_shapes(c), int(g["seed"]))
    assert weights_crc(w) == int(g["weights_crc"])
    gem = dict(model_type="gemma", vocab_size=c.vocab_size, hidden_size=c.hidden_size, intermediate_size=c.intermediate_size,
               num_hidden_layers=c.num_hidden_layers, num_attention_heads=c.num_attention_heads,
               num_key_value_heads=c.num_key_value_heads, head_dim=c.head_dim, rope_theta=c.rope_theta, rms_norm_eps=c.rms_norm_eps)
    vis = dict(model_type="siglip_vision_model", hidden_size=c.v_hidden, intermediate_size=c.v_inter, num_hidden_layers=c.v_layers,
               num_attention_heads=c.v_heads, image_size=c.v_image, patch_size=c.v_patch, layer_norm_eps=c.v_eps)
    cfg = Pi0Config(vision_config=vis, action_config=dict(gem, hidden_size=c.a_hidden, intermediate_size=c.a_inter), llm_config=gem,
                    mm_projector_type="linear", action_dim=c.action_dim, chunk_size=c.chunk_size, compute_dtype="float32")
    m = Pi0ForCausalLM(cfg, device=DEV, train=False)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    return m


def build_from_list(golden_dir, fixture, cls, config):
    g = np.load(os.path.join(golden_dir, fixture), allow_pickle=False)
    w, _ = MW.from_fixture(g)
    m = cls(config(g, "float32"), device=DEV, train=False)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    return m


def model_and_stats(golden_dir, policy):
    """the policy's tiny fp32 model and its statistics lists (state at the model's action_dim, action of 7 entries)"""
    if policy not in _MODELS:
        if policy == "pi0":
            m = build_pi0(golden_dir)
        elif policy == "pi05":
            from dexbotic_amd.model import Pi05ForCausalLM
            from .test_pi05_config import config
            m = build_from_list(golden_dir, "pi05_t1.npz", Pi05ForCausalLM, config)
        else:
            from dexbotic_amd.model import DM0ForCausalLM
            from .test_dm0_config import config
            m = build_from_list(golden_dir, "dm0_t1.npz", DM0ForCausalLM, config)
        m.eval()
        rs = np.random.RandomState(7 + POLICIES.index(policy))
        A = m.config.action_dim
        names = ("min", "max") if QUANTILES[policy] else ("mean", "std")
        draw = lambda n: {names[0]: (-rs.uniform(0.5, 2.0, n)).tolist(), names[1]: rs.uniform(0.5, 2.0, n).tolist()}
        _MODELS[policy] = (m, {"state": draw(A), "action": draw(7)})
    return _MODELS[policy]


def server(golden_dir, policy, **kw):
    from dexbotic_amd.serve import FlowInferenceServer
    m, stats = model_and_stats(golden_dir, policy)
    tok = dm0_tokenizer(40) if policy == "dm0" else pi0_tokenizer(12)
    return FlowInferenceServer(m, tok, json.loads(json.dumps(stats)), policy=policy, **kw), m, stats


def pngs(n, side=40, seed=3):
    from dexbotic_amd.serve import encode_png
    rs = np.random.RandomState(seed)
    frames = [rs.randint(0, 256, size=(side, side, 3)).astype(np.uint8) for _ in range(n)]
    return frames, [encode_png(f) for f in frames]


def files(blobs):
    return [io.BytesIO(b) for b in blobs]


def noise_for(m, B, seed=5):
    c = m.config
    return torch.from_numpy(np.random.RandomState(seed).standard_normal((B, c.chunk_size, c.action_dim)).astype(np.float32)).to(DEV)


def states_for(B, dim=5, seed=9):
    return np.random.RandomState(seed).uniform(-1, 1, (B, dim))


def normalised(states, stats, quantiles, width):
    """PadState -> ActionNorm, restated (pinned to the fixture through answer_formulas' twin in the CPU file's transform test)"""
    s = np.pad(states, [(0, 0), (0, width - states.shape[1])])
    st = {k: np.asarray(v) for k, v in stats["state"].items()}
    if quantiles:
        return ((s - st["min"]) / (st["max"] - st["min"] + 1e-6) * 2.0 - 1.0).astype(np.float32)
    return ((s - st["mean"]) / (st["std"] + 1e-6)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ frames
def test_pi0_process_images_gives_the_references_pixel_tensors(golden_dir):
    """two frames of unequal sides (30 x 44, 44 x 30): black pad, Pillow-exact bicubic 44 -> 28, SigLIP mean / std — the per-frame
    launch path; then the same frame twice (one launch pair) and as a PIL image"""
    from PIL import Image
    from dexbotic_amd.model import DM0ForCausalLM, Pi05ForCausalLM
    from dexbotic_amd.model.dexbotic_arch import DexboticForCausalLM
    from dexbotic_amd.model.pi0.pi0_arch import Pi0ForCausalLM
    g = load(golden_dir)
    m, _ = model_and_stats(golden_dir, "pi0")
    f0, f1 = g["pix/frame0"], g["pix/frame1"]
    assert f0.shape != f1.shape and f0.dtype == np.uint8
    out = m.process_images([f0, f1])
    assert torch.is_tensor(out) and out.device.type == "cuda" and out.dtype == torch.float32
    d = np.abs(out.cpu().numpy() - g["pix/out"]).max()
    print(f"pi0 process_images vs the reference: max abs difference {d:.3e}")
    assert np.array_equal(out.cpu().numpy(), g["pix/out"])
    same = m.process_images([Image.fromarray(f1), torch.from_numpy(f1)])
    assert np.array_equal(same[0].cpu().numpy(), g["pix/out"][1]) and torch.equal(same[0], same[1])
    assert Pi05ForCausalLM.process_images is Pi0ForCausalLM.process_images
    assert DM0ForCausalLM.process_images is DexboticForCausalLM.process_images


# ---------------------------------------------------------------------------------------------------------- requests
@pytest.mark.parametrize("policy", POLICIES)
def test_response_equals_the_pinned_formulas_on_the_raw_chunk(golden_dir, policy):
    """2 samples x 2 views, states given, injected noise: the answer is ToNumpy -> ActionDenorm -> AbsoluteAction -> [..., :7] of the
    chunk the sampler returned, exactly; pi0 / pi0.5 answer with the first sample's chunk, DM0 with both"""
    s, m, stats = server(golden_dir, policy)
    _, blobs = pngs(4)
    states = states_for(2)
    ans = s.get_response(PROMPT, files(blobs), states=json.dumps(states.tolist()), batch_size=2, noise=noise_for(m, 2))
    raw, st = s.last_chunk, s.last_state
    c = m.config
    assert raw.shape == (2, c.chunk_size, c.action_dim) and raw.dtype == np.float32 and np.isfinite(raw).all()
    assert st.dtype == np.float32 and np.array_equal(st, normalised(states, stats, QUANTILES[policy], c.action_dim))
    want = answer_formulas(raw, st, stats, QUANTILES[policy])[..., :7]
    got = np.asarray(ans)
    assert got.shape == ((2, c.chunk_size, 7) if policy == "dm0" else (c.chunk_size, 7))
    assert ans == (want if policy == "dm0" else want[0]).tolist()
    # the statistics of 7 entries were padded in the server's mapping, and stay
    assert all(v.shape == (c.action_dim,) for v in s.norm_stats["action"].values())
    # a list of texts and a list of JSON strings are the same request
    ans2 = s.get_response([PROMPT, PROMPT], files(blobs), states=[json.dumps(r.tolist()) for r in states], batch_size="2",
                          noise=noise_for(m, 2))
    assert ans2 == ans


@pytest.mark.parametrize("policy", POLICIES)
def test_flask_route_equals_get_response(golden_dir, policy):
    s, m, stats = server(golden_dir, policy)
    _, blobs = pngs(4, seed=4)
    states = json.dumps(states_for(2, seed=10).tolist())
    client = s.create_app().test_client()
    torch.manual_seed(21)
    r = client.post("/process_frame", content_type="multipart/form-data",
                    data={"text": PROMPT, "states": states, "batch_size": "2",
                          "image": [(io.BytesIO(b), f"{i}.png") for i, b in enumerate(blobs)]})
    assert r.status_code == 200
    torch.manual_seed(21)
    want = s.get_response(PROMPT, files(blobs), states=states, batch_size=2)
    assert r.get_json() == {"response": want}
    # without states and batch_size: one sample, zero states
    torch.manual_seed(22)
    r = client.post("/process_frame", content_type="multipart/form-data",
                    data={"text": PROMPT, "image": [(io.BytesIO(b), f"{i}.png") for i, b in enumerate(blobs[:3])]})
    torch.manual_seed(22)
    assert r.status_code == 200 and r.get_json() == {"response": s.get_response(PROMPT, files(blobs[:3]))}
    A = m.config.action_dim                                                  # (the zero state is normalised like any other)
    assert np.array_equal(s.last_state, normalised(np.zeros((1, A), dtype=np.float32), stats, QUANTILES[policy], A))


def direct_call(s, m, frames, B, V, image_masks, noise, pad_to=None):
    """inference_action on the request's own tensors, launch by launch"""
    pix = m.process_images(frames).to(dtype=m.dtype)
    pix = pix.view(B, V, *pix.shape[1:])
    if pad_to is not None:
        pix = torch.cat([pix, torch.zeros(B, pad_to - V, *pix.shape[2:], device=DEV, dtype=pix.dtype)], dim=1)
    ids, am = s.tokenize([PROMPT] * B)
    return m.inference_action(input_ids=torch.from_numpy(ids).to(DEV), attention_mask=am, states=torch.from_numpy(s.last_state).to(DEV),
                              images=pix, image_masks=image_masks, noise=noise, use_graph=False)


@pytest.mark.parametrize("policy", POLICIES)
def test_absent_views_padded_and_present(golden_dir, policy, monkeypatch):
    """two of three views sent.  views="pad": bit for bit the direct call with a zero pixel tensor and image_masks [1, 1, 0].
    views="present": only the two views reach the model, masks all True, and the chunk is the padded one within
    helpers.assert_chunk_close's default tolerance (fp32)"""
    s, m, _ = server(golden_dir, policy, views="pad")
    frames, blobs = pngs(4, seed=6)
    states = json.dumps(states_for(2, seed=11).tolist())
    noise = noise_for(m, 2, seed=12)
    ans_pad = s.get_response(PROMPT, files(blobs), states=states, batch_size=2, noise=noise)
    padded = s.last_chunk
    masks = np.array([[True, True, False]] * 2)
    want = direct_call(s, m, frames, 2, 2, masks, noise, pad_to=3)
    assert np.array_equal(padded, want.cpu().numpy())

    p, _, _ = server(golden_dir, policy, views="present")
    seen = []
    real = m.inference_action
    monkeypatch.setattr(m, "inference_action", lambda **kw: (seen.append((tuple(kw["images"].shape), kw["image_masks"].copy())),
                                                              real(**kw))[1])
    ans_present = p.get_response(PROMPT, files(blobs), states=states, batch_size=2, noise=noise)
    monkeypatch.undo()
    assert seen[0][0][:2] == (2, 2) and seen[0][1].shape == (2, 2) and seen[0][1].all()
    d = np.abs(p.last_chunk - padded).max()
    print(f"{policy}: views='present' against 'pad', max abs difference of the chunk {d:.3e}")
    assert_chunk_close(p.last_chunk, padded, what=f"{policy} chunk without the empty view's rows")
    assert np.asarray(ans_present).shape == np.asarray(ans_pad).shape
    # all three views sent: the two modes are one request
    _, blobs3 = pngs(6, seed=6)
    a = s.get_response(PROMPT, files(blobs3), states=states, batch_size=2, noise=noise)
    b = p.get_response(PROMPT, files(blobs3), states=states, batch_size=2, noise=noise)
    assert a == b
    # surplus views are cut
    _, blobs4 = pngs(8, seed=6)
    s4 = s.get_response(PROMPT, files(blobs4), states=states, batch_size=2, noise=noise)
    first3 = [blobs4[i] for i in (0, 1, 2, 4, 5, 6)]
    assert s4 == s.get_response(PROMPT, files(first3), states=states, batch_size=2, noise=noise)


@pytest.mark.parametrize("policy", POLICIES)
def test_second_request_of_a_shape_replays_the_captured_sampler(golden_dir, policy):
    """a request shape nothing else here uses (a server of ONE view, one sample): the first request runs the Euler loop launch by
    launch, the second captures it and replays — the same bits with the same noise — and holds a graph for the third"""
    s, m, _ = server(golden_dir, policy, num_images=1)
    _, blobs = pngs(1, seed=8)
    noise = noise_for(m, 1, seed=13)
    cache = m.__dict__.get("_sampler_graphs")
    before = set(cache.entries) if cache is not None else set()
    first = s.get_response(PROMPT, files(blobs), noise=noise)
    chunk1 = s.last_chunk
    new = set(m._sampler_graphs.entries) - before
    assert len(new) == 1 and m._sampler_graphs.entries[next(iter(new))]["graph"] is None
    second = s.get_response(PROMPT, files(blobs), noise=noise)
    assert set(m._sampler_graphs.entries) - before == new and m._sampler_graphs.entries[next(iter(new))]["graph"] is not None
    assert second == first and np.array_equal(s.last_chunk, chunk1)
    third = s.get_response(PROMPT, files(blobs), noise=noise_for(m, 1, seed=14))
    assert third != first and np.isfinite(s.last_chunk).all()
    assert s.inference_single(files(blobs), PROMPT) is not None and s.last_ms > 0
