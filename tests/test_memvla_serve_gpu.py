"""serve.MemVLAInferenceServer: MemVLA's /process_frame wire format (text, image files, episode_first_frame) and its batched form
(batch_size, slots, lists of texts and flags), against the model calls a request decomposes into."""
import io
import json
import os
import types

import numpy as np
import pytest
import torch

from oracle import cogact_oracle as O
from oracle import memvla_oracle as M
from oracle.weights import make_weights, weights_crc

from .helpers import product_config

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHORT, LONG = "pick up the red block", "put the green cup on the top shelf please"
NORMS = {"min": [-1.0, -2.0, -3.0, -1.0, -1.0, -1.0, 0.0], "max": [1.0, 2.0, 3.0, 1.0, 1.0, 1.0, 1.0]}


def build(golden_dir):
    """the recipe of tests/test_memvla_gpu.py::build, tiny fixture, fp32, served"""
    from dexbotic_amd.model.memvla.memvla_arch import MemVLAConfig, MemVLAForCausalLM
    g = np.load(os.path.join(golden_dir, "memvla_t1.npz"), allow_pickle=False)
    cfg = O.OracleConfig()
    w = make_weights(M.memvla_shapes(cfg, int(g["per_token_size"])), int(g["seed"]))
    assert weights_crc(w) == int(g["weights_crc"])
    base = product_config(cfg, "float32")
    mc = MemVLAConfig(llm_config=base.llm_config, mm_vision_tower=base.mm_vision_tower, mm_projector_type="mlp2x_gelu",
                      action_model_type="DiT-T", action_dim=cfg.action_dim, chunk_size=cfg.chunk_size,
                      compute_dtype="float32", per_token_size=int(g["per_token_size"]), dataloader_type="group", group_size=3,
                      mem_length=int(g["mem_length"]), retrieval_layers=2, use_timestep_pe=True, fusion_type="gate",
                      consolidate_type="tome", retrieval_dropout=0.0)
    m = MemVLAForCausalLM(mc, device=DEV, train=False)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    m.eval()
    return cfg, m


@pytest.fixture(scope="module")
def served(golden_dir):
    from dexbotic_amd.serve import MemVLAInferenceServer, encode_png
    from oracle import image_oracle as IO
    cfg, m = build(golden_dir)
    _, twin = build(golden_dir)                                  # the same weights, driven by hand

    class Tok:
        bos_token_id = None

        def __call__(self, text):
            return types.SimpleNamespace(input_ids=[3 + (sum(map(ord, wd)) % (cfg.vocab_size - 3)) for wd in text.split()])

    srv = MemVLAInferenceServer(m, Tok(), norm_stats=NORMS, num_slots=4)
    blobs = [encode_png(IO.synthetic_image(90, 120, 40 + i)) for i in range(6)]
    gen = torch.Generator().manual_seed(8)
    noise = torch.randn((6, cfg.chunk_size, cfg.action_dim), generator=gen).to(DEV)
    return srv, m, twin, cfg, Tok(), blobs, noise


def files(blobs):
    return [io.BytesIO(b) for b in blobs]


def _by_hand(srv, m, tok, texts, blobs):
    from PIL import Image
    from dexbotic_amd.tokenization.tokenization import tokenizer_image_token
    pix = m.process_images([Image.open(f).convert("RGB") for f in files(blobs)]).to(dtype=m.dtype)
    ids = torch.stack([tokenizer_image_token(srv.build_prompt(t), tok, return_tensors="pt") for t in texts], 0).to(DEV)
    return ids, pix


def test_a_single_request_equals_inference_action(served):
    srv, m, twin, cfg, tok, blobs, noise = served
    for f, flag in enumerate(("True", "False", "False")):
        ids, pix = _by_hand(srv, twin, tok, [SHORT], blobs[f:f + 1])
        want = twin.inference_action(ids, pix, flag, dict(srv.inference_args), noise=noise[f:f + 1])
        got = srv.get_response(SHORT, files(blobs[f:f + 1]), flag, noise=noise[f:f + 1])
        assert got == want and np.asarray(got).shape == (cfg.chunk_size, cfg.action_dim), f
    assert m.cur_timestep == 3 and twin.cur_timestep == 3
    with pytest.raises(ValueError):
        srv.get_response(SHORT, files(blobs[:1]), "true")
    with pytest.raises(ValueError):
        srv.get_response(SHORT, files(blobs[:1]), None)


def test_a_batched_request_with_two_prompt_lengths_equals_the_calls_it_decomposes_into(served):
    srv, m, twin, cfg, tok, blobs, noise = served
    m.model.per_cog_mem_bank.reset()
    twin.model.per_cog_mem_bank.reset()
    texts, slots = [LONG, SHORT, LONG], [3, 0, 1]
    assert len(tok(LONG).input_ids) != len(tok(SHORT).input_ids)
    for f, flags in enumerate((["True", "True", "True"], ["False", "True", "False"], "False")):
        use = blobs[f:f + 3]
        fl = [flags] * 3 if isinstance(flags, str) else flags
        want = [None] * 3
        for rows in ([1], [0, 2]):                               # the shorter prompt first, as the server walks the lengths
            ids, pix = _by_hand(srv, twin, tok, [texts[b] for b in rows], [use[b] for b in rows])
            out = twin.inference_action_batch(ids, pix, [fl[b] for b in rows], dict(srv.inference_args),
                                              slots=[slots[b] for b in rows], num_slots=4, noise=noise[f:f + 3][rows])
            for b, c in zip(rows, out):
                want[b] = c
        # the list forms: python lists and the JSON text a form field carries; batch_size as the form's string
        if f == 1:
            got = srv.get_response(json.dumps(texts), files(use), json.dumps(flags), batch_size="3", slots=json.dumps(slots),
                                   noise=noise[f:f + 3])
        else:
            got = srv.get_response(texts, files(use), flags, batch_size=3, slots=slots, noise=noise[f:f + 3])
        assert got == want and np.asarray(got).shape == (3, cfg.chunk_size, cfg.action_dim), f
        assert got[0] != got[2]
    assert m.model.per_cog_mem_bank.episode_time == [2, 3, 0, 3] == twin.model.per_cog_mem_bank.episode_time


def test_flask_route_carries_the_memvla_fields(served):
    srv, m, twin, cfg, tok, blobs, noise = served
    client = srv.create_app().test_client()
    m.model.per_cog_mem_bank.reset()
    torch.manual_seed(13)
    want = srv.get_response(SHORT, files(blobs[:2]), "True", batch_size=2, slots=[2, 1])
    m.model.per_cog_mem_bank.reset()
    torch.manual_seed(13)
    r = client.post("/process_frame", content_type="multipart/form-data",
                    data={"text": SHORT, "batch_size": "2", "episode_first_frame": "True", "slots": "[2, 1]",
                          "image": [(io.BytesIO(b), f"{i}.png") for i, b in enumerate(blobs[:2])]})
    assert r.status_code == 200 and r.get_json() == {"response": want}
    torch.manual_seed(14)
    want = srv.get_response(SHORT, files(blobs[:1]), "True")
    torch.manual_seed(14)
    r = client.post("/process_frame", content_type="multipart/form-data",
                    data={"text": SHORT, "episode_first_frame": "True", "image": [(io.BytesIO(blobs[0]), "0.png")]})
    assert r.status_code == 200 and r.get_json() == {"response": want}


def test_malformed_lists_and_counts_are_refused_before_the_model_runs(served):
    srv, m, twin, cfg, tok, blobs, noise = served
    bank = m.model.per_cog_mem_bank
    bank.reset()
    bad = [
        dict(text=SHORT, n=3, eff="True", batch_size=2),                              # 3 images, 2 samples
        dict(text=[SHORT] * 3, n=2, eff="True", batch_size=2),                        # 3 texts, 2 samples
        dict(text=json.dumps([SHORT]), n=2, eff="True", batch_size=2),
        dict(text="[not json", n=2, eff="True", batch_size=2),
        dict(text=SHORT, n=2, eff='["True"]', batch_size=2),                          # one flag, 2 samples
        dict(text=SHORT, n=2, eff=["True", "maybe"], batch_size=2),
        dict(text=SHORT, n=2, eff='["True", 1]', batch_size=2),
        dict(text=SHORT, n=2, eff="True", batch_size=2, slots="[0]"),
        dict(text=SHORT, n=2, eff="True", batch_size=2, slots="[0, 0]"),
        dict(text=SHORT, n=2, eff="True", batch_size=2, slots='[0, "1"]'),
        dict(text=SHORT, n=2, eff="True", batch_size=2, slots="[0, 1"),
        dict(text=SHORT, n=2, eff="True", batch_size=2, slots="1"),
        dict(text=SHORT, n=2, eff="True", batch_size=2, slots=[-1, 0]),
        dict(text=SHORT, n=2, eff="True", batch_size="two"),
        dict(text=SHORT, n=2, eff="True", batch_size=0),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            srv.get_response(kw["text"], files(blobs[:kw["n"]]), kw["eff"], batch_size=kw["batch_size"], slots=kw.get("slots"))
    assert bank.episode_time == []
    with pytest.raises(ValueError):                                # a slot the server's num_slots = 4 does not hold
        srv.get_response(SHORT, files(blobs[:2]), "True", batch_size=2, slots=[0, 4])
    assert bank.episode_time == []
