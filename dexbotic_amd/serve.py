"""The action-inference wire format: POST /process_frame, multipart form with a `text` field and one or more `image`
PNG files, answered with {"response": [[...7 floats...] x chunk]} — dexbotic/exp/base_exp.py:638-653 (route),
dexbotic/exp/cogact_exp.py:146-177 (_get_response), dexbotic/client.py:33-61 (the caller).

Only PNG decoding and prompt formatting stay on the host; the frames go to the MI355X as uint8 and are padded,
resized, cropped and normalised there (DexboticForCausalLM.process_images -> dxa_image_preprocess).

``InferenceServer`` speaks the CogACT format (one sample, ``inference_action(ids, pix, args)``; with the optional ``batch_size``
field several, ``inference_action_batch``); ``FlowInferenceServer`` the batched
format of the flow-matching policies pi0 / pi0.5 / DM0 (``states`` and ``batch_size`` beside the frames, absent views masked);
``MemVLAInferenceServer`` MemVLA's (``episode_first_frame`` beside the frames; with ``batch_size`` one frame of several running
episodes, each in its own slot of the memory bank)."""
from __future__ import annotations

import io
import os
import time
from typing import Callable, List, Optional

import torch

from .constants import DEFAULT_IMAGE_TOKEN, IMAGE_TOKEN_INDEX
from .tokenization import conversation as conversation_lib
from .tokenization.tokenization import tokenizer_image_token


class InferenceServer:
    """model: anything with process_images / inference_action / device / dtype / config.chat_template"""

    def __init__(self, model, tokenizer, norm_stats: Optional[dict] = None, port: int = 7891, cfg_scale: float = 1.5,
                 num_ddim_steps: int = 10, assistant_stub: Optional[str] = " ", log: Optional[Callable[[str], None]] = None):
        self.model, self.tokenizer, self.norm_stats, self.port = model, tokenizer, norm_stats, port
        self.inference_args = {"cfg_scale": cfg_scale, "num_ddim_steps": num_ddim_steps, "action_norms": norm_stats}
        self.assistant_stub = assistant_stub                     # cogact_exp.py:159 appends ' ', base_exp.py:683 None
        self.log = log
        self.last_ms = None
        # the host side of a request is one PNG decode and a few hundred KB of byte shuffling: torch's intra-op pool (sized by the
        # host's logical CPUs) is held inside the container's CPU quota, or its spinning workers get the whole process throttled
        # in the middle of a request (hostcpu.py; POST /process_frame p90 55 -> 22 ms)
        from .hostcpu import limit_host_threads
        self.host_threads = limit_host_threads(cap=8)
        self.stage_ms = {} if os.environ.get("DXA_SERVE_STAGES") else None

    # ---- one request ------------------------------------------------------------------------------------------
    def build_prompt(self, text: str) -> str:
        template = getattr(self.model.config, "chat_template", "dexbotic")
        conv = conversation_lib.conv_templates[template].copy()
        conv.append_message(conv.roles[0], DEFAULT_IMAGE_TOKEN + "\n" + text)
        conv.append_message(conv.roles[1], self.assistant_stub)
        return conv.get_prompt()

    def get_response(self, text, images: List, batch_size: Optional[int] = None) -> list:
        """images: file-like objects / paths holding PNG (or anything PIL opens).  cogact_exp.py:146-177.
        ``batch_size`` > 1: the request holds that many samples — images sample-major (as FlowInferenceServer), ``text`` one string
        for all of them or a list (or JSON list) of ``batch_size`` strings — and the answer is [batch_size][chunk][action_dim]."""
        if batch_size is not None and int(batch_size) > 1:
            return self._get_response_batch(text, images, int(batch_size))
        from PIL import Image
        t0 = time.monotonic()
        stages = self.stage_ms if self.stage_ms is not None else None      # tuning: per-stage times (a device sync per stage)

        def mark(name, t_prev):
            if stages is None:
                return t_prev
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            t = time.monotonic()
            stages.setdefault(name, []).append(round(1e3 * (t - t_prev), 2))
            return t
        frames = [Image.open(f).convert("RGB") for f in images]
        t = mark("png_decode", t0)
        pix = self.model.process_images(frames).to(dtype=self.model.dtype)
        if len(frames) > 1:
            pix = pix.unsqueeze(0)                               # [1, views, 3, H, W]
        t = mark("process_images", t)
        ids = tokenizer_image_token(self.build_prompt(text), self.tokenizer, IMAGE_TOKEN_INDEX, return_tensors="pt")
        ids = ids.unsqueeze(0).to(self.model.device)
        t = mark("prompt", t)
        with torch.no_grad():
            out = self.model.inference_action(ids, pix, dict(self.inference_args))
        out = out.tolist() if hasattr(out, "tolist") else out
        mark("inference_action", t)
        self.last_ms = 1e3 * (time.monotonic() - t0)
        if self.log:
            self.log(f"process_frame: {len(frames)} view(s), {self.last_ms:.1f} ms")
        return out

    def _get_response_batch(self, text, images: List, B: int) -> list:
        """B samples in one request: one process_images call for all frames and inference_action_batch per prompt length (the
        prefill takes no padding mask: samples whose prompts tokenise to the same length share a batch — always, with one text)"""
        import json
        from PIL import Image
        t0 = time.monotonic()
        if isinstance(text, str) and text.lstrip().startswith("["):
            try:
                parsed = json.loads(text)
                text = parsed if isinstance(parsed, list) else text
            except ValueError:
                pass
        texts = [text] * B if isinstance(text, str) else list(text)
        if len(texts) != B or not all(isinstance(t, str) for t in texts):
            raise ValueError(f"process_frame: batch_size {B} needs one text or a list of {B} strings, got {len(texts)} entries")
        if len(images) == 0 or len(images) % B != 0:
            raise ValueError(f"process_frame: {len(images)} image(s) do not divide into batch_size {B} samples")
        views = len(images) // B
        frames = [Image.open(f).convert("RGB") for f in images]
        pix = self.model.process_images(frames).to(dtype=self.model.dtype)
        if views > 1:
            pix = pix.view(B, views, *pix.shape[1:])
        ids = [tokenizer_image_token(self.build_prompt(t), self.tokenizer, IMAGE_TOKEN_INDEX, return_tensors="pt") for t in texts]
        out = [None] * B
        with torch.no_grad():
            for n in sorted({int(i.numel()) for i in ids}):
                rows = [b for b in range(B) if int(ids[b].numel()) == n]
                chunks = self.model.inference_action_batch(torch.stack([ids[b] for b in rows], 0).to(self.model.device),
                                                           pix[rows] if len(rows) < B else pix, dict(self.inference_args))
                for b, c in zip(rows, chunks):
                    out[b] = c.tolist() if hasattr(c, "tolist") else c
        self.last_ms = 1e3 * (time.monotonic() - t0)
        if self.log:
            self.log(f"process_frame: {B} sample(s) x {views} view(s), {self.last_ms:.1f} ms")
        return out

    def inference_single(self, image_path, prompt: str) -> list:
        """the exp scripts' ``--task inference_single`` (playground/benchmarks/libero/libero_cogact.py:70-72):
        ``_get_response(prompt, [image_path])`` on one image file (or a list of view files)"""
        paths = [image_path] if isinstance(image_path, (str, bytes)) or hasattr(image_path, "read") else list(image_path)
        return self.get_response(prompt, paths)

    # ---- Flask plumbing ---------------------------------------------------------------------------------------
    def create_app(self):
        from flask import Flask, jsonify, request
        app = Flask(__name__)

        def process_frame():
            files = [io.BytesIO(f.read()) for f in request.files.getlist("image")]
            bs = request.form.get("batch_size")
            return jsonify({"response": self.get_response(request.form.get("text"), files, int(bs) if bs else None)})

        app.add_url_rule("/process_frame", "process_frame", process_frame, methods=["POST"])
        return app

    def run(self) -> None:
        self.create_app().run(host="0.0.0.0", port=self.port, debug=False, threaded=False)


def _json_list(value, n: int, what: str, kind) -> Optional[list]:
    """a form field that is one value for all n samples or a list (or the JSON text of a list) of n: -> the list, or None when
    ``value`` is a single value.  Malformed JSON, another length or entries that are no ``kind``: ValueError."""
    import json
    if isinstance(value, str):
        if not value.lstrip().startswith("["):
            return None
        try:
            value = json.loads(value)
        except ValueError as e:
            raise ValueError(f"process_frame: {what} is not a JSON list: {e}") from None
    if not isinstance(value, (list, tuple)):
        return None
    if len(value) != n or not all(isinstance(v, kind) and not isinstance(v, bool) for v in value):
        raise ValueError(f"process_frame: {what} needs {n} entries of {getattr(kind, '__name__', kind)}, got {list(value)!r}")
    return list(value)


class MemVLAInferenceServer(InferenceServer):
    """POST /process_frame in MemVLA's wire format — MemVLAInferenceConfig (memvla_exp.py:309-358): form fields ``text``, ``image``
    files and ``episode_first_frame`` ('True' on the first frame of an episode), answered {"response": [chunk][action_dim]} by
    ``inference_action``: one frame of the ONE episode the model is running.

    With the optional ``batch_size`` = R the request holds one frame of R running episodes (several robots or simulator instances
    on one set of weights): images sample-major, ``text`` one string for all or a (JSON) list of R, ``episode_first_frame`` one
    string for all or a (JSON) list of R, ``slots`` an optional (JSON) list of R distinct ints — the episode slot of each sample,
    default 0 .. R-1 — and the answer is {"response": [R][chunk][action_dim]} in request order (MemVLAForCausalLM.
    inference_action_batch).  The prefill takes no padding mask: samples whose prompts tokenise to different lengths are served
    as one call per length, each on its own slot ids — a slot is stepped only by the call that names it.  ``num_slots``: how many
    episodes the model holds (default: what the first batched request needs).  The single episode and the slots share the model,
    not an episode, and a single-frame request with 'True' resets the whole memory bank, the slots included."""

    def __init__(self, model, tokenizer, norm_stats: Optional[dict] = None, port: int = 7891, cfg_scale: float = 1.5,
                 num_ddim_steps: int = 10, num_slots: Optional[int] = None, log: Optional[Callable[[str], None]] = None):
        super().__init__(model, tokenizer, norm_stats, port, cfg_scale, num_ddim_steps, " ", log)
        self.num_slots = num_slots

    def parse_request(self, text, n_images: int, episode_first_frame, batch_size, slots=None):
        """the host-only part of a batched request: -> (R, views per sample, R texts, R flags, R slot ids)"""
        try:
            R = int(batch_size)
        except (TypeError, ValueError):
            raise ValueError(f"process_frame: batch_size {batch_size!r} is not a number") from None
        if R < 1 or n_images < R or n_images % R != 0:
            raise ValueError(f"process_frame: {n_images} image(s) do not divide into batch_size {R} samples")
        texts = _json_list(text, R, "text", str)
        if texts is None:
            if not isinstance(text, str):
                raise ValueError(f"process_frame: text is one string or a list of {R} strings")
            texts = [text] * R
        flags = _json_list(episode_first_frame, R, "episode_first_frame", str)
        if flags is None:
            flags = [episode_first_frame] * R
        if any(f not in ("True", "False") for f in flags):
            raise ValueError(f"process_frame: episode_first_frame is 'True' or 'False' (one for all or a list of {R}), got {flags!r}")
        ids = list(range(R)) if slots is None else _json_list(slots, R, "slots", int)
        if ids is None:
            raise ValueError(f"process_frame: slots is a list of {R} ints, got {slots!r}")
        if len(set(ids)) != R or min(ids) < 0:
            raise ValueError(f"process_frame: slots {ids} are not {R} distinct non-negative ints")
        return R, n_images // R, texts, flags, ids

    def get_response(self, text, images: List, episode_first_frame, batch_size=None, slots=None, noise=None) -> list:
        """images: file-like objects / paths holding PNG (or anything PIL opens).  Without ``batch_size``: memvla_exp.py:317-358,
        [chunk][action_dim].  With it: [batch_size][chunk][action_dim], see the class.  ``noise`` injects the sampler's initial
        draw ([1 | batch_size, chunk, action_dim])."""
        from PIL import Image
        t0 = time.monotonic()
        images = list(images)
        kw = {} if noise is None else {"noise": noise}
        if batch_size is None:
            if episode_first_frame not in ("True", "False"):
                raise ValueError(f"process_frame: episode_first_frame is 'True' or 'False', got {episode_first_frame!r}")
            frames = [Image.open(f).convert("RGB") for f in images]
            pix = self.model.process_images(frames).to(dtype=self.model.dtype)
            if len(frames) > 1:
                pix = pix.unsqueeze(0)                               # [1, views, 3, H, W]
            ids = tokenizer_image_token(self.build_prompt(text), self.tokenizer, IMAGE_TOKEN_INDEX, return_tensors="pt")
            with torch.no_grad():
                out = self.model.inference_action(ids.unsqueeze(0).to(self.model.device), pix, episode_first_frame,
                                                  dict(self.inference_args), **kw)
            self.last_ms = 1e3 * (time.monotonic() - t0)
            if self.log:
                self.log(f"process_frame[memvla]: {len(frames)} view(s), first frame {episode_first_frame}, {self.last_ms:.1f} ms")
            return out
        R, views, texts, flags, slot_ids = self.parse_request(text, len(images), episode_first_frame, batch_size, slots)
        frames = [Image.open(f).convert("RGB") for f in images]
        pix = self.model.process_images(frames).to(dtype=self.model.dtype)
        if views > 1:
            pix = pix.view(R, views, *pix.shape[1:])
        ids = [tokenizer_image_token(self.build_prompt(t), self.tokenizer, IMAGE_TOKEN_INDEX, return_tensors="pt") for t in texts]
        out = [None] * R
        with torch.no_grad():
            for n in sorted({int(i.numel()) for i in ids}):        # one call per prompt length, each on its own slots
                rows = [b for b in range(R) if int(ids[b].numel()) == n]
                sub = {} if noise is None else {"noise": noise[rows]}
                chunks = self.model.inference_action_batch(
                    torch.stack([ids[b] for b in rows], 0).to(self.model.device), pix[rows] if len(rows) < R else pix,
                    [flags[b] for b in rows], dict(self.inference_args), slots=[slot_ids[b] for b in rows],
                    num_slots=self.num_slots, **sub)
                for b, c in zip(rows, chunks):
                    out[b] = c
        self.last_ms = 1e3 * (time.monotonic() - t0)
        if self.log:
            self.log(f"process_frame[memvla]: {R} episode(s) x {views} view(s), slots {slot_ids}, {self.last_ms:.1f} ms")
        return out

    def inference_single(self, image_path, prompt: str, episode_first_frame: str = "True") -> list:
        paths = [image_path] if isinstance(image_path, (str, bytes)) or hasattr(image_path, "read") else list(image_path)
        return self.get_response(prompt, paths, episode_first_frame)

    def create_app(self):
        from flask import Flask, jsonify, request
        app = Flask(__name__)

        def process_frame():
            files = [io.BytesIO(f.read()) for f in request.files.getlist("image")]
            answer = self.get_response(request.form.get("text"), files, request.form.get("episode_first_frame"),
                                       batch_size=request.form.get("batch_size"), slots=request.form.get("slots"))
            return jsonify({"response": answer})

        app.add_url_rule("/process_frame", "process_frame", process_frame, methods=["POST"])
        return app


def read_normalization_stats(path: Optional[str]) -> dict:
    """``norm_stats.json`` of a checkpoint directory as the reference's servers read it (pi0_exp.py:378-386): a top-level
    ``"norm_stats"`` key is unwrapped, the lists become float64 arrays; no file -> {"min": -1, "max": 1} (statistics for no key)"""
    import json
    from .data.dataset.transform.common import ToNumpy
    if path is None or not os.path.exists(path):
        return {"min": -1, "max": 1}
    with open(path) as f:
        stats = json.load(f)
    return ToNumpy()(stats.get("norm_stats", stats))


# policy -> (prompt tokeniser, quantile statistics, the whole batch answered)
_FLOW_POLICIES = {"pi0": ("pi0", False, False), "pi05": ("pi0", True, False), "dm0": ("dm0", True, True)}
_FLOW_MODEL_TYPES = {"dexbotic_pi0": "pi0", "dexbotic_pi05": "pi05", "dexbotic_dm0": "dm0"}


class FlowInferenceServer:
    """POST /process_frame for the flow-matching policies — Pi0InferenceConfig._get_response (pi0_exp.py:397-514), Pi05InferenceConfig
    (pi05_exp.py:98-136: quantile statistics), DM0InferenceConfig (dm0_exp.py:404-521: its own tokeniser, the whole batch answered).
    Form fields: ``text``, ``image`` files (``batch_size`` groups of equal length, sample-major), ``states`` (JSON), ``batch_size``.

    A request is host work (PNG decode, tokeniser, a few dozen floats of numpy) around the device work that exists: ONE
    ``process_images`` call for all its frames and the policy's sampler, whose Euler loop is a captured graph per request shape
    (model/mot.py) — the next request of that shape replays it.  Everything small goes up through pinned memory (hostcpu.upload) and
    nothing is read back before the chunk.

    ``views``: what a request with fewer than ``num_images`` views per sample turns into.  "pad" (default, the reference's
    arithmetic): zero pixel tensors with ``image_masks`` False — the tower and the prefix still run over them.  "present": the
    views that exist alone, masks all True — the policies take the camera count from ``images.shape[1]``, masked keys are invisible
    and positions count valid tokens only, so the chunk is the same up to rounding without the rows of the empty views.

    After a request ``last_chunk`` holds the sampler's raw [B, chunk, A] float32 chunk and ``last_state`` the normalised state rows
    the model saw (both host numpy): what the answer was computed from."""

    def __init__(self, model, tokenizer, norm_stats: Optional[dict] = None, *, policy: str, num_images: int = 3,
                 non_delta_mask=(6,), action_dim: int = 7, port: int = 7891, views: str = "pad",
                 log: Optional[Callable[[str], None]] = None):
        from .data.dataset.transform.action import ActionNorm, PadState
        from .data.dataset.transform.common import Pipeline, ToNumpy, ToTensor
        from .data.dataset.transform.output import AbsoluteAction, ActionDenorm
        from .tokenization.process import DM0Tokenization, Pi0Tokenization
        if policy not in _FLOW_POLICIES:
            raise ValueError(f"policy {policy!r}: one of {sorted(_FLOW_POLICIES)}")
        if views not in ("pad", "present"):
            raise ValueError(f"views {views!r}: 'pad' or 'present'")
        tok_kind, quantiles, self.answer_batch = _FLOW_POLICIES[policy]
        self.model, self.tokenizer, self.policy, self.port, self.log = model, tokenizer, policy, port, log
        self.num_images, self.non_delta_mask, self.action_dim, self.views = num_images, list(non_delta_mask), action_dim, views
        # lists -> float64 arrays (what read_normalization_stats gives); ActionDenorm pads these arrays in place
        self.norm_stats = ToNumpy()(norm_stats if norm_stats is not None else {"min": -1, "max": 1})
        self.tokenization_func = (DM0Tokenization if tok_kind == "dm0" else Pi0Tokenization)(tokenizer)
        self.input_transform = Pipeline([PadState(ndim=model.config.action_dim, axis=-1),
                                         ActionNorm(statistic_mapping=self.norm_stats, strict=False, use_quantiles=quantiles),
                                         ToTensor()])
        self.output_transform = Pipeline([ToNumpy(),
                                          ActionDenorm(statistic_mapping=self.norm_stats, strict=False, use_quantiles=quantiles),
                                          AbsoluteAction()])
        self.last_ms = self.last_chunk = self.last_state = None
        from .hostcpu import limit_host_threads                 # as InferenceServer: the intra-op pool inside the CPU quota
        self.host_threads = limit_host_threads(cap=8)
        self.stage_ms = {} if os.environ.get("DXA_SERVE_STAGES") else None

    @classmethod
    def from_pretrained(cls, path: str, tokenizer=None, norm_stats: Optional[dict] = None, device=None, **kwargs):
        """checkpoint directory -> server: the policy from ``config.json``'s ``model_type``, the tokenizer from the directory (slow
        tokenizer, as the reference loads it) unless given, the statistics from ``norm_stats.json`` unless given"""
        import json
        from . import from_pretrained as load_model
        with open(os.path.join(path, "config.json")) as f:
            model_type = json.load(f).get("model_type")
        if model_type not in _FLOW_MODEL_TYPES:
            raise ValueError(f"{path}: model_type {model_type!r} is not a flow policy ({sorted(_FLOW_MODEL_TYPES)})")
        policy = _FLOW_MODEL_TYPES[model_type]
        model = load_model(path, **({} if device is None else {"device": device}))
        model.eval()
        if tokenizer is None:
            from transformers import AutoTokenizer
            tokenizer = AutoTokenizer.from_pretrained(path, use_fast=False, trust_remote_code=policy == "dm0")
        if norm_stats is None:
            norm_stats = read_normalization_stats(os.path.join(path, "norm_stats.json"))
        return cls(model, tokenizer, norm_stats, policy=policy, **kwargs)

    # ---- one request ------------------------------------------------------------------------------------------
    def parse_request(self, text, n_images: int, states=None, batch_size=1):
        """the host-only part: -> (batch_size, views per sample, one prompt per sample, states [batch_size, d]).  What the reference
        asserts is a ValueError here."""
        import json
        import numpy as np
        B = int(batch_size)
        if B < 1 or n_images < B or n_images % B != 0:
            raise ValueError(f"Number of images {n_images} is not divisible by batch size {B}")
        texts = [text] * B if isinstance(text, str) else list(text)
        if len(texts) != B:
            raise ValueError(f"Batch inference requires one text or a list of {B} texts, but got {len(texts)}.")
        if states is None:
            batch_states = np.zeros((B, self.model.config.action_dim), dtype=np.float32)
        else:
            if isinstance(states, str):
                batch_states = np.array(json.loads(states))
                if batch_states.ndim == 1:
                    batch_states = batch_states[None]
            elif isinstance(states, (list, tuple)) and all(isinstance(s, str) for s in states):
                batch_states = np.array([json.loads(s) for s in states])
            else:
                raise ValueError(f"states: a JSON string or a list of JSON strings, got {type(states).__name__}")
            if batch_states.ndim != 2 or batch_states.shape[0] != B:
                raise ValueError(f"Batch inference requires states to be a list with length {B}, but got shape {batch_states.shape}.")
        return B, n_images // B, texts, batch_states

    def tokenize(self, texts: List[str]):
        """-> input_ids int64 [B, model_max_length], attention_mask bool (ids != pad_token_id), host numpy"""
        import numpy as np
        turn = (lambda p: [{"from": "human", "value": p}]) if self.policy == "dm0" else (lambda p: [{"value": p}])
        ids = np.array([self.tokenization_func(turn(p))["input_ids"] for p in texts])
        return ids, ids != self.tokenizer.pad_token_id

    def get_response(self, text, images: List, states=None, batch_size=1, noise=None) -> list:
        """images: file-like objects / paths holding PNG (or anything PIL opens), sample-major.  ``noise`` [B, chunk, A] injects the
        sampler's initial draw.  -> [chunk][action_dim] of the first sample (pi0, pi0.5) or [B][chunk][action_dim] (dm0)."""
        import numpy as np
        from PIL import Image
        from . import hostcpu
        t0 = time.monotonic()
        stages = self.stage_ms

        def mark(name, t_prev):
            if stages is None:
                return t_prev
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            t = time.monotonic()
            stages.setdefault(name, []).append(round(1e3 * (t - t_prev), 2))
            return t
        images = list(images)
        B, V, texts, batch_states = self.parse_request(text, len(images), states, batch_size)
        model, dev = self.model, self.model.device
        frames = [Image.open(f).convert("RGB") for f in images]
        t = mark("png_decode", t0)
        # ---- images: every frame of the request in one process_images call -> [B, V, 3, H, W]
        pix = model.process_images(frames)
        if not torch.is_tensor(pix):
            raise ValueError("process_images gave outputs of unequal shape; one tower takes one frame size")
        pix = pix.to(dtype=model.dtype).view(B, V, *pix.shape[1:])
        n = self.num_images
        if V > n:
            pix, V = pix[:, :n].contiguous(), n
        if V < n and self.views != "present":
            pix = torch.cat([pix, torch.zeros(B, n - V, *pix.shape[2:], device=pix.device, dtype=pix.dtype)], dim=1)
            image_masks = np.tile(np.array([True] * V + [False] * (n - V)), (B, 1))
        else:
            image_masks = np.ones((B, V), dtype=bool)
        t = mark("process_images", t)
        # ---- prompt and states: host numpy, uploaded through pinned memory (a pageable copy would wait for the stream)
        ids, attention_mask = self.tokenize(texts)
        meta = {"non_delta_mask": np.array(self.non_delta_mask)}
        inputs = self.input_transform({"state": batch_states, "meta_data": dict(meta)})
        state_t = inputs["state"]
        kw = {} if noise is None else {"noise": noise}
        t = mark("prompt_states", t)
        with torch.no_grad():
            out = model.inference_action(input_ids=hostcpu.upload(ids, dev), attention_mask=attention_mask,
                                         states=hostcpu.upload(state_t, dev), images=pix, image_masks=image_masks, **kw)
        chunk = out.detach().cpu().numpy()                       # the one readback of the request
        t = mark("inference_action", t)
        # ---- answer: physical units, absolute actions (host float64, the reference's promotion)
        self.last_chunk, self.last_state = chunk, state_t.numpy()
        outputs = self.output_transform({"state": self.last_state, "action": chunk, "meta_data": dict(meta)})
        action = outputs["action"] if self.answer_batch else outputs["action"][0]
        answer = action[..., : self.action_dim].tolist()
        mark("answer", t)
        self.last_ms = 1e3 * (time.monotonic() - t0)
        if self.log:
            self.log(f"process_frame[{self.policy}]: batch {B}, {V} view(s) per sample, {self.last_ms:.1f} ms")
        return answer

    def inference_single(self, image_paths, prompt: str, states=None) -> list:
        """``--task inference_single`` of the exp scripts: one sample from image file(s) on disk"""
        paths = [image_paths] if isinstance(image_paths, (str, bytes)) or hasattr(image_paths, "read") else list(image_paths)
        return self.get_response(prompt, paths, states=states, batch_size=1)

    # ---- Flask plumbing ---------------------------------------------------------------------------------------
    def create_app(self):
        from flask import Flask, jsonify, request
        app = Flask(__name__)

        def process_frame():
            files = [io.BytesIO(f.read()) for f in request.files.getlist("image")]
            answer = self.get_response(request.form.get("text", ""), files, states=request.form.get("states", None),
                                       batch_size=request.form.get("batch_size", 1))
            return jsonify({"response": answer})

        app.add_url_rule("/process_frame", "process_frame", process_frame, methods=["POST"])
        return app

    def run(self) -> None:
        self.create_app().run(host="0.0.0.0", port=self.port, debug=False, threaded=False)


def encode_png(frame) -> bytes:
    """RGB uint8 [h, w, 3] -> PNG bytes, what dexbotic/client.py:40-44 sends (there via cv2.imencode)"""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="PNG")
    return buf.getvalue()
