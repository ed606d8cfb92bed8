"""Prompt tokenisers of the flow policies (dexbotic/tokenization/process.py:116-245): ``Pi0Tokenization`` for pi0 / pi0.5 (the
sentencepiece model of the Gemma tokenizer, fixed length, zero padded) and ``DM0Tokenization`` (the "step" conversation template
with role tokens, fixed length, padded with ``pad_token_id``).  Same constructors, same ``__call__(conversations)`` contract, the
same integer arrays; host code — a prompt is a few dozen tokens."""
from __future__ import annotations

from typing import Dict, List

import numpy as np

from ..constants import IGNORE_INDEX
from . import conversation as conversation_lib


class Pi0Tokenization:
    """prompt = the first turn's ``value``: stripped, newlines and underscores to blanks, encoded with BOS, followed by the encoding
    of a newline; cut to ``tokenizer.model_max_length`` and padded with 0.  ``labels`` are the same ids."""

    def __init__(self, tokenizer, *args, **kwargs):
        self.tokenizer = tokenizer
        self._max_len = tokenizer.model_max_length

    def __call__(self, conversations: List[Dict], **kwargs) -> Dict:
        sp = self.tokenizer.sp_model
        text = conversations[0]["value"].strip().replace("\n", " ").replace("_", " ")
        ids = (sp.encode(text, add_bos=True) + sp.encode("\n"))[: self._max_len]
        ids = ids + [0] * (self._max_len - len(ids))
        return {"input_ids": np.asarray(ids), "labels": np.asarray(ids)}


class DM0Tokenization:
    """"<system><sep>" then per turn "<ROLE>: " and "<text><that role's separator>" (nothing for an empty text), every piece encoded on
    its own without special tokens; an empty trailing assistant turn is dropped first.  ``token_mask`` marks real tokens, ``ar_mask``
    is 1 on them (causal), ``loss_mask`` the assistant's content; ``labels`` = ids where the loss is taken, IGNORE_INDEX elsewhere."""

    def __init__(self, tokenizer, chat_template: str = "step", *args, **kwargs):
        self.tokenizer = tokenizer
        self._max_len = tokenizer.model_max_length
        self.chat_template = chat_template

    def __call__(self, conversations: List[Dict], **kwargs) -> Dict:
        conv = conversation_lib.conv_templates[self.chat_template].copy()
        human, gpt = conv.roles
        roles = {"human": human, "gpt": gpt}
        seps = {human: conv.sep, gpt: conv.sep2}
        enc = lambda s: list(self.tokenizer.encode(s, add_special_tokens=False))

        ids = enc(f"{conv.system}{conv.sep}")
        loss = [False] * len(ids)
        turns = list(conversations)
        if turns and turns[-1].get("from") == "gpt" and not turns[-1].get("value"):
            turns.pop()
        for msg in turns:
            role = roles.get(msg.get("from", "human"))
            if role is None:
                continue
            text = (msg.get("value", "") or "").strip().replace("\n", " ")
            head = enc(f"{role}: ")
            body = enc(f"{text}{seps[role]}" if text else "")
            ids += head + body
            loss += [False] * len(head) + [role == gpt] * len(body)

        n, L = len(ids), self._max_len
        real = [True] * n
        ar = [1] * n
        if n < L:
            pad = [False] * (L - n)
            ids = ids + [self.tokenizer.pad_token_id] * (L - n)
            real, ar, loss = real + pad, ar + pad, loss + pad
        else:
            ids, real, ar, loss = ids[:L], real[:L], ar[:L], loss[:L]
        input_ids = np.asarray(ids)
        return {"input_ids": input_ids, "labels": np.where(np.asarray(loss), input_ids, IGNORE_INDEX),
                "token_mask": np.asarray(real), "ar_mask": np.asarray(ar), "loss_mask": np.asarray(loss)}
