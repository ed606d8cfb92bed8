"""Stand-in tokenizers of the flow-serving fixture (tests/golden/flow_serve_t1.npz): small, deterministic, with exactly the surface
Pi0Tokenization / DM0Tokenization touch — ``sp_model.encode(text, add_bos=)``, ``encode(text, add_special_tokens=)``,
``pad_token_id``, ``model_max_length``.  No real vocabulary is needed to pin what the tokenisers DO with a prompt (cleaning, role
pieces, cutting, padding).  One definition, used by scripts/gen_golden_flow_serve.py (under the reference's classes) and by the tests
(under the native ones).

A text is cut into words and newlines (blanks separate and are dropped); a piece's id is 3 + crc32(piece) mod (vocab - 3), so ids
0 (pi0's pad), 1 (BOS) and 2 (DM0's pad) never come out of a text."""
from __future__ import annotations

import re
import zlib
from typing import List

VOCAB = 250
BOS = 1


def pieces(text: str) -> List[int]:
    return [3 + zlib.crc32(p.encode("utf-8")) % (VOCAB - 3) for p in re.findall(r"\n|[^ \n]+", text)]


class _SentencePiece:
    def encode(self, text: str, add_bos: bool = False) -> List[int]:
        return ([BOS] if add_bos else []) + pieces(text)


class StandInTokenizer:
    def __init__(self, model_max_length: int, pad_token_id: int):
        self.model_max_length, self.pad_token_id = model_max_length, pad_token_id
        self.sp_model = _SentencePiece()

    def encode(self, text: str, add_special_tokens: bool = True) -> List[int]:
        return ([BOS] if add_special_tokens else []) + pieces(text)

    def decode(self, ids) -> str:
        return " ".join(str(int(i)) for i in ids)


def pi0_tokenizer(model_max_length: int = 12) -> StandInTokenizer:
    return StandInTokenizer(model_max_length, pad_token_id=0)


def dm0_tokenizer(model_max_length: int = 48) -> StandInTokenizer:
    return StandInTokenizer(model_max_length, pad_token_id=2)
