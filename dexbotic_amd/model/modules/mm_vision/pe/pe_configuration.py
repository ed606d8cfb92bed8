"""Perception Encoder configuration (mirror of dexbotic/model/modules/mm_vision/pe/pe_configuration.py:7-76)."""
from __future__ import annotations

from dataclasses import asdict, dataclass, field
from typing import List, Optional


@dataclass
class PerceptionEncoderConfig:
    patch_size: int
    width: int
    layers: int
    heads: int
    mlp_ratio: float
    output_dim: Optional[int]

    ls_init_value: Optional[float] = None
    drop_path: float = 0.0

    image_size: int = 224
    use_abs_posemb: bool = True
    use_cls_token: bool = False
    use_rope2d: bool = True

    pool_type: str = "attn"
    attn_pooler_heads: int = 8

    use_ln_pre: bool = True
    use_ln_post: bool = True

    layer_types: List[str] = field(default_factory=list)
    sliding_window_size: int = -1

    def to_dict(self):
        d = asdict(self)
        d["model_type"] = "perception_encoder"       # what build_vision_tower dispatches a plain dict on
        return d

    @classmethod
    def from_any(cls, obj) -> "PerceptionEncoderConfig":
        """a config, a registered name, a dict or any object carrying the fields (unknown keys are ignored)"""
        if isinstance(obj, cls):
            return obj
        if isinstance(obj, str):
            return get_config(obj)
        d = obj if isinstance(obj, dict) else (obj.to_dict() if hasattr(obj, "to_dict") else vars(obj))
        keys = set(cls.__dataclass_fields__)
        return cls(**{k: v for k, v in d.items() if k in keys})


@dataclass
class PE_LANG_L14_728(PerceptionEncoderConfig):
    image_size: int = 728
    patch_size: int = 14
    width: int = 1024
    layers: int = 23
    heads: int = 16
    mlp_ratio: float = 4.0
    pool_type: str = "none"
    output_dim: Optional[int] = None
    use_cls_token: bool = True
    use_ln_post: bool = False
    ls_init_value: float = 0.1


REGISTERED = {"pe_lang_l14_728": PE_LANG_L14_728}


def get_config(config_name: str) -> PerceptionEncoderConfig:
    """the config registered under `config_name` — like the reference, the exact name only"""
    if config_name not in REGISTERED:
        raise ValueError(f"Unknown configuration name: {config_name} (registered: {sorted(REGISTERED)})")
    return REGISTERED[config_name]()
