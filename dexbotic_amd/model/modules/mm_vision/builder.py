"""Vision-tower factory (mirror of dexbotic/model/modules/mm_vision/builder.py:9-34)."""
from __future__ import annotations

from typing import Optional

from ....engine import ParamStore, current_store
from .clip.clip_encoder import CLIPVisionConfig, CLIPVisionTower
from .pe.pe_configuration import PerceptionEncoderConfig
from .pe.pe_encoder import PEVisionTower
from .siglip.siglip_encoder import SiglipVisionConfig, SiglipVisionTower


def build_vision_tower(mm_vision_tower, store: Optional[ParamStore] = None, prefix: str = "model.mm_vision_tower.",
                       **kwargs):
    """Reference signature ``build_vision_tower(mm_vision_tower_cfg, **kwargs)``: `mm_vision_tower` is a checkpoint
    directory / hub name (selected on the substrings 'sig' / 'clip' / 'pe' exactly like the reference; a 'pe' name is a registered
    Perception Encoder configuration, e.g. ``pe_lang_l14_728``), a config object carrying ``mm_vision_tower`` (mm_vision/builder.py:10),
    or a CLIPVisionConfig / SiglipVisionConfig / PerceptionEncoderConfig (synthetic-weight benchmarks).  The arena comes from the
    enclosing build context (engine.building) unless passed explicitly."""
    store = current_store(store)
    vt = getattr(mm_vision_tower, "mm_vision_tower", mm_vision_tower)
    if isinstance(vt, CLIPVisionConfig):
        return CLIPVisionTower(vt, store, prefix, **kwargs)
    if isinstance(vt, SiglipVisionConfig):
        return SiglipVisionTower(vt, store, prefix, **kwargs)
    if isinstance(vt, PerceptionEncoderConfig):
        return PEVisionTower(vt, store, prefix, **kwargs)
    if isinstance(vt, dict):
        model_type = str(vt.get("model_type", ""))
        if "siglip" in model_type:
            return SiglipVisionTower(SiglipVisionConfig.from_any(vt), store, prefix, **kwargs)
        if "perception_encoder" in model_type:
            return PEVisionTower(PerceptionEncoderConfig.from_any(vt), store, prefix, **kwargs)
        return CLIPVisionTower(CLIPVisionConfig.from_any(vt), store, prefix, **kwargs)
    if isinstance(vt, str):
        low = vt.lower()
        if "sig" in low:
            return SiglipVisionTower(vt, store, prefix, **kwargs)
        if "clip" in low:
            return CLIPVisionTower(vt, store, prefix, **kwargs)
        if "pe" in low:
            return PEVisionTower(vt, store, prefix, **kwargs)
    raise ValueError(f"Unknown vision tower: {vt}")
