"""MuVLA, the map-plus-observation navigation policy (dexbotic/model/muvla): see muvla_arch.py."""
from .muvla_arch import MUVLAConfig, MUVLAForCausalLM, MUVLAModel

__all__ = ["MUVLAConfig", "MUVLAForCausalLM", "MUVLAModel"]
