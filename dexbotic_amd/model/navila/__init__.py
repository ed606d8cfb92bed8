"""NaVILA, the video-history VLA (dexbotic/model/navila): see navila_arch.py."""
from .navila_arch import NaVILAConfig, NaVILAForCausalLM, NaVILAModel

__all__ = ["NaVILAConfig", "NaVILAForCausalLM", "NaVILAModel"]
