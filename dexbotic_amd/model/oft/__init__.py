"""OFT, the parallel-decoding VLA with an L1-regression head (dexbotic/model/oft): see oft_arch.py."""
from .oft_arch import OFTConfig, OFTForCausalLM, OFTModel

__all__ = ["OFTConfig", "OFTForCausalLM", "OFTModel"]
