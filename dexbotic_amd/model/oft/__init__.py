"""OFT, the parallel-decoding VLA (dexbotic/model/oft): the L1-regression head in oft_arch.py, the discrete
(vocabulary-bin) head in oft_discrete_arch.py, the diffusion head in oft_diffusion_arch.py."""
from .oft_arch import OFTConfig, OFTForCausalLM, OFTModel
from .oft_diffusion_arch import OFTDiffusionConfig, OFTDiffusionForCausalLM, OFTDiffusionModel
from .oft_discrete_arch import OFTDiscreteConfig, OFTDiscreteForCausalLM, OFTDiscreteModel

__all__ = ["OFTConfig", "OFTForCausalLM", "OFTModel", "OFTDiscreteConfig", "OFTDiscreteForCausalLM", "OFTDiscreteModel",
           "OFTDiffusionConfig", "OFTDiffusionForCausalLM", "OFTDiffusionModel"]
