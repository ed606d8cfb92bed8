from .pe_configuration import PE_LANG_L14_728, PerceptionEncoderConfig, get_config
from .pe_encoder import PEVisionTower

__all__ = ["PE_LANG_L14_728", "PerceptionEncoderConfig", "PEVisionTower", "get_config"]
