"""DM0: dual-expert Qwen3 mixture of transformers with a flow-matching action head (model_type "dexbotic_dm0")."""
from .dm0_arch import DM0Config, DM0ForCausalLM, DM0Model

__all__ = ["DM0Config", "DM0ForCausalLM", "DM0Model"]
