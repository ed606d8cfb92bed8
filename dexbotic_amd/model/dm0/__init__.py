"""DM0: dual-expert Qwen3 mixture of transformers with a flow-matching action head (model_type "dexbotic_dm0"), and DM0-prog, the
same sampler with a progress token (model_type "dexbotic_dm0_prog")."""
from .dm0_arch import DM0Config, DM0ForCausalLM, DM0Model
from .dm0_prog_arch import DM0ProgConfig, DM0ProgForCausalLM, DM0ProgModel

__all__ = ["DM0Config", "DM0ForCausalLM", "DM0Model", "DM0ProgConfig", "DM0ProgForCausalLM", "DM0ProgModel"]
