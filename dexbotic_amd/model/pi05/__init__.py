"""pi0.5: the pi0 mixture whose action expert takes the flow time through adaptive RMSNorms and gated residuals
(model_type "dexbotic_pi05")."""
from .pi05_arch import Pi05Config, Pi05ForCausalLM, Pi05Model

__all__ = ["Pi05Config", "Pi05ForCausalLM", "Pi05Model"]
