"""Action-model factory of the OFT policy (mirror of dexbotic/model/oft/action_model/builder.py:5-48)."""
from __future__ import annotations

from typing import Optional

from ....engine import ParamStore, current_store
from .model import DiscreteActionHead, L1RegressionActionHead

REQUIRED = ("action_model_type", "hidden_size", "action_dim", "chunk_size", "use_proprio", "proprio_dim")


def build_action_model(config, store: Optional[ParamStore] = None, prefix: str = "model.action_head."):
    """reference signature ``build_action_model(config)``; the arena comes from the enclosing build context.  The ``Linear``
    (L1 regression) head and the ``Discrete`` head are built; ``DiT`` is not.

    Deliberate deviation from the reference's builder, which hands a ``DiscreteActionHead`` to any config that asks for one: here
    ``"Discrete"`` is built only for an ``OFTDiscreteConfig`` (model_type ``dexbotic_oft_discrete``).  ``OFTForCausalLM`` has no
    forward for that head (it would read ``action_query`` as a parameter), so any other config is refused at build time."""
    missing = [k for k in REQUIRED if not hasattr(config, k)]
    if missing:                                     # exp/utils.py:43-52 require_config_keys
        raise ValueError(f"Missing required config keys: {missing}")
    model_type = config.action_model_type
    assert model_type in ["Linear", "DiT", "Discrete"], f"Unsupported action model type: {model_type}"
    if "DiT" in model_type:
        raise NotImplementedError("OFT: the 'DiT' (diffusion) head is not built: the reference drives it with diffusers' "
                                  "DDIMScheduler, against which no fixture of this head can be generated here; use 'Linear'")
    if "Discrete" in model_type:
        if getattr(config, "model_type", None) != "dexbotic_oft_discrete":
            raise NotImplementedError("OFT: the 'Discrete' head belongs to OFTDiscreteForCausalLM (model_type dexbotic_oft_discrete): "
                                      "build it from an OFTDiscreteConfig; OFTConfig takes 'Linear'")
        return DiscreteActionHead(store=current_store(store), prefix=prefix, input_dim=config.hidden_size,
                                  vocab_size=config.vocab_size, action_dim=config.action_dim, action_chunk=config.chunk_size,
                                  num_bins=config.num_bins, use_proprio=bool(config.use_proprio), proprio_dim=config.proprio_dim)
    store = current_store(store)
    return L1RegressionActionHead(store=store, prefix=prefix, input_dim=config.hidden_size, hidden_dim=config.hidden_size,
                                  action_dim=config.action_dim, action_chunk=config.chunk_size,
                                  use_proprio=bool(config.use_proprio), proprio_dim=config.proprio_dim)
