"""Action-model factory of the OFT policy (mirror of dexbotic/model/oft/action_model/builder.py:5-48)."""
from __future__ import annotations

from typing import Optional

from ....engine import ParamStore, current_store
from .model import DiffusionActionHead, DiscreteActionHead, L1RegressionActionHead

REQUIRED = ("action_model_type", "hidden_size", "action_dim", "chunk_size", "use_proprio", "proprio_dim")


def build_action_model(config, store: Optional[ParamStore] = None, prefix: str = "model.action_head."):
    """reference signature ``build_action_model(config)``; the arena comes from the enclosing build context.  The ``Linear``
    (L1 regression) head, the ``Discrete`` head and the ``DiT`` (diffusion) head are built.

    Deliberate deviation from the reference's builder, which hands a ``DiscreteActionHead`` to any config that asks for one: here
    ``"Discrete"`` is built only for an ``OFTDiscreteConfig`` (model_type ``dexbotic_oft_discrete``).  ``OFTForCausalLM`` has no
    forward for that head (it would read ``action_query`` as a parameter), so any other config is refused at build time.  ``"DiT"`` is
    built only for an ``OFTDiffusionConfig`` for the same reason; that class keeps the reference's model_type ``dexbotic_oft``, so it
    is told apart by its type."""
    missing = [k for k in REQUIRED if not hasattr(config, k)]
    if missing:                                     # exp/utils.py:43-52 require_config_keys
        raise ValueError(f"Missing required config keys: {missing}")
    model_type = config.action_model_type
    assert model_type in ["Linear", "DiT", "Discrete"], f"Unsupported action model type: {model_type}"
    if "DiT" in model_type:
        from ..oft_diffusion_arch import OFTDiffusionConfig
        if not isinstance(config, OFTDiffusionConfig):
            raise NotImplementedError("OFT: the 'DiT' (diffusion) head belongs to OFTDiffusionForCausalLM: build it from an "
                                      "OFTDiffusionConfig (same model_type dexbotic_oft); OFTConfig takes 'Linear'")
        return DiffusionActionHead(store=current_store(store), prefix=prefix, input_dim=config.hidden_size,
                                   hidden_dim=config.hidden_size, action_dim=config.action_dim, action_chunk=config.chunk_size,
                                   num_diffusion_steps=config.num_diffusion_steps, use_proprio=bool(config.use_proprio),
                                   proprio_dim=config.proprio_dim)
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
