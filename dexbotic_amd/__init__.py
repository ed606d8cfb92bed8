"""dexbotic_amd — MI355X-native (gfx950 / CDNA4) drop-in for the DB-CogACT hot path of dexmal/dexbotic.

Importing the package loads libdexbotic_amd.so through ctypes and fails loudly if it is missing:
there is no CPU or eager-PyTorch fallback for the compute path.

    from dexbotic_amd.model.cogact.cogact_arch import CogActConfig, CogACTForCausalLM

mirrors ``dexbotic.model.cogact.cogact_arch`` (same class names, ``forward`` / ``inference_action``
contracts, ``state_dict`` keys and ``model_type`` registry strings).
"""
import sys as _sys


def _is_build_invocation() -> bool:
    """True only for ``python -m dexbotic_amd.build`` — the one command that must work BEFORE the library exists (the
    ImportError below names it).  runpy imports this package before it runs the build module, so the library check is
    skipped for exactly that command line and for nothing else."""
    oa = list(getattr(_sys, "orig_argv", []))
    return any(a == "-m" and i + 1 < len(oa) and oa[i + 1] == "dexbotic_amd.build" for i, a in enumerate(oa))


if not _is_build_invocation():
    from . import _lib  # noqa: F401  (raises ImportError when the native library is absent)

__version__ = "0.1.0"


def model_registry():
    """``config.model_type`` -> (Config, ForCausalLM): the HF AutoConfig/AutoModel registry strings of the
    reference (dexbotic_arch.py:18, cogact_arch.py:14)."""
    from .model.cogact.cogact_arch import CogActConfig, CogACTForCausalLM
    from .model.dexbotic_arch import DexboticConfig, DexboticForCausalLM
    from .model.dm0.dm0_arch import DM0Config, DM0ForCausalLM
    from .model.dm0.dm0_prog_arch import DM0ProgConfig, DM0ProgForCausalLM
    from .model.memvla.memvla_arch import MemVLAConfig, MemVLAForCausalLM
    from .model.navila.navila_arch import NaVILAConfig, NaVILAForCausalLM
    from .model.oft.oft_arch import OFTConfig, OFTForCausalLM
    from .model.oft.oft_discrete_arch import OFTDiscreteConfig, OFTDiscreteForCausalLM
    from .model.pi0.pi0_arch import Pi0Config, Pi0ForCausalLM
    from .model.pi05.pi05_arch import Pi05Config, Pi05ForCausalLM
    return {"dexbotic": (DexboticConfig, DexboticForCausalLM),
            "dexbotic_cogact": (CogActConfig, CogACTForCausalLM),
            "dexbotic_pi0": (Pi0Config, Pi0ForCausalLM),
            "dexbotic_memvla": (MemVLAConfig, MemVLAForCausalLM),
            "dexbotic_navila": (NaVILAConfig, NaVILAForCausalLM),
            "dexbotic_dm0": (DM0Config, DM0ForCausalLM),
            "dexbotic_dm0_prog": (DM0ProgConfig, DM0ProgForCausalLM),
            "dexbotic_pi05": (Pi05Config, Pi05ForCausalLM),
            "dexbotic_oft": (OFTConfig, OFTForCausalLM),
            "dexbotic_oft_discrete": (OFTDiscreteConfig, OFTDiscreteForCausalLM)}


def __getattr__(name):
    if name in ("Pi05Config", "Pi05ForCausalLM", "Pi05Model"):
        from .model import pi05
        return getattr(pi05, name)
    if name in ("OFTDiscreteConfig", "OFTDiscreteForCausalLM", "OFTDiscreteModel",
                "OFTDiffusionConfig", "OFTDiffusionForCausalLM", "OFTDiffusionModel"):
        from .model import oft
        return getattr(oft, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def hybrid_cogact():
    """HybridCogACTForCausalLM shares model_type "dexbotic_cogact" with CogACT (hybrid_cogact_arch.py:18-22)"""
    from .model.cogact.hybrid_cogact_arch import HybridCogACTForCausalLM
    return HybridCogACTForCausalLM


def discrete_vla():
    """DiscreteVLAForCausalLM shares model_type "dexbotic" with the base class in the reference
    (discrete_vla_arch.py:12-13); exps pick it by class, so it is exported by name here."""
    from .model.discrete_vla.discrete_vla_arch import DiscreteVLAForCausalLM
    return DiscreteVLAForCausalLM


def muvla():
    """MUVLAForCausalLM shares model_type "dexbotic" with the base class in the reference (muvla_arch.py:17-18); exps pick it by
    class, so it is exported by name here."""
    from .model.muvla.muvla_arch import MUVLAForCausalLM
    return MUVLAForCausalLM


def from_pretrained(path: str, **kw):
    """load any registered policy from a reference-format checkpoint directory"""
    import json
    import os
    with open(os.path.join(path, "config.json")) as f:
        cfg = json.load(f)
    mt = cfg.get("model_type", "dexbotic")
    _, cls = model_registry()[mt]
    if mt == "dexbotic_oft" and "DiT" in str(cfg.get("action_model_type")):
        # the diffusion head shares the reference's model_type string with the Linear head (oft_diffusion_arch.py)
        from .model.oft.oft_diffusion_arch import OFTDiffusionForCausalLM as cls
    return cls.from_pretrained(path, **kw)
