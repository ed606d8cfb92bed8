"""Policy classes.  The NaVILA, MuVLA, DM0, DM0-prog, pi0.5 and OFT families and the Perception Encoder tower are exported by name (resolved on first
use, so importing one policy module does not import the others)."""


def __getattr__(name):
    if name in ("NaVILAConfig", "NaVILAForCausalLM", "NaVILAModel"):
        from . import navila
        return getattr(navila, name)
    if name in ("MUVLAConfig", "MUVLAForCausalLM", "MUVLAModel"):
        from . import muvla
        return getattr(muvla, name)
    if name in ("DM0Config", "DM0ForCausalLM", "DM0Model", "DM0ProgConfig", "DM0ProgForCausalLM", "DM0ProgModel"):
        from . import dm0
        return getattr(dm0, name)
    if name in ("Pi05Config", "Pi05ForCausalLM", "Pi05Model"):
        from . import pi05
        return getattr(pi05, name)
    if name in ("OFTConfig", "OFTForCausalLM", "OFTModel", "OFTDiscreteConfig", "OFTDiscreteForCausalLM", "OFTDiscreteModel",
                "OFTDiffusionConfig", "OFTDiffusionForCausalLM", "OFTDiffusionModel"):
        from . import oft
        return getattr(oft, name)
    if name in ("PerceptionEncoderConfig", "PEVisionTower"):
        from .modules.mm_vision import pe
        return getattr(pe, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["NaVILAConfig", "NaVILAForCausalLM", "NaVILAModel", "MUVLAConfig", "MUVLAForCausalLM", "MUVLAModel",
           "DM0Config", "DM0ForCausalLM", "DM0Model", "DM0ProgConfig", "DM0ProgForCausalLM", "DM0ProgModel", "Pi05Config", "Pi05ForCausalLM", "Pi05Model",
           "OFTConfig", "OFTForCausalLM", "OFTModel", "OFTDiscreteConfig", "OFTDiscreteForCausalLM", "OFTDiscreteModel",
           "OFTDiffusionConfig", "OFTDiffusionForCausalLM", "OFTDiffusionModel", "PerceptionEncoderConfig", "PEVisionTower"]
