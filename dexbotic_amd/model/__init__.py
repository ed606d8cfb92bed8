"""Policy classes.  The NaVILA, MuVLA and DM0 families are exported by name (resolved on first use, so importing one policy module
does not import the others)."""


def __getattr__(name):
    if name in ("NaVILAConfig", "NaVILAForCausalLM", "NaVILAModel"):
        from . import navila
        return getattr(navila, name)
    if name in ("MUVLAConfig", "MUVLAForCausalLM", "MUVLAModel"):
        from . import muvla
        return getattr(muvla, name)
    if name in ("DM0Config", "DM0ForCausalLM", "DM0Model"):
        from . import dm0
        return getattr(dm0, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["NaVILAConfig", "NaVILAForCausalLM", "NaVILAModel", "MUVLAConfig", "MUVLAForCausalLM", "MUVLAModel",
           "DM0Config", "DM0ForCausalLM", "DM0Model"]
