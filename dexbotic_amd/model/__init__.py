"""Policy classes.  The NaVILA and MuVLA families are exported by name (resolved on first use, so importing one policy module
does not import the others)."""


def __getattr__(name):
    if name in ("NaVILAConfig", "NaVILAForCausalLM", "NaVILAModel"):
        from . import navila
        return getattr(navila, name)
    if name in ("MUVLAConfig", "MUVLAForCausalLM", "MUVLAModel"):
        from . import muvla
        return getattr(muvla, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["NaVILAConfig", "NaVILAForCausalLM", "NaVILAModel", "MUVLAConfig", "MUVLAForCausalLM", "MUVLAModel"]
