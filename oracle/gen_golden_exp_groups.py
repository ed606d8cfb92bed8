"""Generate tests/golden/exp_groups.json by running the REFERENCE's experiment layer on the NATIVE model — TEST INFRASTRUCTURE.

    python -m oracle.gen_golden_exp_groups        # build container only (needs /root/reference)

The reference's own ``CogACTModelConfig._freeze_model`` (dexbotic/exp/cogact_exp.py:106-124) and
``OptimizerConfig._get_optimizer_grouped_parameters`` (dexbotic/exp/base_exp.py:95-203) are imported and run, unmodified, on
the native model for every freeze / learning-rate case of tests/test_dropin_reference_exp.py; what they decide (the frozen
parameters; per group: learning rate, weight decay, parameter names) is written as JSON, together with the defaults of the
reference's ``TrainerConfig`` / ``CogACTOptimizerConfig`` and the groups built on the *ForCausalLM.  Third-party packages
the reference's exp layer imports but this container lacks (loguru, megfile, easydict, numpydantic, decord, av, cv2, timm,
...) are replaced by inert stand-ins: none of them is touched by the two functions."""
from __future__ import annotations

import importlib.abc
import importlib.machinery
import json
import os
import sys
import types

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden")

MISSING = ("loguru", "megfile", "easydict", "numpydantic", "decord", "av", "cv2", "timm", "albumentations", "deepspeed",
           "wandb", "peft", "flask", "tyro", "imageio", "h5py", "openpi_client")

FREEZES = [dict(), dict(freeze_mm_vision=True), dict(freeze_llm=True, freeze_action_head=True)]
LRS = [dict(), dict(mm_projector_lr=1e-4, mm_vision_lr=2e-6, action_head_lr=5e-5)]
TRAINER_LRS = dict(mm_projector_lr=1e-4, action_head_lr=5e-5)


class _Meta(type):
    """stand-in classes answer any CLASS attribute too (enum members, constants) and subscript like generics"""

    def __getattr__(cls, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _make(name)

    def __getitem__(cls, item):
        return cls

    def __or__(cls, other):
        return cls

    def __ror__(cls, other):
        return cls


def _make(name):
    return _Meta(name, (), {"__init__": lambda self, *a, **k: None, "__call__": lambda self, *a, **k: None,
                            "__getattr__": lambda self, k: (lambda *a, **kw: None)})


class _Anything(types.ModuleType):
    """module stand-in: every attribute is a permissive class (usable as base class, decorator, callable, annotation)"""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        val = _make(name)
        setattr(self, name, val)
        return val


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, fullname, path=None, target=None):
        if fullname.split(".")[0] in MISSING:
            return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
        return None

    def create_module(self, spec):
        m = _Anything(spec.name)
        m.__path__ = []
        return m

    def exec_module(self, module):
        pass


def load_reference_exp():
    import transformers  # noqa: F401  (first: its lazy importer probes optional packages by spec)
    sys.meta_path.append(_StubFinder())
    sys.path.insert(0, REF)
    # pydantic cannot build a schema for a stand-in NDArray: the norm-stats module is not on the path under test
    norm = types.ModuleType("dexbotic.data.utils.normalize")
    norm.RunningStats = norm.NormStats = object
    norm.save = norm.load = lambda *a, **k: None
    import dexbotic.data.utils as du
    sys.modules["dexbotic.data.utils.normalize"] = norm
    du.normalize = norm
    from dexbotic.exp import base_exp, cogact_exp
    return base_exp, cogact_exp


def _native_model():
    from oracle.weights import cogact_shapes, make_weights
    from tests.helpers import CFGS, build_product
    cfg = CFGS["t1"]
    return build_product(cfg, make_weights(cogact_shapes(cfg), 3), "float32", "cpu", train=True)


def _groups(groups, module):
    name_of = {id(p): n for n, p in module.named_parameters()}
    return [{"lr": g["lr"], "weight_decay": g["weight_decay"], "params": [name_of[id(p)] for p in g["params"]]} for g in groups]


def _plain_fields(obj):
    out = {}
    for k, v in vars(obj).items():
        try:
            json.dumps(v)
        except TypeError:
            continue
        out[k] = v
    return out


def main():
    sys.path.insert(0, ROOT)
    base_exp, cogact_exp = load_reference_exp()
    cases = []
    for freeze in FREEZES:
        for lrs in LRS:
            m = _native_model()
            mc = cogact_exp.CogACTModelConfig.__new__(cogact_exp.CogACTModelConfig)   # dataclass fields only; no checkpoint I/O
            for k in ("freeze_llm", "freeze_mm_projector", "freeze_mm_vision", "freeze_action_head"):
                setattr(mc, k, freeze.get(k, False))
            mc._freeze_model(m)                                                     # reference code, native model
            oc = cogact_exp.CogACTOptimizerConfig(base_lr=2e-5, weight_decay=0.1, **lrs)
            cases.append({"freeze": freeze, "lrs": lrs,
                          "frozen": sorted(n for n, p in m.named_parameters() if not p.requires_grad),
                          "groups": _groups(oc._get_optimizer_grouped_parameters(m.model), m.model)})
    tc = base_exp.TrainerConfig(output_dir="<output_dir>")
    oc = cogact_exp.CogACTOptimizerConfig(base_lr=2e-5, weight_decay=0.1, **TRAINER_LRS)
    m = _native_model()
    trainer = {"trainer_config": _plain_fields(tc), "optimizer_config": _plain_fields(oc),
               "groups": _groups(oc._get_optimizer_grouped_parameters(m), m)}            # on the *ForCausalLM
    path = os.path.join(GOLD, "exp_groups.json")
    with open(path, "w") as f:
        json.dump({"cases": cases, "trainer": trainer}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
