"""Drop-in check of the plugin surface: the REFERENCE's own experiment-layer code —
``CogACTModelConfig._freeze_model`` (dexbotic/exp/cogact_exp.py:106-124) and
``OptimizerConfig._get_optimizer_grouped_parameters`` (dexbotic/exp/base_exp.py:95-203) — run, unmodified, on the NATIVE
model by oracle/gen_golden_exp_groups.py; what it decided is committed as tests/golden/exp_groups.json: which parameters
are frozen and the parameter groups (which parameters, which learning rate, weight decay or not — selected by module TYPE
through transformers' get_parameter_names(ALL_LAYERNORM_LAYERS)).  Those groups must be the groups engine.FusedAdamW uses."""
import json
import os
import types

import pytest

from tests.helpers import CFGS, build_product
from oracle.weights import cogact_shapes, make_weights


@pytest.fixture(scope="module")
def ref_exp(golden_dir):
    with open(os.path.join(golden_dir, "exp_groups.json")) as f:
        return json.load(f)


def _case(ref_exp, freeze, lrs):
    for c in ref_exp["cases"]:
        if c["freeze"] == freeze and c["lrs"] == lrs:
            return c
    raise AssertionError(f"exp_groups.json has no case freeze={freeze} lrs={lrs}")


def _param_groups(groups, module):
    """the reference's groups as _get_optimizer_grouped_parameters returned them, on this module's parameters"""
    params = dict(module.named_parameters())
    return [{"lr": g["lr"], "weight_decay": g["weight_decay"], "params": [params[n] for n in g["params"]]} for g in groups]


class _RecordedOptimizerConfig(types.SimpleNamespace):
    """the reference's CogACTOptimizerConfig as recorded: its fields, and the groups its _get_optimizer_grouped_parameters
    built on the *ForCausalLM"""

    def _get_optimizer_grouped_parameters(self, model):
        return _param_groups(self._groups, model)


def _native_model():
    cfg = CFGS["t1"]
    return build_product(cfg, make_weights(cogact_shapes(cfg), 3), "float32", "cpu", train=True)


@pytest.mark.parametrize("lrs", [dict(), dict(mm_projector_lr=1e-4, mm_vision_lr=2e-6, action_head_lr=5e-5)])
@pytest.mark.parametrize("freeze", [dict(), dict(freeze_mm_vision=True), dict(freeze_llm=True, freeze_action_head=True)])
def test_reference_freeze_and_optimizer_groups_on_native_model(ref_exp, lrs, freeze):
    from dexbotic_amd.engine import FusedAdamW, OptimConfig
    case = _case(ref_exp, freeze, lrs)
    m = _native_model()
    named = dict(m.named_parameters())
    for n in case["frozen"]:                                                  # what the reference's _freeze_model froze
        named[n].requires_grad_(False)
    frozen = {n for n, p in m.named_parameters() if not p.requires_grad}
    if freeze.get("freeze_mm_vision"):
        assert frozen and all(".mm_vision_tower." in n for n in frozen)
    groups = _param_groups(case["groups"], m.model)                           # the reference's groups on the native model
    by_param = {}
    for g in groups:
        for p in g["params"]:
            assert id(p) not in by_param, "parameter in two groups"
            by_param[id(p)] = (g["lr"], g["weight_decay"])
    opt = FusedAdamW(m.store, OptimConfig(base_lr=2e-5, weight_decay=0.1, **lrs),
                     exclude=[n for n in m.store.slots if not m.store.params[n].requires_grad] + ["lm_head.weight"])
    lr_of = {"base": 2e-5, "mm_projector": lrs.get("mm_projector_lr"), "mm_vision": lrs.get("mm_vision_lr"),
             "action_head": lrs.get("action_head_lr")}
    seen = 0
    for name, p in m.model.named_parameters():
        full = "model." + name
        if not p.requires_grad:
            assert id(p) not in by_param and full not in opt.group_of
            continue
        lr_key, decayed = opt.group_of[full]
        assert by_param[id(p)] == (lr_of[lr_key], 0.1 if decayed else 0.0), full
        seen += 1
    assert seen == len(by_param) and seen > 0


def test_native_trainer_takes_the_reference_exp_config_objects(ref_exp, tmp_path):
    """NativeDexboticTrainer (the opt-in replacement of DexboticTrainer) constructed from the REFERENCE's config objects as
    exp_groups.json records them — dexbotic.exp.base_exp.TrainerConfig with its defaults (deepspeed zero3.json, gradient_checkpointing=True, bf16, 8 x accum 2,
    cosine) and CogACTOptimizerConfig with per-module learning rates — on the native model: the linked TrainingArguments, and
    the fused optimizer's groups = the groups the reference's _get_optimizer_grouped_parameters returns for the *ForCausalLM
    (what DexboticTrainer.create_optimizer passes, trainer.py:25-36).  CPU: construction only, no step."""
    from dexbotic_amd.exp.trainer import ArenaAdamW, NativeDexboticTrainer, link_exp_config
    rec = ref_exp["trainer"]
    tc = types.SimpleNamespace(**{k: str(tmp_path) if v == "<output_dir>" else v for k, v in rec["trainer_config"].items()})
    assert tc.gradient_checkpointing and tc.deepspeed and tc.gradient_accumulation_steps == 2
    oc = _RecordedOptimizerConfig(**rec["optimizer_config"], _groups=rec["groups"])
    assert oc.base_lr == 2e-5 and oc.weight_decay == 0.1 and oc.mm_projector_lr == 1e-4 and oc.action_head_lr == 5e-5
    exp = types.SimpleNamespace(trainer_config=tc, optimizer_config=oc)
    args = link_exp_config(exp, use_cpu=True, bf16=False, report_to=[])
    assert args.gradient_accumulation_steps == 2 and args.per_device_train_batch_size == 8 and args.learning_rate == 2e-5
    assert args.lr_scheduler_type == "cosine" and args.max_grad_norm == 0.0            # the 1.0 clip runs inside the fused step
    assert not args.gradient_checkpointing and args.deepspeed is None                  # deliberately not forwarded
    m = _native_model()
    tr = NativeDexboticTrainer(model=m, args=args, train_dataset=[0] * 4, exp_config=exp)
    opt = tr.create_optimizer()
    assert isinstance(opt, ArenaAdamW) and tr.core.cfg.max_grad_norm == 1.0 and tr.core.grad_accum == 2
    ref_groups = oc._get_optimizer_grouped_parameters(m)                               # the reference's groups on the *ForCausalLM
    assert len(opt.param_groups) == len(ref_groups) == len(tr.core.opt.group_keys) == 6
    name_of = {id(p): n for n, p in m.named_parameters()}
    unused = set(m.unused_parameter_names())
    for gi, g in enumerate(ref_groups):
        assert opt.param_groups[gi]["lr"] == g["lr"] and opt.param_groups[gi]["weight_decay"] == g["weight_decay"]
        for p in g["params"]:
            n = name_of[id(p)]
            if n in unused:
                assert n not in tr.core.opt.group_of                                   # never gets a gradient: not updated
            else:
                assert tr.core.opt.group_of[n] == tr.core.opt.group_keys[gi], n
