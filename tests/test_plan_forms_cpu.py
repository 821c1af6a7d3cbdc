"""Which launches a plan consists of, checked without a GPU: plan_forms.resolve_forms on plain inputs, and the record names of a handful of plans built
in HOST memory (plan construction only allocates tensors and fills ctypes structs; nothing here launches).  tools/plan_signature.py compares whole launch
lists, arguments included, between two commits."""
import dataclasses
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch

from sea_amd import _native as N
from sea_amd import _switches
from sea_amd.plan_forms import CONDITION, TRAINING, PlanForms, resolve_forms

BF16, F32 = torch.bfloat16, torch.float32


def facts(E=256, F=3, ln="adaln", L=1, xmode="sea", ib="add", after=True):
    """TemporalModel's structural attributes (8 heads, down_proj 2, scale_ratio 8)."""
    return SimpleNamespace(num_variables=F, n_heads=8, num_layers=L, embed_dim=E, internal_embed_dim=E, down_dim=E // 2, mlp_hidden=8 * E, LN_type=ln,
                           exchange_mode=xmode, ib_addition_mode=ib, add_info_after_cross=after)


CFG2, CYLINDER, MULTIPHASE = facts(), facts(1024, 2), facts(2048, 2, ln="ln")


def forms(model, B, T, mode="full", dt=BF16, plan="", kv="", **kw):
    return resolve_forms(model, B, T, mode, dt, plan_switches=dict(t.split("=") for t in plan.split(",") if t), kv_switches=dict(t.split("=") for t in kv.split(",") if t), **kw)


# cfg2 at B = 1, T = 2024 in bf16: row chains with riders, the one-launch front with its third layer, the field MLP as one launch
CFG2_B1 = PlanForms(lanes=False, split_cond=False, chain=True, riders=True, rider_caps=None, gen_a=False, fold_ib=True, hoist_ib=False, ib_rows_here=True, xtail=True, few=False,
                    few_fold_ln=True, hidden_pad=64, front_chain=True, front3=True, adaln_front=True, front_big=False, mlp_fc1=True, mlp_norm_in=True, mlp_block=True,
                    mlp_fc2_proj=False, down_norm=True, proj_norm=True, splitk=True)
NO_RIDERS = dict(riders=False, front_chain=False, front3=False, adaln_front=False)
NO_CHAIN = dict(chain=False, **NO_RIDERS)
# ... at B = 8 (16192 rows): the 18-launch form, condition MLPs with the generated operand on a lane of their own, sea_ib_add
CFG2_B8 = dataclasses.replace(CFG2_B1, split_cond=True, gen_a=True, fold_ib=False, ib_rows_here=False, **NO_CHAIN)
# the shipped cylinder width as a KV-cache step: the few-row launches
CYL_STEP = PlanForms(lanes=False, split_cond=False, chain=False, riders=False, rider_caps=None, gen_a=False, fold_ib=True, hoist_ib=False, ib_rows_here=True, xtail=False, few=True,
                     few_fold_ln=True, hidden_pad=64, front_chain=False, front3=False, adaln_front=False, front_big=False, mlp_fc1=False, mlp_norm_in=False, mlp_block=False,
                     mlp_fc2_proj=False, down_norm=False, proj_norm=False, splitk=True)


def test_forms_of_the_headline_shapes():
    assert forms(CFG2, 1, 2024) == CFG2_B1
    assert forms(CFG2, 8, 2024) == CFG2_B8
    assert forms(CFG2, 16, 70) == CFG2_B1
    no_mlp = dict(mlp_fc1=False, mlp_norm_in=False, mlp_block=False)
    assert forms(CFG2, 1, 1, "step") == dataclasses.replace(CFG2_B1, **NO_CHAIN, **no_mlp)
    assert forms(CFG2, 1, 2024, dt=F32) == dataclasses.replace(CFG2_B1, xtail=False, **NO_CHAIN, **no_mlp)
    assert forms(CYLINDER, 1, 1, "step") == CYL_STEP
    assert forms(CYLINDER, 1, 1, "step", hoisted=True, hoisted_ib=True) == dataclasses.replace(CYL_STEP, hoist_ib=True, ib_rows_here=False)
    assert forms(MULTIPHASE, 1, 1, "step") == dataclasses.replace(CYL_STEP, fold_ib=False, ib_rows_here=False, few_fold_ln=False)
    assert forms(MULTIPHASE, 1, 1, "step", hoisted=True, hoisted_ib=True) == dataclasses.replace(CYL_STEP, hoist_ib=True, ib_rows_here=False, few_fold_ln=False)


def test_training_and_condition_plans_get_no_inference_only_form():
    off = dict(fold_ib=False, ib_rows_here=False, xtail=False, hidden_pad=0, mlp_fc1=False, mlp_norm_in=False, mlp_block=False, proj_norm=False, **NO_CHAIN)
    assert forms(CFG2, 1, 2024, kind=TRAINING) == dataclasses.replace(CFG2_B1, **off)
    assert forms(CFG2, 1, 2024, kind=CONDITION) == dataclasses.replace(CFG2_B1, down_norm=False, **off)
    assert forms(CFG2, 1, 2024, kind=TRAINING, plan="norm=0") == dataclasses.replace(CFG2_B1, down_norm=False, **off)


@pytest.mark.parametrize("switch,flips", [
    ("lanes=all", dict(lanes=True, split_cond=True, fold_ib=False, ib_rows_here=False, xtail=False, **NO_CHAIN)),
    ("lanes=cond", dict(split_cond=True, fold_ib=False, ib_rows_here=False, **NO_RIDERS)),
    ("norm=0", dict(xtail=False, down_norm=False, proj_norm=False, **NO_CHAIN)),
    ("xtail=0", dict(xtail=False, **NO_CHAIN)),
    ("xtail_max_rows=100", dict(xtail=False)),
    ("chain=0", NO_CHAIN),
    ("chain_max_rows=1000", NO_CHAIN),
    ("riders=0", NO_RIDERS),
    ("rider_caps=256:64:64", dict(rider_caps=(256, 64, 64))),
    ("silu=1", dict(gen_a=True)),
    ("fold_ib=0", dict(fold_ib=False, ib_rows_here=False)),
    ("mlp1=0", dict(mlp_fc1=False, mlp_norm_in=False, mlp_block=False, mlp_fc2_proj=True)),
    ("mlpnorm=0", dict(mlp_norm_in=False)),
    ("mlp2=0", dict(mlp_block=False)),
    ("mlpblock=0", dict(mlp_block=False, mlp_fc2_proj=True)),
    ("front=0", dict(front_chain=False, front3=False)),
    ("front3=0", dict(front3=False)),
    ("adaln_gemm=0", dict(front_chain=False, front3=False, adaln_front=False)),
    ("projnorm=0", dict(proj_norm=False)),
    ("splitk=0", dict(splitk=False)),
])
def test_each_plan_switch_flips_the_forms_it_names_at_one_trajectory(switch, flips):
    assert forms(CFG2, 1, 2024, plan=switch) == dataclasses.replace(CFG2_B1, **flips)


@pytest.mark.parametrize("switch,flips", [
    ("lanes=none", dict(split_cond=False)),
    ("silu=0", dict(gen_a=False)),
    ("fold_ib_gen=1", dict(fold_ib=True, ib_rows_here=True)),
    ("front_big=1", dict(front_big=True)),
    ("mlpnorm=0", dict(mlp_norm_in=False)),
    ("mlp1=0", dict(mlp_fc1=False, mlp_norm_in=False, mlp_block=False)),
])
def test_each_plan_switch_flips_the_forms_it_names_at_eight_trajectories(switch, flips):
    assert forms(CFG2, 8, 2024, plan=switch) == dataclasses.replace(CFG2_B8, **flips)


def test_kv_gemv_switch_keeps_the_generic_step_launches():
    assert forms(CYLINDER, 1, 1, "step", kv="gemv=0") == dataclasses.replace(CYL_STEP, few=False)


def test_switches_are_read_from_the_environment_at_every_call(monkeypatch):
    monkeypatch.setenv("SEA_PLAN", "chain=0,mlpblock=0")
    monkeypatch.setenv("SEA_KV", "gemv=0")
    assert resolve_forms(CFG2, 1, 2024, "full", BF16) == dataclasses.replace(CFG2_B1, mlp_block=False, mlp_fc2_proj=True, **NO_CHAIN)
    assert not resolve_forms(CYLINDER, 1, 1, "step", BF16).few
    monkeypatch.delenv("SEA_PLAN")
    monkeypatch.delenv("SEA_KV")
    assert resolve_forms(CFG2, 1, 2024, "full", BF16) == CFG2_B1
    assert resolve_forms(CYLINDER, 1, 1, "step", BF16).few


def test_resolve_forms_is_pure_and_the_switch_list_is_complete():
    src = inspect.getsource(resolve_forms)
    assert "torch.cuda" not in src and "N.lib" not in src
    doc = _switches.__doc__
    keys = set(re.findall(r'\bsw\("(\w+)"', src))
    assert {"lanes", "chain", "riders", "front", "mlpblock", "splitk"} <= keys
    for key in sorted(keys | {"graph_lanes", "enc"}):
        assert re.search(rf"\b{key}\b", doc[doc.index("SEA_PLAN "):doc.index("SEA_KV ")]), f"SEA_PLAN={key} is missing from the list in sea_amd/_switches.py"
    assert set(re.findall(r'\bkvsw\("(\w+)"', src)) == {"gemv"}


# ---------------------------------------------------------------------------------------------------------------- plans in host memory
@pytest.fixture
def host_engine(monkeypatch):
    """make(model facts ..., dtype) -> a TemporalEngine whose buffers live in host memory: the device guard and the two device launches of a plan's
    construction (the weight shadows) are stubbed; every plan builder runs as it is."""
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("libsea_hip.so is not built (python -m sea_amd.build)")
    from sea_amd import engine
    from sea_amd.models.temporal import TemporalModel

    monkeypatch.delenv("SEA_PLAN", raising=False)
    monkeypatch.delenv("SEA_KV", raising=False)
    monkeypatch.setattr(engine, "_require_gpu", lambda device: None)
    monkeypatch.setattr(engine.FlatParams, "sync", lambda self, force=False: None)
    monkeypatch.setattr(engine.FlatParams, "sync_transposed", lambda self, force=False: None)

    def make(E, F, ln, max_len, dtype):
        model = TemporalModel(1, E, 8, max_len, 8, 0, F, 2, 0.0, "sea", "learnable", "mlp", "add", 1, 1, True, ln)
        return engine.TemporalEngine(model, torch.device("cpu"), dtype)
    return make


def names(records):
    return ", ".join(r.name for r in records)


def test_device_guard_still_refuses_a_host_device():
    from sea_amd import engine
    from sea_amd.models.temporal import TemporalModel

    if not os.path.exists(N.LIB_PATH):
        pytest.skip("libsea_hip.so is not built (python -m sea_amd.build)")
    with pytest.raises(RuntimeError, match="runs only on an MI355X"):
        engine.TemporalEngine(TemporalModel(1, 64, 4, 32, 8, 0, 2, 2, 0.0, "sea", "learnable", "mlp", "add", 1, 1, True, "adaln"), torch.device("cpu"), F32)


def test_cfg2_full_context_plans(host_engine):
    eng = host_engine(256, 3, "adaln", 2048, BF16)
    p = eng.plan(1, 2024)
    assert p.forms == CFG2_B1
    assert names(p.records) == ("self.cond_adaln0_qkv_rope, self.attention, self.out_proj_down_qkv, cross0.attention, cross0.tail, cross1.attention, cross1.tail, "
                                "cross2.attention, cross2.tail, mlp.block_norm")
    assert p._clist is not None
    p = eng.plan(8, 2024)
    assert p.forms == CFG2_B8
    assert names(p.records) == ("adaln.cond_gemm.first, fork, adaln.cond_gemm.rest, self.adaln0, self.qkv_rope, self.attention, self.out_proj, join, cross.down_norm_old, "
                                "cross0.qkv_rope, cross0.attention, cross0.tail, cross1.qkv_rope, cross1.attention, cross1.tail, cross2.qkv_rope, cross2.attention, cross2.tail, "
                                "ib_add, mlp.block_norm")


def test_cfg2_fp32_plan(host_engine):
    p = host_engine(256, 3, "adaln", 2048, F32).plan(1, 2024)
    assert names(p.records) == ("adaln.silu, adaln.cond_gemm, self.adaln0, self.qkv_rope, self.attention, self.out_proj, cross.down_norm_old, cross0.qkv_rope, cross0.attention, "
                                "cross0.proj_gelu, cross0.up_sum, cross0.down_norm_new, cross1.qkv_rope, cross1.attention, cross1.proj_gelu, cross1.up_sum, cross1.down_norm_new, "
                                "cross2.qkv_rope, cross2.attention, cross2.proj_gelu, cross2.up_sum, mlp.ib_adaln2, mlp.fc1, mlp.ln_gelu, mlp.fc2, proj_norm")
    assert len(p.records) == 26


def test_cylinder_step_plans(host_engine, monkeypatch):
    from sea_amd import engine, kv_engine

    eng = host_engine(1024, 2, "adaln", 400, BF16)
    few = ("self.qkv_rope, self.attention, self.out_proj, cross.down_old, cross0.qkv_rope, cross0.attention, cross0.proj_gelu, cross0.up_sum, cross0.down_new, "
           "cross1.qkv_rope, cross1.attention, cross1.proj_gelu, cross1.up_sum, mlp.fc1, mlp.fc2, proj, final.norm")
    p = eng.plan(1, 1, "step")
    assert p.forms == CYL_STEP and names(p.records) == "adaln.silu, adaln.cond_gemm, " + few
    cp = kv_engine.cond_plan_for(eng, 5)
    assert names(cp.records) == "adaln.silu, adaln.cond_gemm, ib_add"
    hp = engine.Plan(eng, 1, 1, "step", cond=cp)   # hoisted: no condition launch, the pointers into the condition buffers advance per step
    assert hp.forms == dataclasses.replace(CYL_STEP, hoist_ib=True, ib_rows_here=False) and names(hp.records) == few and len(hp._hoisted) > 0
    monkeypatch.setenv("SEA_KV", "gemv=0")
    p = engine.Plan(eng, 1, 1, "step")
    assert not p.forms.few
    assert names(p.records) == ("adaln.silu, adaln.cond_gemm, self.adaln0, self.qkv_rope, self.attention, self.out_proj, cross.down_old, cross.norm_old, cross0.qkv_rope, "
                                "cross0.attention, cross0.proj_gelu, cross0.up_sum, cross0.down_new, cross0.norm_new, cross1.qkv_rope, cross1.attention, cross1.proj_gelu, "
                                "cross1.up_sum, mlp.ib_adaln2, mlp.fc1, mlp.ln_gelu, mlp.fc2.splitk, mlp.fc2, proj, final.norm")


def test_cfg2_training_plan(host_engine):
    from sea_amd.train_engine import TrainPlan

    p = TrainPlan(host_engine(256, 3, "adaln", 2048, BF16), 1, 70, drop_thr=0, dp=False)
    assert p.forms == forms(CFG2, 1, 70, kind=TRAINING)
    assert names(p.records) == ("adaln.silu, adaln.cond_gemm, self.adaln0, self.qkv_rope, self.attention, self.out_proj, cross.down_norm_old, cross0.qkv_rope, cross0.attention, "
                                "cross0.proj_gelu, cross0.up_sum, cross0.down_norm_new, cross1.qkv_rope, cross1.attention, cross1.proj_gelu, cross1.up_sum, cross1.down_norm_new, "
                                "cross2.qkv_rope, cross2.attention, cross2.proj_gelu, cross2.up_sum, ib_add, mlp.adaln2, mlp.fc1, mlp.ln_gelu, mlp.fc2, proj, final.norm")
    assert len(p._all_records()) == 69
