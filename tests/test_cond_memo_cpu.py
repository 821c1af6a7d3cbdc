"""The condition memo without a GPU: plan_forms.resolve_forms switches PlanForms.cond_memo on exactly where the one-launch front and the riders are planned
(bf16, M <= 4096, AdaLN, one layer) and off under SEA_PLAN=cond_memo=0; the ctypes mirror of SeaAdalnQkv, which carries the memo's pointers, agrees with
the library; a plan built in host memory fills them in ops.fill_adaln_qkv and the pointer audit knows their extents."""
import ctypes as C
import dataclasses
import os
from types import SimpleNamespace

import pytest
import torch

from sea_amd import _native as N
from sea_amd.plan_forms import CONDITION, TRAINING, PlanForms, resolve_forms

BF16, F32 = torch.bfloat16, torch.float32


def facts(E=256, F=3, ln="adaln", L=1):
    return SimpleNamespace(num_variables=F, n_heads=8, num_layers=L, embed_dim=E, internal_embed_dim=E, down_dim=E // 2, mlp_hidden=8 * E, LN_type=ln,
                           exchange_mode="sea", ib_addition_mode="add", add_info_after_cross=True)


def forms(model, B, T, mode="full", dt=BF16, plan="", **kw):
    return resolve_forms(model, B, T, mode, dt, plan_switches=dict(t.split("=") for t in plan.split(",") if t), kv_switches={}, **kw)


@pytest.mark.parametrize("args,kw,want", [
    ((facts(), 1, 2024), {}, True),                       # the bench shape
    ((facts(), 1, 1030), {}, True),
    ((facts(), 2, 520), {}, True),
    ((facts(), 16, 70), {}, True),
    ((facts(), 1, 4096), {}, True),                       # M <= 4096 ...
    ((facts(), 1, 4097), {}, False),                      # ... and not beyond: no row chains, no riders
    ((facts(), 8, 2024), {}, False),
    ((facts(), 1, 2024), dict(dt=F32), False),            # bf16 only
    ((facts(ln="ln"), 1, 2024), {}, False),               # AdaLN only
    ((facts(L=2), 1, 2024), {}, False),                   # one layer
    ((facts(), 1, 1, "step"), {}, False),                 # full-context plans
    ((facts(), 1, 2024), dict(kind=TRAINING), False),     # inference plans
    ((facts(), 1, 2024), dict(kind=CONDITION), False),
    ((facts(), 1, 2024), dict(plan="cond_memo=0"), False),
    ((facts(), 1, 2024), dict(plan="cond_memo=1"), True),
    ((facts(), 1, 2024), dict(plan="riders=0"), False),   # the gates: forms.front_chain and forms.riders
    ((facts(), 1, 2024), dict(plan="front=0"), False),
    ((facts(), 1, 2024), dict(plan="adaln_gemm=0"), False),
    ((facts(), 1, 2024), dict(plan="chain=0"), False),
    ((facts(), 1, 2024), dict(plan="front3=0"), True),    # (the front without its third layer still has AdaLN_0's condition GEMM)
])
def test_cond_memo_is_set_exactly_under_its_gates(args, kw, want):
    fm = forms(*args, **kw)
    assert fm.cond_memo is want
    assert fm.cond_memo == (fm.front_chain and fm.riders and kw.get("plan") != "cond_memo=0")


def test_switch_changes_no_other_form():
    on, off = forms(facts(), 1, 2024), forms(facts(), 1, 2024, plan="cond_memo=0")
    assert on.cond_memo and not off.cond_memo
    assert dataclasses.replace(on, cond_memo=False) == off and dataclasses.asdict(dataclasses.replace(on, cond_memo=False)) == dataclasses.asdict(off)
    assert PlanForms.__dataclass_fields__["cond_memo"].default is False


def test_struct_mirror_carries_the_memo_pointers():
    names = [f[0] for f in N.SeaAdalnQkv._fields_]
    assert names[-7:] == ["memo_stamps", "memo_mods", "memo_epoch", "memo_count", "memo_rows", "ldmemo", "pad_"]
    assert C.sizeof(N.SeaAdalnQkv) % 8 == 0
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("libsea_hip.so is not built (python -m sea_amd.build)")
    lib = N.lib()
    out = (C.c_int * 48)()
    n = lib.sea_struct_sizes(out, 48)
    assert n == len(N.ABI_STRUCTS) and lib.sea_abi_version() == N.ABI_VERSION
    assert out[N.ABI_STRUCTS.index(N.SeaAdalnQkv)] == C.sizeof(N.SeaAdalnQkv)


def test_host_plan_fills_and_audits_the_memo_pointers(monkeypatch):
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("libsea_hip.so is not built (python -m sea_amd.build)")
    from sea_amd import engine, ptrcheck
    from sea_amd.models.temporal import TemporalModel

    monkeypatch.delenv("SEA_KV", raising=False)
    monkeypatch.setattr(engine, "_require_gpu", lambda device: None)
    monkeypatch.setattr(engine.FlatParams, "sync", lambda self, force=False: None)
    monkeypatch.setattr(engine.FlatParams, "sync_transposed", lambda self, force=False: None)

    def plan(switches):
        monkeypatch.setenv("SEA_PLAN", switches)
        eng = engine.TemporalEngine(TemporalModel(1, 256, 8, 1100, 8, 0, 3, 2, 0.0, "sea", "learnable", "mlp", "add", 1, 1, True, "adaln"), torch.device("cpu"), BF16)
        return eng, eng.plan(1, 1030)

    eng, p = plan("")
    front = [r for r in p.records if r.name == "self.cond_adaln0_qkv_rope"][0]
    epoch = eng.params.memo_epoch
    assert p.forms.cond_memo and epoch.dtype == torch.int32 and int(epoch) >= 1 and tuple(p.memo_count.shape) == (2,)
    stamps = set()
    for i, g in enumerate(front.args[0]):
        assert g.memo_epoch == epoch.data_ptr() and g.memo_count == p.memo_count.data_ptr() and g.ldmemo == 512
        assert g.memo_mods == p._mods[f"blocks.0.ln.exp.{i}.0."].data_ptr()
        stamps.add(g.memo_stamps)
        ext = {name: nbytes for name, _, nbytes in ptrcheck._extents(g, 2)}
        assert ext["memo_stamps"] == 1030 * 8 and ext["memo_mods"] == 1030 * 512 * 2 and ext["memo_epoch"] == 4 and ext["memo_count"] == 8
    assert len(stamps) == 3 and 0 not in stamps and None not in stamps   # a stamp buffer per group
    assert front.args[0][0].memo_rows and not front.args[0][1].memo_rows and front.args[6] == 6   # the row riders' stamps: group 0 carries them (6 silu groups + ib)
    names_on = [r.name for r in p.records]
    _, q = plan("cond_memo=0")
    assert not q.forms.cond_memo and q.memo_count is None and [r.name for r in q.records] == names_on
    for g in [r for r in q.records if r.name == "self.cond_adaln0_qkv_rope"][0].args[0]:
        assert not g.memo_stamps and not g.memo_mods and not g.memo_epoch and not g.memo_count and g.ldmemo == 0


def test_reads_of_parameter_data_are_counted():
    """A write through `p.data` moves no version counter; the engine's parameters count the reads of `.data` instead, and stay ordinary parameters."""
    import copy
    import pickle

    from sea_amd.engine import _WatchedParameter

    flat = torch.zeros(8)
    p = torch.nn.Parameter(torch.ones(2, 2))
    view = flat[:4].view(2, 2)
    view.copy_(p.detach())
    p.data = view
    p.__class__ = _WatchedParameter
    assert isinstance(p, torch.nn.Parameter) and p.requires_grad
    v, fv, n = p._version, flat._version, _WatchedParameter.reads
    p.data.mul_(3.0)
    assert (p._version, flat._version) == (v, fv) and _WatchedParameter.reads == n + 1 and float(flat[0]) == 3.0 and type(p.data) is torch.Tensor
    n = _WatchedParameter.reads
    (p * 2).sum().backward()
    lin = torch.nn.Linear(2, 2)
    lin.weight.__class__ = _WatchedParameter
    lin.load_state_dict(lin.state_dict())
    assert _WatchedParameter.reads == n and float(p.grad[0, 0]) == 2.0          # neither autograd nor the state dict reads `.data`
    assert type(pickle.loads(pickle.dumps(p))) is torch.nn.Parameter and isinstance(copy.deepcopy(lin).weight, torch.nn.Parameter)
