"""The rider tiles' condition memo without a GPU: plan_forms.resolve_forms switches PlanForms.rider_memo on where the riders and the one-launch front are planned
and off under SEA_PLAN=rider_memo=0 (the front's memo stays); the ctypes mirror of SeaRowChain, which carries the memo's pointers in group 0, agrees with the
library; a plan built in host memory fills them in ops.fill_row_chain, keeps one stamp set per tile of the rider GEMM and the pointer audit knows their extents."""
import ctypes as C
import dataclasses
import os
from types import SimpleNamespace

import pytest
import torch

from sea_amd import _native as N
from sea_amd.plan_forms import TRAINING, PlanForms, resolve_forms

BF16, F32 = torch.bfloat16, torch.float32


def facts(E=256, F=3, ln="adaln", L=1):
    return SimpleNamespace(num_variables=F, n_heads=8, num_layers=L, embed_dim=E, internal_embed_dim=E, down_dim=E // 2, mlp_hidden=8 * E, LN_type=ln,
                           exchange_mode="sea", ib_addition_mode="add", add_info_after_cross=True)


def forms(model, B, T, mode="full", dt=BF16, plan="", **kw):
    return resolve_forms(model, B, T, mode, dt, plan_switches=dict(t.split("=") for t in plan.split(",") if t), kv_switches={}, **kw)


@pytest.mark.parametrize("args,kw,tiles,front", [
    ((facts(), 1, 2024), {}, True, True),                            # the bench shape
    ((facts(), 2, 520), {}, True, True),
    ((facts(), 1, 2024), dict(plan="rider_memo=0"), False, True),    # the A/B lever: the front's memo stays
    ((facts(), 1, 2024), dict(plan="cond_memo=0"), False, False),    # switches off both
    ((facts(), 1, 2024), dict(plan="cond_memo=0,rider_memo=1"), False, False),
    ((facts(), 1, 2024), dict(plan="riders=0"), False, False),       # the gates: forms.front_chain and forms.riders
    ((facts(), 1, 2024), dict(plan="front=0"), False, False),
    ((facts(), 1, 2024), dict(plan="front3=0"), True, True),         # (the silu launch then rewrites the hidden rows at every forward)
    ((facts(), 8, 2024), {}, False, False),                          # no riders planned
    ((facts(), 1, 2024), dict(dt=F32), False, False),
    ((facts(), 1, 2024), dict(kind=TRAINING), False, False),
    ((facts(), 1, 1, "step"), {}, False, False),
])
def test_rider_memo_is_in_force_exactly_under_its_gates(args, kw, tiles, front):
    fm = forms(*args, **kw)
    assert (fm.cond_memo and fm.rider_memo) is tiles and fm.cond_memo is front
    assert fm.rider_memo == (fm.front_chain and fm.riders and "rider_memo=0" not in kw.get("plan", ""))


def test_switch_changes_no_other_form():
    on, off = forms(facts(), 1, 2024), forms(facts(), 1, 2024, plan="rider_memo=0")
    assert on.rider_memo and not off.rider_memo and on == off
    assert dataclasses.asdict(dataclasses.replace(on, rider_memo=False)) == dataclasses.asdict(off)
    assert PlanForms.__dataclass_fields__["rider_memo"].default is False and not PlanForms.__dataclass_fields__["rider_memo"].compare


def test_struct_mirror_carries_the_tile_memo_pointers():
    names = [f[0] for f in N.SeaRowChain._fields_]
    assert names[-6:] == ["tile_stamps", "tile_cond", "tile_epoch", "tile_count", "tile_sets", "pad_"]
    assert C.sizeof(N.SeaRowChain) % 8 == 0 and C.sizeof(N.SeaRowChain) <= 1024   # (the kernel holds a group's block in four dwords per lane)
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("libsea_hip.so is not built (python -m sea_amd.build)")
    lib = N.lib()
    out = (C.c_int * 48)()
    n = lib.sea_struct_sizes(out, 48)
    assert n == len(N.ABI_STRUCTS) and lib.sea_abi_version() == N.ABI_VERSION
    assert out[N.ABI_STRUCTS.index(N.SeaRowChain)] == C.sizeof(N.SeaRowChain)


def test_host_plan_fills_and_audits_the_tile_memo_pointers(monkeypatch):
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("libsea_hip.so is not built (python -m sea_amd.build)")
    from sea_amd import engine, ptrcheck
    from sea_amd.models.temporal import TemporalModel

    monkeypatch.delenv("SEA_KV", raising=False)
    monkeypatch.setattr(engine, "_require_gpu", lambda device: None)
    monkeypatch.setattr(engine.FlatParams, "sync", lambda self, force=False: None)
    monkeypatch.setattr(engine.FlatParams, "sync_transposed", lambda self, force=False: None)
    M, F, E = 1030, 3, 256
    panels, per_panel = (M + 127) // 128, 2 * F * (2 * E // 128)

    def plan(switches):
        monkeypatch.setenv("SEA_PLAN", switches)
        eng = engine.TemporalEngine(TemporalModel(1, E, 8, 1100, 8, 0, F, 2, 0.0, "sea", "learnable", "mlp", "add", 1, 1, True, "adaln"), torch.device("cpu"), BF16)
        return eng, eng.plan(1, M)

    def hosts(p):
        return [r for r in p.records if r.fn is N.lib().sea_row_chain_riders and r.args[6] > 0]

    eng, p = plan("")
    epoch = eng.params.memo_epoch
    assert p.forms.cond_memo and p.forms.rider_memo and tuple(p.memo_tile_count.shape) == (2,) and p.memo_tile_count.data_ptr() != p.memo_count.data_ptr()
    hs = hosts(p)
    assert len(hs) == F and sum(r.args[6] for r in hs) == panels * per_panel
    stamps = [t for t in p._keep if isinstance(t, torch.Tensor) and t.dtype == torch.int32 and tuple(t.shape[1:]) == (128, 2)]
    assert len(stamps) == 1 and stamps[0].shape[0] == panels * per_panel and int(stamps[0].abs().sum()) == 0   # one set per tile, zeroed
    for r in hs:
        g = r.args[0][0]
        assert g.tile_stamps == stamps[0].data_ptr() and g.tile_sets == panels * per_panel and r.args[5] + r.args[6] <= g.tile_sets
        assert g.tile_epoch == epoch.data_ptr() and g.tile_count == p.memo_tile_count.data_ptr() and not g.tile_cond   # (the condition: patched at every bind)
        assert any(tgt is not None and not isinstance(tgt, list) and C.addressof(tgt) == C.addressof(g) and fld == "tile_cond" for tgt, fld in p._c_patches)
        assert all(not q.tile_stamps and not q.tile_epoch and q.tile_sets == 0 for q in list(r.args[0])[1:])
        ext = {name: nbytes for name, _, nbytes in ptrcheck._extents(g, 2)}
        assert ext["tile_stamps"] == panels * per_panel * 1024 and ext["tile_cond"] == M * 4 and ext["tile_epoch"] == 4 and ext["tile_count"] == 8
    # the buffers a hit relies on are the plan's own and nothing else is laid over them: every rider's output and operand is an allocation of its own
    spans = []
    for g in hs[0].args[3]:
        spans.append((g.Cact, g.Cact + ((g.M - 1) * g.ldcact + g.N) * 2))
        spans.append((g.A, g.A + ((g.M - 1) * g.lda + g.K) * 2))
    assert len(spans) == 4 * F
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    owners = [t for t in p._keep if isinstance(t, torch.Tensor)]
    for lo, hi in spans:
        assert sum(1 for t in owners if t.untyped_storage().data_ptr() <= lo < t.untyped_storage().data_ptr() + t.untyped_storage().nbytes()) == 1
    # a bind patches the condition pointer of every host
    x, ib, out = torch.zeros(1, M, F, E), torch.zeros(1, M, 1), torch.zeros(1, M, F, E)
    p.bind_ptrs(x.data_ptr(), ib.data_ptr(), out.data_ptr())
    assert all(r.args[0][0].tile_cond == ib.data_ptr() for r in hs)
    names_on = [r.name for r in p.records]
    for sw, front in (("rider_memo=0", True), ("cond_memo=0", False)):
        _, q = plan(sw)
        assert q.forms.cond_memo is front and q.memo_tile_count is None and (q.memo_count is not None) == front and [r.name for r in q.records] == names_on
        for r in hosts(q):
            g = r.args[0][0]
            assert not g.tile_stamps and not g.tile_cond and not g.tile_epoch and not g.tile_count and g.tile_sets == 0
        front_rec = [r for r in q.records if r.name == "self.cond_adaln0_qkv_rope"][0]
        assert all(bool(g.memo_stamps) == front for g in front_rec.args[0])
