"""The condition memo of the one-launch front (plan_forms.PlanForms.cond_memo, sea_amd/csrc/adaln_qkv.hip): a workgroup of sea_adaln_qkv whose 32 rows
carry the stamp {condition bits, weight epoch} it sees skips cond_mlp.2 of AdaLN_0 and of ln_cross and reads the modulation rows the plan kept.

The reference of every comparison is a SECOND engine built with SEA_PLAN=cond_memo=0 on the same weights, never the code under test, and equality is
torch.equal: a hit reads the bf16 values a miss rounds.  SEA_TUNE=memo_count=1 makes one lane per memo workgroup count hits / misses into
Plan.memo_count, which is how a test knows that the path it names ran.  (What is memoised is the front launch: F groups of 32-row workgroups and its row riders, 64 rows
each.  The 128 x 128 rider tiles of the chain launches compute as before and are not counted.)"""
import pytest
import torch

from sea_amd.models.temporal import TemporalModel

pytestmark = pytest.mark.gpu

F, E = 3, 256
SHAPES = [(1, 1030),   # not a multiple of 32 or 128 (a partial row block); M >= 1024: mlp_block is planned
          (1, 200),    # chain launches without mlp_block
          (2, 520)]    # two trajectories
GRANULES = ((32, F),           # (rows per memo workgroup, groups): the front's workgroups, one group per field ...
            (64, 2 * F + 1))   # ... and its row riders: the hidden rows of AdaLN_2 and of the final norm of every field, the information-bottleneck rows


def build(state=None, seed=5):
    m = TemporalModel(1, E, 8, 1100, 8, 0, F, 2, 0.0, "sea", "learnable", "mlp", "add", 1, 1, True, "adaln")
    if state is None:
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for p in m.parameters():   # (no parameter at its initial zeros: every modulation depends on the condition)
                p.add_(0.03 * torch.randn(p.shape, generator=g))
    else:
        m.load_state_dict(state)
    m.set_compute_dtype("bf16")
    return m.to("cuda:0").eval()


def state_of(m):
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def inputs(B, T, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, T, F, E, generator=g).cuda(), torch.rand(B, T, 1, generator=g).cuda()


class Pair:
    """The engine under test and the reference engine (SEA_PLAN=cond_memo=0) on the same weights."""

    def __init__(self, monkeypatch, state=None):
        self.mp = monkeypatch
        monkeypatch.delenv("SEA_PLAN", raising=False)
        monkeypatch.setenv("SEA_TUNE", "memo_count=1")
        self.m = build(state)
        self.ref = build(state_of(self.m))

    def plan(self, B, T):
        p = self.m.engine().plan(B, T, "full")
        assert p.forms.cond_memo and p.forms.front_chain and p.forms.riders and p.forms.front3, p.forms   # the forms this file names, or the tests below pass vacuously
        front = p.records[0]
        assert front.name == "self.cond_adaln0_qkv_rope" and front.args[6] == 2 * F and front.args[9] is not None and front.args[0][0].memo_rows   # GRANULES
        return p

    def reference(self, x, ib):
        with self.mp.context() as c, torch.no_grad():
            c.setenv("SEA_PLAN", "cond_memo=0")
            out = self.ref.engine().forward(x, ib).clone()
            assert not self.ref.engine().plan(x.shape[0], x.shape[1], "full").forms.cond_memo
        return out

    def forward(self, x, ib):
        """(output, hits, misses) of one forward of the engine under test."""
        p = self.plan(x.shape[0], x.shape[1])
        p.memo_count.zero_()
        with torch.no_grad():
            out = self.m.engine().forward(x, ib).clone()
        h, s = p.memo_count.tolist()
        return out, h, s


def workgroups(M, rows=None):
    """Memo workgroups that cover `rows` (all M rows when None), over every memoised launch."""
    n = 0
    for gran, groups in GRANULES:
        blocks = {r // gran for r in rows} if rows is not None else set(range((M + gran - 1) // gran))
        n += groups * len(blocks)
    return n


@pytest.mark.parametrize("B,T", SHAPES)
def test_first_call_misses_second_call_hits(monkeypatch, B, T):
    pr = Pair(monkeypatch)
    x, ib = inputs(B, T)
    x2, _ = inputs(B, T, seed=12)
    W = workgroups(B * T)
    out, h, s = pr.forward(x, ib)
    assert torch.equal(out, pr.reference(x, ib)) and (h, s) == (0, W)
    out, h, s = pr.forward(x2, ib)
    assert torch.equal(out, pr.reference(x2, ib)) and (h, s) == (W, 0)
    assert not torch.equal(out, pr.reference(x, ib))


@pytest.mark.parametrize("B,T", SHAPES)
def test_partial_change_misses_exactly_the_covering_workgroups(monkeypatch, B, T):
    pr = Pair(monkeypatch)
    x, ib = inputs(B, T)
    M = B * T
    pr.forward(x, ib)
    old = ib.clone()
    ib[:, 100:140] += 0.25
    ib[:, -1] -= 0.5
    rows = [b * T + t for b in range(B) for t in list(range(100, 140)) + [T - 1]]
    out, h, s = pr.forward(x, ib)
    assert torch.equal(out, pr.reference(x, ib))
    assert s == workgroups(M, rows) and h == workgroups(M) - s and 0 < s < workgroups(M)
    ib.copy_(old)   # the values of before: the stamps hold the changed ones, so the same workgroups miss again
    out, h, s = pr.forward(x, ib)
    assert torch.equal(out, pr.reference(x, ib)) and s == workgroups(M, rows) and h == workgroups(M) - s
    out, h, s = pr.forward(x, ib)
    assert torch.equal(out, pr.reference(x, ib)) and s == 0


def test_keyed_by_value_not_by_pointer(monkeypatch):
    B, T = 2, 520
    pr = Pair(monkeypatch)
    x, ib = inputs(B, T)
    pr.forward(x, ib)
    swapped = ib.flip(0).contiguous()   # the two trajectories' conditions exchanged
    assert not torch.equal(swapped, ib)
    out, h, s = pr.forward(x, swapped)
    assert torch.equal(out, pr.reference(x, swapped)) and s > 0
    fresh = swapped.clone()             # another pointer, the same values
    assert fresh.data_ptr() != swapped.data_ptr()
    out, h, s = pr.forward(x, fresh)
    assert torch.equal(out, pr.reference(x, fresh)) and (h, s) == (workgroups(B * T), 0)


def weight_checker(monkeypatch, pr, x, ib):
    """check(what): the forward of the engine under test equals a FRESH reference engine on its present weights, every memo workgroup misses, and the
    forward after it hits; returns the reference output."""
    W = workgroups(x.shape[0] * x.shape[1])

    def check(what):
        fresh = Pair(monkeypatch, state_of(pr.m))
        want = fresh.reference(x, ib)
        out, h, s = pr.forward(x, ib)
        print(f"{what}: equal {torch.equal(out, want)}, max |diff| {float((out - want).abs().max()):.3e}, hits {h}, misses {s} of {W}")
        assert torch.equal(out, want) and (h, s) == (0, W), (what, h, s)
        out, h, s = pr.forward(x, ib)
        assert torch.equal(out, want) and (h, s) == (W, 0), (what, h, s)
        return want
    return check


def test_train_step_and_load_state_dict_miss_everything(monkeypatch):
    from sea_amd.optim import FlatAdamW

    B, T = 1, 200
    pr = Pair(monkeypatch)
    x, ib = inputs(B, T)
    tgt, _ = inputs(B, T, seed=13)
    m, check = pr.m, weight_checker(monkeypatch, pr, x, ib)
    first = check("as built")
    # one fused train step: FlatAdamW writes the bf16 shadow through raw pointers
    m.train()
    opt = FlatAdamW(m, lr=1e-2)
    m.engine().train_step(x, tgt, ib, opt)
    m.eval()
    second = check("train_step")
    assert not torch.equal(first, second)
    state = state_of(m)
    for k in state:
        if "cond_mlp" in k:
            state[k] = state[k] * 0.5
    m.load_state_dict(state)
    assert not torch.equal(second, check("load_state_dict"))


@pytest.mark.parametrize("name,factor", [("blocks.0.ln.exp.0.0.cond_mlp.2.weight", 1.5), ("blocks.0.ln_cross.1.cond_mlp.0.bias", -2.0)])
def test_in_place_write_through_data_misses_everything(monkeypatch, name, factor):
    """One in-place `p.data.mul_` on a cond_mlp.2.weight and on a cond_mlp.0.bias: the forward equals a fresh reference engine on the new weights and
    every memo workgroup misses.  `p.data` hands out a tensor with a version counter of its own, so the write moves neither flat32._version nor
    p._version; the engine's parameters report the READ of `.data` instead (engine._WatchedParameter), and the next sync() refreshes the bf16 shadow
    and moves the weight epoch on."""
    B, T = 1, 200
    pr = Pair(monkeypatch)
    x, ib = inputs(B, T)
    check = weight_checker(monkeypatch, pr, x, ib)
    first = check("as built")
    with torch.no_grad():
        dict(pr.m.named_parameters())[name].data.mul_(factor)
    assert not torch.equal(first, check(name))


def test_graph_replays_follow_conditions_and_weights(monkeypatch):
    B, T = 1, 1030
    pr = Pair(monkeypatch)
    x, ib = inputs(B, T)
    eng = pr.m.engine()
    with torch.no_grad():
        want = pr.reference(x, ib)
        assert torch.equal(eng.forward_graphed(x, ib), want)
        assert torch.equal(eng.forward_graphed(x, ib), want)      # a replay: every memo workgroup hits
        _, new = inputs(B, T, seed=14)
        ib.copy_(new)
        assert torch.equal(eng.forward_graphed(x, ib), pr.reference(x, ib))
        assert torch.equal(eng.forward_graphed(x, ib), pr.reference(x, ib))
        state = state_of(pr.m)
        state["blocks.0.ln.exp.1.0.cond_mlp.2.weight"] *= 0.5
        pr.m.load_state_dict(state)
        fresh = Pair(monkeypatch, state_of(pr.m))
        want = fresh.reference(x, ib)
        assert not torch.equal(want, pr.reference(x, ib))
        assert torch.equal(eng.forward_graphed(x, ib), want)       # the graph reads the weight epoch from memory: its arguments are baked in
        assert torch.equal(eng.forward_graphed(x, ib), want)


def test_switch_leaves_the_stamp_pointers_null(monkeypatch):
    B, T = 1, 200
    monkeypatch.delenv("SEA_PLAN", raising=False)
    m = build()
    on = m.engine().plan(B, T, "full")
    monkeypatch.setenv("SEA_PLAN", "cond_memo=0")
    off = build(state_of(m)).engine().plan(B, T, "full")
    assert on.forms.cond_memo and not off.forms.cond_memo and off.forms.front_chain and off.forms.riders
    assert [r.name for r in on.records] == [r.name for r in off.records]
    for plan, want in ((on, True), (off, False)):
        front = [r for r in plan.records if r.name == "self.cond_adaln0_qkv_rope"]
        assert len(front) == 1
        for g in front[0].args[0]:
            assert bool(g.memo_stamps) == want and bool(g.memo_mods) == want and bool(g.memo_epoch) == want and bool(g.memo_count) == want
    assert off.memo_count is None
    # the pointer audit (it ran at the first bind) knows every buffer of the memo, the engine's epoch word among them
    x, ib = inputs(B, T)
    m.engine().forward(x, ib)
    ranges = on._known_ranges()
    assert on._audited and ranges.find(m.engine().params.memo_epoch.data_ptr())[2] == "weight epoch"
    for g in on.records[0].args[0]:
        assert all(ranges.find(p) is not None for p in (g.memo_stamps, g.memo_mods, g.memo_count))
