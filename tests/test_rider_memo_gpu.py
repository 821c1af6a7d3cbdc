"""The condition memo of the chain launches' rider tiles (plan_forms.PlanForms.rider_memo, sea_amd/csrc/chain.hip): a 128 x 128 tile of cond_mlp.2 of AdaLN_2 or of
the final norm whose live rows all carry the stamp {condition bits, weight epoch} it sees exits; its modulation stays where the last miss stored it.

The reference of every comparison is a SECOND engine built with SEA_PLAN=cond_memo=0 on the same weights (neither memo), never the code under test, and equality
is torch.equal: a hit leaves the bf16 values a miss stored.  SEA_TUNE=memo_count=1 makes one lane per tile count hits / misses into Plan.memo_tile_count (the
front's workgroups and row riders count into Plan.memo_count as before), which is how a test knows that the path it names ran.

Tiles per 128-row panel: 2 F modules (AdaLN_2 and the final norm of every field) x 2 E / 128 column tiles = 24; every tile owns a stamp set."""
import pytest
import torch

from sea_amd.models.temporal import TemporalModel

pytestmark = pytest.mark.gpu

F, E = 3, 256
SHAPES = [(1, 1030),   # a partial last panel of 6 rows; M >= 1024: mlp_block is planned
          (1, 200),    # chain launches without mlp_block
          (2, 520)]    # M = 1040: the panel of rows 512 - 639 straddles the two trajectories
PER_PANEL = 2 * F * (2 * E // 128)
FRONT = ((32, F), (64, 2 * F + 1))   # the front memo's granules (tests/test_cond_memo_gpu.py): (rows per workgroup, groups)


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


def chain_riders(plan):
    """The chain launches of a plan that carry rider tiles."""
    from sea_amd import _native as N
    return [r for r in plan.records if r.fn is N.lib().sea_row_chain_riders and r.args[6] > 0]


class Pair:
    """The engine under test and the reference engine (SEA_PLAN=cond_memo=0) on the same weights."""

    def __init__(self, monkeypatch, state=None, switches=None):
        self.mp, self.switches = monkeypatch, switches
        monkeypatch.delenv("SEA_PLAN", raising=False)
        monkeypatch.setenv("SEA_TUNE", "memo_count=1")
        self.m = build(state)
        self.ref = build(state_of(self.m))

    def plan(self, B, T):
        with self.mp.context() as c:
            if self.switches:
                c.setenv("SEA_PLAN", self.switches)
            p = self.m.engine().plan(B, T, "full")
        if self.switches is None:
            assert p.forms.cond_memo and p.forms.rider_memo and p.forms.riders and p.forms.front3, p.forms   # the forms this file names, or the tests below pass vacuously
            hosts = chain_riders(p)
            assert hosts and all(r.args[0][0].tile_stamps and r.args[0][0].tile_epoch for r in hosts)
            assert sum(r.args[6] for r in hosts) == PER_PANEL * ((B * T + 127) // 128) == hosts[0].args[0][0].tile_sets
        return p

    def reference(self, x, ib):
        with self.mp.context() as c, torch.no_grad():
            c.setenv("SEA_PLAN", "cond_memo=0")
            out = self.ref.engine().forward(x, ib).clone()
            f = self.ref.engine().plan(x.shape[0], x.shape[1], "full").forms
            assert not f.cond_memo and f.riders
        return out

    def forward(self, x, ib):
        """(output, tile hits, tile misses) of one forward of the engine under test."""
        p = self.plan(x.shape[0], x.shape[1])
        p.memo_tile_count.zero_()
        with torch.no_grad():
            out = self.m.engine().forward(x, ib).clone()
        h, s = p.memo_tile_count.tolist()
        return out, h, s


def tiles(M, rows=None):
    """Rider tiles that cover `rows` (all M rows when None)."""
    panels = {r // 128 for r in rows} if rows is not None else set(range((M + 127) // 128))
    return PER_PANEL * len(panels)


@pytest.mark.parametrize("B,T", SHAPES)
def test_first_call_misses_second_call_hits_with_other_rows(monkeypatch, B, T):
    """The second call has DIFFERENT x and the same conditions: every tile exits, and the modulation the MLP and the final norm read is last step's — a plan
    buffer aliased onto the modulation or hidden rows would show here."""
    pr = Pair(monkeypatch)
    x, ib = inputs(B, T)
    x2, _ = inputs(B, T, seed=12)
    W = tiles(B * T)
    out, h, s = pr.forward(x, ib)
    print(f"first call: tile hits {h}, misses {s} of {W}")
    assert torch.equal(out, pr.reference(x, ib)) and (h, s) == (0, W)
    out, h, s = pr.forward(x2, ib)
    print(f"second call: tile hits {h}, misses {s} of {W}")
    assert torch.equal(out, pr.reference(x2, ib)) and (h, s) == (W, 0)
    assert not torch.equal(out, pr.reference(x, ib))


@pytest.mark.parametrize("B,T", SHAPES)
def test_partial_change_misses_exactly_the_covering_tiles(monkeypatch, B, T):
    pr = Pair(monkeypatch)
    x, ib = inputs(B, T)
    M = B * T
    pr.forward(x, ib)
    old = ib.clone()
    ib[:, 100:140] += 0.25
    ib[:, -1] -= 0.5
    rows = [b * T + t for b in range(B) for t in list(range(100, 140)) + [T - 1]]
    want = tiles(M, rows)
    out, h, s = pr.forward(x, ib)
    print(f"partial change: tile hits {h}, misses {s}; covering tiles {want} of {tiles(M)}")
    assert torch.equal(out, pr.reference(x, ib))
    assert s == want and h == tiles(M) - s and s > 0 and (s < tiles(M) or M <= 256)   # (M = 200: the changed rows touch both panels)
    ib.copy_(old)   # the values of before: the stamps hold the changed ones, so the same tiles miss again
    out, h, s = pr.forward(x, ib)
    assert torch.equal(out, pr.reference(x, ib)) and s == want and h == tiles(M) - s
    out, h, s = pr.forward(x, ib)
    assert torch.equal(out, pr.reference(x, ib)) and (h, s) == (tiles(M), 0)


def weight_checker(monkeypatch, pr, x, ib):
    """check(what): the forward of the engine under test equals a FRESH reference engine on its present weights, every tile misses, and the forward after it
    hits; returns the reference output."""
    W = tiles(x.shape[0] * x.shape[1])

    def check(what):
        fresh = Pair(monkeypatch, state_of(pr.m))
        want = fresh.reference(x, ib)
        out, h, s = pr.forward(x, ib)
        print(f"{what}: equal {torch.equal(out, want)}, max |diff| {float((out - want).abs().max()):.3e}, tile hits {h}, misses {s} of {W}")
        assert torch.equal(out, want) and (h, s) == (0, W), (what, h, s)
        out, h, s = pr.forward(x, ib)
        assert torch.equal(out, want) and (h, s) == (W, 0), (what, h, s)
        return want
    return check


NAMES = ["blocks.0.ln.exp.1.2.cond_mlp.2.weight",   # AdaLN_2 of a field
         "ln.2.cond_mlp.2.weight"]                  # the final norm of a field


def test_load_state_dict_misses_everything(monkeypatch):
    B, T = 1, 200
    pr = Pair(monkeypatch)
    x, ib = inputs(B, T)
    check = weight_checker(monkeypatch, pr, x, ib)
    last = check("as built")
    for name in NAMES:
        state = state_of(pr.m)
        state[name] = state[name] * 1.5
        pr.m.load_state_dict(state)
        now = check("load_state_dict " + name)
        assert not torch.equal(last, now)
        last = now


@pytest.mark.parametrize("name", NAMES)
def test_in_place_write_through_data_misses_everything(monkeypatch, name):
    B, T = 1, 200
    pr = Pair(monkeypatch)
    x, ib = inputs(B, T)
    check = weight_checker(monkeypatch, pr, x, ib)
    first = check("as built")
    with torch.no_grad():
        dict(pr.m.named_parameters())[name].data.mul_(-2.0)
    assert not torch.equal(first, check(name))


def test_graph_replays_follow_conditions_and_weights(monkeypatch):
    B, T = 1, 1030
    pr = Pair(monkeypatch)
    x, ib = inputs(B, T)
    eng = pr.m.engine()
    W = tiles(B * T)
    with torch.no_grad():
        want = pr.reference(x, ib)
        assert torch.equal(eng.forward_graphed(x, ib), want)
        (p, ) = [g[2] for g in eng._graphs.values()]              # the graph's private plan: its stamps and counters are the ones the replays use
        assert p.forms.rider_memo and chain_riders(p)[0].args[0][0].tile_stamps
        p.memo_tile_count.zero_()
        assert torch.equal(eng.forward_graphed(x, ib), want)      # a replay: every tile hits
        assert p.memo_tile_count.tolist() == [W, 0]
        _, new = inputs(B, T, seed=14)
        ib.copy_(new)
        p.memo_tile_count.zero_()
        assert torch.equal(eng.forward_graphed(x, ib), pr.reference(x, ib))
        assert p.memo_tile_count.tolist() == [0, W]
        assert torch.equal(eng.forward_graphed(x, ib), pr.reference(x, ib))
        state = state_of(pr.m)
        for name in NAMES:
            state[name] *= 0.5
        pr.m.load_state_dict(state)
        fresh = Pair(monkeypatch, state_of(pr.m))
        want = fresh.reference(x, ib)
        assert not torch.equal(want, pr.reference(x, ib))
        p.memo_tile_count.zero_()
        assert torch.equal(eng.forward_graphed(x, ib), want)       # the graph reads the weight epoch from memory: its arguments are baked in
        assert p.memo_tile_count.tolist() == [0, W]
        assert torch.equal(eng.forward_graphed(x, ib), want)


def front_workgroups(M):
    return sum(groups * ((M + gran - 1) // gran) for gran, groups in FRONT)


def test_switches_leave_the_tile_pointers_null(monkeypatch):
    B, T = 1, 200
    M = B * T
    monkeypatch.delenv("SEA_PLAN", raising=False)
    monkeypatch.setenv("SEA_TUNE", "memo_count=1")
    m = build()
    on = m.engine().plan(B, T, "full")
    plans = {}
    for sw in ("rider_memo=0", "cond_memo=0"):
        monkeypatch.setenv("SEA_PLAN", sw)
        plans[sw] = (build(state_of(m)), )
        plans[sw] += (plans[sw][0].engine().plan(B, T, "full"), )
    monkeypatch.delenv("SEA_PLAN")
    no_tiles, neither = plans["rider_memo=0"][1], plans["cond_memo=0"][1]
    assert on.forms.cond_memo and on.forms.rider_memo and no_tiles.forms.cond_memo and not no_tiles.forms.rider_memo and not neither.forms.cond_memo
    assert [r.name for r in on.records] == [r.name for r in no_tiles.records] == [r.name for r in neither.records]
    for plan, want in ((on, True), (no_tiles, False), (neither, False)):
        hosts = chain_riders(plan)
        assert len(hosts) == F
        for r in hosts:
            g = r.args[0][0]
            assert bool(g.tile_stamps) == want and bool(g.tile_epoch) == want and bool(g.tile_count) == want and (g.tile_sets > 0) == want
            assert not any(q.tile_stamps or q.tile_cond or q.tile_epoch or q.tile_count for q in list(r.args[0])[1:])   # group 0 carries the memo
        assert (plan.memo_tile_count is not None) == want
    # under rider_memo=0 the front's memo counts as tests/test_cond_memo_gpu.py expects, and the tiles compute at every forward
    x, ib = inputs(B, T)
    x2, _ = inputs(B, T, seed=12)
    ref = Pair(monkeypatch, state_of(m))
    mo = plans["rider_memo=0"][0]
    for xx, want in ((x, [0, front_workgroups(M)]), (x2, [front_workgroups(M), 0])):
        no_tiles.memo_count.zero_()
        with monkeypatch.context() as c, torch.no_grad():
            c.setenv("SEA_PLAN", "rider_memo=0")
            out = mo.engine().forward(xx, ib).clone()
        assert no_tiles.memo_count.tolist() == want and torch.equal(out, ref.reference(xx, ib))
    # the pointer audit (it ran at the first bind) knows every buffer of the tiles' memo, and the condition pointer is the bound one
    with torch.no_grad():
        m.engine().forward(x, ib)
    ranges = on._known_ranges()
    assert on._audited
    for r in chain_riders(on):
        g = r.args[0][0]
        assert g.tile_cond == ib.data_ptr() and ranges.find(g.tile_epoch)[2] == "weight epoch"
        assert all(ranges.find(p) is not None for p in (g.tile_stamps, g.tile_cond, g.tile_count))
        assert g.tile_stamps == chain_riders(on)[0].args[0][0].tile_stamps   # one buffer, a set per tile of the whole rider GEMM
