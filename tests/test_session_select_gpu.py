"""select / resample on a rollout session (sea_amd/rollout_session.py) and the launch under them, sea_kv_cache_gather (sea_amd/csrc/kvstep.hip): the op is a
bitwise indexed copy in all four layout combinations (rows / V^T on either side), a selected session continues like a rollout from the selected
histories in every decode form and across the boundary between sea_kv_rollout's value rows and the generic step plan's V^T, the source is left as it
was, a resampled ensemble follows the oracle's loop row by row, and every refusal comes before a launch.

Tolerances (tests/test_context_rollout_gpu.py): fp32 1e-5 between device paths and 1e-4 to the oracle; bf16 2e-2 and 3e-2."""
import pytest
import torch

from oracle import sea_oracle as O
from oracle.recipe import recipe_inputs
from tests.test_context_rollout_gpu import oracle_rollout
from tests.test_model_gpu import build
from tests.test_rollout_session_gpu import PERSISTENT, SMALL, err, kv_rollout, open_on, tols

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 1. the op
# (B_src, index, n_pos, cap_src, cap_dst)
OP_CASES = (
    (3, [2, 0, 0, 2, 2], 37, 40, 64),       # rows repeated and a row left out
    (4, [3, 2, 1, 0], 13, 16, 16),          # a reversed permutation; n_pos = 13 in a capacity of 16
    (5, [3], 64, 64, 72),                   # a single row from many; exactly one tile
    (2, [1, 0, 1], 1, 8, 8),                # one position
    (2, [1, 1, 0], 70, 136, 72),            # a partial V^T chunk and a second tile; cap_dst < cap_src
    (2, [0, 1, 1], 203, 208, 256),          # four tiles, the last of 11 positions
    (3, [1, 2], 24, 64, 24),                # a destination filled to its capacity, smaller than the source's
)


@pytest.mark.parametrize("src_t,dst_t", [(False, False), (True, True), (False, True), (True, False)])
@pytest.mark.parametrize("hd", [8, 48, 256])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cache_gather_op_is_a_bitwise_indexed_copy(dtype, hd, src_t, dst_t):
    from sea_amd import ops

    g = torch.Generator(device="cuda").manual_seed(hd)
    H = 3
    bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
    shape = lambda b, cap, tr: (b, H, hd, cap) if tr else (b, H, cap, hd)
    checks = []
    for B_src, index, n_pos, cap_src, cap_dst in OP_CASES:
        src = torch.randn(shape(B_src, cap_src, src_t), device="cuda", generator=g).to(dtype)
        dst = torch.full(shape(len(index), cap_dst, dst_t), 7.0, device="cuda", dtype=dtype)
        ops.kv_cache_gather([dict(src=src, dst=dst, n_pos=n_pos, src_transposed=src_t, dst_transposed=dst_t)], index if n_pos % 2 else torch.tensor(index), dtype)
        checks.append((src, dst, index, n_pos))
    torch.cuda.synchronize()
    for src, dst, index, n_pos in checks:
        sel = src.index_select(0, torch.tensor(index, device="cuda"))
        if src_t != dst_t:
            sel = sel.transpose(2, 3)
        want = torch.full_like(dst, 7.0)
        if dst_t:
            want[..., :n_pos] = sel[..., :n_pos]
        else:
            want[:, :, :n_pos] = sel[:, :, :n_pos]
        assert torch.equal(dst.view(bits), want.view(bits)), (tuple(src.shape), index, n_pos)       # the sentinel beyond n_pos included


# ------------------------------------------------------------------------------------------------ 2. several launches, the audit
def test_cache_gather_spans_several_launches_and_the_audit_sees_it():
    from sea_amd import _native as N, ops
    from sea_amd.rollout_session import CacheGather

    n = N.KV_GATHER_MAX + 3
    index = [2, 2, 0, 1]
    srcs = [torch.randn(3, 2, 16, 8, device="cuda") for _ in range(n)]
    dsts = [torch.zeros(4, 2, 8, 24, device="cuda") if i % 2 else torch.zeros(4, 2, 24, 8, device="cuda") for i in range(n)]
    ops.kv_cache_gather([dict(src=a, dst=b, n_pos=9, src_transposed=False, dst_transposed=bool(i % 2)) for i, (a, b) in enumerate(zip(srcs, dsts))],
                        index, torch.float32)
    for i, (a, b) in enumerate(zip(srcs, dsts)):
        b = b.transpose(2, 3) if i % 2 else b
        assert torch.equal(b[:, :, :9], a[index][:, :, :9]) and not b[:, :, 9:].any(), i
    dev_index = torch.tensor(index, dtype=torch.int32, device="cuda")
    cg = CacheGather([dict(src=srcs[0], dst=dsts[0], n_pos=9, src_transposed=False, dst_transposed=False)], dev_index, torch.float32, "test")
    assert cg.audit() > 0
    cg.arr[0].cap_dst = 10 ** 6
    with pytest.raises(RuntimeError, match=r"past the end of its buffer"):
        cg.audit()
    cg.arr[0].cap_dst = 24
    assert cg.audit() > 0
    cg.arr[0].dst += 1 << 44
    with pytest.raises(RuntimeError, match=r"pointer audit .*kv\.cache_gather.*SeaKvGather\.dst"):
        cg.audit()


# ------------------------------------------------------------------------------------------------ 3 - 5. select in and across the decode forms
K, N_FUT = 9, 5


def check_select(m, cfg, s, twin, index, dtype, want_fast):
    """s: the source session, twin: a session brought to the same state by the same calls and never selected from."""
    tol_path, _ = tols(dtype)
    pos = s.position
    t = s.select(index)
    assert t.forked_by == "gather" and t.B == len(index) and t.position == s.position == pos and t.fast == want_fast
    states, conds = s.states(), s.conditions()
    assert torch.equal(t.states(), states[index]) and torch.equal(t.conditions(), conds[index])
    g = torch.Generator().manual_seed(len(index) * 100 + pos)
    futures = torch.rand(len(index), N_FUT, 1, generator=g)                 # a distinct condition sequence per selected row
    got = t.advance(futures.cuda())
    want = kv_rollout(m, states[index], torch.cat((conds[index], futures.cuda()), dim=1), N_FUT)
    print(cfg.embed_dim, dtype, s.B, s.fast, "->", t.B, t.fast, err(got, want))
    assert err(got, want) < tol_path
    for row in (0, len(index) - 1):
        assert err(got[row:row + 1], want[row:row + 1]) < tol_path, row
    # the source goes on as if nothing had been selected from it
    fut = torch.rand(s.B, N_FUT, 1, generator=g).cuda()
    assert torch.equal(s.advance(fut), twin.advance(fut))
    return t


def pair(cfg_args, B, dtype, monkeypatch, kv):
    monkeypatch.setenv("SEA_KV", kv)
    cfg = O.OracleConfig(*cfg_args)
    m = build(cfg, dtype)
    x, _, ib = recipe_inputs(B, K, cfg, seed=83)
    return m, cfg, open_on(m, x, ib, K), open_on(m, x, ib, K)


@pytest.mark.parametrize("cfg_args,B,kv,index,dtype,fast", [
    (SMALL, 2, "fast=1", [1, 1, 0], "fp32", True),          # seven launches
    (SMALL, 2, "fast=0", [1, 1, 0], "fp32", False),         # the generic step plan: keys as rows, values as V^T
    (PERSISTENT, 1, "fast=1", [0, 0, 0], "fp32", True),     # one persistent launch at B = 1 -> seven launches at B = 3
    (SMALL, 2, "fast=1", [1, 1, 0], "bf16", True),
])
def test_select_in_every_decode_form(cfg_args, B, kv, index, dtype, fast, monkeypatch):
    m, cfg, s, twin = pair(cfg_args, B, dtype, monkeypatch, kv)
    assert s.fast == fast
    check_select(m, cfg, s, twin, index, dtype, fast)


def test_select_from_the_generic_plan_into_value_rows(monkeypatch):
    """66 branches decode on the generic step plan (V^T); the three kept ones belong on sea_kv_rollout (value rows) again."""
    m, cfg, s, twin = pair(SMALL, 2, "fp32", monkeypatch, "fast=1")
    wide, wide_twin = s.fork(33), twin.fork(33)
    assert wide.B == 66 and not wide.fast and wide.forked_by == "prefill"
    c = torch.rand(66, 2, 1, generator=torch.Generator().manual_seed(5)).cuda()
    wide.advance(c), wide_twin.advance(c)
    t = check_select(m, cfg, wide, wide_twin, [65, 0, 40], "fp32", True)
    assert t.fast and t.kv_fast is not None and t.step_plan is None


def test_select_from_value_rows_into_the_generic_plan(monkeypatch):
    m, cfg, s, twin = pair(SMALL, 2, "fp32", monkeypatch, "fast=1")
    assert s.fast
    t = check_select(m, cfg, s, twin, [i % 2 for i in range(66)], "fp32", False)
    assert not t.fast and t.step_plan is not None and t.kv_fast is None


# ------------------------------------------------------------------------------------------------ 6. identity
@pytest.mark.parametrize("kv", ["fast=1", "fast=0"])
def test_identity_selection_keeps_bits(kv, monkeypatch):
    m, cfg, s, twin = pair(SMALL, 2, "fp32", monkeypatch, kv)
    f = torch.rand(2, N_FUT, 1, generator=torch.Generator().manual_seed(7)).cuda()
    t = s.select(list(range(2)))
    assert t.fast == s.fast and t.B == 2 and t is not s and t.traj.data_ptr() != s.traj.data_ptr()
    assert torch.equal(t.advance(f), twin.advance(f))


# ------------------------------------------------------------------------------------------------ 7. a particle filter
def test_particle_filter_against_the_oracle(monkeypatch):
    monkeypatch.setenv("SEA_KV", "fast=1")
    cfg = O.OracleConfig(*SMALL)
    m = build(cfg, "fp32")
    k, n_rep, n = 5, 3, 4
    x, _, ib = recipe_inputs(2, k, cfg, seed=89)
    g = torch.Generator().manual_seed(11)
    c1, f = torch.rand(6, 1, generator=g), torch.rand(6, n, 1, generator=g)
    index = [4, 4, 1, 0, 5, 5]
    s = open_on(m, x, ib, k).fork(n_rep)                                    # member b * 3 + j: branch j of history b
    s.step(c1.cuda())
    before = s.states()
    kept = before.clone()
    fast, bufs = s.fast, (s.traj.data_ptr(), s.conds.data_ptr())
    assert s.resample(index) is None
    assert s.position == k and s.B == 6 and s.fast == fast and s.forked_by == "copy"
    assert torch.equal(before, kept) and torch.equal(s.states(), kept[index])
    assert bufs != (s.traj.data_ptr(), s.conds.data_ptr())                  # built in fresh buffers, not copied in place
    got = s.advance(f.cuda())
    assert s.position == k + n
    # every member's explicit history: the opening states of its ancestor's history, that ancestor's step condition, its own conditions afterwards
    parent = torch.tensor(index)
    xh = x[parent // n_rep, :k]
    ibh = torch.cat((ib[parent // n_rep, :k - 1], c1[parent].unsqueeze(1), f), dim=1)
    ref = oracle_rollout(xh, ibh, k, 1 + n, cfg)
    for row in range(6):
        e_step, e_adv = err(s.states()[row, k:k + 1], ref[row, :1]), err(got[row], ref[row, 1:])
        print(row, e_step, e_adv)
        assert e_step < 1e-4 and e_adv < 1e-4, row


# ------------------------------------------------------------------------------------------------ 8. position 0
def test_select_at_position_zero_launches_nothing(monkeypatch):
    from sea_amd import _native as N

    monkeypatch.setenv("SEA_KV", "fast=1")
    cfg = O.OracleConfig(*SMALL)
    m = build(cfg, "fp32")
    x, _, ib = recipe_inputs(1, 1, cfg, seed=97)
    s = open_on(m, x, ib, 1)
    assert s.position == 0
    lib, calls = N.lib(), []
    fn = lib.sea_kv_cache_gather
    monkeypatch.setattr(lib, "sea_kv_cache_gather", lambda *a: calls.append(1) or fn(*a), raising=False)
    t = s.select([0, 0])
    assert not calls and t.B == 2 and t.position == 0 and t.forked_by == "gather"
    futures = torch.rand(2, N_FUT, 1, generator=torch.Generator().manual_seed(13))
    got = t.advance(futures.cuda())
    want = kv_rollout(m, x[[0, 0]], futures, N_FUT)
    print(err(got, want))
    assert err(got, want) < 1e-5
    t.select([1])                                                           # (the counter does see a launch once there is something to copy)
    assert calls


# ------------------------------------------------------------------------------------------------ 9. refusals
@pytest.mark.parametrize("kv", ["fast=1", "fast=0"])
def test_select_errors_come_before_any_launch(kv, monkeypatch):
    from sea_amd import _native as N

    monkeypatch.setenv("SEA_KV", kv)
    cfg = O.OracleConfig(*SMALL)
    m = build(cfg, "fp32")
    x, _, ib = recipe_inputs(2, 6, cfg, seed=101)
    s = open_on(m, x, ib, 6)
    launches = []
    lib = N.lib()
    for name in ("sea_kv_rollout", "sea_run_list_steps", "sea_run_list", "sea_kv_cache_fork", "sea_kv_cache_fill", "sea_kv_cache_gather"):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _f=fn, _n=name: launches.append(_n) or _f(*a), raising=False)
    before = s.states()
    on_device = [torch.tensor(v, device="cuda") for v in ([0, 2], [0.0, 1.0], [True, False], [[0, 1]])]
    short = torch.tensor([1], device="cuda")                                # (made before the allocator is read)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    bad = [[], (), [[0, 1]], [0.5, 1.0], [True, False], torch.tensor([0.0, 1.0]), torch.tensor([True, False]), torch.zeros(0, dtype=torch.int64),
           torch.zeros(2, 2, dtype=torch.int64), [2], [0, -1], torch.tensor([0, 1, 2]), torch.tensor([-1], dtype=torch.int32), 1, None] + on_device
    for index in bad:
        for call in (s.select, s.resample):
            with pytest.raises(ValueError, match="select"):
                call(index)
            assert s.position == 5 and s.B == 2
    for index in ([0], [0, 1, 1], torch.tensor([1, 1, 0]), short):
        with pytest.raises(ValueError, match="resample needs one index per trajectory"):
            s.resample(index)
        assert s.position == 5 and s.B == 2
    assert not launches and torch.cuda.memory_allocated() == held
    assert torch.equal(s.states(), before)
    assert s.select(torch.tensor([1, 0, 1], device="cuda")).B == 3 and launches == ["sea_kv_cache_gather"]      # a device index is fine (and synchronises)
    launches.clear()
    s.close()
    for call in (lambda: s.select([0]), lambda: s.resample([0, 1]), lambda: s.select([])):
        with pytest.raises(ValueError, match="after close"):
            call()
    assert not launches
