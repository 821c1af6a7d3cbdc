"""The stateful KV-cache rollout (sea_amd/rollout_session.py, utils/train_utils.py open_rollout): a session that owns its caches between calls is held
against `rollout(mode='kv')`, against the oracle's restatement of the reference's loop and against the reference's own fixtures
(tests/golden/context_rollout_*.npz), in every decode form; closed loops, state overrides, rewinds, forks (sea_kv_cache_fork, sea_amd/csrc/kvstep.hip),
independence from everything else that runs on the model, and the refusals.

Tolerances (tests/test_context_rollout_gpu.py): fp32 1e-5 between device paths and 1e-4 to the oracle / the reference fixtures; bf16 2e-2 and 3e-2."""
import pytest
import torch

from oracle import sea_oracle as O
from oracle.recipe import recipe_inputs, recipe_params
from tests.conftest import cfg_from_meta, load_golden, rel_l2
from tests.test_context_rollout_gpu import FAST_CASES, GENERIC_CASES, KS, N_STEPS, oracle_rollout
from tests.test_model_gpu import build

pytestmark = pytest.mark.gpu

PERSISTENT = (1, 256, 8, 64, 8, 0, 3, 2, True, "adaln")     # B = 1, one layer, cfg2's widths
SMALL = (2, 64, 4, 64, 8, 0, 3, 2, True, "adaln")           # seven launches (fast=1) or the generic step plan (fast=0)


def tols(dtype):
    return (1e-5, 1e-4) if dtype == "fp32" else (2e-2, 3e-2)


def open_on(m, x, ib, k):
    from sea_amd.utils.train_utils import open_rollout

    return open_rollout(m, x[:, :k].cuda().contiguous(), ib[:, :k - 1].cuda().contiguous())


def steps(s, conds):
    """conds [B, n, 1] fed one step() at a time -> [B, n, F, E]."""
    return torch.stack([s.step(conds[:, i]) for i in range(conds.shape[1])], dim=1)


def kv_rollout(m, x0, ib, n):
    from sea_amd.utils.train_utils import rollout

    return rollout(m, x0.cuda().contiguous(), ib.cuda().contiguous(), n, mode="kv")


def err(a, b):
    return rel_l2(a.cpu().numpy(), b.cpu().numpy() if torch.is_tensor(b) else b)


# ------------------------------------------------------------------------------------------------ 1. the reference's own loop
@pytest.mark.parametrize("name", ["context_rollout_adaln_f3", "context_rollout_ln_f2"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_session_matches_reference_fixture(name, dtype, monkeypatch):
    monkeypatch.setenv("SEA_KV", "")
    g = load_golden(name)
    cfg = cfg_from_meta(g["cfg"])
    m = build(cfg, dtype)
    x, ib, n = torch.from_numpy(g["x"]), torch.from_numpy(g["ib"]), int(g["steps"])
    tol = tols(dtype)[1]
    for k in [int(v) for v in g["ks"]]:
        fut = ib[:, k - 1:k - 1 + n].cuda()
        with open_on(m, x, ib, k) as s:
            a = s.advance(fut)
            assert s.position == k - 1 + n
        with open_on(m, x, ib, k) as s:
            b = steps(s, fut)
        print(name, dtype, k, err(a, g[f"pred_k{k}"]), err(b, g[f"pred_k{k}"]))
        assert err(a, g[f"pred_k{k}"]) < tol, (k, "advance")
        assert err(b, g[f"pred_k{k}"]) < tol, (k, "steps")


# ------------------------------------------------------------------------------------------------ 2. every decode form
def check_form(cfg_args, B, dtype, monkeypatch, kv, fast, ks=KS, n=N_STEPS):
    from sea_amd import kv_engine

    monkeypatch.setenv("SEA_KV", kv)
    cfg = O.OracleConfig(*cfg_args)
    m = build(cfg, dtype)
    assert kv_engine.supported(m.engine(), B) == fast
    x, _, ib = recipe_inputs(B, max(ks) + n, cfg, seed=9)
    tol_path, tol_ref = tols(dtype)
    last = None
    for k in ks:
        fut = ib[:, k - 1:k - 1 + n].cuda()
        s1, s2 = open_on(m, x, ib, k), open_on(m, x, ib, k)
        assert s1.fast == fast and (s1.kv_fast is not None) == fast and (s1.step_plan is not None) == (not fast)
        a = s1.advance(fut)
        b = steps(s2, fut)
        r = kv_rollout(m, x[:, :k], ib, n)
        ref = oracle_rollout(x, ib, k, n, cfg)
        assert a.shape == (B, n, cfg.num_variables, cfg.embed_dim) and a.dtype == torch.float32
        print(cfg_args, dtype, kv, k, err(a, b), err(a, r), err(a, ref), err(b, ref))
        assert err(a, b) < tol_path and err(a, r) < tol_path, (k, err(a, b), err(a, r))
        assert err(a, ref) < tol_ref and err(b, ref) < tol_ref, (k, err(a, ref), err(b, ref))
        assert torch.equal(s1.states()[:, k:], a) and err(s1.states()[:, :k], x[:, :k]) == 0.0
        s2.close()
        last = s1
    return m, last


def test_seven_launch_form(monkeypatch):
    cfg_args, B = FAST_CASES[0]
    check_form(cfg_args, B, "fp32", monkeypatch, "fast=1", True)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_persistent_form(dtype, monkeypatch):
    _, s = check_form(PERSISTENT, 1, dtype, monkeypatch, "fast=1", True)
    kf = s.kv_fast
    assert kf.L == 1 and kf.B == 1 and kf.G.handoff_words > kf.B * kf.F * kf.D      # the persistent form's arena, not given up


@pytest.mark.parametrize("cfg_args,B,kv", [GENERIC_CASES[0], GENERIC_CASES[3]])
def test_generic_step_plan_form(cfg_args, B, kv, monkeypatch):
    m, s = check_form(cfg_args, B, "fp32", monkeypatch, kv, False)
    assert not any(p is s.step_plan for p in m.engine()._plans.values())       # the session's plan is private


def test_fewrow_form_bf16(monkeypatch):
    cfg_args = (1, 1024, 8, 48, 8, 0, 2, 2, True, "adaln")
    _, s = check_form(cfg_args, 1, "bf16", monkeypatch, "", False, ks=(2, 9), n=3)
    assert s.step_plan.forms.few


# ------------------------------------------------------------------------------------------------ results are copies, also at B = 1 and n = 1
def _outside(t, s):
    """Does tensor t share no byte with the session's trajectory and condition buffers?"""
    lo, hi = t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()
    return all(hi <= b.data_ptr() or lo >= b.data_ptr() + b.numel() * b.element_size() for b in (s.traj, s.conds))


@pytest.mark.parametrize("kv,cfg_args,B,n", [("fast=1", PERSISTENT, 1, 4), ("fast=0", PERSISTENT, 1, 4), ("fast=1", SMALL, 2, 1), ("fast=0", SMALL, 2, 1),
                                              ("fast=1", PERSISTENT, 1, 1)])
def test_results_are_tensors_of_their_own(kv, cfg_args, B, n, monkeypatch):
    """advance / states / conditions / step hand out copies where a permuted view would already count as contiguous (B = 1, one step): kept results
    survive a rewind, other conditions and a state override, and lie outside the session's storage."""
    monkeypatch.setenv("SEA_KV", kv)
    cfg = O.OracleConfig(*cfg_args)
    m = build(cfg, "fp32")
    k = 3
    x, z_all, ib = recipe_inputs(B, k + 8, cfg, seed=71)
    s = open_on(m, x, ib, k)
    s.advance(ib[:, k - 1:k + 1].cuda())                                    # positions k, k + 1
    a = s.advance(ib[:, k + 1:k + 1 + n].cuda())                            # the next n positions
    y = s.step(ib[:, k + 1 + n])
    st, co = s.states(), s.conditions()
    kept = [t.clone() for t in (a, y, st, co)]
    for t in (a, y, st, co):
        assert t.is_contiguous() and _outside(t, s)
    s.rewind(k)                                                             # back over everything that was kept
    other = (1.0 - ib[:, k:k + 2 + n]).cuda()
    s.step(other[:, 0], state=z_all[:, 0].cuda())
    b = s.advance(other[:, 1:1 + n])
    s.step(other[:, 1 + n])
    for t, c in zip((a, y, st, co), kept):
        assert torch.equal(t, c)
    assert not torch.equal(a, b) and _outside(b, s) and _outside(s.states(), s) and _outside(s.conditions(), s)
    assert torch.equal(s.states()[:, k].cpu(), z_all[:, 0])


def test_inputs_that_require_grad_are_taken_by_value(monkeypatch):
    """Gradients through a session are out of scope: a condition or state with an autograd history leaves no graph on the session's buffers or results."""
    monkeypatch.setenv("SEA_KV", "fast=1")
    cfg = O.OracleConfig(*SMALL)
    m = build(cfg, "fp32")
    x, z_all, ib = recipe_inputs(2, 8, cfg, seed=73)
    w = torch.ones(1, device="cuda", requires_grad=True)
    s = m.engine().open_rollout(x[:, :3].cuda() * w, ib[:, :2].cuda() * w)
    y1 = s.step(ib[:, 2].cuda() * w, state=z_all[:, 0].cuda() * w)
    y2 = s.advance(ib[:, 3:6].cuda() * w)
    t = s.fork(2)
    for v in (s.traj, s.conds, t.traj, t.conds, y1, y2, s.states(), s.conditions()):
        assert not v.requires_grad and v.grad_fn is None
    plain = open_on(m, x, ib, 3)
    assert torch.equal(plain.step(ib[:, 2], state=z_all[:, 0]), y1) and torch.equal(plain.advance(ib[:, 3:6].cuda()), y2)


# ------------------------------------------------------------------------------------------------ step and advance mixed in one session
@pytest.mark.parametrize("kv,cfg_args,B,dtype", [("fast=0", SMALL, 2, "fp32"), ("", GENERIC_CASES[1][0], 2, "fp32"), ("fast=1", SMALL, 2, "fp32"),
                                                 ("", (1, 1024, 8, 48, 8, 0, 2, 2, True, "adaln"), 1, "bf16")])
def test_mixed_step_and_advance_against_the_oracle(kv, cfg_args, B, dtype, monkeypatch):
    """step, advance(4), step, advance(3), advance(4), step in ONE session: the generic step plan's hoisted condition pointers move between the
    single-step condition plan and the advance ones (re-based, evicted, re-based again); held against the oracle's loop, not against another session."""
    monkeypatch.setenv("SEA_KV", kv)
    cfg = O.OracleConfig(*cfg_args)
    m = build(cfg, dtype)
    k, n = 3, 14
    x, _, ib = recipe_inputs(B, k + n, cfg, seed=79)
    ibg = ib.cuda()
    s = open_on(m, x, ib, k)
    parts, p = [], k - 1
    for cnt in (1, 4, 1, 3, 4, 1):
        parts.append(s.step(ib[:, p]).unsqueeze(1) if cnt == 1 else s.advance(ibg[:, p:p + cnt]))
        p += cnt
    got = torch.cat(parts, dim=1)
    assert got.shape[1] == n and s.position == k - 1 + n
    ref = oracle_rollout(x, ib, k, n, cfg)
    tol_path, tol_ref = tols(dtype)
    r = kv_rollout(m, x[:, :k], ib, n)
    print(kv, cfg_args, dtype, err(got, ref), err(got, r))
    assert err(got, ref) < tol_ref and err(got, r) < tol_path
    for i in (5, 8, 9, n - 1):                                              # the step after advance(4), the end of advance(3), the start of the advance(4) behind it, the last step
        assert err(got[:, i], ref[:, i]) < tol_ref, i


# ------------------------------------------------------------------------------------------------ 3. closed loop
@pytest.mark.parametrize("kv", ["fast=1", "fast=0"])
def test_closed_loop_honours_each_condition(kv, monkeypatch):
    """The condition of every step is computed on the host from the previous output; the session is then held against the OPEN-loop oracle rollout
    under the recorded sequence (so that feedback does not amplify round-off)."""
    monkeypatch.setenv("SEA_KV", kv)
    cfg = O.OracleConfig(*SMALL)
    m = build(cfg, "fp32")
    B, k, n = 2, 3, 8
    x, _, ib = recipe_inputs(B, k, cfg, seed=31)
    s = open_on(m, x, ib, k)
    y, given, outs = x[:, k - 1], [], []
    for _ in range(n):
        c = torch.tanh(y.float().cpu().mean(dim=(1, 2))).reshape(B, 1)     # chosen after seeing the newest state
        given.append(c)
        y = s.step(c)
        outs.append(y)
    got = torch.stack(outs, dim=1)
    ib_rec = torch.cat([ib[:, :k - 1]] + [c.unsqueeze(1) for c in given], dim=1)
    assert len({float(c[0, 0]) for c in given}) == n                       # the conditions did differ from step to step
    ref = oracle_rollout(x, ib_rec, k, n, cfg)
    print(kv, err(got, ref))
    assert err(got, ref) < 1e-4
    assert torch.equal(s.conditions().cpu(), ib_rec)


# ------------------------------------------------------------------------------------------------ 4. state override
@pytest.mark.parametrize("kv,dtype", [("fast=1", "fp32"), ("fast=0", "fp32"), ("fast=1", "bf16")])
def test_state_override_equals_the_loop_on_the_edited_history(kv, dtype, monkeypatch):
    monkeypatch.setenv("SEA_KV", kv)
    cfg = O.OracleConfig(*SMALL)
    m = build(cfg, dtype)
    B, k = 2, 4
    x, z_all, ib = recipe_inputs(B, 12, cfg, seed=37)
    z = z_all[:, 0]
    s = open_on(m, x, ib, k)
    got = [s.step(ib[:, 3]), s.step(ib[:, 4])]            # predictions of positions 4, 5
    assert s.position == 5
    got.append(s.step(ib[:, 5], state=z.cuda()))          # position 5 := z, then predict position 6
    got += [s.step(ib[:, 6]), s.step(ib[:, 7])]
    got = torch.stack(got, dim=1)
    assert torch.equal(s.states()[:, 5].cpu(), z) and s.position == 8
    # the oracle's loop: two steps, replace the newest state, three more
    first = oracle_rollout(x, ib, k, 2, cfg)
    hist = torch.cat((x[:, :k], first[:, :1], z.unsqueeze(1)), dim=1)
    rest = oracle_rollout(hist, ib, 6, 3, cfg)
    ref = torch.cat((first, rest), dim=1)
    print(kv, dtype, err(got, ref))
    assert err(got, ref) < tols(dtype)[1]
    assert err(s.states()[:, 6:], rest) < tols(dtype)[1]


# ------------------------------------------------------------------------------------------------ 5. rewind
@pytest.mark.parametrize("kv,dtype", [("fast=1", "fp32"), ("fast=0", "fp32"), ("fast=1", "bf16")])
def test_rewind_then_other_conditions(kv, dtype, monkeypatch):
    monkeypatch.setenv("SEA_KV", kv)
    cfg = O.OracleConfig(*SMALL)
    m = build(cfg, dtype)
    B, k = 2, 5
    x, _, ib = recipe_inputs(B, 16, cfg, seed=41)
    other = (1.0 - ib[:, 7:10]).contiguous()              # the conditions of positions 7, 8, 9 on the second try
    s = open_on(m, x, ib, k)
    one = steps(s, ib[:, 4:10])                           # predictions of positions 5 .. 10
    assert s.position == 10
    s.rewind(7)
    assert s.position == 7 and s.states().shape[1] == 8
    two = steps(s, other)                                 # positions 8, 9, 10 again
    assert s.position == 10
    hist = torch.cat((x[:, :k], one[:, :3].cpu()), dim=1)                   # the states of positions 0 .. 7 as the session holds them
    ib2 = torch.cat((ib[:, :7], other), dim=1)
    fresh = open_on(m, hist, ib2, 8)
    three = steps(fresh, other)
    tol_path, tol_ref = tols(dtype)
    ref = oracle_rollout(x, ib2, k, 6, cfg)
    print(kv, dtype, err(two, three), err(two, ref[:, 3:]))
    assert err(two, three) < tol_path
    assert err(two, ref[:, 3:]) < tol_ref and err(one[:, :3], ref[:, :3]) < tol_ref
    assert not torch.equal(two, one[:, 3:])


# ------------------------------------------------------------------------------------------------ 6. fork
def check_fork(cfg_args, B, dtype, monkeypatch, kv, n_rep, want):
    monkeypatch.setenv("SEA_KV", kv)
    cfg = O.OracleConfig(*cfg_args)
    m = build(cfg, dtype)
    k, n = 9, 5
    x, _, ib = recipe_inputs(B, k + n, cfg, seed=43)
    g = torch.Generator().manual_seed(B * 100 + n_rep)
    futures = torch.rand(B * n_rep, n, 1, generator=g)                      # B * n_rep distinct condition sequences
    s = open_on(m, x, ib, k)
    lone = open_on(m, x, ib, k)                                             # the same session, never forked
    t = s.fork(n_rep)
    assert t.B == B * n_rep and t.position == s.position == k - 1
    assert t.forked_by in ("copy", "prefill") and (want is None or t.forked_by == want), t.forked_by
    assert s.forked_by is None
    got = t.advance(futures.cuda())
    x_rep = x[:, :k].repeat_interleave(n_rep, dim=0)                        # row b * n_rep + j: branch j of b
    ib_rep = torch.cat((ib[:, :k - 1].repeat_interleave(n_rep, dim=0), futures), dim=1)
    want_out = kv_rollout(m, x_rep, ib_rep, n)
    tol_path, tol_ref = tols(dtype)
    print(cfg_args, B, dtype, kv, n_rep, t.forked_by, err(got, want_out))
    assert err(got, want_out) < tol_path
    for row in (0, B * n_rep - 1):
        assert err(got[row:row + 1], want_out[row:row + 1]) < tol_path
    # the source goes on as if it had never been forked
    fut = ib[:, k - 1:k - 1 + n].cuda()
    assert torch.equal(s.advance(fut), lone.advance(fut))
    assert err(s.states()[:, k:], oracle_rollout(x, ib, k, n, cfg)) < tol_ref
    return t


def test_fork_seven_launch(monkeypatch):
    check_fork(SMALL, 2, "fp32", monkeypatch, "fast=1", 3, "copy")


def test_fork_seven_launch_bf16(monkeypatch):
    check_fork(SMALL, 2, "bf16", monkeypatch, "fast=1", 3, "copy")


def test_fork_persistent_to_seven_launch(monkeypatch):
    t = check_fork(PERSISTENT, 1, "fp32", monkeypatch, "fast=1", 3, "copy")
    assert t.fast and t.B == 3


def test_fork_generic(monkeypatch):
    t = check_fork(SMALL, 2, "fp32", monkeypatch, "fast=0", 3, "copy")
    assert not t.fast


def test_fork_across_a_layout_boundary(monkeypatch):
    """B * n = 66 > 64: the source decodes with sea_kv_rollout (value rows), the fork with the generic step plan (V^T)."""
    t = check_fork(SMALL, 22, "fp32", monkeypatch, "fast=1", 3, None)
    assert not t.fast and t.forked_by == "prefill"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hd", [8, 48, 256])
def test_cache_fork_op_is_a_bitwise_index_copy(dtype, hd):
    from sea_amd import ops

    g = torch.Generator(device="cuda").manual_seed(hd)
    H = 3
    entries, checks = [], []
    for B, n_rep, n_pos, cap_src, cap_dst, tr in ((2, 5, 37, 40, 64, False), (2, 5, 37, 40, 64, True), (3, 1, 13, 16, 24, False), (3, 1, 13, 16, 24, True),
                                                   (1, 5, 70, 136, 72, True), (1, 5, 1, 8, 8, True), (2, 1, 64, 64, 72, True), (1, 5, 203, 208, 256, False)):
        shape = lambda b, cap: (b, H, hd, cap) if tr else (b, H, cap, hd)
        src = torch.randn(shape(B, cap_src), device="cuda", generator=g).to(dtype)
        dst = torch.full(shape(B * n_rep, cap_dst), 7.0, device="cuda", dtype=dtype)
        entries.append(dict(src=src, dst=dst, n_pos=n_pos, transposed=tr))
        checks.append((src, dst, n_rep, n_pos, tr))
    ops.kv_cache_fork(entries, dtype)
    torch.cuda.synchronize()
    for src, dst, n_rep, n_pos, tr in checks:
        idx = torch.arange(src.shape[0], device="cuda").repeat_interleave(n_rep)          # destination row b * n_rep + j <- source row b
        want = torch.full_like(dst, 7.0)
        if tr:
            want[..., :n_pos] = src.index_select(0, idx)[..., :n_pos]
        else:
            want[:, :, :n_pos] = src.index_select(0, idx)[:, :, :n_pos]
        assert torch.equal(dst.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                           want.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), (tuple(src.shape), n_rep, n_pos, tr)   # sentinel rows included


def test_cache_fork_spans_several_launches_and_the_audit_sees_it():
    """More entries than one launch carries (N.KV_FORK_MAX), and the pointer audit of the session's launch list (rollout_session.CacheFork)."""
    from sea_amd import _native as N, ops
    from sea_amd.rollout_session import CacheFork

    n = N.KV_FORK_MAX + 3
    srcs = [torch.randn(1, 2, 16, 8, device="cuda") for _ in range(n)]
    dsts = [torch.zeros(2, 2, 24, 8, device="cuda") for _ in range(n)]
    ops.kv_cache_fork([dict(src=a, dst=b, n_pos=9, transposed=False) for a, b in zip(srcs, dsts)], torch.float32)
    for a, b in zip(srcs, dsts):
        assert torch.equal(b[:, :, :9], a[:, :, :9].expand(2, -1, -1, -1)) and not b[:, :, 9:].any()
    cf = CacheFork([dict(src=srcs[0], dst=dsts[0], n_pos=9, transposed=False)], torch.float32, "test")
    assert cf.audit() > 0
    cf.arr[0].cap_dst = 10 ** 6
    with pytest.raises(RuntimeError, match=r"past the end of its buffer"):
        cf.audit()
    cf.arr[0].cap_dst = 24
    cf.arr[0].dst += 1 << 44
    with pytest.raises(RuntimeError, match=r"pointer audit .*kv\.cache_fork.*SeaKvFork\.dst"):
        cf.audit()


# ------------------------------------------------------------------------------------------------ 7. independence
@pytest.mark.parametrize("kv,cfg_args,B", [("fast=1", SMALL, 2), ("fast=0", SMALL, 2), ("fast=1", PERSISTENT, 1)])
def test_session_is_independent_of_everything_else_on_the_model(kv, cfg_args, B, monkeypatch):
    monkeypatch.setenv("SEA_KV", kv)
    cfg = O.OracleConfig(*cfg_args)
    m = build(cfg, "bf16")
    k = 4
    x, _, ib = recipe_inputs(B, 16, cfg, seed=47)
    xg, ibg = x.cuda(), ib.cuda()
    quiet = open_on(m, x, ib, k)
    want = [quiet.step(ib[:, 3]), quiet.step(ib[:, 4]), quiet.advance(ibg[:, 5:8])]
    s = open_on(m, x, ib, k)
    got = [s.step(ib[:, 3])]
    kv_rollout(m, x[:, :2], ib, 9)                          # the engine's shared decode of the same batch size, over the same positions
    with torch.no_grad():
        m(xg[:, :7].contiguous(), ibg[:, :7].contiguous())
    other = open_on(m, x.flip(0) * 2.0, ib, 6)              # a second session on the same model and batch size
    other.step(ib[:, 0])
    other.advance(ibg[:, 1:4])
    got.append(s.step(ib[:, 4]))
    kv_rollout(m, x[:, :1], ib, 3)
    other.step(ib[:, 2])
    got.append(s.advance(ibg[:, 5:8]))
    for a, b in zip(got, want):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 8. nothing is rebuilt per step
@pytest.mark.parametrize("kv,cfg_args,B", [("fast=1", SMALL, 2), ("fast=0", SMALL, 2), ("fast=1", PERSISTENT, 1)])
def test_no_rebuilds_after_the_first_step(kv, cfg_args, B, monkeypatch):
    from sea_amd import engine, kv_engine, ptrcheck

    monkeypatch.setenv("SEA_KV", kv)
    cfg = O.OracleConfig(*cfg_args)
    m = build(cfg, "bf16")
    x, _, ib = recipe_inputs(B, 3, cfg, seed=53)
    built, audits = [], []
    for cls in (engine.Plan, kv_engine.CondPlan, kv_engine.KvFast):
        orig = cls.__init__
        monkeypatch.setattr(cls, "__init__", lambda self, *a, _o=orig, _n=cls.__name__, **kw: built.append(_n) or _o(self, *a, **kw))
    orig_check = ptrcheck.check_records
    monkeypatch.setattr(ptrcheck, "check_records", lambda *a, **kw: audits.append(1) or orig_check(*a, **kw))
    s = open_on(m, x, ib, 3)
    assert built                                            # (the counters do see the session's own objects)
    c = torch.full((B, 1), 0.25)
    s.step(c)
    buffers = (s.traj.data_ptr(), s.conds.data_ptr())
    built.clear(), audits.clear()
    for _ in range(10):
        s.step(c)
    assert not built and (ptrcheck.always() or not audits)
    conds = torch.full((B, 4, 1), 0.5, device="cuda")
    s.advance(conds)                                        # the first advance(4) builds its condition plan
    s.step(c)
    built.clear(), audits.clear()
    for _ in range(3):
        s.advance(conds)
        s.step(c)
    assert not built and (ptrcheck.always() or not audits)
    assert buffers == (s.traj.data_ptr(), s.conds.data_ptr()) and s.position == 2 + 11 + 5 + 15


# ------------------------------------------------------------------------------------------------ 9. refusals
@pytest.mark.parametrize("cfg_args,match", [
    ((1, 64, 4, 40, 8, 2, 3, 2, True, "adaln"), "exact only for src_len == 0"),
    ((1, 64, 4, 40, 8, 0, 3, 2, True, "adaln", "pool"), "KV-cache rollout does not cover exchange_mode='pool'"),
    ((1, 64, 4, 40, 8, 0, 2, 2, True, "adaln", "sea", "attention"), "KV-cache rollout does not cover ib_addition_mode='attention'"),
])
def test_models_without_an_exact_cache_are_refused(cfg_args, match):
    from sea_amd.utils.train_utils import open_rollout

    cfg = O.OracleConfig(*cfg_args)
    m = build(cfg, "fp32")
    x, _, ib = recipe_inputs(2, 6, cfg, seed=59)
    with pytest.raises(NotImplementedError, match=match):
        open_rollout(m, x[:, :4].cuda(), ib[:, :3].cuda())
    with pytest.raises(NotImplementedError, match=match):
        m.engine().open_rollout(x[:, :4].cuda(), ib[:, :3].cuda())
    eng = m.engine()
    assert not eng._plans and not eng._kv_fast and not eng.__dict__.get("_cond_plans")


@pytest.mark.parametrize("kv", ["fast=1", "fast=0"])
def test_value_errors_come_before_any_launch(kv, monkeypatch):
    from sea_amd import _native as N
    from sea_amd.utils.train_utils import open_rollout

    monkeypatch.setenv("SEA_KV", kv)
    cfg = O.OracleConfig(1, 64, 4, 24, 8, 0, 3, 2, True, "adaln")
    m = build(cfg, "fp32")
    x, _, ib = recipe_inputs(2, 24, cfg, seed=61)
    xg, ibg = x.cuda(), ib.cuda()
    for args, what in (((xg[:, :0], ibg[:, :0]), "k >= 1"), ((xg[:, :5], ibg[:, :5]), "k - 1 = 4"), ((xg[:, :5], ibg[:, :3]), "k - 1 = 4"),
                       ((xg[:, :5], ibg[:, :4, 0]), "k - 1 = 4"), ((xg[:, :5], ibg[:1, :4]), "k - 1 = 4"), ((xg[:, :5, :2], ibg[:, :4]), "F=3"),
                       ((torch.cat((xg, xg[:, :1]), dim=1), ibg), "max_len")):
        with pytest.raises(ValueError, match=what):
            open_rollout(m, *args)
    eng = m.engine()
    assert not eng._plans and not eng._kv_fast and not eng.__dict__.get("_cond_plans")      # no session was created, nothing was built or launched
    # a live session: every refusal leaves it where it was, and launches nothing
    s = open_rollout(m, xg[:, :22].contiguous(), ibg[:, :21].contiguous())
    launches = []
    lib = N.lib()
    for name in ("sea_kv_rollout", "sea_run_list_steps", "sea_run_list", "sea_kv_cache_fork", "sea_kv_cache_fill"):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _f=fn, _n=name: launches.append(_n) or _f(*a), raising=False)
    before = s.states()
    c = ibg[:, 0]
    for call, what in ((lambda: s.step(ibg[:, :2, 0]), "step condition"), (lambda: s.step(c[:1]), "step condition"), (lambda: s.step(c, state=xg[:, 0, :2]), "state"),
                       (lambda: s.advance(ibg[:, :2, 0]), "advance conditions"), (lambda: s.advance(ibg[:1, :2]), "advance conditions"),
                       (lambda: s.advance(ibg[:, :4]), "max_len"),                        # positions 21 .. 24: 24 is not below max_len
                       (lambda: s.rewind(22), "rewind"), (lambda: s.rewind(-1), "rewind"), (lambda: s.fork(0), "n >= 1"), (lambda: s.fork(-2), "n >= 1")):
        with pytest.raises(ValueError, match=what):
            call()
        assert s.position == 21
    assert not launches and torch.equal(s.states(), before)
    out = s.advance(ibg[:, 21:24])                          # up to the last position the caches hold: fine
    assert s.position == 24 and launches and out.shape[1] == 3
    launches.clear()
    with pytest.raises(ValueError, match="max_len"):
        s.step(c)                                           # would feed position 24 = max_len
    assert s.position == 24 and not launches
    s.close()
    s.close()
    for call in (lambda: s.step(c), lambda: s.advance(ibg[:, :1]), lambda: s.states(), lambda: s.rewind(0), lambda: s.fork(2), lambda: s.__enter__()):
        with pytest.raises(ValueError, match="after close"):
            call()
    assert not launches


# ------------------------------------------------------------------------------------------------ 10. the persistent form's give-up
def test_persistent_session_recovers_when_a_handoff_wait_gives_up(monkeypatch):
    cfg = O.OracleConfig(*PERSISTENT)
    m = build(cfg, "fp32")
    k, n = 3, 10
    x, _, ib = recipe_inputs(1, k + n, cfg, seed=67)
    monkeypatch.setenv("SEA_TUNE", "kv_persist=1")
    monkeypatch.setenv("SEA_KV", "fast=1")
    good = open_on(m, x, ib, k)
    small = good.kv_fast.B * good.kv_fast.F * good.kv_fast.D
    assert good.kv_fast.G.handoff_words > small                             # (it did take the persistent form)
    a = good.advance(ib[:, k - 1:k - 1 + n].cuda())
    monkeypatch.setenv("SEA_KV", "fast=1,force_err=1")
    s = open_on(m, x, ib, k)
    first = s.advance(ib[:, k - 1:k + 3].cuda())                            # attempt 0 "fails", attempt 1 recomputes these four steps
    assert s.kv_fast.G.handoff_words == small and int(s.kv_fast.err.item()) == 0      # the session gave the persistent form up for good
    rest = torch.cat([s.step(ib[:, k + 3]), s.step(ib[:, k + 4])] + list(s.advance(ib[:, k + 5:k - 1 + n].cuda()).unbind(1)), dim=0).unsqueeze(0)
    got = torch.cat((first, rest), dim=1)
    ref = oracle_rollout(x, ib, k, n, cfg)
    print(err(got, ref), err(got, a))
    assert err(got, ref) < 1e-4 and err(got, a) < 1e-5
    assert good.kv_fast.G.handoff_words > small                             # another session keeps its own form
