"""Gradient clipping by global norm and skipping of non-finite steps on the device: sea_grad_norm_ctl + sea_adamw_flat_ctl through the raw ABI
(the norm against fp64, fp64 accumulation at 1e25 / 1e-30, non-finite detection at the ends and in the grid-stride tail, a thirty-step chain with
clipped, unclipped and skipped steps against oracle.sea_oracle.adamw_update + sea_amd.optim.step_control in fp64), and through FlatAdamW: the fused
train step and the autograd path, a poisoned batch, the spatial autoencoder, two data-parallel ranks, resume, and the records of train().

References: fp64 on the same inputs; the clip / skip / count rule is sea_amd.optim.step_control (checked by hand in tests/test_grad_clip_cpu.py).
Bounds: 1e-6 relative on the norm (an fp64 sum rounded once to fp32 is 6e-8); 1e-5 on updates and moments, as tests/test_train_ops_gpu.py."""
import copy
import math
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import sea_oracle as O
from tests.conftest import cfg_from_meta, load_golden
from tests.test_model_gpu import build, gpu
from tests.test_train_ops_gpu import _fresh_temporal, _gen, _inputs, _randn, _rel, _slot, _tiny_cfg, _update_err

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GRID = 1024 * 256 * 4          # elements one round of the capped grid covers
B1, B2, EPS = 0.8, 0.995, 1e-6


# ------------------------------------------------------------------------------------------------ raw ABI helpers
def _ctl_slot(step=0):
    """A zeroed control block with 64 NaN canary words on both sides; returns (whole fp32 buffer, the 8 int32 words)."""
    whole, view = _slot(8)
    ctl = view.view(torch.int32)
    ctl.zero_()
    ctl[5] = step
    return whole, ctl


def _canaries_intact(whole, n):
    return bool(torch.isnan(whole[:64]).all() and torch.isnan(whole[64 + n:]).all())


def _norm_ctl(g, ctl, gs=1.0, max_norm=0.0, skip=0, b1=B1, b2=B2, partial=None, cap=1024):
    from sea_amd import _native as N

    partial = torch.empty(1024, device=DEV, dtype=torch.float64) if partial is None else partial
    N.check(N.lib().sea_grad_norm_ctl(g.data_ptr(), g.numel(), gs, max_norm, skip, b1, b2, partial.data_ptr(), cap, ctl.data_ptr(), N.stream_ptr()),
            "sea_grad_norm_ctl")


def _words(ctl):
    """The control block on the host: dict of the eight words."""
    w = ctl.cpu()
    f = w.view(torch.float32)
    return dict(grad_norm=float(f[0]), clip=float(f[1]), inv_bc1=float(f[2]), inv_sqrt_bc2=float(f[3]), applied=int(w[4]), step=int(w[5]),
                skipped=int(w[6]), clipped=int(w[7]), bits=w.clone())


def _log_uniform(n, gen):
    mag = 10.0 ** (-3.0 * torch.rand(n, generator=gen, dtype=torch.float64))
    sgn = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    return (mag * sgn).float()


def _relerr(a, b):
    return abs(a - b) / abs(b)


# ------------------------------------------------------------------------------------------------ 1. the norm against fp64
@pytest.mark.parametrize("gs", [1.0, 0.25])
@pytest.mark.parametrize("n", [4, 8, 1028, GRID + 4, GRID * 3 + 12])
def test_grad_norm_matches_fp64(n, gs):
    g_all, g = _slot(n)
    g.copy_(_log_uniform(n, _gen(n)).to(DEV))
    g_before = g_all.clone()
    ref = gs * float(g.double().norm())
    c_all, ctl = _ctl_slot()
    _norm_ctl(g, ctl, gs=gs)
    a = _words(ctl)
    assert _relerr(a["grad_norm"], ref) <= 1e-6, (a["grad_norm"], ref)
    assert (a["applied"], a["step"], a["skipped"], a["clipped"], a["clip"]) == (1, 1, 0, 0, 1.0)
    b1, b2 = float(torch.tensor(B1)), float(torch.tensor(B2))   # the betas as the fp32 arguments carry them
    assert _relerr(a["inv_bc1"], 1.0 / (1.0 - b1)) <= 1e-6 and _relerr(a["inv_sqrt_bc2"], 1.0 / math.sqrt(1.0 - b2)) <= 1e-6
    _norm_ctl(g, ctl, gs=gs)
    b = _words(ctl)
    assert int(b["bits"][0]) == int(a["bits"][0]), "the norm is not bitwise reproducible"
    assert b["step"] == 2
    assert _relerr(b["inv_bc1"], 1.0 / (1.0 - b1 ** 2)) <= 1e-6 and _relerr(b["inv_sqrt_bc2"], 1.0 / math.sqrt(1.0 - b2 ** 2)) <= 1e-6
    for cap in (1, 3):   # a capped grid: one / three workgroups stride over everything; nothing past partial[cap] is written
        partial = torch.full((cap + 64,), float("nan"), device=DEV, dtype=torch.float64)
        _norm_ctl(g, ctl, gs=gs, partial=partial, cap=cap)
        assert torch.isnan(partial[cap:]).all(), cap
        assert not torch.isnan(partial[:min(cap, (n // 4 + 255) // 256)]).any()
        assert _relerr(_words(ctl)["grad_norm"], ref) <= 1e-6, cap
    assert _canaries_intact(c_all, 8)
    assert torch.equal(g_all.view(torch.int32), g_before.view(torch.int32)), "g was written"


# ------------------------------------------------------------------------------------------------ 2. fp64 accumulation is real
@pytest.mark.parametrize("mag", [1e25, 1e-30])
def test_grad_norm_accumulates_in_fp64(mag):
    """|g| = 1e25: fp32 squares are inf, the norm (3.2e26) is not.  |g| = 1e-30: fp32 squares are 0, the norm (3.2e-29) is not."""
    n = 1028
    g = torch.full((n,), mag, device=DEV)
    g[::2] *= -1
    ref = float(g.double().norm())
    _, ctl = _ctl_slot()
    _norm_ctl(g, ctl, skip=1)
    a = _words(ctl)
    assert math.isfinite(a["grad_norm"]) and a["grad_norm"] != 0.0
    assert _relerr(a["grad_norm"], ref) <= 1e-6 and _relerr(a["grad_norm"], mag * math.sqrt(n)) <= 1e-6
    assert (a["applied"], a["skipped"], a["clip"]) == (1, 0, 1.0)


# ------------------------------------------------------------------------------------------------ 3. non-finite detection
@pytest.mark.parametrize("cap", [1024, 3])
@pytest.mark.parametrize("where", ["first", "last", "tail"])
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_nonfinite_element_is_detected(bad, where, cap):
    n = GRID + 4    # 262145 float4s on 262144 threads: the last float4 (elements n-4 .. n-1) is the grid-stride tail
    g = _log_uniform(n, _gen(7)).to(DEV)
    _, ctl = _ctl_slot()
    _norm_ctl(g, ctl, max_norm=1.0, skip=1, cap=cap)   # a clean call first: the words hold real values
    clean = _words(ctl)
    assert clean["applied"] == 1 and clean["step"] == 1 and clean["clipped"] == 1 and 0.0 < clean["clip"] < 1.0
    g[{"first": 0, "last": n - 1, "tail": n - 3}[where]] = bad
    _norm_ctl(g, ctl, max_norm=1.0, skip=1, cap=cap)
    a = _words(ctl)
    assert not math.isfinite(a["grad_norm"])
    assert (a["applied"], a["clip"], a["skipped"], a["step"], a["clipped"]) == (0, 0.0, 1, 1, 1)
    assert int(a["bits"][2]) == int(clean["bits"][2]) and int(a["bits"][3]) == int(clean["bits"][3]), "a skipped step touched the bias corrections"
    _norm_ctl(g, ctl, max_norm=1.0, skip=0, cap=cap)   # skipping off: applied, unclipped — what sea_adamw_flat does with such gradients
    b = _words(ctl)
    assert not math.isfinite(b["grad_norm"])
    assert (b["applied"], b["clip"], b["skipped"], b["step"], b["clipped"]) == (1, 1.0, 1, 2, 1)


# ------------------------------------------------------------------------------------------------ 4. thirty steps, clipped and skipped
def _adamw_ctl(p, g, m, v, sh, shadow_dtype, lr, wd, gs, ctl):
    from sea_amd import _native as N

    N.check(N.lib().sea_adamw_flat_ctl(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), N.ptr(sh),
                                       N.dtype_code(shadow_dtype) if shadow_dtype is not None else 0, p.numel(), lr, B1, B2, EPS, wd, gs,
                                       ctl.data_ptr(), N.stream_ptr()), "sea_adamw_flat_ctl")


def _chain_grad(n, n_tie, gen):
    gg = _log_uniform(n, gen)
    gg[:n_tie] = 0
    lr = float(1e-3 * (1 + 9 * torch.rand(1, generator=gen)))
    return gg, lr


@pytest.mark.parametrize("n,wd,gs,shadow_dtype", [(4, 0.0, 1.0, torch.bfloat16), (1028, 0.1, 0.25, torch.float32),
                                                  (2048 * 256 * 4 + 12, 0.01, 0.25, torch.bfloat16)])
def test_thirty_step_chain_with_clipping_and_skips(n, wd, gs, shadow_dtype):
    """tests/test_train_ops_gpu.py::test_adamw_flat_30_steps_match_fp64_chain through the controlled pair: max_norm is the median of the thirty
    scaled norms (about half the steps clip), steps 5 and 17 carry one inf and are skipped; the fp64 chain advances on applied steps only."""
    from sea_amd.optim import step_control
    from tests.test_train_ops_gpu import _bf16_ties

    n_tie = n // 4
    seed = n + int(wd * 1000)
    gen = _gen(seed)
    p_init = torch.randn(n, generator=gen)
    norms = []
    for _ in range(30):   # the same generator sequence as the loop below
        gg, _ = _chain_grad(n, n_tie, gen)
        norms.append(gs * float(gg.double().norm()))
    max_norm = float(torch.tensor(norms, dtype=torch.float64).median().float())

    gen = _gen(seed)
    p_all, p = _slot(n)
    m_all, m = _slot(n)
    v_all, v = _slot(n)
    g_all, g = _slot(n)
    sh_all, sh = _slot(n, dtype=shadow_dtype)
    c_all, ctl = _ctl_slot()
    partial = torch.empty(1024, device=DEV, dtype=torch.float64)
    ibits = torch.int16 if shadow_dtype == torch.bfloat16 else torch.int32
    p.copy_(torch.randn(n, generator=gen).to(DEV))
    assert torch.equal(p.cpu(), p_init)
    p[:n_tie] = _bf16_ties(n_tie, n).to(DEV)
    m.zero_()
    v.zero_()
    sh.copy_(p.to(shadow_dtype))
    p0 = p.double().clone()
    rp, rm, rv = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    state = dict(step=0, skipped=0, clipped=0)
    n_clipped = n_unclipped = 0
    for it in range(1, 31):
        gg, lr = _chain_grad(n, n_tie, gen)
        if it in (5, 17):
            gg[n - 1] = float("inf")
        g.copy_(gg.to(DEV))
        g_before = g_all.clone()
        before = [t.clone() for t in (p, m, v, sh)]
        _norm_ctl(g, ctl, gs=gs, max_norm=max_norm, skip=1, partial=partial)
        _adamw_ctl(p, g, m, v, sh, shadow_dtype, lr, wd, gs, ctl)
        r = step_control(gs * float(gg.double().norm()), max_norm, True, **state)
        state = dict(step=r["step"], skipped=r["skipped"], clipped=r["clipped"])
        a = _words(ctl)
        assert (a["applied"], a["step"], a["skipped"], a["clipped"]) == (r["applied"], r["step"], r["skipped"], r["clipped"]), (it, a, r)
        assert torch.equal(g_all.view(torch.int32), g_before.view(torch.int32)), "g was written"
        for whole in (p_all, m_all, v_all, sh_all):
            assert _canaries_intact(whole, n), f"canary overwritten at step {it}"
        assert _canaries_intact(c_all, 8)
        assert torch.equal(sh.view(ibits), p.to(shadow_dtype).view(ibits)), f"shadow != p.to({shadow_dtype}) at step {it}"
        if not r["applied"]:
            assert it in (5, 17) and a["clip"] == 0.0 and not math.isfinite(a["grad_norm"])
            for t, t0 in zip((p, m, v), before[:3]):
                assert torch.equal(t.view(torch.int32), t0.view(torch.int32)), f"a skipped step wrote at step {it}"
            assert torch.equal(sh.view(ibits), before[3].view(ibits))
            continue
        assert _relerr(a["grad_norm"], r["grad_norm"]) <= 1e-6 and abs(a["clip"] - r["clip"]) <= 1e-6 * r["clip"]
        n_clipped += r["clip"] < 1.0
        n_unclipped += r["clip"] == 1.0
        k = r["step"]   # the applied-step index: the bias correction's exponent
        rp, rm, rv = O.adamw_update(rp, g.double() * gs * r["clip"], rm, rv, k, lr, B1, B2, EPS, wd)
        if k in (1, 2, 28):
            assert _update_err(p, rp, p0, k) <= 1e-5, (k, _update_err(p, rp, p0, k))
            assert _rel(m, rm) <= 1e-5 and _rel(v, rv) <= 1e-5, k
    assert n_clipped >= 5 and n_unclipped >= 5, (n_clipped, n_unclipped)
    a = _words(ctl)
    assert (a["step"], a["skipped"], a["clipped"]) == (28, 2, state["clipped"]) and state["clipped"] == n_clipped
    if wd == 0.0:
        assert torch.equal(p[:n_tie], p0[:n_tie].float()), "elements without gradient moved"


# ------------------------------------------------------------------------------------------------ 5. clipping off through the control path
def test_control_path_without_clipping_equals_plain_adamw():
    from sea_amd import _native as N

    n, wd, gs = 1028, 0.1, 0.25
    gen = _gen(55)
    start = torch.randn(n, generator=gen).to(DEV)
    bufs = []
    for _ in range(2):
        p, m, v = start.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        bufs.append((p, m, v))
    (pa, ma, va), (pb, mb, vb) = bufs
    _, ctl = _ctl_slot()
    for step in range(1, 4):
        g = _log_uniform(n, gen).to(DEV)
        lr = 1e-3 * step
        _norm_ctl(g, ctl, gs=gs, max_norm=0.0, skip=0)
        _adamw_ctl(pa, g, ma, va, None, None, lr, wd, gs, ctl)
        N.check(N.lib().sea_adamw_flat(pb.data_ptr(), g.data_ptr(), mb.data_ptr(), vb.data_ptr(), None, 0, n, lr, B1, B2, EPS, wd, step, gs,
                                       N.stream_ptr()), "sea_adamw_flat")
        a = _words(ctl)
        assert (a["applied"], a["clip"], a["step"], a["clipped"]) == (1, 1.0, step, 0)
        assert _update_err(pa, pb.double(), start, step) <= 1e-5
        assert _rel(ma, mb) <= 1e-5 and _rel(va, vb) <= 1e-5


# ------------------------------------------------------------------------------------------------ 6. - 8. through FlatAdamW
LR = 1e-3


def _tiny():
    g = load_golden("model_tiny_adaln_f3")   # the smallest configuration tests/test_train_gpu.py trains
    cfg = cfg_from_meta(g["cfg"])
    return cfg, gpu(g["x"])[:2].contiguous(), gpu(g["tgt"])[:2].contiguous(), gpu(g["ib"])[:2].contiguous()


def _fused(m, opt, x, tgt, ib):
    return lambda: m.engine().train_step(x, tgt, ib, opt)


def _autograd(m, opt, x, tgt, ib):
    from sea_amd.utils.train_utils import SeaMSELoss

    def step():
        opt.zero_grad()
        SeaMSELoss()(m(x, ib), tgt).backward()
        opt.step()
    return step


def _first_norm(m, step_of):
    """The first step's gradient norm of a twin model: one throw-away unclipped step."""
    from sea_amd.utils.train_utils import initialize_optimizer

    opt = initialize_optimizer(m, {"learning_rate": LR})
    step_of(m, opt)()
    eng = m.engine()
    return float(eng.grads[:eng.params.n_live].double().norm())


def _check_clipped_steps(m, opt, step_fn, n_steps, max_norm, skipped=0):
    """n_steps of step_fn() on an optimizer that has applied no step yet; after each, the update of the flat parameter buffer against adamw_update
    in fp64 — fed the gradients the step left in eng.grads (unclipped) times the restated clip, from the parameters saved before the call, with
    the moments chained in fp64 from zero — and the control words against the restatement.  The moments themselves are compared with a second
    fp64 chain that uses the betas as the fp32 arguments of the ABI carry them: 1 - 0.999f is 1.3e-5 (relative) away from 0.001, which is the
    argument's rounding and not the kernel's arithmetic, and it alone would exceed the 1e-5 bound on v.  Returns the restated counters."""
    from sea_amd.optim import step_control

    eng = m.engine()
    P = eng.params
    nl = P.n_live
    state = dict(step=0, skipped=skipped, clipped=0)
    rm = rv = fm = fv = torch.zeros(nl, device=DEV, dtype=torch.float64)
    b1f, b2f = float(torch.tensor(0.9)), float(torch.tensor(0.999))
    for _ in range(n_steps):
        before = P.flat32[:nl].detach().clone()
        step_fn()
        grads = eng.grads[:nl].double()
        norm = float(grads.norm())
        r = step_control(norm, max_norm or 0.0, opt.skip_nonfinite, **state)
        state = dict(step=r["step"], skipped=r["skipped"], clipped=r["clipped"])
        s = opt.step_stats()
        assert (s["applied"], s["applied_steps"], s["skipped_steps"], s["clipped_steps"]) == (1, r["step"], r["skipped"], r["clipped"]), (s, r)
        assert _relerr(float(opt.last_grad_norm), norm) <= 1e-6 and _relerr(s["grad_norm"], norm) <= 1e-6
        assert abs(s["clip"] - r["clip"]) <= 1e-6 * r["clip"]
        rp, rm, rv = O.adamw_update(before.double(), grads * r["clip"], rm, rv, r["step"], LR, 0.9, 0.999, 1e-8, 0.0)
        err = _update_err(P.flat32[:nl], rp, before, 1)
        assert err <= 1e-5, (r["step"], err)
        _, fm, fv = O.adamw_update(before.double(), grads * r["clip"], fm, fv, r["step"], LR, b1f, b2f, 1e-8, 0.0)
        assert _rel(opt._m, fm) <= 1e-5 and _rel(opt._v, fv) <= 1e-5, (r["step"], _rel(opt._m, fm), _rel(opt._v, fv))
        if P.act_dtype != torch.float32:
            assert torch.equal(P.flat_act[:nl].view(torch.int16), P.flat32[:nl].to(torch.bfloat16).view(torch.int16))
    return state


@pytest.mark.parametrize("path", ["fused", "autograd"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_train_step_clips_by_global_norm(dtype, path):
    from sea_amd.utils.train_utils import initialize_optimizer

    cfg, x, tgt, ib = _tiny()
    step_of = (lambda m, o: _fused(m, o, x, tgt, ib)) if path == "fused" else (lambda m, o: _autograd(m, o, x, tgt, ib))
    max_norm = 0.5 * _first_norm(build(cfg, dtype).train(), step_of)
    m = build(cfg, dtype).train()
    opt = initialize_optimizer(m, {"learning_rate": LR, "max_grad_norm": max_norm})
    clips = []
    step = step_of(m, opt)

    def step_and_note():
        step()
        clips.append(opt.step_stats()["clip"])

    state = _check_clipped_steps(m, opt, step_and_note, 3, max_norm)
    assert clips[0] < 1.0 and state["step"] == 3 and state["clipped"] >= 1
    assert abs(clips[0] - 0.5) < 0.01   # half the twin's norm (the twins differ by the order of the backward's atomics)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_poisoned_batch_is_skipped(dtype):
    """One inf in the target (ordinary data) makes every gradient non-finite: with skip_nonfinite the parameters, both moments and the shadow stay
    bitwise what they were and the next clean step is step 1; without it the same batch destroys the parameters."""
    from sea_amd.utils.train_utils import initialize_optimizer

    cfg, x, tgt, ib = _tiny()
    bad_tgt = tgt.clone()
    bad_tgt[0, 0, 0, 0] = float("inf")
    m = build(cfg, dtype).train()
    opt = initialize_optimizer(m, {"learning_rate": LR, "skip_nonfinite_steps": True})
    opt.zero_grad()   # allocates the moments
    P = m.engine().params
    nl = P.n_live
    snap = lambda: [P.flat32[:nl].clone(), opt._m.clone(), opt._v.clone()] + ([P.flat_act[:nl].clone()] if dtype == "bf16" else [])   # noqa: E731
    before = snap()
    m.engine().train_step(x, bad_tgt, ib, opt)
    for a, b in zip(snap(), before):
        assert torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32), b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32))
    s = opt.step_stats()
    assert (s["applied"], s["applied_steps"], s["skipped_steps"], s["clip"]) == (0, 0, 1, 0.0) and not math.isfinite(s["grad_norm"])
    state = _check_clipped_steps(m, opt, _fused(m, opt, x, tgt, ib), 1, None, skipped=1)   # the clean step is applied step 1
    assert state["step"] == 1 and not torch.equal(P.flat32[:nl], before[0])
    assert opt.state_dict()["sea_flat"]["step"] == 1   # the applied steps, not the calls

    twin = build(cfg, dtype).train()
    plain = initialize_optimizer(twin, {"learning_rate": LR})
    twin.engine().train_step(x, bad_tgt, ib, plain)
    assert not torch.isfinite(twin.engine().params.flat32[:nl]).all(), "the poisoned batch did not poison the unprotected step"


def test_spatial_model_clipped_step():
    """FlatAdamW needs nothing from the temporal engine in particular: one clipped step of the spatial autoencoder."""
    from sea_amd.utils.train_utils import initialize_optimizer
    from tests.test_encoder_train_cpu import FIXTURES, fixture_config
    from tests.test_encoder_train_gpu import _loss_backward, _model

    z = load_golden(FIXTURES[0])
    cfg, _, _ = fixture_config(z)
    init = {kk[len("init."):]: z[kk] for kk in z.files if kk.startswith("init.")}
    x = torch.from_numpy(z["x"])

    def step_of(m, opt):
        def step():
            opt.zero_grad()
            _loss_backward(m, x)
            opt.step()
        return step

    max_norm = 0.5 * _first_norm(_model(cfg, init, "fp32"), step_of)
    m = _model(cfg, init, "fp32")
    opt = initialize_optimizer(m, {"learning_rate": LR, "max_grad_norm": max_norm, "skip_nonfinite_steps": True})
    state = _check_clipped_steps(m, opt, step_of(m, opt), 1, max_norm)
    assert state == dict(step=1, skipped=0, clipped=1) and opt.step_stats()["clip"] < 1.0


# ------------------------------------------------------------------------------------------------ 9. data parallel
def _dp_steps(x, tgt, ib, world, rank, max_norm):
    from sea_amd.parallel import parameters_in_sync, shard_batch
    from sea_amd.utils.train_utils import initialize_optimizer
    from tests.test_parallel_gpu import LR as DP_LR, STEPS, _model

    m = _model()
    eng = m.engine()
    conf = {"learning_rate": DP_LR}
    if max_norm is not None:
        conf["max_grad_norm"] = max_norm
    opt = initialize_optimizer(m, conf)
    xs, ts, cs = (shard_batch(t, rank, world).cuda().contiguous() for t in (x, tgt, ib))
    stats, calls, norm1 = [], [], None
    for step in range(STEPS):
        eng.train_step(xs, ts, cs, opt)
        if step == 0:
            norm1 = float((eng.grads[:eng.params.n_live].double() * opt.grad_scale).norm())
        assert parameters_in_sync(eng.params.flat32)
        if max_norm is not None:
            stats.append(opt.step_stats())
        calls.append((int(eng.last_allreduce_calls), len(eng.train_plan(xs.shape[0], xs.shape[1]).grad_buckets()) + 1 if world > 1 else 0, opt.allreduce_calls))
    return eng.params.flat32[:eng.params.n_live].cpu().numpy(), stats, calls, norm1


def _dp_worker(rank, world, port, backend, max_norm, ret):
    import torch.distributed as dist
    from tests.test_parallel_gpu import _data

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(rank if backend == "nccl" else 0)
    dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        ret[rank] = _dp_steps(*_data(), world, rank, max_norm)[:3]
    except Exception as e:  # pragma: no cover
        import traceback

        ret[rank] = repr(e) + "\n" + traceback.format_exc()
    finally:
        dist.destroy_process_group()


def test_data_parallel_ranks_clip_alike():
    """tests/test_parallel_gpu.py::test_train_step_world_n_equals_single_process_global_batch with a max_grad_norm that clips: the norm is that of the
    reduced mean gradient, so both ranks take the same decision without another collective."""
    from tests.test_parallel_gpu import _data, _free_port

    backend = os.environ.get("SEA_TEST_DP_BACKEND", "gloo")
    if backend == "nccl" and torch.cuda.device_count() < 2:
        pytest.skip("needs one GPU per rank")
    x, tgt, ib = _data()
    norm1 = _dp_steps(x, tgt, ib, 1, 0, None)[3]
    max_norm = 0.5 * norm1
    p_single, s_single, _, _ = _dp_steps(x, tgt, ib, 1, 0, max_norm)
    assert s_single[0]["clip"] < 1.0 and s_single[-1]["clipped_steps"] >= 1
    ret = mp.Manager().dict()
    mp.spawn(_dp_worker, args=(2, _free_port(), backend, max_norm, ret), nprocs=2, join=True)
    got = dict(ret)
    assert all(not isinstance(v, str) for v in got.values()), got
    assert np.array_equal(got[0][0], got[1][0])        # bit-identical across ranks
    assert got[0][1] == got[1][1], (got[0][1], got[1][1])   # the same norm, clip and counters on both ranks
    for r in range(2):
        p, stats, calls = got[r]
        assert np.abs(p - p_single).max() <= 2e-5, r
        assert all(seen == want and own == 0 for seen, want, own in calls), calls   # the step's slices and nothing else: no collective was added
        assert [s["applied_steps"] for s in stats] == [1, 2, 3] and stats[0]["clip"] < 1.0
        assert _relerr(stats[0]["grad_norm"], norm1) <= 2e-6   # the single-process global-batch norm: the gradients agree to 1e-6 in L2 (tests/test_parallel_gpu.py), so do their norms


# ------------------------------------------------------------------------------------------------ 10. resume
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_clipped_resume_is_bitwise(dtype):
    """Two clipped steps, state_dict(), a fresh model and optimizer load it, a third step == three steps in one go, bitwise (fixed gradient sequence
    written into p.grad, as tests/test_train_ops_gpu.py::test_flat_adamw_state_dict_resume_is_bitwise); states cross between optimizers with and
    without the options."""
    from sea_amd.utils.train_utils import SeaMSELoss, initialize_optimizer

    cfg = _tiny_cfg()
    x, tgt, ib = _inputs(cfg)
    clipped = dict(learning_rate=2e-3, weight_decay=0.01, max_grad_norm=1.0, skip_nonfinite_steps=True)
    plain = dict(learning_rate=2e-3, weight_decay=0.01)

    def start(model, conf):
        opt = initialize_optimizer(model, conf)
        opt.zero_grad()
        SeaMSELoss()(model(x, ib), tgt).backward()          # binds p.grad to the flat gradient buffer
        return opt

    a = _fresh_temporal(cfg, dtype)
    opt_a = start(a, clipped)
    live = [n for n, p in a.named_parameters() if p.grad is not None]
    seq = [{n: _randn(p.numel(), 900 + 17 * i + j, scale=10.0 ** (-(j % 3))).reshape(p.shape) for j, (n, p) in enumerate(a.named_parameters())
            if n in live} for i in range(3)]

    def run(model, opt, grads):
        params = dict(model.named_parameters())
        for G in grads:
            for n in live:
                params[n].grad.copy_(G[n])
            opt.step()

    def flat(model):
        P = model.engine().params
        return P.flat32[:P.n_live]

    p_start = flat(a).clone()
    run(a, opt_a, seq)
    assert opt_a.step_stats()["clipped_steps"] == 3
    b = _fresh_temporal(cfg, dtype)
    opt_b = start(b, clipped)
    run(b, opt_b, seq[:2])
    sd_m, sd_o = copy.deepcopy(b.state_dict()), copy.deepcopy(opt_b.state_dict())
    assert sd_o["sea_flat"]["step"] == 2 and sd_o["sea_flat"]["ctl"].shape == (8,) and not sd_o["sea_flat"]["ctl"].is_cuda
    c = _fresh_temporal(cfg, dtype, sd_m)
    opt_c = start(c, clipped)
    opt_c.load_state_dict(sd_o)
    s = opt_c.step_stats()
    assert (s["applied_steps"], s["clipped_steps"], s["skipped_steps"]) == (2, 2, 0)
    run(c, opt_c, seq[2:])
    assert torch.equal(flat(a), flat(c))
    assert opt_c.step_stats()["applied_steps"] == 3 and opt_c.step_stats()["clipped_steps"] == 3
    with torch.no_grad():
        assert torch.equal(a.eval()(x, ib), c.eval()(x, ib))

    # a clipped state into a plain optimizer: the bias correction continues from the applied steps
    d = _fresh_temporal(cfg, dtype, sd_m)
    opt_d = start(d, plain)
    opt_d.load_state_dict(sd_o)
    assert opt_d.state_dict()["sea_flat"]["step"] == 2 and "ctl" not in opt_d.state_dict()["sea_flat"]
    # ... and a plain state into an optimizer that only skips: two plain steps + one controlled == three plain steps (to the bounds of case 5)
    e = _fresh_temporal(cfg, dtype)
    opt_e = start(e, plain)
    run(e, opt_e, seq)
    f = _fresh_temporal(cfg, dtype)
    opt_f = start(f, plain)
    run(f, opt_f, seq[:2])
    sd_mf, sd_of = copy.deepcopy(f.state_dict()), copy.deepcopy(opt_f.state_dict())
    assert "ctl" not in sd_of["sea_flat"]
    h = _fresh_temporal(cfg, dtype, sd_mf)
    opt_h = start(h, dict(plain, skip_nonfinite_steps=True))
    opt_h.load_state_dict(sd_of)
    assert opt_h.step_stats()["applied_steps"] == 2
    run(h, opt_h, seq[2:])
    assert opt_h.step_stats()["applied_steps"] == 3 and opt_h.step_stats()["clip"] == 1.0
    assert _update_err(flat(h), flat(e).double(), p_start, 3) <= 1e-5


# ------------------------------------------------------------------------------------------------ 11. the records of train()
class _Tracker:
    def __init__(self):
        self.rows = []

    def record_error(self, phase, epoch, metrics):
        self.rows.append((phase, epoch, dict(metrics)))

    def log_model(self, *a):
        pass

    def finish(self):
        pass


def _temporal_config(save_dir, **extra):
    from tests.test_parallel_gpu import _train_config

    config = _train_config(save_dir, True, 1)
    config.update(epoch_num=2, validation_interval=2, **extra)
    torch.manual_seed(3)
    base = torch.randn(6, 13, 3, 64).cumsum(dim=1) * 0.1
    ib = torch.rand(6, 13, 1)
    batch = lambda sl: (base[sl, :-1], base[sl, 1:].clone(), base[sl, 1:], ib[sl, :-1])   # noqa: E731
    config["loaders"] = ([batch(slice(0, 2)), batch(slice(2, 4))], [batch(slice(4, 6))], [batch(slice(4, 6))])
    return config


@pytest.mark.parametrize("fused", [True, False])
def test_train_records_with_a_poisoned_batch(tmp_path, fused):
    from sea_amd.train.train_temporal import train

    config = _temporal_config(str(tmp_path), max_grad_norm=0.05, skip_nonfinite_steps=True, fused_step=fused)
    config["loaders"][0][1][1][0, 0, 0, 0] = float("inf")   # the second batch's target
    tr = _Tracker()
    torch.manual_seed(11)
    model = train(config, tr)
    rows = [mm for ph, _, mm in tr.rows if ph == "train"]
    assert len(rows) == 2
    for i, row in enumerate(rows):
        assert set(row) == {"Loss", "GradNorm", "SkippedSteps", "ClippedSteps"}
        assert math.isfinite(row["Loss"]) and row["Loss"] > 0 and math.isfinite(row["GradNorm"]) and row["GradNorm"] > 0
        assert row["SkippedSteps"] == i + 1 and 0 <= row["ClippedSteps"] <= i + 1
    P = model.engine().params
    assert torch.isfinite(P.flat32[:P.n_live]).all()
    # the loss is the clean batch's alone: a run over that batch only reports the same first epoch
    config1 = _temporal_config(str(tmp_path), max_grad_norm=0.05, skip_nonfinite_steps=True, fused_step=fused)
    config1["loaders"] = (config1["loaders"][0][:1],) + tuple(config1["loaders"][1:])
    tr1 = _Tracker()
    torch.manual_seed(11)
    train(config1, tr1)
    first = [mm for ph, _, mm in tr1.rows if ph == "train"][0]
    assert abs(first["Loss"] - rows[0]["Loss"]) <= 1e-5 * first["Loss"] and first["SkippedSteps"] == 0


def test_train_records_are_unchanged_without_the_options(tmp_path):
    from sea_amd.train.train_temporal import train

    tr = _Tracker()
    torch.manual_seed(11)
    train(_temporal_config(str(tmp_path)), tr)
    rows = [mm for ph, _, mm in tr.rows if ph == "train"]
    assert len(rows) == 2 and all(list(row) == ["Loss"] for row in rows)


def test_encoder_train_records_with_a_poisoned_batch(tmp_path):
    from sea_amd.train.train_encoder import train

    rng = np.random.Generator(np.random.PCG64(5))
    base = rng.standard_normal((1, 9, 3, 12)).astype(np.float32)
    mk = lambda: torch.from_numpy(base + 0.1 * rng.standard_normal((4, 9, 3, 12)).astype(np.float32))   # noqa: E731
    data, val = [mk(), mk()], [mk()]
    data[1][0, 0, 0, 0] = float("inf")
    cfg = dict(field_groups=[[0, 1], [2]], n_inp=12, MLP_hidden=32, num_layers=2, embed_dim=16, n_heads=8, block_size=9, src_len=0,
               variational=False, dropout=0.0, learning_rate=1e-3, epoch_num=2, validation_interval=2, device="cuda:0", save_dir=str(tmp_path),
               case_name="tiny", run_name="clip", loaders=(data, val, None), max_grad_norm=0.05, skip_nonfinite_steps=True)
    tr = _Tracker()
    torch.manual_seed(0)
    train(cfg, tr)
    rows = [mm for ph, _, mm in tr.rows if ph == "train"]
    assert len(rows) == 2
    for i, row in enumerate(rows):
        assert set(row) == {"Loss", "Recon_Loss", "R2", "GradNorm", "SkippedSteps", "ClippedSteps"}
        assert all(math.isfinite(row[k]) for k in ("Loss", "R2", "GradNorm")) and row["SkippedSteps"] == i + 1
    tr0 = _Tracker()
    cfg0 = {k: v for k, v in cfg.items() if k not in ("max_grad_norm", "skip_nonfinite_steps")}
    cfg0["loaders"] = ([mk(), mk()], val, None)
    torch.manual_seed(0)
    train(cfg0, tr0)
    assert all(list(mm) == ["Loss", "Recon_Loss", "R2"] for ph, _, mm in tr0.rows if ph == "train")
