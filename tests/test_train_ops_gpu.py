"""The loss, metric and optimizer kernels of sea_amd/csrc/train.hip (sea_mse_fwd_bwd, sea_relative_mse, sea_adamw_flat) against fp64 restatements
of their formulas (oracle.sea_oracle.mse_loss / relative_mse / adamw_update run in float64), through the public wrappers and the raw ABI, at the
sizes and layouts where a streaming kernel goes wrong: tails of n % 4 elements, 4-byte-aligned views, grid-stride loops past the capped grid,
capped partial sums, all-zero and large-offset rows, weight decay, schedules, bias correction over 30 steps, shadow rounding and resume."""
import copy

import numpy as np
import pytest
import torch

from oracle import sea_oracle as O
from oracle.recipe import recipe_inputs
from tests.conftest import load_golden
from tests.test_model_gpu import build

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def _randn(n, seed, scale=1.0):
    return (torch.randn(n, generator=_gen(seed), dtype=torch.float64) * scale).float().to(DEV)


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _elem_rel(a, b):
    """max |a - b| / |b| over the elements; where b == 0, a must be 0 too."""
    a, b = a.double(), b.double()
    return float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())


def _update_err(p, rp, p0, steps):
    """rel-L2 of the parameter update p - p0 against the fp64 chain's rp - p0, after taking out what storing p in fp32 costs: one ulp of p per
    step (p is rounded after the weight decay and after the Adam step, as torch.optim.AdamW rounds it).  That floor is no kernel error, and it is
    not small: an update of 1e-4 on a weight of 1.0 is quantised to 6e-4 of itself, and a gradient below eps gives an update of a few ulps, so a
    plain 1e-5 bound on the update cannot hold for fp32 parameters."""
    p32, q32 = p.detach().float(), p0.float()
    inf = torch.full_like(p32, float("inf"))
    ulp = torch.maximum(torch.nextafter(p32.abs(), inf) - p32.abs(), torch.nextafter(q32.abs(), inf) - q32.abs()).double()
    excess = ((p.detach().double() - rp).abs() - steps * ulp).clamp_min(0)
    return float(excess.norm() / (rp - p0.double()).norm().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ MSE
def _mse_abi(out, tgt, dout, cap=1024, scale=1.0, partial=None):
    from sea_amd import _native as N

    loss = torch.full((1,), float("nan"), device=DEV)
    partial = torch.empty(cap, device=DEV) if partial is None else partial
    N.check(N.lib().sea_mse_fwd_bwd(out.data_ptr(), tgt.data_ptr(), N.ptr(dout), loss.data_ptr(), partial.data_ptr(), cap, out.numel(),
                                    scale, N.stream_ptr()), "sea_mse_fwd_bwd")
    return loss


def _mse_ref(out, tgt, scale=1.0):
    o, t = out.double(), tgt.double()
    return O.mse_loss(o, t), 2.0 * scale * (o - t) / o.numel()


MSE_SIZES = [1, 3, 4, 5, 255, 1023, 1024 * 256 * 4 + 4, 1024 * 256 * 4 * 3 + 7]


@pytest.mark.parametrize("n", MSE_SIZES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_mse_loss_and_grad_match_fp64(n, dtype):
    """SeaMSELoss: loss to 1e-5 of the fp64 mean; (3 * loss).backward() gives 3 * 2 (out - tgt) / n.  fp32: 1e-6 per element.  bf16: the
    gradient is handed back in the input's dtype, so it is checked to bf16 rounding (2^-8 relative); its fp32 value is pinned by the ABI test."""
    from sea_amd.utils.train_utils import SeaMSELoss

    x = _randn(n, 10 + n % 97).to(dtype).requires_grad_(True)
    t = _randn(n, 20 + n % 89).to(dtype)
    loss = SeaMSELoss()(x, t)
    (3 * loss).backward()
    ref, dref = _mse_ref(x.detach(), t, scale=3.0)
    assert abs(float(loss.detach()) - float(ref)) <= 1e-5 * float(ref)
    assert x.grad.dtype == dtype and x.grad.shape == x.shape
    assert _elem_rel(x.grad, dref) <= (1e-6 if dtype == torch.float32 else 2.0 ** -8)


@pytest.mark.parametrize("n", MSE_SIZES)
def test_mse_abi_dout_grad_scale_and_determinism(n):
    out, tgt = _randn(n, 30 + n % 7), _randn(n, 40 + n % 5)
    dout = torch.full((n,), float("nan"), device=DEV)
    l1 = _mse_abi(out, tgt, dout, scale=0.25)
    ref, dref = _mse_ref(out, tgt, scale=0.25)
    assert abs(float(l1) - float(ref)) <= 1e-5 * float(ref)
    assert _elem_rel(dout, dref) <= 1e-6
    d1 = dout.clone()
    l2 = _mse_abi(out, tgt, dout, scale=0.25)
    assert torch.equal(l1, l2) and torch.equal(dout, d1), "the reduction order is fixed: a second call is bitwise equal"
    l3 = _mse_abi(out, tgt, None)   # evaluation: no gradient
    assert torch.equal(l1, l3)


@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("n,offset", [(1024 * 256 * 4 + 4, 0), (1024 * 256 * 4 * 3 + 7, 0), (100_003, 1)])
def test_mse_abi_capped_partial_sums(cap, n, offset):
    """n_partial_cap < blocks: few blocks loop over everything; nothing past the cap is written.  offset=1: the 4-byte-aligned path."""
    base_o, base_t = _randn(n + offset, 50), _randn(n + offset, 51)
    out, tgt = base_o[offset:], base_t[offset:]
    ws = torch.full((cap + 64,), float("nan"), device=DEV)
    dout = torch.empty(n, device=DEV)
    loss = _mse_abi(out, tgt, dout, cap=cap, partial=ws)
    ref, dref = _mse_ref(out, tgt)
    assert abs(float(loss.detach()) - float(ref)) <= 1e-5 * float(ref)
    assert _elem_rel(dout, dref) <= 1e-6
    assert torch.isnan(ws[cap:]).all(), "partial sums past n_partial_cap were written"
    assert torch.equal(loss, _mse_abi(out, tgt, dout, cap=cap))


def test_mse_views_misaligned_strided_and_upstream_gradient():
    """A contiguous fp32 view starting 4 bytes into its storage reaches the kernel as it is (.contiguous().float() returns it unchanged); a strided
    view is copied.  Both agree with fp64, and the gradient lands in the base tensor."""
    from sea_amd.utils.train_utils import SeaMSELoss

    big = _randn(9 * 7, 60).reshape(9, 7).requires_grad_(True)
    tgt_base = _randn(9 * 7 + 2, 61)
    x = big[1:]                                             # 28 bytes into the storage
    t = tgt_base[2:].reshape(9, 7)[1:]                      # 36 bytes in: another misalignment
    assert x.is_contiguous() and x.data_ptr() % 16 != 0
    loss = SeaMSELoss()(x, t)
    (3 * loss).backward()
    ref, dref = _mse_ref(x.detach(), t, scale=3.0)
    assert abs(float(loss.detach()) - float(ref)) <= 1e-5 * float(ref)
    assert _elem_rel(big.grad[1:], dref) <= 1e-6 and torch.equal(big.grad[0], torch.zeros(7, device=DEV))

    sb = _randn(33 * 10, 62).reshape(33, 10).requires_grad_(True)
    s = sb[:, ::3]                                          # strided
    st = _randn(33 * 4, 63).reshape(33, 4)
    loss = SeaMSELoss()(s, st)
    loss.backward()
    ref, dref = _mse_ref(s.detach(), st)
    assert abs(float(loss.detach()) - float(ref)) <= 1e-5 * float(ref) and _elem_rel(sb.grad[:, ::3], dref) <= 1e-6
    assert float(sb.grad[:, 1::3].abs().max()) == 0.0


def _tiny_cfg():
    return O.OracleConfig(1, 64, 4, 32, 8, 0, 3, 2, True, "adaln")


def test_engine_mse_loss_and_grad_matches_fp64():
    cfg = _tiny_cfg()
    eng = build(cfg, "fp32").train().engine(DEV)
    for shape, seed in (((2, 5, 3, 64), 70), ((1, 3, 3, 64), 71)):
        n = int(np.prod(shape))
        out, tgt = _randn(n, seed).reshape(shape), _randn(n, seed + 1).reshape(shape)
        loss, dout = eng.mse_loss_and_grad(out, tgt, grad_scale=0.25)
        ref, dref = _mse_ref(out, tgt, scale=0.25)
        assert abs(float(loss.detach()) - float(ref)) <= 1e-5 * float(ref) and _elem_rel(dout, dref) <= 1e-6


def test_mse_refuses_mismatched_target_before_launch():
    from sea_amd import _native as N
    from sea_amd.utils.train_utils import SeaMSELoss

    out = _randn(4 * 6, 80).reshape(4, 6)
    with pytest.raises(ValueError, match=r"\(3, 6\).*\(4, 6\)"):
        SeaMSELoss()(out, out[:3])                          # fewer elements: would be read past its end
    with pytest.raises(ValueError, match=r"\(6, 4\).*\(4, 6\)"):
        SeaMSELoss()(out, out.reshape(6, 4))
    with pytest.raises(ValueError, match="target is on cpu"):
        SeaMSELoss()(out, out.cpu())
    eng = build(_tiny_cfg(), "fp32").train().engine(DEV)
    o = _randn(2 * 3 * 3 * 64, 81).reshape(2, 3, 3, 64)
    with pytest.raises(ValueError, match="bfloat16"):
        eng.mse_loss_and_grad(o, o.to(torch.bfloat16))      # would be reinterpreted as fp32 on the device
    with pytest.raises(ValueError, match="does not match"):
        eng.mse_loss_and_grad(o, o[:1])
    # the ABI refuses what the host would never pass: n = 0 and pointers that are not 4-byte aligned
    raw = torch.zeros(64, device=DEV, dtype=torch.uint8)
    loss, part = torch.empty(1, device=DEV), torch.empty(4, device=DEV)
    assert N.lib().sea_mse_fwd_bwd(o.data_ptr(), o.data_ptr(), 0, loss.data_ptr(), part.data_ptr(), 4, 0, 1.0, N.stream_ptr()) != 0
    assert N.lib().sea_mse_fwd_bwd(raw.data_ptr() + 2, o.data_ptr(), 0, loss.data_ptr(), part.data_ptr(), 4, 4, 1.0, N.stream_ptr()) != 0
    assert N.lib().sea_relative_mse(raw.data_ptr() + 2, o.data_ptr(), loss.data_ptr(), 1, 4, N.stream_ptr()) != 0


# ------------------------------------------------------------------------------------------------ relative MSE
def _rel_ref(p, t, dim=-1):
    return O.relative_mse(p.double(), t.double(), dim=dim)


REL_DS = [1, 2, 3, 4, 5, 7, 63, 64, 65, 257, 419, 420, 4099]


@pytest.mark.parametrize("d", REL_DS)
def test_relative_mse_rows_by_d(d):
    """Every row count of {1, 2, 3, 5, 4097} (the last wave of a block partly idle), aligned and 4 bytes into the storage; 1e-5 per row."""
    from sea_amd.utils.train_utils import relativeMSE

    for rows in (1, 2, 3, 5, 4097):
        for off in (0, 1):
            n = rows * d
            t = _randn(n + off, 90 + d)[off:].reshape(rows, d)
            p = _randn(n + off, 91 + d)[off:].reshape(rows, d)
            p.mul_(0.3).add_(t)
            y = relativeMSE(p, t)
            assert y.shape == (rows,)
            assert _elem_rel(y, _rel_ref(p, t)) <= 1e-5, (rows, off)


@pytest.mark.parametrize("dim", [-1, 0, 2, 3])
def test_relative_mse_dims_of_4d(dim):
    from sea_amd.utils.train_utils import relativeMSE, relativeMSE_with_time

    tr, T, Np, F = 2, 3, 419, 3
    t = _randn(tr * T * Np * F, 100).reshape(tr, T, Np, F)
    p = t + 0.1 * _randn(tr * T * Np * F, 101).reshape(tr, T, Np, F)
    ref = _rel_ref(p, t, dim=dim)
    y = relativeMSE(p, t, dim=dim)
    assert y.shape == ref.shape and _elem_rel(y, ref) <= 1e-5
    assert torch.equal(relativeMSE_with_time(p, t, dim=dim), y)


def test_relative_mse_zero_truth_and_epsilon():
    """All-zero truth rows: the 1e-8 epsilon is the whole denominator.  Tiny truth rows: it is comparable to sum t^2."""
    from sea_amd.utils.train_utils import relativeMSE

    d = 65
    t = _randn(6 * d, 110).reshape(6, d)
    p = _randn(6 * d, 111).reshape(6, d)
    t[0] = 0
    t[1] = 0
    p[1] = 0                                                # 0 / 1e-8 = 0
    p[2] = 1e-6 * p[2]
    t[2] = 0
    t[3] = 1e-5 * t[3]                                      # sum t^2 ~ 6.5e-9
    p[3] = t[3] + 1e-5 * p[3]
    y = relativeMSE(p, t)
    ref = _rel_ref(p, t)
    assert float(y[1]) == 0.0
    keep = ref != 0
    assert _elem_rel(y[keep], ref[keep]) <= 1e-5


@pytest.mark.parametrize("d", [420, 4099])
def test_relative_mse_large_common_offset(d):
    """Rows of 1e3 + noise: sum t^2 ~ 1e6 d must still be accumulated to 1e-5."""
    from sea_amd.utils.train_utils import relativeMSE

    rows = 37
    t = 1e3 + _randn(rows * d, 120).reshape(rows, d)
    p = t + 1e-2 * _randn(rows * d, 121).reshape(rows, d)
    assert _elem_rel(relativeMSE(p, t), _rel_ref(p, t)) <= 1e-5


@pytest.mark.parametrize("d,off", [((1 << 20) + 4, 0), ((1 << 20) + 3, 0), ((1 << 20) + 4, 1)])
def test_relative_mse_abi_one_long_row(d, off):
    from sea_amd import _native as N

    t = _randn(d + off, 130)[off:]
    p = t + 0.5 * _randn(d + off, 131)[off:]
    y = torch.full((3,), float("nan"), device=DEV)
    N.check(N.lib().sea_relative_mse(p.data_ptr(), t.data_ptr(), y.data_ptr(), 1, d, N.stream_ptr()), "sea_relative_mse")
    assert _elem_rel(y[:1], _rel_ref(p, t).reshape(1)) <= 1e-5
    assert torch.isnan(y[1:]).all()


# ------------------------------------------------------------------------------------------------ AdamW, direct
def _bf16_ties(n, seed):
    """fp32 values exactly half-way between two bf16 neighbours (low 16 bits 0x8000), with even and odd upper halves."""
    hi = torch.randint(0x3c00, 0x4000, (n,), generator=_gen(seed), dtype=torch.int32)
    sign = torch.randint(0, 2, (n,), generator=_gen(seed + 1), dtype=torch.int32) << 31
    bits = sign | (hi << 16) | 0x8000
    return bits.view(torch.float32)


def _slot(n, pad=64, dtype=torch.float32):
    """A NaN-filled buffer with `pad` canary elements on both sides; returns (whole, view)."""
    whole = torch.full((n + 2 * pad,), float("nan"), device=DEV, dtype=dtype)
    return whole, whole[pad:pad + n]


ADAMW_CASES = [  # n, weight_decay, grad_scale, shadow dtype
    (4, 0.0, 1.0, torch.bfloat16),
    (8, 0.01, 0.25, None),
    (1028, 0.1, 1.0, torch.bfloat16),
    (1028, 0.01, 0.25, torch.float32),
    (2048 * 256 * 4 + 12, 0.1, 0.25, torch.bfloat16),
    (2048 * 256 * 4 + 12, 0.0, 1.0, None),
]


@pytest.mark.parametrize("n,wd,gs,shadow_dtype", ADAMW_CASES)
def test_adamw_flat_30_steps_match_fp64_chain(n, wd, gs, shadow_dtype):
    """30 steps, a fresh gradient (|g| in 1e-3..1) and lr every step, betas (0.8, 0.995), eps 1e-6: p, m, v against adamw_update chained in
    fp64 after steps 1, 2 and 30 (the update p - p0 to 1e-5 beyond the fp32 storage floor of _update_err; m and v to 1e-5 rel-L2).  A quarter of the elements get no gradient and start
    on bf16 rounding ties, so with wd = 0 they stay there and pin round-to-nearest-even of the shadow, which must be bitwise p.to(bf16) after
    every step.  Nothing outside p, m, v (and the shadow when one is given) is written; g is read only."""
    from sea_amd import _native as N

    b1, b2, eps = 0.8, 0.995, 1e-6
    gen = _gen(n + int(wd * 1000))
    p_all, p = _slot(n)
    m_all, m = _slot(n)
    v_all, v = _slot(n)
    g_all, g = _slot(n)
    p.copy_(torch.randn(n, generator=gen).to(DEV))
    n_tie = n // 4
    p[:n_tie] = _bf16_ties(n_tie, n).to(DEV)
    m.zero_()
    v.zero_()
    sh_all, sh = _slot(n, dtype=shadow_dtype) if shadow_dtype is not None else (None, None)
    p0 = p.double().clone()
    rp, rm, rv = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for step in range(1, 31):
        mag = 10.0 ** (-3.0 * torch.rand(n, generator=gen, dtype=torch.float64))
        sgn = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
        gg = (mag * sgn).float()
        gg[:n_tie] = 0
        g.copy_(gg.to(DEV))
        g_before = g_all.clone()
        lr = float(1e-3 * (1 + 9 * torch.rand(1, generator=gen)))
        N.check(N.lib().sea_adamw_flat(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), N.ptr(sh),
                                       N.dtype_code(shadow_dtype) if shadow_dtype is not None else 0, n, lr, b1, b2, eps, wd, step, gs,
                                       N.stream_ptr()), "sea_adamw_flat")
        rp, rm, rv = O.adamw_update(rp, g.double() * gs, rm, rv, step, lr, b1, b2, eps, wd)
        assert torch.equal(g_all.view(torch.int32), g_before.view(torch.int32)), "g was written"
        for whole in (p_all, m_all, v_all) + ((sh_all,) if sh_all is not None else ()):
            assert torch.isnan(whole[:64]).all() and torch.isnan(whole[64 + n:]).all(), f"canary overwritten at step {step}"
        if sh is not None:
            want = p.to(shadow_dtype)
            assert torch.equal(sh.view(torch.int16 if shadow_dtype == torch.bfloat16 else torch.int32),
                               want.view(torch.int16 if shadow_dtype == torch.bfloat16 else torch.int32)), f"shadow != p.to({shadow_dtype}) at step {step}"
        if step in (1, 2, 30):
            assert _update_err(p, rp, p0, step) <= 1e-5, (step, _update_err(p, rp, p0, step))
            assert _rel(m, rm) <= 1e-5 and _rel(v, rv) <= 1e-5, step
    if wd == 0.0:
        assert torch.equal(p[:n_tie], p0[:n_tie].float()), "elements without gradient moved"


def test_adamw_flat_refuses_bad_arguments():
    from sea_amd import _native as N

    buf = torch.zeros(16, device=DEV)
    args = lambda n, step, off=0: (buf.data_ptr() + off, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 0, 0, n, 1e-3, 0.9, 0.999, 1e-8, 0.0,  # noqa: E731
                                   step, 1.0, N.stream_ptr())
    assert N.lib().sea_adamw_flat(*args(6, 1)) != 0
    assert N.lib().sea_adamw_flat(*args(8, 0)) != 0
    assert N.lib().sea_adamw_flat(*args(8, 1, off=4)) != 0
    assert torch.equal(buf, torch.zeros(16, device=DEV))


# ------------------------------------------------------------------------------------------------ AdamW through a model
def _fresh_temporal(cfg, dtype, sd=None):
    from sea_amd.models.temporal import TemporalModel

    if sd is None:
        return build(cfg, dtype).train()
    m = TemporalModel(cfg.num_layers, cfg.embed_dim, cfg.n_heads, cfg.max_len, cfg.scale_ratio, cfg.src_len, cfg.num_variables,
                      cfg.down_proj, 0.0, cfg.exchange_mode, "learnable", cfg.ib_scale_mode, cfg.ib_addition_mode, 1, 1, cfg.add_info_after_cross, cfg.LN_type)
    m.load_state_dict({k: t.cpu() for k, t in sd.items()}, strict=True)
    m.set_compute_dtype(dtype)
    return m.to(DEV).train()


def _inputs(cfg):
    x, tgt, ib = recipe_inputs(2, 12, cfg, seed=7)
    return x.to(DEV), tgt.to(DEV), ib.to(DEV)


def _check_scheduled_steps(m, opt, sched, step_fn, n_steps, wd):
    """Run n_steps of step_fn() (a forward + backward), opt.step(), sched.step(); each step's parameters against adamw_update in fp64 at the
    scheduled lr, fed the gradients the model produced.  Parameters without a gradient (dead) stay bitwise unchanged."""
    p0 = {k: p.detach().clone() for k, p in m.named_parameters()}
    ref = {}
    lrs = []
    for step in range(1, n_steps + 1):
        opt.zero_grad()
        step_fn()
        lr = opt.param_groups[0]["lr"]
        lrs.append(lr)
        opt.step()
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().double().clone() for k, p in m.named_parameters() if p.grad is not None}   # what the step read: it leaves them
        assert grads, "no live parameters"
        sched.step()
        for k, p in m.named_parameters():
            if k not in grads:
                assert torch.equal(p, p0[k]), (k, step)
                continue
            rp, rm, rv = ref.get(k, (p0[k].double(), torch.zeros_like(grads[k]), torch.zeros_like(grads[k])))
            ref[k] = O.adamw_update(rp, grads[k], rm, rv, step, lr, 0.9, 0.999, 1e-8, wd)
            err = _update_err(p, ref[k][0], p0[k], step)
            assert err <= 1e-5, (k, step, err)
    assert lrs == sorted(lrs) and lrs[0] < lrs[-1], "the linear schedule did not raise the lr"
    return ref


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_flat_adamw_linear_schedule_weight_decay_and_resume(dtype):
    from sea_amd.utils.train_utils import SeaMSELoss, initialize_optimizer

    cfg = _tiny_cfg()
    x, tgt, ib = _inputs(cfg)
    conf = dict(learning_rate=3e-3, weight_decay=0.05, scheduler="linear", epoch_num=5)
    m = _fresh_temporal(cfg, dtype)
    opt, sched = initialize_optimizer(m, conf)
    _check_scheduled_steps(m, opt, sched, lambda: SeaMSELoss()(m(x, ib), tgt).backward(), 4, 0.05)

    # step() with no backward since zero_grad(): nothing moves and the bias-correction step does not advance
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    opt.zero_grad()
    opt.step()
    assert opt.state_dict()["sea_flat"]["step"] == 4
    assert all(torch.equal(p, before[k]) for k, p in m.named_parameters())

    # the weight packs the forward reads were refreshed by the step: the forward equals that of a model built from the state_dict
    P = m.engine().params
    if dtype == "bf16":
        assert torch.equal(P.flat_act[:P.n_live].view(torch.int16), P.flat32[:P.n_live].to(torch.bfloat16).view(torch.int16))
    fresh = _fresh_temporal(cfg, dtype, m.state_dict())
    with torch.no_grad():
        a, b = m.eval()(x, ib), fresh.eval()(x, ib)
    assert torch.equal(a, b) if dtype == "fp32" else _rel(a, b) <= 1e-2
    # ... and the training forward and backward (the transposed pack feeds the data gradients): same loss, same gradients up to the order of
    # the backward's fp32 atomics.  A stale transposed pack would be ~lr away from the weights: fp32 catches it, bf16 rounding may hide it.
    m.train()
    fresh.train()
    opt.zero_grad()
    lm, lf = SeaMSELoss()(m(x, ib), tgt), SeaMSELoss()(fresh(x, ib), tgt)
    assert torch.equal(lm, lf) if dtype == "fp32" else abs(float(lm) - float(lf)) <= 1e-2 * float(lf)
    lm.backward()
    lf.backward()
    gm = torch.cat([p.grad.reshape(-1) for p in m.parameters() if p.grad is not None])
    gf = torch.cat([p.grad.reshape(-1) for p in fresh.parameters() if p.grad is not None])
    assert gm.shape == gf.shape and _rel(gm, gf) <= (1e-5 if dtype == "fp32" else 2e-2)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_flat_adamw_state_dict_resume_is_bitwise(dtype):
    """k steps, state_dict() of model and optimizer, a fresh pair loads them, k more steps == 2k uninterrupted steps, bitwise.  The gradients are a
    fixed sequence written into p.grad (a backward accumulates with fp32 atomics, so two backwards need not agree to the bit)."""
    from sea_amd.utils.train_utils import SeaMSELoss, initialize_optimizer

    cfg = _tiny_cfg()
    x, tgt, ib = _inputs(cfg)
    conf = dict(learning_rate=2e-3, weight_decay=0.01)
    k = 3

    def start(model):
        opt = initialize_optimizer(model, conf)
        opt.zero_grad()
        SeaMSELoss()(model(x, ib), tgt).backward()          # binds p.grad to the flat gradient buffer
        return opt

    a = _fresh_temporal(cfg, dtype)
    opt_a = start(a)
    live = [n for n, p in a.named_parameters() if p.grad is not None]
    seq = [{n: _randn(p.numel(), 300 + 17 * i + j, scale=10.0 ** (-(j % 3))).reshape(p.shape) for j, (n, p) in enumerate(a.named_parameters())
            if n in live} for i in range(2 * k)]

    def run(model, opt, grads):
        params = dict(model.named_parameters())
        for G in grads:
            for n in live:
                params[n].grad.copy_(G[n])
            opt.step()

    run(a, opt_a, seq)
    b = _fresh_temporal(cfg, dtype)
    opt_b = start(b)
    run(b, opt_b, seq[:k])
    sd_m, sd_o = copy.deepcopy(b.state_dict()), copy.deepcopy(opt_b.state_dict())
    c = _fresh_temporal(cfg, dtype, sd_m)
    opt_c = start(c)
    opt_c.load_state_dict(sd_o)
    assert opt_c.state_dict()["sea_flat"]["step"] == k
    run(c, opt_c, seq[k:])
    pa, pc = dict(a.named_parameters()), dict(c.named_parameters())
    for n in pa:
        assert torch.equal(pa[n], pc[n]), n
    with torch.no_grad():
        assert torch.equal(a.eval()(x, ib), c.eval()(x, ib))


def test_flat_adamw_spatial_model_schedule_and_weight_decay():
    """The spatial autoencoder shares FlatAdamW: the same per-step fp64 check, linear schedule and weight decay, on a small fixture model."""
    from tests.test_encoder_train_cpu import FIXTURES, fixture_config
    from tests.test_encoder_train_gpu import _loss_backward, _model
    from sea_amd.utils.train_utils import initialize_optimizer

    z = load_golden(FIXTURES[0])
    cfg, _, _ = fixture_config(z)
    init = {kk[len("init."):]: z[kk] for kk in z.files if kk.startswith("init.")}
    m = _model(cfg, init, "fp32")
    x = torch.from_numpy(z["x"])
    opt, sched = initialize_optimizer(m, dict(learning_rate=1e-3, weight_decay=0.05, scheduler="linear", epoch_num=5))
    _check_scheduled_steps(m, opt, sched, lambda: _loss_backward(m, x), 3, 0.05)
