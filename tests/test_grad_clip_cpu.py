"""Gradient clipping and non-finite-step skipping without a GPU: the two entry points (sea_grad_norm_ctl, sea_adamw_flat_ctl) are exported and
refuse malformed arguments before touching a device, FlatAdamW and initialize_optimizer validate and forward the two options on a CPU model,
and `sea_amd.optim.step_control` — the plain-Python restatement of the device-side rule, which tests/test_grad_clip_gpu.py uses as its
reference — gives the hand-computed answers."""
import math

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from sea_amd import build, _native

    build.build(verbose=False)
    return _native.lib()


def test_symbols_are_exported_and_listed(lib):
    from sea_amd import _native as N

    for name in ("sea_grad_norm_ctl", "sea_adamw_flat_ctl"):
        assert hasattr(lib, name) and name in N.EXPORTED_SYMBOLS
    assert (N.CTL_GRAD_NORM, N.CTL_CLIP, N.CTL_INV_BC1, N.CTL_INV_SQRT_BC2, N.CTL_APPLIED, N.CTL_STEP, N.CTL_SKIPPED, N.CTL_CLIPPED,
            N.CTL_WORDS) == tuple(range(9))


# made-up, aligned, never dereferenced addresses: every case breaks exactly one thing, so the checks refuse it before a launch
G, PART, CTL = 0x10000, 0x20000, 0x30000


def _norm_args(g=G, n=8, gs=1.0, max_norm=1.0, skip=1, b1=0.9, b2=0.999, partial=PART, cap=1024, ctl=CTL):
    return (g, n, gs, max_norm, skip, b1, b2, partial, cap, ctl, None)


@pytest.mark.parametrize("what,change", [
    ("null g", dict(g=None)), ("null partial", dict(partial=None)), ("null ctl", dict(ctl=None)), ("n = 6", dict(n=6)), ("n = 0", dict(n=0)),
    ("misaligned ctl", dict(ctl=CTL + 4)), ("misaligned g", dict(g=G + 8)), ("misaligned partial", dict(partial=PART + 4)),
    ("n_partial_cap = 0", dict(cap=0)), ("beta1 = 1", dict(b1=1.0)), ("beta2 < 0", dict(b2=-0.1)), ("NaN max_norm", dict(max_norm=float("nan")))])
def test_grad_norm_ctl_refuses_bad_arguments_without_a_device(lib, what, change):
    assert lib.sea_grad_norm_ctl(*_norm_args(**change)) != 0, what
    assert b"sea_grad_norm_ctl" in lib.sea_last_error()


def _adamw_args(p=0x40000, g=G, m=0x50000, v=0x60000, shadow=None, sd=0, n=8, ctl=CTL):
    return (p, g, m, v, shadow, sd, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, ctl, None)


@pytest.mark.parametrize("what,change", [
    ("null p", dict(p=None)), ("null g", dict(g=None)), ("null m", dict(m=None)), ("null v", dict(v=None)), ("null ctl", dict(ctl=None)),
    ("n = 6", dict(n=6)), ("misaligned ctl", dict(ctl=CTL + 8)), ("misaligned p", dict(p=0x40004)), ("misaligned shadow", dict(shadow=0x70002, sd=1)),
    ("bad shadow dtype", dict(shadow=0x70000, sd=7))])
def test_adamw_flat_ctl_refuses_bad_arguments_without_a_device(lib, what, change):
    assert lib.sea_adamw_flat_ctl(*_adamw_args(**change)) != 0, what
    assert b"sea_adamw_flat_ctl" in lib.sea_last_error()


# ------------------------------------------------------------------------------------------------ the optimizer on the host
def _cpu_model():
    from sea_amd.models.temporal import TemporalModel

    return TemporalModel(1, 32, 2, 8, 2, 0, 2, 2, 0.0, "sea", "learnable", "mlp", "add", 1, 1, True, "adaln")


@pytest.mark.parametrize("x", [0, -1, float("inf"), float("nan"), 0.0, True, "1.0"])
def test_constructor_refuses_a_bad_max_grad_norm(x):
    from sea_amd.optim import FlatAdamW

    with pytest.raises(ValueError, match="max_grad_norm"):
        FlatAdamW(_cpu_model(), max_grad_norm=x)


def test_options_default_off_and_initialize_optimizer_forwards_them():
    from sea_amd.optim import FlatAdamW
    from sea_amd.utils.train_utils import initialize_optimizer

    m = _cpu_model()
    for opt in (FlatAdamW(m), initialize_optimizer(m, dict(learning_rate=1e-3))):
        assert opt.max_grad_norm is None and opt.skip_nonfinite is False and not opt.controlled
        assert opt.last_grad_norm is None and opt.last_applied is None
        with pytest.raises(RuntimeError, match="max_grad_norm"):
            opt.step_stats()
        assert "ctl" not in opt.state_dict()["sea_flat"]
    opt = initialize_optimizer(m, dict(learning_rate=1e-3, max_grad_norm=0.5, skip_nonfinite_steps=True))
    assert opt.max_grad_norm == 0.5 and opt.skip_nonfinite is True and opt.controlled
    opt, sched = initialize_optimizer(m, dict(learning_rate=1e-3, max_grad_norm=2, scheduler="linear", epoch_num=3))
    assert opt.max_grad_norm == 2.0 and opt.skip_nonfinite is False and opt.controlled and sched is not None
    assert initialize_optimizer(m, dict(learning_rate=1e-3, skip_nonfinite_steps=True)).controlled
    assert "ctl" not in opt.state_dict()["sea_flat"]   # no device was touched: there is no control block yet


# ------------------------------------------------------------------------------------------------ the rule, by hand
def _f32(x):
    return float(torch.tensor(x, dtype=torch.float64).float())


def test_step_control_by_hand():
    from sea_amd.optim import step_control

    # a norm exactly at max_norm: clip_grad_norm_'s 1e-6 in the denominator makes the factor 1 / (1 + 1e-6) < 1 — it counts as clipped
    r = step_control(1.0, 1.0, True, step=3, skipped=1, clipped=2)
    assert r == dict(grad_norm=1.0, clip=_f32(1.0 / 1.000001), applied=1, step=4, skipped=1, clipped=3)
    assert r["clip"] < 1.0 and abs(r["clip"] - 0.999999) < 1e-7
    # ... unless fp32 cannot tell the factor from 1: 1000 / (1000 + 1e-6) = 1 - 1e-9 is stored as 1.0f, and a factor of 1 is not a clip
    assert step_control(1000.0, 1000.0, False, step=0) == dict(grad_norm=1000.0, clip=1.0, applied=1, step=1, skipped=0, clipped=0)
    # just above
    r = step_control(1.25, 1.0, False, step=0)
    assert r == dict(grad_norm=1.25, clip=_f32(1.0 / 1.250001), applied=1, step=1, skipped=0, clipped=1)
    assert abs(r["clip"] - 0.8) < 1e-6
    # below: no clip; max_norm <= 0: no clipping at all
    assert step_control(0.5, 1.0, True, step=7, clipped=4) == dict(grad_norm=0.5, clip=1.0, applied=1, step=8, skipped=0, clipped=4)
    assert step_control(50.0, 0.0, True, step=7) == dict(grad_norm=50.0, clip=1.0, applied=1, step=8, skipped=0, clipped=0)
    # non-finite with skipping on: nothing advances but the skip count
    for bad in (float("inf"), float("nan")):
        r = step_control(bad, 1.0, True, step=3, skipped=1, clipped=2)
        assert (r["clip"], r["applied"], r["step"], r["skipped"], r["clipped"]) == (0.0, 0, 3, 2, 2)
        assert not math.isfinite(r["grad_norm"])
        # ... and off: applied unclipped, which is what the plain AdamW launch does
        r = step_control(bad, 1.0, False, step=3, skipped=1, clipped=2)
        assert (r["clip"], r["applied"], r["step"], r["skipped"], r["clipped"]) == (1.0, 1, 4, 1, 2)
    # finite in fp64, infinite once rounded to the fp32 word the device stores: judged on the fp32 value
    r = step_control(1e39, 1.0, True, step=3)
    assert r["grad_norm"] == float("inf") and r["applied"] == 0 and r["skipped"] == 1
