"""Rollouts from a multi-step context (sea_amd/utils/train_utils.py rollout, engine.rollout_kv, kv_engine.KvFast): the known states at positions
0 .. k-1 are prefilled by one full-context forward, sea_kv_cache_fill (sea_amd/csrc/kvstep.hip) moves their keys / values into the decode caches and
the exact KV decode continues from position k.  Every decode form is held against the device recompute loop from the same context and against the
oracle's restatement of the reference's loop; the reference itself pins two cases (tests/golden/context_rollout_*.npz).

Tolerances: fp32 1e-5 between device paths and 1e-4 to the oracle; bf16 2e-2 between paths and 3e-2 to the oracle (the existing KV tests' bars)."""
import warnings

import pytest
import torch

from oracle import sea_oracle as O
from oracle.recipe import recipe_inputs, recipe_params
from tests.conftest import cfg_from_meta, load_golden, rel_l2
from tests.test_model_gpu import build

pytestmark = pytest.mark.gpu

KS = (2, 9, 37)
N_STEPS = 5


def oracle_rollout(x, ib, k, n, cfg):
    """The reference's loop started from x[:, :k] (fp64 oracle)."""
    p = {key: v.double() for key, v in recipe_params(cfg).items()}
    a = x[:, :k].double()
    with torch.no_grad():
        for i in range(n):
            out = O.model_forward(a, ib[:, :k + i].double(), p, cfg)
            a = torch.cat((a, out[:, -1:]), dim=1)
    return a[:, k:].float()


def roll(m, x, ib, k, n, mode, monkeypatch=None, kv=None):
    from sea_amd.utils.train_utils import rollout

    if monkeypatch is not None:
        monkeypatch.setenv("SEA_KV", kv or "")
    return rollout(m, x[:, :k].cuda().contiguous(), ib.cuda().contiguous(), n, mode=mode)


def check_context_cases(cfg, B, dtype, monkeypatch, kv="", ks=KS, n=N_STEPS, fast=None):
    from sea_amd import kv_engine

    m = build(cfg, dtype)
    if fast is not None:
        monkeypatch.setenv("SEA_KV", kv)
        assert kv_engine.supported(m.engine(), B) == fast
    x, _, ib = recipe_inputs(B, max(ks) + n, cfg, seed=9)
    tol_path, tol_ref = (1e-5, 1e-4) if dtype == "fp32" else (2e-2, 3e-2)
    for k in ks:
        a = roll(m, x, ib, k, n, "kv", monkeypatch, kv).cpu().numpy()
        r = roll(m, x, ib, k, n, "recompute", monkeypatch, kv).cpu().numpy()
        ref = oracle_rollout(x, ib, k, n, cfg).numpy()
        assert a.shape == (B, n, cfg.num_variables, cfg.embed_dim)
        assert rel_l2(a, r) < tol_path, (k, rel_l2(a, r))
        assert rel_l2(a, ref) < tol_ref, (k, rel_l2(a, ref))
    return m


# ------------------------------------------------------------------------------------------------ the reference's own loop
@pytest.mark.parametrize("name", ["context_rollout_adaln_f3", "context_rollout_ln_f2"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_context_rollout_matches_reference_fixture(name, dtype, monkeypatch):
    g = load_golden(name)
    cfg = cfg_from_meta(g["cfg"])
    m = build(cfg, dtype)
    x, ib, n = torch.from_numpy(g["x"]), torch.from_numpy(g["ib"]), int(g["steps"])
    tol = 1e-4 if dtype == "fp32" else 3e-2
    for k in [int(v) for v in g["ks"]]:
        for mode in ("kv", "recompute"):
            out = roll(m, x, ib, k, n, mode, monkeypatch, "").cpu().numpy()
            assert rel_l2(out, g[f"pred_k{k}"]) < tol, (k, mode)


# ------------------------------------------------------------------------------------------------ every decode form against recompute and the oracle
FAST_CASES = [
    ((2, 64, 4, 64, 8, 0, 3, 2, True, "adaln", "sea", "add", "mlp"), 2),        # two layers, F = 3
    ((2, 64, 8, 64, 4, 0, 1, 1, True, "adaln", "sea", "add", "linear"), 5),     # one field, head dim 8
    ((2, 128, 8, 64, 4, 0, 2, 2, False, "ln", "sea", "none", "mlp"), 5),        # F = 2, no info-bottleneck, ib before the block
    ((2, 128, 4, 64, 8, 0, 4, 2, True, "adaln", "sea", "add", "fourier"), 2),   # four fields, Fourier info-bottleneck
]


@pytest.mark.parametrize("cfg_args,B", FAST_CASES)
def test_seven_launch_decode_from_context_fp32(cfg_args, B, monkeypatch):
    check_context_cases(O.OracleConfig(*cfg_args), B, "fp32", monkeypatch, "fast=1", fast=True)


def test_persistent_decode_from_context(monkeypatch):
    """B = 1, one layer, cfg2's widths: the one-launch persistent form decodes from position k."""
    cfg = O.OracleConfig(1, 256, 8, 64, 8, 0, 3, 2, True, "adaln")
    for dtype in ("fp32", "bf16"):
        check_context_cases(cfg, 1, dtype, monkeypatch, "fast=1", fast=True)


GENERIC_CASES = [
    ((1, 64, 4, 64, 8, 0, 3, 2, True, "adaln"), 2, "fast=0"),                                  # the generic step plan instead of sea_kv_rollout
    ((1, 96, 2, 64, 8, 0, 3, 2, True, "adaln"), 2, ""),                                        # head dim 48: outside sea_kv_rollout's limits
    ((1, 64, 4, 64, 8, 0, 3, 2, True, "adaln", "addition"), 2, ""),                            # 'addition' exchange
    ((1, 64, 4, 64, 8, 0, 2, 2, False, "ln", "sea", "concat"), 2, ""),                         # 'concat' info-bottleneck (in front of the block)
]


@pytest.mark.parametrize("cfg_args,B,kv", GENERIC_CASES)
def test_generic_step_plan_decode_from_context_fp32(cfg_args, B, kv, monkeypatch):
    check_context_cases(O.OracleConfig(*cfg_args), B, "fp32", monkeypatch, kv, fast=False)


def test_fewrow_decode_from_context_bf16(monkeypatch):
    """E = 1024 (the shipped cylinder width): the few-row launches of the step plan."""
    from sea_amd import kv_engine

    cfg = O.OracleConfig(1, 1024, 8, 48, 8, 0, 2, 2, True, "adaln")
    m = check_context_cases(cfg, 1, "bf16", monkeypatch, "", ks=(2, 9), n=3, fast=False)
    p = next(p for key, p in m.engine()._plans.items() if key[:3] == (1, 1, "step"))
    assert p.forms.few
    assert not kv_engine.supported(m.engine(), 1)


# ------------------------------------------------------------------------------------------------ resume = one long rollout
@pytest.mark.parametrize("form", ["persistent", "fast", "generic"])
def test_resumed_rollout_equals_one_long_rollout(form, monkeypatch):
    cfg = O.OracleConfig(1, 256, 8, 64, 8, 0, 3, 2, True, "adaln") if form == "persistent" else O.OracleConfig(2, 64, 4, 64, 8, 0, 3, 2, True, "adaln")
    B = 1 if form == "persistent" else 2
    kv = "fast=0" if form == "generic" else "fast=1"
    for dtype, tol in (("fp32", 1e-5), ("bf16", 2e-2)):
        m = build(cfg, dtype)
        x, _, ib = recipe_inputs(B, 24, cfg, seed=13)
        x0, ibg = x[:, :3].cuda().contiguous(), ib.cuda().contiguous()
        n1, n2 = 7, 6
        whole = roll(m, x0.cpu(), ib, 3, n1 + n2, "kv", monkeypatch, kv)
        first = roll(m, x0.cpu(), ib, 3, n1, "kv", monkeypatch, kv)
        ctx = torch.cat((x0, first), dim=1)
        second = roll(m, ctx.cpu(), ib, 3 + n1, n2, "kv", monkeypatch, kv)
        assert torch.equal(first, whole[:, :n1]) or rel_l2(first.cpu().numpy(), whole[:, :n1].cpu().numpy()) < tol
        assert rel_l2(second.cpu().numpy(), whole[:, n1:].cpu().numpy()) < tol, (dtype, form)


# ------------------------------------------------------------------------------------------------ boundaries
@pytest.mark.parametrize("kv", ["fast=1", "fast=0"])
def test_context_boundaries(kv, monkeypatch):
    from sea_amd.utils.train_utils import rollout

    monkeypatch.setenv("SEA_KV", kv)
    cfg = O.OracleConfig(1, 64, 4, 24, 8, 0, 3, 2, True, "adaln")
    m = build(cfg, "fp32")
    x, _, ib = recipe_inputs(2, 24, cfg, seed=17)
    xg, ibg = x.cuda(), ib.cuda()
    # k + n - 1 = max_len: the last position of the caches
    a = rollout(m, xg[:, :10].contiguous(), ibg, 15, mode="kv")
    b = rollout(m, xg[:, :10].contiguous(), ibg, 15, mode="recompute")
    assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) < 1e-5
    # k = max_len, one step: the full forward's last row
    one = rollout(m, xg.contiguous(), ibg, 1, mode="kv")
    with torch.no_grad():
        full = m(xg.contiguous(), ibg)
    assert torch.equal(one[:, 0], full[:, -1])
    # refused before any launch: a fresh model's engine has built no plan, no condition pass and no decode workspace
    m2 = build(cfg, "fp32")
    eng = m2.engine()
    for args, what in (((xg[:, :10].contiguous(), ibg, 16), "max_len"), ((xg[:, :10].contiguous(), ibg[:, :12], 5), "too short"),
                       ((xg[:, :0].contiguous(), ibg, 3), "k >= 1")):
        for mode in ("kv", "recompute"):
            with pytest.raises(ValueError, match=what):
                rollout(m2, *args, mode=mode)
    assert not eng._plans and not eng._kv_fast and not eng.__dict__.get("_cond_plans")


def test_k1_is_the_single_state_path_bitwise(monkeypatch):
    """k = 1: no prefill, no fill launch; the same trajectory as before."""
    from sea_amd import kv_engine
    from sea_amd.utils.train_utils import rollout

    cfg = O.OracleConfig(1, 64, 4, 32, 8, 0, 3, 2, True, "adaln")
    runs = []
    orig = kv_engine.CacheFill.run
    monkeypatch.setattr(kv_engine.CacheFill, "run", lambda self: runs.append(1) or orig(self))
    for kv in ("fast=1", "fast=0"):
        monkeypatch.setenv("SEA_KV", kv)
        m = build(cfg, "bf16")
        x, _, ib = recipe_inputs(2, 16, cfg, seed=19)
        runs.clear()
        a = rollout(m, x[:, :1].cuda().contiguous(), ib.cuda(), 12, mode="kv")
        assert not runs and not any(key[:2] == (2, 1) and key[2] == "full" for key in m.engine()._plans)
        r = rollout(m, x[:, :1].cuda().contiguous(), ib.cuda(), 12, mode="recompute")
        assert rel_l2(a.cpu().numpy(), r.cpu().numpy()) < 2e-2
        b = rollout(m, x[:, :1].cuda().contiguous(), ib.cuda(), 12, mode="kv")
        assert torch.equal(a, b)
        rollout(m, x[:, :4].cuda().contiguous(), ib.cuda(), 5, mode="kv")
        assert runs


# ------------------------------------------------------------------------------------------------ sea_kv_cache_fill itself
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hd", [8, 16, 48, 64, 96, 256])
def test_cache_fill_op_matches_torch_copy(dtype, hd):
    from sea_amd import ops

    g = torch.Generator(device="cuda").manual_seed(hd)
    B, H = 2, 3
    entries, checks = [], []
    for n_pos, cap_src, cap_dst, v_rows in ((37, 40, 64, True), (37, 40, 64, False), (70, 72, 136, True), (5, 8, 16, False), (64, 64, 64, True)):
        K = torch.randn(B, H, cap_src, hd, device="cuda", generator=g).to(dtype)
        Vt = torch.randn(B, H, hd, cap_src, device="cuda", generator=g).to(dtype)
        Kd = torch.full((B, H, cap_dst, hd), 7.0, device="cuda", dtype=dtype)
        Vd = torch.full((B, H, cap_dst, hd) if v_rows else (B, H, hd, cap_dst), 7.0, device="cuda", dtype=dtype)
        entries.append(dict(K=K, Vt=Vt, Kd=Kd, Vd=Vd, n_pos=n_pos, v_rows=v_rows))
        checks.append((K, Vt, Kd, Vd, n_pos, v_rows))
    ops.kv_cache_fill(entries, dtype)
    torch.cuda.synchronize()
    for K, Vt, Kd, Vd, n_pos, v_rows in checks:
        assert torch.equal(Kd[:, :, :n_pos], K[:, :, :n_pos])
        assert bool((Kd[:, :, n_pos:] == 7.0).all())
        if v_rows:
            assert torch.equal(Vd[:, :, :n_pos], Vt[..., :n_pos].transpose(2, 3))
            assert bool((Vd[:, :, n_pos:] == 7.0).all())
        else:
            assert torch.equal(Vd[..., :n_pos], Vt[..., :n_pos])
            assert bool((Vd[..., n_pos:] == 7.0).all())


def test_cache_fill_refuses_bad_arguments():
    from sea_amd import _native as N

    L = N.lib()
    t = torch.zeros(1, 1, 16, 16, device="cuda")
    arr = (N.SeaKvFill * 1)()
    e = arr[0]
    e.K = e.Vt = e.Kd = e.Vd = t.data_ptr()
    e.B, e.H, e.hd, e.n_pos, e.cap_src, e.cap_dst, e.v_rows = 1, 1, 16, 8, 16, 16, 1
    for field, bad in (("hd", 12), ("hd", 264), ("n_pos", 17), ("n_pos", 0), ("cap_src", 12), ("v_rows", 2), ("B", 0)):
        old = getattr(e, field)
        setattr(e, field, bad)
        assert L.sea_kv_cache_fill(arr, 1, N.SEA_F32, N.stream_ptr()) == -1, field
        assert b"sea_kv_cache_fill" in L.sea_last_error()
        setattr(e, field, old)
    e.Kd = t.data_ptr() + 4
    assert L.sea_kv_cache_fill(arr, 1, N.SEA_F32, N.stream_ptr()) == -1 and b"misaligned" in L.sea_last_error()
    e.Kd = t.data_ptr()
    assert L.sea_kv_cache_fill(arr, 0, N.SEA_F32, N.stream_ptr()) == -1
    assert L.sea_kv_cache_fill(arr, 1, 7, N.stream_ptr()) == -1
    assert L.sea_kv_cache_fill(arr, 1, N.SEA_F32, N.stream_ptr()) == 0
    torch.cuda.synchronize()


def test_fill_destination_out_of_range_is_refused_by_the_audit(monkeypatch):
    from sea_amd import kv_engine
    from sea_amd.utils.train_utils import rollout

    monkeypatch.setenv("SEA_KV", "fast=0")
    cfg = O.OracleConfig(1, 64, 4, 32, 8, 0, 3, 2, True, "adaln")
    m = build(cfg, "fp32")
    x, _, ib = recipe_inputs(1, 16, cfg, seed=23)
    rollout(m, x[:, :6].cuda().contiguous(), ib.cuda(), 4, mode="kv")
    p = next(p for key, p in m.engine()._plans.items() if key[:3] == (1, 1, "step"))
    cf = next(iter(p._fills.values()))
    assert isinstance(cf, kv_engine.CacheFill) and cf.audit() > 0
    e = cf.arr[0]
    good = e.Kd
    e.Kd = good + (1 << 44)
    with pytest.raises(RuntimeError, match=r"pointer audit .*kv\.cache_fill.*SeaKvFill\.Kd"):
        cf.audit()
    e.Kd = good
    e.cap_dst = 10 ** 6                                    # the destination would run past its cache
    with pytest.raises(RuntimeError, match=r"past the end of its buffer"):
        cf.audit()
    e.cap_dst = p.kv["Ks"][0][0].shape[2]
    assert cf.audit() > 0


# ------------------------------------------------------------------------------------------------ models without an exact cache
@pytest.mark.parametrize("cfg_args", [
    (1, 64, 4, 40, 8, 2, 3, 2, True, "adaln"),                                   # src_len = 2
    (1, 64, 4, 40, 8, 0, 3, 2, True, "adaln", "pool"),                           # 'pool' exchange
    (1, 64, 4, 40, 8, 0, 2, 2, True, "adaln", "sea", "attention"),               # info-bottleneck attention
])
def test_non_exact_models_warn_and_recompute_from_context(cfg_args):
    from sea_amd.utils import train_utils

    cfg = O.OracleConfig(*cfg_args)
    m = build(cfg, "fp32")
    x, _, ib = recipe_inputs(2, 16, cfg, seed=29)
    train_utils._KV_FALLBACK_WARNED.clear()
    with pytest.warns(RuntimeWarning, match="not exact"):
        a = roll(m, x, ib, 4, 5, "kv")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        b = roll(m, x, ib, 4, 5, "kv")                   # the warning is given once
    r = roll(m, x, ib, 4, 5, "recompute")
    assert torch.equal(a, r) and torch.equal(b, r)
    ref = oracle_rollout(x, ib, 4, 5, cfg).numpy()
    assert rel_l2(a.cpu().numpy(), ref) < 1e-4
