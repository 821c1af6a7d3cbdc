"""Ensemble weighting and resampling on the device: sea_decode_member_sse through Decode.member_sse and FieldLikelihood, sea_resample_systematic through
systematic_resample, and the particle-filter cycle around a rollout session.

References: the fp64 restatements of tests/test_ensemble_cpu.py.  member_sse: let e be the relative L2 error of the [Bm, n_fields] result against
`restate_member_sse` and e_c that of the composed bf16 path (forward() + torch reductions) on the same inputs; the fused launch must keep
e <= 2e-2 (the bf16 decode tolerance) and e <= 2 e_c + 1e-6 (both paths make the same roundings and differ in summation order only);
fp32 (composed): e <= 1e-4.  Shapes: those of tests/test_decode_loss_gpu.py (the smallest at which the tiling can go wrong), the batch read as
members x histories:
  a  M = 18 rows, P = 9: a member boundary inside a 16-row wave tile; hidden 40             members / histories 2 / 1, 1 / 2
  b  M = 132, P = 4: full tiles plus a 4-row tail; n_inp 37                                  11 / 3, 33 / 1, 1 / 33
  c  P = 2, B = 35; hidden 624                                                               5 / 7, 35 / 1
each without counts and with the file's ragged counts (0, 1, C - 1, C).  The observation is the first `histories` entries of the fixture target.

Resampling: index and resampled equal `restate_resample` exactly — tests/test_ensemble_cpu.py asserts for every input used here that each search
threshold stays 1e-9 W away from every cumulative weight, four orders above the error of an fp64 scan — ess and logw_out (fp64 results stored as f32)
to 1e-5 relative, or absolute near 0."""
import functools

import numpy as np
import pytest
import torch

from tests.test_decode_loss_cpu import rel
from tests.test_decode_loss_gpu import DEV, TOL_BF16, TOL_F32, case, counts_sets, decoder, device_target
from tests.test_ensemble_cpu import RESAMPLE_N, extra_resample_cases, resample_inputs, restate_member_sse, restate_resample

pytestmark = pytest.mark.gpu

SPLITS = {"a": ((2, 1), (1, 2)), "b": ((11, 3), (33, 1), (1, 33)), "c": ((5, 7), (35, 1))}   # (members, histories)


@functools.lru_cache(maxsize=None)
def reference(name, members, counts_key):
    c = case(name)
    counts = None if counts_key is None else list(counts_key)
    return restate_member_sse(c["w1"], c["w2"], c["b2"], c["groups"], c["z"], c["target"][:c["B"] // members], counts, members)


def key(counts):
    return None if counts is None else tuple(counts)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fused_member_sse_against_fp64(name):
    c = case(name)
    dec = decoder(name, "bf16")
    z, tgt = c["z"].to(DEV), device_target(name)
    n_fields = tgt.shape[2]
    for members, hist in SPLITS[name]:
        for counts in counts_sets(name):
            ref = reference(name, members, key(counts))
            got = dec.member_sse(z, tgt[:hist], counts=counts, members=members, fused=True)
            comp = dec.member_sse(z, tgt[:hist], counts=counts, members=members, fused=False)
            assert got.shape == (c["B"], n_fields) and got.dtype == torch.float32 and not got.requires_grad and got.grad_fn is None
            assert torch.equal(comp, dec.member_sse(z, tgt[:hist], counts=counts, members=members))     # fused=None: below 8192 rows the composed path (measured rule)
            e, e_c = rel(got.cpu(), ref), rel(comp.cpu(), ref)
            print(f"member_sse shape {name} members {members} x {hist} counts {counts}: fused e {e:.3e}; composed e_c {e_c:.3e}")
            assert e <= TOL_BF16, (members, counts, e)
            assert e <= 2 * e_c + 1e-6, (members, counts, e, e_c)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fp32_composed_member_sse_against_fp64(name):
    c = case(name)
    dec = decoder(name, "fp32")
    z, tgt = c["z"].to(DEV), device_target(name)
    for members, hist in SPLITS[name]:
        for counts in counts_sets(name)[:2]:
            got = dec.member_sse(z, tgt[:hist], counts=counts, members=members)
            e = rel(got.cpu(), reference(name, members, key(counts)))
            print(f"member_sse shape {name} members {members} x {hist} counts {counts}: fp32 e {e:.3e}")
            assert e <= TOL_F32


@pytest.mark.parametrize("name", ["a", "b"])
def test_members_without_valid_cells_score_exactly_zero(name):
    c = case(name)
    dec = decoder(name, "bf16")
    z, tgt = c["z"].to(DEV), device_target(name)
    members, hist = SPLITS[name][0]
    got = dec.member_sse(z, tgt[:hist], counts=[0] * c["P"], members=members, fused=True)
    assert got.shape[0] == c["B"] and float(got.abs().max()) == 0.0
    # one patch valid: every other patch of a member adds exactly nothing
    only = [0] * c["P"]
    only[-1] = c["n_inp"]
    ref = reference(name, members, key(only))
    got = dec.member_sse(z, tgt[:hist], counts=only, members=members, fused=True)
    assert rel(got.cpu(), ref) <= TOL_BF16 and float(got.min()) > 0.0


@pytest.mark.parametrize("name", ["a", "b"])
def test_nan_in_invalid_slots_and_pad_columns_is_neutral(name):
    c = case(name)
    dec = decoder(name, "bf16")
    z = c["z"].to(DEV)
    C, counts = c["n_inp"], c["counts"]
    members, hist = SPLITS[name][0]
    width = C + 4 if C % 4 == 0 else None                     # shape a: four pad columns behind the cell; shape b: 37 -> 40
    clean = device_target(name, 0.0, width)[:hist]
    dirty = device_target(name, float("nan"), width)[:hist].clone()
    base = dec.member_sse(z, clean, counts=None, members=members, fused=True)
    got = dec.member_sse(z, dirty, counts=None, members=members, fused=True)          # the pad columns alone
    assert torch.equal(base, got) and bool(torch.isfinite(got).all())
    for p, n in enumerate(counts):                            # slots at or beyond the patch's count
        dirty[:, p, :, n:] = float("nan")
    base = dec.member_sse(z, clean, counts=counts, members=members, fused=True)
    got = dec.member_sse(z, dirty, counts=counts, members=members, fused=True)
    assert torch.equal(base, got) and bool(torch.isfinite(got).all())


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_member_sse_bits_do_not_depend_on_the_run_or_on_members(name):
    c = case(name)
    dec = decoder(name, "bf16")
    z, tgt = c["z"].to(DEV), device_target(name)
    for members, hist in SPLITS[name]:
        for counts in counts_sets(name)[:2]:
            a = dec.member_sse(z, tgt[:hist], counts=counts, members=members, fused=True)
            b = dec.member_sse(z, tgt[:hist], counts=counts, members=members, fused=True)
            one = dec.member_sse(z, tgt[:hist].repeat_interleave(members, dim=0), counts=counts, members=1, fused=True)
            assert torch.equal(a, b) and torch.equal(a, one), (members, counts)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_both_workgroup_forms_give_the_same_bits(name, monkeypatch):
    """64 rows per workgroup against 128 (SEA_TUNE sse_rows=, the switch tools/ensemble_bench.py measures with; the default depends on the hidden width):
    a row's sum does not depend on the block it sits in."""
    c = case(name)
    dec = decoder(name, "bf16")
    z, tgt = c["z"].to(DEV), device_target(name)
    members, hist = SPLITS[name][0]
    for counts in counts_sets(name)[:2]:
        monkeypatch.setenv("SEA_TUNE", "sse_rows=128")
        a = dec.member_sse(z, tgt[:hist], counts=counts, members=members, fused=True)
        monkeypatch.setenv("SEA_TUNE", "sse_rows=64")
        b = dec.member_sse(z, tgt[:hist], counts=counts, members=members, fused=True)
        assert torch.equal(a, b) and rel(b.cpu(), reference(name, members, key(counts))) <= TOL_BF16


def test_default_path_takes_the_fused_launch_from_8192_rows_on(monkeypatch):
    """fused=None: the composed path below 8192 rows (Bm * P), the fused launch from there on (the measured rule of Decode.member_sse); fp32 never."""
    from sea_amd import ops

    c = case("a")
    P = 64
    g = torch.Generator().manual_seed(31)
    z = torch.randn(128, P, len(c["groups"]), c["D"], generator=g).to(DEV)
    obs = torch.randn(2, P, 3, c["n_inp"], generator=g).to(DEV)
    calls, real = [], ops.decode_member_sse
    monkeypatch.setattr(ops, "decode_member_sse", lambda *a, **k: (calls.append(a[0][0]["H"].shape[0]), real(*a, **k))[1])
    dec = decoder("a", "bf16")
    at = dec.member_sse(z, obs, members=64)                                   # 128 x 64 = 8192 rows
    assert calls == [8192] and torch.equal(at, dec.member_sse(z, obs, members=64, fused=True))
    calls.clear()
    below = dec.member_sse(z[:127], obs[:1], members=127)                     # 8128 rows
    assert calls == [] and torch.equal(below, dec.member_sse(z[:127], obs[:1], members=127, fused=False))
    assert rel(at.cpu(), dec.member_sse(z, obs, members=64, fused=False).cpu()) <= 1e-5      # the same fp32 Y, summed in another order
    decoder("a", "fp32").member_sse(z, obs, members=64)
    assert calls == []


# ------------------------------------------------------------------------------------------------ resampling
def check_resample(logw, u, n, thr, what):
    from sea_amd.ensemble import systematic_resample

    index, out, ess, res = systematic_resample(logw.to(DEV), n, u=u.to(DEV), ess_threshold=thr)
    again = systematic_resample(logw.to(DEV).reshape(-1), n, u=u.to(DEV), ess_threshold=thr)
    G = logw.numel() // n
    assert index.dtype == torch.int32 and index.shape == (G * n,) and index.is_cuda and res.dtype == torch.int32 and res.shape == (G,)
    assert out.dtype == torch.float32 and out.shape == (G * n,) and ess.dtype == torch.float32 and ess.shape == (G,)
    for a, b in zip((index, out, ess, res), again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what                # two runs: the same bits
    r_index, r_out, r_ess, r_res = restate_resample(logw.numpy(), u.numpy(), n, -1.0 if thr is None else thr)
    assert np.array_equal(res.cpu().numpy(), r_res), (what, res.tolist(), r_res.tolist())
    assert np.array_equal(index.cpu().numpy(), r_index), what
    assert np.allclose(ess.cpu().numpy().astype(np.float64), r_ess, rtol=1e-5, atol=1e-5), (what, ess.tolist(), r_ess.tolist())
    got = out.cpu().numpy().astype(np.float64)
    fin = np.isfinite(r_out)
    assert np.array_equal(np.isneginf(got), np.isneginf(r_out)) and np.array_equal(np.isfinite(got), fin), what
    assert np.allclose(got[fin], r_out[fin], rtol=1e-5, atol=1e-5), what
    return index, out, ess, res


@pytest.mark.parametrize("n", RESAMPLE_N)
def test_resample_matches_the_restatement(n):
    logw, u = resample_inputs(n)
    index, out, ess, res = check_resample(logw, u, n, None, n)
    assert res.tolist() == [1, 1, 1] and float(out.abs().max()) == 0.0
    idx = index.view(3, n).cpu() - torch.arange(3).view(3, 1) * n
    assert int(idx.min()) >= 0 and int(idx.max()) < n and bool((idx[:, 1:] >= idx[:, :-1]).all())      # inside its history, non-decreasing


def test_resample_edge_cases_match_the_restatement():
    got = {}
    for name, (logw, u, thr) in extra_resample_cases().items():
        got[name] = check_resample(logw, u, logw.shape[1], thr, name)
    assert got["an all-dead history"][3].tolist() == [1, -1, 1]
    assert got["ess gate"][3].tolist() == [0, 1]
    out = got["ess gate"][1].view(2, -1)
    assert abs(float(out[0].double().exp().sum()) - 1.0) <= 1e-5 and float(out[1].abs().max()) == 0.0   # kept: normalised; resampled: equal weights
    assert got["uniform"][0].tolist() == list(range(100))
    # the prior is added first: a prior that cancels the log-weights gives the uniform case above
    from sea_amd.ensemble import systematic_resample

    logw = (3 * torch.randn(2, 50, generator=torch.Generator().manual_seed(5))).to(DEV)
    index, _, ess, _ = systematic_resample(logw, 50, u=torch.full((2,), 0.5, device=DEV), prior=-logw.reshape(-1))
    assert index.tolist() == list(range(100)) and np.allclose(ess.cpu().numpy(), 50.0, rtol=1e-5)
    index, _, _, res = systematic_resample(logw, 50)                                        # u drawn on the device
    assert res.tolist() == [1, 1] and int((index.view(2, 50).cpu() // 50 != torch.arange(2).view(2, 1)).sum()) == 0


# ------------------------------------------------------------------------------------------------ end to end
def test_particle_filter_cycle_on_a_rollout_session():
    """fork, step, weigh on decoded fields, resample on the device, gather the caches: the weights are those of the fp64 restatement on the returned
    states, the resampled session holds the gathered states bit for bit and steps like before.select(index), and neither new function synchronises."""
    from sea_amd.ensemble import FieldLikelihood, systematic_resample
    from oracle.recipe import recipe_inputs
    from tests.test_input_grad_gpu import cfg_of
    from tests.test_model_gpu import build
    from tests.test_rollout_session_gpu import open_on

    c = case("a")
    P, D, n_mem, B, k = 4, c["D"], 8, 2, 3
    cfg = cfg_of(1, P * D, 4, len(c["groups"]))
    m = build(cfg, "bf16")
    x, _, ib = recipe_inputs(B, k + 4, cfg, seed=9)
    dec = decoder("a", "bf16")
    g = torch.Generator().manual_seed(12)
    obs = torch.randn(B, P, 3, c["n_inp"], generator=g)
    counts, sigma = [12, 0, 7, 11], [0.5, 1.0, 2.0]
    conds = torch.rand(B * n_mem, 1, generator=g).to(DEV)
    conds2 = torch.rand(B * n_mem, 1, generator=g).to(DEV)
    u = torch.rand(B, generator=g).to(DEV)

    ens = open_on(m, x, ib, k).fork(n_mem)
    y = ens.step(conds)                                                                   # [16, 2, 64]
    assert y.shape == (B * n_mem, len(c["groups"]), P * D)
    like = FieldLikelihood(dec, P, n_mem, counts=counts, sigma=sigma, fused=True)         # the fused launch (the default takes it from 8192 rows on)
    obs_d = obs.to(DEV)
    logw = like(y, obs_d)                                                                 # the first call uploads the counts (cached per counts object)
    assert logw.shape == (B * n_mem,) and logw.dtype == torch.float32 and logw.is_cuda
    z = y.cpu().reshape(B * n_mem, len(c["groups"]), P, D).permute(0, 2, 1, 3)
    sse = restate_member_sse(c["w1"], c["w2"], c["b2"], c["groups"], z, obs, counts, n_mem)
    ref = -0.5 * (sse / torch.tensor(sigma, dtype=torch.float64) ** 2).sum(1)
    comp = FieldLikelihood(dec, P, n_mem, counts=counts, sigma=sigma, fused=False)(y, obs_d)
    e, e_c = rel(logw.cpu(), ref), rel(comp.cpu(), ref)
    print(f"particle filter: log-weights fused e {e:.3e}, composed e_c {e_c:.3e}")
    assert e <= TOL_BF16 and e <= 2 * e_c + 1e-6
    assert torch.equal(FieldLikelihood(dec, P, n_mem, counts=counts, sigma=sigma)(y, obs_d), comp)
    ref_layout = FieldLikelihood(dec, P, n_mem, counts=counts, sigma=sigma, layout="BPCF", fused=True)(y, obs_d.permute(0, 1, 3, 2).contiguous())
    assert torch.equal(ref_layout, logw)                                                  # the reference's layout: the same bits

    # neither function waits for the device
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        logw2 = like(y, obs_d)
        index, logw_out, ess, resampled = systematic_resample(logw2, n_mem, u=u)
        systematic_resample(logw2, n_mem, ess_threshold=0.5, prior=logw_out)              # u drawn on the device
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(logw2, logw)
    assert index.dtype == torch.int32 and index.is_cuda and resampled.tolist() == [1, 1]
    idx = index.view(B, n_mem).cpu()
    assert bool((idx // n_mem == torch.arange(B).view(B, 1)).all()) and bool((idx[:, 1:] >= idx[:, :-1]).all())
    assert float(logw_out.abs().max()) == 0.0 and bool((ess >= 1.0).all()) and bool((ess <= n_mem + 1e-3).all())

    before = ens.states()
    twin = ens.select(index)                                                              # a session of its own from the ensemble before the resampling
    ens.resample(index)                                                                   # the device index goes in as it is
    assert torch.equal(ens.states(), before[index.long()])
    assert torch.equal(ens.step(conds2), twin.step(conds2))
    twin.close()
    ens.close()
