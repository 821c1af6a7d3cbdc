"""The forecast of an ensemble on the device: sea_decode_member_moments through Decode.member_moments and EnsembleFields, and unpatch_spread.

Reference: the fp64 restatement of tests/test_ensemble_moments_cpu.py (`restate_member_moments`), on the same float32 weights the device gets.  Let e
be the relative L2 error of a result against it and e_c that of the composed bf16 path (forward() + torch reductions) on the same inputs.  The fused
launch must keep, for the mean, e <= 2e-2 (the bf16 decode tolerance) and e <= 2 e_c + 1e-6; for the variance e <= 2 e_c + 1e-6
(both paths make the same roundings and differ in summation order only; no fixed tolerance for a variance can be stated in advance); fp32 (composed):
e <= 1e-4 for both.  Shapes: those of tests/test_decode_loss_gpu.py with the (members, histories) splits of tests/test_ensemble_gpu.py
  a  2 / 1, 1 / 2      fewer members than one 16-member block; a single member gives variance exactly 0
  b  11 / 3, 33 / 1, 1 / 33      a partial block; two full blocks plus one member
  c  5 / 7, 35 / 1      the widest hidden width, 624
and two synthetic ensembles on shape a's decoder, P = 3, one history of 130 and of 257 members (390 and 771 rows): beyond the 128 members one
workgroup finishes, so two and three chunks go through the workspace and the finish launch.  Each runs without counts and with ragged counts
(0, 1, C - 1, C), with equal weights and with seeded random log-weights that hold -inf and NaN members and, where there are several histories, one
history without a live member."""
import functools

import numpy as np
import pytest
import torch

from tests.test_decode_loss_cpu import rel
from tests.test_decode_loss_gpu import DEV, TOL_BF16, TOL_F32, case, counts_sets, decoder
from tests.test_ensemble_gpu import SPLITS
from tests.test_ensemble_moments_cpu import restate_member_moments, restate_weights

pytestmark = pytest.mark.gpu

SYN = {"s130": 130, "s257": 257}
SYN_P = 3
IDS = ["a", "b", "c", "s130", "s257"]


def base(cid):
    return "a" if cid in SYN else cid


@functools.lru_cache(maxsize=None)
def latents(cid):
    """z [Bm, P, G, D] on the host, computed once and never modified."""
    if cid in SYN:
        c = case("a")
        return torch.randn(SYN[cid], SYN_P, len(c["groups"]), c["D"], generator=torch.Generator().manual_seed(40 + SYN[cid]))
    return case(cid)["z"]


def splits(cid):
    return ((SYN[cid], 1),) if cid in SYN else SPLITS[cid]


def count_sets(cid):
    if cid in SYN:
        C = case("a")["n_inp"]
        return [None, [0, C - 1, C], [1, C, 0]]
    return counts_sets(cid)


@functools.lru_cache(maxsize=None)
def host_weights(cid, members, hist, mode):
    """None (equal weights) or the float32 weights [hist * members] of seeded random log-weights with dead members, through the fp64 restatement."""
    if mode == "uniform":
        return None
    lw = 2 * torch.randn(hist, members, generator=torch.Generator().manual_seed(100 * members + hist))
    if members >= 2:
        lw[0, 0] = float("-inf")
    if members >= 3:
        lw[0, members - 1] = float("nan")
    if members >= 5:
        lw[0, members // 2] = float("-inf")
    if members >= 130:
        lw[0, 16:32] = float("nan")       # a whole 16-member block without a live member
        lw[0, 128:] = float("-inf")       # and a whole chunk
        lw[0, 129] = 0.5
    if hist >= 2:
        lw[hist - 1] = float("nan")       # no live member: equal weights
    w = torch.from_numpy(restate_weights(lw.reshape(-1).numpy(), members)).to(torch.float32)
    if hist >= 2:
        assert torch.equal(w.view(hist, members)[hist - 1], torch.full((members,), 1.0 / members))
    return w


def key(counts):
    return None if counts is None else tuple(counts)


@functools.lru_cache(maxsize=None)
def reference(cid, members, hist, counts_key, mode, unbiased=False):
    c = case(base(cid))
    counts = None if counts_key is None else list(counts_key)
    mean, var, _ = restate_member_moments(c["w1"], c["w2"], c["b2"], c["groups"], latents(cid), members, host_weights(cid, members, hist, mode), counts, unbiased)
    return mean, var


def dev_w(cid, members, hist, mode):
    w = host_weights(cid, members, hist, mode)
    return None if w is None else w.to(DEV)


def full_width(t, Cp):
    """The Cp-wide buffer a [B, P, F, n_inp] result is a view of."""
    return torch.as_strided(t, tuple(t.shape[:3]) + (Cp,), t.stride(), t.storage_offset())


@pytest.mark.parametrize("cid", IDS)
def test_fused_moments_against_fp64(cid):
    c = case(base(cid))
    dec = decoder(base(cid), "bf16")
    z = latents(cid).to(DEV)
    n_fields, C = sum(len(g) for g in c["groups"]), c["n_inp"]
    for members, hist in splits(cid):
        for counts in count_sets(cid):
            for mode, unbiased in (("uniform", False), ("random", False), ("random", True)):
                if unbiased and counts is not None:
                    continue
                w = dev_w(cid, members, hist, mode)
                r_mean, r_var = reference(cid, members, hist, key(counts), mode, unbiased)
                mean, var = dec.member_moments(z, members, weights=w, counts=counts, unbiased=unbiased, fused=True)
                c_mean, c_var = dec.member_moments(z, members, weights=w, counts=counts, unbiased=unbiased, fused=False)
                for t in (mean, var, c_mean, c_var):
                    assert t.shape == (hist, z.shape[1], n_fields, C) and t.dtype == torch.float32 and not t.requires_grad and t.grad_fn is None
                e_m, ec_m, e_v, ec_v = rel(mean.cpu(), r_mean), rel(c_mean.cpu(), r_mean), rel(var.cpu(), r_var), rel(c_var.cpu(), r_var)
                print(f"member_moments {cid} members {members} x {hist} counts {counts} weights {mode}{' unbiased' if unbiased else ''}: "
                      f"mean fused e {e_m:.3e} composed e_c {ec_m:.3e}; var fused e {e_v:.3e} composed e_c {ec_v:.3e}")
                assert e_m <= TOL_BF16, (members, counts, mode, e_m)
                assert e_m <= 2 * ec_m + 1e-6, (members, counts, mode, e_m, ec_m)
                assert e_v <= 2 * ec_v + 1e-6, (members, counts, mode, e_v, ec_v)
                assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(var).all()) and float(var.min()) >= 0.0
                if members == 1:
                    assert float(var.abs().max()) == 0.0


@pytest.mark.parametrize("cid", ["a", "b", "c", "s130"])
def test_fp32_composed_moments_against_fp64(cid):
    dec = decoder(base(cid), "fp32")
    z = latents(cid).to(DEV)
    for members, hist in splits(cid):
        for counts in count_sets(cid)[:2]:
            for mode in ("uniform", "random"):
                mean, var = dec.member_moments(z, members, weights=dev_w(cid, members, hist, mode), counts=counts)
                r_mean, r_var = reference(cid, members, hist, key(counts), mode)
                e_m, e_v = rel(mean.cpu(), r_mean), rel(var.cpu(), r_var)
                print(f"member_moments {cid} members {members} x {hist} counts {counts} weights {mode}: fp32 mean e {e_m:.3e} var e {e_v:.3e}")
                assert e_m <= TOL_F32 and e_v <= TOL_F32


@pytest.mark.parametrize("copies", [2, 33, 130])
def test_variance_is_centred(copies):
    """A history of identical members: var <= 1e-10 mean^2 + 1e-30 elementwise.  A centred fp32 sum leaves a few (2^-24 y)^2 ~ 4e-15 y^2; the
    uncentred E[y^2] - E[y]^2 leaves about 2^-24 y^2 ~ 6e-8 y^2: the bound sits between the two."""
    c = case("a")
    dec = decoder("a", "bf16")
    row = 3.0 * torch.randn(1, 5, len(c["groups"]), c["D"], generator=torch.Generator().manual_seed(77))      # large fields: a large y^2
    z = row.expand(copies, -1, -1, -1).contiguous().to(DEV)
    lw = 2 * torch.randn(copies, generator=torch.Generator().manual_seed(copies))
    for w in (None, torch.from_numpy(restate_weights(lw.numpy(), copies)).float().to(DEV)):
        for unbiased in (False, True):
            mean, var = dec.member_moments(z, copies, weights=w, unbiased=unbiased, fused=True)
            one, _ = dec.member_moments(z[:1], 1, fused=True)
            assert float(mean.abs().max()) > 0.1
            assert bool((var <= 1e-10 * mean * mean + 1e-30).all()), (copies, float(var.max()))
            assert rel(mean.cpu(), one.cpu()) <= 1e-6


@pytest.mark.parametrize("cid,split", [("a", 0), ("b", 0), ("b", 1), ("c", 0), ("s130", 0), ("s257", 0)])
def test_dead_members_are_skipped(cid, split):
    """NaN in the latents of every zero-weight member changes no bit; all the weight on one member returns that member's decoded row, variance 0."""
    dec = decoder(base(cid), "bf16")
    zh = latents(cid)
    members, hist = splits(cid)[split]
    w = host_weights(cid, members, hist, "random")
    dead = w == 0
    assert bool(dead.any()) and bool((~dead).any())
    dirty = zh.clone()
    dirty[dead] = float("nan")
    for counts in count_sets(cid)[:2]:
        clean = dec.member_moments(zh.to(DEV), members, weights=w.to(DEV), counts=counts, fused=True)
        got = dec.member_moments(dirty.to(DEV), members, weights=w.to(DEV), counts=counts, fused=True)
        for a, b in zip(clean, got):
            assert torch.equal(a, b) and bool(torch.isfinite(b).all())
    for j in sorted({0, members // 2, members - 1}):
        one_hot = torch.zeros(hist, members)
        one_hot[:, j] = 1.0
        dirty = zh.clone().view(hist, members, *zh.shape[1:])
        keep = dirty[:, j].clone()
        dirty[:] = float("nan")
        dirty[:, j] = keep
        mean, var = dec.member_moments(dirty.reshape(zh.shape).to(DEV), members, weights=one_hot.reshape(-1).to(DEV), fused=True)
        alone, var1 = dec.member_moments(keep.contiguous().to(DEV), 1, fused=True)
        assert torch.equal(mean, alone), (cid, members, j)
        assert float(var.abs().max()) == 0.0 and float(var1.abs().max()) == 0.0
        _, var_u = dec.member_moments(dirty.reshape(zh.shape).to(DEV), members, weights=one_hot.reshape(-1).to(DEV), unbiased=True, fused=True)
        assert float(var_u.abs().max()) == 0.0                           # 1 / (1 - 1) is not Inf: a degenerate history has variance 0


@pytest.mark.parametrize("cid", ["a", "b", "s130"])
def test_invalid_slots_and_pad_columns_are_exactly_zero(cid):
    c = case(base(cid))
    dec = decoder(base(cid), "bf16")
    z = latents(cid).to(DEV)
    C, Cp = c["n_inp"], dec._n_inp_p
    assert Cp > C
    members, hist = splits(cid)[0]
    P = z.shape[1]
    for fused in (True, False):
        for counts in count_sets(cid):
            mean, var = dec.member_moments(z, members, weights=dev_w(cid, members, hist, "random"), counts=counts, fused=fused)
            for t in (mean, var):
                wide = full_width(t, Cp)
                assert float(wide[..., C:].abs().max()) == 0.0, (fused, counts)
                for p, n in enumerate(counts or []):
                    if n < C:
                        assert float(wide[:, p, :, n:].abs().max()) == 0.0, (fused, counts, p)
                    if n:
                        assert float(mean[:, p, :, :n].abs().min()) > 0.0
        mean, var = dec.member_moments(z, members, counts=[0] * P, fused=fused)
        assert float(full_width(mean, Cp).abs().max()) == 0.0 and float(full_width(var, Cp).abs().max()) == 0.0


@pytest.mark.parametrize("cid", IDS)
def test_moment_bits_do_not_depend_on_the_run_or_on_the_other_histories(cid):
    dec = decoder(base(cid), "bf16")
    z = latents(cid).to(DEV)
    for members, hist in splits(cid):
        for counts in count_sets(cid)[:2]:
            for mode in ("uniform", "random"):
                w = dev_w(cid, members, hist, mode)
                a = dec.member_moments(z, members, weights=w, counts=counts, unbiased=True, fused=True)
                b = dec.member_moments(z, members, weights=w, counts=counts, unbiased=True, fused=True)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (members, counts, mode)
                if hist > 1:       # history 0 alone: the same bits (11 / 3: history 0 of the call equals the 11 / 1 call on its rows)
                    one = dec.member_moments(z[:members], members, weights=None if w is None else w[:members].contiguous(), counts=counts, unbiased=True, fused=True)
                    assert torch.equal(a[0][:1], one[0]) and torch.equal(a[1][:1], one[1]), (members, counts, mode)


def test_fused_path_never_allocates_a_member_sized_buffer():
    """A condition, not a measurement, at 64 members x 64 patches on shape a's decoder: the fused call may raise the peak of allocated memory by less
    than the hidden rows plus the two outputs plus 1 MB, and stays below two thirds of ONE [Bm, P, F, Cp] fp32 tensor of decoded member fields (its
    own buffers — bf16 latents 0.26 MB, hidden rows 0.66 MB, outputs 0.05 MB — are 0.61 of that tensor at this small decoder); the composed path on
    the same inputs exceeds that tensor, so the bound is not vacuous."""
    c = case("a")
    dec = decoder("a", "bf16")
    members, P = 64, 64
    G, n_fields, Cp = len(c["groups"]), 3, dec._n_inp_p
    z = torch.randn(members, P, G, c["D"], generator=torch.Generator().manual_seed(6)).to(DEV)
    member_tensor = members * P * n_fields * Cp * 4
    hidden = G * members * P * c["hidden"] * 2
    outputs = 2 * P * n_fields * Cp * 4
    bound = hidden + outputs + (1 << 20)

    def rise(fused):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        out = dec.member_moments(z, members, fused=fused)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, out

    rise(True), rise(False)    # shadow copies of the weights and the allocator's pools exist from here on
    r_fused, got = rise(True)
    r_comp, comp = rise(False)
    print(f"member_moments peak extra memory at {members} members x {P} patches: fused {r_fused} B, composed {r_comp} B, bound {bound} B, "
          f"one tensor of member fields {member_tensor} B")
    assert r_fused < bound, (r_fused, bound)
    assert r_fused <= member_tensor * 2 // 3, (r_fused, member_tensor)
    assert r_comp > member_tensor, (r_comp, member_tensor)
    assert rel(got[0].cpu(), comp[0].cpu()) <= 1e-5 and rel(got[1].cpu(), comp[1].cpu()) <= 1e-4      # the same fp32 Y, reduced in another order


def test_default_path_takes_the_fused_launch_from_4096_rows_on(monkeypatch):
    """fused=None: the composed path below 4096 rows (B * members * P), the fused launch from there on (the measured rule of Decode.member_moments:
    4096 rows is the smallest size at which the two paths were timed); fp32 never."""
    from sea_amd import ops

    c = case("a")
    P = 64
    z = torch.randn(64, P, len(c["groups"]), c["D"], generator=torch.Generator().manual_seed(31)).to(DEV)
    calls, real = [], ops.decode_member_moments
    monkeypatch.setattr(ops, "decode_member_moments", lambda *a, **k: (calls.append(a[0][0]["H"].shape[0]), real(*a, **k))[1])
    dec = decoder("a", "bf16")
    at = dec.member_moments(z, 32)                                            # 64 x 64 = 4096 rows, two histories
    assert calls == [4096]
    forced = dec.member_moments(z, 32, fused=True)
    assert torch.equal(at[0], forced[0]) and torch.equal(at[1], forced[1])
    calls.clear()
    below = dec.member_moments(z[:63], 63)                                    # 4032 rows
    comp = dec.member_moments(z[:63], 63, fused=False)
    assert calls == [] and torch.equal(below[0], comp[0]) and torch.equal(below[1], comp[1])
    decoder("a", "fp32").member_moments(z, 32)
    assert calls == []


# ------------------------------------------------------------------------------------------------ end to end
def test_ensemble_fields_on_a_rollout_session():
    """fork, step, weigh, resample gated by the effective sample size, forecast: EnsembleFields on the states and the log-weights as they come equals
    Decode.member_moments with the fp64-restated weights, within the parity bounds; both layouts; nothing is read back."""
    from sea_amd.ensemble import EnsembleFields, FieldLikelihood, systematic_resample
    from oracle.recipe import recipe_inputs
    from tests.test_input_grad_gpu import cfg_of
    from tests.test_model_gpu import build
    from tests.test_rollout_session_gpu import open_on

    c = case("a")
    P, D, n_mem, B, k = 4, c["D"], 8, 2, 3
    G = len(c["groups"])
    cfg = cfg_of(1, P * D, 4, G)
    m = build(cfg, "bf16")
    x, _, ib = recipe_inputs(B, k + 4, cfg, seed=9)
    dec = decoder("a", "bf16")
    g = torch.Generator().manual_seed(12)
    obs = torch.randn(B, P, 3, c["n_inp"], generator=g).to(DEV)
    counts = [12, 0, 7, 11]
    conds = torch.rand(B * n_mem, 1, generator=g).to(DEV)
    u = torch.rand(B, generator=g).to(DEV)

    ens = open_on(m, x, ib, k).fork(n_mem)
    y = ens.step(conds)
    logw = FieldLikelihood(dec, P, n_mem, counts=counts, sigma=[8.0, 8.0, 8.0], fused=True)(y, obs)
    _, logw_out, ess, resampled = systematic_resample(logw, n_mem, u=u, ess_threshold=0.5)
    fields = EnsembleFields(dec, P, n_mem, counts=counts, fused=True)
    z = y.reshape(B * n_mem, G, P, D).permute(0, 2, 1, 3)
    zh = z.cpu()
    raw = logw.clone()
    raw[3] = float("nan")                                                    # a dead member among the raw log-weights
    for lw in (logw_out, raw, None):
        wh = None if lw is None else torch.from_numpy(restate_weights(lw.cpu().numpy(), n_mem)).float()
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")                              # the counts were uploaded by the likelihood above (cached per counts object)
        try:
            mean, var = fields(y, logw=lw)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        assert mean.shape == (B, P, 3, c["n_inp"]) and var.shape == mean.shape and mean.is_cuda and mean.dtype == torch.float32
        direct = dec.member_moments(z, n_mem, weights=None if wh is None else wh.to(DEV), counts=counts, fused=True)
        comp = dec.member_moments(z, n_mem, weights=None if wh is None else wh.to(DEV), counts=counts, fused=False)
        r_mean, r_var, _ = restate_member_moments(c["w1"], c["w2"], c["b2"], c["groups"], zh, n_mem, wh, counts)
        e_m, ec_m, e_v, ec_v = rel(mean.cpu(), r_mean), rel(comp[0].cpu(), r_mean), rel(var.cpu(), r_var), rel(comp[1].cpu(), r_var)
        print(f"EnsembleFields resampled {resampled.tolist()} ess {ess.tolist()}: mean e {e_m:.3e} e_c {ec_m:.3e}; var e {e_v:.3e} e_c {ec_v:.3e}; "
              f"against member_moments with restated weights: mean {rel(mean.cpu(), direct[0].cpu()):.3e} var {rel(var.cpu(), direct[1].cpu()):.3e}")
        assert e_m <= TOL_BF16 and e_m <= 2 * ec_m + 1e-6 and e_v <= 2 * ec_v + 1e-6
        assert rel(mean.cpu(), direct[0].cpu()) <= 1e-5 and rel(var.cpu(), direct[1].cpu()) <= 1e-4      # float32 weights from tensor ops against the restated ones
        assert float(mean[:, 1].abs().max()) == 0.0 and float(var[:, 1].abs().max()) == 0.0                 # counts[1] == 0
        t_mean, t_var = fields(y, logw=lw, layout="BPCF")
        assert t_mean.shape == (B, P, c["n_inp"], 3) and torch.equal(t_mean.permute(0, 1, 3, 2), mean) and torch.equal(t_var.permute(0, 1, 3, 2), var)
        _, var_u = fields(y, logw=lw, unbiased=True)
        w64 = torch.full((B, n_mem), 1.0 / n_mem, dtype=torch.float64) if wh is None else wh.double().view(B, n_mem)
        assert rel(var_u.cpu(), var.cpu().double() / (1.0 - (w64 * w64).sum(1)).view(B, 1, 1, 1)) <= 1e-5
    ens.close()


def test_unpatch_spread_puts_the_spread_on_the_mesh_in_physical_units():
    """unpatch_spread(var.sqrt()) on the 3 x 4 partition of tests/golden/unpatch_3x4.npz: |a| * std gathered by the index map — no shift, and the sign
    of a negative scale does not reach a standard deviation."""
    from sea_amd.models.encoder_decoder import Decode
    from sea_amd.utils.data_processors import DataPartitioner2D, MeshUnpatcher, MinMaxScaler
    from tests.conftest import load_golden

    g = load_golden("unpatch_3x4")
    m, n = (int(v) for v in g["mn"])
    xy = torch.from_numpy(g["xy"])
    part = DataPartitioner2D(xy[0], xy[1], m=m, n=n, pad_id=-1, pad_field_value=0, device=DEV)
    idx = torch.from_numpy(g["index_map"])
    assert torch.equal(part.padded_index_map.cpu().long(), idx)
    P, C = idx.shape
    assert P == 12
    groups, D, members, B = [[0], [1]], 16, 8, 2
    scalers = []
    for rng_, lo, hi in (((-1, 1), -1.0, 3.0), ((1, -1), 0.5, 2.0)):             # the second inverse scale is negative: a = (2.0 - 0.5) / (-1 - 1)
        sc = MinMaxScaler(feature_range=rng_)
        sc.min_val, sc.max_val = torch.tensor(lo), torch.tensor(hi)
        scalers.append(sc)
    a = [sc.inverse_affine()[0] for sc in scalers]
    assert a[0] > 0 > a[1]
    torch.manual_seed(14)
    dec = Decode(groups, (C + 3) // 4 * 4, 40, D).requires_grad_(False).set_compute_dtype("bf16").to(DEV)
    z = torch.randn(B * members, P, 2, D, generator=torch.Generator().manual_seed(15)).to(DEV)
    counts = (idx >= 0).sum(1).tolist()
    mean, var = dec.member_moments(z, members, counts=counts, fused=True)
    std = var.sqrt()
    mu = MeshUnpatcher(part, groups, scalers)
    out = mu.unpatch_spread(std[..., :C])
    npts = xy.shape[1]
    assert out.shape == (B, npts, 2)
    ref = torch.zeros(B, npts, 2)
    sh = std.cpu()
    for p in range(P):
        for s in range(C):
            if idx[p, s] >= 0:
                for f in range(2):
                    ref[:, idx[p, s], f] = abs(a[f]) * sh[:, p, f, s]
    assert float(ref.min()) >= 0.0 and float(ref.max()) > 0.0
    assert rel(out.cpu(), ref) <= 1e-6 and float(out.min()) >= 0.0
    assert torch.equal(mu.unpatch_spread(std[..., :C].permute(0, 1, 3, 2).contiguous(), layout="BPCF"), out)
