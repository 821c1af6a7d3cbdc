"""Dense-snapshot score with a precision map and its latent gradient on the device: sea_decode_field_grad through Decode.field_loss and
FieldLikelihood.score_and_grad / nudge.

Reference: the fp64 restatement of the contract in tests/test_field_grad_cpu.py (`restate_field_grad`), which agrees with torch.autograd and, without
weights, with the reference fixtures' decoded-field loss.  The project's parity rule (tests/test_decode_loss_gpu.py, tests/test_sensor_grad_gpu.py): let
e(x) be the relative L2 error against the restatement and e_c the error of the composed bf16 path (forward() under autograd plus torch ops with the
same selects) on the same inputs; the fused launch must keep e(wsse), e(dz) <= 2e-2 and <= 2 e_c + 1e-6; the fp32 composed path <= 1e-4.  Besides the
whole tensors every member with at least MIN_LIVE weighted cells in a field is compared on its OWN rows (<= 2e-2): a single wrong cell weight passes
the whole-tensor bound (tests/test_field_grad_cpu.py shows it), not this one.

Shapes a, b, c of tests/test_decode_loss_gpu.case; c (hidden 624: the SP = 640 form with a masked contraction; 70 rows: two row tiles) in the splits
(35, 1), (7, 5), (5, 7), (1, 35) — a history boundary inside a tile — with counts None, [0, 160] and [1, 159].  Precision maps: tests/test_field_grad_cpu.precision_map
(30 % zeros, one patch all zero, one block with the last column alone live); every case runs without a field precision and with field 1 switched off."""
import pytest
import torch

from tests.test_decode_loss_cpu import rel
from tests.test_decode_loss_gpu import DEV, TOL_BF16, TOL_F32, case, decoder
from tests.test_field_grad_cpu import (MIN_LIVE, SPLITS, _weights_fp64, counts_sets, field_precision_of, host_case, live_cells, per_member_rel, precision_map,
                                       reference, restate_field_grad, snapshot)

pytestmark = pytest.mark.gpu


def run(dec, name, members, obs, pm=None, fp=None, counts=None, fused=True, z=None, upstream=None):
    """(wsse, dz) on the host of one Decode.field_loss call and its backward (of sum wsse, or of sum upstream * wsse)."""
    c = case(name)
    zz = (c["z"] if z is None else z).to(DEV).requires_grad_(True)
    wsse = dec.field_loss(zz, obs.to(DEV), members=members, counts=counts, precision=None if pm is None else pm.to(DEV),
                          field_precision=None if fp is None else fp.to(DEV), fused=fused)
    F = sum(len(g) for g in c["groups"])
    assert wsse.shape == (zz.shape[0], F) and wsse.dtype == torch.float32 and wsse.grad_fn is not None
    (wsse.sum() if upstream is None else (wsse * upstream.to(DEV)).sum()).backward()
    return wsse.detach().cpu(), zz.grad.detach().cpu()


def test_the_cases_are_those_of_the_decoded_field_loss_tests():
    for name in ("a", "b", "c"):
        a, b = case(name), host_case(name)
        assert a["groups"] == b["groups"] and a["counts"] == b["counts"]
        assert all(torch.equal(a[k], b[k]) for k in ("z", "target")) and all(torch.equal(x, y) for k in ("w1", "w2", "b2") for x, y in zip(a[k], b[k]))


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fused_score_and_gradient_against_fp64(name):
    c = case(name)
    dec = decoder(name, "bf16")
    for members, hist in SPLITS[name]:
        obs, pm = snapshot(name, hist), precision_map(name, hist)
        for counts in counts_sets(name):
            for with_fp in (False, True):
                fp = field_precision_of(name) if with_fp else None
                ref = reference(name, members, hist, None if counts is None else tuple(counts), with_fp)
                got = run(dec, name, members, obs, pm, fp, counts, fused=True)
                comp = run(dec, name, members, obs, pm, fp, counts, fused=False)
                per_field, _ = live_cells(obs, pm, fp, counts, members, c["B"], c["P"], c["groups"], c["n_inp"])
                enough = (per_field >= MIN_LIVE).any(1)
                tag = f"field_grad shape {name} members {members} x {hist} counts {counts} field_precision {with_fp}"
                for what, x, x_c, r in (("wsse", got[0], comp[0], ref[0]), ("dz", got[1], comp[1], ref[1])):
                    e, e_c, e_m = rel(x, r), rel(x_c, r), per_member_rel(x, r, enough)
                    print(f"{tag}: {what} fused e {e:.3e} composed e_c {e_c:.3e} worst member ({int(enough.sum())} compared) {e_m:.3e}")
                    assert e <= TOL_BF16 and e <= 2 * e_c + 1e-6, (tag, what, e, e_c)
                    assert e_m <= TOL_BF16, (tag, what, e_m)
                if with_fp:   # the field that is switched off scores exactly 0
                    assert float(got[0][:, 1].abs().max()) == 0.0


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fp32_composed_path_against_fp64(name):
    dec = decoder(name, "fp32")
    members, hist = SPLITS[name][1]
    obs, pm = snapshot(name, hist), precision_map(name, hist)
    for counts in counts_sets(name)[:2]:
        for with_fp in (False, True):
            fp = field_precision_of(name) if with_fp else None
            ref = reference(name, members, hist, None if counts is None else tuple(counts), with_fp)
            got = run(dec, name, members, obs, pm, fp, counts, fused=None)
            print(f"field_grad shape {name} members {members} x {hist} counts {counts} field_precision {with_fp}: fp32 e(wsse) {rel(got[0], ref[0]):.3e} "
                  f"e(dz) {rel(got[1], ref[1]):.3e}")
            assert rel(got[0], ref[0]) <= TOL_F32 and rel(got[1], ref[1]) <= TOL_F32


def _dead(name, obs, pm, fp, counts, hist):
    c = case(name)
    F = sum(len(g) for g in c["groups"])
    w, _ = _weights_fp64(obs, pm, fp, counts, 1, hist, c["P"], F, c["n_inp"])      # one row per (history, patch)
    return (w == 0).view(hist, c["P"], F, c["n_inp"])


@pytest.mark.parametrize("name,members,hist", [("a", 1, 2), ("b", 11, 3), ("c", 7, 5)])
def test_cells_without_weight_are_exactly_neutral(name, members, hist):
    """NaN in obs AND in precision at every cell beyond counts, with precision 0 or in the switched-off field, and in pad columns behind the cell:
    no bit of wsse or dz changes.  A patch without a live cell has dz exactly 0.  Negative and NaN precision act as 0."""
    c = case(name)
    dec = decoder(name, "bf16")
    C_, P = c["n_inp"], c["P"]
    obs, pm, fp = snapshot(name, hist), precision_map(name, hist), field_precision_of(name)
    for counts in counts_sets(name):
        base = run(dec, name, members, obs, pm, fp, counts)
        dead = _dead(name, obs, pm, fp, counts, hist)
        assert bool(dead.any()) and not bool(dead.all())
        width = C_ + 4                                                              # pad columns behind the cell, full of NaN
        obs2, pm2 = torch.full(tuple(obs.shape[:3]) + (width,), float("nan")), torch.full(tuple(obs.shape[:3]) + (width,), float("nan"))
        obs2[..., :C_], pm2[..., :C_] = obs, pm
        obs2[..., :C_][dead] = float("nan")
        pm2[..., :C_][dead] = float("nan")
        got = run(dec, name, members, obs2, pm2, fp, counts)
        assert torch.equal(base[0], got[0]) and torch.equal(base[1], got[1]), counts
        assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
        neg = pm.clone()
        neg[pm == 0] = -3.0
        got = run(dec, name, members, obs, neg, torch.where(fp > 0, fp, torch.full_like(fp, float("nan"))), counts)   # the field switched off by NaN
        assert torch.equal(base[0], got[0]) and torch.equal(base[1], got[1]), counts
        # (history 0, patch 0) has no live cell: its members' rows of dz are exactly 0, their other patches are not
        assert float(base[1][:members, 0].abs().max()) == 0.0
        if counts is None:
            assert float(base[1][:members, P - 1].abs().max()) > 0
        if counts is not None:
            for p, n in enumerate(counts):
                if n == 0:
                    assert float(base[1][:, p].abs().max()) == 0.0


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_a_member_does_not_depend_on_the_split_or_its_row_tile(name):
    """Every history sees the same snapshot and map, so every member has the same observation in every split: the same bits of wsse and dz in all of
    them; member 0 of the (B, 1) call equals a 1-member call on its own rows; two runs give the same bits."""
    c = case(name)
    dec = decoder(name, "bf16")
    obs1, pm1, fp = snapshot(name, 1), precision_map(name, 1), field_precision_of(name)
    for counts in counts_sets(name):
        outs = []
        for members, hist in SPLITS[name]:
            outs.append(run(dec, name, members, obs1.expand(hist, -1, -1, -1).contiguous(), pm1.expand(hist, -1, -1, -1).contiguous(), fp, counts))
        for o in outs[1:]:
            assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]), counts
        assert float(outs[0][0].abs().max()) > 0 and float(outs[0][1].abs().max()) > 0
        alone = run(dec, name, 1, obs1, pm1, fp, counts, z=c["z"][:1])
        assert torch.equal(alone[0][0], outs[0][0][0]) and torch.equal(alone[1][0], outs[0][1][0]), counts
        last = run(dec, name, 1, obs1, pm1, fp, counts, z=c["z"][-1:])               # a row of the last tile, moved to row 0
        assert torch.equal(last[0][0], outs[0][0][-1]) and torch.equal(last[1][0], outs[0][1][-1]), counts
        again = run(dec, name, *SPLITS[name][0][:1], obs1, pm1, fp, counts)
        assert torch.equal(again[0], outs[0][0]) and torch.equal(again[1], outs[0][1])


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_score_only_launch_has_the_bits_of_the_gradient_launch(name):
    from sea_amd import ops

    c = case(name)
    dec = decoder(name, "bf16")
    members, hist = SPLITS[name][1]
    obs, pm, fp = snapshot(name, hist), precision_map(name, hist), field_precision_of(name)
    for counts in counts_sets(name):
        wsse, _ = run(dec, name, members, obs, pm, fp, counts)
        z = c["z"].to(DEV)
        with torch.no_grad():
            a = dec.field_loss(z.clone().requires_grad_(True), obs.to(DEV), members=members, counts=counts, precision=pm.to(DEV), field_precision=fp.to(DEV), fused=True)
            assert ops.last_form()[:2] == ("field_grad.rows64", 0)
        b = dec.field_loss(z, obs.to(DEV), members=members, counts=counts, precision=pm.to(DEV), field_precision=fp.to(DEV), fused=True)   # z does not require grad
        assert a.grad_fn is None and b.grad_fn is None
        assert torch.equal(a.cpu(), wsse) and torch.equal(b.cpu(), wsse), counts


def test_the_entry_point_writes_every_element_and_refuses_dh_in_some_groups():
    from sea_amd import ops

    name = "a"
    c = case(name)
    dec = decoder(name, "bf16")
    z = c["z"].to(DEV)
    hid, pre = dec._first_layer(z, torch.bfloat16)
    _, W2 = dec._weights(torch.bfloat16)
    G, P, C_ = len(hid), c["P"], c["n_inp"]
    obs = snapshot(name, 1).reshape(P, 3, C_).to(DEV)
    pm = precision_map(name, 1).reshape(P, 3, C_).to(DEV)
    dpre = [torch.full_like(h, float("nan")) for h in hid]
    groups = [dict(H=hid[g], W2=W2[g], bias=dec._shadow[3][g], dH=dpre[g], Z=pre[g]) for g in range(G)]
    work = torch.full((z.shape[0] * P * 3 + 5,), float("nan"), device=DEV)
    wsse = ops.decode_field_grad(groups, obs, C_, dec._n_inp_p, P, members=2, prec=pm, counts=torch.tensor(c["counts"], dtype=torch.int32, device=DEV), work=work)
    assert ops.last_form()[:2] == ("field_grad.rows64", 1)
    assert all(bool(torch.isfinite(d.float()).all()) for d in dpre) and bool(torch.isfinite(wsse).all())
    assert bool(torch.isfinite(work[:-5]).all()) and bool(torch.isnan(work[-5:]).all())          # its M * n_fields elements, and nothing behind them
    del groups[1]["dH"]
    with pytest.raises(ValueError, match="all of them, or none"):
        ops.decode_field_grad(groups, obs, C_, dec._n_inp_p, P, members=2, prec=pm)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_without_weights_it_ties_to_member_sse_and_mse_loss(name):
    """No map, no field precision: wsse against Decode.member_sse(fused=True), and with one member per snapshot the gradient of sum wsse against
    n_valid * the gradient of Decode.mse_loss(fused=True).  Different launches round different tiles: TOL_BF16, not bit equality."""
    c = case(name)
    dec = decoder(name, "bf16")
    B, P, C_ = c["B"], c["P"], c["n_inp"]
    F = sum(len(g) for g in c["groups"])
    tgt = c["target"]
    for counts in counts_sets(name)[:2]:
        members, hist = SPLITS[name][1]
        wsse, _ = run(dec, name, members, tgt[:hist].contiguous(), None, None, counts)
        sse = dec.member_sse(c["z"].to(DEV), tgt[:hist].contiguous().to(DEV), counts=counts, members=members, fused=True).cpu()
        wsse1, dz1 = run(dec, name, 1, tgt, None, None, counts)
        z = c["z"].to(DEV).requires_grad_(True)
        Cw = (C_ + 3) // 4 * 4
        t = torch.zeros(B, P, F, Cw)
        t[..., :C_] = tgt
        loss = dec.mse_loss(z, t.to(DEV), counts=counts, fused=True)
        loss.backward()
        n_valid = B * F * (P * C_ if counts is None else sum(counts))
        e_s, e_l, e_g = rel(wsse, sse), rel(wsse1.sum(), loss.detach().cpu() * n_valid), rel(dz1, z.grad.cpu() * n_valid)
        print(f"field_grad shape {name} counts {counts}: no weights, against member_sse e {e_s:.3e}; against mse_loss e(loss) {e_l:.3e} e(dz) {e_g:.3e}")
        assert e_s <= TOL_BF16 and e_l <= TOL_BF16 and e_g <= TOL_BF16


def test_upstream_gradients_per_member_and_group():
    """The documented contract of the backward: an upstream gradient per member and field GROUP scales the saved gradient; one that differs between the
    fields of a group turns that member's slice of that group into NaN, and nothing else."""
    name = "a"                                                                       # groups [[0, 1], [2]]
    c = case(name)
    dec = decoder(name, "bf16")
    obs, pm, fp = snapshot(name, 1), precision_map(name, 1), torch.tensor([1.5, 0.25, 0.5])
    _, dz = run(dec, name, 2, obs, pm, fp, c["counts"])
    up_g = torch.tensor([[0.5, -2.0], [3.0, 0.25]])
    up = torch.stack([up_g[:, 0], up_g[:, 0], up_g[:, 1]], 1)
    _, dz_up = run(dec, name, 2, obs, pm, fp, c["counts"], upstream=up)
    assert torch.equal(dz_up, dz * up_g.view(2, 1, 2, 1))
    ref = restate_field_grad(c["w1"], c["w2"], c["b2"], c["groups"], c["z"], obs, pm, fp, c["counts"], 2)[1] * up_g.double().view(2, 1, 2, 1)
    assert rel(dz_up, ref) <= TOL_BF16
    up[1, 1] = 7.0                                                                   # member 1: fields 0 and 1 of group 0 disagree
    _, dz_bad = run(dec, name, 2, obs, pm, fp, c["counts"], upstream=up)
    assert bool(torch.isnan(dz_bad[1, :, 0]).all()) and torch.equal(dz_bad[0], dz_up[0]) and torch.equal(dz_bad[1, :, 1], dz_up[1, :, 1])


def _states(name):
    """What a rollout session returns for the case's latents: [Bm, n_groups, P * D] (the inverse of the likelihoods' re-layout)."""
    z = case(name)["z"]
    Bm, P, G, D = z.shape
    return z.permute(0, 2, 1, 3).reshape(Bm, G, P * D).contiguous()


@pytest.mark.parametrize("name,members,hist", [("a", 2, 1), ("b", 11, 3), ("b", 1, 33)])
def test_field_likelihood_score_and_grad_and_nudge(name, members, hist):
    from sea_amd.ensemble import FieldLikelihood

    c = case(name)
    dec = decoder(name, "bf16")
    P, G, D, Bm, C_ = c["P"], len(c["groups"]), c["D"], c["B"], c["n_inp"]
    counts, sigma = c["counts"], [0.5, 1.0, 2.0]
    obs, pm = snapshot(name, hist), precision_map(name, hist)
    y = _states(name).to(DEV)
    obs_d, pm_d = obs.to(DEV), pm.to(DEV)
    like = FieldLikelihood(dec, P, members, counts=counts, sigma=sigma, fused=True)

    # without a precision: today's call, bit for bit
    z = c["z"].to(DEV)
    today = (dec.member_sse(z, obs_d, counts=counts, members=members, fused=True) * like._field_scale(z.device)).sum(1)
    assert torch.equal(like(y, obs_d), today) and torch.equal(like(y, obs_d, "BPFC"), today)

    fp = 1.0 / torch.tensor(sigma, dtype=torch.float64) ** 2
    restated = lambda zz: restate_field_grad(c["w1"], c["w2"], c["b2"], c["groups"], zz, obs, pm, fp, counts, members)   # noqa: E731
    relayout = lambda t: t.reshape(Bm, G, P, D).permute(0, 2, 1, 3)                  # noqa: E731
    wsse0, dz0 = restated(c["z"])
    logw_ref, grad_ref = -0.5 * wsse0.sum(1), (-0.5 * dz0).permute(0, 2, 1, 3).reshape(Bm, G, P * D)
    like(y, obs_d, pm_d), like.score_and_grad(y, obs_d, pm_d)                        # the first calls upload the counts and build sigma's tensors
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                                          # nothing is read back
    try:
        logw_call = like(y, obs_d, pm_d)
        logw, grad = like.score_and_grad(y, obs_d, pm_d)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert logw.shape == (Bm,) and grad.shape == y.shape and grad.dtype == torch.float32
    assert torch.equal(logw, logw_call)                                              # the score-only launch and the gradient launch: the same bits
    comp = FieldLikelihood(dec, P, members, counts=counts, sigma=sigma, fused=False).score_and_grad(y, obs_d, pm_d)
    for what, x, x_c, r in (("logw", logw, comp[0], logw_ref), ("dlogw_dy", grad, comp[1], grad_ref)):
        e, e_c = rel(x.cpu(), r), rel(x_c.cpu(), r)
        print(f"FieldLikelihood shape {name} members {members} x {hist}: {what} fused e {e:.3e} composed e_c {e_c:.3e}")
        assert e <= TOL_BF16 and e <= 2 * e_c + 1e-6
    # the reference's layout: the same bits
    like_ref = FieldLikelihood(dec, P, members, counts=counts, sigma=sigma, layout="BPCF", fused=True)
    lw2, g2 = like_ref.score_and_grad(y, obs_d.permute(0, 1, 3, 2).contiguous(), pm_d.permute(0, 1, 3, 2).contiguous())
    assert torch.equal(lw2, logw) and torch.equal(g2, grad)
    assert torch.equal(like.score_and_grad(y, obs_d.permute(0, 1, 3, 2).contiguous(), pm_d.permute(0, 1, 3, 2).contiguous(), layout="BPCF")[1], grad)

    # nudge is y + rate * dlogw_dy, bit for bit, for a number and for a rate per member
    rate = 0.125
    y1 = like.nudge(y, obs_d, pm_d, rate=rate)
    assert y1.dtype == y.dtype and torch.equal(y1, (y.float() + rate * grad).to(y.dtype))
    assert torch.equal(like.nudge(y, obs_d, pm_d, rate=torch.full((Bm,), rate, device=DEV)), y1)
    assert torch.equal(like.nudge(y, obs_d, pm_d, rate=0.0), y)

    # the sign of the gradient: a small step from rate 0 raises the fp64-restated log-weight of EVERY member that has a live cell.  The step length
    # comes from the restatement alone: halved until the restated gradient raises every such member, then halved once more
    per_field, _ = live_cells(obs, pm, fp, counts, members, Bm, P, c["groups"], C_)
    alive = per_field.sum(1) > 0
    assert int(alive.sum()) >= Bm - 1
    logw_of = lambda zz: -0.5 * restated(zz)[0].sum(1)                               # noqa: E731
    step = 1.0
    while step > 1e-9 and not bool((logw_of(c["z"].double() + step * (-0.5 * dz0))[alive] > logw_ref[alive]).all()):
        step *= 0.5
    step *= 0.5
    assert step > 1e-9
    y_step = like.nudge(y, obs_d, pm_d, rate=step)
    after = logw_of(relayout(y_step.cpu().double()))
    gain = (after - logw_ref)[alive]
    print(f"FieldLikelihood shape {name} members {members} x {hist}: nudge with rate {step:g} raises the restated logw of {int(alive.sum())} members by "
          f"{float(gain.min()):.3e} .. {float(gain.max()):.3e}")
    assert bool((gain > 0).all())
    assert torch.equal(after[~alive], logw_ref[~alive])                              # a member without a live cell does not move


def test_single_trajectory_nudge_from_a_gappy_frame_without_sigma():
    """members = 1, no sigma, no counts: the case no other dense tool covers."""
    from sea_amd.ensemble import FieldLikelihood

    name = "c"
    c = case(name)
    dec = decoder(name, "bf16")
    obs, pm = snapshot(name, 35), precision_map(name, 35)
    y = _states(name).to(DEV)
    like = FieldLikelihood(dec, c["P"], 1, fused=True)
    logw, grad = like.score_and_grad(y, obs.to(DEV), pm.to(DEV))
    wsse, dz = reference(name, 1, 35, None, False)
    e_w, e_g = rel(logw.cpu(), -0.5 * wsse.sum(1)), rel(grad.cpu(), (-0.5 * dz).permute(0, 2, 1, 3).reshape(y.shape))
    print(f"FieldLikelihood shape c, single trajectories: logw e {e_w:.3e} dlogw_dy e {e_g:.3e}")
    assert e_w <= TOL_BF16 and e_g <= TOL_BF16
    assert float(grad[0, :, :c["D"]].abs().max()) == 0.0                               # (history 0, patch 0) is masked out: that slice of the state is not pulled
