"""The packed form of the CRPS loss launch on the device: sea_decode_member_crps_grad_packed (ops.decode_member_crps_grad(pack=True)) against the unpacked
entry point on the same operands.  Every comparison is BIT equality (`same`), so no tolerance appears: loss, sums, status and every dH of the packed form
are the unpacked form's.  Base shapes: P = 2, F = 2, C = 40 in Cp = 64, counts (40, 33) and (0, 1), S = 264 unless a test says otherwise; the operands are
tests/test_crps_loss_gpu.py's edge_case (exact quarter-integer decodes, a precision map with a tenth of the cells dead and obs NaN there, log-weights with
a dominant and a dead member)."""
from unittest import mock

import pytest
import torch

from tests.test_crps_loss_gpu import BF, DEV, autograd_case, dev, edge_case, loss_and_grad, reference, same
from tests.test_decode_loss_gpu import case, decoder
from tests.test_field_verify_gpu import X_COUNTS, exact_case

pytestmark = pytest.mark.gpu

COUNTS = ((40, 33), (0, 1))
S0 = 264


def run(t, n, pack, unbiased=True, groups=None, P=2, hist=None, fw=None, Z=None, fill=float("nan"), with_prec=True, with_counts=True):
    """ops.decode_member_crps_grad(pack=pack) on a case dict, as tests/test_crps_loss_gpu.py's run_crps (hist: that history alone); the outputs' buffers are
    prefilled with `fill`.  Returns (loss, sums, status, dH per group, the noted form)."""
    from sea_amd import ops

    H, obs, prec, logw = t["H"], t["obs"], (t["prec"] if with_prec else None), t["logw"]
    F = obs.shape[1]
    groups = ((0, F),) if groups is None else groups
    if hist is not None:
        H, obs = H[hist * n * P:(hist + 1) * n * P], obs[hist * P:(hist + 1) * P]
        prec = None if prec is None else prec[hist * P:(hist + 1) * P]
        logw = None if logw is None else logw[hist * n:(hist + 1) * n]
        Z = None if Z is None else Z[hist * n * P:(hist + 1) * n * P]
    Cp = t["Cp"]
    Hd = H.to(DEV).to(BF)
    grp = []
    for f0, nf in groups:
        grp.append(dict(H=Hd, W2=t["W2"][f0 * Cp:(f0 + nf) * Cp].to(DEV).to(BF).contiguous(), bias=t["bias"][f0 * Cp:(f0 + nf) * Cp].to(DEV).contiguous(),
                        dH=torch.full(tuple(H.shape), fill, device=DEV, dtype=BF)))
        if Z is not None:
            grp[-1]["Z"] = Z.to(DEV).to(BF)
    loss, sums, status = ops.decode_member_crps_grad(grp, obs.to(DEV), t["C"], Cp, P, n, prec=dev(prec), field_weight=dev(fw), counts=dev(t["counts"]) if with_counts else None,
                                                     logw=dev(logw), unbiased=unbiased, pack=pack)
    return loss, sums, status, [g["dH"] for g in grp], ops.last_form()


def form_of(S, n):
    from sea_amd import ops

    NP, HG = ops.decode_member_crps_pack_shape(S, n)
    return "decode.member_crps_grad.pk%d%s" % (NP, "" if HG == 64 // NP else "h%d" % HG), HG


def assert_same(a, b, tag):
    assert same(a[0], b[0]), (tag, "loss")
    assert same(a[1], b[1]), (tag, "sums")
    assert torch.equal(a[2], b[2]), (tag, "status")
    assert len(a[3]) == len(b[3])
    for x, y in zip(a[3], b[3]):
        assert not bool(torch.isnan(x.float()).any()), (tag, "dH not fully written")
        assert same(x, y), (tag, "dH")


def compare(t, n, tag, S, **kw):
    """pack=True against pack=False on the same operands; the noted forms are the packed one and an unpacked one."""
    want, _ = form_of(S, n)
    a = run(t, n, True, **kw)
    assert a[4][0] == want and a[4][1] == (S + 127) // 128 * 128, (tag, a[4], want)
    b = run(t, n, False, **kw)
    assert b[4][0] in ("decode.member_crps_grad.w8", "decode.member_crps_grad.w4"), (tag, b[4])
    assert_same(a, b, tag)
    return a


# ------------------------------------------------------------------------------------------------ 1: member and history edges
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 9, 16, 17, 32])
def test_member_and_history_edges(n):
    """A segment narrower than NP (1, 3, 5, 9, 17 members), a full one, and the histories 1, HG - 1, HG, HG + 1 and 2 HG + 1: a last group with missing
    histories, one history alone in its group."""
    _, HG = form_of(S0, n)
    done = []
    for B in sorted({1, max(HG - 1, 1), HG, HG + 1, 2 * HG + 1}):
        for counts in COUNTS:
            t = edge_case(n, 2, 40, 64, S0, B, 2, counts, 7000 + 64 * n + B)
            a = compare(t, n, (n, B, counts), S0)
            assert bool((a[2] > 0).all())                                                           # every history is scored
        done.append(B)
    print(f"crps pack N = {n} (HG = {HG}): B in {done} x counts {COUNTS}: loss, sums, status and dH bit-equal to the unpacked form")


# ------------------------------------------------------------------------------------------------ 2: exact operands
@pytest.mark.parametrize("n", [2, 16])
def test_gradient_is_exact_on_exact_operands_through_the_packed_form(n):
    """tests/test_crps_loss_gpu.py's exactness claim (equal weights, unbiased=False, N a power of two: dH EQUALS the fp64 restatement rounded once),
    through the packed form."""
    want, _ = form_of(40, n)
    for counts in X_COUNTS:
        for wp in (False, True):
            t = exact_case(n, counts, wp, False)
            ref = reference(t, n, False)
            loss, sums, status, (dH,), form = run(t, n, True, unbiased=False)
            assert form[0] == want
            assert not bool(torch.isnan(dH.float()).any()) and not bool(torch.isnan(loss).any()) and not bool(torch.isnan(sums).any())
            assert torch.equal(dH.cpu().view(torch.int16), ref["dH_exact"][0].to(torch.float32).to(BF).view(torch.int16)), (n, counts, wp)
            assert torch.equal(sums[..., 0].cpu(), ref["count"])
    print(f"crps pack N = {n}: dH equals the fp64 restatement rounded once on exact operands (4 cases)")


# ------------------------------------------------------------------------------------------------ 3: dead and unscored segments inside a group
@pytest.mark.parametrize("n", [4, 16])
def test_dead_and_unscored_segments_inside_a_packed_group(n):
    _, HG = form_of(S0, n)
    B, P = HG + 1, 2
    t = dict(edge_case(n, 2, 40, 64, S0, B, P, (40, 33), 7900 + n))                             # obs is NaN wherever the precision is 0
    assert bool(torch.isnan(t["obs"][t["prec"] == 0]).all()) and bool((t["prec"] == 0).any())
    lw = torch.zeros(B, n)
    lw[0, 1] = float("-inf")                                                                    # a dead member
    nan_h, dead_h = 1, min(2, B - 1)
    lw[nan_h, 0] = float("nan")                                                                 # a history that is not scored
    if dead_h != nan_h:
        lw[dead_h, :] = float("-inf")                                                           # no live member
    t["logw"] = lw.reshape(-1)
    a = run(t, n, True, fill=7.0)
    b = run(t, n, False, fill=7.0)
    assert_same(a, b, ("dead segments", n))                                                     # the neighbours' bits included
    loss, sums, status, (dH,), _ = a
    rows = dH.view(B, n, P, S0).float()
    want = [n] * B
    want[0], want[nan_h], want[dead_h] = n - 1, -1, -1
    assert status.tolist() == want
    assert float(rows[0, 1].abs().max()) == 0.0 and float(rows[0, 0].abs().max()) > 0.0        # exactly 0 over the prefill
    for h in {nan_h, dead_h}:
        assert float(rows[h].abs().max()) == 0.0 and float(loss[h].abs().max()) == 0.0 and float(sums[h].abs().max()) == 0.0
    assert float(loss[0].min()) > 0.0 and float(loss[B - 1].min()) > 0.0
    for h in range(B):                                                                          # each history's outputs: those of a call holding it alone
        alone = run(t, n, True, hist=h, fill=3.0)
        r = n * P
        assert same(alone[0][0], loss[h]) and same(alone[1][0], sums[h]) and int(alone[2][0]) == int(status[h]) and same(alone[3][0], dH[h * r:(h + 1) * r]), h
    print(f"crps pack N = {n}, B = {B}: a dead member, a NaN log-weight, a history without live members, obs NaN at precision 0: status {want[:4]}.., zero rows exact, "
          f"every history equal to a call holding it alone")


# ------------------------------------------------------------------------------------------------ 4: the edges of the launch
def test_two_column_chunks():
    n, C_, Cp = 4, 530, 544
    _, HG = form_of(40, n)
    for counts in ((C_, 513), (512, 1)):                                                        # 17 tiles: two chunks; 512 leaves the second chunk nothing
        t = edge_case(n, 2, C_, Cp, 40, HG + 1, 2, counts, 8100)
        compare(t, n, ("two chunks", counts), 40)


@pytest.mark.parametrize("n,S", [(4, 136), (4, 392), (8, 640), (2, 640), (2, 512), (32, 520)])
def test_hidden_widths(n, S):
    """S = 136 (padded to 256 by masking); the 4-wave instantiations above S = 384, with the one that runs 16 histories per workgroup (2 members at S = 640)
    and the fullest LDS (2 members at S = 512: 32 histories)."""
    name, HG = form_of(S, n)
    assert (name == "decode.member_crps_grad.pk2h16") == (n == 2 and S == 640)
    B = HG + 1 if HG <= 16 else 33
    t = edge_case(n, 2, 40, 64, S, B, 2, (40, 33), 8200 + S + n)
    compare(t, n, (n, S), S)


def test_two_groups_with_gelu_grad_and_a_zero_field_weight():
    n, F, P = 5, 3, 2
    _, HG = form_of(40, n)
    t = edge_case(n, F, 40, 64, 40, HG + 1, P, (40, 33), 8300)
    Z = torch.randint(-12, 13, tuple(t["H"].shape), generator=torch.Generator().manual_seed(8301)).float() / 4
    fw = torch.tensor([1.0, 0.0, 0.5])
    a = compare(t, n, "two groups, Z, field weights 1, 0, 0.5", 40, groups=((0, 2), (2, 1)), Z=Z, fw=fw)
    assert float(a[0][:, 1].abs().max()) == 0.0 and float(a[0][:, 0].min()) > 0.0


@pytest.mark.parametrize("what", ["prec None", "counts None", "biased", "unbiased"])
def test_optional_operands(what):
    n = 3
    _, HG = form_of(S0, n)
    t = edge_case(n, 2, 40, 64, S0, HG + 1, 2, (40, 33), 8400)
    kw = {"prec None": dict(with_prec=False), "counts None": dict(with_counts=False), "biased": dict(unbiased=False), "unbiased": dict(unbiased=True)}[what]
    if what == "prec None":                                                                     # without the precision map every cell is live: obs must be finite
        t = dict(t, obs=torch.nan_to_num(t["obs"], nan=0.25))
    compare(t, n, what, S0, **kw)


# ------------------------------------------------------------------------------------------------ 5: refusals
def test_refusals():
    t = edge_case(33, 1, 40, 64, 40, 1, 1, (40,), 8500)
    with pytest.raises(RuntimeError, match="sea_decode_member_crps_grad_packed: unsupported: members=33 above 32"):
        run(t, 33, True, P=1)
    k = autograd_case()
    c = case("a")
    dec = decoder("a", "bf16")
    n = 33
    z = torch.randn(n, k["P"], k["G"], c["D"], generator=torch.Generator().manual_seed(8501)).to(DEV).requires_grad_(True)
    obs = k["obs"][:1].to(DEV)
    with pytest.raises(ValueError, match=r"the packed form carries 1 \.\. 32 members"):
        dec.member_crps_loss(z, obs, n, fused=True, pack=True)
    loss, _ = dec.member_crps_loss(z, obs, n, fused=True)                                      # pack=None falls back silently: the unpacked form
    loss.sum().backward()
    assert bool(torch.isfinite(z.grad).all())


# ------------------------------------------------------------------------------------------------ 6: through the Python surface
def test_member_crps_loss_and_ensemble_loss_with_pack():
    from sea_amd import ops
    from sea_amd.utils.train_utils import EnsembleCRPSLoss

    k = autograd_case()
    c = case("a")
    dec = decoder("a", "bf16")
    real = ops.decode_member_crps_grad
    seen = []

    def spy(*a, **kw):
        out = real(*a, **kw)
        seen.append((kw.get("pack"), ops.last_form()[0]))
        return out

    with mock.patch.object(ops, "decode_member_crps_grad", side_effect=spy):
        lp, cp, gp = loss_and_grad(dec, k, True, pack=True)
        lq, cq, gq = loss_and_grad(dec, k, True, pack=True)
        lu, cu, gu = loss_and_grad(dec, k, True, pack=False)
        ln, cn, gn = loss_and_grad(dec, k, True)                                                # pack=None at a tiny shape: the unpacked form
    assert [s[0] for s in seen] == [True, True, False, False]
    assert seen[0][1] == "decode.member_crps_grad.pk4" and seen[2][1] == seen[3][1] == "decode.member_crps_grad.w8"
    assert same(lp, lu) and torch.equal(cp, cu) and same(gp, gu) and float(gp.abs().max()) > 0.0
    assert same(lp, lq) and same(gp, gq)                                                        # two runs, the same bits
    assert same(ln, lu) and same(gn, gu)

    B, n, P, G, D, F = k["B"], k["n"], k["P"], k["G"], c["D"], k["F"]
    T = 2
    g = torch.Generator().manual_seed(8600)
    out0 = torch.randn(B * n, T, G, P * D, generator=g)
    fields = torch.randn(B, T, P, F, c["n_inp"], generator=g).to(DEV)
    res = {}
    for pack in (True, False):
        out = out0.to(DEV).requires_grad_(True)
        loss = EnsembleCRPSLoss(dec, P, n, counts=k["counts"], fused=True, pack=pack)(out, fields)
        loss.backward()
        res[pack] = (loss.detach(), out.grad.detach())
    assert same(res[True][0], res[False][0]) and same(res[True][1], res[False][1]) and float(res[True][1].abs().max()) > 0.0
    print(f"crps pack through Decode.member_crps_loss and EnsembleCRPSLoss (2 histories x 4 members x 3 patches): loss and gradients bit-equal to pack=False; forms {seen}")


def test_pack_none_takes_the_packed_form_at_the_measured_sizes():
    """4 members x 64 histories x 64 patches = 16384 rows, the smallest measured size: pack=None resolves to the packed form there, with pack=False's bits."""
    from sea_amd import ops

    c = case("a")
    dec = decoder("a", "bf16")
    B, n, P, G, F = 64, 4, 64, len(c["groups"]), sum(len(g) for g in c["groups"])
    g = torch.Generator().manual_seed(8700)
    z0 = torch.randn(B * n, P, G, c["D"], generator=g).to(DEV)
    obs = torch.randn(B, P, F, c["n_inp"], generator=g).to(DEV)
    real, seen, res = ops.decode_member_crps_grad, [], {}

    def spy(*a, **kw):
        out = real(*a, **kw)
        seen.append((kw.get("pack"), ops.last_form()[0]))
        return out

    with mock.patch.object(ops, "decode_member_crps_grad", side_effect=spy):
        for pack in (None, False):
            z = z0.clone().requires_grad_(True)
            loss, _ = dec.member_crps_loss(z, obs, n, pack=pack)
            loss.sum().backward()
            res[pack] = (loss.detach(), z.grad.detach())
    assert seen == [(True, "decode.member_crps_grad.pk4"), (False, "decode.member_crps_grad.w8")], seen
    assert same(res[None][0], res[False][0]) and same(res[None][1], res[False][1]) and float(res[None][1].abs().max()) > 0.0
