"""The CRPS of the decoded fields as a loss, on the device: sea_decode_member_crps_grad through ops.decode_member_crps_grad, Decode.member_crps_loss and
EnsembleCRPSLoss through a temporal model.

Reference: `restate_crps_grad` of tests/test_crps_loss_cpu.py (the fp64 restatement of the CRPS and of its derivative, tied there to torch.autograd of
the pairwise formula) on the exact operands of tests/test_field_verify_gpu.py (`exact_case`: the decoded values are exact quarter-integers).
  exact       equal weights, unbiased=False, N a power of two: G is exactly representable in bf16 (tests/test_crps_loss_cpu.py verifies the premise: the
              trailing bf16 term of G is then 0), the second product then adds at most 80 multiples of 1 / N^2 of at most 2 / N — exact in fp32 in any order — so dH with Z = NULL EQUALS the
              restatement rounded to bf16 once, bit for bit; loss has the bits of float32(sums[..., 1]) of ops.decode_member_verify on the same operands
  general     loss within SUMS_TOL max(1, |ref|) (tests/test_field_verify_gpu.py's derived bound); dH per element within
              2^-9 (|dH_ref| + sum_c |G_ref| |W2|) + 40 * 2^-24 sum_c |G_ref| |W2|: one bf16 ulp on every rounded operand and on the output, fp32
              accumulation over 40 terms — derived, not measured (with Z: dH_ref carries gelu'(Z) in fp64)
  end to end  bf16 fused: e <= 2 e_c + 1e-6 for z.grad (e: against the fp64 restatement on fp64-decoded values; e_c: fused=False on the same inputs —
              the project's rule in tests/test_field_verify_gpu.py); through a temporal model the same rule per parameter tensor, against the run with the
              fp32 decoder on the composed path"""
import functools
import math

import pytest
import torch

from tests.test_crps_loss_cpu import restate_crps_grad
from tests.test_decode_loss_cpu import rel
from tests.test_decode_loss_gpu import DEV, TOL_BF16, case, decoder
from tests.test_field_verify_cpu import field_logw
from tests.test_field_verify_gpu import SUMS_TOL, X_B, X_COUNTS, X_F, X_P, X_S, exact_case

pytestmark = pytest.mark.gpu

F64 = torch.float64
BF = torch.bfloat16


def dev(t):
    return None if t is None else t.to(DEV)


def gelu_grad64(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def run_crps(t, n, unbiased, groups=((0, X_F),), P=X_P, hist=None, fw=None, Z=None, fill=float("nan")):
    """ops.decode_member_crps_grad on a case dict (H, W2 [F * Cp, S], bias, obs [B * P, F, C], prec, logw, counts, C, Cp); groups: (first field, fields) per
    group, all reading the same hidden rows; hist: that history alone.  Returns (loss, sums, status, dH [M, S] per group), the outputs' buffers
    prefilled with `fill`."""
    from sea_amd import ops

    H, obs, prec, logw = t["H"], t["obs"], t["prec"], t["logw"]
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
    loss, sums, status = ops.decode_member_crps_grad(grp, obs.to(DEV), t["C"], Cp, P, n, prec=dev(prec), field_weight=dev(fw), counts=dev(t["counts"]), logw=dev(logw),
                                                     unbiased=unbiased)
    return loss, sums, status, [g["dH"] for g in grp]


def reference(t, n, unbiased, groups=((0, X_F),), fw=None, Z=None):
    """dict(loss [B, F], count, dH [M, S] per group in fp64 from G rounded to bf16 (what the contract multiplies), absW = sum_c |G| |W2| per group (with Z:
    dH carries gelu'(Z), the bound's sum does not)) from the restatement on the case's exact decoded values."""
    B, P, F, C_ = t["w"].shape
    r = restate_crps_grad(t["Y"], t["obs"].view(B, P, F, -1), t["w"], t["logw"], n, unbiased, fw)
    M, Cp = t["H"].shape[0], t["Cp"]
    G = r["G"].reshape(M, F, C_)
    Gb = G.to(torch.float32).to(BF).to(F64)
    dH, dH_exact, absW = [], [], []
    for f0, nf in groups:
        W = t["W2"].view(F, Cp, -1)[f0:f0 + nf, :C_].to(BF).to(F64).reshape(nf * C_, -1)       # [nf C, S]
        gz = 1.0 if Z is None else gelu_grad64(Z.to(BF).to(F64))
        dH.append((Gb[:, f0:f0 + nf].reshape(M, -1) @ W) * gz)
        dH_exact.append((G[:, f0:f0 + nf].reshape(M, -1) @ W) * gz)
        absW.append(G[:, f0:f0 + nf].reshape(M, -1).abs() @ W.abs())                              # the bound's sum as it is stated: without gelu'(Z)
    return dict(loss=r["loss"], count=r["count"], dH=dH, dH_exact=dH_exact, absW=absW, G=r["G"])


def dh_ratio(got, ref_dh, absW):
    """max over the elements of |got - ref| / bound, bound = 2^-9 (|ref| + absW) + 40 * 2^-24 absW; an element whose bound is 0 must be exactly 0."""
    got = got.cpu().to(F64)
    bound = 2.0 ** -9 * (ref_dh.abs() + absW) + 40 * 2.0 ** -24 * absW
    err = (got - ref_dh).abs()
    zero = bound == 0
    assert float(err[zero].max() if bool(zero.any()) else 0.0) == 0.0
    return float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16 if a.dtype == BF else (torch.int32 if a.element_size() == 4 else torch.int64)),
                                                                      b.view(torch.int16 if b.dtype == BF else (torch.int32 if b.element_size() == 4 else torch.int64)))


# ------------------------------------------------------------------------------------------------ 1: exact
@pytest.mark.parametrize("n", [2, 16, 64, 128])
def test_gradient_is_exact_on_exact_operands(n):
    from sea_amd import ops
    from tests.test_field_verify_gpu import run_exact

    for counts in X_COUNTS:
        for wp in (False, True):
            t = exact_case(n, counts, wp, False)
            ref = reference(t, n, False)
            loss, sums, status, (dH,) = run_crps(t, n, False)
            assert ops.last_form()[0] == "decode.member_crps_grad.w8"
            assert not bool(torch.isnan(dH.float()).any()) and not bool(torch.isnan(loss).any()) and not bool(torch.isnan(sums).any())   # fully written
            assert torch.equal(dH.cpu().view(torch.int16), ref["dH_exact"][0].to(torch.float32).to(BF).view(torch.int16)), (n, counts, wp)
            assert torch.equal(ref["dH"][0], ref["dH_exact"][0])                                # the premise: rounding G changed nothing
            v = run_exact(t, n, False, maps=())
            assert same(sums, v["sums"]) and same(loss, v["sums"][..., 1].to(torch.float32)) and torch.equal(status, v["status"])
            assert torch.equal(sums[..., 0].cpu(), ref["count"])
            rows = dH.view(X_B, n, X_P, X_S)
            for p, c in enumerate(counts):
                if c == 0:
                    assert float(rows[:, :, p].float().abs().max()) == 0.0                      # a patch without a valid cell
    # a dead member's rows and an unscored history: exactly 0, whatever the prefill
    t = dict(exact_case(n, X_COUNTS[0], True, False))
    lw = torch.zeros(X_B, n)
    lw[0, 1] = float("-inf")
    lw[1, 0] = float("nan")
    t["logw"] = lw.reshape(-1)
    loss, sums, status, (dH,) = run_crps(t, n, False, fill=7.0)
    rows = dH.view(X_B, n, X_P, X_S).float()
    assert status.tolist() == [n - 1, -1]
    assert float(rows[0, 1].abs().max()) == 0.0 and float(rows[1].abs().max()) == 0.0 and float(rows[0, 0].abs().max()) > 0.0
    assert float(loss[1].abs().max()) == 0.0 and float(sums[1].abs().max()) == 0.0 and float(loss[0].min()) > 0.0


# ------------------------------------------------------------------------------------------------ 2: general
@pytest.mark.parametrize("n", [1, 5, 17, 65])
def test_loss_and_gradient_against_fp64(n):
    """The bound 2^-9 (|dH_ref| + sum |G_ref| |W2|) + 40 * 2^-24 sum |G_ref| |W2| on exact_case's operands with log-weights, for the counts (40, 33) and
    (0, 1), with and without the precision map.  The counts (0, 1) leave patch 1 ONE valid cell: a row's sum then has one term per field and no
    rounding error cancels — the case that needs G as two bf16 terms (one term alone may be 2^-8 off, as may the one rounding of dH)."""
    worst_l, worst_d = 0.0, 0.0
    for counts in X_COUNTS:
        for wp in (False, True):
            t = exact_case(n, counts, wp, True)
            ref = reference(t, n, True)
            loss, sums, status, (dH,) = run_crps(t, n, True)
            # the f32 store of the loss is one more rounding than the fp64 sums carry: the bound is held on sums, the loss is its float32
            sr = float(((sums[..., 1].cpu() - ref["loss"]).abs() / (SUMS_TOL * ref["loss"].abs().clamp_min(1.0))).max())
            assert same(loss, sums[..., 1].to(torch.float32)) and torch.equal(sums[..., 0].cpu(), ref["count"])
            d = dh_ratio(dH, ref["dH_exact"][0], ref["absW"][0])
            print(f"crps loss N = {n} counts {counts} prec {wp}: fp64 sum error / bound {sr:.3e}, dH error / bound {d:.3e}")
            worst_l, worst_d = max(worst_l, sr), max(worst_d, d)
    print(f"crps loss N = {n}: largest error / bound over 4 cases: fp64 sum {worst_l:.3e} (bound {SUMS_TOL:.1e}), dH {worst_d:.3e} (bound 2^-9 (|dH| + sum |G||W2|) + 40 2^-24 sum |G||W2|)")
    assert worst_l <= 1.0 and worst_d <= 1.0, (n, worst_l, worst_d)


# ------------------------------------------------------------------------------------------------ 3: the edges of the launch
@functools.lru_cache(maxsize=None)
def edge_case(n, F, C_, Cp, S, B, P, counts, seed):
    """exact_case's construction for any field count, width and hidden width, with a precision map (a tenth dead, obs NaN there) and field_logw."""
    g = torch.Generator().manual_seed(seed)
    M = B * n * P
    H = torch.zeros(M, S)
    cols = torch.stack([torch.randperm(S, generator=g)[:4] for _ in range(M)])
    H.scatter_(1, cols, torch.randint(0, 2, (M, 4), generator=g).float() * 2 - 1)
    W2 = torch.zeros(F * Cp, S)
    W2.view(F, Cp, S)[:, :C_] = torch.randint(-1, 2, (F, C_, S), generator=g).float()
    bias = torch.zeros(F * Cp)
    bias.view(F, Cp)[:, :C_] = torch.randint(-8, 9, (F, C_), generator=g).float() / 4
    obs = torch.randint(-12, 13, (B * P, F, C_), generator=g).float() / 4
    prec = 0.25 + 1.75 * torch.rand(B * P, F, C_, generator=g)
    miss = torch.rand(B * P, F, C_, generator=g) < 0.1
    prec[miss] = 0.0
    obs[miss] = float("nan")
    Y = (H.double() @ W2.double().t() + bias.double()).view(B * n, P, F, Cp)[..., :C_].contiguous()
    w = prec.view(B, P, F, C_).to(F64)
    w = torch.where((torch.arange(C_) < torch.tensor(counts)[:, None]).view(1, P, 1, C_), w, torch.zeros((), dtype=F64))
    return dict(H=H, W2=W2, bias=bias, obs=obs, prec=prec, logw=field_logw(n, B, seed + 1), counts=torch.tensor(counts, dtype=torch.int32), C=C_, Cp=Cp, Y=Y, w=w)


def check_edge(t, n, groups, P, tag, Z=None, fw=None, form=None):
    from sea_amd import ops

    ref = reference(t, n, True, groups=groups, fw=fw, Z=Z)
    loss, sums, status, dH = run_crps(t, n, True, groups=groups, P=P, fw=fw, Z=Z)
    if form is not None:
        assert ops.last_form()[0] == form, ops.last_form()
    scale = 1.0 if fw is None else fw.to(F64).view(1, -1)
    sr = float(((scale * sums[..., 1].cpu() - ref["loss"]).abs() / (SUMS_TOL * ref["loss"].abs().clamp_min(1.0))).max())
    assert torch.equal(sums[..., 0].cpu(), ref["count"])
    worst = 0.0
    for g in range(len(groups)):
        assert not bool(torch.isnan(dH[g].float()).any()), tag
        worst = max(worst, dh_ratio(dH[g], ref["dH_exact"][g], ref["absW"][g]))
    print(f"crps loss edge {tag}: fp64 sum error / bound {sr:.3e}, dH error / bound {worst:.3e}")
    assert sr <= 1.0 and worst <= 1.0, (tag, sr, worst)
    return loss, sums, status, dH


def test_two_groups_add_their_own_fields_only():
    """[[0, 1], [2]]: the fields of one group add into its dH, the third does not leak; a field weight of 0 silences a field exactly."""
    n, F, P = 5, 3, 2
    t = edge_case(n, F, 40, 64, 40, 2, P, (40, 33), 5100)
    check_edge(t, n, ((0, 2), (2, 1)), P, "two groups")
    fw = torch.tensor([1.0, 0.0, 0.5])
    loss, _, _, dH = check_edge(t, n, ((0, 2), (2, 1)), P, "two groups, field weights 1, 0, 0.5", fw=fw)
    assert float(loss[:, 1].abs().max()) == 0.0
    # group 0 with field 1 silenced is field 0 alone
    t0 = dict(t, W2=t["W2"][:64], bias=t["bias"][:64], obs=t["obs"][:, :1], prec=t["prec"][:, :1])
    solo = run_crps(t0, n, True, groups=((0, 1),), P=P)
    assert same(solo[3][0], dH[0])


def test_a_field_wider_than_one_chunk_of_tiles():
    """530 columns in 544 are 17 tiles, two chunks: the finish launch adds the chunks' partials in order; counts 512 leave the second chunk nothing.  Patch 1 of (512, 1) has ONE valid cell."""
    n, C_, Cp = 5, 530, 544
    for counts in ((C_, 513), (512, 1)):
        t = exact_case(n, counts, True, True, C_, Cp)
        ref = reference(t, n, True)
        loss, sums, status, (dH,) = run_crps(t, n, True)
        sr = float(((sums[..., 1].cpu() - ref["loss"]).abs() / (SUMS_TOL * ref["loss"].abs().clamp_min(1.0))).max())
        # the issue holds this case to the general bounds with 40 accumulated terms; the field has 530
        d = dh_ratio(dH, ref["dH_exact"][0], ref["absW"][0])
        print(f"crps loss wide field counts {counts}: fp64 sum error / bound {sr:.3e}, dH error / bound {d:.3e}")
        assert sr <= 1.0 and d <= 1.0, (counts, sr, d)


@pytest.mark.parametrize("n,S,form", [(5, 264, "decode.member_crps_grad.w8"), (128, 384, "decode.member_crps_grad.w8"), (64, 640, "decode.member_crps_grad.w4"),
                                      (17, 512, "decode.member_crps_grad.w4")])
def test_wide_hidden_rows(n, S, form):
    """S = 264 (padded to 384 by masking), the widest form at 128 members (384), and the 4-wave forms above it up to 64 members."""
    from sea_amd import ops

    B, P = (2, 2) if n <= 17 else (1, 1)
    t = edge_case(n, 2, 40, 64, S, B, P, (40, 33)[:P], 5200 + S)
    check_edge(t, n, ((0, 2),), P, f"N = {n}, S = {S}", form=form)
    assert ops.last_form()[1] == (S + 127) // 128 * 128


def test_unsupported_shape_is_refused_by_the_library():
    t = edge_case(65, 1, 40, 64, 392, 1, 1, (40,), 5300)
    with pytest.raises(RuntimeError, match="members=65 above 64 at hidden width S=392"):
        run_crps(t, 65, True, groups=((0, 1),), P=1)


def test_gelu_grad_of_the_pre_activation():
    n, P = 17, 2
    t = edge_case(n, 2, 40, 64, 40, 2, P, (40, 33), 5400)
    Z = torch.randint(-12, 13, tuple(t["H"].shape), generator=torch.Generator().manual_seed(5401)).float() / 4
    check_edge(t, n, ((0, 2),), P, "gelu'(Z)", Z=Z)


# ------------------------------------------------------------------------------------------------ 4: reproducibility
@pytest.mark.parametrize("n", [5, 128])
def test_two_runs_and_a_history_alone_give_the_same_bits(n):
    t = exact_case(n, X_COUNTS[0], True, True)
    a = run_crps(t, n, True)
    b = run_crps(t, n, True, fill=3.0)
    assert same(a[0], b[0]) and same(a[1], b[1]) and torch.equal(a[2], b[2]) and same(a[3][0], b[3][0])
    alone = run_crps(t, n, True, hist=1)
    rows = n * X_P
    assert same(alone[0][0], a[0][1]) and same(alone[1][0], a[1][1]) and int(alone[2][0]) == int(a[2][1]) and same(alone[3][0], a[3][0][rows:2 * rows])


# ------------------------------------------------------------------------------------------------ 5: autograd
def decode64(c, z):
    """The decoder of case c in fp64 (exact GELU) on z [Bm, P, G, D] -> [Bm, P, F, C]."""
    out = []
    for g, grp in enumerate(c["groups"]):
        pre = z[:, :, g] @ c["w1"][g].to(F64).t()
        Hh = 0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0)))
        out.append((Hh @ c["w2"][g].to(F64).t() + c["b2"][g].to(F64)).view(z.shape[0], z.shape[1], len(grp), c["n_inp"]))
    return torch.cat(out, dim=2)


@functools.lru_cache(maxsize=None)
def autograd_case():
    c = case("a")
    B, n, P = 2, 4, 3
    G, D, C_ = len(c["groups"]), c["D"], c["n_inp"]
    F = sum(len(g) for g in c["groups"])
    g = torch.Generator().manual_seed(5500)
    z = torch.randn(B * n, P, G, D, generator=g)
    z64 = z.to(F64).requires_grad_(True)
    Y = decode64(c, z64)
    obs = (Y.detach().view(B, n, P, F, C_).mean(1) + 0.5 * torch.randn(B, P, F, C_, generator=g, dtype=F64)).to(torch.float32)
    prec = 0.25 + 1.75 * torch.rand(B, P, F, C_, generator=g)
    prec[torch.rand(B, P, F, C_, generator=g) < 0.1] = 0.0
    counts = [C_, max(C_ - 5, 1), 0]
    logw = field_logw(n, B, 5501)
    w = torch.where((torch.arange(C_) < torch.tensor(counts)[:, None]).view(1, P, 1, C_), prec.to(torch.float32), torch.zeros(())).to(F64)
    r = restate_crps_grad(Y.detach(), obs, w, logw, n, True)
    (dz,) = torch.autograd.grad(Y, z64, r["G"])
    return dict(z=z, obs=obs, prec=prec, counts=counts, logw=logw, loss=r["loss"], count=r["count"], dz=dz, B=B, n=n, P=P, F=F, G=G)


def loss_and_grad(dec, k, fused, upstream=None, **kw):
    z = k["z"].to(DEV).requires_grad_(True)
    loss, count = dec.member_crps_loss(z, k["obs"].to(DEV), k["n"], counts=k["counts"], precision=k["prec"].to(DEV), logw=k["logw"].to(DEV), unbiased=True, fused=fused, **kw)
    assert loss.shape == (k["B"], k["F"]) and loss.dtype == torch.float32 and loss.requires_grad and not count.requires_grad
    (loss.sum() if upstream is None else (loss * upstream).sum()).backward()
    return loss.detach(), count.detach(), z.grad.detach()


def test_member_crps_loss_against_fp64():
    k = autograd_case()
    dec = decoder("a", "bf16")
    lf, cf, gf = loss_and_grad(dec, k, True)
    lc, cc, gc = loss_and_grad(dec, k, False)
    e, e_c = rel(gf.cpu(), k["dz"]), rel(gc.cpu(), k["dz"])
    el, el_c = rel(lf.cpu(), k["loss"]), rel(lc.cpu(), k["loss"])
    print(f"crps loss end to end (shape a, 2 histories x 4 members x 3 patches): z.grad fused {e:.3e} composed {e_c:.3e}; loss fused {el:.3e} composed {el_c:.3e}")
    assert torch.equal(cf.cpu(), k["count"]) and torch.equal(cc.cpu(), k["count"])
    assert e <= 2 * e_c + 1e-6 and el <= 2 * el_c + 1e-6
    # under no_grad: member_verify without maps, the same loss bits
    with torch.no_grad():
        ln, cn = dec.member_crps_loss(k["z"].to(DEV), k["obs"].to(DEV), k["n"], counts=k["counts"], precision=k["prec"].to(DEV), logw=k["logw"].to(DEV), fused=True)
    assert same(ln, lf) and torch.equal(cn, cf) and not ln.requires_grad
    lz, _ = dec.member_crps_loss(k["z"].to(DEV), k["obs"].to(DEV), k["n"], counts=k["counts"], precision=k["prec"].to(DEV), logw=k["logw"].to(DEV), fused=True)
    assert same(lz, lf) and not lz.requires_grad                                                # z without grad


def test_upstream_gradients_scale_per_history_and_group():
    k = autograd_case()
    c = case("a")
    dec = decoder("a", "bf16")
    sizes = [len(g) for g in c["groups"]]
    _, _, g1 = loss_and_grad(dec, k, True)
    per_group = torch.tensor([[0.5 + b + 2.0 * g for g in range(len(sizes))] for b in range(k["B"])])          # [B, G]
    up = torch.cat([per_group[:, g:g + 1].expand(k["B"], s) for g, s in enumerate(sizes)], dim=1).contiguous().to(DEV)
    _, _, g2 = loss_and_grad(dec, k, True, upstream=up)
    want = g1.view(k["B"], k["n"], k["P"], k["G"], -1) * per_group.to(DEV).view(k["B"], 1, 1, k["G"], 1)
    assert torch.equal(g2.view_as(want), want.to(g2.dtype))
    # a factor that differs inside a group: NaN in that history's group slice only
    gi = next(i for i, s in enumerate(sizes) if s >= 2)
    off = sum(sizes[:gi])
    bad = up.clone()
    bad[1, off + 1] += 1.0
    _, _, g3 = loss_and_grad(dec, k, True, upstream=bad)
    g3v = g3.view_as(want)
    assert bool(torch.isnan(g3v[1, :, :, gi]).all())
    mask = torch.ones_like(g3v, dtype=torch.bool)
    mask[1, :, :, gi] = False
    assert torch.equal(g3v[mask], g2.view_as(want)[mask])
    # the composed path carries per-field upstream gradients exactly: no NaN
    _, _, g4 = loss_and_grad(dec, k, False, upstream=bad)
    assert bool(torch.isfinite(g4).all())


def test_identical_members_reduce_to_the_mean_absolute_error():
    """unbiased=False and equal members: the pair term vanishes, CRPS = mean |y - obs|, and the members' gradients add up to the gradient of that mean
    absolute error through the decoder (the sign of the error in front of W2)."""
    k = autograd_case()
    dec = decoder("a", "bf16")
    n, P = k["n"], k["P"]
    z1 = k["z"][:1].to(DEV)
    zrep = z1.expand(n, -1, -1, -1).contiguous().requires_grad_(True)
    obs = k["obs"][:1].to(DEV)
    loss, count = dec.member_crps_loss(zrep, obs, n, unbiased=False, fused=True)
    loss.sum().backward()
    zs = z1.clone().requires_grad_(True)
    y = dec(zs)
    mae = (y - obs).abs().sum()
    mae.backward()
    assert float(count.sum()) == obs.numel()
    assert abs(float(loss.sum()) - float(mae)) <= 1e-4 * float(mae)
    summed = zrep.grad.sum(0, keepdim=True)
    cos = float((summed * zs.grad).sum() / (summed.norm() * zs.grad.norm()))
    print(f"crps loss identical members: loss {float(loss.sum()):.6f} mean absolute error sum {float(mae):.6f}; cosine of the summed z.grad to the MAE gradient {cos:.6f}, "
          f"relative difference {rel(summed.cpu(), zs.grad.cpu()):.3e}")
    assert rel(summed.cpu(), zs.grad.cpu()) <= TOL_BF16


# ------------------------------------------------------------------------------------------------ 6: through the model
def test_ensemble_crps_loss_trains_the_temporal_model():
    from oracle.recipe import recipe_inputs
    from sea_amd.utils.train_utils import EnsembleCRPSLoss
    from tests.test_input_grad_gpu import cfg_of
    from tests.test_model_gpu import build, gpu

    c = case("a")
    P, D, G = 4, c["D"], len(c["groups"])
    F = sum(len(g) for g in c["groups"])
    cfg = cfg_of(1, P * D, 4, G)
    B, n, T = 1, 4, 3
    x, _, ib = recipe_inputs(B * n, T, cfg, seed=9)                                                # four trajectories: the members of one history
    fields = torch.randn(B, T, P, F, c["n_inp"], generator=torch.Generator().manual_seed(4)).to(DEV)
    counts = [12, 0, 7, 11]

    def grads(fused, dtype="bf16"):
        m = build(cfg, "fp32").train()
        loss = EnsembleCRPSLoss(decoder("a", dtype), P, n, counts=counts, fused=fused)(m(gpu(x), gpu(ib)), fields)
        assert loss.dim() == 0 and loss.dtype == torch.float32
        loss.backward()
        return loss.item(), {k: p.grad.detach().cpu() for k, p in m.named_parameters() if p.grad is not None}

    # the reference: the same fp32 model with the fp32 decoder on the composed path (fp64 formulas on fp32-decoded fields); e and e_c are the distances of
    # the two bf16-decoder runs from it, per parameter tensor — the project's rule, as test_member_crps_loss_against_fp64 holds it for z.grad
    l_ref, g_ref = grads(False, "fp32")
    l_fused, g_fused = grads(True)
    l_comp, g_comp = grads(False)
    assert all(bool(torch.isfinite(g).all()) for g in g_fused.values())
    live = [k for k, g in g_ref.items() if float(g.norm()) > 0.0]   # some parameters never receive a gradient
    assert len(live) >= 10
    e = {k: rel(g_fused[k], g_ref[k]) for k in live}
    e_c = {k: rel(g_comp[k], g_ref[k]) for k in live}
    worst = max(live, key=lambda k: e[k] / (2 * e_c[k] + 1e-6))
    print(f"ensemble crps loss end to end: loss fp32 {l_ref:.6f} fused {l_fused:.6f} composed {l_comp:.6f}; parameter gradients against the fp32-decoder run over {len(live)} "
          f"tensors: fused largest {max(e.values()):.3e}, composed largest {max(e_c.values()):.3e}, largest e / (2 e_c + 1e-6) {e[worst] / (2 * e_c[worst] + 1e-6):.3f} "
          f"(e {e[worst]:.3e}, e_c {e_c[worst]:.3e}, {worst})")
    assert abs(l_fused - l_ref) <= 2 * abs(l_comp - l_ref) + 1e-6
    for k in live:
        assert e[k] <= 2 * e_c[k] + 1e-6, (k, e[k], e_c[k])
