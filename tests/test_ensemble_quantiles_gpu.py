"""Quantile and exceedance-probability maps of an ensemble on the device: sea_decode_member_quantiles through ops.decode_member_quantiles,
Decode.member_quantiles and EnsembleQuantiles end to end and on a rollout session.

Reference: `restate_quantiles` of tests/test_ensemble_quantiles_cpu.py — the fp64 restatement from the definitions, below_i accumulated over j ascending.
  kernel      on EXACT operands (tests/test_field_verify_gpu.py's exact_case: decoded values are exact multiples of 0.25, ties occur): quant EQUAL BITS —
              the restatement sees the same f32 values and weights and adds in the same order, so every decision cum_i >= tau W has the same fp64
              operands (the test also checks that no decision is nearer than 1e-12 W to flipping without being an exact tie); exceed within
              1e-6 max(1, max |ref|) — tests/test_verify_gpu.py's bound for an fp64 result stored as f32.
  end to end  bf16 fused: e <= 2 e_c + 1e-6 for the quantile maps (e: against the restatement on fp64-decoded values; e_c: the composed path on the same
              inputs — the project's rule; it applies because an order statistic with fixed weights is 1-Lipschitz in the members' values); fused against
              composed <= 1e-4.  Exceedance is discontinuous in the values and is compared on the same values only."""
import functools

import pytest
import torch

from tests.test_decode_loss_cpu import rel
from tests.test_decode_loss_gpu import DEV, case, decoder
from tests.test_ensemble_quantiles_cpu import restate_quantiles
from tests.test_field_enkf_cpu import field_case, field_cases
from tests.test_field_verify_cpu import field_logw
from tests.test_field_verify_gpu import X_B, X_C, X_COUNTS, X_CP, X_F, X_MEMBERS, X_P, decode_exact, dev, exact_case, run_exact
from tests.test_verify_cpu import close

pytestmark = pytest.mark.gpu

F64 = torch.float64
LEVELS = (0.0, 0.1, 0.5, 0.9, 1.0)
THR = torch.tensor([[-1.0, 0.25], [0.5, 0.5]])


def weights_of(n, B=X_B):
    """float32 weights [B * n] with a dominant member and, from two members on, a dead one (field_logw through normalised_weights)."""
    from sea_amd.ensemble import normalised_weights

    return normalised_weights(field_logw(n, B, 900 + n), n)


def dead_rows_nan(H, w, n, P=X_P):
    """H with the hidden rows of every dead member NaN: they reach nothing."""
    H = H.clone()
    for m in range(w.numel()):
        if not float(w[m]) > 0:
            H[m * P:(m + 1) * P] = float("nan")
    return H


def members_first(Y, n):
    """[B * n, P, F, C] float64 exact values -> float32 [B, n, P, F, C]: what the launch compares."""
    return Y.view(-1, n, *Y.shape[1:]).to(torch.float32)


def masked(t, counts, C_):
    """The restatement's maps with the invalid columns 0."""
    valid = (torch.arange(C_) < torch.tensor(counts)[:, None]).view(1, 1, len(counts), 1, C_)
    return None if t is None else torch.where(valid, t, torch.zeros((), dtype=t.dtype))


def run(t, n, levels=LEVELS, thr=THR, w=None, H=None, hist=None, out=None):
    """ops.decode_member_quantiles on an exact case (hist: that history alone)."""
    from sea_amd import ops

    P = X_P
    H = t["H"] if H is None else H
    if hist is not None:
        H = H[hist * n * P:(hist + 1) * n * P]
        w = None if w is None else w[hist * n:(hist + 1) * n]
    grp = [dict(H=H.to(DEV).to(torch.bfloat16), W2=t["W2"].to(DEV).to(torch.bfloat16), bias=t["bias"].to(DEV))]
    return ops.decode_member_quantiles(grp, t["C"], t["Cp"], P, n, levels=levels, thr=dev(thr), w=dev(w), counts=t["counts"].to(DEV), out=out)


def prefilled(B, width, levels=LEVELS, thr=THR):
    return dict(quant=torch.full((len(levels), B, X_P, X_F, width), float("nan"), device=DEV), exceed=torch.full((thr.shape[0], B, X_P, X_F, width), float("nan"), device=DEV))


def check_exact(got, t, n, w, counts, C_, tag, H=None):
    """quant equal bits, exceed within the bound, pad and invalid columns exactly 0; returns exceed's error / bound."""
    Y = t["Y"] if H is None else decode_exact(H, t["W2"], t["bias"], None, counts, n, C_, t["Cp"])["Y"]
    ref = restate_quantiles(members_first(Y, n), None if w is None else w.view(X_B, n), LEVELS, THR)
    assert ref["margin"] > 1e-12, tag + (ref["margin"],)                    # decided: bit equality does not rest on luck
    q, e = got["quant"].cpu(), got["exceed"].cpu()
    assert not bool(torch.isnan(q).any()) and not bool(torch.isnan(e).any()), tag   # every element was written
    assert float(q[..., C_:].abs().max() if q.shape[-1] > C_ else 0.0) == 0.0 and float(e[..., C_:].abs().max() if e.shape[-1] > C_ else 0.0) == 0.0, tag
    assert torch.equal(q[..., :C_], masked(ref["quant"], counts, C_)), tag
    ok, ratio = close(e[..., :C_], masked(ref["exceed"], counts, C_), 1e-6)
    assert ok, tag + (ratio,)
    return ratio


# ------------------------------------------------------------------------------------------------ 1: the kernel on exact operands
@pytest.mark.parametrize("n", X_MEMBERS)
def test_kernel_against_fp64_on_exact_operands(n):
    from sea_amd import ops

    worst, cases = 0.0, 0
    for counts in X_COUNTS:
        t = exact_case(n, counts, False, False)
        for w in (None, weights_of(n)):
            H = None if w is None else dead_rows_nan(t["H"], w, n)
            out = prefilled(X_B, X_C + 5)
            got = run(t, n, w=w, H=H, out=out)
            assert ops.last_form()[0] == "decode.member_quantiles" and all(got[k].data_ptr() == out[k].data_ptr() for k in out)
            worst, cases = max(worst, check_exact(got, t, n, w, counts, X_C, (n, counts, w is None), H=H)), cases + 1
    print(f"ensemble quantiles N = {n}: quant equal bits; exceed largest error / bound over {cases} cases {worst:.3e} (bound 1e-6)")


# ------------------------------------------------------------------------------------------------ 2: the same values as the verify launch
@functools.lru_cache(maxsize=None)
def random_case(S, n=3, B=2, P=1, F=2, C_=X_C, Cp=X_CP):
    """bf16-exact random operands: dict(H [B n P, S], W2 [F Cp, S], bias, Y float64 [B, n, P, F, C] decoded in fp64)."""
    g = torch.Generator().manual_seed(7000 + S + n)
    H = torch.randn(B * n * P, S, generator=g).to(torch.bfloat16).float()
    W2 = torch.zeros(F * Cp, S)
    W2.view(F, Cp, S)[:, :C_] = (torch.randn(F, C_, S, generator=g) * (2.0 / S ** 0.5)).to(torch.bfloat16).float()
    bias = torch.zeros(F * Cp)
    bias.view(F, Cp)[:, :C_] = torch.randn(F, C_, generator=g) * 0.1
    Y = (H.double() @ W2.double().t() + bias.double()).view(B, n, P, F, Cp)[..., :C_].contiguous()
    return dict(H=H, W2=W2, bias=bias, Y=Y, n=n, B=B, P=P, F=F, C=C_, Cp=Cp)


def groups_of(t):
    return [dict(H=t["H"].to(DEV).to(torch.bfloat16), W2=t["W2"].to(DEV).to(torch.bfloat16), bias=t["bias"].to(DEV))]


def test_one_member_has_the_bits_of_the_verify_launch():
    from sea_amd import ops

    t = exact_case(1, X_COUNTS[0], False, False)
    got = run(t, 1)
    mean = run_exact(t, 1, True, maps=("mean",))["mean"]
    for k in range(len(LEVELS)):
        assert torch.equal(got["quant"][k], mean), k
    for S in (40, 640):                                                    # random operands: the order of the fp32 sums shows in the bits
        r = random_case(S, n=1)
        q = ops.decode_member_quantiles(groups_of(r), r["C"], r["Cp"], r["P"], 1, levels=(0.0, 0.3, 1.0))["quant"]
        obs = torch.zeros(r["B"] * r["P"], r["F"], r["C"], device=DEV)
        mean = ops.decode_member_verify(groups_of(r), obs, r["C"], r["Cp"], r["P"], 1, maps=("mean",))["mean"]
        assert all(torch.equal(q[k], mean) for k in range(3)), S
        assert rel(mean.cpu().double(), r["Y"][:, 0]) <= 1e-5


@pytest.mark.parametrize("n", [2, 17, 64, 128])
def test_exceedance_is_one_minus_the_pit_of_the_verify_launch(n):
    from sea_amd import ops

    t = exact_case(n, X_COUNTS[0], False, True)
    lw = t["logw"]
    w = weights_of(n)                                                      # field_logw(n, B, 900 + n): the case's own log-weights, normalised
    got = run(t, n, levels=(), w=w)["exceed"]
    assert run(t, n, levels=(), w=w)["quant"] is None
    Y = t["Y"].view(X_B, n, X_P, X_F, X_C)
    live = (w > 0).view(X_B, n, 1, 1, 1)
    worst = 0.0
    for k in range(THR.shape[0]):
        obs = THR[k].view(1, X_F, 1).expand(X_B * X_P, X_F, X_C).contiguous().to(DEV)
        pit = ops.decode_member_verify(groups_of(dict(H=t["H"], W2=t["W2"], bias=t["bias"])), obs, X_C, X_CP, X_P, n, counts=t["counts"].to(DEV), logw=dev(lw),
                                       maps=("pit",))["pit"]
        tie = (live & (Y == THR[k].view(1, 1, 1, X_F, 1).double())).any(1)
        valid = (torch.arange(X_C) < t["counts"][:, None]).view(1, X_P, 1, X_C).expand_as(tie)
        on = valid & ~tie
        assert bool(on.any())
        err = float((got[k].cpu()[on].double() - (1.0 - pit.cpu()[on].double())).abs().max())
        worst = max(worst, err)
        assert err <= 2e-6, (n, k, err)
    print(f"ensemble quantiles N = {n}: exceed against 1 - pit of the verify launch, largest difference {worst:.3e} (bound 2e-6)")


# ------------------------------------------------------------------------------------------------ 3: chunk and tile edges
def test_a_field_wider_than_one_chunk_of_tiles():
    """530 columns in 544 are 17 tiles: a workgroup reads out 16, so a field has two chunks; counts 513 leave the second chunk ONE valid column, counts
    512 none (it leaves at once)."""
    n, C_, Cp = 5, 530, 544
    w = weights_of(n)
    for counts in ((C_, 513), (512, 513)):
        t = exact_case(n, counts, False, False, C_, Cp)
        H = dead_rows_nan(t["H"], w, n)
        got = run(t, n, w=w, H=H, out=prefilled(X_B, C_ + 3))
        ratio = check_exact(got, t, n, w, counts, C_, (counts,), H=H)
        again = run(t, n, w=w, H=H)
        assert torch.equal(again["quant"], got["quant"][..., :C_]) and torch.equal(again["exceed"], got["exceed"][..., :C_])
        alone = run(t, n, w=w, H=H, hist=1)
        assert torch.equal(alone["quant"][:, 0], again["quant"][:, 1]) and torch.equal(alone["exceed"][:, 0], again["exceed"][:, 1])
        print(f"ensemble quantiles chunks counts {counts}: quant equal bits; exceed error / bound {ratio:.3e}")


# ------------------------------------------------------------------------------------------------ 4: every hidden-width form
@pytest.mark.parametrize("S", [128, 256, 384, 512, 640])
def test_every_hidden_width_form(S):
    """Each SP the dispatcher instantiates at its widest S, M = 2 * 3 * 1 rows, random bf16-exact operands.  e: the relative L2 error of the quantile
    maps against the restatement on fp64-decoded values; e_c: that of the composed counterpart — the same operands decoded by an fp32 matrix product on
    the host, then _composed_quantiles.  Both round fp32 sums of exact products and differ in their order: e <= 2 e_c + 1e-6."""
    from sea_amd import ops
    from sea_amd.ensemble import _composed_quantiles

    r = random_case(S)
    n, B = r["n"], r["B"]
    w = torch.tensor([0.5, 0.2, 0.3, 0.25, 0.0, 0.75])
    levels = (0.0, 0.4, 0.6, 1.0)
    thr = torch.tensor([[0.0, 0.1]])
    ref = restate_quantiles(r["Y"], w.view(B, n), levels, thr)
    out = dict(quant=torch.full((4, B, r["P"], r["F"], r["C"]), float("nan"), device=DEV), exceed=torch.full((1, B, r["P"], r["F"], r["C"]), float("nan"), device=DEV))
    got = ops.decode_member_quantiles(groups_of(r), r["C"], r["Cp"], r["P"], n, levels=levels, thr=thr.to(DEV), w=w.to(DEV), out=out)
    assert ops.last_form()[:2] == ("decode.member_quantiles", S)
    Yc = (r["H"] @ r["W2"].t() + r["bias"]).view(B, n, r["P"], r["F"], r["Cp"])[..., :r["C"]]
    qc, ec = _composed_quantiles(Yc, w.view(B, n), levels, thr)
    e, e_c = rel(got["quant"].cpu().double(), ref["quant"]), rel(qc.double(), ref["quant"])
    print(f"ensemble quantiles form SP = {S}: quant e {e:.3e} e_c {e_c:.3e}; exceed max difference {float((got['exceed'].cpu().double() - ref['exceed']).abs().max()):.3e}")
    assert e <= 2 * e_c + 1e-6, (S, e, e_c)
    # exceedance on the same values: away from cells where a member is within 1e-4 of the threshold, the indicator sums are the same
    near = ((r["Y"] - thr[0].view(1, 1, 1, r["F"], 1).double()).abs() < 1e-4).any(1)
    ok, ratio = close(got["exceed"].cpu()[0][~near], ref["exceed"][0][~near], 1e-6)
    assert ok, (S, ratio)


# ------------------------------------------------------------------------------------------------ 5: determinism and isolation
@pytest.mark.parametrize("n", [5, 64, 128])
def test_bits_histories_nan_rows_and_single_products(n):
    t = exact_case(n, X_COUNTS[0], False, False)
    w = weights_of(n)
    want = run(t, n, w=w)
    again = run(t, n, w=w)
    assert torch.equal(again["quant"], want["quant"]) and torch.equal(again["exceed"], want["exceed"])          # two runs, the same bits
    for h in range(X_B):                                                   # a history alone reproduces its slice
        alone = run(t, n, w=w, hist=h)
        assert torch.equal(alone["quant"][:, 0], want["quant"][:, h]) and torch.equal(alone["exceed"][:, 0], want["exceed"][:, h]), (n, h)
    only_t, only_q = run(t, n, levels=(), w=w), run(t, n, thr=None, w=w)   # a thresholds-only and a levels-only call
    assert only_t["quant"] is None and only_q["exceed"] is None
    assert torch.equal(only_t["exceed"], want["exceed"]) and torch.equal(only_q["quant"], want["quant"])
    j, p = (1 + 2) % n, 1                                                  # history 1: member 1 leads, member 2 is dead, member 3 is live
    assert float(w[n + j]) > 0
    H = t["H"].clone()
    H[(n + j) * X_P + p] = float("nan")
    got = run(t, n, w=w, H=H)
    for k in ("quant", "exceed"):
        nan = torch.isnan(got[k].cpu())
        mark = torch.zeros_like(nan)
        mark[:, 1, p, :, :int(t["counts"][p])] = True
        assert torch.equal(nan, mark), (n, k)                              # exactly the cells of that (history, patch)
        assert torch.equal(got[k].cpu()[~mark], want[k].cpu()[~mark]), (n, k)


# ------------------------------------------------------------------------------------------------ 6: refusals
def test_refusals_leave_the_process_usable():
    from sea_amd import ops

    t = exact_case(5, X_COUNTS[0], False, False)
    grp = groups_of(dict(H=t["H"], W2=t["W2"], bias=t["bias"]))
    before = run(t, 5)
    with pytest.raises(ValueError, match="bf16 only"):
        ops.decode_member_quantiles([dict(H=grp[0]["H"].float(), W2=grp[0]["W2"].float(), bias=grp[0]["bias"])], X_C, X_CP, X_P, 5, levels=(0.5,), dtype=torch.float32)
    with pytest.raises(ValueError, match="bf16 only"):
        ops.decode_member_quantiles([dict(H=grp[0]["H"].float(), W2=grp[0]["W2"].float(), bias=grp[0]["bias"])], X_C, X_CP, X_P, 5, levels=(0.5,))
    big = torch.zeros(X_B * 129 * X_P, 40, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="members = 129"):
        ops.decode_member_quantiles([dict(grp[0], H=big)], X_C, X_CP, X_P, 129, levels=(0.5,))
    wide = dict(H=torch.zeros(20, 648, device=DEV, dtype=torch.bfloat16), W2=torch.zeros(X_F * X_CP, 648, device=DEV, dtype=torch.bfloat16), bias=grp[0]["bias"])
    with pytest.raises(ValueError, match="up to 640"):
        ops.decode_member_quantiles([wide], X_C, X_CP, X_P, 5, levels=(0.5,))
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        ops.decode_member_quantiles(grp, X_C, X_CP, X_P, 5, levels=(0.5, 1.5))
    assert ops.last_form()[0] == "decode.member_quantiles"                  # nothing else was launched in between
    after = run(t, 5)
    assert torch.equal(after["quant"], before["quant"]) and torch.equal(after["exceed"], before["exceed"])


# ------------------------------------------------------------------------------------------------ 7: end to end
CASES = [c for c in field_cases() if not c[4]]                              # without a precision map: the maps do not read one
BY_SHAPE = {name: [c for c in CASES if c[0] == name] for name in ("a", "b", "c")}
E2E_LEVELS = (0.05, 0.5, 0.95)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_quantiles_bf16_against_fp64(name):
    from sea_amd.ensemble import EnsembleQuantiles, normalised_weights

    worst = {}
    P = case(name)["P"]
    for case_ in BY_SHAPE[name]:
        _, members, hist, cnt, wp, local = case_
        k = field_case(*case_)
        logw = torch.randn(hist * members, generator=torch.Generator().manual_seed(66 + members + hist)) if members % 2 else None
        w = None if logw is None else normalised_weights(logw, members).view(hist, members)
        F, C_ = k["obs"].shape[2:]
        ref = restate_quantiles(k["Y"].view(hist, members, P, F, C_), w, E2E_LEVELS, None)["quant"]
        if k["counts"] is not None:
            ref = masked(ref, k["counts"], C_)
        thr = torch.zeros(2, F)
        y, lw = k["y"].to(DEV), dev(logw)
        q, e_map = EnsembleQuantiles(decoder(name, "bf16"), P, members, levels=E2E_LEVELS, thresholds=thr, counts=k["counts"], fused=True)(y, lw)
        q_c, e_map_c = EnsembleQuantiles(decoder(name, "bf16"), P, members, levels=E2E_LEVELS, thresholds=thr, counts=k["counts"], fused=False)(y, lw)
        assert q.dtype == torch.float32 and q.shape == (3, hist, P, F, C_) and e_map.shape == (2, hist, P, F, C_) and q_c.shape == q.shape and e_map_c.shape == e_map.shape
        assert bool((q[1:] >= q[:-1]).all()) and float(e_map.min()) >= 0.0 and float(e_map.max()) <= 1.0 + 1e-6
        if k["counts"] is not None:
            dead = ~(torch.arange(C_) < torch.tensor(k["counts"])[:, None]).view(1, 1, P, 1, C_).expand(3, hist, P, F, C_)
            assert float(q.cpu()[dead].abs().max() if bool(dead.any()) else 0.0) == 0.0 and float(q_c.cpu()[dead].abs().max() if bool(dead.any()) else 0.0) == 0.0
        if float(ref.abs().max()) == 0.0:
            assert float(q.abs().max()) == 0.0
            continue
        e, e_c, fc = rel(q.cpu().double(), ref), rel(q_c.cpu().double(), ref), rel(q.cpu(), q_c.cpu())
        print(f"ensemble quantiles {name} members {members} x {hist} counts {cnt}: fused {e:.3e} composed {e_c:.3e} fused vs composed {fc:.3e}")
        assert e <= 2 * e_c + 1e-6, (members, hist, cnt, e, e_c)
        assert fc <= 1e-4, (members, hist, cnt, fc)
        worst["e"], worst["fc"] = max(worst.get("e", 0.0), e), max(worst.get("fc", 0.0), fc)
    print(f"ensemble quantiles shape {name} worst: " + " ".join(f"{q_} {v:.3e}" for q_, v in worst.items()))


def test_default_rule_and_layout():
    """fused=None: the fused launch in bf16 up to 128 members from 4096 decoder rows on, the composed path below, in fp32 and above 128 members;
    layout="BPCF" returns permuted views of the same maps."""
    from sea_amd import ops
    from sea_amd.ensemble import EnsembleQuantiles

    c = case("a")
    P, G, D_, F, C_ = 64, len(c["groups"]), c["D"], sum(len(g) for g in c["groups"]), c["n_inp"]
    dec = decoder("a", "bf16")
    g = torch.Generator().manual_seed(4)
    for members, fused in ((64, True), (32, False)):
        y = torch.randn(members, G, P * D_, generator=g).to(DEV).to(torch.bfloat16)
        q, e = EnsembleQuantiles(dec, P, members, levels=(0.5,))(y)
        assert (ops.last_form()[0] == "decode.member_quantiles") is fused
        assert e is None and q.shape == (1, 1, P, F, C_)
        q2, _ = EnsembleQuantiles(dec, P, members, levels=(0.5,), fused=not fused)(y)
        assert rel(q.cpu(), q2.cpu()) <= 1e-4
        qt, _ = EnsembleQuantiles(dec, P, members, levels=(0.5,), layout="BPCF", fused=fused)(y)
        assert qt.shape == (1, 1, P, C_, F) and torch.equal(qt.permute(0, 1, 2, 4, 3), q)
    with pytest.raises(ValueError, match="bf16 only"):
        decoder("a", "fp32").member_quantiles(torch.zeros(2, P, G, D_, device=DEV), 2, levels=(0.5,), fused=True)
    q32, _ = EnsembleQuantiles(decoder("a", "fp32"), P, 64, levels=(0.5,))(torch.randn(64, G, P * D_, generator=g).to(DEV))       # fp32: the composed path
    assert q32.shape == (1, 1, P, F, C_)


# ------------------------------------------------------------------------------------------------ 8: on a rollout session
def test_quantiles_on_a_rollout_session():
    """open_rollout -> fork(n) -> step -> EnsembleQuantiles(levels=(0, 0.5, 1)): q_0 <= q_0.5 <= q_1 everywhere, EnsembleFields' mean inside the
    envelope up to 1e-2 (bf16, another decode order), and the `logw_out` of systematic_resample is accepted as log-weights."""
    from sea_amd.ensemble import EnsembleFields, EnsembleQuantiles, systematic_resample
    from oracle.recipe import recipe_inputs
    from tests.test_input_grad_gpu import cfg_of
    from tests.test_model_gpu import build
    from tests.test_rollout_session_gpu import open_on

    c = case("a")
    P, D_, n_mem, B, kk = 4, c["D"], 8, 2, 3
    G, C_ = len(c["groups"]), c["n_inp"]
    F = sum(len(g) for g in c["groups"])
    cfg = cfg_of(1, P * D_, 4, G)
    m = build(cfg, "bf16")
    x, _, ib = recipe_inputs(B, kk + 4, cfg, seed=9)
    dec = decoder("a", "bf16")
    g = torch.Generator().manual_seed(22)
    conds = torch.rand(B * n_mem, 1, generator=g).to(DEV)
    counts = [C_, C_ - 1, 1, C_]
    y = open_on(m, x, ib, kk).fork(n_mem).step(conds)
    prod = EnsembleQuantiles(dec, P, n_mem, levels=(0, 0.5, 1), thresholds=[0.0], counts=counts, fused=True)
    q, e = prod(y)
    mean, _ = EnsembleFields(dec, P, n_mem, counts=counts, fused=True)(y)
    assert q.shape == (3, B, P, F, C_) and e.shape == (1, B, P, F, C_) and not bool(torch.isnan(q).any())
    assert bool((q[0] <= q[1]).all()) and bool((q[1] <= q[2]).all())
    assert bool((mean >= q[0] - 1e-2).all()) and bool((mean <= q[2] + 1e-2).all())
    logw = torch.randn(B * n_mem, generator=g).to(DEV)
    _, logw_out, _, _ = systematic_resample(logw, n_mem, ess_threshold=0.0)   # nothing is resampled: the normalised log-weights come back
    qw, ew = prod(y, logw_out)
    assert bool((qw[0] <= qw[1]).all()) and bool((qw[1] <= qw[2]).all()) and torch.equal(qw[0], q[0]) and torch.equal(qw[2], q[2])   # every member is live: the same envelope
    assert float(ew.min()) >= 0.0 and float(ew.max()) <= 1.0 + 1e-6
    valid = (torch.arange(C_) < torch.tensor(counts)[:, None]).view(1, 1, P, 1, C_).to(DEV)
    assert float(torch.where(valid, torch.zeros((), device=DEV), q).abs().max()) == 0.0
    print(f"ensemble quantiles session: envelope width mean {float((q[2] - q[0]).mean()):.3e}, median - mean max {float((q[1] - mean).abs().max()):.3e}")
