"""Verification of an ensemble against a dense snapshot on the device: sea_decode_member_verify through ops.decode_member_verify, Decode.member_verify and
FieldVerification end to end and on a rollout session.

Reference: `restate_field_verify` of tests/test_field_verify_cpu.py — the fp64 restatement `restate_verify` of tests/test_verify_cpu.py (the double sum
over member pairs) with every cell a sensor, field by field.
  kernel      on EXACT operands (hidden rows with four entries of +-1, second-layer weights in {-1, 0, 1}, bias and readings multiples of 0.25: the
              decoded values are exact multiples of 0.25 whatever the order of the products, ties occur, and the restatement gets the same values):
              rank, hist, status and the two counts in sums exact; the f32 maps within 1e-6 max(1, max |ref|) — tests/test_verify_gpu.py's bound by its
              own argument: the arithmetic is fp64 over at most 128 + 64 terms, the margin covers the fp32 store (6e-8 relative) and nothing else; the
              fp64 sums within SUMS_TOL max(1, max |ref|) (below); against ops.ensemble_verify on the same values: equal bits per cell (both kernels
              call the same device functions)
  end to end  bf16 fused: e <= 2 e_c + 1e-6 for the mean, spread and crps maps and the derived per-field means (e: against the fp64 restatement on
              fp64-decoded values; e_c: fused=False on the same inputs — the project's rule in test_verify_gpu.py and test_field_enkf_gpu.py); fused
              against composed maps <= 1e-4; fp32 (composed) <= TOL_F32; rank and pit are discontinuous in the decoded values and are compared on the
              same values only"""
import functools

import pytest
import torch

from tests.test_decode_loss_cpu import rel
from tests.test_decode_loss_gpu import DEV, TOL_F32, case, decoder
from tests.test_field_enkf_cpu import field_case, field_cases
from tests.test_field_verify_cpu import MAPS, field_logw, restate_field_verify
from tests.test_verify_cpu import FLOATS, close
from tests.test_verify_gpu import same_bits

pytestmark = pytest.mark.gpu

F64 = torch.float64
# A sum of sums[b, f, :] here runs over at most 2 patches x 40 cells = 80 cells, each of them an fp64 sum over at most 128 (the walk) + 64 (the lanes)
# terms: 272 roundings of 2^-53 (the one wider case, 2 x 530 cells of 5 members, has 1060 + 69 terms and is held to the same, tighter figure), with tests/test_verify_gpu.py's three digits for the cancellation between the CRPS's two terms (two from 1 / c <= 100
# under the dominant member, one from the member-pair term against their difference)
SUMS_TOL = 1e3 * 272 * 2.0 ** -53                                                           # 3.0e-11
X_B, X_P, X_F, X_C, X_CP, X_S = 2, 2, 2, 40, 64, 40
X_MEMBERS = (1, 2, 5, 17, 64, 65, 128)
X_COUNTS = ((X_C, 33), (0, 1))


def dev(t):
    return None if t is None else t.to(DEV)


# ------------------------------------------------------------------------------------------------ exact operands
@functools.lru_cache(maxsize=None)
def exact_case(n, counts, with_prec, with_logw, C_=X_C, Cp=X_CP):
    """dict(H, W2, bias, obs, prec, logw, counts, Y, w): operands on which the decode is exact (the trick of test_gram_is_exact_on_integer_operands),
    the decoded members Y [B * n, P, F, C] float64 and the cells' weights w [B, P, F, C]; with_prec: precisions in [0.25, 2], a tenth of the cells
    dead (precision 0, obs NaN there); with_logw: verify_case's log-weights (a dominant member, a dead member; two members leave one)."""
    g = torch.Generator().manual_seed(400 + 16 * n + 4 * counts[0] + 2 * with_prec + with_logw)
    B, P, F, S = X_B, X_P, X_F, X_S
    M = B * n * P
    H = torch.zeros(M, S)
    cols = torch.stack([torch.randperm(S, generator=g)[:4] for _ in range(M)])
    H.scatter_(1, cols, torch.randint(0, 2, (M, 4), generator=g).float() * 2 - 1)
    W2 = torch.zeros(F * Cp, S)
    W2.view(F, Cp, S)[:, :C_] = torch.randint(-1, 2, (F, C_, S), generator=g).float()
    bias = torch.zeros(F * Cp)
    bias.view(F, Cp)[:, :C_] = torch.randint(-8, 9, (F, C_), generator=g).float() / 4
    obs = torch.randint(-12, 13, (B * P, F, C_), generator=g).float() / 4
    prec = None
    if with_prec:
        prec = 0.25 + 1.75 * torch.rand(B * P, F, C_, generator=g)
        miss = torch.rand(B * P, F, C_, generator=g) < 0.1
        prec[miss] = 0.0
        obs[miss] = float("nan")
    logw = field_logw(n, B, 900 + n) if with_logw else None
    return dict(H=H, W2=W2, bias=bias, obs=obs, prec=prec, logw=logw, counts=torch.tensor(counts, dtype=torch.int32), C=C_, Cp=Cp,
                **decode_exact(H, W2, bias, prec, counts, n, C_, Cp))


def decode_exact(H, W2, bias, prec, counts, n, C_=X_C, Cp=X_CP):
    B, P, F = X_B, X_P, X_F
    Y = (H.double() @ W2.double().t() + bias.double()).view(B * n, P, F, Cp)[..., :C_].contiguous()
    w = torch.ones(B, P, F, C_, dtype=F64) if prec is None else prec.view(B, P, F, C_).to(F64)
    w = torch.where((torch.arange(C_) < torch.tensor(counts)[:, None]).view(1, P, 1, C_), w, torch.zeros((), dtype=F64))
    return dict(Y=Y, w=w)


def run_exact(t, n, unbiased, accumulate=False, out=None, maps=MAPS, H=None, hist=None):
    """ops.decode_member_verify on an exact case (hist: that history alone)."""
    from sea_amd import ops

    P = X_P
    H = t["H"] if H is None else H
    obs, prec, logw = t["obs"], t["prec"], t["logw"]
    if hist is not None:
        H, obs = H[hist * n * P:(hist + 1) * n * P], obs[hist * P:(hist + 1) * P]
        prec = None if prec is None else prec[hist * P:(hist + 1) * P]
        logw = None if logw is None else logw[hist * n:(hist + 1) * n]
    grp = [dict(H=H.to(DEV).to(torch.bfloat16), W2=t["W2"].to(DEV).to(torch.bfloat16), bias=t["bias"].to(DEV))]
    return ops.decode_member_verify(grp, obs.to(DEV), t["C"], t["Cp"], P, n, prec=dev(prec), counts=t["counts"].to(DEV), logw=dev(logw), unbiased=unbiased,
                                    accumulate=accumulate, maps=maps, out=out)


def prefilled(B, n, fill, width=X_C):
    """Output buffers that hold NaN or -7: every element has to be written."""
    out = {k: torch.full((B, X_P, X_F, width), fill, device=DEV) for k in FLOATS}
    out.update(rank=torch.full((B, X_P, X_F, width), -7, device=DEV, dtype=torch.int32), sums=torch.full((B, X_F, 8), fill, device=DEV, dtype=F64),
               hist=torch.full((B, X_F, n + 1), -7, device=DEV, dtype=torch.int64), status=torch.full((B,), -7, device=DEV, dtype=torch.int32))
    return out


def check_exact(got, ref, tag):
    """The kernel's bounds (the module docstring); returns the largest error / bound of the f32 maps and of the fp64 sums."""
    got = {k: v.cpu() for k, v in got.items()}
    assert torch.equal(got["rank"].long(), ref["rank"]), tag
    assert torch.equal(got["hist"], ref["hist"]) and torch.equal(got["status"].long(), ref["status"]), tag
    assert torch.equal(got["sums"][..., 0], ref["sums"][..., 0]) and torch.equal(got["sums"][..., 6], ref["sums"][..., 6]), tag
    w32, w64 = 0.0, 0.0
    for k in FLOATS:
        ok, ratio = close(got[k], ref[k], 1e-6)
        w32 = max(w32, ratio)
        assert ok, tag + (k, ratio)
    for j in range(8):
        ok, ratio = close(got["sums"][..., j], ref["sums"][..., j], SUMS_TOL)
        w64 = max(w64, ratio)
        assert ok, tag + ("sums", j, ratio)
    return w32, w64


# ------------------------------------------------------------------------------------------------ 1: the kernel on the same predictions
@pytest.mark.parametrize("n", X_MEMBERS)
def test_kernel_against_fp64_on_exact_operands(n):
    worst32, worst64, cases = 0.0, 0.0, 0
    for counts in X_COUNTS:
        for wp in (False, True):
            for wl in (False, True):
                t = exact_case(n, counts, wp, wl)
                for unbiased in (True, False):
                    ref = restate_field_verify(t["Y"], t["obs"].view(X_B, X_P, X_F, X_C), t["w"], t["logw"], n, unbiased)
                    out = prefilled(X_B, n, float("nan"))
                    got = run_exact(t, n, unbiased, out=out)
                    assert all(got[k].data_ptr() == out[k].data_ptr() for k in out)
                    a, b = check_exact(got, ref, (n, counts, wp, wl, unbiased))
                    worst32, worst64, cases = max(worst32, a), max(worst64, b), cases + 1
                if wl and n >= 2:
                    assert int(ref["status"][0]) == n - 1                               # the dead member is not counted; with two members c = 0
    print(f"field verify N = {n}: largest error / bound over {cases} cases: f32 maps {worst32:.3e} (bound 1e-6), fp64 sums {worst64:.3e} (bound {SUMS_TOL:.1e})")


@pytest.mark.parametrize("n,wl", [(5, False), (5, True), (128, False), (128, True)])
def test_a_nan_latent_row_of_a_live_member_marks_its_history_alone(n, wl):
    t = exact_case(n, X_COUNTS[0], True, wl)
    j = (1 + 2) % n                                                                      # history 1: member 1 leads, member 2 is dead, member 3 is live
    H = t["H"].clone()
    H[(n + j) * X_P:(n + j + 1) * X_P] = float("nan")
    d = decode_exact(H, t["W2"], t["bias"], t["prec"], X_COUNTS[0], n)
    assert bool(torch.isnan(d["Y"][n + j]).all()) and not bool(torch.isnan(d["Y"][:n]).any())
    ref = restate_field_verify(d["Y"], t["obs"].view(X_B, X_P, X_F, X_C), t["w"], t["logw"], n, True)
    got = run_exact(t, n, True, out=prefilled(X_B, n, 7.0), H=H)
    check_exact(got, ref, (n, wl))
    live1 = t["w"][1] > 0
    assert torch.equal(got["rank"][1].cpu()[live1], torch.full((int(live1.sum()),), -2, dtype=torch.int32)) and bool(torch.isnan(got["crps"][1].cpu()[live1]).all())
    assert torch.equal(got["sums"][1, :, 6].cpu(), live1.sum((0, 2)).to(F64)) and float(got["sums"][1, :, :6].abs().max()) == 0.0 and int(got["hist"][1].sum()) == 0
    clean = run_exact(t, n, True)
    assert same_bits({k: v[0] for k, v in got.items()}, {k: v[0] for k, v in clean.items()})   # history 0 does not see it
    if wl:                                                                               # a NaN row of the DEAD member reaches nothing
        H = t["H"].clone()
        H[(n + 2) * X_P:(n + 3) * X_P] = float("nan")
        assert same_bits(run_exact(t, n, True, H=H), clean)


def test_a_field_wider_than_one_chunk_of_tiles():
    """530 columns in 544 are 17 tiles: a workgroup scores 16, so a field has two chunks whose partials the finish launch adds in order; counts 513
    leave the second chunk ONE valid column, counts 512 none (it leaves at once), and the columns from 513 on are dead cells of the maps."""
    n, C_, Cp = 5, 530, 544
    for counts in ((C_, 513), (512, 1)):
        t = exact_case(n, counts, True, True, C_, Cp)
        ref = restate_field_verify(t["Y"], t["obs"].view(X_B, X_P, X_F, C_), t["w"], t["logw"], n, True)
        out = prefilled(X_B, n, float("nan"), C_ + 3)
        got = run_exact(t, n, True, out=out)
        assert all(float(got[k][..., C_:].abs().max()) == 0.0 for k in FLOATS) and bool((got["rank"][..., C_:] == -1).all())
        check_exact({k: v[..., :C_] if k in MAPS else v for k, v in got.items()}, ref, (counts,))
        assert same_bits(run_exact(t, n, True, out=prefilled(X_B, n, 7.0, C_ + 3)), got)
        alone = run_exact(t, n, True, hist=1)
        assert same_bits({k: v[0] for k, v in alone.items()}, {k: v[1][..., :C_] if k in MAPS else v[1] for k, v in got.items()})


# ------------------------------------------------------------------------------------------------ 2: against the sensor kernel
@pytest.mark.parametrize("n", [2, 17, 64, 128])
def test_cells_are_scored_as_sensors(n):
    """ops.ensemble_verify on the same exact values with every cell a sensor, (patch, field, cell) order: ranks equal, the f32 maps equal BITS (one
    device function scores a cell and a sensor), status equal; the sums pooled over the fields within the sums bound (the sensor launch adds
    16-sensor tiles, the field launch 32-column tiles per field)."""
    from sea_amd import ops

    B, P, F, C_ = X_B, X_P, X_F, X_C
    for counts, wp, wl in ((X_COUNTS[0], True, True), (X_COUNTS[0], False, False), (X_COUNTS[1], True, False)):
        t = exact_case(n, counts, wp, wl)
        got = run_exact(t, n, True)
        pred = t["Y"].reshape(B * n, P * F * C_).to(torch.float32).to(DEV)
        s = ops.ensemble_verify(pred, t["obs"].reshape(B, P * F * C_).to(DEV), n, prec=t["w"].reshape(B, P * F * C_).to(torch.float32).to(DEV), logw=dev(t["logw"]),
                                unbiased=True)
        assert torch.equal(got["status"], s["status"])
        assert same_bits({k: got[k].reshape(B, -1) for k in MAPS}, {k: s[k] for k in MAPS}), (n, counts, wp, wl)
        assert torch.equal(got["hist"].sum(1), s["hist"]) and torch.equal(got["sums"].sum(1)[:, 0], s["sums"][:, 0]) and torch.equal(got["sums"].sum(1)[:, 6], s["sums"][:, 6])
        for j in range(8):
            ok, ratio = close(got["sums"].sum(1)[:, j].cpu(), s["sums"][:, j].cpu(), SUMS_TOL)
            assert ok, (n, counts, wp, wl, j, ratio)


# ------------------------------------------------------------------------------------------------ 3: every output element, bits, histories, accumulation
@pytest.mark.parametrize("n", [5, 64, 128])
def test_prefilled_outputs_bits_histories_and_accumulation(n):
    from sea_amd import ops

    for counts in X_COUNTS:
        t = exact_case(n, counts, True, True)
        want = run_exact(t, n, True)
        assert ops.last_form()[0] == "decode.member_verify"
        for fill, width in ((float("nan"), X_C), (-7.0, X_C + 9)):                        # a wider map: the columns from C on are dead cells
            out = prefilled(X_B, n, fill, width)
            got = run_exact(t, n, True, out=out)
            assert same_bits({k: v[..., :X_C] if k in MAPS else v for k, v in got.items()}, want), (n, counts, fill)
            if width > X_C:
                assert all(float(got[k][..., X_C:].abs().max()) == 0.0 for k in FLOATS) and bool((got["rank"][..., X_C:] == -1).all())
        assert same_bits(run_exact(t, n, True), want)                                     # two runs, the same bits
        for maps in ((), ("rank",), ("crps", "pit"), ("mean", "spread", "crps", "pit")):
            got = run_exact(t, n, True, maps=maps)
            assert set(got) == set(maps) | {"sums", "hist", "status"} and same_bits(got, want, keys=got.keys()), (n, counts, maps)
        for h in range(X_B):                                                             # a history alone reproduces its own outputs
            alone = run_exact(t, n, True, hist=h)
            assert same_bits({k: v[0] for k, v in alone.items()}, {k: v[h] for k, v in want.items()}), (n, counts, h)
        t2 = exact_case(n, counts, False, True)                                           # accumulate = the sum of two calls, in the calls' order
        other = run_exact(t2, n, True)
        acc = run_exact(t2, n, True, accumulate=True, out=dict(sums=want["sums"].clone(), hist=want["hist"].clone()))
        assert torch.equal(acc["hist"], want["hist"] + other["hist"]) and same_bits(dict(s=acc["sums"]), dict(s=want["sums"] + other["sums"]))
        assert same_bits(acc, other, keys=MAPS + ("status",))
    lw = exact_case(n, X_COUNTS[0], True, True)["logw"].clone()                           # invalid log-weights: history 1 is not scored, history 0 is untouched
    lw[n] = float("inf")
    t = dict(exact_case(n, X_COUNTS[0], True, True), logw=lw)
    got = run_exact(t, n, True, out=prefilled(X_B, n, float("nan")))
    want = run_exact(exact_case(n, X_COUNTS[0], True, True), n, True)
    assert got["status"].tolist() == [want["status"][0].item(), -1] and same_bits({k: v[0] for k, v in got.items()}, {k: v[0] for k, v in want.items()})
    assert all(float(got[k][1].abs().max()) == 0.0 for k in FLOATS + ("sums", "hist")) and bool((got["rank"][1] == -1).all())


# ------------------------------------------------------------------------------------------------ 4: end to end
CASES = field_cases()
BY_SHAPE = {name: [c for c in CASES if c[0] == name] for name in ("a", "b", "c")}


def latents(k):
    y = k["y"].to(DEV)
    Bm, G, E = y.shape
    P = k["obs"].shape[1]
    return y.reshape(Bm, G, P, E // P).permute(0, 2, 1, 3)


@functools.lru_cache(maxsize=None)
def e2e_reference(name, members, hist, cnt, wp, local, dtype="bf16"):
    """field_case's inputs, log-weights for odd member counts, and the fp64 restatement on the fp64-decoded values (the weights: field_case's w)."""
    k = field_case(name, members, hist, cnt, wp, local, dtype)
    logw = torch.randn(hist * members, generator=torch.Generator().manual_seed(66 + members + hist)) if members % 2 else None
    return k, logw, restate_field_verify(k["Y"], k["obs"], k["w"], logw, members, True)


def verifier(name, k, members, dtype, fused):
    from sea_amd.ensemble import FieldVerification

    return FieldVerification(decoder(name, dtype), case(name)["P"], members, counts=k["counts"], sigma=k["sigma"], fused=fused)


def errors(s, ref):
    """Relative L2 errors of the continuous maps, and the largest relative error of the derived per-field means over the fields with a live cell."""
    cnt = ref["sums"][..., 0]
    on = cnt > 0
    derived = ((s.mean_crps, ref["sums"][..., 1] / cnt), (s.rmse, (ref["sums"][..., 2] / cnt).sqrt()), (s.mean_spread, (ref["sums"][..., 3] / cnt).sqrt()),
               (s.consistency, ref["sums"][..., 4] / cnt))
    e = {q: rel(getattr(s, q).cpu(), ref[q]) for q in ("mean", "spread", "crps")}
    e["derived"] = max(float(((got.cpu()[on] - want[on]).abs() / want[on].abs().clamp_min(1e-300)).max()) for got, want in derived) if bool(on.any()) else 0.0
    return e


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_verification_bf16_against_fp64(name):
    worst = {}
    for case_ in BY_SHAPE[name]:
        _, members, hist, cnt, wp, local = case_
        k, logw, ref = e2e_reference(*case_)
        y, obs, prec, lw = k["y"].to(DEV), dev(k["obs"]), dev(k["prec"]), dev(logw)
        s = verifier(name, k, members, "bf16", True)(y, obs, prec, lw)
        s_c = verifier(name, k, members, "bf16", False)(y, obs, prec, lw)
        P, F, C_ = k["obs"].shape[1:]
        assert s.crps.dtype == torch.float32 and s.crps.shape == (hist, P, F, C_) and s.rank.dtype == torch.int32 and s.sums.dtype == F64
        assert s.sums.shape == (hist, F, 8) and s.hist.shape == (hist, F, members + 1) and s.status.shape == (hist,)
        for t in (s, s_c):
            assert torch.equal(t.status.cpu().long(), ref["status"]) and torch.equal(t.sums[..., 0].cpu(), ref["sums"][..., 0])
            assert torch.equal(t.hist.sum(2).cpu().double(), ref["sums"][..., 0]) and torch.equal((t.rank == -1).cpu(), k["w"] == 0)
        if float(ref["sums"][..., 0].sum()) == 0.0:
            assert all(float(getattr(s, q).abs().max()) == 0.0 for q in FLOATS)
            continue
        e, e_c = errors(s, ref), errors(s_c, ref)
        fc = {q: rel(getattr(s, q).cpu(), getattr(s_c, q).cpu()) for q in ("mean", "spread", "crps")}
        print(f"field verify {name} members {members} x {hist} counts {cnt} prec {wp}: fused " + " ".join(f"{q} {v:.3e}" for q, v in e.items())
              + "; composed " + " ".join(f"{q} {v:.3e}" for q, v in e_c.items()) + "; fused vs composed " + " ".join(f"{q} {v:.3e}" for q, v in fc.items()))
        for q in e:
            assert e[q] <= 2 * e_c[q] + 1e-6, (members, hist, cnt, wp, q, e[q], e_c[q])
            worst[q] = max(worst.get(q, 0.0), e[q])
        for q in fc:
            assert fc[q] <= 1e-4, (members, hist, cnt, wp, q, fc[q])
            worst["fc " + q] = max(worst.get("fc " + q, 0.0), fc[q])
    print(f"field verify shape {name} worst: " + " ".join(f"{q} {v:.3e}" for q, v in worst.items()))


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_verification_fp32_against_fp64(name):
    worst = {}
    for case_ in BY_SHAPE[name]:
        _, members, hist, cnt, wp, local = case_
        if name == "a" and members in (17, 128) and hist == 3:
            continue                                                                      # the composed path is the same code at every size: the extremes are kept
        k, logw, ref = e2e_reference(*case_, "fp32")
        s = verifier(name, k, members, "fp32", None)(k["y"].to(DEV), dev(k["obs"]), dev(k["prec"]), dev(logw))
        if float(ref["sums"][..., 0].sum()) == 0.0:
            continue
        e = errors(s, ref)
        for q in e:
            assert e[q] <= TOL_F32, (members, hist, cnt, wp, q, e[q])
            worst[q] = max(worst.get(q, 0.0), e[q])
    print(f"field verify fp32 shape {name} worst: " + " ".join(f"{q} {v:.3e}" for q, v in worst.items()))


# ------------------------------------------------------------------------------------------------ 5: no host work; a rollout session; the mesh
def test_verification_around_an_analysis_on_a_rollout_session():
    """open_rollout -> fork(n + 1) -> step: the first n members of a history are the ensemble, the last one is the truth — a self-consistent one: drawn
    like the members (its own condition), so it lies in the one-parameter family the ensemble samples.  The snapshot is the truth's exact decoded field
    plus noise of the variance 1 / precision that the analysis is told (trace(C) = 50 per history, the fixture of test_field_enkf_gpu's session test);
    the scores are taken against the truth itself.  FieldVerification (the forecast) -> FieldKalman.analyse -> FieldVerification (the analysis): nothing
    is read back or uploaded in a warm call, the mesh-wide mean CRPS does not rise, every live cell is in a histogram, and into= adds the two up."""
    from sea_amd.ensemble import FieldKalman, FieldVerification
    from oracle.recipe import recipe_inputs
    from tests.test_field_enkf_cpu import decode_members, field_weights
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
    conds = torch.rand(B * (n_mem + 1), 1, generator=g).to(DEV)
    counts = [C_, C_ - 1, 1, C_]
    base = 0.5 + torch.rand(B, P, F, C_, generator=g)
    base[torch.rand(B, P, F, C_, generator=g) < 0.2] = 0.0
    y_all = open_on(m, x, ib, kk).fork(n_mem + 1).step(conds)
    E = y_all.shape[-1]
    y = y_all.view(B, n_mem + 1, G, E)[:, :n_mem].reshape(B * n_mem, G, E).contiguous()
    fields = lambda t: decode_members("a", t.detach().cpu().double().reshape(-1, G, P, D_).permute(0, 2, 1, 3))   # noqa: E731
    Yv, truth = fields(y).view(B, n_mem, P, F, C_), fields(y_all.view(B, n_mem + 1, G, E)[:, n_mem])
    w0 = field_weights((B, P, F, C_), None, base, counts)
    anom = Yv - Yv.mean(1, keepdim=True)
    trace = (w0 * (anom * anom).sum(1) / (n_mem - 1)).sum(dim=(1, 2, 3), keepdim=True)
    assert bool((trace > 0).all())
    prec = (base.double() * 50.0 / trace).to(torch.float32)
    noise = torch.randn(B, P, F, C_, generator=g) * torch.where(prec > 0, prec.rsqrt(), torch.zeros(()))
    obs = (truth + noise).to(torch.float32)
    live = field_weights((B, P, F, C_), None, prec, counts) > 0
    ka = FieldKalman(dec, P, n_mem, counts=counts, fused=True)
    ver = FieldVerification(dec, P, n_mem, counts=counts, fused=True)
    obs_d, prec_d, truth_d = obs.to(DEV), prec.to(DEV), truth.to(torch.float32).to(DEV)
    ver(y, truth_d, prec_d)                                                              # the first call on a device uploads the counts
    ka.transform(y, obs_d, prec_d)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        forecast = ver(y, truth_d, prec_d)
        ya = ka.analyse(y, obs_d, prec_d)
        analysis = ver(ya, truth_d, prec_d)
        crps_f, crps_a, infl = forecast.pooled().mean_crps, analysis.pooled().mean_crps, forecast.suggested_inflation
        total = ver(ya, truth_d, prec_d, into=ver(y, truth_d, prec_d, maps=()), maps=("rank",))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    print(f"field verify session: mean crps against the truth, forecast {crps_f.tolist()} analysis {crps_a.tolist()}; suggested inflation per field {infl.tolist()}")
    assert bool((crps_a <= crps_f).all())
    assert torch.equal(forecast.count.cpu(), live.sum((1, 3)).to(F64)) and torch.equal(forecast.hist.sum(2).cpu(), live.sum((1, 3)))
    assert torch.equal((forecast.rank >= 0).cpu(), live) and forecast.status.tolist() == [n_mem] * B
    assert total.crps is None and total.rank is not None and torch.equal(total.hist, forecast.hist + analysis.hist)
    assert same_bits(dict(s=total.sums), dict(s=forecast.sums + analysis.sums))


def test_maps_on_the_mesh():
    """unpatch_map puts pit and rank on the mesh unchanged, unpatch_spread the CRPS in physical units (|a| crps), on the 3 x 4 partition of
    tests/golden/unpatch_3x4.npz; "BPCF" observations give the same scores."""
    from sea_amd.ensemble import FieldVerification
    from sea_amd.models.encoder_decoder import Decode
    from sea_amd.utils.data_processors import DataPartitioner2D, MeshUnpatcher, MinMaxScaler
    from tests.conftest import load_golden

    gd = load_golden("unpatch_3x4")
    m, n = (int(v) for v in gd["mn"])
    xy = torch.from_numpy(gd["xy"])
    part = DataPartitioner2D(xy[0], xy[1], m=m, n=n, pad_id=-1, pad_field_value=0, device=DEV)
    idx = torch.from_numpy(gd["index_map"])
    P, C = idx.shape
    groups, D, members, B = [[0], [1]], 16, 8, 2
    scalers = []
    for rng_, lo, hi in (((-1, 1), -1.0, 3.0), ((1, -1), 0.5, 2.0)):
        sc = MinMaxScaler(feature_range=rng_)
        sc.min_val, sc.max_val = torch.tensor(lo), torch.tensor(hi)
        scalers.append(sc)
    a = [sc.inverse_affine()[0] for sc in scalers]
    torch.manual_seed(14)
    n_inp = (C + 3) // 4 * 4
    dec = Decode(groups, n_inp, 40, D).requires_grad_(False).set_compute_dtype("bf16").to(DEV)
    g = torch.Generator().manual_seed(16)
    y = torch.randn(B * members, 2, P * D, generator=g).to(DEV)
    obs = torch.randn(B, P, 2, n_inp, generator=g).to(DEV)
    counts = (idx >= 0).sum(1).tolist()
    s = FieldVerification(dec, P, members, counts=counts, fused=True)(y, obs)
    s2 = FieldVerification(dec, P, members, counts=counts, layout="BPCF", fused=True)(y, obs.permute(0, 1, 3, 2).contiguous())
    assert same_bits({k: getattr(s, k) for k in MAPS + ("sums", "hist")}, {k: getattr(s2, k) for k in MAPS + ("sums", "hist")})
    mu = MeshUnpatcher(part, groups, scalers)
    npts = xy.shape[1]
    rank_m, pit_m, crps_m = mu.unpatch_map(s.rank[..., :C]), mu.unpatch_map(s.pit[..., :C]), mu.unpatch_spread(s.crps[..., :C])
    assert rank_m.shape == (B, npts, 2) and rank_m.dtype == torch.float32
    ref = {q: torch.zeros(B, npts, 2) for q in ("rank", "pit", "crps")}
    for p in range(P):
        for c_ in range(C):
            if idx[p, c_] >= 0:
                for f in range(2):
                    ref["rank"][:, idx[p, c_], f] = s.rank.cpu()[:, p, f, c_].float()
                    ref["pit"][:, idx[p, c_], f] = s.pit.cpu()[:, p, f, c_]
                    ref["crps"][:, idx[p, c_], f] = abs(a[f]) * s.crps.cpu()[:, p, f, c_]
    assert torch.equal(rank_m.cpu(), ref["rank"]) and torch.equal(pit_m.cpu(), ref["pit"]) and rel(crps_m.cpu(), ref["crps"]) <= 1e-6
    assert float(rank_m.min()) >= 0.0 and float(rank_m.max()) <= members                  # every mesh point is a live cell
    assert torch.equal(mu.unpatch_map(s.rank[..., :C].permute(0, 1, 3, 2).contiguous(), layout="BPCF"), rank_m)


# ------------------------------------------------------------------------------------------------ 6: the default rule
def test_default_rule_takes_the_fused_launches_from_4096_rows_on(monkeypatch):
    """fused=None: the fused launches in bf16 up to 128 members from 4096 decoder rows on (every measured row of profiles/field_verify_bench.txt), the
    composed path below, in fp32 and above 128 members."""
    from sea_amd import ops
    from sea_amd.ensemble import FieldVerification

    c = case("a")
    P, G, D_, F, C_ = 64, len(c["groups"]), c["D"], sum(len(g) for g in c["groups"]), c["n_inp"]
    dec = decoder("a", "bf16")
    g = torch.Generator().manual_seed(4)
    obs = torch.randn(1, P, F, C_, generator=g).to(DEV)
    calls = []
    native = ops.decode_member_verify
    monkeypatch.setattr(ops, "decode_member_verify", lambda *a, **k: (calls.append(1), native(*a, **k))[1])
    for members, fused in ((64, True), (32, False)):
        y = torch.randn(members, G, P * D_, generator=g).to(DEV).to(torch.bfloat16)
        ver = FieldVerification(dec, P, members, sigma=3.0)
        assert ver._fused_for(y) is fused
        del calls[:]
        s = ver(y, obs)
        assert len(calls) == (1 if fused else 0) and s.status.tolist() == [members]
        assert (ops.last_form()[0] == "decode.member_verify") is fused
    assert FieldVerification(decoder("a", "fp32"), P, 64)._fused_for(torch.zeros(64, G, P * D_)) is False
    assert FieldVerification(dec, P, 129)._fused_for(torch.zeros(129, G, P * D_)) is False
    assert FieldVerification(dec, P, 32, fused=True)._fused_for(torch.zeros(32, G, P * D_)) is True
