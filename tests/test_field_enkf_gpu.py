"""The ensemble Kalman analysis from a dense snapshot on the device: sea_decode_member_gram through Decode.member_gram, sea_enkf_transform_gram
through ops.enkf_transform_gram, and FieldKalman on top of both.

References: the fp64 restatements of tests/test_field_enkf_cpu.py on that file's inputs (cond(I + C) <= 1e4 is asserted there, per input).  Let e be
the relative L2 error of a result against the restatement and e_c that of the composed bf16 path (forward() + fp64 torch ops) on the same inputs.
  gram, proj   fused against composed <= 1e-4 (the project's bound for a quadratic quantity reduced in another order,
               tests/test_ensemble_moments_gpu.py), and e <= 2 e_c + 1e-6; count exact; gram exactly symmetric
  D            on the device's own gram / proj / count copied to the host: max |D - D_ref| <= 1e-6 max(1, max |D_ref|) (tests/test_enkf_gpu.py's bound:
               the fp32 store at cond <= 1e4); status exact
  increment    bf16: e <= 2 e_c + 1e-6 and e <= 2 x the CPU file's envelope; fp32 (composed): e <= 1e-4
Shapes a, b, c of tests/test_decode_loss_gpu.py (hidden 40, 64, 624; Cp 32 and 64 with C no multiple of 32; 1 - 3 groups; P 9, 4, 2); 2, 5, 17, 64 and
128 members on fresh states of shape a, the shapes' own splits on b and c; without counts and with ragged ones; 1 and 3 (or 7) histories; with and
without a precision map; one domain and a [P, P] taper with an all-zero row."""
import pytest
import torch

from tests.test_decode_loss_cpu import rel
from tests.test_decode_loss_gpu import DEV, TOL_F32, case, decoder
from tests.test_field_enkf_cpu import F64, field_case, field_cases, field_envelope, restate_mix, restate_transform_gram

pytestmark = pytest.mark.gpu

CASES = field_cases()
BY_SHAPE = {name: [c for c in CASES if c[0] == name] for name in ("a", "b", "c")}


def dev(t):
    return None if t is None else t.to(DEV)


def latents(k):
    """z [Bm, P, G, D] on the device from the case's states y [Bm, G, P * D] (the re-layout of FieldLikelihood)."""
    y = k["y"].to(DEV)
    Bm, G, E = y.shape
    P = k["obs"].shape[1]
    return y.reshape(Bm, G, P, E // P).permute(0, 2, 1, 3)


def field_precision(k):
    F = k["obs"].shape[2]
    return torch.full((F,), 1.0 / k["sigma"] ** 2, dtype=torch.float32, device=DEV)


def gram_of(dec, k, members, fused, z=None, obs=None, prec="case"):
    return dec.member_gram(latents(k) if z is None else z, dev(k["obs"]) if obs is None else obs, members, counts=k["counts"],
                           precision=dev(k["prec"]) if isinstance(prec, str) else prec, field_precision=field_precision(k), fused=fused)


def kalman(name, k, members, dtype, fused):
    from sea_amd.ensemble import FieldKalman

    return FieldKalman(decoder(name, dtype), case(name)["P"], members, counts=k["counts"], sigma=k["sigma"], inflation=k["rho"], anomaly_gain=k["alpha"],
                       taper=k["taper"], fused=fused)


# ------------------------------------------------------------------------------------------------ 1: the gram kernel
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_gram_against_the_composed_path_and_fp64(name):
    dec = decoder(name, "bf16")
    worst = dict(gc=0.0, pc=0.0, g=0.0, p=0.0)
    for _, members, hist, cnt, wp, local in BY_SHAPE[name]:
        k = field_case(name, members, hist, cnt, wp, local)
        gram, proj, count = gram_of(dec, k, members, True)
        c_gram, c_proj, c_count = gram_of(dec, k, members, False)
        P = case(name)["P"]
        assert gram.shape == (hist, P, members, members) and gram.dtype == torch.float64 and proj.shape == (hist, P, members) and proj.dtype == torch.float64
        assert count.shape == (hist, P) and count.dtype == torch.int32
        assert torch.equal(count.cpu().long(), k["count"]) and torch.equal(c_count.cpu().long(), k["count"])
        assert torch.equal(gram, gram.transpose(-1, -2))                         # exactly symmetric
        live = k["count"] > 0
        if not bool(live.any()):
            assert float(gram.abs().max()) == 0.0 and float(proj.abs().max()) == 0.0
            continue
        assert float(gram.cpu()[~live].abs().max() if bool((~live).any()) else 0.0) == 0.0
        e_gc, e_pc = rel(gram.cpu(), c_gram.cpu()), rel(proj.cpu(), c_proj.cpu())
        e_g, ec_g, e_p, ec_p = rel(gram.cpu(), k["gram"]), rel(c_gram.cpu(), k["gram"]), rel(proj.cpu(), k["proj"]), rel(c_proj.cpu(), k["proj"])
        print(f"member_gram {name} members {members} x {hist} counts {cnt} prec {wp}: fused vs composed gram {e_gc:.3e} proj {e_pc:.3e}; "
              f"gram fused e {e_g:.3e} composed e_c {ec_g:.3e}; proj fused e {e_p:.3e} composed e_c {ec_p:.3e}")
        assert e_gc <= 1e-4 and e_pc <= 1e-4, (members, hist, cnt, wp, e_gc, e_pc)
        assert e_g <= 2 * ec_g + 1e-6 and e_p <= 2 * ec_p + 1e-6, (members, hist, cnt, wp, e_g, ec_g, e_p, ec_p)
        worst = dict(gc=max(worst["gc"], e_gc), pc=max(worst["pc"], e_pc), g=max(worst["g"], e_g), p=max(worst["p"], e_p))
    print(f"member_gram shape {name} worst: fused vs composed gram {worst['gc']:.3e} proj {worst['pc']:.3e}; vs fp64 gram {worst['g']:.3e} proj {worst['p']:.3e}")


@pytest.mark.parametrize("name,members,hist", [("a", 17, 3), ("a", 128, 1), ("c", 5, 7)])
def test_prefilled_outputs_are_fully_overwritten(name, members, hist):
    from sea_amd import ops

    dec = decoder(name, "bf16")
    k = field_case(*next(c for c in BY_SHAPE[name] if c[1:5] == (members, hist, True, True)))
    want = gram_of(dec, k, members, True)
    z = latents(k)
    Bm, P, G, D_ = z.shape
    hid, _ = dec._first_layer(z, torch.bfloat16)
    _, W2 = dec._weights(torch.bfloat16)
    cnt, _ = dec._valid_counts(k["counts"], P, z.device, allow_empty=True, what="member_gram")
    F, C_ = k["obs"].shape[2], case(name)["n_inp"]
    for fill in (float("nan"), 7.0):
        out = (torch.full((hist, P, members, members), fill, dtype=F64, device=DEV), torch.full((hist, P, members), fill, dtype=F64, device=DEV),
               torch.full((hist, P), -77, dtype=torch.int32, device=DEV))
        got = ops.decode_member_gram([dict(H=hid[g], W2=W2[g], bias=dec._shadow[3][g]) for g in range(G)], dev(k["obs"]).reshape(hist * P, F, C_), C_, dec._n_inp_p, P,
                                     members, prec_field=field_precision(k), prec=dev(k["prec"]).reshape(hist * P, F, C_), counts=cnt, out=out)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert ops.last_form()[0] == "decode.member_gram"


@pytest.mark.parametrize("members", [2, 16, 32, 64, 128])
def test_gram_is_exact_on_integer_operands(members):
    """The path from the decode accumulators through the LDS image into the operands of the f32 MFMA, the block ownership and the mirror, on data for
    which every step is exact: hidden rows with four entries of +-1, second-layer weights in {-1, 0, 1}, integer bias and readings, unit weights and a
    power-of-two member count.  Then y is a small integer, the mean and the anomalies are multiples of 1 / N below 16, a chain of four products stays
    below 2^24 / N^2 in units of 1 / N^2 — exact in fp32 — and everything above is fp64: gram, proj and count must EQUAL the fp64 products of random
    (asymmetric) members.  A swapped row / column map, a wrong k pairing or a wrong mirror cannot pass."""
    from sea_amd import ops

    g = torch.Generator().manual_seed(300 + members)
    B, P, F, C_, Cp, S = 2, 2, 2, 40, 64, 40
    M = B * members * P
    H = torch.zeros(M, S)
    cols = torch.stack([torch.randperm(S, generator=g)[:4] for _ in range(M)])
    H.scatter_(1, cols, torch.randint(0, 2, (M, 4), generator=g).float() * 2 - 1)
    W2 = torch.zeros(F * Cp, S)
    W2.view(F, Cp, S)[:, :C_] = torch.randint(-1, 2, (F, C_, S), generator=g).float()
    bias = torch.zeros(F * Cp)
    bias.view(F, Cp)[:, :C_] = torch.randint(-2, 3, (F, C_), generator=g).float()
    obs = torch.randint(-4, 5, (B * P, F, C_), generator=g).float()
    counts = torch.tensor([C_, 33], dtype=torch.int32)
    gram, proj, count = ops.decode_member_gram([dict(H=H.to(DEV).to(torch.bfloat16), W2=W2.to(DEV).to(torch.bfloat16), bias=bias.to(DEV))], obs.to(DEV), C_, Cp, P, members,
                                               counts=counts.to(DEV))
    Y = (H.double() @ W2.double().t() + bias.double()).view(B, members, P, F, Cp)[..., :C_]
    valid = (torch.arange(C_) < counts[:, None]).view(1, 1, P, 1, C_)
    A = torch.where(valid, Y - Y.mean(1, keepdim=True), torch.zeros((), dtype=F64))                        # [B, N, P, F, C]
    E = torch.where(valid[:, 0], obs.view(B, P, F, C_).double() - Y.mean(1), torch.zeros((), dtype=F64))   # [B, P, F, C]
    Ap = A.permute(0, 2, 1, 3, 4).reshape(B, P, members, F * C_)
    want_gram = Ap @ Ap.transpose(-1, -2)
    want_proj = (Ap @ E.reshape(B, P, F * C_, 1)).squeeze(-1)
    assert float(A.abs().max()) < 16 and not torch.equal(want_gram[0, 0], want_gram[0, 1])
    assert torch.equal(count.cpu(), (counts * F).view(1, P).expand(B, P).to(torch.int32))
    assert torch.equal(gram.cpu(), want_gram), float((gram.cpu() - want_gram).abs().max())
    assert torch.equal(proj.cpu(), want_proj), float((proj.cpu() - want_proj).abs().max())


# ------------------------------------------------------------------------------------------------ 2: bits
@pytest.mark.parametrize("name,members,hist", [("a", 5, 3), ("a", 64, 3), ("a", 128, 3), ("b", 11, 3), ("c", 5, 7)])
def test_gram_bits(name, members, hist):
    dec = decoder(name, "bf16")
    case_id = next(c for c in BY_SHAPE[name] if c[1:5] == (members, hist, True, True))
    k = field_case(*case_id)
    z, obs, prec = latents(k), dev(k["obs"]), dev(k["prec"])
    first = gram_of(dec, k, members, True)
    again = gram_of(dec, k, members, True)
    for a, b in zip(first, again):
        assert torch.equal(a, b)                                                  # two runs: the same bits
    h = 1                                                                         # a history alone equals that history beside the others
    alone = dec.member_gram(z[h * members:(h + 1) * members], obs[h:h + 1], members, counts=k["counts"], precision=prec[h:h + 1],
                            field_precision=field_precision(k), fused=True)
    for a, b in zip(alone, first):
        assert torch.equal(a[0], b[h])
    # NaN (and Inf) in obs and in the precision map at cells without weight change no bit: invalid slots, cells whose precision is 0
    C_ = case(name)["n_inp"]
    dead = ~(k["w"] > 0)
    obs2, prec2 = k["obs"].clone(), k["prec"].clone()
    obs2[dead] = float("nan")
    prec2[dead] = float("nan")
    invalid = dead & (torch.arange(C_) >= torch.tensor(k["counts"])[:, None]).view(1, -1, 1, C_)
    obs2[invalid] = float("inf")
    prec2[invalid & (torch.arange(C_) % 2 == 0)] = -3.0
    poisoned = gram_of(dec, k, members, True, obs=obs2.to(DEV), prec=prec2.to(DEV))
    for a, b in zip(poisoned, first):
        assert torch.equal(a, b)


@pytest.mark.parametrize("members,local", [(5, True), (17, False), (128, True)])
def test_a_nan_latent_stops_its_own_problems_only(members, local):
    from sea_amd import ops

    name, hist = "a", 3
    k = field_case(name, members, hist, False, False, next(c[5] for c in BY_SHAPE[name] if c[1:5] == (members, hist, False, False)))
    dec = decoder(name, "bf16")
    P = case(name)["P"]
    taper = torch.eye(P) if local else None
    z = latents(k).contiguous()
    clean = gram_of(dec, k, members, True, z=z)
    D0, s0 = ops.enkf_transform_gram(*clean, taper=dev(taper), rho=k["rho"], alpha=k["alpha"])
    hb, pb, jb = 1, 2, members - 1
    zb = z.clone()
    zb[hb * members + jb, pb, 0, 3] = float("nan")                                # one latent element of one member in one patch
    gram, proj, count = gram_of(dec, k, members, True, z=zb)
    want = clean[2].clone()
    want[hb, pb] = -1
    assert torch.equal(count, want)
    keep = torch.ones(hist, P, dtype=torch.bool, device=DEV)
    keep[hb, pb] = False
    assert torch.equal(gram[keep], clean[0][keep]) and torch.equal(proj[keep], clean[1][keep])
    D, status = ops.enkf_transform_gram(gram, proj, count, taper=dev(taper), rho=k["rho"], alpha=k["alpha"])
    if local:
        assert int(status[hb, pb]) == -1 and float(D[hb, pb].abs().max()) == 0.0
        assert torch.equal(status[keep], s0[keep]) and torch.equal(D[keep], D0[keep])
    else:
        assert int(status[hb, 0]) == -1 and float(D[hb].abs().max()) == 0.0
        others = [b for b in range(hist) if b != hb]
        assert torch.equal(status[others], s0[others]) and torch.equal(D[others], D0[others])


# ------------------------------------------------------------------------------------------------ 3: the transform on the same gram / proj
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_transform_against_fp64_on_the_same_partials(name):
    from sea_amd import ops

    dec = decoder(name, "bf16")
    worst = 0.0
    for _, members, hist, cnt, wp, local in BY_SHAPE[name]:
        k = field_case(name, members, hist, cnt, wp, local)
        gram, proj, count = gram_of(dec, k, members, True)
        D, status = ops.enkf_transform_gram(gram, proj, count, taper=dev(k["taper"]), rho=k["rho"], alpha=k["alpha"])
        assert ops.last_form()[0] == "enkf.transform_gram"
        D_ref, s_ref, cond = restate_transform_gram(gram.cpu(), proj.cpu(), count.cpu().long(), k["taper"], k["rho"], k["alpha"])
        Ld = 1 if k["taper"] is None else k["taper"].shape[0]
        assert D.shape == (hist, Ld, members, members) and D.dtype == torch.float32 and status.dtype == torch.int32
        assert torch.equal(status.cpu().long(), s_ref) and torch.equal(s_ref, k["status"])
        err = float((D.cpu().double() - D_ref).abs().max())
        bound = 1e-6 * max(1.0, float(D_ref.abs().max()))
        worst = max(worst, err / bound)
        print(f"enkf_transform_gram {name} members {members} x {hist} counts {cnt} prec {wp} local {local}: max |D - D_ref| {err:.3e} bound {bound:.3e} "
              f"cond {float(cond.max()):.3e}")
        assert err <= bound, (members, hist, cnt, wp, local, err, bound)
        again, _ = ops.enkf_transform_gram(gram, proj, count, taper=dev(k["taper"]), rho=k["rho"], alpha=k["alpha"])
        assert torch.equal(again, D)
    print(f"enkf_transform_gram shape {name} worst: {worst:.3f} of the bound")


def test_no_live_cell_is_no_update():
    name, members, hist = "a", 5, 3
    k = field_case(name, members, hist, False, False, next(c[5] for c in BY_SHAPE[name] if c[1:5] == (members, hist, False, False)))
    from sea_amd.ensemble import FieldKalman

    P = case(name)["P"]
    y = k["y"].to(DEV)
    for taper in (None, torch.ones(P, P)):
        ka = FieldKalman(decoder(name, "bf16"), P, members, counts=[0] * P, sigma=k["sigma"], inflation=1.0, taper=taper, fused=True)
        D, status = ka.transform(y, dev(k["obs"]))
        assert float(D.abs().max()) == 0.0 and int(status.abs().max()) == 0
        assert torch.equal(ka.analyse(y, dev(k["obs"])), y)
    ka = FieldKalman(decoder(name, "bf16"), P, members, sigma=k["sigma"], inflation=1.0, fused=True)      # every cell missing through the precision map
    D, status = ka.transform(y, torch.full_like(dev(k["obs"]), float("nan")), torch.zeros_like(dev(k["obs"])))
    assert float(D.abs().max()) == 0.0 and int(status.abs().max()) == 0


# ------------------------------------------------------------------------------------------------ 4: against the sensor path
@pytest.mark.parametrize("members,hist,cnt,wp", [(5, 3, True, True), (17, 1, False, False), (64, 1, True, True)])
def test_field_kalman_against_sensor_kalman_with_every_valid_cell_a_sensor(members, hist, cnt, wp):
    """The same analysis through the two routes of the library.  Both decode in bf16 with fp32 accumulation; they differ in the order of the fp32 sums
    (the sensor path forms C in fp64 from stored fp32 predictions, the field path sums products in fp32 inside a 32-column tile).  A relative
    perturbation eps of C and v moves W = (I + C)^-1 by W dC W = eps (W - W^2), whose norm is at most eps / 4, and D is built from W and W v with
    factors of order 1: with eps = 1e-4, the bound for a quadratic quantity reduced in another order, the two D agree to 1e-4 on top of item 3's
    bound.  The measured value is printed."""
    from sea_amd.ensemble import SensorKalman, SensorSet

    name = "a"
    local = next(c[5] for c in BY_SHAPE[name] if c[1:5] == (members, hist, cnt, wp))
    k = field_case(name, members, hist, cnt, wp, local)
    c = case(name)
    P, C_ = c["P"], c["n_inp"]
    flat = [f for g in c["groups"] for f in g]
    F = len(flat)
    counts = k["counts"] if k["counts"] is not None else [C_] * P
    cells = [(p, fi, cc) for p in range(P) for fi in range(F) for cc in range(counts[p])]          # every VALID cell
    dec = decoder(name, "bf16")
    s = SensorSet(dec, P, [p for p, _, _ in cells], [cc for _, _, cc in cells], [flat[fi] for _, fi, _ in cells])
    idx = torch.tensor([(p * F + fi) * C_ + cc for p, fi, cc in cells])
    obs_k = k["obs"].reshape(hist, -1)[:, idx]
    prec_k = (torch.ones(hist, P * F * C_) if k["prec"] is None else k["prec"].reshape(hist, -1))[:, idx]
    obs_k = torch.where(prec_k > 0, obs_k, torch.zeros(()))                                        # the sensor path takes no NaN readings on the host check
    taper_k = None if k["taper"] is None else k["taper"][:, [p for p, _, _ in cells]].contiguous()
    sk = SensorKalman(dec, P, members, s, sigma=k["sigma"], inflation=k["rho"], anomaly_gain=k["alpha"], taper=taper_k, fused=True)
    D_s, st_s, _ = sk.transform(k["y"].to(DEV), obs_k.to(DEV), prec_k.to(DEV))
    D_f, st_f = kalman(name, k, members, "bf16", True).transform(k["y"].to(DEV), dev(k["obs"]), dev(k["prec"]))
    assert torch.equal(st_s, st_f)
    err = float((D_f.double() - D_s.double()).abs().max())
    bound = 1e-6 * max(1.0, float(D_s.abs().max())) + 1e-4
    print(f"field vs sensor kalman members {members} x {hist} counts {cnt} prec {wp} local {local}: max |D_field - D_sensor| {err:.3e} (bound {bound:.3e}), "
          f"max |D| {float(D_s.abs().max()):.3e}, {len(cells)} cells")
    assert err <= bound, (err, bound)


# ------------------------------------------------------------------------------------------------ 5: end to end
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_analyse_bf16_against_fp64(name):
    from sea_amd import ops

    env = field_envelope()
    worst = 0.0
    for _, members, hist, cnt, wp, local in BY_SHAPE[name]:
        k = field_case(name, members, hist, cnt, wp, local)
        y, obs, prec = k["y"].to(DEV), dev(k["obs"]), dev(k["prec"])
        ka = kalman(name, k, members, "bf16", True)
        ya, inc = ka.analyse(y, obs, prec, increment=True)
        yc, inc_c = kalman(name, k, members, "bf16", False).analyse(y, obs, prec, increment=True)
        assert ya.dtype == y.dtype and ya.shape == y.shape and inc.dtype == torch.float32 and yc.dtype == y.dtype
        if float(k["inc"].abs().max()) == 0.0:
            assert float(inc.abs().max()) == 0.0 and torch.equal(ya, y)
            continue
        e, e_c = rel(inc.cpu(), k["inc"]), rel(inc_c.cpu(), k["inc"])
        worst = max(worst, e)
        print(f"field enkf analyse {name} members {members} x {hist} counts {cnt} prec {wp} local {local}: fused e {e:.3e}; composed e_c {e_c:.3e}; envelope {env:.3e}")
        assert e <= 2 * e_c + 1e-6, (members, hist, cnt, wp, local, e, e_c)
        assert e <= 2 * env, (members, hist, cnt, wp, local, e, env)
        D, status = ka.transform(y, obs, prec)                                    # analyse is transform + ensemble_mix, bit for bit
        assert torch.equal(status.cpu().long(), k["status"])
        out, inc2 = ops.ensemble_mix(y, D, case(name)["P"], output=True, increment=True)
        assert torch.equal(out, ya) and torch.equal(inc2, inc)
    print(f"field enkf analyse shape {name} worst fused e {worst:.3e} (envelope {env:.3e})")


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_analyse_fp32_against_fp64(name):
    worst = 0.0
    for _, members, hist, cnt, wp, local in BY_SHAPE[name]:
        if name == "a" and members in (17, 128) and hist == 3:
            continue                                                              # the composed path is the same code at every size: the extremes are kept
        k = field_case(name, members, hist, cnt, wp, local, "fp32")
        y = k["y"].to(DEV)
        ya, inc = kalman(name, k, members, "fp32", None).analyse(y, dev(k["obs"]), dev(k["prec"]), increment=True)
        if float(k["inc"].abs().max()) == 0.0:
            assert float(inc.abs().max()) == 0.0
            continue
        e = rel(inc.cpu(), k["inc"])
        worst = max(worst, e)
        assert ya.dtype == torch.float32 and e <= TOL_F32, (members, hist, cnt, wp, local, e)
        assert torch.equal(ya, y + inc)
    print(f"field enkf analyse fp32 shape {name} worst e {worst:.3e}")


def test_default_rule_takes_the_fused_launches_from_4096_rows_on(monkeypatch):
    from sea_amd import ops
    from sea_amd.ensemble import FieldKalman

    c = case("a")
    P, G, D_, F, C_ = 64, len(c["groups"]), c["D"], sum(len(g) for g in c["groups"]), c["n_inp"]
    dec = decoder("a", "bf16")
    g = torch.Generator().manual_seed(4)
    obs = torch.randn(1, P, F, C_, generator=g).to(DEV)
    calls = []
    native = ops.decode_member_gram
    monkeypatch.setattr(ops, "decode_member_gram", lambda *a, **k: (calls.append(1), native(*a, **k))[1])
    for members, fused in ((64, True), (32, False)):
        y = torch.randn(members, G, P * D_, generator=g).to(DEV).to(torch.bfloat16)
        ka = FieldKalman(dec, P, members, sigma=3.0)
        assert ka._fused_for(y) is fused
        del calls[:]
        ka.transform(y, obs)
        assert len(calls) == (1 if fused else 0)                                  # the decode is fused from 4096 rows on ...
        assert ops.last_form()[0] == "enkf.transform_gram"                        # ... and the transform launch serves both
    ka32 = FieldKalman(decoder("a", "fp32"), P, 64)
    assert ka32._fused_for(torch.zeros(64, G, P * D_)) is False and ka32._native_tail() is True
    assert FieldKalman(dec, P, 64, fused=False)._native_tail() is False


# ------------------------------------------------------------------------------------------------ 6: on a rollout session
def test_analysis_on_a_rollout_session():
    """open_rollout -> fork(n) -> step -> analyse -> step(c, state=y_a) on a forked session: nothing is read back, shapes and dtype are kept, and the
    precision-weighted misfit of the ensemble-mean field drops — in the fp64 restatement and on the device."""
    from sea_amd.ensemble import FieldKalman
    from oracle.recipe import recipe_inputs
    from tests.test_field_enkf_cpu import decode_members, field_weights, restate_field_enkf
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
    conds2 = torch.rand(B * n_mem, 1, generator=g).to(DEV)
    counts = [C_, C_ - 1, 1, C_]
    base = 0.5 + torch.rand(B, P, F, C_, generator=g)
    base[torch.rand(B, P, F, C_, generator=g) < 0.2] = 0.0

    ens = open_on(m, x, ib, kk).fork(n_mem)
    y = ens.step(conds)

    # the CPU side: the snapshot is member 0's exact decoded field (a truth inside the ensemble's span); the precisions are scaled so that
    # trace(C) = 50 per history (cond(I + C) <= 51); the restated analysis must lower the misfit by at least 10 %
    relayout = lambda t: t.reshape(B * n_mem, G, P, D_).permute(0, 2, 1, 3)              # noqa: E731
    fields = lambda yy: decode_members("a", relayout(yy.double()))                       # noqa: E731
    y_host = y.detach().cpu()
    Y0 = fields(y_host)
    Yv = Y0.view(B, n_mem, P, F, C_)
    obs = Yv[:, 0].to(torch.float32)
    w0 = field_weights((B, P, F, C_), None, base, counts)
    anom = Yv - Yv.mean(1, keepdim=True)
    trace = (w0 * (anom * anom).sum(1) / (n_mem - 1)).sum(dim=(1, 2, 3), keepdim=True)
    assert bool((trace > 0).all())
    prec = (base.double() * 50.0 / trace).to(torch.float32)
    w = field_weights((B, P, F, C_), None, prec, counts)
    misfit = lambda YY: float((w * (YY.view(B, n_mem, P, F, C_).mean(1) - obs.double()) ** 2).sum())   # noqa: E731
    r = restate_field_enkf(Y0, obs, w, n_mem, None, 1.0, 0.5)
    y_ref = y_host.double() + restate_mix(y_host, r["D"], P)
    before, after_ref = misfit(Y0), misfit(fields(y_ref))
    print(f"field enkf session: restated misfit of the ensemble-mean field {before:.4f} -> {after_ref:.4f}; cond(I + C) {float(r['cond'].max()):.2f}")
    assert float(r["cond"].max()) <= 1e4 and int(r["status"].min()) > 0 and after_ref <= 0.9 * before

    ka = FieldKalman(dec, P, n_mem, counts=counts, fused=True)
    obs_d, prec_d = obs.to(DEV), prec.to(DEV)
    ka.transform(y, obs_d, prec_d)                                                       # the first call on a device uploads the counts
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                                              # nothing is read back, nothing uploaded after the first call
    try:
        ya = ka.analyse(y, obs_d, prec_d)
        D, status = ka.transform(y, obs_d, prec_d)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert ya.shape == y.shape and ya.dtype == y.dtype and bool(torch.isfinite(ya.float()).all())
    assert torch.equal(status.cpu().long(), r["status"]) and bool(torch.isfinite(D).all())
    after = misfit(fields(ya.detach().cpu()))
    print(f"field enkf session: misfit after the analysis on the device {after:.4f}")
    assert after < before
    y2 = ens.step(conds2, state=ya)                                                       # the session takes the analysed state
    assert y2.shape == y.shape and y2.dtype == y.dtype and bool(torch.isfinite(y2.float()).all())
