"""The ensemble Kalman analysis from a dense snapshot, without a GPU: the fp64 restatement of sea_decode_member_gram and sea_enkf_transform_gram
(include/sea_hip.h) against tests/test_enkf_cpu.py's restatement of the sensor form with every valid cell as a sensor, and against the state-space
Kalman formulas; the inputs of tests/test_field_enkf_gpu.py, their conditioning and their bf16 envelope; patch_taper; the refusals of the Python
layers and of both entry points."""
import ctypes as C
import functools
import math

import pytest
import torch

from tests.test_decode_loss_cpu import rel
from tests.test_enkf_cpu import COND_MAX, restate_enkf, restate_mix
from tests.test_sensor_cpu import host_case, make_decoder, restate_sensor

F64 = torch.float64
ZERO = torch.zeros((), dtype=F64)


# ------------------------------------------------------------------------------------------------ the contract, in fp64
def field_weights(shape, field_precision, precision, counts):
    """w [B, P, F, C] float64 of contract 1: valid ? max(pf, 0) * max(prec, 0) : 0, by selects (a NaN counts as 0)."""
    B, P, F, C_ = shape
    w = torch.ones(B, P, F, C_, dtype=F64)
    if field_precision is not None:
        pf = torch.as_tensor(field_precision, dtype=F64).view(1, 1, F, 1)
        w = w * torch.where(pf > 0, pf, ZERO)
    if precision is not None:
        pm = precision[..., :C_].to(F64)
        w = w * torch.where(pm > 0, pm, ZERO)
    if counts is not None:
        valid = (torch.arange(C_) < torch.tensor(list(counts))[:, None]).view(1, P, 1, C_)
        w = torch.where(valid, w, ZERO)
    return w


def restate_member_gram(Y, obs, w, members):
    """Contract 1 from the decoded members Y [B * N, P, F, C] (float64), obs [B, P, F, >= C], w [B, P, F, C]: (gram [B, P, N, N], proj [B, P, N],
    count [B, P] int64), cell by cell over the live cells only (a cell without weight never enters)."""
    n = members
    Bm, P, F, C_ = Y.shape
    B = Bm // n
    gram, proj, count = torch.zeros(B, P, n, n, dtype=F64), torch.zeros(B, P, n, dtype=F64), torch.zeros(B, P, dtype=torch.int64)
    for b in range(B):
        for p in range(P):
            live = w[b, p] > 0                                                     # [F, C]
            count[b, p] = int(live.sum())
            yl, ol, wl = Y[b * n:(b + 1) * n, p][:, live], obs[b, p][..., :C_].to(F64)[live], w[b, p][live]
            if not (bool(torch.isfinite(yl).all()) and bool(torch.isfinite(ol).all()) and bool(torch.isfinite(wl).all())):
                count[b, p] = -1
                gram[b, p], proj[b, p] = float("nan"), float("nan")
                continue
            ybar = yl.mean(0)
            a = yl - ybar
            gram[b, p] = (a * wl) @ a.t()
            proj[b, p] = (a * wl) @ (ol - ybar)
    return gram, proj, count


def restate_transform_gram(gram, proj, count, taper, rho, alpha):
    """Contract 2 in fp64, problem by problem, with torch.linalg.inv: (D [B, Ld, N, N], status [B, Ld] int64, cond [B, Ld] of I + C)."""
    B, Q, n, _ = gram.shape
    Ld = 1 if taper is None else taper.shape[0]
    D, status, cond = torch.zeros(B, Ld, n, n, dtype=F64), torch.zeros(B, Ld, dtype=torch.int64), torch.ones(B, Ld, dtype=F64)
    eye = torch.eye(n, dtype=F64)
    Pi = eye - 1.0 / n
    for b in range(B):
        for d in range(Ld):
            Cm, v, live, bad = torch.zeros(n, n, dtype=F64), torch.zeros(n, dtype=F64), 0, False
            for q in range(Q):
                t = 1.0 if taper is None else float(taper[d, q])
                if not t > 0 or int(count[b, q]) == 0:
                    continue
                if int(count[b, q]) < 0:
                    bad = True
                    continue
                live += int(count[b, q])
                Cm += t * gram[b, q]
                v += t * proj[b, q]
            Cm, v = Cm * (rho * rho / (n - 1)), v * (rho / math.sqrt(n - 1))
            if bad or not (bool(torch.isfinite(Cm).all()) and bool(torch.isfinite(v).all())):
                status[b, d] = -1
                continue
            status[b, d] = live
            M = eye + Cm
            cond[b, d] = torch.linalg.cond(M)
            W = torch.linalg.inv(M)
            G = (W @ v).unsqueeze(1).expand(n, n) / math.sqrt(n - 1) - alpha * (eye - W)
            D[b, d] = (rho - 1.0) * Pi + rho * (G - G.mean(0, keepdim=True))
    return D, status, cond


def restate_field_enkf(Y, obs, w, members, taper, rho, alpha):
    """Contracts 1 and 2: dict(gram, proj, count, D, status, cond)."""
    gram, proj, count = restate_member_gram(Y, obs, w, members)
    D, status, cond = restate_transform_gram(gram, proj, count, taper, rho, alpha)
    return dict(gram=gram, proj=proj, count=count, D=D, status=status, cond=cond)


def as_sensors(Y, obs, w, taper):
    """Every cell a sensor, in (patch, field, cell) order: (pred [B * N, K], obs [B, K], prec [B, K], taper [Ld, K] or None) for restate_enkf."""
    Bm, P, F, C_ = Y.shape
    B = obs.shape[0]
    tk = None if taper is None else taper.to(F64)[:, :, None].expand(taper.shape[0], P, F * C_).reshape(taper.shape[0], P * F * C_)
    return Y.reshape(Bm, P * F * C_), obs[..., :C_].reshape(B, P * F * C_), w.reshape(B, P * F * C_), tk


def decode_members(name, z, round_bf16=False):
    """The decoder of a shape on z [Bm, P, G, D] in fp64 (tests/test_sensor_cpu.restate_sensor with every cell a sensor): Y [Bm, P, F, C]."""
    c = host_case(name)
    Bm, P = z.shape[:2]
    flat = [f for g in c["groups"] for f in g]
    F, C_ = len(flat), c["n_inp"]
    patch = [p for p in range(P) for _ in range(F * C_)]
    field = [f for _ in range(P) for f in flat for _ in range(C_)]
    cell = [k for _ in range(P * F) for k in range(C_)]
    _, pred = restate_sensor(c["w1"], c["w2"], c["b2"], c["groups"], z, patch, cell, field, torch.zeros(1, len(patch)), None, Bm, round_bf16=round_bf16)
    return pred.view(Bm, P, F, C_)


# ------------------------------------------------------------------------------------------------ the inputs of the GPU test
# sigma per shape: a dense snapshot makes C = rho^2 / (N - 1) sum w a a^T large — its largest eigenvalue is about (cells) * (spread / sigma)^2 — so the error
# of one cell is set to a few times the member spread; test_inputs_are_well_conditioned holds every input to cond(I + C) <= 1e4
SIGMA = {"a": 3.0, "b": 3.0, "c": 3.0}
MEMBERS_A = (2, 5, 17, 64, 128)
OWN_SPLITS = {"b": ((11, 3), (33, 1)), "c": ((5, 7), (35, 1))}


def ragged_counts(name, members):
    """0, 1, C - 1, C over the patches; shape c has two patches, so its two splits take one half each."""
    c = host_case(name)
    C_, P = c["n_inp"], c["P"]
    if name == "c":
        return [1, C_ - 1] if members == 5 else [0, C_]
    return ([0, 1, C_ - 1, C_] * P)[:P]


def field_cases():
    """(shape, members, histories, ragged counts, precision map, local)."""
    out = []
    for m in MEMBERS_A:
        for h in (1, 3):
            for cnt in (False, True):
                for wp in (False, True):
                    out.append(("a", m, h, cnt, wp, (m + h + cnt + wp) % 2 == 1))
    for name in ("b", "c"):
        for m, h in OWN_SPLITS[name]:
            for cnt in (False, True):
                for wp in (False, True):
                    out.append((name, m, h, cnt, wp, (m + cnt + wp) % 2 == 0))
    return out


@functools.lru_cache(maxsize=None)
def field_states(name, members, hist, dtype="bf16"):
    """y [Bm, G, P * D] in the act dtype (bf16: rounded once, here) and z float64 [Bm, P, G, D]: the shape's own states for b and c, fresh ones on a."""
    c = host_case(name)
    P, G, D_ = c["P"], len(c["groups"]), c["D"]
    if name == "a":
        z0 = torch.randn(hist * members, P, G, D_, generator=torch.Generator().manual_seed(9000 + 10 * members + hist))
    else:
        z0 = c["z"][:hist * members]
    Bm = z0.shape[0]
    assert Bm == hist * members
    y = z0.permute(0, 2, 1, 3).reshape(Bm, G, P * D_).contiguous()
    y = y.to(torch.bfloat16) if dtype == "bf16" else y.clone()
    return y, y.to(F64).view(Bm, G, P, D_).permute(0, 2, 1, 3).contiguous()


@functools.lru_cache(maxsize=None)
def decoded(name, members, hist, dtype="bf16", round_bf16=False):
    return decode_members(name, field_states(name, members, hist, dtype)[1], round_bf16=round_bf16)


@functools.lru_cache(maxsize=None)
def field_case(name, members, hist, with_counts, with_prec, local, dtype="bf16"):
    """An end-to-end input and its fp64 restatement: dict(y, z, obs, prec, counts, sigma, taper, rho, alpha, Y, w, gram, proj, count, D, status, cond, inc).
    obs: random normal around the decoded values' scale; with_prec: a map in [0.25, 2] with a tenth of the cells missing (precision 0, obs NaN there);
    local: a [P, P] taper in [0, 1] with a third of its entries 0 and row 1 all zero."""
    c = host_case(name)
    P, C_ = c["P"], c["n_inp"]
    F = sum(len(g) for g in c["groups"])
    g = torch.Generator().manual_seed(70000 + 100 * members + 10 * hist + 4 * with_counts + 2 * with_prec + local + ord(name))
    y, z = field_states(name, members, hist, dtype)
    Y = decoded(name, members, hist, dtype)
    obs = Y.view(hist, members, P, F, C_).mean(1).to(torch.float32) + torch.randn(hist, P, F, C_, generator=g)
    prec = None
    if with_prec:
        prec = 0.25 + 1.75 * torch.rand(hist, P, F, C_, generator=g)
        miss = torch.rand(hist, P, F, C_, generator=g) < 0.1
        prec[miss] = 0.0
        obs[miss] = float("nan")
    counts = ragged_counts(name, members) if with_counts else None
    taper = None
    if local:
        taper = torch.rand(P, P, generator=g)
        taper[torch.rand(P, P, generator=g) < 1.0 / 3.0] = 0.0
        taper[1] = 0.0
    sigma = SIGMA[name]
    rho, alpha = (1.05, 0.5) if members % 2 else (1.0, 0.5)
    w = field_weights((hist, P, F, C_), [1.0 / sigma ** 2] * F, prec, counts)
    r = restate_field_enkf(Y, obs, w, members, taper, rho, alpha)
    r.update(y=y, z=z, obs=obs, prec=prec, counts=counts, sigma=sigma, taper=taper, rho=rho, alpha=alpha, Y=Y, w=w, inc=restate_mix(y, r["D"], P))
    return r


@functools.lru_cache(maxsize=None)
def field_envelope():
    """The largest relative L2 error of the increment, over the end-to-end inputs, that decoder operands rounded to bf16 cause on their own."""
    worst = 0.0
    for name, members, hist, cnt, wp, local in field_cases():
        k = field_case(name, members, hist, cnt, wp, local)
        if float(k["inc"].abs().max()) == 0.0:
            continue
        Yr = decoded(name, members, hist, "bf16", True)
        r = restate_field_enkf(Yr, k["obs"], k["w"], members, k["taper"], k["rho"], k["alpha"])
        e = rel(restate_mix(k["y"], r["D"], host_case(name)["P"]), k["inc"])
        print(f"field enkf shape {name} members {members} x {hist} counts {cnt} prec {wp} local {local}: bf16 operands e(inc) {e:.3e} cond {float(k['cond'].max()):.3e}")
        worst = max(worst, e)
    print(f"field enkf bf16 envelope: {worst:.3e}")
    return worst


# ------------------------------------------------------------------------------------------------ the restatement against the sensor form
def synthetic(n, B, P, F, C_, with_counts, with_prec, seed):
    g = torch.Generator().manual_seed(seed)
    Y = torch.randn(B * n, P, F, C_, generator=g, dtype=F64)
    obs = torch.randn(B, P, F, C_ + 1, generator=g, dtype=F64)
    prec = None
    if with_prec:
        prec = 0.25 + 2.0 * torch.rand(B, P, F, C_ + 1, generator=g, dtype=F64)
        miss = torch.rand(B, P, F, C_ + 1, generator=g) < 0.2
        prec[miss] = 0.0
        obs[miss] = float("nan")
    counts = ([0, 1, C_ - 1, C_] * P)[:P] if with_counts else None
    return Y, obs, prec, counts


@pytest.mark.parametrize("n", [2, 5, 64])
@pytest.mark.parametrize("rho", [1.0, 1.1])
@pytest.mark.parametrize("with_counts", [False, True])
@pytest.mark.parametrize("with_prec", [False, True])
def test_gram_form_is_the_sensor_form_with_every_valid_cell_a_sensor(n, rho, with_counts, with_prec):
    B, P, F, C_ = 2, 4, 2, 7
    Y, obs, prec, counts = synthetic(n, B, P, F, C_, with_counts, with_prec, 11 * n + int(10 * rho) + 2 * with_counts + with_prec)
    w = field_weights((B, P, F, C_), [0.5, 0.125], prec, counts)
    g = torch.Generator().manual_seed(5 + n)
    T = torch.rand(P, P, generator=g, dtype=F64)
    T[torch.rand(P, P, generator=g) < 0.3] = 0.0
    T[2] = 0.0                                                                    # a domain that sees nothing
    Pi = torch.eye(n, dtype=F64) - 1.0 / n
    for taper in (None, T):
        r = restate_field_enkf(Y, obs, w, n, taper, rho, 0.5)
        pred, ok, pk, tk = as_sensors(Y, obs, w, taper)
        D_ref, status_ref, _ = restate_enkf(pred, ok, pk, tk, n, rho, 0.5)
        assert torch.equal(r["status"], status_ref)
        assert float((r["D"] - D_ref).abs().max()) <= 1e-10, (n, rho, taper is None)
        assert int(r["status"].min()) >= 0
        assert torch.equal(r["gram"], r["gram"].transpose(-1, -2)) or float((r["gram"] - r["gram"].transpose(-1, -2)).abs().max()) <= 1e-12
        if taper is not None:
            assert int(r["status"][0, 2]) == 0
            assert torch.equal(r["D"][:, 2], ((rho - 1.0) * Pi).expand(B, n, n))  # exactly (rho - 1) Pi
        if with_counts:
            assert int(r["count"][0, 0]) == 0 and int(r["count"][0, 3]) > 0


def test_a_nan_at_a_live_cell_marks_its_patch_alone():
    n, B, P, F, C_ = 5, 2, 3, 2, 6
    Y, obs, _, _ = synthetic(n, B, P, F, C_, False, False, 3)
    w = field_weights((B, P, F, C_), None, None, None)
    Y[n + 2, 1, 0, 3] = float("nan")                                              # member 2 of history 1, patch 1
    T = torch.eye(P, dtype=F64)
    r = restate_field_enkf(Y, obs, w, n, T, 1.0, 0.5)
    assert r["count"].tolist() == [[F * C_] * P, [F * C_, -1, F * C_]]
    assert r["status"].tolist() == [[F * C_] * P, [F * C_, -1, F * C_]]
    assert float(r["D"][1, 1].abs().max()) == 0.0 and float(r["D"][1, 0].abs().max()) > 0.0
    r1 = restate_field_enkf(Y, obs, w, n, None, 1.0, 0.5)
    assert r1["status"].tolist() == [[P * F * C_], [-1]]


@pytest.mark.parametrize("n", [2, 5, 64])
@pytest.mark.parametrize("rho", [1.0, 1.1])
def test_gram_form_is_the_state_space_analysis_for_a_linear_decoder(n, rho):
    g = torch.Generator().manual_seed(17 * n + int(10 * rho))
    n_state, P, F, C_ = 30, 3, 2, 4
    K = P * F * C_
    for alpha in (0.5, 0.0, 1.0):
        X = torch.randn(n_state, n, generator=g, dtype=F64)
        H = torch.randn(K, n_state, generator=g, dtype=F64) / math.sqrt(n_state)
        obs = torch.randn(1, P, F, C_, generator=g, dtype=F64)
        prec = 0.25 + 2.0 * torch.rand(1, P, F, C_, generator=g, dtype=F64)
        prec[torch.rand(1, P, F, C_, generator=g) < 0.25] = 0.0
        prec[0, 0, 0, 0] = 1.0
        Y = (H @ X).t().contiguous().view(n, P, F, C_)
        w = field_weights((1, P, F, C_), None, prec, None)
        r = restate_field_enkf(Y, obs, w, n, None, rho, alpha)
        D = r["D"][0, 0]
        assert int(r["status"][0, 0]) == int((prec > 0).sum())
        Xa = X + X @ D
        live = (prec > 0).reshape(K)
        Hl, R = H[live], torch.diag(1.0 / prec.reshape(K)[live])
        xbar = X.mean(1, keepdim=True)
        A = rho * (X - xbar)
        Pf = A @ A.t() / (n - 1)
        Kg = Pf @ Hl.t() @ torch.linalg.inv(Hl @ Pf @ Hl.t() + R)
        mean_a = xbar[:, 0] + Kg @ (obs.reshape(K)[live] - Hl @ xbar[:, 0])
        anom_a = A - alpha * Kg @ Hl @ A
        assert float((Xa.mean(1) - mean_a).abs().max()) <= 1e-10, (n, rho, alpha)
        assert float((Xa - Xa.mean(1, keepdim=True) - anom_a).abs().max()) <= 1e-10, (n, rho, alpha)


# ------------------------------------------------------------------------------------------------ the GPU inputs
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_inputs_are_well_conditioned(name):
    worst = 0.0
    for nm, members, hist, cnt, wp, local in field_cases():
        if nm != name:
            continue
        k = field_case(nm, members, hist, cnt, wp, local)
        cond = float(k["cond"].max())
        worst = max(worst, cond)
        assert cond <= COND_MAX, (nm, members, hist, cnt, wp, local, cond)
        assert int(k["status"].min()) >= 0 and int(k["count"].min()) >= 0
        c = host_case(nm)
        Yv = k["Y"].view(hist, members, *k["Y"].shape[1:])
        spread, size = float(Yv.std(dim=1, unbiased=False).square().mean().sqrt()), float(k["Y"].square().mean().sqrt())
        assert 0.1 * size <= spread <= 10.0 * size, (nm, members, spread, size)    # the members differ by about as much as the fields are large
        if local:
            assert int(k["status"][:, 1].max()) == 0 and (k["rho"] != 1.0 or float(k["D"][:, 1].abs().max()) == 0.0)      # the all-zero row of the taper
        assert c["P"] == k["obs"].shape[1]
    print(f"field enkf shape {name}: largest cond(I + C) {worst:.3e}")


def test_the_bf16_envelope_of_the_increment():
    e = field_envelope()
    assert 0.0 < e <= 2e-2            # what bf16 operands cost on their own stays below the bf16 decode tolerance: the GPU bound measures the kernel


# ------------------------------------------------------------------------------------------------ patch_taper
def test_patch_taper_on_the_synthetic_mesh():
    from sea_amd.ensemble import gaspari_cohn
    from sea_amd.models.encoder_decoder import Decode
    from sea_amd.utils.data_processors import DataPartitioner2D, MeshProcessor, MeshUnpatcher
    from tests.conftest import load_golden

    gld = load_golden("unpatch_5x5")
    m, n = (int(v) for v in gld["mn"])
    xy = torch.from_numpy(gld["xy"]).clone()
    part = DataPartitioner2D(xy[0], xy[1], m=m, n=n, device="cpu")
    P, C_ = part.padded_index_map.shape
    groups = [[0, 1], [2]]
    mesh = MeshUnpatcher(part, groups)
    radius = 0.3 * float(xy[0].max() - xy[0].min())
    t = mesh.patch_taper(radius)
    assert t.shape == (P, P) and t.dtype == torch.float32 and t.is_contiguous() and bool((t >= 0).all()) and bool((t <= 1).all())
    idx = part.padded_index_map.long()
    cen = torch.stack([part.full_coords[idx[p][idx[p] >= 0]].mean(0) for p in range(P)])
    direct = gaspari_cohn((cen[:, None, :] - cen[None, :, :]).norm(dim=-1), radius)
    assert float((t - direct).abs().max()) <= 1e-6
    assert float((t.diagonal() - 1.0).abs().max()) <= 1e-6 and torch.equal(t, t.t()) and float(t[0, P - 1]) == 0.0
    # sensor_taper's results are what they were: the definition, patch by patch (tests/test_enkf_cpu.py holds the rest)
    dec = Decode(groups, C_, 16, 8)
    imap0 = torch.from_numpy(gld["index_map"])
    points = [int(imap0[0, 0]), int(imap0[24, 0]), int(imap0[12, 3])]
    s = mesh.sensor_set(dec, points, [0, 2, 1])
    ts = mesh.sensor_taper(s, radius)
    for p in (0, 7, 24):
        dist = (part.full_coords[torch.tensor(points)] - cen[p]).norm(dim=1)
        assert float((ts[p] - gaspari_cohn(dist, radius)).abs().max()) <= 1e-6
    for bad in (0.0, -1.0, None):
        with pytest.raises(ValueError):
            mesh.patch_taper(bad)
    proc = MeshProcessor(dict(dimension="2D", field_groups=groups, m=m, n=n), xy, device="cpu")
    with pytest.raises(ValueError, match="patchify_and_scale first"):
        proc.patch_taper(radius)


# ------------------------------------------------------------------------------------------------ refusals of the Python layers
def test_python_layers_refuse_before_a_device_is_touched():
    from sea_amd import ops
    from sea_amd.ensemble import FieldKalman
    from sea_amd.utils.train_utils import FieldKalman as FK2

    assert FK2 is FieldKalman
    c = host_case("a")
    dec = make_decoder("a").set_compute_dtype("bf16")
    P, D_, G, C_ = c["P"], c["D"], len(c["groups"]), c["n_inp"]
    F = sum(len(g) for g in c["groups"])
    for members in (1, 129, 0, True, 2.0):
        with pytest.raises(ValueError):
            FieldKalman(dec, P, members)
    for kw in (dict(inflation=0.9), dict(inflation=float("inf")), dict(anomaly_gain=-0.1), dict(anomaly_gain=1.1), dict(taper=torch.ones(P, P + 1)),
               dict(taper=torch.ones(P)), dict(taper=torch.full((P, P), 2.0)), dict(taper=torch.ones(P, P, dtype=torch.int32)), dict(sigma=-1.0),
               dict(sigma=[1.0, 2.0]), dict(layout="PBFC"), dict(fused="yes")):
        with pytest.raises(ValueError):
            FieldKalman(dec, P, 2, **kw)
    with pytest.raises(ValueError):
        FieldKalman(dec, 0, 2)
    ka = FieldKalman(dec, P, 2, sigma=[0.5, 1.0, 2.0][:F] if F <= 3 else 1.0, inflation=1.05, taper=torch.ones(P, P), fused=True)
    if F == 3:
        assert ka._prec_host == [4.0, 1.0, 0.25]
    y, obs = torch.zeros(4, G, P * D_), torch.zeros(2, P, F, C_)
    for yy, oo, pp in ((torch.zeros(3, G, P * D_), obs, None), (torch.zeros(4, G, P * D_ + 1), obs, None), (y, torch.zeros(2, P + 1, F, C_), None), (y, obs.double(), None),
                       (y, obs[0], None), (y, obs, torch.ones(2, P, F, C_ + 1)), (y, obs, -torch.ones(2, P, F, C_)), (y, obs, torch.ones(2, P, F, C_).double())):
        with pytest.raises(ValueError):
            ka.analyse(yy, oo, pp)
    with pytest.raises(RuntimeError, match="MI355X"):
        ka.analyse(y, obs)
    z = torch.zeros(4, P, G, D_)
    for kw in (dict(members=1), dict(members=129), dict(members=3), dict(obs=torch.zeros(2, P, F, C_ - 1)), dict(obs=obs.double()), dict(precision=torch.ones(2, P, F, C_ + 4)),
               dict(field_precision=torch.ones(F + 1)), dict(z=torch.zeros(4, P, G + 1, D_))):
        args = dict(z=z, obs=obs, members=2)
        args.update(kw)
        with pytest.raises(ValueError):
            dec.member_gram(**args)
    with pytest.raises(ValueError, match="bf16 only"):
        make_decoder("a").member_gram(z, obs, 2, fused=True)
    gram, proj, count = torch.zeros(2, P, 2, 2, dtype=F64), torch.zeros(2, P, 2, dtype=F64), torch.zeros(2, P, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.enkf_transform_gram(gram, proj, count)
    for kw in (dict(gram=gram.float()), dict(gram=torch.zeros(2, P, 2, 3, dtype=F64)), dict(proj=proj[:, :, :1]), dict(count=count.long()), dict(taper=torch.ones(2, P + 1)),
               dict(taper=torch.ones(P, P, dtype=F64)), dict(rho=0.5), dict(alpha=1.5), dict(gram=torch.zeros(2, P, 129, 129, dtype=F64))):
        args = dict(gram=gram, proj=proj, count=count)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.enkf_transform_gram(**args)


# ------------------------------------------------------------------------------------------------ the entry points without a device
@pytest.fixture(scope="module")
def lib():
    from sea_amd import build, _native

    build.build(verbose=False)
    return _native.lib()


def _gram_tables(n_groups=2):
    """A well-formed sea_decode_member_gram table over made-up (aligned, never dereferenced) addresses: shape a, 4 members of 2 histories."""
    from sea_amd import _native as N

    arr, p = (N.SeaDecodeMseGroup * n_groups)(), N.SeaDecodeMemberGram()
    for g in range(n_groups):
        arr[g].H, arr[g].W2, arr[g].bias = 0x100000 + 0x10000 * g, 0x200000 + 0x10000 * g, 0x300000 + 0x10000 * g
        arr[g].ldh, arr[g].ldw, arr[g].n_fields, arr[g].field0 = 40, 40, 2 if g == 0 else 1, 0 if g == 0 else 2
    p.obs, p.prec_field, p.prec, p.counts, p.gram, p.proj, p.count = 0x400000, 0x410000, 0x420000, 0x430000, 0x440000, 0x450000, 0x460000
    p.ld_row, p.ld_field, p.ld_prow, p.ld_pfield = 3 * 24, 24, 3 * 24, 24
    p.M, p.S, p.C, p.Cp, p.P, p.members, p.n_fields_total = 2 * 4 * 9, 40, 21, 32, 9, 4, 3
    return arr, p


def _tgram_table():
    from sea_amd import _native as N

    p = N.SeaEnkfTransformGram()
    p.gram, p.proj, p.count, p.taper, p.D, p.status = 0x100000, 0x110000, 0x120000, 0x130000, 0x140000, 0x150000
    p.ld_taper, p.rho, p.alpha = 9, 1.0, 0.5
    p.B, p.N, p.Q, p.Ld = 2, 8, 9, 9
    return p


def test_symbols_and_struct_layouts(lib):
    from sea_amd import _native as N

    for name in ("sea_decode_member_gram", "sea_enkf_transform_gram"):
        assert hasattr(lib, name) and name in N.EXPORTED_SYMBOLS
    assert C.sizeof(N.SeaDecodeMemberGram) == 120 and C.sizeof(N.SeaEnkfTransformGram) == 88            # include/sea_hip.h states them
    assert N.SeaDecodeMemberGram.ld_row.offset == 56 and N.SeaDecodeMemberGram.M.offset == 88 and N.SeaDecodeMemberGram.members.offset == 108
    assert N.SeaEnkfTransformGram.ld_taper.offset == 48 and N.SeaEnkfTransformGram.rho.offset == 56 and N.SeaEnkfTransformGram.B.offset == 72
    assert lib.sea_abi_version() == 8 and len(N.ABI_STRUCTS) == 33 and N.ABI_STRUCTS[-1] is N.SeaKvFork
    # the library reads the fields where the binding writes them: its messages quote the values back
    arr, p = _gram_tables()
    p.members = 1
    assert lib.sea_decode_member_gram(arr, 2, C.byref(p), N.SEA_BF16, None) == -1 and b"members=1" in lib.sea_last_error()
    arr, p = _gram_tables()
    p.ld_pfield = 20
    assert lib.sea_decode_member_gram(arr, 2, C.byref(p), N.SEA_BF16, None) == -1 and b"ld_pfield=20 must cover C=21" in lib.sea_last_error()
    arr, p = _gram_tables()
    p.M = 71
    assert lib.sea_decode_member_gram(arr, 2, C.byref(p), N.SEA_BF16, None) == -1 and b"M=71 is not a multiple of P * members = 9 * 4" in lib.sea_last_error()
    p = _tgram_table()
    p.ld_taper = 8
    assert lib.sea_enkf_transform_gram(C.byref(p), None) == -1 and b"ld_taper=8 must cover Q=9" in lib.sea_last_error()
    p = _tgram_table()
    p.rho = 0.5
    assert lib.sea_enkf_transform_gram(C.byref(p), None) == -1 and b"rho=0.5" in lib.sea_last_error()


G_BREAKS = {"null obs": ("obs", None), "null gram": ("gram", None), "null proj": ("proj", None), "null count": ("count", None), "misaligned obs": ("obs", 0x400002),
            "misaligned prec": ("prec", 0x420001), "misaligned gram": ("gram", 0x440004), "misaligned proj": ("proj", 0x450004), "misaligned count": ("count", 0x460002),
            "members = 1": ("members", 1), "M = 0": ("M", 0), "M not a multiple": ("M", 70), "S odd": ("S", 36), "Cp = 40": ("Cp", 40), "C above Cp": ("C", 33),
            "C = 0": ("C", 0), "P = 0": ("P", 0), "ld_field short": ("ld_field", 20), "ld_pfield short": ("ld_pfield", 20), "fields": ("n_fields_total", 4)}


@pytest.mark.parametrize("what", sorted(G_BREAKS) + ["bad dtype", "no groups", "group null", "group overlap", "ldh short"])
def test_member_gram_refuses_bad_arguments_without_a_device(lib, what):
    from sea_amd import _native as N

    arr, p = _gram_tables()
    dt, ng = N.SEA_BF16, 2
    if what in G_BREAKS:
        setattr(p, *G_BREAKS[what])
    elif what == "bad dtype":
        dt = 5
    elif what == "no groups":
        ng = 0
    elif what == "group null":
        arr[1].W2 = None
    elif what == "group overlap":
        arr[1].field0 = 1
    else:
        arr[0].ldh = 32
    assert lib.sea_decode_member_gram(arr, ng, C.byref(p), dt, None) == -1, what
    assert b"sea_decode_member_gram" in lib.sea_last_error()


T_BREAKS = {"null gram": ("gram", None), "null proj": ("proj", None), "null count": ("count", None), "null D": ("D", None), "null status": ("status", None),
            "misaligned gram": ("gram", 0x100004), "misaligned taper": ("taper", 0x130001), "N = 1": ("N", 1), "Q = 0": ("Q", 0), "B = 0": ("B", 0), "Ld = 0": ("Ld", 0),
            "domains without a taper": ("taper", None), "ld_taper short": ("ld_taper", 8), "rho below 1": ("rho", 0.99), "rho nan": ("rho", float("nan")),
            "rho inf": ("rho", float("inf")), "alpha above 1": ("alpha", 1.5), "alpha negative": ("alpha", -0.1)}


@pytest.mark.parametrize("what", sorted(T_BREAKS))
def test_transform_gram_refuses_bad_arguments_without_a_device(lib, what):
    p = _tgram_table()
    setattr(p, *T_BREAKS[what])
    assert lib.sea_enkf_transform_gram(C.byref(p), None) == -1, what
    assert b"sea_enkf_transform_gram" in lib.sea_last_error()


def test_unsupported_forms_and_null_tables(lib):
    from sea_amd import _native as N

    arr, p = _gram_tables()
    assert lib.sea_decode_member_gram(arr, 2, C.byref(p), N.SEA_F32, None) == -3 and b"sea_decode_member_gram" in lib.sea_last_error()
    arr, p = _gram_tables()
    p.S = 648
    for g in range(2):
        arr[g].ldh = arr[g].ldw = 648
    assert lib.sea_decode_member_gram(arr, 2, C.byref(p), N.SEA_BF16, None) == -3 and b"S=648" in lib.sea_last_error()
    arr, p = _gram_tables()
    p.members, p.M = 129, 2 * 129 * 9
    assert lib.sea_decode_member_gram(arr, 2, C.byref(p), N.SEA_BF16, None) == -3 and b"members=129" in lib.sea_last_error()
    assert lib.sea_decode_member_gram(None, 2, C.byref(p), N.SEA_BF16, None) == -1 and lib.sea_decode_member_gram(arr, 2, None, N.SEA_BF16, None) == -1
    p = _tgram_table()
    p.N = 129
    assert lib.sea_enkf_transform_gram(C.byref(p), None) == -3 and b"N=129" in lib.sea_last_error()
    assert lib.sea_enkf_transform_gram(None, None) == -1 and b"sea_enkf_transform_gram" in lib.sea_last_error()
    # prec_field, prec, counts and the taper (one domain) may be NULL: such tables pass the pointer checks and fail only at the check this test breaks
    arr, p = _gram_tables()
    p.prec_field = p.prec = p.counts = None
    p.members, p.M = 129, 2 * 129 * 9
    assert lib.sea_decode_member_gram(arr, 2, C.byref(p), N.SEA_BF16, None) == -3
    p = _tgram_table()
    p.taper, p.Ld, p.alpha = None, 1, 2.0
    assert lib.sea_enkf_transform_gram(C.byref(p), None) == -1 and b"alpha=2" in lib.sea_last_error()
    from sea_amd import ops

    assert ops.last_form() == ("", 0, 0) or ops.last_form()[0] not in ("decode.member_gram", "enkf.transform_gram")   # a refused call notes nothing
