"""Dense-snapshot score with a precision map and its latent gradient (sea_decode_field_grad, Decode.field_loss, FieldLikelihood.score_and_grad / nudge)
without a GPU: the contract restated in fp64 agrees with torch.autograd and, without weights, with the decoded-field loss the reference fixtures pin
(tests/test_decode_loss_cpu.restate on tests/golden/decode_mse_*.npz); the entry point is exported and checks its arguments before touching a device;
the Python layers refuse malformed arguments, CPU tensors and a trainable decoder.

`restate_field_grad`, `precision_map`, `field_precision_of`, `SPLITS` and `per_member_rel` below are what tests/test_field_grad_gpu.py compares with."""
import ctypes as C
import functools
import math

import pytest
import torch

from tests.test_decode_loss_cpu import load_fixture, rel, restate

TOL_BF16 = 2e-2          # the project's bf16 decode tolerance (tests/test_decode_loss_gpu.py)
MIN_LIVE = 16            # per-member comparisons need this many weighted cells per compared sum (per_member_rel states why)
COUNTS_C2 = [1, 159]
SPLITS = {"a": [(2, 1), (1, 2)], "b": [(33, 1), (11, 3), (3, 11), (1, 33)], "c": [(35, 1), (7, 5), (5, 7), (1, 35)]}   # (members, histories): every split that divides B


# ------------------------------------------------------------------------------------------------ the contract, in fp64
def _weights_fp64(obs, precision, field_precision, counts, members, Bm, P, F, C_):
    """(w [M, F, C], observation rows [M, F, C]) of include/sea_hip.h, sea_decode_field_grad: rows through trow(m), the weight by selects."""
    f64 = torch.float64
    B, M = Bm // members, Bm * P
    rows = torch.arange(M)
    mem, patch = rows // P, rows % P
    trow = (mem // members) * P + patch
    ob = obs.detach().to(f64)[..., :C_].reshape(B * P, F, C_)[trow]
    pw = torch.ones(M, F, C_, dtype=f64) if precision is None else precision.detach().to(f64)[..., :C_].reshape(B * P, F, C_)[trow]
    fw = torch.ones(F, dtype=f64) if field_precision is None else torch.as_tensor(field_precision).detach().to(f64)
    fw = fw.view(1, F, 1)
    if counts is None:
        valid = torch.ones(M, 1, C_, dtype=torch.bool)
    else:
        cnt = torch.as_tensor(counts).clamp(0, C_)
        valid = (torch.arange(C_) < cnt[patch, None]).view(M, 1, C_)
    live = valid & (pw > 0) & (fw > 0)                                   # NaN compares false
    return torch.where(live, fw * pw, torch.zeros((), dtype=f64)), ob


def restate_field_grad(w1, w2, b2, groups, z, obs, precision, field_precision, counts, members, cell_weights=None):
    """include/sea_hip.h, sea_decode_field_grad, with the two small ends around it, in fp64 and without autograd.
    w1[g] [S, D], w2[g] [n_g * C, S], b2[g] [n_g * C]; z [Bm, P, G, D]; obs, precision [Bm / members, P, F, >= C]; field_precision F numbers or None;
    counts P integers or None.  cell_weights: a [M, F, C] fp64 tensor that REPLACES the weights (tests that plant a wrong weight).
    Returns (wsse [Bm, F], dz [Bm, P, G, D])."""
    f64 = torch.float64
    Bm, P, G, D = z.shape
    M = Bm * P
    n_f = [len(g) for g in groups]
    F = sum(n_f)
    C_ = w2[0].shape[0] // n_f[0]
    w, ob = _weights_fp64(obs, precision, field_precision, counts, members, Bm, P, F, C_)
    if cell_weights is not None:
        w = cell_weights
    zz = z.detach().to(f64).reshape(M, G, D)
    rows = torch.zeros(M, F, dtype=f64)
    dz = torch.empty(M, G, D, dtype=f64)
    f0 = 0
    for g in range(G):
        pre = zz[:, g] @ w1[g].to(f64).t()
        H = 0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0)))
        Y = (H @ w2[g].to(f64).t() + b2[g].to(f64)).view(M, n_f[g], C_)
        wg = w[:, f0:f0 + n_f[g]]
        d = torch.where(wg > 0, Y - ob[:, f0:f0 + n_f[g]], torch.zeros((), dtype=f64))
        rows[:, f0:f0 + n_f[g]] = (wg * d * d).sum(-1)
        dH = 2.0 * (wg * d).reshape(M, -1) @ w2[g].to(f64)
        gelu_grad = 0.5 * (1.0 + torch.erf(pre / math.sqrt(2.0))) + pre * torch.exp(-0.5 * pre * pre) / math.sqrt(2.0 * math.pi)
        dz[:, g] = (dH * gelu_grad) @ w1[g].to(f64)
        f0 += n_f[g]
    return rows.view(Bm, P, F).sum(1), dz.view(Bm, P, G, D)


def live_cells(obs, precision, field_precision, counts, members, Bm, P, groups, C_):
    """Weighted cells per (member, field) and per (member, patch, group): what decides which members a per-member comparison may use."""
    F = sum(len(g) for g in groups)
    w, _ = _weights_fp64(obs, precision, field_precision, counts, members, Bm, P, F, C_)
    n = (w > 0).view(Bm, P, F, C_)
    per_field = n.sum(dim=(1, 3))
    per_group, f0 = [], 0
    for grp in groups:
        per_group.append(n[:, :, f0:f0 + len(grp)].sum(dim=(2, 3)))
        f0 += len(grp)
    return per_field, torch.stack(per_group, 2)                          # [Bm, F], [Bm, P, G]


def per_member_rel(got, ref, enough):
    """The largest relative L2 error of a member's own row block against its reference, over the members with `enough` (bool [Bm]).
    A member's sums over a handful of cells are no measure of a bf16 kernel: y - obs cancels, and the relative error of ONE residual is
    (rounding of y) / |y - obs|, unbounded as the cell happens to fit.  Over MIN_LIVE = 16 cells the sums are dominated by residuals of the size of
    the fields themselves (obs and y are both O(1) here), and the error is the 2^-9 of the bf16 operands times a small factor.  Members below
    that are still covered by the whole-tensor bounds and by the bit-exact neutrality and independence tests."""
    worst = 0.0
    for m in torch.nonzero(enough).flatten().tolist():
        worst = max(worst, rel(got[m], ref[m]))
    return worst


# ------------------------------------------------------------------------------------------------ cases shared with the GPU tests
@functools.lru_cache(maxsize=None)
def host_case(name):
    """Shapes a, b, c of tests/test_decode_loss_gpu.case, rebuilt here so that this file imports no module marked gpu."""
    if name in ("a", "b"):
        fx = load_fixture("decode_mse_" + name)
        return dict(groups=fx["groups"], n_inp=fx["n_inp"], hidden=fx["hidden"], D=fx["D"], B=fx["B"], P=fx["P"], w1=fx["w1"], w2=fx["w2"], b2=fx["b2"],
                    z=fx["z"], target=fx["target"], counts=fx["counts"].tolist())
    g = torch.Generator().manual_seed(23)
    groups, n_inp, hidden, D, B, P = [[0, 1]], 160, 624, 32, 35, 2
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale  # noqa: E731
    return dict(groups=groups, n_inp=n_inp, hidden=hidden, D=D, B=B, P=P, w1=[rn(hidden, D, scale=2.0 / math.sqrt(D))], w2=[rn(2 * n_inp, hidden, scale=2.0 / math.sqrt(hidden))],
                b2=[rn(2 * n_inp, scale=0.1)], z=rn(B, P, 1, D), target=rn(B, P, 2, n_inp), counts=[0, 160])


def counts_sets(name):
    return [None, host_case(name)["counts"]] + ([COUNTS_C2] if name == "c" else [])


def snapshot(name, hist):
    """The observation of a split with `hist` histories: the first `hist` snapshots of the case's target (history h of any split sees target[h])."""
    return host_case(name)["target"][:hist].contiguous()


def field_precision_of(name):
    """Field 1 switched off, the others weighted unequally."""
    F = sum(len(g) for g in host_case(name)["groups"])
    return torch.tensor([1.5, 0.0, 0.5][:F])


@functools.lru_cache(maxsize=None)
def precision_map(name, hist):
    """A seeded precision map [hist, P, F, C]: values in [0.25, 4], about 30 % exact zeros, the whole patch (history 0, patch 0) zero, and in one block
    (history hist - 1, patch P - 1, one field) the last column alone live.  That block sits in field 0 — except with one history and two patches
    (shape c, one history), where field 0 of patch 1 is the only block counts [0, 160] and field_precision leave alive: it sits in field 1 there, live
    in the runs without a field precision."""
    c = host_case(name)
    P, C_ = c["P"], c["n_inp"]
    F = sum(len(g) for g in c["groups"])
    g = torch.Generator().manual_seed(1000 * hist + {"a": 1, "b": 2, "c": 3}[name])
    pm = 0.25 + 3.75 * torch.rand(hist, P, F, C_, generator=g)
    pm[torch.rand(hist, P, F, C_, generator=g) < 0.3] = 0.0
    pm[0, 0] = 0.0
    f_last = 1 if (hist == 1 and P == 2) else 0
    pm[hist - 1, P - 1, f_last] = 0.0
    pm[hist - 1, P - 1, f_last, C_ - 1] = 2.0
    return pm


def all_cases():
    for name in ("a", "b", "c"):
        for members, hist in SPLITS[name]:
            for counts in counts_sets(name):
                for with_fp in (False, True):
                    yield name, members, hist, counts, with_fp


@functools.lru_cache(maxsize=None)
def reference(name, members, hist, counts_key, with_fp):
    c = host_case(name)
    counts = None if counts_key is None else list(counts_key)
    fp = field_precision_of(name) if with_fp else None
    return restate_field_grad(c["w1"], c["w2"], c["b2"], c["groups"], c["z"], snapshot(name, hist), precision_map(name, hist), fp, counts, members)


def make_decoder(name):
    from sea_amd.models.encoder_decoder import Decode

    c = host_case(name)
    dec = Decode(c["groups"], c["n_inp"], c["hidden"], c["D"])
    with torch.no_grad():
        for g, m in enumerate(dec.decoders):
            m.layer1.weight.copy_(c["w1"][g])
            m.layer2.weight.copy_(c["w2"][g])
            m.layer2.bias.copy_(c["b2"][g])
    return dec


# ------------------------------------------------------------------------------------------------ the restatement
def _autograd_fp64(c, z, obs, precision, field_precision, counts, members, upstream=None):
    """The same score through differentiable torch ops in fp64; d (sum upstream * wsse) / dz by torch.autograd."""
    f64 = torch.float64
    Bm, P, G, D = z.shape
    n_f = [len(g) for g in c["groups"]]
    F, C_ = sum(n_f), c["n_inp"]
    w, ob = _weights_fp64(obs, precision, field_precision, counts, members, Bm, P, F, C_)
    zz = z.detach().to(f64).clone().requires_grad_(True)
    outs = []
    for g in range(G):
        pre = zz.reshape(Bm * P, G, D)[:, g] @ c["w1"][g].to(f64).t()
        outs.append((torch.nn.functional.gelu(pre) @ c["w2"][g].to(f64).t() + c["b2"][g].to(f64)).view(Bm * P, n_f[g], C_))
    y = torch.cat(outs, 1)
    d = torch.where(w > 0, y - ob, torch.zeros((), dtype=f64))
    wsse = (w * d * d).sum(-1).view(Bm, P, F).sum(1)
    (wsse if upstream is None else wsse * upstream).sum().backward()
    return wsse.detach(), zz.grad


@pytest.mark.parametrize("name,members,hist", [("a", 2, 1), ("a", 1, 2), ("b", 11, 3), ("c", 7, 5)])
def test_restatement_agrees_with_autograd(name, members, hist):
    c = host_case(name)
    for counts in counts_sets(name):
        for with_fp in (False, True):
            fp = field_precision_of(name) if with_fp else None
            wsse, dz = reference(name, members, hist, None if counts is None else tuple(counts), with_fp)
            a_wsse, a_dz = _autograd_fp64(c, c["z"], snapshot(name, hist), precision_map(name, hist), fp, counts, members)
            assert rel(wsse, a_wsse) <= 1e-12 and rel(dz, a_dz) <= 1e-10, (counts, with_fp)


@pytest.mark.parametrize("name", ["decode_mse_a", "decode_mse_b"])
@pytest.mark.parametrize("masked", [False, True])
def test_without_weights_it_is_the_decoded_field_loss_of_the_reference_fixtures(name, masked):
    """No map, no field precision, one member per snapshot: sum wsse = loss * n_valid and dz = n_valid * d loss / dz, with loss and dz those of
    tests/test_decode_loss_cpu.restate, which reproduces the reference's Decode + F.mse_loss on these fixtures."""
    fx = load_fixture(name)
    counts = fx["counts"] if masked else None
    loss, dz_mse, _ = restate(fx["w1"], fx["w2"], fx["b2"], fx["groups"], fx["z"], fx["target"], counts)
    B, P = fx["z"].shape[:2]
    F, C_ = sum(len(g) for g in fx["groups"]), fx["n_inp"]
    n_valid = B * F * (P * C_ if counts is None else int(torch.as_tensor(counts).clamp(0, C_).sum()))
    wsse, dz = restate_field_grad(fx["w1"], fx["w2"], fx["b2"], fx["groups"], fx["z"], fx["target"], None, None, None if counts is None else counts.tolist(), 1)
    assert wsse.shape == (B, F) and float(wsse.min()) > 0
    assert rel(wsse.sum(), loss * n_valid) <= 1e-12
    assert rel(dz, dz_mse * n_valid) <= 1e-12
    ref_loss, ref_dz = (fx["loss_masked"], fx["dz_masked"]) if masked else (fx["loss"], fx["dz"])    # ... and so the reference's own numbers
    assert rel(wsse.sum() / n_valid, ref_loss) <= 1e-9 and rel(dz / n_valid, ref_dz) <= 1e-9


def test_selects_make_weightless_cells_neutral_and_members_independent():
    c = host_case("a")
    args = (c["w1"], c["w2"], c["b2"], c["groups"])
    obs, pm, fp, counts = snapshot("a", 2), precision_map("a", 2), field_precision_of("a"), c["counts"]
    base = restate_field_grad(*args, c["z"], obs, pm, fp, counts, 1)
    w, _ = _weights_fp64(obs, pm, fp, counts, 1, 2, c["P"], 3, c["n_inp"])
    dead = (w == 0).view(2, c["P"], 3, c["n_inp"])
    obs2, pm2 = obs.clone(), pm.clone()
    obs2[dead] = float("nan")
    pm2[dead] = float("nan")
    got = restate_field_grad(*args, c["z"], obs2, pm2, fp, counts, 1)
    assert torch.equal(base[0], got[0]) and torch.equal(base[1], got[1]) and bool(torch.isfinite(got[1]).all())
    pm3 = pm.clone()
    pm3[pm == 0] = -1.0                                                   # negative acts as 0
    got = restate_field_grad(*args, c["z"], obs, pm3, fp, counts, 1)
    assert torch.equal(base[0], got[0]) and torch.equal(base[1], got[1])
    assert float(base[0][:, 1].abs().max()) == 0.0                        # the field that field_precision switches off
    assert float(base[1][0, 0].abs().max()) == 0.0 and float(base[1][0, 1].abs().max()) > 0   # (history 0, patch 0) has no live cell
    # members of one history share its snapshot: two members on history 0's snapshot are member 0 scored twice
    twice = restate_field_grad(*args, c["z"][:1].repeat(2, 1, 1, 1), obs[:1], pm[:1], fp, counts, 2)
    assert torch.equal(twice[0][0], base[0][0]) and torch.equal(twice[0][1], base[0][0]) and torch.equal(twice[1][1], base[1][0])


def test_every_relative_error_case_has_a_nonzero_reference():
    """The GPU tests divide by these norms; and every case must keep members with enough live cells for the per-member comparison."""
    for name, members, hist, counts, with_fp in all_cases():
        c = host_case(name)
        wsse, dz = reference(name, members, hist, None if counts is None else tuple(counts), with_fp)
        assert float(wsse.norm()) > 0 and float(dz.norm()) > 0, (name, members, hist, counts, with_fp)
        fp = field_precision_of(name) if with_fp else None
        per_field, _ = live_cells(snapshot(name, hist), precision_map(name, hist), fp, counts, members, c["B"], c["P"], c["groups"], c["n_inp"])
        enough = (per_field >= MIN_LIVE).any(1)
        assert int(enough.sum()) >= max(1, c["B"] // 2), (name, members, hist, counts, with_fp, int(enough.sum()))
        assert bool(torch.isfinite(dz).all())


def test_one_wrong_cell_weight_passes_a_whole_tensor_bound_and_fails_the_per_member_one():
    """Why the GPU test compares per member besides the whole tensor: shape b, one member per snapshot, ONE cell of ONE member weighted 1.8x too much.
    The whole [33, 3] score and the whole gradient stay inside TOL_BF16 — a whole-tensor bound alone would pass this kernel — the member's own rows do not."""
    c = host_case("b")
    args = (c["w1"], c["w2"], c["b2"], c["groups"], c["z"], snapshot("b", 33), precision_map("b", 33), None, None, 1)
    ref_wsse, ref_dz = restate_field_grad(*args)
    P, C_ = c["P"], c["n_inp"]
    w, ob = _weights_fp64(args[5], args[6], None, None, 1, 33, P, 3, C_)
    member = 17
    # the member's weighted cell with the largest residual in field 0 (patch 1: not the zeroed one)
    one = restate_field_grad(*args[:5], args[5], args[6], None, None, 1, cell_weights=w)     # identical weights: the restatement is reproduced
    assert torch.equal(one[0], ref_wsse)
    row = member * P + 1
    zz = c["z"].double().reshape(33 * P, 3, c["D"])
    pre = zz[row, 0] @ c["w1"][0].double().t()
    y = (0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0)))) @ c["w2"][0].double().t() + c["b2"][0].double()
    cell = int(torch.argmax(w[row, 0] * (y - ob[row, 0]) ** 2))
    assert float(w[row, 0, cell]) > 0
    wrong = w.clone()
    wrong[row, 0, cell] *= 1.8
    bad_wsse, bad_dz = restate_field_grad(*args, cell_weights=wrong)
    per_field, _ = live_cells(args[5], args[6], None, None, 1, 33, P, c["groups"], C_)
    enough = (per_field >= MIN_LIVE).any(1)
    assert bool(enough[member])
    whole_w, whole_g = rel(bad_wsse, ref_wsse), rel(bad_dz, ref_dz)
    mem_w, mem_g = per_member_rel(bad_wsse, ref_wsse, enough), per_member_rel(bad_dz, ref_dz, enough)
    print(f"one wrong cell weight: whole tensor e(wsse) {whole_w:.3e} e(dz) {whole_g:.3e}; per member e(wsse) {mem_w:.3e} e(dz) {mem_g:.3e}")
    assert 0 < whole_w <= TOL_BF16 and 0 < whole_g <= TOL_BF16
    assert mem_w > TOL_BF16 and mem_g > TOL_BF16


def test_an_upstream_gradient_per_member_and_group_scales_the_saved_gradient():
    """What Decode.field_loss's backward relies on: wsse[bm, f] depends on z[bm, :, g(f), :] alone, so d (sum c[bm, g(f)] wsse[bm, f]) / dz is the gradient
    of sum wsse scaled per member and group."""
    c = host_case("a")
    obs, pm, fp = snapshot("a", 1), precision_map("a", 1), field_precision_of("a")
    _, dz = restate_field_grad(c["w1"], c["w2"], c["b2"], c["groups"], c["z"], obs, pm, fp, c["counts"], 2)
    up_g = torch.tensor([[0.5, -2.0], [3.0, 0.25]], dtype=torch.float64)                     # [member, group]
    up = torch.stack([up_g[:, 0], up_g[:, 0], up_g[:, 1]], 1)                                # groups [[0, 1], [2]]
    _, a_dz = _autograd_fp64(c, c["z"], obs, pm, fp, c["counts"], 2, upstream=up)
    assert rel(dz * up_g.view(2, 1, 2, 1), a_dz) <= 1e-10


# ------------------------------------------------------------------------------------------------ the entry point, without a GPU
@pytest.fixture(scope="module")
def lib():
    from sea_amd import build, _native

    build.build(verbose=False)
    return _native.lib()


def _table(n_groups=2):
    """A well-formed sea_decode_field_grad table over made-up (aligned, never dereferenced) addresses: shape a with 2 members of one history.  Every test
    below breaks exactly one thing, so the checks refuse it before anything could be launched."""
    from sea_amd import _native as N

    g = (N.SeaDecodeMseGroup * N.DECODE_MSE_MAX_GROUPS)()
    for i in range(n_groups):
        base = 0x10000 * (i + 1)
        g[i].H, g[i].W2, g[i].bias, g[i].dH, g[i].Z = base, base + 0x1000, base + 0x2000, base + 0x3000, base + 0x4000
        g[i].ldh = g[i].ldw = g[i].lddh = g[i].ldz = 40
        g[i].n_fields, g[i].field0 = (2, 0) if i == 0 else (1, 2)
    p = N.SeaDecodeFieldGrad()
    p.obs, p.prec, p.field_prec, p.counts, p.wsse, p.work = 0x100000, 0x110000, 0x120004, 0x130004, 0x140004, 0x150004
    p.ld_row, p.ld_field, p.work_cap = 48, 16, 18 * 3
    p.M, p.S, p.C, p.Cp, p.P, p.members, p.n_fields_total = 18, 40, 12, 32, 9, 2, 3
    p.grad_scale = 1.0
    return g, p


def test_symbol_and_struct_layout(lib):
    from sea_amd import _native as N

    assert hasattr(lib, "sea_decode_field_grad") and "sea_decode_field_grad" in N.EXPORTED_SYMBOLS
    assert C.sizeof(N.SeaDecodeFieldGrad) == 104                        # include/sea_hip.h states it
    assert N.SeaDecodeFieldGrad.ld_row.offset == 48 and N.SeaDecodeFieldGrad.M.offset == 72 and N.SeaDecodeFieldGrad.grad_scale.offset == 100
    assert lib.sea_abi_version() == 8 and len(N.ABI_STRUCTS) == 33 and N.ABI_STRUCTS[-1] is N.SeaKvFork
    # the library reads the fields where the binding writes them: its messages quote the values back
    call = lambda g, p, n=2, dt=N.SEA_BF16: lib.sea_decode_field_grad(g, n, C.byref(p), dt, None)   # noqa: E731
    g, p = _table()
    p.members = 4
    assert call(g, p) == -1 and b"M=18 is not a multiple of P * members = 9 * 4" in lib.sea_last_error()
    g, p = _table()
    p.work_cap -= 1
    assert call(g, p) == -1 and b"sea_decode_field_grad: workspace of 53 floats is too small: 54 needed" in lib.sea_last_error()
    g, p = _table()
    p.ld_row, p.ld_field = 50, 16
    assert call(g, p) == -1 and b"ld_row=50, ld_field=16" in lib.sea_last_error()
    g, p = _table()
    g[1].lddh, g[1].ldz = 36, 56
    assert call(g, p) == -1 and b"group 1: row strides lddh=36 ldz=56" in lib.sea_last_error()
    g, p = _table()
    p.grad_scale = float("inf")
    assert call(g, p) == -1 and b"grad_scale must be finite" in lib.sea_last_error()


GROUP_BREAKS = {"null H": (0, "H", None), "null W2": (1, "W2", None), "null bias": (0, "bias", None), "misaligned W2": (1, "W2", 0x21008), "misaligned dH": (0, "dH", 0x13008),
                "misaligned Z": (1, "Z", 0x24004), "ldh % 8": (0, "ldh", 44), "short ldw": (1, "ldw", 32), "lddh < S": (1, "lddh", 32), "ldz < S": (0, "ldz", 32),
                "n_fields = 0": (1, "n_fields", 0), "field0 < 0": (0, "field0", -1),
                "dH NULL in group 1 only": (1, "dH", None), "dH NULL in group 0 only": (0, "dH", None),
                "field ranges overlap": (1, "field0", 1), "field range past the end": (1, "field0", 3)}
PARAM_BREAKS = {"null obs": ("obs", None), "null wsse": ("wsse", None), "null work": ("work", None), "misaligned obs": ("obs", 0x100004), "misaligned prec": ("prec", 0x110008),
                "misaligned field_prec": ("field_prec", 0x120002), "misaligned counts": ("counts", 0x130002), "M < 1": ("M", 0), "S % 8": ("S", 36), "Cp = 48": ("Cp", 48),
                "C > Cp": ("C", 33), "P < 1": ("P", 0), "members = 0": ("members", 0), "M % (P members)": ("members", 4), "M % P": ("P", 4), "short work_cap": ("work_cap", 53),
                "row stride": ("ld_row", 46), "field stride": ("ld_field", 14), "n_fields_total = 0": ("n_fields_total", 0),
                "grad_scale = inf": ("grad_scale", float("inf")), "grad_scale = nan": ("grad_scale", float("nan"))}


@pytest.mark.parametrize("what", sorted(GROUP_BREAKS) + sorted(PARAM_BREAKS) + ["field ranges leave a gap", "no groups", "too many groups"])
def test_bad_arguments_are_refused_without_a_device(lib, what):
    from sea_amd import _native as N

    g, p = _table()
    n = 2
    if what in GROUP_BREAKS:
        i, field, value = GROUP_BREAKS[what]
        setattr(g[i], field, value)
    elif what in PARAM_BREAKS:
        setattr(p, *PARAM_BREAKS[what])
    elif what == "field ranges leave a gap":
        p.n_fields_total, p.work_cap = 4, 18 * 4                         # groups cover fields 0, 1 and 3 of four
        g[1].field0 = 3
    else:
        n = 0 if what == "no groups" else 17
    assert lib.sea_decode_field_grad(g, n, C.byref(p), N.SEA_BF16, None) == -1, what
    msg = lib.sea_last_error()
    assert b"sea_decode_field_grad" in msg
    if what in GROUP_BREAKS:
        assert b"group %d" % GROUP_BREAKS[what][0] in msg, msg
    if what.startswith("dH NULL"):
        assert b"all groups, or none" in msg
    if what == "field ranges overlap":
        assert b"overlap" in msg
    if what == "field ranges leave a gap":
        assert b"cover 3 of the 4 fields" in msg
    if what.startswith("grad_scale"):
        assert b"grad_scale" in msg


def test_unsupported_forms_score_only_tables_and_null_tables(lib):
    from sea_amd import _native as N

    g, p = _table()
    assert lib.sea_decode_field_grad(g, 2, C.byref(p), N.SEA_F32, None) == -3   # fp32: unsupported, not an argument error
    assert b"sea_decode_field_grad" in lib.sea_last_error() and b"bf16 only" in lib.sea_last_error()
    g, p = _table()
    p.S = 648
    for i in range(2):
        g[i].ldh = g[i].ldw = g[i].lddh = g[i].ldz = 648
    assert lib.sea_decode_field_grad(g, 2, C.byref(p), N.SEA_BF16, None) == -3 and b"S=648" in lib.sea_last_error()
    assert lib.sea_decode_field_grad(None, 1, C.byref(p), N.SEA_BF16, None) == -1
    assert lib.sea_decode_field_grad(g, 1, None, N.SEA_BF16, None) == -1
    assert lib.sea_decode_field_grad(g, 2, C.byref(p), 7, None) == -1
    # score-only (dH NULL in every group): Z, lddh and ldz are not looked at; prec, field_prec and counts are nullable.  The table is well formed up
    # to the unsupported width, which is the last thing looked at: nothing else refuses it
    g, p = _table()
    p.S = 648
    p.prec = p.field_prec = p.counts = None
    for i in range(2):
        g[i].ldh = g[i].ldw = 648
        g[i].dH, g[i].Z, g[i].lddh, g[i].ldz = None, 0x24004, 0, 0
    assert lib.sea_decode_field_grad(g, 2, C.byref(p), N.SEA_BF16, None) == -3 and b"S=648" in lib.sea_last_error()


# ------------------------------------------------------------------------------------------------ refusals of the Python layers
def _ops_args(M=18, S=40, C_=12, Cp=32, n_f=(2, 1), P=9, members=2, grad=True):
    bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)   # noqa: E731
    groups = [dict(H=bf(M, S), W2=bf(n * Cp, S), bias=torch.zeros(n * Cp)) for n in n_f]
    if grad:
        for g in groups:
            g.update(dH=bf(M, S), Z=bf(M, S))
    F = sum(n_f)
    return dict(groups=groups, obs=torch.zeros(M // members, F, C_), C_=C_, Cp=Cp, n_patches=P, members=members, prec=torch.ones(M // members, F, C_),
                field_prec=torch.ones(F), counts=torch.zeros(P, dtype=torch.int32))


def test_ops_decode_field_grad_refuses_cpu_tensors_and_malformed_operands():
    from sea_amd import ops

    with pytest.raises(RuntimeError, match="MI355X"):
        ops.decode_field_grad(**_ops_args())
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.decode_field_grad(**_ops_args(grad=False))                    # score-only
    a = _ops_args()
    del a["groups"][0]["Z"]                                               # Z is optional per group
    a["prec"] = a["field_prec"] = a["counts"] = None
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.decode_field_grad(**a)

    def bad(match, **change):
        a = _ops_args()
        for k, v in change.items():
            if callable(v):
                v(a)
            else:
                a[k] = v
        with pytest.raises(ValueError, match=match):
            ops.decode_field_grad(**a)

    bad("bf16 only", dtype=torch.float32)
    bad("groups", groups=[])
    bad("groups", groups=_ops_args()["groups"] * 9)
    bad("Cp", Cp=48)
    bad("Cp", C_=33)
    bad("grad_scale", grad_scale=float("inf"))
    bad("grad_scale", grad_scale="1")
    bad("multiple of 8", f=lambda a: a["groups"][0].update(H=torch.zeros(18, 36, dtype=torch.bfloat16)))
    bad("multiple of 8", f=lambda a: [g.update({k: torch.zeros(g[k].shape[0], 648, dtype=torch.bfloat16) for k in ("H", "W2", "dH", "Z")}) for g in a["groups"]])
    bad("positive integers", members=0)
    bad("not a multiple of n_patches", members=4)
    bad("all of them, or none", f=lambda a: a["groups"][1].pop("dH"))
    bad("group 1: dH", f=lambda a: a["groups"][1].update(dH=torch.zeros(17, 40, dtype=torch.bfloat16)))
    bad("group 0: dH", f=lambda a: a["groups"][0].update(dH=torch.zeros(18, 40)))
    bad("group 0: Z", f=lambda a: a["groups"][0].update(Z=torch.zeros(18, 40)))
    bad("unit inner stride", f=lambda a: a["groups"][0].update(H=torch.zeros(40, 18, dtype=torch.bfloat16).t()))
    bad("row stride", f=lambda a: a["groups"][1].update(H=torch.zeros(18, 44, dtype=torch.bfloat16)[:, :40]))
    bad("16-byte", f=lambda a: a["groups"][1].update(H=torch.zeros(18 * 40 + 4, dtype=torch.bfloat16)[4:].view(18, 40)))
    bad("not a multiple of Cp", f=lambda a: a["groups"][0].update(W2=torch.zeros(40, 40, dtype=torch.bfloat16)))
    bad("bias", f=lambda a: a["groups"][0].update(bias=torch.zeros(64, dtype=torch.float64)))
    bad("obs must be float32", obs=torch.zeros(9, 3, 12, dtype=torch.float64))
    bad("obs must be float32", obs=torch.zeros(18, 3, 12))                # one row per (history, patch), not per member
    bad("obs must be float32", obs=torch.zeros(9, 3, 8))
    bad("multiples of 4", obs=torch.zeros(9, 3, 13)[..., :12], prec=None)
    bad("prec must be None or a float32 map", prec=torch.ones(9, 3, 12, dtype=torch.float64))
    bad("prec must be None or a float32 map", prec=torch.ones(9, 3, 16))
    bad("prec needs obs's strides", prec=torch.ones(9, 3, 16)[..., :12])
    bad("field_prec", field_prec=torch.ones(2))
    bad("field_prec", field_prec=torch.ones(3, dtype=torch.float64))
    bad("counts", counts=torch.zeros(9, dtype=torch.int64))
    bad("counts", counts=torch.zeros(8, dtype=torch.int32))
    bad("workspace", work=torch.zeros(18 * 3 - 1))
    bad("workspace", work=torch.zeros(18 * 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="a Z without a dH"):
        a = _ops_args(grad=False)
        a["groups"][0]["Z"] = torch.zeros(18, 40, dtype=torch.bfloat16)
        ops.decode_field_grad(**a)


def test_field_loss_and_field_likelihood_refuse_before_a_device_is_touched():
    from sea_amd.ensemble import FieldLikelihood

    c = host_case("a")
    dec = make_decoder("a").set_compute_dtype("bf16").requires_grad_(False)
    P, D, G, C_ = c["P"], c["D"], len(c["groups"]), c["n_inp"]
    z, obs = torch.zeros(4, P, G, D, requires_grad=True), torch.zeros(2, P, 3, C_)
    bad = [dict(z=torch.zeros(4, P, G)), dict(z=torch.zeros(4, P, G + 1, D)), dict(members=3), dict(members=True), dict(members=0),
           dict(obs=torch.zeros(2, P, 3, C_ - 1)), dict(obs=torch.zeros(4, P, 3, C_)), dict(obs=torch.zeros(2, P, 2, C_)), dict(obs=obs.double()),
           dict(obs=torch.zeros(2, P, 3, C_, requires_grad=True)), dict(obs=torch.zeros(2, P, 3, C_, device="meta")),
           dict(precision=torch.ones(2, P, 3, C_ + 4)), dict(precision=torch.ones(2, P, 3, C_).double()), dict(precision=torch.ones(2, P, 3, C_, requires_grad=True)),
           dict(field_precision=torch.ones(2)), dict(field_precision=torch.ones(3).double()), dict(field_precision=[1.0, 1.0, 1.0]),
           dict(field_precision=torch.ones(3, requires_grad=True)), dict(counts=[1, 2, 3]), dict(counts=[0] * 8 + [C_ + 1])]
    for kw in bad:
        args = dict(z=z, obs=obs, members=2)
        args.update(kw)
        zz = args.pop("z")
        with pytest.raises(ValueError):
            dec.field_loss(zz, **args)
    trainable = make_decoder("a").set_compute_dtype("bf16")               # its parameters require grad
    with pytest.raises(ValueError, match="frozen observation operator"):
        trainable.field_loss(z, obs, members=2)
    with pytest.raises(ValueError, match="bf16 only"):
        make_decoder("a").requires_grad_(False).field_loss(z, obs, members=2, fused=True)     # fp32: no fused launch
    for fused in (None, True, False):                                     # well-formed, but on the host
        with pytest.raises(RuntimeError, match="MI355X"):
            dec.field_loss(z, obs, members=2, precision=torch.ones_like(obs), field_precision=torch.ones(3), counts=[0] * P, fused=fused)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="MI355X"):
            trainable.field_loss(z, obs, members=1 * 2)                    # nothing to drop without grad mode: the call proceeds to the device check

    y = torch.zeros(4, G, P * D)
    like = FieldLikelihood(dec, P, 2, sigma=[0.5, 1.0, 2.0])
    assert torch.equal(like._field_prec(torch.device("cpu")), torch.tensor([4.0, 1.0, 0.25]))
    pm = torch.ones_like(obs)
    for yy, oo, pp in ((torch.zeros(4, G, P * D + 1), obs, pm), (torch.zeros(3, G, P * D), obs, pm), (y, torch.zeros(1, P, 3, C_), None), (y, obs, torch.ones(2, P, 3, C_ + 1)),
                       (y, obs, pm.double()), (y, obs, -pm), (y, obs.double(), pm)):
        for fn in (like, like.score_and_grad, like.nudge):
            with pytest.raises(ValueError):
                fn(yy, oo, pp)
    with pytest.raises(ValueError, match="layout"):
        like(y, obs, pm, layout="PBFC")
    with pytest.raises(ValueError, match="bf16 only"):
        FieldLikelihood(make_decoder("a").requires_grad_(False), P, 2, fused=True).score_and_grad(y, obs, pm)
    for rate in (torch.ones(3), torch.ones(4, 1), torch.ones(4, dtype=torch.float64), torch.ones(4, device="meta"), float("nan"), float("inf"), "1", True, None):
        with pytest.raises(ValueError, match="rate"):
            like.nudge(y, obs, pm, rate=rate)
    for fn, kw in ((like, {}), (like.score_and_grad, {}), (like.nudge, dict(rate=torch.ones(4)))):
        with pytest.raises(RuntimeError, match="MI355X"):
            fn(y, obs, pm, **kw)
        with pytest.raises(RuntimeError, match="MI355X"):
            fn(y, obs.permute(0, 1, 3, 2).contiguous(), pm.permute(0, 1, 3, 2).contiguous(), layout="BPCF", **kw)
    with pytest.raises(RuntimeError, match="MI355X"):
        like(y, obs, "BPFC")                                              # the layout as third positional argument, as before the precision map
    with pytest.raises(RuntimeError, match="MI355X"):
        like.score_and_grad(y, obs)                                       # no map: every valid cell with weight 1


def test_the_default_path_follows_the_measured_rows():
    """Decode.field_loss(fused=None), profiles/field_grad_bench.txt: fused from 4096 rows on in bf16 — with the gradient above hidden width 512 only from
    16384 rows on — and the composed path wherever nothing was measured (below 4096 rows) and in fp32."""
    bf, f32 = torch.bfloat16, torch.float32
    narrow, wide = make_decoder("a"), make_decoder("c")                  # hidden 40 and 624
    for dec in (narrow, wide):
        for grad in (False, True):
            assert not dec._field_loss_default(bf, 4095, grad) and not dec._field_loss_default(f32, 1 << 20, grad)
            assert dec._field_loss_default(bf, 16384, grad)
        assert dec._field_loss_default(bf, 4096, False)
    assert narrow._field_loss_default(bf, 4096, True) and not wide._field_loss_default(bf, 4096, True) and not wide._field_loss_default(bf, 16383, True)
