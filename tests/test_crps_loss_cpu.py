"""The CRPS of the decoded fields as a loss, on the host: the fp64 restatement of a cell's CRPS and of its derivative with respect to the members'
values (`restate_crps_grad`, on `restate_field_verify`'s conventions) against torch.autograd of the pairwise formula; the tie order; the exactness
premise the GPU test relies on; the composed path (sea_amd.ensemble._composed_crps) against the restatement; the struct layout and the argument checks
of sea_decode_member_crps_grad without a device; the refusals of Decode.member_crps_loss and EnsembleCRPSLoss."""
import ctypes as C

import pytest
import torch

from tests.test_field_verify_cpu import field_logw, restate_field_verify
from tests.test_sensor_cpu import host_case, make_decoder

F64 = torch.float64


# ------------------------------------------------------------------------------------------------ the contract, in fp64
def restate_crps_grad(Y, obs, w, logw, n, unbiased, field_weight=None):
    """include/sea_hip.h, sea_decode_member_crps_grad, from the decoded members, history by history, in fp64.  Y [B * n, P, F, C], obs [B, P, F, >= C],
    w [B, P, F, C] (0: dead), logw None / [B * n], field_weight None / [F].  below_m is the weight of the members j with (x_j, j) < (x_m, m), from the
    definition (an n x n comparison), not from a sort.  Returns dict(crps [B, P, F, C] (0 where not live and good), G [B * n, P, F, C] =
    fw w_m (sign(x_m - y) - (2 below_m + w_m - 1) / c), loss [B, F] = fw sum crps, count [B, F])."""
    Bm, P, F, C_ = Y.shape
    B = Bm // n
    crps, G = torch.zeros(B, P, F, C_, dtype=F64), torch.zeros(B, n, P, F, C_, dtype=F64)
    count = torch.zeros(B, F, dtype=F64)
    fw = torch.ones(F, dtype=F64) if field_weight is None else field_weight.to(F64)
    idx = torch.arange(n)
    for b in range(B):
        lw = torch.zeros(n, dtype=F64) if logw is None else logw[b * n:(b + 1) * n].to(F64)
        if bool(torch.isnan(lw).any()) or bool((lw == float("inf")).any()) or not bool(torch.isfinite(lw).any()):
            continue
        alive = lw != float("-inf")
        e = torch.where(alive, (lw - lw[alive].max()).exp(), torch.zeros((), dtype=F64))
        wm = e / e.sum()                                                        # [n]: 0 for a dead member
        c = 1.0 - float((wm * wm).sum()) if unbiased else 1.0
        x = Y[b * n:(b + 1) * n].to(F64)                                        # [n, P, F, C]
        y, p = obs[b, ..., :C_].to(F64), w[b].to(F64)
        al = alive.view(n, 1, 1, 1)
        good = (p > 0) & torch.isfinite(y) & torch.isfinite(p) & (torch.isfinite(x) | ~al).all(0)
        use = good.unsqueeze(0) & al
        xa = torch.where(use, x, torch.zeros((), dtype=F64))
        ya = torch.where(good, y, torch.zeros((), dtype=F64))
        wv = torch.where(use, wm.view(n, 1, 1, 1), torch.zeros((), dtype=F64))
        lower = (xa.unsqueeze(0) < xa.unsqueeze(1)) | ((xa.unsqueeze(0) == xa.unsqueeze(1)) & (idx.view(1, n) < idx.view(n, 1)).view(n, n, 1, 1, 1))   # [m, j]
        below = (lower.to(F64) * wv.unsqueeze(0)).sum(1)
        d = xa - ya
        t = 2.0 * below + wv - 1.0
        crps[b] = (wv * d.abs()).sum(0) - ((wv * d * t).sum(0) / c if c > 0 else 0.0)
        G[b] = torch.where(use, wv * (torch.sign(d) - (t / c if c > 0 else torch.zeros_like(t))), torch.zeros((), dtype=F64))
        count[b] = good.to(F64).sum((0, 2))
    G = G * fw.view(1, 1, 1, F, 1)
    return dict(crps=crps, G=G.view(Bm, P, F, C_), loss=fw.view(1, F) * crps.sum((1, 3)), count=count)


def pairwise_crps(x, y, wm, c):
    """sum_m w_m |x_m - y| - 1 / (2 c) sum_ij w_i w_j |x_i - x_j| for x [n, K], y [K]: what torch.autograd differentiates."""
    pair = (wm.view(-1, 1, 1) * wm.view(1, -1, 1) * (x.unsqueeze(0) - x.unsqueeze(1)).abs()).sum((0, 1))
    return (wm.view(-1, 1) * (x - y).abs()).sum(0) - pair / (2.0 * c)


@pytest.mark.parametrize("n", [2, 5, 17, 64])
@pytest.mark.parametrize("unbiased", [True, False])
def test_restatement_is_the_derivative_of_the_pairwise_formula(n, unbiased):
    """Tie-free random values, softmax weights with one dead member: crps and G against torch.autograd in fp64, to 1e-12."""
    g = torch.Generator().manual_seed(7000 + n + unbiased)
    K = 48
    x = torch.randn(n, K, generator=g, dtype=F64)
    y = torch.randn(K, generator=g, dtype=F64)
    logw = torch.randn(n, generator=g)
    if n > 2:
        logw[1] = float("-inf")
    alive = logw != float("-inf")
    wm = torch.where(alive, (logw.double() - logw[alive].double().max()).exp(), torch.zeros((), dtype=F64))
    wm = wm / wm.sum()
    c = 1.0 - float((wm * wm).sum()) if unbiased else 1.0
    xv = x.clone().requires_grad_(True)
    val = pairwise_crps(xv, y, wm, c)
    (grad,) = torch.autograd.grad(val.sum(), xv)
    r = restate_crps_grad(x.view(n, 1, 1, K), y.view(1, 1, 1, K), torch.ones(1, 1, 1, K, dtype=F64), logw, n, unbiased)
    assert float((r["crps"].view(K) - val.detach()).abs().max()) <= 1e-12
    assert float((r["G"].view(n, K) - grad).abs().max()) <= 1e-12
    if n > 2:
        assert float(r["G"].view(n, K)[1].abs().max()) == 0.0                                   # the dead member
    # ... and the sums are restate_field_verify's (the pairwise double sum written independently)
    ref = restate_field_verify(x.view(n, 1, 1, K), y.view(1, 1, 1, K), torch.ones(1, 1, 1, K, dtype=F64), logw, n, unbiased)
    assert abs(float(r["loss"][0, 0]) - float(ref["sums"][0, 0, 1])) <= 1e-12 * max(1.0, abs(float(ref["sums"][0, 0, 1])))
    assert float(r["count"][0, 0]) == float(ref["sums"][0, 0, 0])


@pytest.mark.parametrize("n", [2, 5, 17])
def test_ties_take_the_value_index_order(n):
    """Quarter-integer values tie.  With equal weights the derivative is a function of the POSITION in the order (value, index): exchanging two
    members that tie at a cell leaves that cell's G where it was — the two members swap their G — and the lower index holds the smaller `below`,
    2 w^2 / c apart when adjacent.  With any weights sum_m G[m] = sum_m w_m sign(x_m - y): the pair term has no net pull."""
    g = torch.Generator().manual_seed(7100 + n)
    K = 64
    x = torch.randint(-3, 4, (n, K), generator=g).double() / 4
    y = torch.randint(-3, 4, (K,), generator=g).double() / 4
    one = torch.ones(1, 1, 1, K, dtype=F64)
    for unbiased in (True, False):
        r = restate_crps_grad(x.view(n, 1, 1, K), y.view(1, 1, 1, K), one, None, n, unbiased)["G"].view(n, K)
        i, j = 0, n - 1
        xs = x.clone()
        xs[[i, j]] = x[[j, i]]
        s = restate_crps_grad(xs.view(n, 1, 1, K), y.view(1, 1, 1, K), one, None, n, unbiased)["G"].view(n, K)
        tied = x[i] == x[j]
        assert int(tied.sum()) >= 3
        assert torch.equal(s[:, tied], r[:, tied])                                              # positions keep their G: the two members swapped theirs
        c = 1.0 - 1.0 / n if unbiased else 1.0
        if n == 2:
            assert float(((r[i] - r[j])[tied] - 2.0 / (n * n * c)).abs().max()) <= 1e-15
        else:
            assert bool(((r[i] - r[j])[tied] >= 2.0 / (n * n * c) - 1e-15).all())
        logw = torch.randn(n, generator=g)
        wm = torch.softmax(logw.double(), 0)
        rw = restate_crps_grad(x.view(n, 1, 1, K), y.view(1, 1, 1, K), one, logw, n, unbiased)["G"].view(n, K)
        assert float((rw.sum(0) - (wm.view(n, 1) * torch.sign(x - y)).sum(0)).abs().max()) <= 1e-14


@pytest.mark.parametrize("n", [2, 4, 8, 16, 32, 64, 128])
def test_equal_weight_gradients_on_quarter_integers_are_exact_in_bf16(n):
    """The exactness premise of the GPU test: equal weights, N a power of two up to 128, unbiased=False: G = (N sign + N - 2 k - 1) / N^2 with k the
    members below — an integer of at most 8 bits over a power of two — is representable in bf16, so the kernel's one rounding changes nothing."""
    g = torch.Generator().manual_seed(7200 + n)
    K = 96
    x = torch.randint(-12, 13, (n, K), generator=g).double() / 4
    y = torch.randint(-12, 13, (K,), generator=g).double() / 4
    G = restate_crps_grad(x.view(n, 1, 1, K), y.view(1, 1, 1, K), torch.ones(1, 1, 1, K, dtype=F64), None, n, False)["G"]
    assert torch.equal(G.to(torch.float32).to(torch.bfloat16).to(F64), G)
    assert float(G.abs().max()) > 0.0


@pytest.mark.parametrize("n,unbiased", [(1, True), (2, True), (5, False), (17, True)])
def test_composed_path_against_the_restatement(n, unbiased):
    """_composed_crps (a stable sort) against the restatement (the n x n comparison) on values with ties, a precision map with dead cells (obs NaN
    there), counts, log-weights with a dead member, a field weight; and through _CrpsComposedFn's backward with a per-(history, field) upstream."""
    from sea_amd.ensemble import _CrpsComposedFn, _composed_crps, _field_cell_weights

    g = torch.Generator().manual_seed(7300 + n)
    B, P, F, C_ = 3, 2, 3, 11
    Y = torch.randint(-6, 7, (B * n, P, F, C_), generator=g).float() / 4
    obs = torch.randint(-6, 7, (B, P, F, C_ + 2), generator=g).float() / 4
    prec = 0.25 + torch.rand(B, P, F, C_ + 2, generator=g)
    miss = torch.rand(B, P, F, C_ + 2, generator=g) < 0.15
    prec[miss] = 0.0
    obs[miss] = float("nan")
    Y[n - 1, 0, 1, 3] = float("inf")                                                            # a bad cell of history 0
    counts = torch.tensor([C_, 7], dtype=torch.int32)
    logw = field_logw(n, B, 11 + n)
    fw = torch.tensor([1.0, 0.5, 0.0])
    w = _field_cell_weights((B, P, F, C_), None, prec, counts, torch.device("cpu"))
    ref = restate_crps_grad(Y.double(), obs, w.double(), logw, n, unbiased, fw)
    loss, count, G = _composed_crps(Y, obs, w, logw, n, unbiased, fw)
    assert loss.dtype == torch.float32 and loss.shape == (B, F) and torch.equal(count, ref["count"])
    assert float((loss.double() - ref["loss"]).abs().max()) <= 1e-6 * max(1.0, float(ref["loss"].abs().max()))
    assert float((G - ref["G"]).abs().max()) <= 1e-13
    assert float(G[..., 2, :].abs().max()) == 0.0 and bool(torch.isfinite(G).all())
    Yv = Y.clone().requires_grad_(True)
    lv, cv = _CrpsComposedFn.apply(Yv, obs, w, logw, n, unbiased, fw)
    assert not cv.requires_grad and torch.equal(lv, loss)
    up = torch.rand(B, F, generator=g) + 0.5
    (lv * up).sum().backward()
    want = ref["G"].view(B, n, P, F, C_) * up.double().view(B, 1, 1, F, 1)
    assert float((Yv.grad.double().view(B, n, P, F, C_) - want).abs().max()) <= 1e-6


# ------------------------------------------------------------------------------------------------ the entry points without a device
@pytest.fixture(scope="module")
def lib():
    from sea_amd import build, _native

    build.build(verbose=False)
    return _native.lib()


def _tables(n_groups=2):
    """A well-formed sea_decode_member_crps_grad table over made-up (aligned, never dereferenced) addresses: 4 members of 2 histories, 9 patches, 3 fields."""
    from sea_amd import _native as N

    arr, p = (N.SeaDecodeMseGroup * n_groups)(), N.SeaDecodeMemberCrpsGrad()
    for g in range(n_groups):
        arr[g].H, arr[g].W2, arr[g].bias, arr[g].dH, arr[g].Z = 0x100000 + 0x10000 * g, 0x200000 + 0x10000 * g, 0x300000 + 0x10000 * g, 0x800000 + 0x10000 * g, 0x900000 + 0x10000 * g
        arr[g].ldh, arr[g].ldw, arr[g].lddh, arr[g].ldz, arr[g].n_fields, arr[g].field0 = 40, 40, 40, 40, 2 if g == 0 else 1, 0 if g == 0 else 2
    p.obs, p.prec_field, p.prec, p.field_weight, p.counts, p.logw = 0x400000, 0x410000, 0x420000, 0x450000, 0x430000, 0x440000
    p.loss, p.sums, p.status, p.work = 0x500000, 0x600000, 0x620000, 0x700000
    p.ld_row, p.ld_field, p.ld_prow, p.ld_pfield = 3 * 24, 24, 3 * 24, 24
    p.M, p.S, p.C, p.Cp, p.P, p.members, p.n_fields_total, p.unbiased = 2 * 4 * 9, 40, 21, 32, 9, 4, 3, 1
    p.work_bytes = 2 * 9 * 3 * (64 + 4 * 4 * 40)
    return arr, p


def test_symbols_and_struct_layout(lib):
    from sea_amd import _native as N

    for name in ("sea_decode_member_crps_grad", "sea_decode_member_crps_grad_ws_bytes"):
        assert hasattr(lib, name) and name in N.EXPORTED_SYMBOLS
    T = N.SeaDecodeMemberCrpsGrad
    assert C.sizeof(T) == 152                                                               # include/sea_hip.h states it
    assert T.field_weight.offset == 24 and T.loss.offset == 48 and T.work.offset == 72 and T.ld_row.offset == 80 and T.work_bytes.offset == 112
    assert T.M.offset == 120 and T.members.offset == 140 and T.unbiased.offset == 148
    assert lib.sea_abi_version() == 8 and len(N.ABI_STRUCTS) == 33 and N.ABI_STRUCTS[-1] is N.SeaKvFork and T not in N.ABI_STRUCTS
    # per (history, patch, field, chunk of 512 columns): 8 fp64 sums and an fp32 [members, S] partial of dH
    ws = lib.sea_decode_member_crps_grad_ws_bytes
    assert ws(2, 9, 3, 4, 32, 40) == 2 * 9 * 3 * (64 + 4 * 4 * 40) and ws(1, 1, 1, 128, 512, 384) == 64 + 4 * 128 * 384 and ws(1, 1, 1, 64, 544, 640) == 2 * (64 + 4 * 64 * 640)
    for bad in ((0, 9, 3, 4, 32, 40), (65536, 9, 3, 4, 32, 40), (2, 0, 3, 4, 32, 40), (2, 9, 0, 4, 32, 40), (2, 9, 3, 0, 32, 40), (2, 9, 3, 129, 32, 40), (2, 9, 3, 4, 40, 40),
                (2, 9, 3, 4, 32, 36), (2, 9, 3, 4, 32, 648), (2, 9, 3, 65, 32, 392)):
        assert ws(*bad) == -1, bad
    for field, value, msg in (("members", 0, b"members=0"), ("ld_pfield", 20, b"ld_pfield=20 must cover C=21"), ("M", 71, b"M=71 is not a multiple of P * members = 9 * 4"),
                              ("unbiased", 2, b"unbiased=2"), ("work_bytes", 38015, b"work_bytes=38015 below the 38016")):
        arr, p = _tables()
        setattr(p, field, value)
        assert lib.sea_decode_member_crps_grad(arr, 2, C.byref(p), N.SEA_BF16, None) == -1 and msg in lib.sea_last_error(), (field, lib.sea_last_error())


BREAKS = {"null obs": ("obs", None), "null loss": ("loss", None), "null sums": ("sums", None), "null status": ("status", None), "null work": ("work", None),
          "misaligned obs": ("obs", 0x400002), "misaligned prec": ("prec", 0x420001), "misaligned prec_field": ("prec_field", 0x410003),
          "misaligned field_weight": ("field_weight", 0x450002), "misaligned counts": ("counts", 0x430002), "misaligned logw": ("logw", 0x440001),
          "misaligned loss": ("loss", 0x500002), "misaligned sums": ("sums", 0x600004), "misaligned status": ("status", 0x620002), "misaligned work": ("work", 0x700004),
          "members = 0": ("members", 0), "M = 0": ("M", 0), "M not a multiple": ("M", 70), "S odd": ("S", 36), "Cp = 40": ("Cp", 40), "C above Cp": ("C", 33), "C = 0": ("C", 0),
          "P = 0": ("P", 0), "ld_field short": ("ld_field", 20), "ld_row negative": ("ld_row", -1), "ld_pfield short": ("ld_pfield", 20), "fields": ("n_fields_total", 4),
          "unbiased = 2": ("unbiased", 2), "workspace one byte short": ("work_bytes", 38015)}


@pytest.mark.parametrize("what", sorted(BREAKS) + ["bad dtype", "no groups", "too many groups", "group null", "group null dH", "group misaligned", "group misaligned Z",
                                                   "group overlap", "group missing", "ldh short", "lddh short", "ldz short"])
def test_crps_grad_refuses_bad_arguments_without_a_device(lib, what):
    from sea_amd import _native as N

    arr, p = _tables()
    dt, ng = N.SEA_BF16, 2
    if what in BREAKS:
        setattr(p, *BREAKS[what])
    elif what == "bad dtype":
        dt = 5
    elif what == "no groups":
        ng = 0
    elif what == "too many groups":
        ng = N.DECODE_MSE_MAX_GROUPS + 1
    elif what == "group null":
        arr[1].W2 = None
    elif what == "group null dH":
        arr[0].dH = None
    elif what == "group misaligned":
        arr[0].bias = 0x300008
    elif what == "group misaligned Z":
        arr[1].Z = 0x900008
    elif what == "group overlap":
        arr[1].field0 = 1
    elif what == "group missing":
        ng = 1
    elif what == "ldh short":
        arr[0].ldh = 32
    elif what == "lddh short":
        arr[1].lddh = 32
    else:
        arr[0].ldz = 8
    assert lib.sea_decode_member_crps_grad(arr, ng, C.byref(p), dt, None) == -1, what
    assert b"sea_decode_member_crps_grad" in lib.sea_last_error()


def test_unsupported_forms_and_null_tables(lib):
    from sea_amd import _native as N, ops

    arr, p = _tables()
    assert lib.sea_decode_member_crps_grad(arr, 2, C.byref(p), N.SEA_F32, None) == -3 and b"sea_decode_member_crps_grad" in lib.sea_last_error()

    def widened(S, members):
        arr, p = _tables()
        p.S, p.members, p.M = S, members, 2 * members * 9
        for g in range(2):
            arr[g].ldh = arr[g].ldw = arr[g].lddh = arr[g].ldz = S
        return arr, p

    arr, p = widened(648, 4)
    assert lib.sea_decode_member_crps_grad(arr, 2, C.byref(p), N.SEA_BF16, None) == -3 and b"S=648" in lib.sea_last_error()
    arr, p = widened(40, 129)
    assert lib.sea_decode_member_crps_grad(arr, 2, C.byref(p), N.SEA_BF16, None) == -3 and b"members=129" in lib.sea_last_error()
    arr, p = widened(392, 65)                                                                    # the form the register file does not hold
    assert lib.sea_decode_member_crps_grad(arr, 2, C.byref(p), N.SEA_BF16, None) == -3 and b"members=65 above 64 at hidden width S=392" in lib.sea_last_error()
    assert not ops.decode_member_crps_grad_supported(392, 65) and ops.decode_member_crps_grad_supported(384, 128) and ops.decode_member_crps_grad_supported(640, 64)
    assert lib.sea_decode_member_crps_grad(None, 2, C.byref(p), N.SEA_BF16, None) == -1 and lib.sea_decode_member_crps_grad(arr, 2, None, N.SEA_BF16, None) == -1
    # prec_field, prec, field_weight, counts, logw and Z may be NULL: such a table passes the pointer checks and fails only at the check this test breaks
    arr, p = _tables()
    p.prec_field = p.prec = p.field_weight = p.counts = p.logw = None
    arr[0].Z = arr[1].Z = None
    arr[0].ldz = arr[1].ldz = 0
    p.ld_pfield, p.work_bytes = 0, 7
    assert lib.sea_decode_member_crps_grad(arr, 2, C.byref(p), N.SEA_BF16, None) == -1 and b"work_bytes=7" in lib.sea_last_error()
    assert ops.last_form() == ("", 0, 0) or not ops.last_form()[0].startswith("decode.member_crps_grad")   # a refused call notes nothing


# ------------------------------------------------------------------------------------------------ the Python layers refuse before any device work
def _loss_args(members=2, B=2):
    c = host_case("a")
    dec = make_decoder("a").requires_grad_(False)
    P, F, C_ = c["P"], sum(len(g) for g in c["groups"]), c["n_inp"]
    z = torch.zeros(B * members, P, len(c["groups"]), c["D"])
    obs = torch.zeros(B, P, F, C_)
    return dec, z, obs, P, F, C_


def test_member_crps_loss_refuses_malformed_arguments():
    dec, z, obs, P, F, C_ = _loss_args()
    ok = dict(members=2)
    for kw, exc in ((dict(members=3), "members"), (dict(members=0), "members"), (dict(members=True), "members"), (dict(members=2.0), "members"),
                    (dict(obs=obs[:1]), "obs must be"), (dict(obs=obs.double()), "float32"), (dict(obs=obs[..., :C_ - 1]), "obs must be"),
                    (dict(obs=obs.clone().requires_grad_(True)), "must not require grad"),
                    (dict(precision=torch.ones(2, P, F, C_ + 1)), "precision must have"), (dict(precision=torch.ones(2, P, F, C_).double()), "float32"),
                    (dict(field_precision=torch.ones(F + 1)), "field_precision"), (dict(field_precision=torch.ones(F).double()), "field_precision"),
                    (dict(field_weight=torch.ones(F + 1)), "field_weight"), (dict(field_weight=torch.ones(F).double()), "field_weight"),
                    (dict(field_weight=torch.tensor([1.0, -0.5, 1.0][:F] + [1.0] * max(0, F - 3))), "finite and >= 0"),
                    (dict(field_weight=torch.tensor([float("nan")] + [1.0] * (F - 1))), "finite and >= 0"),
                    (dict(field_weight=[1.0] * F), "field_weight"),
                    (dict(logw=torch.zeros(3)), "logw"), (dict(logw=torch.zeros(4).double()), "logw"),
                    (dict(counts=[1] * (P + 1)), "counts"), (dict(counts=[C_ + 1] + [0] * (P - 1)), "counts"),
                    (dict(fused=True), "bf16 only")):
        args = dict(ok, obs=obs)
        args.update(kw)
        o = args.pop("obs")
        with pytest.raises(ValueError, match=exc):
            dec.member_crps_loss(z, o, **args)
    with pytest.raises(ValueError, match="z must be"):
        dec.member_crps_loss(z[..., :-1], obs, 2)
    with pytest.raises(ValueError, match="z must be"):
        dec.member_crps_loss(z[0], obs, 2)
    live = make_decoder("a")                                                                     # a decoder parameter that requires grad
    with pytest.raises(ValueError, match="requires grad"):
        live.member_crps_loss(z.clone().requires_grad_(True), obs, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                                   # well-formed arguments reach the device check, and only then
        dec.member_crps_loss(z, obs, 2)
    dec.set_compute_dtype("bf16")
    big = torch.zeros(2 * 129, P, z.shape[2], z.shape[3])
    with pytest.raises(ValueError, match="carry up to 64 members"):
        dec.member_crps_loss(big, obs, 129, fused=True)


def test_ensemble_crps_loss_refuses_malformed_arguments():
    from sea_amd.utils.train_utils import EnsembleCRPSLoss

    dec, z, obs, P, F, C_ = _loss_args()
    G, D = z.shape[2], z.shape[3]
    for kw in (dict(n_patches=0), dict(n_patches=2.0), dict(members=0), dict(members=True), dict(layout="PBFC"), dict(field_weight=[1.0] * (F + 1)),
               dict(field_weight=[-1.0] + [1.0] * (F - 1)), dict(field_weight=[float("inf")] + [1.0] * (F - 1))):
        args = dict(n_patches=P, members=2)
        args.update(kw)
        with pytest.raises(ValueError, match="EnsembleCRPSLoss"):
            EnsembleCRPSLoss(dec, **args)
    loss_fn = EnsembleCRPSLoss(dec, P, 2, field_weight=[1.0] * F)
    assert list(loss_fn.parameters()) == []
    B, T = 2, 3
    out = torch.zeros(B * 2, T, G, P * D)
    fields = torch.zeros(B, T, P, F, C_)
    for o, f, kw in ((out[:3], fields, {}), (out[..., :-1], fields, {}), (out[0], fields, {}), (out, fields[:1], {}), (out, fields[:, :2], {}), (out, fields[:, :, :1], {}),
                     (out, fields[0], {}), (out, fields, dict(precision=torch.ones(B, T, P, F, C_ + 1))), (out, fields, dict(logw=torch.zeros(B))),
                     (out, fields, dict(logw=torch.zeros(B * 2).double())), (out, fields, dict(layout="BFPC"))):
        with pytest.raises(ValueError, match="EnsembleCRPSLoss"):
            loss_fn(o, f, **kw)
    with pytest.raises(ValueError, match="obs must be"):                                         # the decoder's own check, behind the re-layout
        EnsembleCRPSLoss(dec, P, 3)(torch.zeros(3, T, G, P * D), torch.zeros(1, T, P, F, C_ - 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss_fn(out, fields)


# ------------------------------------------------------------------------------------------------ EnsembleCRPSLoss's re-layout, against an explicit loop
class _LinearDecoder:
    """Stands in for Decode on the host: two field groups ([[0, 1], [2]]), a fixed linear map per group from D latent values to the group's fields x C
    cells, and member_crps_loss as the composed path computes it (sea_amd.ensemble._CrpsComposedFn).  It records what EnsembleCRPSLoss hands it."""
    field_groups = [[0, 1], [2]]

    def __init__(self, D, C_, seed):
        g = torch.Generator().manual_seed(seed)
        self.C = C_
        self.W = [torch.randn(2 * C_, D, generator=g, dtype=F64), torch.randn(C_, D, generator=g, dtype=F64)]
        self.seen = {}

    def decode(self, z):   # z [rows, P, G, D] -> [rows, P, 3, C]
        rows, P = z.shape[0], z.shape[1]
        return torch.cat([(z[:, :, g].to(F64) @ self.W[g].t()).view(rows, P, -1, self.C) for g in range(2)], dim=2)

    def member_crps_loss(self, z, obs, members, counts=None, precision=None, field_precision=None, field_weight=None, logw=None, unbiased=True, fused=None):
        from sea_amd.ensemble import _CrpsComposedFn, _field_cell_weights

        self.seen = dict(z=tuple(z.shape), obs=tuple(obs.shape), members=members, logw=None if logw is None else logw.clone(), fused=fused)
        B, P, F, C_ = obs.shape[0], obs.shape[1], obs.shape[2], self.C
        cnt = None if counts is None else torch.tensor(counts, dtype=torch.int32)
        w = _field_cell_weights((B, P, F, C_), field_precision, precision, cnt, torch.device("cpu"))
        return _CrpsComposedFn.apply(self.decode(z), obs, w, logw, members, unbiased, field_weight)


@pytest.mark.parametrize("layout", ["BPFC", "BPCF"])
def test_ensemble_crps_loss_relayout_against_an_explicit_loop(layout):
    """B = 2 histories, T = 2 steps, 3 members, P = 2 patches: EnsembleCRPSLoss's views and permutes (fork order: row b * members + j is member j of
    history b; (b, t) is the history of the score; logw [B * members] repeated over t; the precision map; the reference's BPCF layout) against a loop
    that takes every (b, t) apart by hand and scores it with the fp64 restatement — value and the gradient with respect to the model output."""
    from sea_amd.utils.train_utils import EnsembleCRPSLoss

    B, T, n, P, G, D, C_, F = 2, 2, 3, 2, 2, 4, 5, 3
    g = torch.Generator().manual_seed(7400)
    dec = _LinearDecoder(D, C_, 7401)
    out = torch.randn(B * n, T, G, P * D, generator=g, dtype=F64).requires_grad_(True)
    fields = torch.randn(B, T, P, F, C_, generator=g)
    prec = 0.25 + torch.rand(B, T, P, F, C_, generator=g)
    prec[torch.rand(B, T, P, F, C_, generator=g) < 0.2] = 0.0
    logw = torch.randn(B * n, generator=g)
    counts = [C_, 3]
    fw = [1.0, 0.5, 2.0]
    rel_ = (lambda t: t) if layout == "BPFC" else (lambda t: t.permute(0, 1, 2, 4, 3).contiguous())
    loss = EnsembleCRPSLoss(dec, P, n, counts=counts, layout=layout, unbiased=True, field_weight=fw, fused=False)(out, rel_(fields), precision=rel_(prec), logw=logw)
    assert dec.seen["z"] == (B * T * n, P, G, D) and dec.seen["obs"] == (B * T, P, F, C_) and dec.seen["members"] == n and dec.seen["fused"] is False
    assert torch.equal(dec.seen["logw"].view(B, T, n), logw.view(B, 1, n).expand(B, T, n))
    (grad,) = torch.autograd.grad(loss, out)

    valid = (torch.arange(C_) < torch.tensor(counts)[:, None]).view(1, P, 1, C_)
    total, cells, want = 0.0, 0.0, torch.zeros(B * n, T, G, P * D, dtype=F64)
    for b in range(B):
        for t in range(T):
            zb = torch.stack([torch.stack([torch.stack([out.detach()[b * n + j, t, gi, p * D:(p + 1) * D] for gi in range(G)]) for p in range(P)]) for j in range(n)])   # [n, P, G, D]
            zb = zb.clone().requires_grad_(True)
            Y = dec.decode(zb)
            w = torch.where(valid, prec[b, t].unsqueeze(0).to(F64), torch.zeros((), dtype=F64))
            r = restate_crps_grad(Y.detach(), fields[b, t].unsqueeze(0), w, logw[b * n:(b + 1) * n], n, True, torch.tensor(fw))
            total, cells = total + float(r["loss"].sum()), cells + float(r["count"].sum())
            (dz,) = torch.autograd.grad(Y, zb, r["G"])
            for j in range(n):
                for gi in range(G):
                    for p in range(P):
                        want[b * n + j, t, gi, p * D:(p + 1) * D] = dz[j, p, gi]
    assert cells > 0 and abs(float(loss) - total / cells) <= 1e-6 * abs(total / cells)              # the loss is stored as float32
    assert float((grad - want / cells).abs().max()) <= 1e-6 * float((want / cells).abs().max())


def test_default_rule_sends_refused_shapes_to_the_composed_path():
    """fused=None never resolves to a shape the fused form refuses: a hidden width above 640 in bf16 with 4096+ rows reaches the device check (the
    composed path), not the fused path's ValueError; fused=True on the same shape raises."""
    from sea_amd.models.encoder_decoder import Decode

    dec = Decode([[0, 1], [2]], 8, 648, 8).requires_grad_(False).set_compute_dtype("bf16")
    z, obs = torch.zeros(64 * 64, 1, 2, 8), torch.zeros(64, 1, 3, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dec.member_crps_loss(z, obs, 64)
    with pytest.raises(ValueError, match="carry up to 64 members"):
        dec.member_crps_loss(z, obs, 64, fused=True)


def test_checked_field_weights_are_not_read_back():
    """EnsembleCRPSLoss checks field_weight on the host at construction and marks the per-device copy; Decode takes a marked tensor as it is (no .cpu()
    of a device tensor per call), and checks an unmarked one."""
    from sea_amd.utils.train_utils import EnsembleCRPSLoss

    dec, z, obs, P, F, C_ = _loss_args()
    loss_fn = EnsembleCRPSLoss(dec, P, 2, field_weight=[1.0] * F)
    t = loss_fn._field_weight_on(torch.device("cpu"))
    assert getattr(t, "_sea_checked_field_weight", False) and loss_fn._field_weight_on(torch.device("cpu")) is t
    dec._fw_cache = None
    assert torch.equal(dec._field_weight_on(t, F, torch.device("cpu"), "x"), t) and dec._fw_cache is None      # the host check and its cache were passed over
    plain = torch.ones(F)
    dec._field_weight_on(plain, F, torch.device("cpu"), "x")
    assert dec._fw_cache is not None
