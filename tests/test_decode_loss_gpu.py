"""Decoded-field loss on the device: sea_decode_mse through Decode.mse_loss and FieldSpaceLoss, Decode.forward with a gradient to z.

Reference: the fp64 restatement of the contract in tests/test_decode_loss_cpu.py (`restate`), which reproduces the reference's Decode + F.mse_loss
(tests/golden/decode_mse_*.npz).  Let e(x) be the relative L2 error against it and e_c the error of the composed bf16 path (existing entry points:
forward, sea_mse_fwd_bwd, two data-gradient launches) on the same inputs.  The fused launch must keep e(loss), e(dz) <= 2e-2 (the bf16 decode tolerance,
DESIGN.md section 7) and <= 2 e_c + 1e-6: both paths make the same roundings and differ in summation order only.  fp32 (composed): <= 1e-4.

Shapes, the smallest where the kernel can still go wrong:
  a  groups [[0, 1], [2]], n_inp 12 (Cp 32), hidden 40 (a multiple of 8, not of 32), D 16, P 9, B 2: M = 18 is less than one row tile;
  b  groups [[0], [1], [2]], n_inp 37 (Cp 64, odd: the target gets the row-aligned width 40), hidden 64, D 8, P 4, B 33: M = 132, full tiles + a 4-row tail;
  c  one group [[0, 1]], n_inp 160, hidden 624 (the widest shipped width: the full accumulator budget), D 32, P 2, B 35.
Each runs without counts and with ragged counts that include 0, 1, C - 1 and C."""
import functools
import math

import pytest
import torch

from tests.test_decode_loss_cpu import load_fixture, rel, restate

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL_BF16, TOL_F32 = 2e-2, 1e-4


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs of a shape on the host (float32-representable), computed once and never modified."""
    if name in ("a", "b"):
        fx = load_fixture("decode_mse_" + name)
        return dict(groups=fx["groups"], n_inp=fx["n_inp"], hidden=fx["hidden"], D=fx["D"], B=fx["B"], P=fx["P"], w1=fx["w1"], w2=fx["w2"], b2=fx["b2"],
                    z=fx["z"], target=fx["target"], counts=fx["counts"].tolist())
    g = torch.Generator().manual_seed(23)
    groups, n_inp, hidden, D, B, P = [[0, 1]], 160, 624, 32, 35, 2
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale  # noqa: E731
    return dict(groups=groups, n_inp=n_inp, hidden=hidden, D=D, B=B, P=P, w1=[rn(hidden, D, scale=2.0 / math.sqrt(D))], w2=[rn(2 * n_inp, hidden, scale=2.0 / math.sqrt(hidden))],
                b2=[rn(2 * n_inp, scale=0.1)], z=rn(B, P, 1, D), target=rn(B, P, 2, n_inp), counts=[0, 160])


COUNTS_C2 = [1, 159]   # shape c has two patches: its ragged counts come in two sets, together 0, 1, C - 1, C


@functools.lru_cache(maxsize=None)
def reference(name, counts_key):
    c = case(name)
    counts = None if counts_key is None else list(counts_key)
    loss, dz, _ = restate(c["w1"], c["w2"], c["b2"], c["groups"], c["z"], c["target"], counts)
    return loss, dz


def decoder(name, dtype):
    from sea_amd.models.encoder_decoder import Decode

    c = case(name)
    dec = Decode(c["groups"], c["n_inp"], c["hidden"], c["D"])
    with torch.no_grad():
        for g, m in enumerate(dec.decoders):
            m.layer1.weight.copy_(c["w1"][g])
            m.layer2.weight.copy_(c["w2"][g])
            m.layer2.bias.copy_(c["b2"][g])
    return dec.requires_grad_(False).set_compute_dtype(dtype).to(DEV)


def device_target(name, fill=0.0, width=None):
    """The target in a row-aligned width (n_inp rounded up to 4, or `width`), the pad columns holding `fill`."""
    c = case(name)
    C = c["n_inp"]
    Cw = (C + 3) // 4 * 4 if width is None else width
    t = torch.full(tuple(c["target"].shape[:3]) + (Cw,), fill, dtype=torch.float32)
    t[..., :C] = c["target"]
    return t.to(DEV)


def loss_and_grad(dec, z_host, target, counts, fused):
    z = z_host.to(DEV).requires_grad_(True)
    loss = dec.mse_loss(z, target, counts=counts, fused=fused)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss.backward()
    return loss.detach().cpu(), z.grad.detach().cpu()


def counts_sets(name):
    return [None, case(name)["counts"]] + ([COUNTS_C2] if name == "c" else [])


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fused_loss_and_gradient_against_fp64(name):
    c = case(name)
    dec = decoder(name, "bf16")
    tgt = device_target(name)
    for counts in counts_sets(name):
        ref_loss, ref_dz = reference(name, None if counts is None else tuple(counts))
        loss, dz = loss_and_grad(dec, c["z"], tgt, counts, fused=True)
        loss_c, dz_c = loss_and_grad(dec, c["z"], tgt, counts, fused=False)
        e_loss, e_dz, ec_loss, ec_dz = rel(loss, ref_loss), rel(dz, ref_dz), rel(loss_c, ref_loss), rel(dz_c, ref_dz)
        print(f"decode_mse shape {name} counts {counts}: fused e(loss) {e_loss:.3e} e(dz) {e_dz:.3e}; composed e_c(loss) {ec_loss:.3e} e_c(dz) {ec_dz:.3e}")
        assert e_loss <= TOL_BF16 and e_dz <= TOL_BF16, (counts, e_loss, e_dz)
        assert e_loss <= 2 * ec_loss + 1e-6, (counts, e_loss, ec_loss)
        assert e_dz <= 2 * ec_dz + 1e-6, (counts, e_dz, ec_dz)
        if counts is not None:   # a patch without valid slots gets no gradient
            for p, n in enumerate(counts):
                if n == 0:
                    assert float(dz[:, p].abs().max()) == 0.0


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fp32_composed_path_against_fp64(name):
    c = case(name)
    dec = decoder(name, "fp32")
    tgt = device_target(name)
    for counts in counts_sets(name)[:2]:
        ref_loss, ref_dz = reference(name, None if counts is None else tuple(counts))
        loss, dz = loss_and_grad(dec, c["z"], tgt, counts, fused=None)
        print(f"decode_mse shape {name} counts {counts}: fp32 e(loss) {rel(loss, ref_loss):.3e} e(dz) {rel(dz, ref_dz):.3e}")
        assert rel(loss, ref_loss) <= TOL_F32 and rel(dz, ref_dz) <= TOL_F32


def test_unaligned_target_width_is_accepted():
    """C == n_inp = 37 (rows of 37 floats: not 16-byte aligned) gives the bits of the row-aligned target."""
    c = case("b")
    dec = decoder("b", "bf16")
    a = loss_and_grad(dec, c["z"], device_target("b"), c["counts"], fused=True)
    b = loss_and_grad(dec, c["z"], c["target"].to(DEV), c["counts"], fused=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("fill", [1e30, float("nan")])
def test_invalid_slots_and_pad_columns_are_exactly_neutral(name, fill):
    c = case(name)
    dec = decoder(name, "bf16")
    C, counts = c["n_inp"], c["counts"]
    width = C + 4 if C % 4 == 0 else None                     # shape a: four pad columns behind the cell; shape b: 37 -> 40
    clean = device_target(name, 0.0, width)
    base = loss_and_grad(dec, c["z"], clean, counts, fused=True)
    dirty = device_target(name, fill, width)                  # columns [C, width)
    for p, n in enumerate(counts):                            # slots at or beyond the patch's count
        dirty[:, p, :, n:] = fill
    got = loss_and_grad(dec, c["z"], dirty, counts, fused=True)
    assert torch.equal(base[0], got[0]) and torch.equal(base[1], got[1])
    assert bool(torch.isfinite(got[0])) and bool(torch.isfinite(got[1]).all())
    # without counts the pad columns alone
    base = loss_and_grad(dec, c["z"], clean, None, fused=True)
    got = loss_and_grad(dec, c["z"], device_target(name, fill, width), None, fused=True)
    assert torch.equal(base[0], got[0]) and torch.equal(base[1], got[1])
    for p, n in enumerate(counts):
        if n == 0:
            assert float(loss_and_grad(dec, c["z"], clean, counts, fused=True)[1][:, p].abs().max()) == 0.0


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_two_runs_give_the_same_bits(name):
    c = case(name)
    dec = decoder(name, "bf16")
    tgt = device_target(name)
    for counts in counts_sets(name)[:2]:
        a = loss_and_grad(dec, c["z"], tgt, counts, fused=True)
        b = loss_and_grad(dec, c["z"], tgt, counts, fused=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _decode_fp64(c, z, cot):
    """d <Decode(z), cot> / d z in fp64 through torch.autograd."""
    f64 = torch.float64
    z = z.to(f64).clone().requires_grad_(True)
    B, P, G, D = z.shape
    outs = []
    for g, grp in enumerate(c["groups"]):
        pre = z[:, :, g] @ c["w1"][g].to(f64).t()
        h = 0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0)))
        outs.append((h @ c["w2"][g].to(f64).t() + c["b2"][g].to(f64)).view(B, P, len(grp), -1))
    y = torch.cat(outs, 2)
    (y * cot.to(f64)).sum().backward()
    return y.detach(), z.grad


@pytest.mark.parametrize("name,dtype,tol", [("a", "bf16", TOL_BF16), ("b", "bf16", TOL_BF16), ("b", "fp32", TOL_F32), ("a", "fp32", TOL_F32)])
def test_forward_with_grad(name, dtype, tol):
    c = case(name)
    dec = decoder(name, dtype)
    zd = c["z"].to(DEV)
    with torch.no_grad():
        y0 = dec(zd).clone()                                   # before the grad path or mse_loss was ever used on this decoder
    z = zd.clone().requires_grad_(True)
    y1 = dec(z)
    assert y1.grad_fn is not None and y1.shape == y0.shape
    assert torch.equal(y1.detach(), y0)                        # the same values as the inference forward
    cot = torch.randn(y0.shape, generator=torch.Generator().manual_seed(5))
    y1.backward(cot.to(DEV))                                   # an arbitrary downstream loss: a fixed random cotangent
    y_ref, dz_ref = _decode_fp64(c, c["z"], cot)
    print(f"decode forward-with-grad {name} {dtype}: e(y) {rel(y1.detach().cpu(), y_ref):.3e} e(dz) {rel(z.grad.cpu(), dz_ref):.3e}")
    assert rel(y1.detach().cpu(), y_ref) <= tol and rel(z.grad.cpu(), dz_ref) <= tol
    dec.mse_loss(zd.clone().requires_grad_(True), device_target(name), counts=c["counts"]).backward()
    with torch.no_grad():
        assert torch.equal(dec(zd), y0)                        # the inference forward launches what it launched before
    assert torch.equal(dec(zd.clone().requires_grad_(False)), y0)
    trainable = decoder(name, dtype).requires_grad_(True)
    with pytest.raises(ValueError, match=r"requires_grad_\(False\)"):
        trainable(z)


def test_fused_path_never_allocates_a_layer2_output():
    """A condition, not a measurement: loss + backward on the fused path may raise the peak of allocated memory by less than ONE layer-2 output
    (M * n_fields * Cp * 4 bytes); the composed path on the same inputs exceeds that, so the bound is not vacuous."""
    from sea_amd.models.encoder_decoder import Decode

    B, P, n_inp, hidden, D = 64, 64, 160, 64, 8
    groups = [[0, 1], [2]]
    torch.manual_seed(3)
    dec = Decode(groups, n_inp, hidden, D).requires_grad_(False).set_compute_dtype("bf16").to(DEV)
    M, n_fields, Cp = B * P, 3, dec._n_inp_p
    bound = M * n_fields * Cp * 4
    z = torch.randn(B, P, 2, D, device=DEV)
    tgt = torch.randn(B, P, n_fields, n_inp, device=DEV)

    def rise(fused):
        zz = z.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        loss = dec.mse_loss(zz, tgt, fused=fused)
        loss.backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, loss.item(), zz.grad

    rise(True), rise(False)    # shadow copies of the weights and the allocator's pools exist from here on
    r_fused, l_fused, g_fused = rise(True)
    r_comp, l_comp, g_comp = rise(False)
    print(f"decode_mse peak extra memory at M = {M}: fused {r_fused} B, composed {r_comp} B, one layer-2 output {bound} B")
    assert r_fused < bound, (r_fused, bound)
    assert r_comp > bound, (r_comp, bound)
    assert abs(l_fused - l_comp) <= 1e-3 * abs(l_comp) and rel(g_fused.cpu(), g_comp.cpu()) <= TOL_BF16


def test_field_space_loss_trains_the_temporal_model():
    """FieldSpaceLoss(model(x, ib), fields).backward() fills the temporal parameters' gradients as the composed path does, and one optimizer step
    lowers the loss."""
    from oracle.recipe import recipe_inputs
    from sea_amd.utils.train_utils import FieldSpaceLoss, initialize_optimizer
    from tests.test_input_grad_gpu import cfg_of
    from tests.test_model_gpu import build, gpu

    c = case("a")
    P, D, G = 4, c["D"], len(c["groups"])
    cfg = cfg_of(1, P * D, 4, G)
    B, T = 2, 7
    x, _, ib = recipe_inputs(B, T, cfg, seed=9)
    fields = torch.randn(B, T, P, 3, c["n_inp"], generator=torch.Generator().manual_seed(4)).to(DEV)
    counts = [12, 0, 7, 11]
    dec = decoder("a", "bf16")

    def grads(fused):
        m = build(cfg, "fp32").train()
        loss_fn = FieldSpaceLoss(dec, P, counts=counts, fused=fused)
        loss = loss_fn(m(gpu(x), gpu(ib)), fields)
        loss.backward()
        return m, loss_fn, loss.item(), {k: p.grad.detach().cpu() for k, p in m.named_parameters() if p.grad is not None}

    m, loss_fn, l_fused, g_fused = grads(True)
    _, _, l_comp, g_comp = grads(False)
    assert abs(l_fused - l_comp) <= 1e-3 * abs(l_comp)
    live = [k for k, g in g_comp.items() if float(g.norm()) > 0.0]   # some parameters never receive a gradient
    assert len(live) >= 10
    worst = max(rel(g_fused[k], g_comp[k]) for k in live)
    print(f"field-space loss end to end: loss fused {l_fused:.6f} composed {l_comp:.6f}, worst parameter-gradient difference {worst:.3e} over {len(live)} tensors")
    assert worst <= TOL_BF16
    # the reference's layout gives the same loss
    l_ref_layout = FieldSpaceLoss(dec, P, counts=counts, layout="BPCF")(m(gpu(x), gpu(ib)), fields.permute(0, 1, 2, 4, 3).contiguous()).item()
    assert abs(l_ref_layout - l_fused) <= 1e-6 * abs(l_fused)
    m = build(cfg, "fp32").train()
    opt = initialize_optimizer(m, dict(learning_rate=1e-3))
    opt.zero_grad()
    loss = loss_fn(m(gpu(x), gpu(ib)), fields)
    loss.backward()
    opt.step()
    with torch.no_grad():
        after = loss_fn(m(gpu(x), gpu(ib)), fields).item()
    assert after < loss.item(), (after, loss.item())
