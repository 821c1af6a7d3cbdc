"""The condition-gradient entry points against fp64 at edge shapes: sea_silu_outer_bwd_dc (the AdaLN condition MLPs) and sea_ib_bwd_dc (the
information-bottleneck layer, all three ib_scale_modes).  dc is ADDED to a non-zero buffer; the parameter gradients the same calls produce equal those of
sea_silu_outer_bwd / sea_ib_bwd to rounding."""
import ctypes
import math

import pytest
import torch

from sea_amd import _native as N
from sea_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _rnd(*shape, g, scale=1.0):
    return torch.randn(*shape, generator=g, device=DEV) * scale


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("K2,n_groups", [(4, 1), (64, 1), (2048, 1), (4, 30), (64, 30), (2048, 26)])
@pytest.mark.parametrize("M", [1, 3, 63, 65, 4097])
def test_silu_outer_bwd_dc_matches_fp64(M, K2, n_groups, dtype):
    g = _gen(M * 7 + K2 + n_groups)
    c = torch.rand(M, generator=g, device=DEV) * 2 - 0.5
    groups, ref_groups = [], []
    for _ in range(n_groups):
        w1, b1 = _rnd(K2, g=g, scale=0.5), _rnd(K2, g=g, scale=0.2)
        dHid = _rnd(M, K2, g=g).to(dtype)
        groups.append(dict(dHid=dHid, w1=w1, b1=b1, dw1=torch.zeros(K2, device=DEV), db1=torch.zeros(K2, device=DEV)))
    dc0 = _rnd(M, g=g)
    dc = dc0.clone()
    for s in range(0, n_groups, N.MAX_SILU_BWD_GROUPS):   # one launch carries at most MAX_SILU_BWD_GROUPS groups: the launches add into one dc
        ops.silu_outer_bwd_dc(groups[s:s + N.MAX_SILU_BWD_GROUPS], c, dc, M, dtype)
    ref_dc = dc0.double().clone()
    cd = c.double()
    for gr in groups:
        pre = cd[:, None] * gr["w1"].double() + gr["b1"].double()
        sg = torch.sigmoid(pre)
        dpre = gr["dHid"].double() * sg * (1 + pre * (1 - sg))
        ref_dc += (dpre * gr["w1"].double()).sum(1)
        assert rel(gr["dw1"], (dpre * cd[:, None]).sum(0)) < 1e-4
        assert rel(gr["db1"], dpre.sum(0)) < 1e-4
    assert rel(dc - dc0, ref_dc - dc0.double()) < 1e-4
    # the parameter gradients equal those of sea_silu_outer_bwd
    for s in range(0, n_groups, N.MAX_SILU_BWD_GROUPS):
        chunk = groups[s:s + N.MAX_SILU_BWD_GROUPS]
        plain = [dict(gr, dw1=torch.zeros(K2, device=DEV), db1=torch.zeros(K2, device=DEV)) for gr in chunk]
        ws = torch.empty(len(chunk) * min((M + 3) // 4, 256) * 2 * K2, device=DEV)
        ops.silu_outer_bwd(plain, c, M, dtype, ws=ws)
        for a, b in zip(chunk, plain):
            assert torch.allclose(a["dw1"], b["dw1"], rtol=1e-5, atol=1e-5 * float(b["dw1"].abs().max()))
            assert torch.allclose(a["db1"], b["db1"], rtol=1e-5, atol=1e-5 * float(b["db1"].abs().max()))


def _ib_reference(mode, c, dX, layer, masks):
    """dc of sum_f <dX_f, mask_f * ib(c)> in fp64 by autograd: the layer as the oracle states it (oracle/sea_oracle.py info_bottleneck)."""
    cd = c.double().clone().requires_grad_(True)
    col = cd[:, None]
    if mode == 0:
        pre = col * layer["w1"].double() + layer["b1"].double()
        hid = torch.nn.functional.gelu(torch.nn.functional.layer_norm(pre, (pre.shape[1],), layer["lnw"].double(), layer["lnb"].double(), 1e-5))
        ib = hid @ layer["w2"].double().t() + layer["b2"].double()
    elif mode == 1:
        ib = col * layer["w1"].double() + layer["b1"].double()
    else:
        proj = (col * layer["w1"].double()) * 2 * math.pi
        ib = torch.cat([torch.sin(proj), torch.cos(proj)], dim=-1)
    tot = sum(((m if m is not None else 1.0) * ib * d.double()).sum() for d, m in zip(dX, masks))
    (g,) = torch.autograd.grad(tot, [cd])
    return g


# (mode, h, E, fields, dropout on the layer's output — the 'mlp' layer only has it)
IB_CASES = [(0, 1, 8, 1, False), (0, 8, 264, 3, False), (0, 64, 2048, 2, False), (0, 8, 2048, 8, False), (0, 64, 8, 1, False),
            (0, 1, 8, 2, True), (0, 8, 264, 3, True), (0, 64, 2048, 8, True),
            (1, 0, 8, 1, False), (1, 0, 264, 5, False), (1, 0, 2048, 8, False), (2, 0, 8, 1, False), (2, 0, 264, 4, False), (2, 0, 2048, 8, False)]


@pytest.mark.parametrize("mode,h,E,fields,drop", IB_CASES)
@pytest.mark.parametrize("M", [1, 65, 4097])
def test_ib_bwd_dc_matches_fp64(M, mode, h, E, fields, drop):
    g = _gen(M + 31 * E + h + fields + mode)
    c = torch.rand(M, generator=g, device=DEV)
    dX = [_rnd(M, E, g=g) for _ in range(fields)]
    if mode == 0:
        layer = dict(w1=_rnd(h, g=g), b1=_rnd(h, g=g, scale=0.1), lnw=1 + _rnd(h, g=g, scale=0.1), lnb=_rnd(h, g=g, scale=0.1), w2=_rnd(E, h, g=g, scale=0.3),
                     b2=_rnd(E, g=g, scale=0.1))
    elif mode == 1:
        layer = dict(w1=_rnd(E, g=g), b1=_rnd(E, g=g, scale=0.1))
    else:
        layer = dict(w1=_rnd(E // 2, g=g))
    dropt, masks = None, [None] * fields
    if drop:
        thr, seed, stream = 26, 1234, 5
        dropt = (seed, stream, thr)
        masks = []
        for f in range(fields):
            mk = torch.empty(M, E, device=DEV)
            N.check(N.lib().sea_dropout_mask(mk.data_ptr(), M, E, seed, stream + f, thr, N.stream_ptr()), "mask")
            masks.append(mk.double())
    dc0 = _rnd(M, g=g)
    dc = dc0.clone()
    lk = {k: v for k, v in layer.items() if k != "b2"}   # (b2 does not reach the gradient)
    ops.ib_bwd_dc(dX, c, dc, mode=mode, drop=dropt, **lk)
    ref = _ib_reference(mode, c, dX, layer, masks)
    assert rel(dc - dc0, ref) < 1e-4, rel(dc - dc0, ref)
    # with the parameter gradients asked for, they equal sea_ib_bwd's (where sea_ib_bwd takes the shape: its one-wave-per-row form holds E (h + 1)
    # floats in LDS)
    if mode == 2 or (mode == 0 and E * (h + 1) * 4 > 160 * 1024):
        return
    names = ("dw1", "db1", "dlnw", "dlnb", "dw2", "db2") if mode == 0 else ("dw1", "db1")
    shapes = dict(dw1=layer["w1"].shape, db1=layer["b1"].shape, dlnw=(h,), dlnb=(h,), dw2=(E, h), db2=(E,))
    mine = {k: torch.zeros(shapes[k], device=DEV) for k in names}
    theirs = {k: torch.zeros(shapes[k], device=DEV) for k in names}
    dc2 = torch.zeros(M, device=DEV)
    ops.ib_bwd_dc(dX, c, dc2, mode=mode, drop=dropt, **lk, **mine)
    P = N.SeaIbBwdParams()
    ops.fill_ib_bwd_params(P, dX, c, mode=mode, drop=dropt, **lk, **theirs)
    N.check(N.lib().sea_ib_bwd(ctypes.byref(P), N.stream_ptr()), "sea_ib_bwd")
    for k in names:
        scale = float(theirs[k].abs().max()) + 1e-30
        assert torch.allclose(mine[k], theirs[k], rtol=1e-5, atol=1e-5 * scale), k
    assert rel(dc2, ref) < 1e-4
