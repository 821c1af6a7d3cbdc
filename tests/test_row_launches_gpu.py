"""The row-owning launches of the rollout step — sea_mlp_fc1_ln_gelu, sea_mlp_fc2_proj_norm, sea_mlp_block, sea_gemm_adaln, sea_exchange_tail, sea_row_chain,
sea_row_chain_riders, sea_adaln_qkv — per row against fp64 at the edges of their row tiles, in the discipline of test_forced_forms_gpu.py.

Reference: the fp64 formula of include/sea_hip.h on the operands as rounded to bf16, NO intermediate rounded.  Two checks per output:

  global  ||out - ref|| / ||ref|| at the bound test_ops_gpu.py uses for that output (6e-3 a bf16 output, 1.2e-2 Q / K / V behind a chain, 1.5e-2 behind
          sea_adaln_qkv, 8e-3 sea_mlp_block; 2e-5 an fp32 output with nothing rounded upstream).  An fp32 output BEHIND a rounded operand (form B's X behind
          the rounded g; down.Y32 / mean / rstd behind the rounded x; Y32 of the MLP launches behind the rounded x3) has no bound there against an un-rounded
          reference: it takes the bound of the bf16 output of the same launch, whose error it shares up to the last rounding.
  local   max over rows ||err_row|| / rms over rows ||ref_row|| (rowerr): a row per head for Q / K / V, one row for mean / rstd.

Local bounds (LOCAL): 3 x the largest rowerr(emulation, reference) over every case of this file, where the emulation is the same fp64 formula with a rounding to
bf16 at exactly the points where the kernels round (named in each *_formula); with the rounding off it restates the reference to 1e-12.  Both are checked and
measured on the CPU by `python tests/test_row_launches_gpu.py`, which prints the worst case per output kind.  fp32 outputs with nothing rounded upstream: 4 x 2e-5.

Every launch: outputs in NaN frames, caches pre-filled with NaN (outside [pos0, pos0 + T) still NaN afterwards, inside finite), every row-major input the first M
rows of a tensor one full tile taller whose extra rows are NaN, ops.last_form() asserted right after the launch."""
import math
import os
import sys

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.test_forced_forms_gpu import BF, dev, force, frame_untouched, framed, gelu64, rel, rnd, rope64, rope_table, rowerr  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
F32_GLOBAL, F32_LOCAL = 2e-5, 4 * 2e-5
# 3 x the largest rowerr(emulation, reference) over every case of the file (python tests/test_row_launches_gpu.py, on the CPU); the measured value and its case:
LOCAL = {
    "fc1.Hg": 3 * 2.907e-03,   # mlp (128, 1024, (2750, 2752, 2753), 0) group 2 (ln, None)
    "fc2.Y32": 3 * 2.441e-03,   # mlp (256, 2048, (2750, 2752, 2753), 0) group 0 (None, ln)
    "fc2.Yact": 3 * 3.125e-03,   # mlp (128, 1024, (2750, 2752, 2753), 0) group 2 (ln, None)
    "blk.Y32": 3 * 2.925e-03,   # mlp (128, 1024, (2750, 2752, 2753), 0) group 1 (adaln_add, adaln)
    "blk.Yact": 3 * 3.431e-03,   # mlp (128, 1024, (2750, 2752, 2753), 0) group 1 (adaln_add, adaln)
    "adaln.Yact": 3 * 2.456e-03,   # gemm_adaln d=64 K=72 group 4 M=65
    "adaln.mod": 3 * 2.180e-03,   # gemm_adaln d=64 K=72 group 5 M=65
    "tail.X": 3 * 2.077e-03,   # exchange_tail D=128 S=2 group 2 M=17
    "tail.Xact": 3 * 3.118e-03,   # exchange_tail D=128 S=2 group 2 M=17
    "tail.Y32": 3 * 2.556e-03,   # exchange_tail D=64 S=4 group 2 M=17
    "tail.Yact": 3 * 3.337e-03,   # exchange_tail D=64 S=4 group 1 M=16
    "tail.mean": 3 * 3.048e-03,   # exchange_tail D=64 S=4 group 1 M=16
    "tail.rstd": 3 * 5.024e-04,   # exchange_tail D=128 S=1 group 1 M=16
    "chain.X": 3 * 2.109e-03,   # row_chain D=128 hd=32 form B B=1 T=17 pos0=0
    "chain.Xact": 3 * 3.053e-03,   # row_chain D=64 hd=32 form B B=3 T=11 pos0=3
    "chain.Y32": 3 * 3.359e-03,   # row_chain D=64 hd=16 form B B=1 T=17 pos0=0
    "chain.Yact": 3 * 3.654e-03,   # row_chain D=64 hd=16 form B B=2 T=17 pos0=0
    "chain.mean": 3 * 3.724e-03,   # row_chain D=128 hd=16 form B B=1 T=16 pos0=3
    "chain.rstd": 3 * 5.331e-04,   # row_chain D=64 hd=16 form B B=1 T=15 pos0=0
    "chain.Q": 3 * 5.792e-03,   # row_chain D=128 hd=16 form B B=2 T=17 pos0=0
    "chain.K": 3 * 5.317e-03,   # row_chain D=128 hd=16 form B B=1 T=15 pos0=3
    "chain.V": 3 * 5.549e-03,   # row_chain D=128 hd=16 form B B=1 T=17 pos0=3
    "rider.C": 3 * 1.971e-03,   # chain rider group 1
    "aqkv.Q": 3 * 4.888e-03,   # adaln_qkv H=16 B=1 T=33 pos0=3 third=False field 0
    "aqkv.K": 3 * 4.640e-03,   # adaln_qkv H=16 B=1 T=33 pos0=3 third=False field 0
    "aqkv.V": 3 * 4.566e-03,   # adaln_qkv H=16 B=1 T=31 pos0=0 third=False field 1
    "aqkv.mod3": 3 * 3.167e-03,   # adaln_qkv H=8 B=1 T=33 pos0=0 third=True field 0
    "aqkv.Hid": 3 * 2.323e-03,   # adaln_qkv silu rider rows=65 group 1
}
GLOBAL = {"fc1.Hg": 6e-3, "fc2.Y32": 6e-3, "fc2.Yact": 6e-3, "blk.Y32": 8e-3, "blk.Yact": 8e-3, "adaln.Yact": 6e-3, "adaln.mod": 6e-3,
          "tail.X": 6e-3, "tail.Xact": 6e-3, "tail.Y32": 6e-3, "tail.Yact": 6e-3, "tail.mean": 6e-3, "tail.rstd": 6e-3,
          "chain.X": 6e-3, "chain.Xact": 6e-3, "chain.Y32": 6e-3, "chain.Yact": 6e-3, "chain.mean": 6e-3, "chain.rstd": 6e-3,
          "chain.Q": 1.2e-2, "chain.K": 1.2e-2, "chain.V": 1.2e-2, "rider.C": 6e-3,
          "aqkv.Q": 1.5e-2, "aqkv.K": 1.5e-2, "aqkv.V": 1.5e-2, "aqkv.mod3": 6e-3, "aqkv.Hid": 6e-3}


# ------------------------------------------------------------------------------------------------ helpers
def rounder(rt):
    return (lambda t: t.to(rt).double()) if rt is not None else (lambda t: t)


def ln64(v, eps=1e-5):
    """(xhat, mean, rstd) of the rows of v: biased variance, as SeaNormGroup."""
    mu = v.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((v - mu) ** 2).mean(-1, keepdim=True) + eps)
    return (v - mu) * rstd, mu[..., 0], rstd[..., 0]


def modulate(xh, gamma, beta, mod):
    """SeaNormGroup: y = xhat (gamma + (mod ? 1 + mod[:, :d] : 0)) + (beta + (mod ? mod[:, d:] : 0))."""
    d = xh.shape[-1]
    b = beta.double() if beta is not None else 0.0
    if mod is None:
        return xh * gamma.double() + b
    return xh * (gamma.double() + 1 + mod.double()[:, :d]) + (b + mod.double()[:, d:])


def tall(t, extra):
    """The first M rows of a tensor `extra` rows taller whose extra rows are NaN (t itself when it is None)."""
    if t is None:
        return None
    big = torch.full((t.shape[0] + extra,) + tuple(t.shape[1:]), NAN, device=t.device, dtype=t.dtype)
    big[:t.shape[0]] = t
    return big[:t.shape[0]]


def tall_cols(t, extra, c0, c1):
    """tall() of a wider tensor, then its columns [c0, c1): rows inside the caller's strided layout."""
    return tall(t, extra)[:, c0:c1]


def guarded(shape, dtype, pad=64, device=None):
    """(whole, view): a contiguous NaN tensor of `shape` with `pad` NaN elements in front of it and behind it."""
    n = math.prod(shape)
    flat = torch.full((n + 2 * pad,), NAN, device=device if device is not None else dev(), dtype=dtype)
    return flat, flat[pad:pad + n].view(shape)


def guard_untouched(flat, pad=64):
    return bool(torch.isnan(flat[:pad].float()).all() and torch.isnan(flat[-pad:].float()).all())


def out2d(M, N_, dtype):
    """A framed [M, N] output: (frame, view)."""
    return framed(M, N_, dtype)


_SEEN = {}   # kind -> [worst global, worst local, checks] of the running test


def errors(out, ref, row=None):
    """(global, local) error of one output; row: the row length (a row per head), None: the output's own rows."""
    o, r = (out, ref) if row is None else (out.reshape(-1, row), ref.reshape(-1, row))
    return rel(out, ref), rowerr(o, r)


def check(kind, out, ref, what, row=None, f32=False, g32=F32_GLOBAL):
    """Both checks of one output; row: the row length (a row per head).  f32: an fp32 output with nothing rounded upstream."""
    assert torch.isfinite(out.float()).all(), (what, kind, "not finite")
    eg, el = errors(out, ref, row)
    gb, lb = (g32, F32_LOCAL) if f32 else (GLOBAL[kind], LOCAL[kind])
    print(f"{what} {kind}: global {eg:.3e} (< {gb:.1e})  local {el:.3e} (< {lb:.3e})")
    w = _SEEN.setdefault(kind, [0.0, 0.0, 0, gb, lb])
    w[0], w[1], w[2] = max(w[0], eg), max(w[1], el), w[2] + 1
    assert eg < gb, (what, kind, "global", eg, gb)
    assert el < lb, (what, kind, "local", el, lb)


@pytest.fixture(autouse=True)
def _one_line_per_test(request):
    """The line of profiles/row_launches_gpu_errors.txt: the largest global and local error of every output kind the test checked, beside their bounds."""
    _SEEN.clear()
    yield
    if _SEEN:
        print("ROW_LAUNCHES " + request.node.name + ": " + "; ".join(
            f"{k} global {w[0]:.3e} (< {w[3]:.1e}) local {w[1]:.3e} (< {w[4]:.3e}) over {w[2]}" for k, w in sorted(_SEEN.items())))


def launched(ops, form):
    """ops.last_form() right after the launch, before the synchronise."""
    got = ops.last_form()
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:   # a device fault: nothing more is started on this device
        pytest.exit(f"device error behind {got}: {e}", returncode=3)
    assert got[0] == form, (form, got)
    return got


def cache_window(kind, cache, ref, pos0, T, hd, what, transposed=False):
    """A cache [B, H, cap, hd] (transposed: [B, H, hd, cap]) that was NaN before the launch: positions [pos0, pos0 + T) against ref [B, H, T, hd], a row per head;
    every other position still NaN."""
    c = cache.transpose(2, 3) if transposed else cache
    assert bool(torch.isnan(c[:, :, :pos0].float()).all()) and bool(torch.isnan(c[:, :, pos0 + T:].float()).all()), (what, kind, "outside the window")
    check(kind, c[:, :, pos0:pos0 + T], ref, what, row=hd)


# ------------------------------------------------------------------------------------------------ the field MLP: fc1, fc2, the block
MLP_SHAPES = [(256, 2048), (128, 1024)]
MLP_EDGE_MS = [(1, 31, 33), (32, 64, 65)]       # a group's first tile follows another group's ragged one
MLP_ROUNDS_MS = (2750, 2752, 2753)              # 86 + 86 + 87 = 259 tiles -> per_xcd = 33, 264 launched: dead tiles, a group boundary inside an XCD's range
MLP_PROLOGUES = (None, "adaln_add", "ln")
MLP_NORMS = (None, "ln", "adaln")


def mlp_cases():
    """(E, S, Ms, rot): group i takes prologue (i + rot) % 3 and final norm (i + 2 rot + 1) % 3 — every prologue and every norm on every edge row count."""
    cases = [(E, S, Ms, rot) for E, S in MLP_SHAPES for Ms in MLP_EDGE_MS for rot in range(3)]
    return cases + [(E, S, MLP_ROUNDS_MS, 0) for E, S in MLP_SHAPES]


def mlp_group(E, S, M, pro, norm, seed, device=None):
    """The operands of one group of the three MLP launches (32 NaN rows behind every row-major input)."""
    kw = dict(device=device)
    g = dict(E=E, S=S, M=M, pro=pro, norm=norm,
             W1=rnd(S, E, dtype=BF, scale=0.08, seed=seed + 1, **kw), b1=0.2 * rnd(S, seed=seed + 2, **kw),
             lnw=1 + 0.1 * rnd(S, seed=seed + 3, **kw), lnb=0.1 * rnd(S, seed=seed + 4, **kw),
             W2=rnd(E, S, dtype=BF, scale=0.03, seed=seed + 5, **kw), b2=0.2 * rnd(E, seed=seed + 6, **kw),
             Wp=rnd(E, E, dtype=BF, scale=0.08, seed=seed + 7, **kw), bp=0.2 * rnd(E, seed=seed + 8, **kw),
             x=tall(rnd(M, E, seed=seed + 9, **kw) * 1.3 + 0.2, 32), Hg_in=tall(rnd(M, S, dtype=BF, seed=seed + 10, **kw), 32),
             gamma=(1 + 0.1 * rnd(E, seed=seed + 11, **kw)) if norm else None, beta=0.1 * rnd(E, seed=seed + 12, **kw) if norm == "adaln" else None,
             mod=tall(rnd(M, 2 * E, dtype=BF, scale=0.3, seed=seed + 13, **kw), 32) if norm == "adaln" else None,
             A=None, add=None, pmod=None, pg=None, pb=None)
    if pro is None:
        g["A"] = tall(rnd(M, E, dtype=BF, seed=seed + 14, **kw), 32)
    else:
        g["pg"] = 1 + 0.1 * rnd(E, seed=seed + 15, **kw)
        if pro == "adaln_add":
            g.update(add=tall(0.5 * rnd(M, E, seed=seed + 16, **kw), 32), pb=0.1 * rnd(E, seed=seed + 17, **kw),
                     pmod=tall(rnd(M, 2 * E, dtype=BF, scale=0.3, seed=seed + 18, **kw), 32))
    return g


def mlp_groups(E, S, Ms, rot, device=None):
    return [mlp_group(E, S, M, MLP_PROLOGUES[(i + rot) % 3], MLP_NORMS[(i + 2 * rot + 1) % 3], 7000 + 100 * i + E + 31 * M, device) for i, M in enumerate(Ms)]


def mlp_formula(g, rt=None):
    """Hg of sea_mlp_fc1_ln_gelu, Y of sea_mlp_fc2_proj_norm on Hg_in and R = x, Y of sea_mlp_block (residual: x + addend with a prologue, else x).  Rounded where
    the kernels round: the normalised rows (operand of fc1), the hidden rows (stored by fc1; operand of fc2 in the block), x3 (operand of proj); the act outputs."""
    r = rounder(rt)
    E = g["E"]
    res = g["x"].double() + (g["add"].double() if g["add"] is not None else 0.0)
    a = g["A"].double() if g["pro"] is None else r(modulate(ln64(res)[0], g["pg"], g["pb"], g["pmod"]))
    h = gelu64(ln64(a @ g["W1"].double().t() + g["b1"].double())[0] * g["lnw"].double() + g["lnb"].double())

    def tail(hid, resid):
        x3 = r(hid @ g["W2"].double().t() + g["b2"].double() + resid)
        y = x3 @ g["Wp"].double().t() + g["bp"].double()
        return modulate(ln64(y)[0], g["gamma"], g["beta"], g["mod"]) if g["norm"] else y

    y2, yb = tail(g["Hg_in"].double(), g["x"].double()), tail(r(h), res if g["pro"] is not None else g["x"].double())
    return {"fc1.Hg": r(h), "Xout": res, "fc2.Y32": y2, "fc2.Yact": r(y2), "blk.Y32": yb, "blk.Yact": r(yb)}


_MLP_REF = {}


def _mlp_ref(case):
    """(groups, fp64 references) of one case, computed once per session and left unchanged."""
    if case not in _MLP_REF:
        groups = mlp_groups(*case)
        _MLP_REF[case] = (groups, [mlp_formula(g) for g in groups])
    return _MLP_REF[case]


def _first(g, Hg=None, Xout=None):
    d = dict(W1=g["W1"], b1=g["b1"], lnw=g["lnw"], lnb=g["lnb"])
    if Hg is not None:
        d["Hg"] = Hg
    if g["pro"] is None:
        d["A"] = g["A"]
    else:
        d["norm"] = dict(X32=g["x"], gamma=g["pg"], beta=g["pb"], mod=g["pmod"], addend=g["add"], Xout=Xout)
    return d


def _per_xcd(Ms):
    total = sum((M + 31) // 32 for M in Ms)
    return ((total + 7) // 8, 8 * ((total + 7) // 8)) if total > 256 else (0, total)


@pytest.mark.parametrize("case", mlp_cases(), ids=str)
def test_mlp_fc1_rows(case):
    from sea_amd import ops

    E, S, Ms, rot = case
    groups, refs = _mlp_ref(case)
    outs = [(out2d(g["M"], S, BF), out2d(g["M"], E, torch.float32) if g["pro"] else None) for g in groups]
    ops.mlp_fc1_ln_gelu([_first(g, Hg=o[0][1], Xout=o[1][1] if o[1] else None) for g, o in zip(groups, outs)])
    got = launched(ops, "mlp_fc1.rows32")
    assert got[1:] == _per_xcd(Ms), got
    if Ms == MLP_ROUNDS_MS:
        assert got[1] > 0, got
    for i, (g, ref, ((hbig, Hg), xo)) in enumerate(zip(groups, refs, outs)):
        what = f"mlp_fc1 {case} group {i} ({g['pro']})"
        check("fc1.Hg", Hg, ref["fc1.Hg"], what)
        assert frame_untouched(hbig, S), what
        if xo is not None:
            want = g["x"] + g["add"] if g["add"] is not None else g["x"]
            assert torch.equal(xo[1], want), (what, "Xout is not x + addend bit for bit")
            assert frame_untouched(xo[0], E), what


@pytest.mark.parametrize("case", mlp_cases(), ids=str)
def test_mlp_fc2_rows(case):
    from sea_amd import ops

    E, S, Ms, rot = case
    groups, refs = _mlp_ref(case)
    outs = [(out2d(g["M"], E, torch.float32), out2d(g["M"], E, BF)) for g in groups]
    ops.mlp_fc2_proj_norm([dict(Hg=g["Hg_in"], W2=g["W2"], b2=g["b2"], R=g["x"], Wproj=g["Wp"], bproj=g["bp"], Y32=o[0][1], Yact=o[1][1], gamma=g["gamma"],
                                beta=g["beta"], mod=g["mod"]) for g, o in zip(groups, outs)])
    got = launched(ops, "mlp_fc2.rows32")
    assert got[1:] == _per_xcd(Ms), got
    if Ms == MLP_ROUNDS_MS:
        assert got[1] > 0, got
    for i, (g, ref, ((big32, Y32), (bigact, Yact))) in enumerate(zip(groups, refs, outs)):
        what = f"mlp_fc2 {case} group {i} ({g['norm']})"
        check("fc2.Y32", Y32, ref["fc2.Y32"], what)
        check("fc2.Yact", Yact, ref["fc2.Yact"], what)
        assert frame_untouched(big32, E) and frame_untouched(bigact, E), what


@pytest.mark.parametrize("case", mlp_cases(), ids=str)
def test_mlp_block_rows(case):
    from sea_amd import ops

    E, S, Ms, rot = case
    groups, refs = _mlp_ref(case)
    outs = [(out2d(g["M"], E, torch.float32), out2d(g["M"], E, BF)) for g in groups]
    ops.mlp_block([dict(_first(g), W2=g["W2"], b2=g["b2"], R=(g["x"] if g["pro"] is None else None), Wproj=g["Wp"], bproj=g["bp"], Y32=o[0][1], Yact=o[1][1],
                        gamma=g["gamma"], beta=g["beta"], mod=g["mod"]) for g, o in zip(groups, outs)])
    got = launched(ops, "mlp_block.rows32")
    assert got[1:] == _per_xcd(Ms), got
    if Ms == MLP_ROUNDS_MS:
        assert got[1] > 0, got
    for i, (g, ref, ((big32, Y32), (bigact, Yact))) in enumerate(zip(groups, refs, outs)):
        what = f"mlp_block {case} group {i} ({g['pro']}, {g['norm']})"
        check("blk.Y32", Y32, ref["blk.Y32"], what)
        check("blk.Yact", Yact, ref["blk.Yact"], what)
        assert frame_untouched(big32, E) and frame_untouched(bigact, E), what


# ------------------------------------------------------------------------------------------------ sea_gemm_adaln
ADALN_MS = (63, 64, 65)
ADALN_CASES = [(64, 128), (64, 72), (200, 400), (256, 512)]   # (d, K): d = 200 a ragged last column tile under a statistic that spans column tiles; K != 2 d once
# the smallest group set the launcher's own rule (t128 >= 512) sends to 128-row tiles: 16 groups (SEA_MAX_ADALN_GROUPS) of 16 column tiles (d = 1024, or 2 d = 2048
# for a plain group) need two row tiles each — M = 129, the last row tile one row high
ADALN_128 = dict(d=1024, K=64, M=129, n=16)


def adaln_group(M, d, K, plain, seed, extra, device=None):
    kw = dict(device=device)
    g = dict(M=M, d=d, K=K, plain=plain, A=tall(rnd(M, K, dtype=BF, scale=0.5, seed=seed + 1, **kw), extra), W=rnd(2 * d, K, dtype=BF, scale=K ** -0.5, seed=seed + 2, **kw),
             bias=0.3 * rnd(2 * d, seed=seed + 3, **kw))
    if not plain:
        g.update(X=tall_cols(rnd(M, 3 * d, seed=seed + 4, **kw) * 1.3 + 0.2, extra, d, 2 * d), gamma=1 + 0.1 * rnd(d, seed=seed + 5, **kw), beta=0.1 * rnd(d, seed=seed + 6, **kw))
    return g


def adaln_formula(g, rt=None):
    """Rounded where the kernel rounds: the act outputs alone (the modulation stays in fp32 registers)."""
    r = rounder(rt)
    mod = g["A"].double() @ g["W"].double().t() + g["bias"].double()
    if g["plain"]:
        return {"adaln.mod": r(mod)}
    xh, mean, rstd = ln64(g["X"].double())
    y = modulate(xh, g["gamma"], g["beta"], mod)
    return {"Y32": y, "adaln.Yact": r(y), "mean": mean, "rstd": rstd}


def adaln_groups(d, K, device=None):
    """A normalising and a plain group per row count, in one launch."""
    return [adaln_group(M, d, K, plain, 7600 + 10 * i + d + K + 100 * plain, 64, device) for i, M in enumerate(ADALN_MS) for plain in (0, 1)]


def adaln_groups_128(device=None):
    c = ADALN_128
    return [adaln_group(c["M"], c["d"], c["K"], i % 2, 7700 + 10 * i, 128, device) for i in range(c["n"])]


def _adaln_run(groups, form, tiles, what):
    from sea_amd import ops

    launch, outs = [], []
    for g in groups:
        M, d = g["M"], g["d"]
        if g["plain"]:
            o = dict(Yact=out2d(M, 2 * d, BF))
            launch.append(dict(A=g["A"], W=g["W"], bias=g["bias"], Yact=o["Yact"][1]))
        else:
            o = dict(Yact=out2d(M, d, BF), Y32=out2d(M, d, torch.float32), mean=guarded((M,), torch.float32), rstd=guarded((M,), torch.float32))
            launch.append(dict(A=g["A"], W=g["W"], bias=g["bias"], X=g["X"], gamma=g["gamma"], beta=g["beta"], Yact=o["Yact"][1], Y32=o["Y32"][1], mean=o["mean"][1],
                               rstd=o["rstd"][1]))
        outs.append(o)
    ops.gemm_adaln(launch)
    got = launched(ops, form)
    assert got[1] == tiles, (what, got)
    for i, (g, o) in enumerate(zip(groups, outs)):
        ref, w = adaln_formula(g), f"{what} group {i} M={g['M']}"
        if g["plain"]:
            check("adaln.mod", o["Yact"][1], ref["adaln.mod"], w)
            assert frame_untouched(o["Yact"][0], 2 * g["d"]), w
            continue
        check("adaln.Yact", o["Yact"][1], ref["adaln.Yact"], w)
        check("adaln.Y32", o["Y32"][1], ref["Y32"], w, f32=True)
        check("adaln.mean", o["mean"][1], ref["mean"], w, f32=True, g32=1e-5)
        check("adaln.rstd", o["rstd"][1], ref["rstd"], w, f32=True, g32=1e-5)
        assert frame_untouched(o["Yact"][0], g["d"]) and frame_untouched(o["Y32"][0], g["d"]) and guard_untouched(o["mean"][0]) and guard_untouched(o["rstd"][0]), w


@pytest.mark.parametrize("d,K", ADALN_CASES)
def test_gemm_adaln_rows64(d, K):
    tiles = sum((M + 63) // 64 * ((d + 63) // 64 + (2 * d + 127) // 128) for M in ADALN_MS)
    _adaln_run(adaln_groups(d, K), "gemm_adaln.rows64", tiles, f"gemm_adaln d={d} K={K}")


def test_gemm_adaln_rows128_by_the_launchers_rule():
    _adaln_run(adaln_groups_128(), "gemm_adaln.rows128", 512, "gemm_adaln 128-row tiles")


# ------------------------------------------------------------------------------------------------ the exchange tail and the row chain
TAIL_MS = (15, 16, 17)
TAIL_CASES = [(128, 256, 1), (128, 256, 2), (64, 128, 4)]   # (D, E, segments)
CHAIN_BT = [(1, 15), (1, 16), (1, 17), (3, 11), (2, 17)]   # the last two: tiles that straddle trajectories, a ragged last tile
CHAIN_POS0 = (0, 3)
CHAIN_CASES = [(D, E, hd, form) for D, E in ((128, 256), (64, 128)) for hd in (16, 32) for form in "AB"]


def tail_operands(D, E, M, S, form, seed, extra, device=None):
    """The operands of sea_exchange_tail / sea_row_chain for one group: form B (S segments) or form A (a2), the down-projection and its AdaLN."""
    kw = dict(device=device)
    g = dict(D=D, E=E, M=M, S=S, form=form, Wd=rnd(D, E, dtype=BF, scale=0.1, seed=seed + 1, **kw), bd=0.2 * rnd(D, seed=seed + 2, **kw),
             xin=tall_cols(rnd(M, 3 * E, seed=seed + 3, **kw), extra, E, 2 * E), mod=tall(rnd(M, 2 * D, dtype=BF, scale=0.5, seed=seed + 4, **kw), extra),
             gamma=1 + 0.1 * rnd(D, seed=seed + 5, **kw), beta=0.1 * rnd(D, seed=seed + 6, **kw), b2=0.2 * rnd(E, seed=seed + 7, **kw))
    if form == "B":
        g.update(att=[tall(rnd(M, D, dtype=BF, seed=seed + 10 + s, **kw), extra) for s in range(S)], Wp=[rnd(D, D, dtype=BF, scale=0.15, seed=seed + 20 + s, **kw) for s in range(S)],
                 W2=rnd(E, D, dtype=BF, scale=0.1, seed=seed + 8, **kw), bias_scale=float(S))
    else:
        g.update(a2=tall(rnd(M, E, dtype=BF, seed=seed + 9, **kw), extra), W2=rnd(E, E, dtype=BF, scale=0.1, seed=seed + 8, **kw), bias_scale=1.0, att=[], Wp=[])
    return g


def tail_formula(g, rt=None):
    """x, Xact, the normalised rows y, mean, rstd.  Rounded where the kernels round: the SUM of the GELU outputs g (operand of the up-projection), x as the operand
    of the down-projection; the act outputs."""
    r = rounder(rt)
    if g["form"] == "B":
        gs = r(sum(gelu64(a.double() @ w.double().t()) for a, w in zip(g["att"], g["Wp"])))
        x = g["xin"].double() + gs @ g["W2"].double().t() + g["bias_scale"] * g["b2"].double()
    else:
        x = g["xin"].double() + g["a2"].double() @ g["W2"].double().t() + g["b2"].double()
    xh, mean, rstd = ln64(r(x) @ g["Wd"].double().t() + g["bd"].double())
    y = modulate(xh, g["gamma"], g["beta"], g["mod"])
    return {"X": x, "Xact": r(x), "Y32": y, "Yact": r(y), "mean": mean, "rstd": rstd}


def tail_groups(D, E, S, device=None):
    return [tail_operands(D, E, M, S, "B", 7800 + 100 * i + D + S, 16, device) for i, M in enumerate(TAIL_MS)]


@pytest.mark.parametrize("has_down", [True, False])
@pytest.mark.parametrize("D,E,S", TAIL_CASES)
def test_exchange_tail_rows(D, E, S, has_down):
    from sea_amd import ops

    groups = tail_groups(D, E, S)
    launch, outs = [], []
    for g in groups:
        M = g["M"]
        o = dict(X=out2d(M, E, torch.float32), Xact=out2d(M, E, BF))
        o["X"][1].copy_(g["xin"])   # updated in place
        d = dict(att=g["att"], Wp=g["Wp"], Wup=g["W2"], bup=g["b2"], bias_scale=g["bias_scale"], X=o["X"][1], Xact=o["Xact"][1])
        if has_down:
            o.update(Yact=out2d(M, D, BF), Y32=out2d(M, D, torch.float32), mean=guarded((M,), torch.float32), rstd=guarded((M,), torch.float32))
            d["down"] = dict(W=g["Wd"], bias=g["bd"], gamma=g["gamma"], beta=g["beta"], mod=g["mod"], Yact=o["Yact"][1], Y32=o["Y32"][1], mean=o["mean"][1], rstd=o["rstd"][1])
        launch.append(d)
        outs.append(o)
    ops.exchange_tail_grouped(launch)
    got = launched(ops, "xtail.rows16")
    assert got[1:] == (2, S), got
    for i, (g, o) in enumerate(zip(groups, outs)):
        ref, what = tail_formula(g), f"exchange_tail D={D} S={S} down={has_down} group {i} M={g['M']}"
        for k in ("X", "Xact") + (("Y32", "Yact", "mean", "rstd") if has_down else ()):
            check("tail." + k, o[k][1], ref[k], what)
            assert guard_untouched(o[k][0]) if k in ("mean", "rstd") else frame_untouched(o[k][0], o[k][1].shape[1]), (what, k)


def chain_operands(D, E, hd, B, T, pos0, form, device=None):
    """tail_operands plus two q and two k | v projections of the normalised rows, the rotary table and the cache geometry."""
    kw = dict(device=device)
    seed = 7900 + D + 7 * hd + 100 * B + 13 * T + 1000 * pos0
    g = tail_operands(D, E, B * T, 2, form, seed, 32, device)
    g.update(B=B, T=T, H=D // hd, hd=hd, pos0=pos0, cap=(pos0 + T) // 8 * 8 + 8, table=rope_table(hd, pos0 + T, device=device if device is not None else dev()),
             Wq=[rnd(D, D, dtype=BF, scale=D ** -0.5, seed=seed + 30 + k, **kw) for k in range(2)], bq=[rnd(D, seed=seed + 34 + k, **kw) for k in range(2)],
             Wkv=[rnd(2 * D, D, dtype=BF, scale=D ** -0.5, seed=seed + 40 + k, **kw) for k in range(2)], bkv=[rnd(2 * D, seed=seed + 44 + k, **kw) for k in range(2)])
    return g


def chain_formula(g, rt=None):
    """tail_formula and, from the normalised rows rounded as the projections' operand, Q / K / V [B, H, T, hd] (rotary embedding on q and k, the q scale)."""
    from sea_amd.ops import q_scale

    r = rounder(rt)
    out = tail_formula(g, rt)
    B, T, H, hd, D = g["B"], g["T"], g["H"], g["hd"], g["D"]
    y = r(out["Y32"])
    for k in range(2):
        q = (y @ g["Wq"][k].double().t() + g["bq"][k].double()).reshape(B, T, H, hd)
        kv = y @ g["Wkv"][k].double().t() + g["bkv"][k].double()
        out[f"Q{k}"] = r(rope64(q, g["table"], g["pos0"]) * q_scale(hd)).permute(0, 2, 1, 3)
        out[f"K{k}"] = r(rope64(kv[:, :D].reshape(B, T, H, hd), g["table"], g["pos0"])).permute(0, 2, 1, 3)
        out[f"V{k}"] = r(kv[:, D:]).reshape(B, T, H, hd).permute(0, 2, 1, 3)
    return out


def chain_form(rows, hd):
    """The form sea_row_chain notes: 32-row workgroups hold the rotary rows of head dim 16 only — at head dim 32 the launcher falls back to 16-row workgroups."""
    return "chain.rows32" if rows == 32 and hd == 16 else "chain.rows16"


def chain_launch_groups(g):
    """The three group kinds (everything / no projections / no down-projection) on the operands g, every output NaN: (launch dicts, outputs)."""
    M, D, E, B, T, H, hd, cap = (g[k] for k in ("M", "D", "E", "B", "T", "H", "hd", "cap"))
    o = dict(X=out2d(M, E, torch.float32), Xact=out2d(M, E, BF), Yact=out2d(M, D, BF), Y32=out2d(M, D, torch.float32), mean=guarded((M,), torch.float32),
             rstd=guarded((M,), torch.float32), X_b=out2d(M, E, torch.float32), Yact_b=out2d(M, D, BF), X_c=out2d(M, E, torch.float32))
    for k in range(2):
        o[f"Q{k}"], o[f"K{k}"], o[f"Vt{k}"], o[f"V{k}"] = guarded((B, H, T, hd), BF), guarded((B, H, cap, hd), BF), guarded((B, H, hd, cap), BF), guarded((B, H, cap, hd), BF)
    proj = []
    for k in range(2):
        proj += [dict(W=g["Wq"][k], bias=g["bq"][k], col0=0, Q=o[f"Q{k}"][1]), dict(W=g["Wkv"][k], bias=g["bkv"][k], col0=D, K=o[f"K{k}"][1], Vt=o[f"Vt{k}"][1], V=o[f"V{k}"][1])]
    common = dict(W2=g["W2"], b2=g["b2"], bias_scale=g["bias_scale"], Xin=g["xin"], att=g["att"], Wp=g["Wp"], a2=g.get("a2"))
    down = dict(W=g["Wd"], bias=g["bd"], gamma=g["gamma"], beta=g["beta"], mod=g["mod"])
    launch = [dict(common, X=o["X"][1], Xact=o["Xact"][1], down=dict(down, Yact=o["Yact"][1], Y32=o["Y32"][1], mean=o["mean"][1], rstd=o["rstd"][1]), proj=proj),
              dict(common, X=o["X_b"][1], down=dict(down, Yact=o["Yact_b"][1])), dict(common, X=o["X_c"][1])]
    return launch, o


def chain_check(g, ref, o, what):
    B, T, H, hd, pos0 = (g[k] for k in ("B", "T", "H", "hd", "pos0"))
    for k in ("X", "X_b", "X_c"):
        if g["form"] == "A":
            check("chain.X(A)", o[k][1], ref["X"], what, f32=True)   # nothing rounded upstream
        else:
            check("chain.X", o[k][1], ref["X"], what)
    check("chain.Xact", o["Xact"][1], ref["Xact"], what)
    check("chain.Yact", o["Yact"][1], ref["Yact"], what)
    check("chain.Yact", o["Yact_b"][1], ref["Yact"], what)
    for k in ("Y32", "mean", "rstd"):
        check("chain." + k, o[k][1], ref[k], what)
    for k in ("X", "Xact", "Yact", "Y32", "X_b", "Yact_b", "X_c"):
        assert frame_untouched(o[k][0], o[k][1].shape[1]), (what, k)
    for k in range(2):
        check("chain.Q", o[f"Q{k}"][1], ref[f"Q{k}"], what, row=hd)
        cache_window("chain.K", o[f"K{k}"][1], ref[f"K{k}"], pos0, T, hd, what)
        cache_window("chain.V", o[f"Vt{k}"][1], ref[f"V{k}"], pos0, T, hd, what, transposed=True)
        cache_window("chain.V", o[f"V{k}"][1], ref[f"V{k}"], pos0, T, hd, what)
    for k, v in o.items():
        if v[0].dim() == 1:
            assert guard_untouched(v[0]), (what, k)


def chain_run(monkeypatch, g, rows, **riders):
    from sea_amd import ops

    launch, o = chain_launch_groups(g)
    force(monkeypatch, f"chain_rows={rows}")
    ops.row_chain(launch, rope=g["table"], H=g["H"], hd=g["hd"], T=g["T"], pos0=g["pos0"], cap=g["cap"], q_scale_=ops.q_scale(g["hd"]), **riders)
    return launched(ops, chain_form(rows, g["hd"])), o


@pytest.mark.parametrize("D,E,hd,form", CHAIN_CASES)
def test_row_chain_rows(monkeypatch, D, E, hd, form):
    from sea_amd import ops

    assert ops.row_chain_supported(BF, D, E, 2 if form == "B" else 0, hd)
    for B, T in CHAIN_BT:
        for pos0 in CHAIN_POS0:
            g = chain_operands(D, E, hd, B, T, pos0, form)
            ref = chain_formula(g)
            for rows in (16, 32):
                got, o = chain_run(monkeypatch, g, rows)
                assert got[1:] == (0, 0), got
                chain_check(g, ref, o, f"row_chain D={D} hd={hd} form {form} B={B} T={T} pos0={pos0} rows={rows} -> {got[0]}")


# ------------------------------------------------------------------------------------------------ sea_row_chain_riders
RIDER = dict(M=203, Ns=(256, 512), K=512, split=6)   # 2 x 2 + 2 x 4 = 12 tiles of 128 x 128, numbered across both groups; the split falls inside the second group
RIDER_CHAIN = (128, 256, 16, 2, 17, 3, "B")          # the chain the riders travel with
IB_CASES = [(63, 256, 8), (65, 128, 4)]              # (rows, E, h): 64 rows per info-bottleneck workgroup


def rider_operands(M=None, device=None):
    c = RIDER
    M = c["M"] if M is None else M
    return [dict(A=tall(rnd(M, c["K"], dtype=BF, seed=8100 + i, device=device), 128), W=rnd(N_, c["K"], dtype=BF, scale=c["K"] ** -0.5, seed=8110 + i, device=device),
                 bias=(rnd(N_, seed=8120 + i, device=device) if i == 0 else None)) for i, N_ in enumerate(c["Ns"])]


def rider_formula(g, rt=None):
    """Rounded where the kernel rounds: the stored output."""
    v = g["A"].double() @ g["W"].double().t()
    return rounder(rt)(v + g["bias"].double() if g["bias"] is not None else v)


def ib_operands(M, E, h, device=None):
    kw = dict(device=device)
    return dict(M=M, E=E, h=h, c=tall(torch.rand(M, generator=torch.Generator().manual_seed(8200 + M)).to(device if device is not None else dev()), 64),
                w1=rnd(h, seed=8201 + M, **kw), b1=rnd(h, seed=8202 + M, **kw), lnw=1 + 0.1 * rnd(h, seed=8203 + M, **kw), lnb=0.1 * rnd(h, seed=8204 + M, **kw),
                w2=rnd(E, h, scale=0.3, seed=8205 + M, **kw), b2=0.1 * rnd(E, seed=8206 + M, **kw))


def ib_formula(g):
    """sea_silu_outer_ib: W2 . gelu(LN_h(w1 c + b1)) + b2, fp32 throughout."""
    pre = g["c"].double()[:, None] * g["w1"].double() + g["b1"].double()
    return gelu64(ln64(pre)[0] * g["lnw"].double() + g["lnb"].double()) @ g["w2"].double().t() + g["b2"].double()


def _same_outputs(o1, o2):
    return all(torch.equal(o1[k][0].nan_to_num(12345.0), o2[k][0].nan_to_num(12345.0)) for k in o1)


def test_row_chain_riders_split_over_two_launches(monkeypatch):
    """Two rider GEMMs cut into 12 tiles over the launches [0, 6) and [6, 12): after the first every tile from 6 on is wholly NaN, after the second everything meets
    the fp64 product; the chain's own outputs of both launches are bit for bit those of a launch without riders."""
    c = RIDER
    g = chain_operands(*RIDER_CHAIN)
    ref = chain_formula(g)
    _, plain = chain_run(monkeypatch, g, 16)
    riders = rider_operands()
    Cs = [out2d(c["M"], N_, BF) for N_ in c["Ns"]]
    rd = [dict(A=r["A"], W=r["W"], bias=r["bias"], Cact=C_[1]) for r, C_ in zip(riders, Cs)]
    k = c["split"]
    got, o1 = chain_run(monkeypatch, g, 16, riders=rd, tile0=0, n_tiles=k)
    assert got[1:] == (k, 0), got
    assert torch.isfinite(Cs[0][1].float()).all()                       # tiles 0 .. 3: the whole first group
    assert torch.isfinite(Cs[1][1][:128, :256].float()).all()           # tiles 4, 5: row tile 0, column tiles 0 and 1 of the second
    assert bool(torch.isnan(Cs[1][1][:128, 256:].float()).all()) and bool(torch.isnan(Cs[1][1][128:].float()).all())
    got, o2 = chain_run(monkeypatch, g, 16, riders=rd, tile0=k, n_tiles=12 - k)
    assert got[1:] == (12 - k, 0), got
    for i, (r, C_) in enumerate(zip(riders, Cs)):
        check("rider.C", C_[1], rider_formula(r), f"chain rider group {i}")
        assert frame_untouched(C_[0], c["Ns"][i]), i
    chain_check(g, ref, o2, "row_chain with riders")
    assert _same_outputs(plain, o1) and _same_outputs(plain, o2)


@pytest.mark.parametrize("M,E,h", IB_CASES)
def test_row_chain_ib_rider(monkeypatch, M, E, h):
    g = chain_operands(*RIDER_CHAIN)
    ib = ib_operands(M, E, h)
    big, X = out2d(M, E, torch.float32)
    _, plain = chain_run(monkeypatch, g, 16)
    got, o = chain_run(monkeypatch, g, 16, ib=dict(xs=[X], c=ib["c"], w1=ib["w1"], b1=ib["b1"], lnw=ib["lnw"], lnb=ib["lnb"], w2=ib["w2"], b2=ib["b2"]))
    assert got[1:] == (0, (M + 63) // 64), got
    check("ib.X", X, ib_formula(ib), f"chain ib rider M={M} E={E} h={h}", f32=True)
    assert frame_untouched(big, E)
    assert _same_outputs(plain, o)


# ------------------------------------------------------------------------------------------------ sea_adaln_qkv
AQKV_E = 256
AQKV_BT = [(1, 31), (1, 32), (1, 33), (3, 11)]
AQKV_POS0 = (0, 3)
AQKV_SILU_M = {0: 63, 3: 65}   # rows of the row riders (64 per workgroup), by pos0


def aqkv_operands(H, B, T, pos0, third, field=0, device=None):
    kw = dict(device=device)
    E, M = AQKV_E, B * T
    hd = E // H
    seed = 8300 + H + 100 * B + 13 * T + 1000 * pos0 + 50 * field
    dv = device if device is not None else dev()
    g = dict(E=E, M=M, B=B, T=T, H=H, hd=hd, pos0=pos0, cap=(pos0 + T) // 8 * 8 + 8, table=rope_table(hd, pos0 + T, device=dv), third=third,
             cond=tall(torch.rand(M, generator=torch.Generator().manual_seed(seed)).to(dv), 32), X=tall_cols(rnd(M, 3 * E, seed=seed + 1, **kw) * 1.3 + 0.2, 32, E, 2 * E),
             w1=rnd(2 * E, seed=seed + 2, **kw), b1=rnd(2 * E, seed=seed + 3, **kw), W2c=rnd(2 * E, 2 * E, dtype=BF, scale=(2 * E) ** -0.5, seed=seed + 4, **kw),
             b2c=0.3 * rnd(2 * E, seed=seed + 5, **kw), gamma=1 + 0.1 * rnd(E, seed=seed + 6, **kw), beta=0.1 * rnd(E, seed=seed + 7, **kw),
             Wqkv=rnd(3 * E, E, dtype=BF, scale=E ** -0.5, seed=seed + 8, **kw), bqkv=rnd(3 * E, seed=seed + 9, **kw))
    if third:
        g.update(w13=rnd(256, seed=seed + 10, **kw), b13=rnd(256, seed=seed + 11, **kw), W3=rnd(256, 256, dtype=BF, scale=1 / 16, seed=seed + 12, **kw), b3=0.3 * rnd(256, seed=seed + 13, **kw))
    return g


def silu64(x):
    return x / (1 + torch.exp(-x))


def aqkv_formula(g, rt=None):
    """Rounded where the kernel rounds: the generated hidden rows, the modulation (bf16 in LDS), the normalised rows, the outputs; the third layer's hidden rows."""
    from sea_amd.ops import q_scale

    r = rounder(rt)
    E, B, T, H, hd = g["E"], g["B"], g["T"], g["H"], g["hd"]
    c = g["cond"].double()[:, None]
    mod = r(r(silu64(c * g["w1"].double() + g["b1"].double())) @ g["W2c"].double().t() + g["b2c"].double())
    y = r(modulate(ln64(g["X"].double())[0], g["gamma"], g["beta"], mod))
    qkv = y @ g["Wqkv"].double().t() + g["bqkv"].double()
    q, k, v = (qkv[:, j * E:(j + 1) * E].reshape(B, T, H, hd) for j in range(3))
    out = {"Q": r(rope64(q, g["table"], g["pos0"]) * q_scale(hd)).permute(0, 2, 1, 3), "K": r(rope64(k, g["table"], g["pos0"])).permute(0, 2, 1, 3), "V": r(v).permute(0, 2, 1, 3)}
    if g["third"]:
        out["mod3"] = r(r(silu64(c * g["w13"].double() + g["b13"].double())) @ g["W3"].double().t() + g["b3"].double())
    return out


def silu_operands(Ms, device=None):
    kw = dict(device=device)
    return dict(c=tall(torch.rand(Ms, generator=torch.Generator().manual_seed(8400 + Ms)).to(device if device is not None else dev()), 64),
                groups=[(rnd(512, seed=8410 + Ms + k, **kw), rnd(512, seed=8420 + Ms + k, **kw)) for k in range(2)])


def silu_formula(c, w1, b1, rt=None):
    return rounder(rt)(silu64(c.double()[:, None] * w1.double() + b1.double()))


@pytest.mark.parametrize("third", [False, True])
@pytest.mark.parametrize("H", [8, 16])
def test_adaln_qkv_rows(H, third):
    """Two fields per launch at every (B, T) and pos0, with two GEMM riders, two silu row riders and the information-bottleneck row rider."""
    from sea_amd import ops

    E = AQKV_E
    hd = E // H
    for B, T in AQKV_BT:
        for pos0 in AQKV_POS0:
            fields = [aqkv_operands(H, B, T, pos0, third, field=f) for f in range(2)]   # the second field's first tile follows the ragged last tile of the first
            M, cap, Ms = fields[0]["M"], fields[0]["cap"], AQKV_SILU_M[pos0]
            refs, outs, launch = [], [], []
            for g in fields:
                refs.append(aqkv_formula(g))
                o = dict(Q=guarded((B, H, T, hd), BF), K=guarded((B, H, cap, hd), BF), Vt=guarded((B, H, hd, cap), BF))
                d = dict(X=g["X"], cond=g["cond"], w1=g["w1"], b1=g["b1"], W2c=g["W2c"], b2c=g["b2c"], gamma=g["gamma"], beta=g["beta"], Wqkv=g["Wqkv"], bqkv=g["bqkv"],
                         Q=o["Q"][1], K=o["K"][1], Vt=o["Vt"][1])
                if third:
                    o["mod3"] = out2d(M, 256, BF)
                    d["third"] = dict(w1=g["w13"], b1=g["b13"], W=g["W3"], bias=g["b3"], out=o["mod3"][1])
                outs.append(o)
                launch.append(d)
            su = silu_operands(Ms)
            hid = [out2d(Ms, 512, BF) for _ in su["groups"]]
            ib = ib_operands(Ms, 256, 8)
            ib["c"] = su["c"]   # the information-bottleneck rows are evaluated on silu_c
            ibig, iX = out2d(Ms, 256, torch.float32)
            riders = rider_operands(Ms)
            Cs = [out2d(Ms, N_, BF) for N_ in RIDER["Ns"]]
            ops.adaln_qkv(launch, fields[0]["table"], H, hd, T, pos0, cap, ops.q_scale(hd), riders=[dict(A=r["A"], W=r["W"], bias=r["bias"], Cact=C_[1]) for r, C_ in zip(riders, Cs)],
                          silu=[dict(w1=w_, b1=b_, Hid=h_[1]) for (w_, b_), h_ in zip(su["groups"], hid)], silu_c=su["c"],
                          ib=dict(xs=[iX], c=None, w1=ib["w1"], b1=ib["b1"], lnw=ib["lnw"], lnb=ib["lnb"], w2=ib["w2"], b2=ib["b2"]))
            got = launched(ops, "adaln_qkv.rows32_mod3" if third else "adaln_qkv.rows32")
            n_rt = (Ms + 127) // 128
            assert got[1:] == (n_rt * 2 + n_rt * 4, 2 * ((Ms + 63) // 64) + (Ms + 63) // 64), got
            what = f"adaln_qkv H={H} B={B} T={T} pos0={pos0} third={third}"
            for f, (ref, o) in enumerate(zip(refs, outs)):
                w = what + f" field {f}"
                check("aqkv.Q", o["Q"][1], ref["Q"], w, row=hd)
                cache_window("aqkv.K", o["K"][1], ref["K"], pos0, T, hd, w)
                cache_window("aqkv.V", o["Vt"][1], ref["V"], pos0, T, hd, w, transposed=True)
                for k in ("Q", "K", "Vt"):
                    assert guard_untouched(o[k][0]), (w, k)
                if third:
                    check("aqkv.mod3", o["mod3"][1], ref["mod3"], w)
                    assert frame_untouched(o["mod3"][0], 256), w
            for (w_, b_), h_ in zip(su["groups"], hid):
                check("aqkv.Hid", h_[1], silu_formula(su["c"], w_, b_), what)
                assert frame_untouched(h_[0], 512), what
            check("ib.X", iX, ib_formula(ib), what, f32=True)
            assert frame_untouched(ibig, 256), what
            for i, (r, C_) in enumerate(zip(riders, Cs)):
                check("rider.C", C_[1], rider_formula(r), what + f" rider {i}")
                assert frame_untouched(C_[0], RIDER["Ns"][i]), what


# ------------------------------------------------------------------------------------------------ the emulation behind LOCAL, on the CPU
def emulation_cases(device="cpu"):
    """Yields (what, {kind: (reference, emulation, exact, row length or None)}) for every case the tests of this file launch."""
    def three(formula, g, keys, **kw):
        ref, emu, exact = formula(g), formula(g, BF), formula(g, None)
        return {k2: (ref[k1], emu[k1], exact[k1], kw.get("row")) for k1, k2 in keys}

    for case in mlp_cases():
        for i, g in enumerate(mlp_groups(*case, device=device)):
            yield f"mlp {case} group {i} ({g['pro']}, {g['norm']})", three(mlp_formula, g, [(k, k) for k in LOCAL if k[:3] in ("fc1", "fc2", "blk")])
    for d, K in ADALN_CASES:
        for i, g in enumerate(adaln_groups(d, K, device)):
            yield f"gemm_adaln d={d} K={K} group {i} M={g['M']}", three(adaln_formula, g, [("adaln.mod", "adaln.mod")] if g["plain"] else [("adaln.Yact", "adaln.Yact")])
    for i, g in enumerate(adaln_groups_128(device)):
        yield f"gemm_adaln 128-row tiles group {i}", three(adaln_formula, g, [("adaln.mod", "adaln.mod")] if g["plain"] else [("adaln.Yact", "adaln.Yact")])
    for D, E, S in TAIL_CASES:
        for i, g in enumerate(tail_groups(D, E, S, device)):
            yield f"exchange_tail D={D} S={S} group {i} M={g['M']}", three(tail_formula, g, [(k, "tail." + k) for k in ("X", "Xact", "Y32", "Yact", "mean", "rstd")])
    for D, E, hd, form in CHAIN_CASES:
        for B, T in CHAIN_BT:
            for pos0 in CHAIN_POS0:
                g = chain_operands(D, E, hd, B, T, pos0, form, device)
                ref, emu, exact = chain_formula(g), chain_formula(g, BF), chain_formula(g, None)
                out = {"chain." + k: (ref[k], emu[k], exact[k], None) for k in (("X",) if form == "B" else ()) + ("Xact", "Y32", "Yact", "mean", "rstd")}
                for k in range(2):
                    for n in "QKV":
                        out[f"chain.{n}#{k}"] = (ref[f"{n}{k}"], emu[f"{n}{k}"], exact[f"{n}{k}"], hd)
                yield f"row_chain D={D} hd={hd} form {form} B={B} T={T} pos0={pos0}", out
    for i, g in enumerate(rider_operands(device=device)):
        yield f"chain rider group {i}", {"rider.C": (rider_formula(g), rider_formula(g, BF), rider_formula(g, None), None)}
    for H in (8, 16):
        for third in (False, True):
            for B, T in AQKV_BT:
                for pos0 in AQKV_POS0:
                    for f in range(2):
                        g = aqkv_operands(H, B, T, pos0, third, f, device)
                        ref, emu, exact = aqkv_formula(g), aqkv_formula(g, BF), aqkv_formula(g, None)
                        out = {"aqkv." + n: (ref[n], emu[n], exact[n], g["hd"]) for n in "QKV"}
                        if third:
                            out["aqkv.mod3"] = (ref["mod3"], emu["mod3"], exact["mod3"], None)
                        yield f"adaln_qkv H={H} B={B} T={T} pos0={pos0} third={third} field {f}", out
    for Ms in sorted(set(AQKV_SILU_M.values())):
        su = silu_operands(Ms, device)
        for k, (w_, b_) in enumerate(su["groups"]):
            yield f"adaln_qkv silu rider rows={Ms} group {k}", {"aqkv.Hid": (silu_formula(su["c"], w_, b_), silu_formula(su["c"], w_, b_, BF), silu_formula(su["c"], w_, b_, None), None)}
        for i, r in enumerate(rider_operands(Ms, device)):
            yield f"adaln_qkv rider rows={Ms} group {i}", {"rider.C": (rider_formula(r), rider_formula(r, BF), rider_formula(r, None), None)}


def measure_local(device="cpu", verbose=True):
    """{kind: (largest rowerr(emulation, reference), its case)}; asserts that the emulation without rounding restates the reference to 1e-12."""
    worst = {k: (0.0, "") for k in LOCAL}
    for what, outs in emulation_cases(device):
        line = []
        for key, (ref, emu, exact, row) in outs.items():
            kind = key.split("#")[0]
            assert float((exact - ref).norm()) <= 1e-12 * max(float(ref.norm()), 1.0), (what, key)
            e = rowerr(emu.reshape(-1, row), ref.reshape(-1, row)) if row else rowerr(emu, ref)
            line.append(f"{key} local {e:.3e} (global {rel(emu, ref):.3e})")
            if e > worst[kind][0]:
                worst[kind] = (e, what)
        if verbose:
            print(f"{what}: " + "  ".join(line))
    return worst


if __name__ == "__main__":
    for kind, (v, what) in measure_local().items():
        print(f"{kind}: measured {v:.3e} at {what}; LOCAL = 3 * {LOCAL[kind] / 3:.3e}")
