"""The CRPS of the decoded fields as a loss on the clock (Decode.member_crps_loss, sea_decode_member_crps_grad): loss + backward, fused against composed.

  ms per call at the two decoder sizes of tools/decode_loss_bench.py (cylinder: hidden 480, D 16; multiphase: hidden 624, D 32; P = 64 patches, fields
  [[0, 1], [2]], the same synthetic wake-refined mesh with its counts, n_inp 1628), bf16, in two regimes:
    DA        64 and 128 members x 64 patches, 1 and 4 histories (tools/field_verify_bench.py's shapes)
    training  4 and 8 members, 64 and 256 histories (a batch of (trajectory, step) pairs of an ensemble-trained temporal model), and 2, 16 and 32
              members x 64 histories
  and per row:
    grad fused      Decode.member_crps_loss(fused=True, pack=False), loss.sum().backward(): first layer (pre-activation kept), the two launches of
                    sea_decode_member_crps_grad, the data-gradient launch against W1^T
    grad pack       the same with pack=True (up to 32 members): sea_decode_member_crps_grad_packed, several histories per workgroup — measured in the same
                    windows as grad fused, the forms alternating; `bits` says whether its loss and z.grad are grad fused's, bit for bit
    grad composed   Decode.member_crps_loss(fused=False), loss.sum().backward(): forward() under autograd plus the fp64 formulas as torch ops
    score fused     Decode.member_verify(fused=True, maps=()) under no_grad: the score-only launches the gradient form is built on (must not move)
  beside each the peak of allocated memory above its value before the call and the number of device launches of one call as the profiler counts them.
  A shape the fused gradient form refuses (above 64 members at a hidden width above 384) is listed as refused.  Device time: windows of back-to-back
  calls between two events, at least 20 ms each, the forms alternating inside every repeat (tools/ensemble_bench.device_ms): the median of the windows.
  Decode.member_crps_loss's fused=None rule and its pack=None rule (crps_loss_pack_rule) are read from these rows.

    python tools/crps_loss_bench.py [--reps 5] [--regimes da,training] [--out profiles/crps_pack_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.decode_loss_bench import SIZES, mesh  # noqa: E402
from tools.ensemble_bench import device_ms, extra_bytes  # noqa: E402
from tools.sensor_bench import count_launches  # noqa: E402

REGIMES = {"da": [(64, 1), (64, 4), (128, 1), (128, 4)], "training": [(4, 64), (8, 64), (4, 256), (8, 256), (2, 64), (16, 64), (32, 64)]}   # (members, histories)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="cylinder,multiphase")
    ap.add_argument("--regimes", default="da,training")
    ap.add_argument("--max-composed-rows", type=int, default=1 << 30, help="skip the composed path above this many decoder rows (its fp64 tensors)")
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("crps_loss_bench.py needs an MI355X: no GPU visible")
    from sea_amd import ops
    from sea_amd.models.encoder_decoder import Decode

    dev = torch.device("cuda", 0)
    groups, P, F = [[0, 1], [2]], 64, 3
    n_inp, mesh_counts = mesh(dev)
    lines, recs = [], []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out:
            with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"crps_loss_bench: Decode.member_crps_loss, loss.sum().backward(), P = {P}, fields {groups}, n_inp = {n_inp}, the mesh's counts, bf16, device time in ms, "
         f"median of {args.reps} windows (lo-hi: the windows' range); MB: peak of allocated memory above its value before the call; n: device launches of one call")
    emit(f"{'regime':<9}{'size':<11}{'members':>8}{'B':>5}{'rows':>8}{'grad fused':>12}{'lo-hi':>16}{'grad comp':>11}{'lo-hi':>16}{'comp/fused':>11}{'grad pack':>11}{'lo-hi':>16}{'fused/pack':>11}{'bits':>6}{'score fused':>12}{'lo-hi':>16}"
         f"{'MB fused':>10}{'MB comp':>10}{'n fused':>8}{'n comp':>7}{'rel loss':>10}{'rel dz':>9}  form")
    for regime in args.regimes.split(","):
        for name in args.sizes.split(","):
            sz = SIZES[name]
            torch.manual_seed(1)
            dec = Decode(groups, n_inp, sz["hidden"], sz["D"]).requires_grad_(False).set_compute_dtype("bf16").to(dev)
            for members, B in REGIMES[regime]:
                Bm = B * members
                g = torch.Generator().manual_seed(100 + B + members)
                z = (torch.randn(B, 1, P, len(groups), sz["D"], generator=g) + 0.3 * torch.randn(B, members, P, len(groups), sz["D"], generator=g)).view(Bm, P, len(groups), sz["D"])
                z = z.to(dev).requires_grad_(True)
                obs = torch.randn(B, P, F, n_inp, generator=g).to(dev)
                carried = ops.decode_member_crps_grad_supported(sz["hidden"], members)
                packed = carried and ops.decode_member_crps_pack_supported(sz["hidden"], members)
                with_comp = Bm * P <= args.max_composed_rows

                def grad(fused, pack=False, z=z, dec=dec, obs=obs, members=members):
                    z.grad = None
                    loss, _ = dec.member_crps_loss(z, obs, members, counts=mesh_counts, fused=fused, pack=pack)
                    loss.sum().backward()
                    return loss.detach(), z.grad

                def score(z=z, dec=dec, obs=obs, members=members):
                    with torch.no_grad():
                        return dec.member_verify(z, obs, members, counts=mesh_counts, fused=True, maps=())["sums"]

                fns, tags = [], []
                if carried:
                    fns.append(lambda gr=grad: gr(True))
                    tags.append("fused")
                if packed:
                    fns.append(lambda gr=grad: gr(True, True))
                    tags.append("pack")
                if with_comp:
                    fns.append(lambda gr=grad: gr(False))
                    tags.append("comp")
                fns.append(score)
                tags.append("score")
                t, spread = device_ms(fns, args.reps)
                ms = dict(zip(tags, t))
                sp = dict(zip(tags, ("%.3f-%.3f" % s for s in spread)))
                mem = {k: extra_bytes(fn) for k, fn in zip(tags, fns) if k != "score"}
                nl = {k: (None if args.no_launch_count else count_launches(fn)) for k, fn in zip(tags, fns) if k != "score"}
                e_l = e_g = float("nan")
                form, bits = "refused", "-"
                if carried:
                    lf, gf = grad(True)
                    lf, gf = lf.clone(), gf.clone()
                    form = "carried"
                    if packed:
                        lp, gp = grad(True, True)
                        form = "carried, pk%d x %d histories" % ops.decode_member_crps_pack_shape(sz["hidden"], members)
                        bits = "same" if torch.equal(lp.view(torch.int32), lf.view(torch.int32)) and torch.equal(gp.view(torch.int32), gf.view(torch.int32)) else "DIFFER"
                    if with_comp:
                        lc, gc = grad(False)
                        e_l, e_g = float((lf - lc).norm() / lc.norm()), float((gf - gc).norm() / gc.norm())
                recs.append(dict(regime=regime, size=name, members=members, B=B, rows=Bm * P, ms=ms, spread=sp, extra_bytes=mem, launches=nl, form=form, pack_bits=bits,
                                 fused_vs_composed_loss_rel_l2=e_l, fused_vs_composed_dz_rel_l2=e_g))
                f3 = lambda k: ("%.4f" % ms[k]) if k in ms else "-"   # noqa: E731
                ratio = ("%.2f" % (ms["comp"] / ms["fused"])) if "fused" in ms and "comp" in ms else "-"
                pratio = ("%.2f" % (ms["fused"] / ms["pack"])) if "fused" in ms and "pack" in ms else "-"
                mb = lambda k: ("%.1f" % (mem[k] / 2 ** 20)) if k in mem else "-"   # noqa: E731
                emit(f"{regime:<9}{name:<11}{members:>8}{B:>5}{Bm * P:>8}{f3('fused'):>12}{sp.get('fused', '-'):>16}{f3('comp'):>11}{sp.get('comp', '-'):>16}{ratio:>11}"
                     f"{f3('pack'):>11}{sp.get('pack', '-'):>16}{pratio:>11}{bits:>6}{f3('score'):>12}{sp.get('score', '-'):>16}{mb('fused'):>10}{mb('comp'):>10}{str(nl.get('fused', '-')):>8}{str(nl.get('comp', '-')):>7}{e_l:>10.1e}{e_g:>9.1e}  {form}")
                flush()
                z.grad = None
                del z, obs, fns
                torch.cuda.empty_cache()
    emit(json.dumps(dict(tool="crps_loss_bench", n_inp=n_inp, rows=recs)))
    flush()


if __name__ == "__main__":
    main()
