"""The dense-snapshot score with a precision map and its latent gradient on the clock (Decode.field_loss, sea_decode_field_grad):

  ms per call at the two decoder sizes of tools/decode_loss_bench.py (cylinder: hidden 480, D 16; multiphase: hidden 624, D 32; P = 64 patches,
  fields [[0, 1], [2]], the same synthetic wake-refined mesh, n_inp 1628), 64 members per history, B = 1 and 4 histories, bf16, for four settings:
    valid        every column valid, no map                      counts    the mesh's counts, no map
    map          a precision map with 30 % of the cells missing  map+cnt   the same map with the mesh's counts
  (the map settings also carry a field precision), and per setting:
    score fused     Decode.field_loss(fused=True) under no_grad: first layer, the score-only form of sea_decode_field_grad, finish
    score composed  Decode.field_loss(fused=False) under no_grad: forward() plus torch ops with the same selects
    grad fused      Decode.field_loss(fused=True).sum().backward(): first layer (pre-activation kept), sea_decode_field_grad + finish, data-gradient launch
    grad composed   Decode.field_loss(fused=False).sum().backward(): forward() under autograd, the torch ops and their backward
    mse fused       Decode.mse_loss(fused=True) + backward against the snapshot repeated per member (no map, no per-member score): where no map is asked for
  beside each the peak of allocated memory above its value before the call, and (last, once per form) the number of device launches of one call as
  the profiler counts them.  Device time: windows of back-to-back calls between two events, at least 20 ms each, the forms alternating inside every
  repeat (tools/ensemble_bench.device_ms).  Decode.field_loss's fused=None rule is read from these rows.

    python tools/field_grad_bench.py [--reps 7] [--out profiles/field_grad_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.decode_loss_bench import SIZES, mesh  # noqa: E402
from tools.ensemble_bench import MEMBERS, device_ms, extra_bytes  # noqa: E402
from tools.sensor_bench import count_launches  # noqa: E402

SETTINGS = ("valid", "counts", "map", "map+cnt")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="cylinder,multiphase")
    ap.add_argument("--histories", default="1,4")
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("field_grad_bench.py needs an MI355X: no GPU visible")
    from sea_amd.models.encoder_decoder import Decode

    dev = torch.device("cuda", 0)
    groups, P, F = [[0, 1], [2]], 64, 3
    n_inp, mesh_counts = mesh(dev)
    lines, record = [], dict(tool="field_grad_bench", n_inp=n_inp, members=MEMBERS)

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out:
            with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"field_grad_bench: Decode.field_loss, {MEMBERS} members per history, P = {P}, fields {groups}, n_inp = {n_inp}, bf16, device time in ms, median of "
         f"{args.reps} windows (lo-hi: the windows' range); map: 30 % of the cells missing, field precision [1.5, 0.5, 2]; MB: peak of allocated memory above its value before the call")
    emit(f"{'size':<11}{'B':>3}{'rows':>7}{'setting':>9}{'score fused':>13}{'lo-hi':>14}{'score comp':>12}{'lo-hi':>14}{'comp/fused':>11}{'grad fused':>12}{'lo-hi':>14}"
         f"{'grad comp':>11}{'lo-hi':>14}{'comp/fused':>11}{'mse fused':>11}{'MB sc f':>9}{'MB sc c':>9}{'MB gr f':>9}{'MB gr c':>9}{'rel wsse':>10}{'rel dz':>9}")
    recs, keep = [], {}
    for name in args.sizes.split(","):
        sz = SIZES[name]
        torch.manual_seed(1)
        dec = Decode(groups, n_inp, sz["hidden"], sz["D"]).requires_grad_(False).set_compute_dtype("bf16").to(dev)
        for B in [int(v) for v in args.histories.split(",")]:
            Bm = B * MEMBERS
            g = torch.Generator().manual_seed(100 + B)
            z = torch.randn(Bm, P, len(groups), sz["D"], device=dev, requires_grad=True)
            obs = torch.randn(B, P, F, n_inp, generator=g).to(dev)
            pm = 0.25 + 3.75 * torch.rand(B, P, F, n_inp, generator=g)
            pm[torch.rand(B, P, F, n_inp, generator=g) < 0.3] = 0.0
            pm = pm.to(dev)
            fp = torch.tensor([1.5, 0.5, 2.0], device=dev)
            per_member = obs.repeat_interleave(MEMBERS, 0)                       # mse_loss takes one target per row of z
            for setting in SETTINGS:
                counts = mesh_counts if setting in ("counts", "map+cnt") else None
                prec, fprec = (pm, fp) if setting.startswith("map") else (None, None)

                def score(fused, z=z, counts=counts, prec=prec, fprec=fprec, dec=dec, obs=obs):
                    with torch.no_grad():
                        return dec.field_loss(z, obs, members=MEMBERS, counts=counts, precision=prec, field_precision=fprec, fused=fused)

                def grad(fused, z=z, counts=counts, prec=prec, fprec=fprec, dec=dec, obs=obs):
                    z.grad = None
                    dec.field_loss(z, obs, members=MEMBERS, counts=counts, precision=prec, field_precision=fprec, fused=fused).sum().backward()
                    return z.grad

                def mse(z=z, counts=counts, dec=dec, per_member=per_member):
                    z.grad = None
                    dec.mse_loss(z, per_member, counts=counts, fused=True).backward()
                    return z.grad

                fns = [lambda s=score: s(True), lambda s=score: s(False), lambda g=grad: g(True), lambda g=grad: g(False)] + ([mse] if prec is None else [])   # bound now: the names are rebound per setting
                t, spread = device_ms(fns, args.reps)
                e_w = float((fns[0]() - fns[1]()).norm() / fns[1]().norm())
                a, b = fns[2]().clone(), fns[3]().clone()
                e_g = float((a - b).norm() / b.norm())
                mem = [extra_bytes(fn) for fn in fns[:4]]
                rec = dict(size=name, B=B, rows=Bm * P, setting=setting, score_fused_ms=t[0], score_composed_ms=t[1], grad_fused_ms=t[2], grad_composed_ms=t[3],
                           mse_fused_ms=t[4] if prec is None else None, spread_ms=spread, extra_bytes=dict(zip(("score_fused", "score_composed", "grad_fused", "grad_composed"), mem)),
                           fused_vs_composed_wsse_rel_l2=e_w, fused_vs_composed_dz_rel_l2=e_g)
                recs.append(rec)
                w = ["%.3f-%.3f" % s for s in spread]
                emit(f"{name:<11}{B:>3}{Bm * P:>7}{setting:>9}{t[0]:>13.4f}{w[0]:>14}{t[1]:>12.4f}{w[1]:>14}{t[1] / t[0]:>11.2f}{t[2]:>12.4f}{w[2]:>14}{t[3]:>11.4f}{w[3]:>14}"
                     f"{t[3] / t[2]:>11.2f}{(('%.4f' % t[4]) if prec is None else '-'):>11}" + "".join(f"{m / 2**20:>9.1f}" for m in mem) + f"{e_w:>10.1e}{e_g:>9.1e}")
                flush()
                if name == "cylinder" and B == 1 and setting == "map+cnt":
                    keep = dict(score_fused=fns[0], score_composed=fns[1], grad_fused=fns[2], grad_composed=fns[3])
            z.grad = None
            del z, per_member
            torch.cuda.empty_cache()
    record["field_loss"] = recs
    emit(json.dumps(record))
    flush()
    if keep and not args.no_launch_count:
        counts = {k: count_launches(fn) for k, fn in keep.items()}
        emit("device launches of one call (cylinder, B = 1, map+cnt), by the profiler: " + ", ".join(f"{k} {'not available' if v is None else v}" for k, v in counts.items()))
        flush()


if __name__ == "__main__":
    main()
