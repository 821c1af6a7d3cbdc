"""Sensors that read a derived quantity on the clock (DerivedSensorSet through Decode.sensor_sse / Decode.sensor_loss; sea_decode_derived_sensor_sse and
sea_decode_derived_sensor_grad):

  ms per call at the cylinder decoder of tools/decode_loss_bench.py (hidden 480, D 16; P = 64 patches, fields [[0, 1], [2]], the same synthetic
  wake-refined mesh), 64 members per history, B = 1 and 4 histories, bf16, K = 16, 256 and 4096 SPEED readings |(u, v)| (fields 0 and 1, with an
  inverse affine) spread evenly over 4, 32 and all 64 patches as in tools/sensor_bench.py, a precision per history and reading with a tenth of the
  readings missing:
    score      Decode.sensor_sse(derived set, fused=True): sea_decode_derived_sensor_sse
    plain 2K   Decode.sensor_sse(fused=True) on the 2 K COMPONENT sensors of the same states (the baseline: the same gathered rows, tiles and
               launch count: what is left is the epilogue — measured at about 5 % of the call)
    comp       Decode.sensor_sse(derived set, fused=False): forward() over every cell, a gather of both sources, the derived values in torch ops
    grad       Decode.sensor_loss(derived set, fused=True).sum().backward(): sea_decode_derived_sensor_grad
    plain 2K g Decode.sensor_loss(fused=True).sum().backward() on the 2 K component sensors
    comp g     Decode.sensor_loss(derived set, fused=False).sum().backward(): the composed path under autograd
  beside each the peak of allocated memory above its value before the call, and (last, once per form) the number of device launches of one call as
  the profiler counts them.  Device time: windows of back-to-back calls between two events, at least 20 ms each, the forms alternating inside every
  repeat (tools/ensemble_bench.device_ms); lo-hi is the range of the windows, which a difference of medians must exceed to mean anything.

    python tools/derived_sensor_bench.py [--reps 7] [--out profiles/derived_sensor_bench.txt]
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
from tools.sensor_bench import count_launches, spread_sensors  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("derived_sensor_bench.py needs an MI355X: no GPU visible")
    from sea_amd.ensemble import DerivedField, DerivedSensorSet, SensorSet
    from sea_amd.models.encoder_decoder import Decode

    dev = torch.device("cuda", 0)
    groups, P = [[0, 1], [2]], 64
    n_inp, _ = mesh(dev)
    sz = SIZES["cylinder"]
    lines, record = [], dict(tool="derived_sensor_bench", n_inp=n_inp, members=MEMBERS, hidden=sz["hidden"])

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out:
            with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"derived_sensor_bench: K speed readings |(u, v)| of a DerivedSensorSet against the 2 K component sensors of a SensorSet and against the composed path; "
         f"cylinder decoder (hidden {sz['hidden']}, D {sz['D']}), {MEMBERS} members per history, P = {P}, fields {groups}, n_inp = {n_inp}, bf16, precision [B, K] with a "
         f"tenth of the readings missing, device time in ms, median of {args.reps} windows (lo-hi: the windows' range)")
    emit(f"{'B':>2}{'K':>6}{'patches':>8}{'K_pad':>7} |{'score':>8}{'lo-hi':>14}{'plain 2K':>10}{'lo-hi':>14}{'ratio':>7}{'comp':>8}{'lo-hi':>14} |"
         f"{'grad':>8}{'lo-hi':>14}{'plain 2K g':>11}{'lo-hi':>14}{'ratio':>7}{'comp g':>8}{'lo-hi':>14} |"
         f"{'MB: score':>10}{'plain':>7}{'comp':>8}{'grad':>7}{'plain g':>8}{'comp g':>8}{'rel dz':>9}")
    torch.manual_seed(1)
    dec = Decode(groups, n_inp, sz["hidden"], sz["D"]).requires_grad_(False).set_compute_dtype("bf16").to(dev)
    speed = DerivedField("magnitude", 0, 1, scale_a=0.5, shift_a=0.5, scale_b=0.25, shift_b=0.0)   # an inverse affine, as MeshUnpatcher.derived_fields gives
    recs, keep = [], {}
    for B in (1, 4):
        Bm = B * MEMBERS
        z = torch.randn(Bm, P, len(groups), sz["D"], device=dev, requires_grad=True)
        for K in (16, 256, 4096):
            for n_obs in (4, 32, 64):
                if K < n_obs and n_obs == 64:
                    continue                                                # K = 16 over 32 and over 64 patches is the same set
                g = torch.Generator().manual_seed(K + n_obs)
                patch, cell, _, q = spread_sensors(K, n_obs, P, n_inp, groups, g)
                s = DerivedSensorSet(dec, P, patch, cell, [speed] * K)
                s2 = SensorSet(dec, P, patch * 2, cell * 2, [0] * K + [1] * K)
                assert s.K_pad == s2.K_pad                                  # the same gathered rows in the same number of tiles
                obs = (1.0 + torch.randn(B, K, generator=g)).to(dev)
                prec = 0.5 + torch.rand(B, K, generator=g)
                prec[torch.rand(B, K, generator=g) < 0.1] = 0.0
                prec = prec.to(dev)
                obs2, prec2 = torch.cat([obs, obs], 1).contiguous(), torch.cat([prec, prec], 1).contiguous()

                def score(fused=True, z=z, s=s, obs=obs, prec=prec):
                    return dec.sensor_sse(z, s, obs, precision=prec, members=MEMBERS, fused=fused)

                def plain(z=z, s2=s2, obs2=obs2, prec2=prec2):
                    return dec.sensor_sse(z, s2, obs2, precision=prec2, members=MEMBERS, fused=True)

                def comp():
                    return score(False)

                def grad(fused=True, z=z, s=s, obs=obs, prec=prec):
                    z.grad = None
                    dec.sensor_loss(z, s, obs, precision=prec, members=MEMBERS, fused=fused).sum().backward()
                    return z.grad

                def plain_g(z=z, s2=s2, obs2=obs2, prec2=prec2):
                    z.grad = None
                    dec.sensor_loss(z, s2, obs2, precision=prec2, members=MEMBERS, fused=True).sum().backward()
                    return z.grad

                def comp_g():
                    return grad(False)

                fns = [score, plain, comp, grad, plain_g, comp_g]
                ms, spread = device_ms(fns, args.reps)
                a, b = grad().clone(), comp_g().clone()
                err = float((a - b).norm() / b.norm())
                mem = [extra_bytes(f) for f in fns]
                names = ("score", "plain2k", "composed", "grad", "plain2k_grad", "composed_grad")
                rec = dict(B=B, K=K, patches=q, K_pad=s.K_pad, ms=dict(zip(names, ms)), windows=dict(zip(names, spread)), extra_bytes=dict(zip(names, mem)),
                           fused_vs_composed_dz_rel_l2=err)
                recs.append(rec)
                w = ["%.3f-%.3f" % sp for sp in spread]
                mb = [m / 2**20 for m in mem]
                emit(f"{B:>2}{K:>6}{q:>8}{s.K_pad:>7} |{ms[0]:>8.4f}{w[0]:>14}{ms[1]:>10.4f}{w[1]:>14}{ms[0] / ms[1]:>7.2f}{ms[2]:>8.4f}{w[2]:>14} |"
                     f"{ms[3]:>8.4f}{w[3]:>14}{ms[4]:>11.4f}{w[4]:>14}{ms[3] / ms[4]:>7.2f}{ms[5]:>8.4f}{w[5]:>14} |"
                     f"{mb[0]:>10.2f}{mb[1]:>7.2f}{mb[2]:>8.2f}{mb[3]:>7.2f}{mb[4]:>8.2f}{mb[5]:>8.2f}{err:>9.1e}")
                flush()
                if B == 1 and K == 256 and n_obs == 32:
                    keep = dict(zip(names, fns))
        z.grad = None
        del z
        torch.cuda.empty_cache()
    record["rows"] = recs
    emit(json.dumps(record))
    flush()
    if keep and not args.no_launch_count:
        counts = {k: count_launches(fn) for k, fn in keep.items()}
        emit("device launches of one call (B = 1, K = 256 over 32 patches), by the profiler: "
             + ", ".join(f"{k} {'not available' if v is None else v}" for k, v in counts.items()))
        flush()


if __name__ == "__main__":
    main()
