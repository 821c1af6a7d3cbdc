"""The sparse-sensor score with its latent gradient on the clock (Decode.sensor_loss + backward, sea_decode_sensor_grad):

  ms per call at the two decoder sizes of tools/decode_loss_bench.py (cylinder: hidden 480, D 16; multiphase: hidden 624, D 32; P = 64 patches,
  fields [[0, 1], [2]], the same synthetic wake-refined mesh), 64 members per history, B = 1 and 4 histories, bf16, for the sensor layouts of
  tools/sensor_bench.py (K = 16, 256 and 4096 sensors spread evenly over 4, 32 and all 64 patches, a precision per history and sensor with a tenth
  of the readings missing):
    fused      Decode.sensor_loss(fused=True).sum().backward(): gather of the observed patches, first layer over those rows (pre-activation kept),
               sea_decode_sensor_grad + finish, data-gradient launch against W1^T, index_copy_ into the zeroed dz
    composed   Decode.sensor_loss(fused=False).sum().backward(): forward() over every cell under autograd, a gather at the sensors, torch
               reductions, and their backward over all P patches
    score      Decode.sensor_sse(fused=True): the score alone — what the gradient adds is fused - score
  beside each the peak of allocated memory above its value before the call, and (last, once per form) the number of device launches of one call as
  the profiler counts them.  Device time: windows of back-to-back calls between two events, at least 20 ms each, the three forms alternating inside
  every repeat (tools/ensemble_bench.device_ms).  There is no earlier path of this kind to compare the kernel with: the comparison is fused against
  composed, and against the score-only call.

    python tools/sensor_grad_bench.py [--reps 7] [--out profiles/sensor_grad_bench.txt]
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
    ap.add_argument("--sizes", default="cylinder,multiphase")
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sensor_grad_bench.py needs an MI355X: no GPU visible")
    from sea_amd.ensemble import SensorSet
    from sea_amd.models.encoder_decoder import Decode

    dev = torch.device("cuda", 0)
    groups, P = [[0, 1], [2]], 64
    n_inp, _ = mesh(dev)
    lines, record = [], dict(tool="sensor_grad_bench", n_inp=n_inp, members=MEMBERS)

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out:
            with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"sensor_grad_bench: Decode.sensor_loss + backward, {MEMBERS} members per history, P = {P}, fields {groups}, n_inp = {n_inp}, bf16, precision [B, K] with a "
         f"tenth of the readings missing, device time, median of {args.reps} windows; score = Decode.sensor_sse(fused=True), no gradient")
    emit(f"{'size':<11}{'B':>3}{'K':>6}{'patches':>8}{'K_pad':>7}{'fused ms':>10}{'composed ms':>13}{'score ms':>10}{'fused lo-hi':>16}{'composed lo-hi':>16}{'comp/fused':>11}{'fused-score':>12}"
         f"{'fused MB':>10}{'composed MB':>13}{'score MB':>10}{'rel dz':>9}")
    recs, keep = [], {}
    for name in args.sizes.split(","):
        sz = SIZES[name]
        torch.manual_seed(1)
        dec = Decode(groups, n_inp, sz["hidden"], sz["D"]).requires_grad_(False).set_compute_dtype("bf16").to(dev)
        for B in (1, 4):
            Bm = B * MEMBERS
            z = torch.randn(Bm, P, len(groups), sz["D"], device=dev, requires_grad=True)
            for K in (16, 256, 4096):
                for n_obs in (4, 32, 64):
                    if K < n_obs and n_obs == 64:
                        continue                                            # K = 16 over 32 and over 64 patches is the same set
                    g = torch.Generator().manual_seed(K + n_obs)
                    patch, cell, field, q = spread_sensors(K, n_obs, P, n_inp, groups, g)
                    s = SensorSet(dec, P, patch, cell, field)
                    obs = torch.randn(B, K, generator=g).to(dev)
                    prec = 0.5 + torch.rand(B, K, generator=g)
                    prec[torch.rand(B, K, generator=g) < 0.1] = 0.0
                    prec = prec.to(dev)

                    def loss_backward(fused, z=z, s=s, obs=obs, prec=prec, dec=dec):
                        z.grad = None
                        dec.sensor_loss(z, s, obs, precision=prec, members=MEMBERS, fused=fused).sum().backward()
                        return z.grad

                    def fused():
                        return loss_backward(True)

                    def composed():
                        return loss_backward(False)

                    def score(z=z, s=s, obs=obs, prec=prec, dec=dec):
                        return dec.sensor_sse(z, s, obs, precision=prec, members=MEMBERS, fused=True)

                    (tf, tc, ts), spread = device_ms([fused, composed, score], args.reps)
                    a, b = fused().clone(), composed().clone()
                    err = float((a - b).norm() / b.norm())
                    mem_f, mem_c, mem_s = extra_bytes(fused), extra_bytes(composed), extra_bytes(score)
                    rec = dict(size=name, B=B, K=K, patches=q, K_pad=s.K_pad, fused_ms=tf, composed_ms=tc, score_ms=ts, spread_ms=spread, fused_extra_bytes=mem_f,
                               composed_extra_bytes=mem_c, score_extra_bytes=mem_s, fused_vs_composed_dz_rel_l2=err)
                    recs.append(rec)
                    wf, wc = "%.3f-%.3f" % spread[0], "%.3f-%.3f" % spread[1]                # the windows' range: what a difference of medians must exceed
                    emit(f"{name:<11}{B:>3}{K:>6}{q:>8}{s.K_pad:>7}{tf:>10.4f}{tc:>13.4f}{ts:>10.4f}{wf:>16}{wc:>16}{tc / tf:>11.2f}{tf - ts:>12.4f}{mem_f / 2**20:>10.2f}"
                         f"{mem_c / 2**20:>13.2f}{mem_s / 2**20:>10.2f}{err:>9.1e}")
                    flush()
                    if name == "cylinder" and B == 1 and K == 256 and n_obs == 32:
                        keep = dict(fused=fused, composed=composed, score=score)
            z.grad = None
            del z
            torch.cuda.empty_cache()
    record["sensor_loss"] = recs
    emit(json.dumps(record))
    flush()
    if keep and not args.no_launch_count:
        counts = {k: count_launches(fn) for k, fn in keep.items()}
        emit("device launches of one call (cylinder, B = 1, K = 256 over 32 patches), by the profiler: "
             + ", ".join(f"{k} {'not available' if v is None else v}" for k, v in counts.items()))
        flush()


if __name__ == "__main__":
    main()
