"""Verification of an ensemble at the sensors on the clock (SensorVerification.from_predictions: sea_ensemble_verify):

  ms of one from_predictions call on predictions that exist already (float32 [B * members, K], as SensorKalman.transform returns them), 64 members per
  history, K = 16, 256 and 4096 sensors, B = 1 and 4 histories, a precision per history and sensor with a tenth of the readings missing, with and
  without log-weights, and two rows at 128 members:
    fused      SensorVerification(fused=True): the two launches of sea_ensemble_verify
    composed   SensorVerification(fused=False): the same formulas as fp64 torch ops on the device (a stable sort, a cumulative sum, gathers)
  beside each the peak of allocated memory above its value before the call, the largest difference between the two paths' CRPS, and (last, once per
  form) the number of device launches of one call as the profiler counts them.  Device time: windows of back-to-back calls between two events, at
  least 20 ms each, the forms alternating inside every repeat (tools/ensemble_bench.device_ms).  The decoder only names the sensors here: nothing is
  decoded.

    python tools/verify_bench.py [--reps 7] [--out profiles/verify_bench.txt]
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
        raise SystemExit("verify_bench.py needs an MI355X: no GPU visible")
    from sea_amd.ensemble import SensorSet, SensorVerification
    from sea_amd.models.encoder_decoder import Decode

    dev = torch.device("cuda", 0)
    groups, P = [[0, 1], [2]], 64
    n_inp, _ = mesh(dev)
    sz = SIZES["cylinder"]
    lines, record = [], dict(tool="verify_bench", n_inp=n_inp)

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out:
            with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"verify_bench: SensorVerification.from_predictions, unbiased, P = {P}, fields {groups}, n_inp = {n_inp}, precision [B, K] with a tenth of the readings "
         f"missing, device time in ms, median of {args.reps} windows (min .. max)")
    emit(f"{'members':>8}{'B':>3}{'K':>6}{'logw':>6}{'fused':>10}{'(min':>9}{'max)':>9}{'composed':>10}{'(min':>9}{'max)':>9}{'comp/fused':>11}{'fused MB':>10}{'comp MB':>9}"
         f"{'max|dcrps|':>12}")
    torch.manual_seed(1)
    dec = Decode(groups, n_inp, sz["hidden"], sz["D"]).requires_grad_(False).set_compute_dtype("bf16").to(dev)
    recs, keep = [], {}
    rows = [(MEMBERS, B, K, wl) for B in (1, 4) for K in (16, 256, 4096) for wl in (False, True)] + [(128, 1, 256, False), (128, 4, 4096, True)]
    for n, B, K, wl in rows:
        g = torch.Generator().manual_seed(K + n)
        patch, cell, field, _ = spread_sensors(K, 64, P, n_inp, groups, g)
        s = SensorSet(dec, P, patch, cell, field)
        pred = torch.randn(B * n, K, generator=g).to(dev)
        obs = torch.randn(B, K, generator=g).to(dev)
        prec = 0.5 + torch.rand(B, K, generator=g)
        prec[torch.rand(B, K, generator=g) < 0.1] = 0.0
        prec = prec.to(dev)
        logw = torch.randn(B * n, generator=g).to(dev) if wl else None
        vf, vc = SensorVerification(dec, P, n, s, fused=True), SensorVerification(dec, P, n, s, fused=False)

        def fused(vf=vf, pred=pred, obs=obs, prec=prec, logw=logw):
            return vf.from_predictions(pred, obs, prec, logw)

        def comp(vc=vc, pred=pred, obs=obs, prec=prec, logw=logw):
            return vc.from_predictions(pred, obs, prec, logw)

        (tf, tc), (sf, sc) = device_ms([fused, comp], args.reps)
        mem_f, mem_c = extra_bytes(fused), extra_bytes(comp)
        a, b = fused(), comp()
        err = float((a.crps - b.crps).abs().max())
        same = bool(torch.equal(a.rank, b.rank)) and bool(torch.equal(a.hist, b.hist))
        recs.append(dict(members=n, B=B, K=K, logw=wl, fused_ms=tf, fused_spread_ms=sf, composed_ms=tc, composed_spread_ms=sc, fused_extra_bytes=mem_f,
                         composed_extra_bytes=mem_c, max_abs_crps_difference=err, ranks_and_histograms_equal=same))
        emit(f"{n:>8}{B:>3}{K:>6}{'yes' if wl else 'no':>6}{tf:>10.4f}{sf[0]:>9.4f}{sf[1]:>9.4f}{tc:>10.4f}{sc[0]:>9.4f}{sc[1]:>9.4f}{tc / tf:>11.2f}{mem_f / 2**20:>10.2f}"
             f"{mem_c / 2**20:>9.2f}{err:>12.1e}")
        flush()
        if n == MEMBERS and B == 1 and K == 256 and not wl:
            keep["fused"], keep["composed"] = fused, comp
    record["verify"] = recs
    emit(json.dumps(record))
    flush()
    if keep and not args.no_launch_count:
        counts = {k: count_launches(fn) for k, fn in keep.items()}
        emit(f"device launches of one from_predictions call ({MEMBERS} members, B = 1, K = 256, no log-weights), by the profiler: "
             + "; ".join(f"{k}: {'not available' if v is None else v}" for k, v in counts.items()))
        flush()


if __name__ == "__main__":
    main()
