"""The ensemble Kalman analysis from sensor readings on the clock (SensorKalman: sea_enkf_transform, sea_ensemble_mix):

  ms of the transform launch, of the mix launch and of the whole analyse call at the two decoder sizes of tools/decode_loss_bench.py (cylinder: hidden
  480, D 16; multiphase: hidden 624, D 32; P = 64 patches, fields [[0, 1], [2]], the same synthetic mesh), 64 members per history, B = 1 and 4
  histories, bf16, K = 16, 256 and 4096 sensors spread over all patches (tools/sensor_bench.spread_sensors), a precision per history and sensor with
  a tenth of the readings missing, with one analysis domain and with P domains (a random taper, a third of it zero):
    fused      SensorKalman(fused=True): the two launches behind Decode.sensor_sse's predictions
    composed   SensorKalman(fused=False): the same formulas as fp64 torch ops on the device (torch.linalg's Cholesky) and batched fp32 matrix products
  beside each the peak of allocated memory above its value before the call, and (last, once per form) the number of device launches of one analyse
  call as the profiler counts them.  Device time: windows of back-to-back calls between two events, at least 20 ms each, the forms alternating
  inside every repeat (tools/ensemble_bench.device_ms).  If torch.linalg is not available on the device the composed columns say so and the kernels
  are reported alone.

    python tools/enkf_bench.py [--reps 7] [--out profiles/enkf_bench.txt]
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
        raise SystemExit("enkf_bench.py needs an MI355X: no GPU visible")
    from sea_amd import ops
    from sea_amd.ensemble import SensorKalman, SensorSet, _composed_mix, _composed_transform
    from sea_amd.models.encoder_decoder import Decode

    dev = torch.device("cuda", 0)
    groups, P = [[0, 1], [2]], 64
    n_inp, _ = mesh(dev)
    lines, record = [], dict(tool="enkf_bench", n_inp=n_inp, members=MEMBERS)

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out:
            with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    have_linalg = True
    try:
        _composed_transform(torch.randn(4, 3, device=dev), torch.randn(1, 3, device=dev), None, None, 4, 1.0, 0.5)
        torch.cuda.synchronize()
    except Exception as exc:   # noqa: BLE001
        have_linalg = False
        emit(f"enkf_bench: torch.linalg's Cholesky is not available on the device in this torch build ({type(exc).__name__}: {exc}): the kernels are reported alone")

    emit(f"enkf_bench: SensorKalman, {MEMBERS} members per history, P = {P}, fields {groups}, n_inp = {n_inp}, bf16, inflation 1.05, anomaly gain 0.5, precision "
         f"[B, K] with a tenth of the readings missing, device time in ms, median of {args.reps} windows; domains 1: no taper, {P}: a taper [P, K], a third of it 0")
    emit(f"{'size':<11}{'B':>3}{'K':>6}{'dom':>5}{'transform':>11}{'t comp':>9}{'mix':>9}{'mix comp':>10}{'analyse':>10}{'an comp':>10}{'comp/fused':>11}"
         f"{'fused MB':>10}{'comp MB':>9}{'rel':>9}")
    recs, keep = [], {}
    for name in args.sizes.split(","):
        sz = SIZES[name]
        torch.manual_seed(1)
        dec = Decode(groups, n_inp, sz["hidden"], sz["D"]).requires_grad_(False).set_compute_dtype("bf16").to(dev)
        for B in (1, 4):
            Bm = B * MEMBERS
            y = torch.randn(Bm, len(groups), P * sz["D"], device=dev).to(torch.bfloat16)
            for K in (16, 256, 4096):
                g = torch.Generator().manual_seed(K + 64)
                patch, cell, field, _ = spread_sensors(K, 64, P, n_inp, groups, g)
                s = SensorSet(dec, P, patch, cell, field)
                obs = torch.randn(B, K, generator=g).to(dev)
                prec = (0.5 + torch.rand(B, K, generator=g)) * (16.0 / K)     # the total weight of the readings does not grow with K
                prec[torch.rand(B, K, generator=g) < 0.1] = 0.0
                prec = prec.to(dev)
                for Ld in (1, P):
                    taper = None
                    if Ld > 1:
                        taper = torch.rand(P, K, generator=g)
                        taper[torch.rand(P, K, generator=g) < 1.0 / 3.0] = 0.0
                    kf = SensorKalman(dec, P, MEMBERS, s, inflation=1.05, taper=taper, fused=True)
                    kc = SensorKalman(dec, P, MEMBERS, s, inflation=1.05, taper=taper, fused=False)
                    D, status, pred = kf.transform(y, obs, prec)
                    tap = kf._taper_on(dev)

                    def t_fused():
                        return ops.enkf_transform(pred, obs, MEMBERS, prec=prec, taper=tap, rho=1.05, alpha=0.5)

                    def t_comp():
                        return _composed_transform(pred, obs, prec, tap, MEMBERS, 1.05, 0.5)

                    def m_fused():
                        return ops.ensemble_mix(y, D, P)

                    def m_comp():
                        return (y.to(torch.float32) + _composed_mix(y, D, P)).to(y.dtype)

                    def a_fused():
                        return kf.analyse(y, obs, prec)

                    def a_comp():
                        return kc.analyse(y, obs, prec)

                    fns = [t_fused, m_fused, a_fused] + ([t_comp, m_comp, a_comp] if have_linalg else [])
                    ms, spread = device_ms(fns, args.reps)
                    tf, mf, af = ms[:3]
                    tc, mc, ac = ms[3:] if have_linalg else (float("nan"),) * 3
                    mem_f = extra_bytes(a_fused)
                    mem_c = extra_bytes(a_comp) if have_linalg else 0
                    err = float("nan")
                    if have_linalg:
                        a = kf.analyse(y, obs, prec, increment=True)[1]
                        b = kc.analyse(y, obs, prec, increment=True)[1]
                        err = float((a - b).norm() / b.norm())
                    rec = dict(size=name, B=B, K=K, domains=Ld, transform_ms=tf, transform_composed_ms=tc, mix_ms=mf, mix_composed_ms=mc, analyse_ms=af,
                               analyse_composed_ms=ac, spread_ms=spread, fused_extra_bytes=mem_f, composed_extra_bytes=mem_c, fused_vs_composed_rel_l2=err,
                               worst_status=int(status.min()))
                    recs.append(rec)
                    emit(f"{name:<11}{B:>3}{K:>6}{Ld:>5}{tf:>11.4f}{tc:>9.4f}{mf:>9.4f}{mc:>10.4f}{af:>10.4f}{ac:>10.4f}{ac / af:>11.2f}{mem_f / 2**20:>10.2f}"
                         f"{mem_c / 2**20:>9.2f}{err:>9.1e}")
                    flush()
                    if name == "cylinder" and B == 1 and K == 256:
                        keep[f"fused, {Ld} domain(s)"] = lambda k=kf, y=y, o=obs, w=prec: k.analyse(y, o, w)
                        if have_linalg:
                            keep[f"composed, {Ld} domain(s)"] = lambda k=kc, y=y, o=obs, w=prec: k.analyse(y, o, w)
            del y
            torch.cuda.empty_cache()
    record["enkf"] = recs
    emit(json.dumps(record))
    flush()
    if keep and not args.no_launch_count:
        counts = {k: count_launches(fn) for k, fn in keep.items()}
        emit("device launches of one analyse call (cylinder, B = 1, K = 256; the predictions' launches included), by the profiler: "
             + "; ".join(f"{k}: {'not available' if v is None else v}" for k, v in counts.items()))
        flush()


if __name__ == "__main__":
    main()
