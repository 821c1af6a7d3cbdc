"""Quantile and exceedance maps of an ensemble on the clock (EnsembleQuantiles: sea_decode_member_quantiles behind the decoder's first layer):

  ms of one call at the two decoder sizes of tools/decode_loss_bench.py (cylinder: hidden 480, D 16; multiphase: hidden 624, D 32; P = 64 patches,
  fields [[0, 1], [2]], the same synthetic mesh, n_inp 1628), 64 and 128 members per history, B = 1 and 4 histories, bf16, with every column valid
  and with the mesh's counts, log-weights given, levels (0.05, 0.5, 0.95) and one threshold per field:
    fused      EnsembleQuantiles(fused=True): three quantile maps and one exceedance map
    thr only   EnsembleQuantiles(levels=(), fused=True): the exceedance map alone — the launch does not run the O(N^2) walk
    composed   EnsembleQuantiles(fused=False): Decode.forward plus a stable sort and cumulative weights in fp64 torch ops
    verify     FieldVerification(fused=True) without maps on the same states, in the same run: the nearest existing yardstick (the same decode, the
               same walk, plus its finish launch)
  beside each the peak of allocated memory above its value before the call (the fused call must not hold the members' decoded fields,
  B * members * P * 3 * n_inp * 4 bytes in fp32; its own maps are 4 * B * P * 3 * n_inp_p * 4 bytes), and (last, once per form) the number of
  device launches of one call as the profiler counts them.  Device time: windows of back-to-back calls between two events, at least 20 ms each, the
  forms alternating inside every repeat (tools/ensemble_bench.device_ms).

    python tools/quantile_bench.py [--reps 5] [--out profiles/ensemble_quantiles_bench.txt]
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

LEVELS = (0.05, 0.5, 0.95)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="cylinder,multiphase")
    ap.add_argument("--members", default="64,128")
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("quantile_bench.py needs an MI355X: no GPU visible")
    from sea_amd.ensemble import EnsembleQuantiles, FieldVerification
    from sea_amd.models.encoder_decoder import Decode

    dev = torch.device("cuda", 0)
    groups, P, F = [[0, 1], [2]], 64, 3
    n_inp, mesh_counts = mesh(dev)
    mesh_counts = mesh_counts[:P].contiguous()
    lines, record = [], dict(tool="quantile_bench", n_inp=n_inp, levels=LEVELS)

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out:
            with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"quantile_bench: EnsembleQuantiles, P = {P}, fields {groups}, n_inp = {n_inp}, bf16, levels {LEVELS}, one threshold per field, log-weights given, "
         f"device time in ms, median of {args.reps} windows; counts all: every column valid ({P * F * n_inp} cells per history), mesh: the mesh's counts "
         f"({int(mesh_counts.sum()) * F} cells); rows = B * members * P; maps MB: the four maps a call returns; fields MB: the members' decoded fields in fp32, "
         f"which the fused call must not hold; verify: FieldVerification(fused=True) without maps on the same states")
    emit(f"{'size':<11}{'N':>4}{'B':>3}{'counts':>7}{'rows':>7}{'fused':>9}{'thr only':>9}{'composed':>10}{'verify':>9}{'comp/fused':>11}{'fused MB':>10}{'thr MB':>8}{'comp MB':>10}"
         f"{'maps MB':>9}{'fields MB':>10}{'rel q':>10}")
    recs, launches = [], None
    for name in args.sizes.split(","):
        sz = SIZES[name]
        torch.manual_seed(1)
        dec = Decode(groups, n_inp, sz["hidden"], sz["D"]).requires_grad_(False).set_compute_dtype("bf16").to(dev)
        thr = torch.zeros(1, F)
        for n in (int(v) for v in args.members.split(",")):
            for B in (1, 4):
                Bm = B * n
                g = torch.Generator().manual_seed(64 + B + n)
                y = torch.randn(Bm, len(groups), P * sz["D"], device=dev).to(torch.bfloat16)
                obs = torch.randn(B, P, F, n_inp, generator=g).to(dev)
                logw = torch.randn(Bm, generator=g).to(dev)
                for cname, counts in (("all", None), ("mesh", mesh_counts)):
                    qf = EnsembleQuantiles(dec, P, n, levels=LEVELS, thresholds=thr, counts=counts, fused=True)
                    qt = EnsembleQuantiles(dec, P, n, levels=(), thresholds=thr, counts=counts, fused=True)
                    qc = EnsembleQuantiles(dec, P, n, levels=LEVELS, thresholds=thr, counts=counts, fused=False)
                    vf = FieldVerification(dec, P, n, counts=counts, sigma=0.5, fused=True)

                    def fused():
                        return qf(y, logw)

                    def thr_only():
                        return qt(y, logw)

                    def comp():
                        return qc(y, logw)

                    def verify():
                        return vf(y, obs, None, logw, maps=())

                    ms, spread = device_ms([fused, thr_only, comp, verify], args.reps)
                    mem = [extra_bytes(fn) for fn in (fused, thr_only, comp)]
                    a, b = fused()[0], comp()[0]
                    err = float((a - b).norm() / b.norm())
                    maps_mb = (len(LEVELS) + 1) * B * P * F * a.stride(3) * 4 / 2**20
                    del a, b
                    fields_mb = Bm * P * F * n_inp * 4 / 2**20
                    recs.append(dict(size=name, members=n, B=B, counts=cname, rows=Bm * P, fused_ms=ms[0], thr_only_ms=ms[1], composed_ms=ms[2], verify_no_maps_ms=ms[3],
                                     spread_ms=spread, fused_extra_bytes=mem[0], thr_only_extra_bytes=mem[1], composed_extra_bytes=mem[2], maps_bytes=int(maps_mb * 2**20),
                                     decoded_fields_bytes=Bm * P * F * n_inp * 4, fused_vs_composed_quant_rel_l2=err))
                    emit(f"{name:<11}{n:>4}{B:>3}{cname:>7}{Bm * P:>7}{ms[0]:>9.4f}{ms[1]:>9.4f}{ms[2]:>10.4f}{ms[3]:>9.4f}{ms[2] / ms[0]:>11.2f}{mem[0] / 2**20:>10.2f}"
                         f"{mem[1] / 2**20:>8.2f}{mem[2] / 2**20:>10.2f}{maps_mb:>9.2f}{fields_mb:>10.2f}{err:>10.1e}")
                    flush()
                    if name == "cylinder" and B == 1 and n == 64 and cname == "mesh" and not args.no_launch_count:
                        launches = {k: count_launches(fn) for k, fn in (("fused", fused), ("thresholds only", thr_only), ("composed", comp), ("verify, no maps", verify))}
                del y, obs, logw
                torch.cuda.empty_cache()
    record["quantiles"] = recs
    if launches is not None:
        record["launches"] = launches
        emit("device launches of one call (cylinder, 64 members, B = 1, the mesh's counts; the decoder's first layer and the weights' normalisation included), by the "
             "profiler: " + "; ".join(f"{k}: {'not available' if v is None else v}" for k, v in launches.items()))
    emit(json.dumps(record))
    flush()


if __name__ == "__main__":
    main()
