"""Threshold scores of an ensemble on the clock (FieldThresholdVerification: sea_decode_member_brier behind the decoder's first layer;
SensorThresholdVerification.from_predictions: sea_ensemble_brier):

  dense   ms of one call at the two decoder sizes of tools/decode_loss_bench.py (cylinder: hidden 480, D 16; multiphase: hidden 624, D 32; P = 64
          patches, fields [[0, 1], [2]], the same synthetic mesh, n_inp 1628), 64 and 128 members per history, B = 1 and 4 histories, bf16, T = 1 and 3
          thresholds per field, with every column valid and with the mesh's counts:
            fused      FieldThresholdVerification(fused=True) without maps, and (+maps) with both maps
            composed   FieldThresholdVerification(fused=False): Decode.forward plus the formulas in fp64 torch ops
            thr only   EnsembleQuantiles(levels=(), thresholds=the same T, fused=True) on the same states: the same decode and read-out without the
                       readings, the histograms and the finish launch — the yardstick; `ratio` is fused / thr only
          beside each the peak of allocated memory above its value before the call (the members' decoded fields alone would be B * members * P * 3 *
          n_inp * 4 bytes in fp32), and (last, once per form) the number of device launches of one call as the profiler counts them.
  sensor  ms of one from_predictions call at 16 - 4096 sensors, 64 and 128 members, one and four histories, T = 3: fused against composed.
Device time: windows of back-to-back calls between two events, at least 20 ms each, the forms alternating inside every repeat
(tools/ensemble_bench.device_ms).

    python tools/brier_bench.py [--reps 5] [--out profiles/brier_bench.txt]
    python tools/brier_bench.py --errors [--out profiles/brier_gpu_errors.txt]     the largest error / bound ratios the GPU tests print
"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.decode_loss_bench import SIZES, mesh  # noqa: E402
from tools.ensemble_bench import device_ms, extra_bytes  # noqa: E402
from tools.sensor_bench import count_launches  # noqa: E402

THRESHOLDS = (0.0, -0.5, 0.5)
SENSORS = (16, 64, 256, 1024, 4096)


def errors(out):
    """Run tests/test_brier_gpu.py and keep the lines in which its tests print their largest error / bound ratios and excluded shares."""
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_brier_gpu.py"), "-q", "-s", "-m", "gpu"], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    keep = [l.lstrip(".") for l in r.stdout.splitlines() if re.match(r"^\.*brier ", l)]
    tail = [l for l in r.stdout.splitlines() if re.search(r"\d+ (passed|failed)", l)]
    text = "\n".join(["brier_bench --errors: what tests/test_brier_gpu.py printed (python -m pytest tests/test_brier_gpu.py -q -s -m gpu)"] + keep + tail) + "\n"
    print(text, end="")
    if out:
        with open(os.path.join(ROOT, out) if not os.path.isabs(out) else out, "w") as f:
            f.write(text)
    return r.returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="cylinder,multiphase")
    ap.add_argument("--members", default="64,128")
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--errors", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("brier_bench.py needs an MI355X: no GPU visible")
    if args.errors:
        raise SystemExit(errors(args.out))
    from sea_amd.ensemble import EnsembleQuantiles, FieldThresholdVerification, SensorSet, SensorThresholdVerification
    from sea_amd.models.encoder_decoder import Decode

    dev = torch.device("cuda", 0)
    groups, P, F = [[0, 1], [2]], 64, 3
    n_inp, mesh_counts = mesh(dev)
    mesh_counts = mesh_counts[:P].contiguous()
    lines, record = [], dict(tool="brier_bench", n_inp=n_inp)

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out:
            with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"brier_bench: FieldThresholdVerification, P = {P}, fields {groups}, n_inp = {n_inp}, bf16, equal weights, device time in ms, median of {args.reps} windows; "
         f"counts all: every column valid ({P * F * n_inp} cells per history), mesh: the mesh's counts ({int(mesh_counts.sum()) * F} cells); rows = B * members * P; "
         f"thr only: EnsembleQuantiles(levels=(), the same T thresholds, fused=True) on the same states; ratio = fused / thr only; fields MB: the members' decoded "
         f"fields in fp32, which the fused call must not hold")
    emit(f"{'size':<11}{'N':>4}{'B':>3}{'T':>2}{'counts':>7}{'rows':>7}{'fused':>9}{'+maps':>9}{'composed':>10}{'thr only':>9}{'ratio':>7}{'comp/fused':>11}{'fused MB':>10}"
         f"{'+maps MB':>10}{'comp MB':>10}{'fields MB':>10}")
    recs, launches = [], None
    for name in args.sizes.split(","):
        sz = SIZES[name]
        torch.manual_seed(1)
        dec = Decode(groups, n_inp, sz["hidden"], sz["D"]).requires_grad_(False).set_compute_dtype("bf16").to(dev)
        for n in (int(v) for v in args.members.split(",")):
            for B in (1, 4):
                Bm = B * n
                g = torch.Generator().manual_seed(64 + B + n)
                y = torch.randn(Bm, len(groups), P * sz["D"], device=dev).to(torch.bfloat16)
                obs = torch.randn(B, P, F, n_inp, generator=g).to(dev)
                for T in (1, 3):
                    thr = torch.tensor(THRESHOLDS[:T]).view(T, 1).expand(T, F).contiguous()
                    for cname, counts in (("all", None), ("mesh", mesh_counts)):
                        vf = FieldThresholdVerification(dec, P, n, thr, counts=counts, fused=True)
                        vc = FieldThresholdVerification(dec, P, n, thr, counts=counts, fused=False)
                        qt = EnsembleQuantiles(dec, P, n, levels=(), thresholds=thr, counts=counts, fused=True)

                        def fused():
                            return vf(y, obs)

                        def fused_maps():
                            return vf(y, obs, maps=("prob", "brier"))

                        def comp():
                            return vc(y, obs)

                        def thr_only():
                            return qt(y)

                        ms, spread = device_ms([fused, fused_maps, comp, thr_only], args.reps)
                        mem = [extra_bytes(fn) for fn in (fused, fused_maps, comp)]
                        a, b = fused(), comp()
                        err = float((a.brier - b.brier).abs().max())
                        del a, b
                        fields_mb = Bm * P * F * n_inp * 4 / 2**20
                        recs.append(dict(size=name, members=n, B=B, T=T, counts=cname, rows=Bm * P, fused_ms=ms[0], fused_maps_ms=ms[1], composed_ms=ms[2], thr_only_ms=ms[3],
                                         spread_ms=spread, fused_extra_bytes=mem[0], fused_maps_extra_bytes=mem[1], composed_extra_bytes=mem[2],
                                         decoded_fields_bytes=Bm * P * F * n_inp * 4, fused_vs_composed_brier_abs=err))
                        emit(f"{name:<11}{n:>4}{B:>3}{T:>2}{cname:>7}{Bm * P:>7}{ms[0]:>9.4f}{ms[1]:>9.4f}{ms[2]:>10.4f}{ms[3]:>9.4f}{ms[0] / ms[3]:>7.2f}{ms[2] / ms[0]:>11.2f}"
                             f"{mem[0] / 2**20:>10.2f}{mem[1] / 2**20:>10.2f}{mem[2] / 2**20:>10.2f}{fields_mb:>10.2f}")
                        flush()
                        if name == "cylinder" and B == 1 and n == 64 and cname == "mesh" and T == 3 and not args.no_launch_count:
                            launches = {k: count_launches(fn) for k, fn in (("fused", fused), ("fused with maps", fused_maps), ("composed", comp), ("thresholds only", thr_only))}
                        del vf, vc, qt
                        torch.cuda.empty_cache()
                del y, obs
                torch.cuda.empty_cache()
    record["dense"] = recs
    if launches is not None:
        record["launches"] = launches
        emit("device launches of one call (cylinder, 64 members, B = 1, T = 3, the mesh's counts; the decoder's first layer included), by the profiler: "
             + "; ".join(f"{k}: {'not available' if v is None else v}" for k, v in launches.items()))

    # the sensor form: predictions that exist already
    sz = SIZES["cylinder"]
    torch.manual_seed(1)
    dec = Decode(groups, n_inp, sz["hidden"], sz["D"]).requires_grad_(False).set_compute_dtype("bf16").to(dev)
    emit(f"sensor form: SensorThresholdVerification.from_predictions, T = 3, precisions given, equal weights and log-weights, device time in ms, median of {args.reps} windows")
    emit(f"{'N':>4}{'B':>3}{'K':>6}{'logw':>6}{'fused':>9}{'composed':>10}{'comp/fused':>11}")
    srecs = []
    for n in (int(v) for v in args.members.split(",")):
        for B in (1, 4):
            for K in SENSORS:
                g = torch.Generator().manual_seed(K + n + B)
                sset = SensorSet(dec, P, torch.randint(0, P, (K,), generator=g).tolist(), torch.randint(0, n_inp, (K,), generator=g).tolist(),
                                 torch.randint(0, F, (K,), generator=g).tolist())
                pred = torch.randn(B * n, K, generator=g).to(dev)
                ob = torch.randn(B, K, generator=g).to(dev)
                prec = (0.5 + torch.rand(B, K, generator=g)).to(dev)
                sf = SensorThresholdVerification(dec, P, n, sset, THRESHOLDS, fused=True)
                sc = SensorThresholdVerification(dec, P, n, sset, THRESHOLDS, fused=False)
                for lname, lw in (("no", None), ("yes", torch.randn(B * n, generator=g).to(dev))):
                    ms, spread = device_ms([lambda: sf.from_predictions(pred, ob, prec, logw=lw), lambda: sc.from_predictions(pred, ob, prec, logw=lw)], args.reps)
                    srecs.append(dict(members=n, B=B, K=K, logw=lname, fused_ms=ms[0], composed_ms=ms[1], spread_ms=spread))
                    emit(f"{n:>4}{B:>3}{K:>6}{lname:>6}{ms[0]:>9.4f}{ms[1]:>10.4f}{ms[1] / ms[0]:>11.2f}")
                    flush()
    record["sensor"] = srecs
    emit(json.dumps(record))
    flush()


if __name__ == "__main__":
    main()
