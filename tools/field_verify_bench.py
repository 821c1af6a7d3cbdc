"""Verification of an ensemble against a dense snapshot on the clock (FieldVerification: sea_decode_member_verify behind the decoder's first layer):

  ms of one verify call at the two decoder sizes of tools/decode_loss_bench.py (cylinder: hidden 480, D 16; multiphase: hidden 624, D 32; P = 64
  patches, fields [[0, 1], [2]], the same synthetic mesh, n_inp 1628), 64 and 128 members per history, B = 1 and 4 histories, bf16, with every column
  valid and with the mesh's counts, a precision map with a tenth of the cells missing, log-weights given:
    fused      FieldVerification(fused=True) with all five maps, and with no map (sums and histograms only)
    composed   FieldVerification(fused=False): Decode.forward plus the formulas as fp64 torch ops with every cell a sensor (all five maps)
  beside each the peak of allocated memory above its value before the call (torch.cuda.max_memory_allocated around the call: the fused call must not
  hold the members' decoded fields, B * members * P * 3 * n_inp * 4 bytes in fp32), and (last, once per form) the number of device launches of one
  call as the profiler counts them.  Device time: windows of back-to-back calls between two events, at least 20 ms each, the forms alternating inside
  every repeat (tools/ensemble_bench.device_ms).  The last rows show the other route that existed before: SensorVerification with every valid cell
  declared a sensor, cylinder, one history, 64 members (a row that does not fit says so).

    python tools/field_verify_bench.py [--reps 5] [--out profiles/field_verify_bench.txt]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="cylinder,multiphase")
    ap.add_argument("--members", default="64,128")
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--no-sensor-rows", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("field_verify_bench.py needs an MI355X: no GPU visible")
    from sea_amd.ensemble import FieldVerification, SensorSet, SensorVerification
    from sea_amd.models.encoder_decoder import Decode

    dev = torch.device("cuda", 0)
    groups, P, F = [[0, 1], [2]], 64, 3
    n_inp, mesh_counts = mesh(dev)
    mesh_counts = mesh_counts[:P].contiguous()
    lines, record = [], dict(tool="field_verify_bench", n_inp=n_inp)

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out:
            with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"field_verify_bench: FieldVerification, P = {P}, fields {groups}, n_inp = {n_inp}, bf16, sigma 0.5, a precision map with a tenth of the cells missing, "
         f"log-weights given, device time in ms, median of {args.reps} windows; counts all: every column valid ({P * F * n_inp} cells per history), mesh: the "
         f"mesh's counts ({int(mesh_counts.sum()) * F} cells); rows = B * members * P; fields MB: the members' decoded fields in fp32, which the fused call must not hold")
    emit(f"{'size':<11}{'N':>4}{'B':>3}{'counts':>7}{'rows':>7}{'fused':>9}{'no maps':>9}{'composed':>10}{'comp/fused':>11}{'fused MB':>10}{'no-map MB':>10}{'comp MB':>10}"
         f"{'fields MB':>10}{'rel crps':>10}")
    recs, keep = [], {}
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
                prec = 0.5 + torch.rand(B, P, F, n_inp, generator=g)
                prec[torch.rand(B, P, F, n_inp, generator=g) < 0.1] = 0.0
                prec = prec.to(dev)
                logw = torch.randn(Bm, generator=g).to(dev)
                for cname, counts in (("all", None), ("mesh", mesh_counts)):
                    vf = FieldVerification(dec, P, n, counts=counts, sigma=0.5, fused=True)
                    vc = FieldVerification(dec, P, n, counts=counts, sigma=0.5, fused=False)

                    def fused():
                        return vf(y, obs, prec, logw)

                    def fused_no_maps():
                        return vf(y, obs, prec, logw, maps=())

                    def comp():
                        return vc(y, obs, prec, logw)

                    ms, spread = device_ms([fused, fused_no_maps, comp], args.reps)
                    mem = [extra_bytes(fn) for fn in (fused, fused_no_maps, comp)]
                    a, b = fused().crps, comp().crps
                    err = float((a - b).norm() / b.norm())
                    del a, b
                    fields_mb = Bm * P * F * n_inp * 4 / 2**20
                    rec = dict(size=name, members=n, B=B, counts=cname, rows=Bm * P, fused_ms=ms[0], fused_no_maps_ms=ms[1], composed_ms=ms[2], spread_ms=spread,
                               fused_extra_bytes=mem[0], fused_no_maps_extra_bytes=mem[1], composed_extra_bytes=mem[2], decoded_fields_bytes=Bm * P * F * n_inp * 4,
                               fused_vs_composed_crps_rel_l2=err)
                    recs.append(rec)
                    emit(f"{name:<11}{n:>4}{B:>3}{cname:>7}{Bm * P:>7}{ms[0]:>9.4f}{ms[1]:>9.4f}{ms[2]:>10.4f}{ms[2] / ms[0]:>11.2f}{mem[0] / 2**20:>10.2f}{mem[1] / 2**20:>10.2f}"
                         f"{mem[2] / 2**20:>10.2f}{fields_mb:>10.2f}{err:>10.1e}")
                    flush()
                    if name == "cylinder" and B == 1 and n == 64 and cname == "mesh":
                        keep["fused"], keep["fused, no maps"], keep["composed"] = fused, fused_no_maps, comp
                        if not args.no_launch_count:
                            launches = {k: count_launches(fn) for k, fn in keep.items()}
                            record["launches"] = launches
                        keep.clear()
                del y, obs, prec, logw
                torch.cuda.empty_cache()
    record["field_verify"] = recs
    if "launches" in record:
        emit("device launches of one verify call (cylinder, 64 members, B = 1, the mesh's counts; the decoder's first layer included), by the profiler: "
             + "; ".join(f"{k}: {'not available' if v is None else v}" for k, v in record["launches"].items()))
        flush()

    # the other route: every valid cell a sensor of SensorVerification
    srecs = []
    if not args.no_sensor_rows:
        sz, n = SIZES["cylinder"], 64
        torch.manual_seed(1)
        dec = Decode(groups, n_inp, sz["hidden"], sz["D"]).requires_grad_(False).set_compute_dtype("bf16").to(dev)
        y = torch.randn(n, len(groups), P * sz["D"], device=dev).to(torch.bfloat16)
        host_counts = [int(v) for v in mesh_counts.cpu().tolist()]
        flat = [f for grp in groups for f in grp]
        emit(f"{'sensors as cells':<18}{'K':>8}{'verify':>10}{'extra MB':>10}   (SensorVerification, cylinder, 64 members, B = 1, every valid cell a sensor)")
        for cname, cnts in (("mesh", host_counts), ("all", [n_inp] * P)):
            try:
                patch = [p for p in range(P) for _ in range(F * cnts[p])]
                field = [f for p in range(P) for f in flat for _ in range(cnts[p])]
                cell = [c for p in range(P) for _ in range(F) for c in range(cnts[p])]
                K = len(patch)
                s = SensorSet(dec, P, patch, cell, field)
                vs = SensorVerification(dec, P, n, s, sigma=0.5, fused=True)
                g = torch.Generator().manual_seed(5)
                obs_k = torch.randn(1, K, generator=g).to(dev)
                fn = lambda: vs(y, obs_k)          # noqa: E731
                ms, _ = device_ms([fn], max(3, args.reps // 2))
                mem = extra_bytes(fn)
                srecs.append(dict(counts=cname, K=K, verify_ms=ms[0], extra_bytes=mem))
                emit(f"{cname:<18}{K:>8}{ms[0]:>10.4f}{mem / 2**20:>10.2f}")
            except (ValueError, MemoryError, torch.cuda.OutOfMemoryError) as exc:   # a size the sensor route does not take: the row says so (any other error ends the run)
                emit(f"{cname:<18} does not fit: {type(exc).__name__}: {str(exc)[:160]}")
            flush()
    record["sensor_route"] = srecs
    emit(json.dumps(record))
    flush()


if __name__ == "__main__":
    main()
