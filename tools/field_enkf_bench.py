"""The ensemble Kalman analysis from a dense snapshot on the clock (FieldKalman: sea_decode_member_gram, sea_enkf_transform_gram, sea_ensemble_mix):

  ms of the gram launch, of the transform launch and of the whole analyse call at the two decoder sizes of tools/decode_loss_bench.py (cylinder: hidden
  480, D 16; multiphase: hidden 624, D 32; P = 64 patches, fields [[0, 1], [2]], the same synthetic mesh, n_inp 1628), 64 members per history, B = 1
  and 4 histories, bf16, with one analysis domain and with P domains (a random [P, P] taper, a third of it zero), with every column valid and with
  the mesh's counts; a precision map with a tenth of the cells missing:
    fused      FieldKalman(fused=True): the three launches behind the decoder's first layer
    composed   FieldKalman(fused=False): Decode.forward plus the same formulas as fp64 torch ops and batched fp32 matrix products
  beside each the peak of allocated memory above its value before the call, and (last, once per form) the number of device launches of one analyse
  call as the profiler counts them.  Device time: windows of back-to-back calls between two events, at least 20 ms each, the forms alternating
  inside every repeat (tools/ensemble_bench.device_ms).  The last rows show the route that existed before FieldKalman: SensorKalman with every valid
  cell declared a sensor, one history, one domain, at the mesh's counts and with every column valid (the largest size; a row that does not fit says so).

    python tools/field_enkf_bench.py [--reps 7] [--out profiles/field_enkf_bench.txt]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="cylinder,multiphase")
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--no-sensor-rows", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("field_enkf_bench.py needs an MI355X: no GPU visible")
    from sea_amd import ops
    from sea_amd.ensemble import FieldKalman, SensorKalman, SensorSet, _composed_transform_gram
    from sea_amd.models.encoder_decoder import Decode

    dev = torch.device("cuda", 0)
    groups, P, F = [[0, 1], [2]], 64, 3
    n_inp, mesh_counts = mesh(dev)
    mesh_counts = mesh_counts[:P].contiguous()
    lines, record = [], dict(tool="field_enkf_bench", n_inp=n_inp, members=MEMBERS)

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out:
            with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    have_linalg = True
    try:
        _composed_transform_gram(torch.eye(4, device=dev, dtype=torch.float64).view(1, 1, 4, 4), torch.ones(1, 1, 4, device=dev, dtype=torch.float64),
                                 torch.ones(1, 1, device=dev, dtype=torch.int32), None, 4, 1.0, 0.5)
        torch.cuda.synchronize()
    except Exception as exc:   # noqa: BLE001
        have_linalg = False
        emit(f"field_enkf_bench: torch.linalg's Cholesky is not available on the device in this torch build ({type(exc).__name__}: {exc}): the kernels are reported alone")

    emit(f"field_enkf_bench: FieldKalman, {MEMBERS} members per history, P = {P}, fields {groups}, n_inp = {n_inp}, bf16, inflation 1.05, anomaly gain 0.5, a precision "
         f"map with a tenth of the cells missing, device time in ms, median of {args.reps} windows; domains 1: no taper, {P}: a taper [P, P], a third of it 0; "
         f"counts all: every column valid ({P * F * n_inp} cells per history), mesh: the mesh's counts ({int(mesh_counts.sum()) * F} cells)")
    emit(f"{'size':<11}{'B':>3}{'dom':>5}{'counts':>7}{'gram':>9}{'transform':>11}{'t comp':>9}{'analyse':>10}{'an comp':>10}{'comp/fused':>11}{'fused MB':>10}{'comp MB':>10}"
         f"{'rel':>9}")
    recs, keep = [], {}
    for name in args.sizes.split(","):
        sz = SIZES[name]
        torch.manual_seed(1)
        dec = Decode(groups, n_inp, sz["hidden"], sz["D"]).requires_grad_(False).set_compute_dtype("bf16").to(dev)
        for B in (1, 4):
            Bm = B * MEMBERS
            g = torch.Generator().manual_seed(64 + B)
            y = torch.randn(Bm, len(groups), P * sz["D"], device=dev).to(torch.bfloat16)
            obs = torch.randn(B, P, F, n_inp, generator=g).to(dev)
            prec = 0.5 + torch.rand(B, P, F, n_inp, generator=g)
            prec[torch.rand(B, P, F, n_inp, generator=g) < 0.1] = 0.0
            prec = prec.to(dev)
            z = y.reshape(Bm, len(groups), P, sz["D"]).permute(0, 2, 1, 3)
            for Ld in (1, P):
                taper = None
                if Ld > 1:
                    taper = torch.rand(P, P, generator=g)
                    taper[torch.rand(P, P, generator=g) < 1.0 / 3.0] = 0.0
                for cname, counts in (("all", None), ("mesh", mesh_counts)):
                    cells = P * F * n_inp if counts is None else int(counts.sum()) * F
                    sigma = (cells / 16.0) ** 0.5          # the total weight of the snapshot does not grow with the number of cells
                    kf = FieldKalman(dec, P, MEMBERS, counts=counts, sigma=sigma, inflation=1.05, taper=taper, fused=True)
                    kc = FieldKalman(dec, P, MEMBERS, counts=counts, sigma=sigma, inflation=1.05, taper=taper, fused=False)
                    D, status = kf.transform(y, obs, prec)
                    pf, tap = kf._field_precision(dev), kf._taper_on(dev)
                    gram, proj, count = dec.member_gram(z, obs, MEMBERS, counts=counts, precision=prec, field_precision=pf, fused=True)

                    def g_fused():
                        return dec.member_gram(z, obs, MEMBERS, counts=counts, precision=prec, field_precision=pf, fused=True)

                    def t_fused():
                        return ops.enkf_transform_gram(gram, proj, count, taper=tap, rho=1.05, alpha=0.5)

                    def t_comp():
                        return _composed_transform_gram(gram, proj, count, tap, MEMBERS, 1.05, 0.5)

                    def a_fused():
                        return kf.analyse(y, obs, prec)

                    def a_comp():
                        return kc.analyse(y, obs, prec)

                    fns = [g_fused, t_fused, a_fused] + ([t_comp, a_comp] if have_linalg else [])
                    ms, spread = device_ms(fns, args.reps)
                    gf, tf, af = ms[:3]
                    tc, ac = ms[3:] if have_linalg else (float("nan"),) * 2
                    mem_f = extra_bytes(a_fused)
                    mem_c = extra_bytes(a_comp) if have_linalg else 0
                    err = float("nan")
                    if have_linalg:
                        a = kf.analyse(y, obs, prec, increment=True)[1]
                        b = kc.analyse(y, obs, prec, increment=True)[1]
                        err = float((a - b).norm() / b.norm())
                    rec = dict(size=name, B=B, domains=Ld, counts=cname, cells=cells, gram_ms=gf, transform_ms=tf, transform_composed_ms=tc, analyse_ms=af,
                               analyse_composed_ms=ac, spread_ms=spread, fused_extra_bytes=mem_f, composed_extra_bytes=mem_c, fused_vs_composed_rel_l2=err,
                               worst_status=int(status.min()))
                    recs.append(rec)
                    emit(f"{name:<11}{B:>3}{Ld:>5}{cname:>7}{gf:>9.4f}{tf:>11.4f}{tc:>9.4f}{af:>10.4f}{ac:>10.4f}{ac / af:>11.2f}{mem_f / 2**20:>10.2f}{mem_c / 2**20:>10.2f}"
                         f"{err:>9.1e}")
                    flush()
                    if name == "cylinder" and B == 1 and cname == "mesh":
                        keep[f"fused, {Ld} domain(s)"] = lambda k=kf, y=y, o=obs, w=prec: k.analyse(y, o, w)
                        if have_linalg:
                            keep[f"composed, {Ld} domain(s)"] = lambda k=kc, y=y, o=obs, w=prec: k.analyse(y, o, w)
            del y, obs, prec
            torch.cuda.empty_cache()
    record["field_enkf"] = recs
    if keep and not args.no_launch_count:
        counts_ = {k: count_launches(fn) for k, fn in keep.items()}
        emit("device launches of one analyse call (cylinder, B = 1, the mesh's counts; the decoder's first layer included), by the profiler: "
             + "; ".join(f"{k}: {'not available' if v is None else v}" for k, v in counts_.items()))
        flush()
    keep.clear()

    # the route without FieldKalman: every valid cell a sensor of SensorKalman
    srecs = []
    if not args.no_sensor_rows:
        sz = SIZES["cylinder"]
        torch.manual_seed(1)
        dec = Decode(groups, n_inp, sz["hidden"], sz["D"]).requires_grad_(False).set_compute_dtype("bf16").to(dev)
        y = torch.randn(MEMBERS, len(groups), P * sz["D"], device=dev).to(torch.bfloat16)
        host_counts = [int(v) for v in mesh_counts.cpu().tolist()]
        flat = [f for grp in groups for f in grp]
        emit(f"{'sensors as cells':<18}{'K':>8}{'analyse':>10}{'extra MB':>10}   (SensorKalman, cylinder, B = 1, one domain, every valid cell a sensor)")
        for cname, cnts in (("mesh", host_counts), ("all", [n_inp] * P)):
            try:
                patch = [p for p in range(P) for _ in range(F * cnts[p])]
                field = [f for p in range(P) for f in flat for _ in range(cnts[p])]
                cell = [c for p in range(P) for _ in range(F) for c in range(cnts[p])]
                K = len(patch)
                s = SensorSet(dec, P, patch, cell, field)
                ks = SensorKalman(dec, P, MEMBERS, s, sigma=(K / 16.0) ** 0.5, inflation=1.05, fused=True)
                g = torch.Generator().manual_seed(5)
                obs_k = torch.randn(1, K, generator=g).to(dev)
                fn = lambda: ks.analyse(y, obs_k)          # noqa: E731
                ms, _ = device_ms([fn], max(3, args.reps // 2))
                mem = extra_bytes(fn)
                srecs.append(dict(counts=cname, K=K, analyse_ms=ms[0], extra_bytes=mem))
                emit(f"{cname:<18}{K:>8}{ms[0]:>10.4f}{mem / 2**20:>10.2f}")
            except (ValueError, MemoryError, torch.cuda.OutOfMemoryError) as exc:   # a size the sensor route does not take: the row says so (any other error ends the run)
                emit(f"{cname:<18} does not fit: {type(exc).__name__}: {str(exc)[:160]}")
            flush()
    record["sensor_route"] = srecs
    emit(json.dumps(record))
    flush()


if __name__ == "__main__":
    main()
