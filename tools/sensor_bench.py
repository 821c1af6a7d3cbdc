"""Scoring an ensemble against sparse sensor readings on the clock (Decode.sensor_sse, sea_decode_sensor_sse):

  ms per scoring call at the two decoder sizes of tools/decode_loss_bench.py (cylinder: hidden 480, D 16; multiphase: hidden 624, D 32; P = 64
  patches, fields [[0, 1], [2]], the same synthetic wake-refined mesh), 64 members per history, B = 1 and 4 histories, bf16, for K = 16, 256 and
  4096 sensors spread evenly over 4, 32 and all 64 patches (random fields and cells; K = 16 reaches at most 16 patches), a precision per history
  and sensor with a tenth of the readings missing:
    fused      Decode.sensor_sse(fused=True): gather of the observed patches, first layer over those rows, sea_decode_sensor_sse + finish
    composed   Decode.sensor_sse(fused=False): forward() over every cell, a gather at the sensors, torch reductions
    dense      Decode.member_sse(fused=None) against a dense observation: what a user without sensor scoring would call
  beside each the peak of allocated memory above its value before the call, and (last, once per form) the number of device launches of one call as
  the profiler counts them.  Device time: windows of back-to-back calls between two events, at least 20 ms each, the three forms alternating inside
  every repeat (tools/ensemble_bench.device_ms).

    python tools/sensor_bench.py [--reps 7] [--out profiles/sensor_bench.txt]
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


def spread_sensors(K, n_obs, P, n_inp, groups, g):
    """K sensors over min(K, n_obs) patches chosen evenly from the P patches, round-robin; random fields and cells."""
    q = min(K, n_obs)
    patches = [round(i * (P - 1) / max(q - 1, 1)) for i in range(q)] if q > 1 else [P // 2]
    fields = [f for grp in groups for f in grp]
    patch = [patches[k % q] for k in range(K)]
    cell = torch.randint(n_inp, (K,), generator=g).tolist()
    field = [fields[i] for i in torch.randint(len(fields), (K,), generator=g).tolist()]
    return patch, cell, field, q


def count_launches(fn):
    """Device kernels of one call, as the profiler sees them (None when the profiler is not available)."""
    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = 0
        for e in prof.events():
            if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower():
                n += 1
        return n
    except Exception as exc:   # noqa: BLE001  (a tool: the table above does not depend on this leg)
        print(f"sensor_bench: launch count not available: {exc}", flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="cylinder,multiphase")
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sensor_bench.py needs an MI355X: no GPU visible")
    from sea_amd.ensemble import SensorSet
    from sea_amd.models.encoder_decoder import Decode

    dev = torch.device("cuda", 0)
    groups, P, n_fields = [[0, 1], [2]], 64, 3
    n_inp, _ = mesh(dev)
    lines, record = [], dict(tool="sensor_bench", n_inp=n_inp, members=MEMBERS)

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out:
            with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"sensor_bench: Decode.sensor_sse, {MEMBERS} members per history, P = {P}, fields {groups}, n_inp = {n_inp}, bf16, precision [B, K] with a tenth of the "
         f"readings missing, device time, median of {args.reps} windows; dense = Decode.member_sse(fused=None) against a dense observation")
    emit(f"{'size':<11}{'B':>3}{'K':>6}{'patches':>8}{'K_pad':>7}{'fused ms':>10}{'composed ms':>13}{'dense ms':>10}{'comp/fused':>11}{'dense/fused':>12}"
         f"{'fused MB':>10}{'composed MB':>13}{'dense MB':>10}{'rel':>9}")
    recs, keep = [], {}
    for name in args.sizes.split(","):
        sz = SIZES[name]
        torch.manual_seed(1)
        dec = Decode(groups, n_inp, sz["hidden"], sz["D"]).requires_grad_(False).set_compute_dtype("bf16").to(dev)
        for B in (1, 4):
            Bm = B * MEMBERS
            z = torch.randn(Bm, P, len(groups), sz["D"], device=dev)
            dense_obs = torch.randn(B, P, n_fields, n_inp, device=dev)
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

                    def fused():
                        return dec.sensor_sse(z, s, obs, precision=prec, members=MEMBERS, fused=True)

                    def composed():
                        return dec.sensor_sse(z, s, obs, precision=prec, members=MEMBERS, fused=False)

                    def dense():
                        return dec.member_sse(z, dense_obs, members=MEMBERS)

                    (tf, tc, td), spread = device_ms([fused, composed, dense], args.reps)
                    a, b = fused(), composed()
                    err = float((a - b).norm() / b.norm())
                    mem_f, mem_c, mem_d = extra_bytes(fused), extra_bytes(composed), extra_bytes(dense)
                    rec = dict(size=name, B=B, K=K, patches=q, K_pad=s.K_pad, fused_ms=tf, composed_ms=tc, dense_ms=td, spread_ms=spread, fused_extra_bytes=mem_f,
                               composed_extra_bytes=mem_c, dense_extra_bytes=mem_d, fused_vs_composed_rel_l2=err)
                    recs.append(rec)
                    emit(f"{name:<11}{B:>3}{K:>6}{q:>8}{s.K_pad:>7}{tf:>10.4f}{tc:>13.4f}{td:>10.4f}{tc / tf:>11.2f}{td / tf:>12.2f}{mem_f / 2**20:>10.2f}"
                         f"{mem_c / 2**20:>13.2f}{mem_d / 2**20:>10.2f}{err:>9.1e}")
                    flush()
                    if name == "cylinder" and B == 1 and K == 256 and n_obs == 32:
                        keep = dict(fused=lambda d=dec, z=z, s=s, o=obs, w=prec: d.sensor_sse(z, s, o, precision=w, members=MEMBERS, fused=True),
                                    composed=lambda d=dec, z=z, s=s, o=obs, w=prec: d.sensor_sse(z, s, o, precision=w, members=MEMBERS, fused=False),
                                    dense=lambda d=dec, z=z, t=dense_obs: d.member_sse(z, t, members=MEMBERS))
            del z, dense_obs
            torch.cuda.empty_cache()
    record["sensor_sse"] = recs
    emit(json.dumps(record))
    flush()
    if keep and not args.no_launch_count:
        counts = {k: count_launches(fn) for k, fn in keep.items()}
        emit("device launches of one call (cylinder, B = 1, K = 256 over 32 patches), by the profiler: "
             + ", ".join(f"{k} {'not available' if v is None else v}" for k, v in counts.items()))
        flush()


if __name__ == "__main__":
    main()
