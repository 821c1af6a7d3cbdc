"""CRPS, rank and spread verification of a DERIVED field on the clock (DerivedVerification: sea_decode_derived_verify behind the decoder's first layer):

  ms of one call at the cylinder's decoder size of tools/decode_loss_bench.py (hidden 480, D 16; P = 64 patches, fields [[0, 1], [2]], the same synthetic
  mesh with its counts, n_inp 1628), 64 and 128 members per history, B = 1 and 4 histories, bf16, log-weights given, ONE derived field — the speed
  sqrt(u^2 + v^2) of fields 0 and 1 — verified against a snapshot of the source fields, with all five maps and without maps:
    fused      fused=True: the two launches of sea_decode_derived_verify; neither the members' decoded fields nor the derived field are written
    composed   fused=False: Decode.forward plus _composed_derived plus the fp64 formulas (_composed_field_verify)
    member     FieldVerification (fused) on the same states: all THREE decoded fields; "/3" is that time per field — the yardstick: a derived field
               should cost about one field of the member call plus one more decode per tile
  beside each the peak of allocated memory above its value before the call, and (once) the number of device launches of one call as the profiler
  counts them.  Device time: windows of back-to-back calls between two events, at least 20 ms each, the forms alternating inside every repeat
  (tools/ensemble_bench.device_ms).

    python tools/derived_verify_bench.py [--reps 5] [--out profiles/derived_verify_bench.txt]
    python tools/derived_verify_bench.py --errors [--out profiles/derived_verify_gpu_errors.txt]     the errors the GPU tests print
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


def errors(out):
    """Run tests/test_derived_verify_gpu.py and keep the lines in which its tests print their errors."""
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_derived_verify_gpu.py"), "-q", "-s", "-m", "gpu"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    keep = [l.lstrip(".") for l in r.stdout.splitlines() if re.match(r"^\.*derived verify ", l)]
    tail = [l for l in r.stdout.splitlines()[-3:] if "passed" in l or "failed" in l]
    text = "\n".join(["derived_verify_bench --errors: what tests/test_derived_verify_gpu.py printed (python -m pytest tests/test_derived_verify_gpu.py -q -s -m gpu)"]
                     + keep + tail) + "\n"
    print(text, end="")
    if out:
        with open(os.path.join(ROOT, out) if not os.path.isabs(out) else out, "w") as f:
            f.write(text)
    if r.returncode:
        print(r.stdout[-6000:])
    return r.returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--members", default="64,128")
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--errors", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("derived_verify_bench.py needs an MI355X: no GPU visible")
    if args.errors:
        raise SystemExit(errors(args.out))
    from sea_amd.ensemble import FIELD_MAPS, DerivedField, DerivedVerification, FieldVerification
    from sea_amd.models.encoder_decoder import Decode

    dev = torch.device("cuda", 0)
    groups, P, F = [[0, 1], [2]], 64, 3
    n_inp, counts = mesh(dev)
    counts = counts[:P].contiguous()
    sz = SIZES["cylinder"]
    lines, record = [], dict(tool="derived_verify_bench", n_inp=n_inp)

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out:
            with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"derived_verify_bench: one derived field (the speed of fields 0 and 1), cylinder decoder (hidden {sz['hidden']}, D {sz['D']}), P = {P}, fields {groups}, "
         f"n_inp = {n_inp}, the mesh's counts ({int(counts.sum())} cells per field and history), bf16, log-weights given, observed='fields', device time in ms, median of "
         f"{args.reps} windows; rows = B * members * P; maps: all five per-cell maps; sums: maps=(); member: FieldVerification on all three decoded fields (/3: per "
         f"field); MB: peak memory above the level before the call; fields MB: the members' decoded fields in fp32, which the fused calls never hold")
    emit(f"{'N':>4}{'B':>3}{'rows':>7}{'what':>6}{'fused':>9}{'composed':>10}{'comp/fused':>11}{'member':>9}{'member/3':>9}{'fused/(m/3)':>12}{'fused MB':>10}{'comp MB':>10}"
         f"{'fields MB':>10}")
    torch.manual_seed(1)
    dec = Decode(groups, n_inp, sz["hidden"], sz["D"]).requires_grad_(False).set_compute_dtype("bf16").to(dev)
    speed = [DerivedField("magnitude", 0, 1, 1.5, -0.25, 1.5, 0.1, name="speed")]
    recs, launches = [], None
    for n in (int(v) for v in args.members.split(",")):
        for B in (1, 4):
            Bm = B * n
            g = torch.Generator().manual_seed(64 + B + n)
            y = torch.randn(Bm, len(groups), P * sz["D"], device=dev).to(torch.bfloat16)
            obs = torch.randn(B, P, F, n_inp, generator=g).to(dev)
            logw = torch.randn(Bm, generator=g).to(dev)
            f_, c_ = (DerivedVerification(dec, P, n, speed, counts=counts, sigma=0.5, fused=fu) for fu in (True, False))
            m_ = FieldVerification(dec, P, n, counts=counts, sigma=0.5, fused=True)
            forms = {what: tuple((lambda o=o, mp=mp: o(y, obs, None, logw, maps=mp)) for o in (f_, c_, m_)) for what, mp in (("maps", FIELD_MAPS), ("sums", ()))}
            fields_mb = Bm * P * F * n_inp * 4 / 2**20
            for what, fns in forms.items():
                ms, spread = device_ms(list(fns), args.reps)
                mem = [extra_bytes(fn) for fn in fns[:2]]
                recs.append(dict(members=n, B=B, rows=Bm * P, what=what, fused_ms=ms[0], composed_ms=ms[1], member_three_fields_ms=ms[2], spread_ms=spread,
                                 fused_extra_bytes=mem[0], composed_extra_bytes=mem[1], decoded_fields_bytes=Bm * P * F * n_inp * 4))
                emit(f"{n:>4}{B:>3}{Bm * P:>7}{what:>6}{ms[0]:>9.4f}{ms[1]:>10.4f}{ms[1] / ms[0]:>11.2f}{ms[2]:>9.4f}{ms[2] / 3:>9.4f}{ms[0] / (ms[2] / 3):>12.2f}"
                     f"{mem[0] / 2**20:>10.2f}{mem[1] / 2**20:>10.2f}{fields_mb:>10.2f}")
                flush()
                if B == 1 and n == 64 and not args.no_launch_count:
                    launches = launches or {}
                    launches.update({f"{what} {k}": count_launches(fn) for k, fn in zip(("fused", "composed", "member"), fns)})
            del y, obs, logw, forms
            torch.cuda.empty_cache()
    record["rows"] = recs
    if launches is not None:
        record["launches"] = launches
        emit("device launches of one call (64 members, B = 1; the decoder's first layer included), by the profiler: "
             + "; ".join(f"{k}: {'not available' if v is None else v}" for k, v in launches.items()))
    emit(json.dumps(record))
    flush()


if __name__ == "__main__":
    main()
