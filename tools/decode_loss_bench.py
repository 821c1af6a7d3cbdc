"""Loss on decoded fields + its latent gradient on the clock: Decode.mse_loss fused (sea_decode_mse) against composed (forward + sea_mse_fwd_bwd + two
data-gradient launches; with counts the masking runs in torch) at the two shipped decoder sizes — cylinder: hidden 480, D 16, T 399, batch_size 2;
multiphase: hidden 624, D 32, T 199, batch_size 4 — with P = 64 patches, three fields in groups [[0, 1], [2]] and the padded cell size of
`bench.py --mode decode` (the same synthetic wake-refined mesh).  Per size, B = 1 and the shipped batch_size, with every column valid and with the
mesh's per-cell counts:

    ms            median wall time of loss + backward to z over --reps repeats after a warm-up (device drained around every repeat)
    extra MB      peak of allocated memory above its value just before the call
    MFMA          fused only: 2 products x 2 M S (columns walked) / time, as a fraction of the 2.5 PFLOP/s dense bf16 peak
    target GB/s   fused only: bytes of the valid target rows read once / time

    python tools/decode_loss_bench.py [--reps 5] [--out profiles/decode_loss_bench.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SIZES = {"cylinder": dict(hidden=480, D=16, T=399, batch=2), "multiphase": dict(hidden=624, D=32, T=199, batch=4)}
BF16_PEAK = 2.5e15


def mesh(dev):
    """The partitioner of bench.py --mode decode: 30000 points, denser towards x = 0.3, 8 x 8 cells."""
    from sea_amd.utils.data_processors import DataPartitioner2D

    gen = torch.Generator().manual_seed(7)
    n_points = 30000
    px = torch.rand(n_points, generator=gen)
    px[: n_points // 3] = 0.25 + 0.1 * torch.rand(n_points // 3, generator=gen)
    py = torch.rand(n_points, generator=gen)
    part = DataPartitioner2D(px, py, m=9, n=9, device=dev)
    C_pad = part.padded_index_map.shape[1]
    counts = (part.padded_index_map != part.pad_id).sum(1).to(torch.int32)
    return (C_pad + 3) // 4 * 4, counts


def measure(dec, z, tgt, counts, fused, reps):
    def run():
        zz = z.detach().requires_grad_(True)
        loss = dec.mse_loss(zz, tgt, counts=counts, fused=fused)
        loss.backward()
        return loss

    run()
    times, peak = [], 0
    for _ in range(reps):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        t0 = time.perf_counter()
        loss = run()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        peak = max(peak, torch.cuda.max_memory_allocated() - before)
    return statistics.median(times), peak, float(loss.detach())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="cylinder,multiphase")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_loss_bench.py needs an MI355X: no GPU visible")
    from sea_amd.models.encoder_decoder import Decode

    dev = torch.device("cuda", 0)
    groups, P, n_fields = [[0, 1], [2]], 64, 3
    n_inp, counts = mesh(dev)
    lines, records = [], []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"decode_loss_bench: P = {P}, fields {groups}, n_inp = {n_inp} (valid cells per patch {int(counts.min())} .. {int(counts.max())}, "
         f"{float(counts.sum()) / (P * n_inp):.2f} of the slots), bf16, median of {args.reps}")
    emit(f"{'size':<11}{'B':>3}{'rows':>7} {'counts':<7}{'fused ms':>10}{'composed ms':>13}{'ratio':>7}{'fused MB':>10}{'composed MB':>13}{'MFMA':>7}{'target GB/s':>13}")
    for name in args.sizes.split(","):
        sz = SIZES[name]
        torch.manual_seed(1)
        dec = Decode(groups, n_inp, sz["hidden"], sz["D"]).requires_grad_(False).set_compute_dtype("bf16").to(dev)
        tiles = (n_inp + 31) // 32 * 32 * n_fields
        for B in sorted({1, sz["batch"]}):
            rows = B * sz["T"]
            M = rows * P
            z = torch.randn(rows, P, len(groups), sz["D"], device=dev)
            tgt = torch.randn(rows, P, n_fields, n_inp, device=dev)
            for cnt in (None, counts):
                ms_f, mem_f, l_f = measure(dec, z, tgt, cnt, True, args.reps)
                ms_c, mem_c, l_c = measure(dec, z, tgt, cnt, False, args.reps)
                flops = 2 * 2.0 * M * tiles * sz["hidden"]
                valid = n_fields * (n_inp * P if cnt is None else int(cnt.sum())) * rows
                rec = dict(size=name, B=B, rows=M, counts=cnt is not None, fused_ms=ms_f, composed_ms=ms_c, fused_extra_bytes=mem_f, composed_extra_bytes=mem_c,
                           mfma_fraction=flops / (ms_f * 1e-3) / BF16_PEAK, target_gbs=valid * 4 / (ms_f * 1e-3) / 1e9, loss_fused=l_f, loss_composed=l_c)
                records.append(rec)
                emit(f"{name:<11}{B:>3}{M:>7} {'mesh' if rec['counts'] else 'all':<7}{ms_f:>10.3f}{ms_c:>13.3f}{ms_c / ms_f:>7.2f}{mem_f / 2**20:>10.1f}{mem_c / 2**20:>13.1f}"
                     f"{rec['mfma_fraction']:>7.3f}{rec['target_gbs']:>13.1f}")
            del z, tgt
            torch.cuda.empty_cache()
    emit(json.dumps(dict(tool="decode_loss_bench", n_inp=n_inp, records=records)))
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
