"""Ensemble weighting and resampling on the clock (sea_amd/ensemble.py, Decode.member_sse, sea_resample_systematic):

  (a) ms per Decode.member_sse — fused (sea_decode_member_sse, with 128 and with 64 rows per workgroup: SEA_TUNE sse_rows) against composed (forward() +
      torch reductions over its [rows, n_fields * Cp] fp32 output) — at the two decoder sizes of tools/decode_loss_bench.py (cylinder: hidden 480, D 16;
      multiphase: hidden 624, D 32; P = 64 patches, fields [[0, 1], [2]], the same synthetic wake-refined mesh), 64 members per history, B = 1 and 4
      histories, every column valid and with the mesh's per-cell counts; beside each the peak of allocated memory above its value before the call.
      Device time: windows of back-to-back calls between two events, at least 20 ms each, the three forms alternating inside every repeat.
      MFMA: 2 M S (columns walked) / fused time as a fraction of the 2.5 PFLOP/s dense bf16 peak (the first-layer launch is inside the time);
  (b) us per sea_resample_systematic (ops.resample_systematic, 4 histories) at n = 64 and 4096 members against the same steps written in eager torch
      (fp64, cumsum + searchsorted, the ESS decision read back on the host as a hand-written loop does) — host clock around a drained batch of calls;
  (c) one observation cycle at the cylinder width (one layer, E = 1024, F = 2, history of 64 states, one history forked into 64 members):
      step -> FieldLikelihood -> systematic_resample -> resample — with the fused scoring launch (fused=True) and with the default rule (fused=None: the
      composed scoring below 8192 rows) — against step -> decoder forward + reductions -> eager resampling -> resample, alternating, host clock,
      drained around every batch of cycles.

  (m) --moments (this leg alone): ms per Decode.member_moments — fused (sea_decode_member_moments) against composed (forward() + torch reductions:
      mean, then centred squares) — at the sizes, members and meshes of (a), equal weights, with the peak of allocated memory above its value
      before the call and the fused launch's MFMA fraction over the column tiles it walks (with counts: ceil(count / 32) tiles per patch).

    python tools/ensemble_bench.py [--reps 7] [--out profiles/ensemble_bench.txt]
    python tools/ensemble_bench.py --moments [--out profiles/ensemble_moments_bench.txt]
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

from tools.decode_loss_bench import BF16_PEAK, SIZES, mesh  # noqa: E402

MEMBERS = 64


def set_rows(rows):
    """sea_decode_member_sse reads SEA_TUNE per call: the two forms are measured in one process."""
    if rows is None:
        os.environ.pop("SEA_TUNE", None)
    else:
        os.environ["SEA_TUNE"] = f"sse_rows={rows}"


def device_ms(fns, reps, min_ms=20.0):
    """Median device time in ms of one call of each fn: per repeat one window (a batch of back-to-back calls between two events, sized to last at
    least min_ms) for every fn in turn, so that the forms alternate."""
    batches = []
    for fn in fns:
        fn()
        torch.cuda.synchronize()
        batch = 4
        while True:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(batch):
                fn()
            e1.record()
            e1.synchronize()
            if e0.elapsed_time(e1) >= min_ms or batch >= 1 << 12:
                break
            batch *= 2
        batches.append(batch)
    out = [[] for _ in fns]
    for _ in range(reps):
        for i, (fn, batch) in enumerate(zip(fns, batches)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(batch):
                fn()
            e1.record()
            e1.synchronize()
            out[i].append(e0.elapsed_time(e1) / batch)
    return [statistics.median(v) for v in out], [(min(v), max(v)) for v in out]


def extra_bytes(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def host_us(fns, reps, batch):
    """Median host-clock time in us of one call of each fn, a drained batch per window, the fns alternating."""
    out = [[] for _ in fns]
    for r in range(reps + 1):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(batch):
                fn()
            torch.cuda.synchronize()
            if r:
                out[i].append((time.perf_counter() - t0) * 1e6 / batch)
    return [statistics.median(v) for v in out]


def eager_resample(logw, u, n, ess_frac):
    """sea_resample_systematic written with torch ops, as a user would today: fp64, and the ESS decision taken on the host."""
    lw = logw.view(-1, n).double()
    G = lw.shape[0]
    live = torch.isfinite(lw)
    mx = torch.where(live, lw, torch.full_like(lw, -float("inf"))).max(1, keepdim=True).values
    w = torch.where(live, (lw - mx).exp(), torch.zeros_like(lw))
    c = w.cumsum(1)
    W = c[:, -1:]
    ess = (W * W).squeeze(1) / (w * w).sum(1)
    ident = torch.arange(G * n, device=lw.device).view(G, n)
    do = ess < ess_frac * n if ess_frac >= 0 else torch.ones(G, dtype=torch.bool, device=lw.device)
    if not bool(do.any()):                                            # the host round trip
        return ident.reshape(-1).int(), (lw - mx - W.log()).float().reshape(-1), ess.float(), do.int()
    thr = (torch.arange(n, device=lw.device).double() + u.double().view(G, 1)) / n * W
    pick = torch.searchsorted(c, thr, right=True).clamp_max(n - 1)
    index = torch.where(do.view(G, 1), pick + torch.arange(G, device=lw.device).view(G, 1) * n, ident)
    out = torch.where(do.view(G, 1), torch.zeros_like(lw), lw - mx - W.log())
    return index.reshape(-1).int(), out.float().reshape(-1), ess.float(), do.int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="cylinder,multiphase")
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--moments", action="store_true", help="measure Decode.member_moments (leg m) instead of the legs of --parts")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_bench.py needs an MI355X: no GPU visible")
    from sea_amd import ops
    from sea_amd.ensemble import FieldLikelihood, systematic_resample
    from sea_amd.models.encoder_decoder import Decode

    dev = torch.device("cuda", 0)
    groups, P, n_fields = [[0, 1], [2]], 64, 3
    n_inp, counts = mesh(dev)
    lines, record = [], dict(tool="ensemble_bench", n_inp=n_inp, members=MEMBERS)

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    parts = ["m"] if args.moments else args.parts.split(",")
    if "m" in parts:
        emit(f"ensemble_bench (m): Decode.member_moments, {MEMBERS} members per history, P = {P}, fields {groups}, n_inp = {n_inp} (valid cells per patch "
             f"{int(counts.min())} .. {int(counts.max())}, {float(counts.sum()) / (P * n_inp):.2f} of the slots), bf16, equal weights, device time, median of {args.reps} windows")
        emit(f"{'size':<11}{'B':>3}{'rows':>7} {'counts':<7}{'fused ms':>10}{'composed ms':>13}{'comp/fused':>11}{'fused MB':>10}{'composed MB':>13}{'MFMA':>7}{'rel mean':>10}{'rel var':>10}")
        recs = []
        for name in args.sizes.split(","):
            sz = SIZES[name]
            torch.manual_seed(1)
            dec = Decode(groups, n_inp, sz["hidden"], sz["D"]).requires_grad_(False).set_compute_dtype("bf16").to(dev)
            for B in (1, 4):
                Bm = B * MEMBERS
                M = Bm * P
                z = torch.randn(Bm, P, len(groups), sz["D"], device=dev)
                for cnt in (None, counts):
                    def fused():
                        return dec.member_moments(z, MEMBERS, counts=cnt, fused=True)

                    def composed():
                        return dec.member_moments(z, MEMBERS, counts=cnt, fused=False)

                    (tf, tc), spread = device_ms([fused, composed], args.reps)
                    a, b = fused(), composed()
                    err_m, err_v = float((a[0] - b[0]).norm() / b[0].norm()), float((a[1] - b[1]).norm() / b[1].norm())
                    mem_f, mem_c = extra_bytes(fused), extra_bytes(composed)
                    walked = (n_inp + 31) // 32 * 32 if cnt is None else float(((cnt.clamp(0, n_inp) + 31) // 32 * 32).float().mean())
                    rec = dict(size=name, B=B, rows=M, counts=cnt is not None, fused_ms=tf, composed_ms=tc, spread_ms=spread, fused_extra_bytes=mem_f,
                               composed_extra_bytes=mem_c, mfma_fraction=2.0 * M * walked * n_fields * sz["hidden"] / (tf * 1e-3) / BF16_PEAK,
                               fused_vs_composed_rel_l2_mean=err_m, fused_vs_composed_rel_l2_var=err_v)
                    recs.append(rec)
                    emit(f"{name:<11}{B:>3}{M:>7} {'mesh' if rec['counts'] else 'all':<7}{tf:>10.4f}{tc:>13.4f}{tc / tf:>11.2f}{mem_f / 2**20:>10.2f}{mem_c / 2**20:>13.2f}"
                         f"{rec['mfma_fraction']:>7.3f}{err_m:>10.1e}{err_v:>10.1e}")
                del z
                torch.cuda.empty_cache()
        record["member_moments"] = recs
    if "a" in parts:
        emit(f"ensemble_bench (a): Decode.member_sse, {MEMBERS} members per history, P = {P}, fields {groups}, n_inp = {n_inp} (valid cells per patch "
             f"{int(counts.min())} .. {int(counts.max())}, {float(counts.sum()) / (P * n_inp):.2f} of the slots), bf16, device time, median of {args.reps} windows")
        emit(f"{'size':<11}{'B':>3}{'rows':>7} {'counts':<7}{'fused128 ms':>12}{'fused64 ms':>12}{'composed ms':>13}{'comp/f128':>10}{'fused MB':>10}{'composed MB':>13}{'MFMA':>7}")
        recs = []
        for name in args.sizes.split(","):
            sz = SIZES[name]
            torch.manual_seed(1)
            dec = Decode(groups, n_inp, sz["hidden"], sz["D"]).requires_grad_(False).set_compute_dtype("bf16").to(dev)
            cols = (n_inp + 31) // 32 * 32 * n_fields
            for B in (1, 4):
                Bm = B * MEMBERS
                M = Bm * P
                z = torch.randn(Bm, P, len(groups), sz["D"], device=dev)
                obs = torch.randn(B, P, n_fields, n_inp, device=dev)
                for cnt in (None, counts):
                    def fused(rows):
                        def run():
                            set_rows(rows)
                            return dec.member_sse(z, obs, counts=cnt, members=MEMBERS, fused=True)
                        return run

                    def composed():
                        return dec.member_sse(z, obs, counts=cnt, members=MEMBERS, fused=False)

                    (f128, f64, comp), spread = device_ms([fused(128), fused(64), composed], args.reps)
                    a, b = fused(128)(), composed()
                    err = float((a - b).norm() / b.norm())
                    mem_f, mem_c = extra_bytes(fused(128)), extra_bytes(composed)
                    set_rows(None)
                    rec = dict(size=name, B=B, rows=M, counts=cnt is not None, fused128_ms=f128, fused64_ms=f64, composed_ms=comp, spread_ms=spread,
                               fused_extra_bytes=mem_f, composed_extra_bytes=mem_c, mfma_fraction=2.0 * M * cols * sz["hidden"] / (f128 * 1e-3) / BF16_PEAK,
                               fused_vs_composed_rel_l2=err)
                    recs.append(rec)
                    emit(f"{name:<11}{B:>3}{M:>7} {'mesh' if rec['counts'] else 'all':<7}{f128:>12.4f}{f64:>12.4f}{comp:>13.4f}{comp / f128:>10.2f}{mem_f / 2**20:>10.2f}"
                         f"{mem_c / 2**20:>13.2f}{rec['mfma_fraction']:>7.3f}")
                del z, obs
                torch.cuda.empty_cache()
        record["member_sse"] = recs

    if "b" in parts:
        emit("ensemble_bench (b): sea_resample_systematic against eager torch (fp64, host ESS decision), 4 histories, ess threshold 0.5, host clock over drained batches of 50")
        recs = []
        for n in (64, 4096):
            g = torch.Generator().manual_seed(n)
            logw = (3 * torch.randn(4 * n, generator=g)).to(dev)
            u = torch.rand(4, generator=g).to(dev)
            native, eager = host_us([lambda: ops.resample_systematic(logw, u, n, 0.5), lambda: eager_resample(logw, u, n, 0.5)], args.reps, 50)
            dev_ms, _ = device_ms([lambda: ops.resample_systematic(logw, u, n, 0.5)], args.reps, min_ms=5.0)
            same = bool(torch.equal(ops.resample_systematic(logw, u, n, 0.5)[0], eager_resample(logw, u, n, 0.5)[0]))
            recs.append(dict(n=n, native_us=native, eager_us=eager, native_device_us=dev_ms[0] * 1e3, same_index=same))
            emit(f"n = {n:>5}: native {native:8.1f} us per call (device time {dev_ms[0] * 1e3:.1f} us)   eager {eager:8.1f} us   ratio {eager / native:.1f}   same index: {same}")
        record["resample"] = recs

    if "c" in parts:
        from sea_amd.models.temporal import TemporalModel
        from sea_amd.utils.train_utils import open_rollout

        sz = SIZES["cylinder"]
        E, F, k = P * sz["D"], len(groups), 64
        torch.manual_seed(42)
        model = TemporalModel(1, E, 8, 2024, 8, 0, F, 2, 0.0, "sea", "learnable", "mlp", "add", 1, 1, True, "adaln")
        model.set_compute_dtype("bf16")
        model = model.to(dev).eval()
        torch.manual_seed(1)
        dec = Decode(groups, n_inp, sz["hidden"], sz["D"]).requires_grad_(False).set_compute_dtype("bf16").to(dev)
        g = torch.Generator().manual_seed(77)
        x = (0.5 * torch.randn(1, k, F, E, generator=g)).to(dev)
        ib = torch.rand(1, k, 1, generator=g).to(dev)
        obs = torch.randn(1, P, n_fields, n_inp, generator=g).to(dev)
        src = open_rollout(model, x, ib[:, :k - 1].contiguous())
        ens_n, ens_e = src.fork(MEMBERS), src.fork(MEMBERS)
        like = FieldLikelihood(dec, P, MEMBERS, counts=counts, sigma=10.0, fused=True)                 # the fused launch at any size
        like_default = FieldLikelihood(dec, P, MEMBERS, counts=counts, sigma=10.0)                    # fused=None: the composed path below 8192 rows
        ens_d = src.fork(MEMBERS)
        cond = torch.rand(MEMBERS, 1, generator=g).to(dev)
        valid = (torch.arange(n_inp, device=dev) < counts[:, None]).view(1, P, 1, n_inp)

        def native_cycle():
            y = ens_n.step(cond)
            index, _, _, _ = systematic_resample(like(y, obs), MEMBERS)
            ens_n.resample(index)

        def default_cycle():
            y = ens_d.step(cond)
            index, _, _, _ = systematic_resample(like_default(y, obs), MEMBERS)
            ens_d.resample(index)

        def eager_cycle():
            y = ens_e.step(cond)
            zz = y.reshape(MEMBERS, F, P, sz["D"]).permute(0, 2, 1, 3)
            d = torch.where(valid, dec(zz) - obs, torch.zeros((), device=dev))
            logw = -0.5 * (d * d).sum(dim=(1, 2, 3)) / 100.0
            index, _, _, _ = eager_resample(logw, torch.rand(1, device=dev), MEMBERS, -1.0)
            ens_e.resample(index)

        native, default, eager = host_us([native_cycle, default_cycle, eager_cycle], args.reps, 4)
        record["cycle"] = dict(width="cylinder", E=E, F=F, k=k, members=MEMBERS, rows=MEMBERS * P, forked_by=ens_n.forked_by, fused_ms=native / 1e3,
                               default_ms=default / 1e3, eager_ms=eager / 1e3)
        emit(f"ensemble_bench (c): observation cycle at the cylinder width (E = {E}, F = {F}, {MEMBERS} members from a history of {k}, fork by {ens_n.forked_by}, "
             f"{MEMBERS * P} rows, mesh counts): step + FieldLikelihood + systematic_resample + resample with FieldLikelihood(fused=True) {native / 1e3:.3f} ms, with "
             f"fused=None ({'fused' if MEMBERS * P >= 8192 else 'composed'} scoring at this size) {default / 1e3:.3f} ms   hand-written eager weighting and resampling "
             f"{eager / 1e3:.3f} ms   eager / fused {eager / native:.2f}")
        for s in (ens_n, ens_d, ens_e, src):
            s.close()

    emit(json.dumps(record))
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
