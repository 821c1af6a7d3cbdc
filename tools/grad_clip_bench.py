"""Gradient clipping / non-finite skipping on the clock (sea_grad_norm_ctl + sea_adamw_flat_ctl against sea_adamw_flat), at the live parameter
count of three models: cfg3 (bench.py --mode train: E 256, B 8, T 2024) and the two shipped temporal configurations at their own size (cylinder:
E 1024, batch 2, T 399, dropout 0.1; multiphase: E 2048, batch 4, T 199).  Per model:

    norm us        sea_grad_norm_ctl, both launches      }  device events around --calls back-to-back calls on one stream (so launch gaps are
    adamw_ctl us   sea_adamw_flat_ctl                    }  in), median of --reps windows after a warm-up window; the three are interleaved
    adamw us       sea_adamw_flat                        }  window by window
    norm GB/s      4 n bytes / norm time;  adamw GB/s: 30 n bytes (p, g, m, v read; p, m, v, bf16 shadow written) / adamw time.  The buffers of
                   the smaller models fit the 256 MB Infinity Cache: their rates are cache rates, not HBM rates
    step ms        engine.train_step with the feature off / max_grad_norm / max_grad_norm + skip_nonfinite: host clock around --steps steps ending
                   in a synchronise, median of --reps windows, the three optimizers interleaved window by window on one model

    python tools/grad_clip_bench.py [--reps 5] [--calls 200] [--steps 10] [--out profiles/grad_clip_bench.txt]
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


def models(dev, names):
    """(name, model, (x, tgt, ib), learning rate) one at a time: bf16, seed 42, synthetic inputs of the model's own shape."""
    import bench
    from sea_amd.configs import get_config
    from sea_amd.models.temporal import TemporalModel

    for name in names:
        torch.manual_seed(42)
        if name == "cfg3":
            c = bench.CFG
            m, B, T, F, E, lr = bench.build_model(dev, "bf16"), 8, c["max_len"], c["F"], c["E"], 1e-4
        else:
            c = get_config(name, "temporal")
            B, T, F, E, lr = c["batch_size"], c["dataset_src_len"], c["num_fields"], c["embed_dim"], c["learning_rate"]
            m = TemporalModel(c["num_layers"], E, c["n_heads"], c["block_size"], c["scale_ratio"], c["src_len"], F, c["down_proj"], c["dropout"],
                              c["exchange_mode"], c["pos_encoding_mode"], c["ib_scale_mode"], c["ib_addition_mode"], c["ib_mlp_layers"], c["ib_num"],
                              c["add_info_after_cross"], c["LN_type"])
            m.set_compute_dtype("bf16")
            m = m.to(dev)
        yield name, m.train(), bench.inputs(B, T, F, E, 0, dev), lr
        del m
        torch.cuda.empty_cache()


def kernel_times(n, dev, calls, reps):
    """Median microseconds per call of the three entry points over buffers of n floats."""
    from sea_amd import _native as N

    L, s = N.lib(), N.stream_ptr()
    p, m, v = (torch.randn(n, device=dev).abs_() * 1e-2 for _ in range(3))
    g = torch.randn(n, device=dev) * 1e-2
    shadow = torch.empty(n, device=dev, dtype=torch.bfloat16)
    partial = torch.empty(1024, device=dev, dtype=torch.float64)
    ctl = torch.zeros(N.CTL_WORDS, device=dev, dtype=torch.int32)
    P = lambda t: t.data_ptr()   # noqa: E731
    fns = {
        "norm": lambda: L.sea_grad_norm_ctl(P(g), n, 1.0, 1.0, 1, 0.9, 0.999, P(partial), 1024, P(ctl), s),
        "adamw_ctl": lambda: L.sea_adamw_flat_ctl(P(p), P(g), P(m), P(v), P(shadow), N.SEA_BF16, n, 1e-4, 0.9, 0.999, 1e-8, 0.0, 1.0, P(ctl), s),
        "adamw": lambda: L.sea_adamw_flat(P(p), P(g), P(m), P(v), P(shadow), N.SEA_BF16, n, 1e-4, 0.9, 0.999, 1e-8, 0.0, 7, 1.0, s),
    }
    times = {k: [] for k in fns}
    for rep in range(reps + 1):   # window 0 warms up
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                N.check(fn(), k)
            b.record()
            b.synchronize()
            if rep:
                times[k].append(a.elapsed_time(b) * 1e3 / calls)
    assert int(ctl[N.CTL_APPLIED]) == 1 and torch.isfinite(p).all()
    return {k: statistics.median(t) for k, t in times.items()}


def step_times(model, data, lr, steps, reps):
    """Median milliseconds per engine.train_step with the feature off, clipping, clipping + skipping."""
    from sea_amd.utils.train_utils import initialize_optimizer

    eng = model.engine()
    x, tgt, ib = data
    opts = {"off": initialize_optimizer(model, {"learning_rate": lr}),
            "clip": initialize_optimizer(model, {"learning_rate": lr, "max_grad_norm": 1.0}),
            "clip+skip": initialize_optimizer(model, {"learning_rate": lr, "max_grad_norm": 1.0, "skip_nonfinite_steps": True})}
    times = {k: [] for k in opts}
    for rep in range(reps + 1):   # window 0 warms up
        for k, opt in opts.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                loss = eng.train_step(x, tgt, ib, opt)
            torch.cuda.synchronize()
            if rep:
                times[k].append((time.perf_counter() - t0) / steps * 1e3)
    assert torch.isfinite(loss).all()
    stats = opts["clip+skip"].step_stats()
    return {k: statistics.median(t) for k, t in times.items()}, {k: (min(t), max(t)) for k, t in times.items()}, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--models", default="cfg3,cylinder_flow,multiphase_flow")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grad_clip_bench.py needs an MI355X: no GPU visible")
    dev = torch.device("cuda", 0)
    lines, records = [], []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"grad_clip_bench: bf16, kernels: median of {args.reps} windows of {args.calls} back-to-back calls (device events); "
         f"train_step: median [min .. max] of {args.reps} windows of {args.steps} steps (host clock, synchronised)")
    emit(f"{'model':<16}{'n_live':>11}{'norm us':>9}{'adamw_ctl us':>14}{'adamw us':>10}{'norm GB/s':>11}{'adamw GB/s':>12}"
         f"{'step off ms':>26}{'clip ms':>26}{'clip+skip ms':>26}{'clip cost':>11}")
    for name, model, data, lr in models(dev, args.models.split(",")):
        n = model.engine().params.n_live
        kt = kernel_times(n, dev, args.calls, args.reps)
        st, spread, stats = step_times(model, data, lr, args.steps, args.reps)
        rec = dict(model=name, n_live=n, norm_us=kt["norm"], adamw_ctl_us=kt["adamw_ctl"], adamw_us=kt["adamw"], norm_gbs=4.0 * n / kt["norm"] / 1e3,
                   adamw_gbs=30.0 * n / kt["adamw"] / 1e3, step_ms=st, step_ms_min_max=spread, last_step_stats=stats)
        records.append(rec)
        cell = lambda k: f"{st[k]:.3f} [{spread[k][0]:.3f} .. {spread[k][1]:.3f}]"   # noqa: E731
        emit(f"{name:<16}{n:>11}{kt['norm']:>9.2f}{kt['adamw_ctl']:>14.2f}{kt['adamw']:>10.2f}{rec['norm_gbs']:>11.0f}{rec['adamw_gbs']:>12.0f}"
             f"{cell('off'):>26}{cell('clip'):>26}{cell('clip+skip'):>26}{(st['clip'] / st['off'] - 1) * 100:>10.2f}%")
    emit(json.dumps(dict(tool="grad_clip_bench", records=records)))
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
