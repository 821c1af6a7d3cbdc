"""Rollouts from a multi-step context: prefill (the full-context forward over the k known states + the sea_kv_cache_fill launch), the decode's ms per
step next to the single-state (k = 1) figure, and the total against the recompute rollout from the same context.

    python tools/context_rollout_bench.py [--ks 1,64,399,1024] [--steps 100] [--widths cfg2,cylinder,multiphase] [--dtype bf16]

Widths: cfg2 (E = 256, H = 8, F = 3, adaln, sea_kv_rollout: B = 1 runs the persistent form), the shipped cylinder (E = 1024, F = 2, adaln) and
multiphase (E = 2048, F = 2, ln) widths (the generic step plan's few-row launches); one layer, max_len 2024, B = 1.  Prints one table row per (width, k)
and one JSON line at the end.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

WIDTHS = {"cfg2": (256, 3, "adaln"), "cylinder": (1024, 2, "adaln"), "multiphase": (2048, 2, "ln")}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    from sea_amd import kv_engine
    from sea_amd.models.temporal import TemporalModel
    from sea_amd.utils.train_utils import rollout

    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,64,399,1024")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--widths", default="cfg2,cylinder,multiphase")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-recompute", action="store_true", help="skip the recompute rollouts (the slow column)")
    a = ap.parse_args()
    ks, n = [int(v) for v in a.ks.split(",")], a.steps
    dev = torch.device("cuda:0")
    rows = []
    print(f"{'width':<11}{'k':>6}{'fwd ms':>9}{'fill ms':>9}{'dec ms/step':>13}{'k=1 ms/step':>13}{'total ms':>10}{'recompute ms':>14}")
    for wname in a.widths.split(","):
        E, F, ln = WIDTHS[wname]
        torch.manual_seed(42)
        model = TemporalModel(1, E, 8, 2024, 8, 0, F, 2, 0.0, "sea", "learnable", "mlp", "add", 1, 1, True, ln)
        model.set_compute_dtype(a.dtype)
        model = model.to(dev).eval()
        eng = model.engine(dev)
        g = torch.Generator().manual_seed(77)
        x = torch.randn(1, max(ks), F, E, generator=g).to(dev)
        ib = torch.rand(1, max(ks) + n, 1, generator=g).to(dev)
        base = None
        for k in ks:
            x0 = x[:, :k].contiguous()
            total = timed(lambda: rollout(model, x0, ib, n, mode="kv"), a.reps)
            fwd = fill = 0.0
            if k > 1:
                with torch.no_grad():
                    fwd = timed(lambda: eng.forward(x0, ib[:, :k]), a.reps)
                full = eng.plan(1, k, "full")
                fills = [cf for holder in ([eng._kv_fast[1]] if 1 in eng._kv_fast else []) + [p for p in eng._plans.values() if p.mode == "step"]
                         for key, cf in holder.__dict__.get("_fills", {}).items() if cf.full is full]
                fill = timed(fills[0].run, max(a.reps, 10)) if fills else float("nan")
            dec = (total - fwd - fill) / max(n - (k > 1), 1)
            if k == 1:
                base = total / n
            rec = float("nan") if a.no_recompute else timed(lambda: rollout(model, x0, ib, n, mode="recompute"), 1)
            row = dict(width=wname, E=E, F=F, ln=ln, k=k, steps=n, forward_ms=fwd, fill_ms=fill, decode_ms_per_step=dec,
                       k1_ms_per_step=base, total_ms=total, recompute_ms=rec, fast=kv_engine.supported(eng, 1))
            rows.append(row)
            print(f"{wname:<11}{k:>6}{fwd:>9.3f}{fill:>9.3f}{dec:>13.4f}{(base or float('nan')):>13.4f}{total:>10.2f}{rec:>14.1f}", flush=True)
        del model, eng
        torch.cuda.empty_cache()
    print(json.dumps({"context_rollout": rows, "dtype": a.dtype}))


if __name__ == "__main__":
    main()
