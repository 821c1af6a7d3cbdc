"""The price of a condition-memo MISS: the bench's rollout step (cfg2, B = 1, T = 2024, bf16, plain replay) timed with the conditions left alone and with EVERY
condition changed before each step, in one process.  The script uses nothing the memo added, so the same file times the commit before the memo and the
commits after it: run it in both trees on one box and compare the `changing` figures (a memo build pays the stamp check and one 1 MB table write per field on
every step there; `constant` is the all-hit step).  Both loops issue the same in-place update of the condition tensor in front of every step (+ 0 or +- delta).
    python tools/cond_memo_miss_price.py [steps] [repeats]     -> one JSON line"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from sea_amd.models.temporal import TemporalModel


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    dev = torch.device("cuda:0")
    m = TemporalModel(1, 256, 8, 2024, 8, 0, 3, 2, 0.0, "sea", "learnable", "mlp", "add", 1, 1, True, "adaln")
    m.set_compute_dtype("bf16")
    m = m.to(dev).eval()
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(1, 2024, 3, 256, generator=g).to(dev)
    ib = torch.rand(1, 2024, 1, generator=g).to(dev)
    eng = m.engine(dev)

    def loop(delta):
        sign = 1.0
        for _ in range(20):
            eng.forward(x, ib)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            ib.add_(sign * delta)   # every condition of the step differs from the step before (delta = 0: none does)
            sign = -sign
            out = eng.forward(x, ib)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        return (time.perf_counter() - t0) / steps * 1e3

    res = {"constant": [], "changing": []}
    with torch.no_grad():
        for _ in range(repeats):   # alternately, so that a drift of the box shows in both
            res["constant"].append(round(loop(0.0), 5))
            res["changing"].append(round(loop(1e-3), 5))
    forms = eng.plan(1, 2024, "full").forms
    print(json.dumps({"ms_per_step": res, "steps": steps, "cond_memo": bool(getattr(forms, "cond_memo", False))}))


if __name__ == "__main__":
    main()
