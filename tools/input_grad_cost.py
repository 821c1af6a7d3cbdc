"""Cost of the input gradients: the cfg3-shaped backward (BASELINE.json configs[2]: B = 8, T = 2024, bf16) of the ordinary training plan against the plan
that also writes d loss / d x and d loss / d condition (engine.train_plan(..., want_dx=True, want_dc=True)).  Prints one JSON line.

    python tools/input_grad_cost.py [--iters 20]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from oracle.recipe import recipe_inputs, recipe_params  # noqa: E402
from oracle.sea_oracle import OracleConfig  # noqa: E402
from sea_amd.models.temporal import TemporalModel  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dtype", default="bf16")
    args = ap.parse_args()
    cfg = OracleConfig(1, 256, 8, 2024, 8, 0, 3, 2, True, "adaln")
    B, T = 8, 2024
    m = TemporalModel(cfg.num_layers, cfg.embed_dim, cfg.n_heads, cfg.max_len, cfg.scale_ratio, cfg.src_len, cfg.num_variables, cfg.down_proj, 0.0,
                      "sea", "learnable", "mlp", "add", 1, 1, True, "adaln")
    p = recipe_params(cfg)
    with torch.no_grad():
        for k, prm in m.named_parameters():
            prm.copy_(p[k])
    m.set_compute_dtype(args.dtype)
    m = m.to("cuda:0").train()
    x, tgt, ib = (t.cuda() for t in recipe_inputs(B, T, cfg, seed=1))
    eng = m.engine()
    res = {"config": "cfg3", "B": B, "T": T, "dtype": args.dtype}
    for label, want in (("params_only", False), ("with_dx_dc", True)):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        out, plan = eng.forward_train(x, ib, want, want)
        torch.cuda.synchronize()
        res[label + "_plan_workspace_gb"] = round((torch.cuda.memory_allocated() - before) / 1e9, 3)   # the first plan includes the engine's flat buffers
        _, dout = eng.mse_loss_and_grad(out, tgt)
        dx = torch.empty_like(x) if want else None
        dc = torch.zeros(B * T, device=x.device) if want else None
        times = []
        for i in range(args.iters + 3):
            if dc is not None:
                dc.zero_()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.backward(plan, dout, dx=dx, dc=dc)
            b.record()
            torch.cuda.synchronize()
            if i >= 3:
                times.append(a.elapsed_time(b))
        times.sort()
        res[label + "_ms_median"] = round(times[len(times) // 2], 3)
        res[label + "_ms_min"] = round(times[0], 3)
        res[label + "_launches"] = len(plan.bwd)
    res["extra_ms_median"] = round(res["with_dx_dc_ms_median"] - res["params_only_ms_median"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
