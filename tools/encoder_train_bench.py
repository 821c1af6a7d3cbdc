"""Spatial autoencoder training step (forward + backward + AdamW) at the shipped spatial configs, seeded synthetic data:
B = 128 snapshots, P = 81 patches, n_inp = 512 (as bench.py --mode encode), bf16 operands.  One JSON line per (config, form): ms per step from HIP
events over --steps timed steps after --warmup, and the libsea_hip launches per step (native_launches_per_step: the PyTorch fills and copies
of padding and gradient temporaries are not counted; a rocprofv3 --kernel-trace run counts every kernel).  Forms: "composed" (the default) and "fused"
(SEA_PLAN=enc=fused: sea_encoder_block_fwd / _bwd).

    python tools/encoder_train_bench.py [--steps 20] [--warmup 3] [--configs cylinder,multiphase]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from sea_amd.configs import cylinder_flow, multiphase_flow
from sea_amd.models.encoder_decoder import SpatialModel
from sea_amd.utils.train_utils import SeaMSELoss, initialize_optimizer

CONFIGS = {"cylinder": cylinder_flow.get_config_spatial, "multiphase": multiphase_flow.get_config_spatial}


def run(name, form, steps, warmup, B=128, P=81, n_inp=512):
    os.environ["SEA_PLAN"] = f"enc={form}"
    c = CONFIGS[name]()
    torch.manual_seed(0)
    m = SpatialModel(c["field_groups"], n_inp, c["MLP_hidden"], c["num_layers"], c["embed_dim"], c["n_heads"], P, 0, dropout=0.0)
    m = m.set_compute_dtype("bf16").to("cuda:0").train()
    F = sum(len(g) for g in c["field_groups"])
    x = torch.randn(B, P, F, n_inp, device="cuda:0")
    opt = initialize_optimizer(m, dict(learning_rate=1e-4))
    loss_fn = SeaMSELoss()

    def step():
        opt.zero_grad()
        xd = x.clone()
        loss = loss_fn(m(xd), xd)
        loss.backward()
        opt.step()
        return loss

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    eng = m.engine()
    n0 = eng.launches
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        loss = step()
    t1.record()
    torch.cuda.synchronize()
    # per step: the engine's forward / backward launches + MSE (1) + AdamW (1)
    launches = (eng.launches - n0) // steps + 2
    print(json.dumps(dict(tool="encoder_train_bench", config=name, form=form, B=B, P=P, n_inp=n_inp, dtype="bf16", width=c["embed_dim"] * len(c["field_groups"]),
                          steps=steps, ms_per_step=round(t0.elapsed_time(t1) / steps, 3), native_launches_per_step=launches, loss=float(loss.detach()))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="cylinder,multiphase")
    ap.add_argument("--forms", default="composed,fused")
    a = ap.parse_args()
    for n in a.configs.split(","):
        for f in a.forms.split(","):
            run(n, f, a.steps, a.warmup)
