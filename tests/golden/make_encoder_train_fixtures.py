"""Generate the spatial-autoencoder training fixtures under tests/golden/ by RUNNING THE REFERENCE on CPU.

The reference's own SpatialModel in train() mode (dropout 0), nn.MSELoss against the masked input, one loss.backward(), then
three torch.optim.AdamW steps at lr 1e-3 from the initial parameters.  Both cases have -9999 entries in the input and an n_inp that
is not a multiple of 32.  Each .npz stores: x (input as given, -9999 included), x_masked, meta, init.<name>, grad.<name>, loss,
after3.<name>.  Runs only where the reference tree is present; the .npz files it writes are committed.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_encoder_train_fixtures.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
# the reference tree: $SEA_REFERENCE, else a `reference` directory beside the repository
REF = os.environ.get("SEA_REFERENCE", os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(HERE))), "reference"))
sys.path.insert(0, REF)

import numpy as np
import torch

from models.encoder_decoder import SpatialModel as RefSpatialModel  # reference

# name: (field_groups, n_inp, MLP_hidden, num_layers, embed_dim, n_heads, B, P, seed)
CASES = {
    "encoder_train_cyl_small": ([[0, 1], [2]], 20, 48, 2, 16, 8, 3, 9, 11),      # W = 32, 8 heads of 4 (padded to 8 inside)
    "encoder_train_three_groups": ([[0], [1, 2], [3]], 12, 40, 1, 16, 6, 2, 10, 12),   # W = 48, 6 heads of 8
}
LR, STEPS = 1e-3, 3


def make(name, groups, n_inp, hidden, layers, E, H, B, P, seed):
    torch.manual_seed(seed)
    m = RefSpatialModel(groups, n_inp, hidden, layers, E, H, max_len=P, src_len=0, dropout=0.0, variational=False).double()
    with torch.no_grad():   # non-trivial LayerNorm parameters and biases (the reference initialises them to 1 / 0)
        for k, p in m.named_parameters():
            if k.endswith("bias") or "ln" in k or "layers.1" in k:
                p.add_(0.1 * torch.randn_like(p))
    m.train()
    F = sum(len(g) for g in groups)
    x = torch.randn(B, P, F, n_inp, dtype=torch.float64)
    x[torch.rand_like(x) < 0.1] = -9999.0
    x_given = x.clone()
    init = {k: p.detach().clone() for k, p in m.named_parameters()}
    loss_fn = torch.nn.MSELoss()
    out = m(x)                     # masks x in place, as the reference's train loop relies on
    loss = loss_fn(out, x)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    x_masked = x.detach().clone()
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(init[k])
    opt = torch.optim.AdamW(m.parameters(), lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    for _ in range(STEPS):
        opt.zero_grad()
        xs = x_given.clone()
        o = m(xs)
        loss_fn(o, xs).backward()
        opt.step()
    arrs = dict(x=x_given.float().numpy(), x_masked=x_masked.float().numpy(), loss=np.array(float(loss.detach()), dtype=np.float64),
                meta=np.array([n_inp, hidden, layers, E, H, B, P], dtype=np.int64), lr=np.array(LR), steps=np.array(STEPS),
                field_groups=np.array([gi for gi, g in enumerate(groups) for _ in g], dtype=np.int64))
    for k in init:
        arrs["init." + k] = init[k].float().numpy()
        arrs["grad." + k] = grads[k].float().numpy()
        arrs["after3." + k] = m.state_dict()[k].float().numpy()
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrs)
    print(f"wrote {path}: loss {float(loss):.6f}, {len(init)} parameters")


if __name__ == "__main__":
    for n, c in CASES.items():
        make(n, *c)
