"""Generate the decoded-field loss fixtures under tests/golden/ by RUNNING THE REFERENCE on CPU in fp64.

The reference's own Decode (models/encoder_decoder.py) and torch.nn.functional.mse_loss: loss = mse_loss(Decode(z), target) and dz = d loss / d z,
once with every column of a cell valid and once over the valid slots only (`counts[p]` leading columns of patch p: mse_loss over the selected
elements).  Inputs and weights are float32-representable and stored as float32; loss and dz as float64.  Each decode_mse_<shape>.npz stores:
meta (field groups flattened with -1 separators, n_inp, hidden, embed_dim, B, P), w1.<g>, w2.<g>, b2.<g>, z, target, counts, loss, dz, loss_masked,
dz_masked.  Runs only where the reference tree is present; the .npz files it writes are committed.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_decode_mse_fixtures.py
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
from torch.nn.functional import mse_loss

from models.encoder_decoder import Decode as RefDecode  # reference

# name: (field_groups, n_inp, MLP_hidden, embed_dim, B, P, counts, seed)
CASES = {
    "decode_mse_a": ([[0, 1], [2]], 12, 40, 16, 2, 9, [0, 1, 11, 12, 5, 12, 3, 7, 12], 21),
    "decode_mse_b": ([[0], [1], [2]], 37, 64, 8, 33, 4, [0, 1, 36, 37], 22),
}


def make(name, groups, n_inp, hidden, D, B, P, counts, seed):
    torch.manual_seed(seed)
    dec = RefDecode(groups, n_inp, hidden, D).float()
    with torch.no_grad():
        for p in dec.parameters():   # larger than the default init, so that the GELU is exercised away from 0
            p.mul_(2.0)
    dec = dec.double()               # float32-representable values, fp64 arithmetic
    F = sum(len(g) for g in groups)
    z = torch.randn(B, P, len(groups), D).double().requires_grad_(True)
    target = torch.randn(B, P, F, n_inp).double()
    cnt = torch.tensor(counts)
    valid = (torch.arange(n_inp) < cnt[:, None]).view(1, P, 1, n_inp).expand(B, P, F, n_inp)
    out = {}
    y = dec(z)
    loss = mse_loss(y, target)
    (dz,) = torch.autograd.grad(loss, z)
    out["loss"], out["dz"] = loss.detach().numpy(), dz.numpy()
    y = dec(z)
    loss_m = mse_loss(y[valid], target[valid])
    (dz_m,) = torch.autograd.grad(loss_m, z)
    out["loss_masked"], out["dz_masked"] = loss_m.detach().numpy(), dz_m.numpy()
    flat = []
    for g in groups:
        flat += list(g) + [-1]
    out["meta"] = np.array([n_inp, hidden, D, B, P] + flat, dtype=np.int64)
    out["z"], out["target"], out["counts"] = z.detach().float().numpy(), target.float().numpy(), cnt.numpy().astype(np.int32)
    for g, m in enumerate(dec.decoders):
        out[f"w1.{g}"] = m.layer1.weight.detach().float().numpy()
        out[f"w2.{g}"] = m.layer2.weight.detach().float().numpy()
        out[f"b2.{g}"] = m.layer2.bias.detach().float().numpy()
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, "loss", float(loss.detach()), "masked", float(loss_m.detach()), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    for name, case in CASES.items():
        make(name, *case)
