"""Generate the input-gradient fixtures tests/golden/input_grad_*.npz by RUNNING THE REFERENCE on CPU in fp64 (as make_fixtures.py does, with its helpers).

d loss / d x and d loss / d condition of the reference's TemporalModel (weights from oracle/recipe.py on both sides):
  input_grad_adaln_mlp_add       AdaLN, info-bottleneck MLP added after the exchange; loss = MSE(model(x, ib), tgt)
  input_grad_fourier_attn_pre    Fourier info-bottleneck rows attended to, in front of the block; same loss
  input_grad_unroll3_adaln       a 3-step unrolled loss with growing windows T, T+1, T+2 (the evaluation loop's pattern, utils/train_utils.py:202-209):
                                 each step's last row is fed back and scored; the parameter gradients are stored too

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_input_grad_fixtures.py
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_fixtures as mf  # noqa: E402
import torch  # noqa: E402

from oracle.recipe import recipe_inputs  # noqa: E402
from oracle.sea_oracle import OracleConfig  # noqa: E402

CASES = {
    "input_grad_adaln_mlp_add": (OracleConfig(2, 64, 4, 24, 4, 0, 3, 2, True, "adaln"), 2, 7),
    "input_grad_fourier_attn_pre": (OracleConfig(1, 64, 4, 24, 4, 0, 2, 2, False, "adaln", "sea", "attention", "fourier"), 2, 7),
}
UNROLL = ("input_grad_unroll3_adaln", OracleConfig(1, 32, 2, 24, 4, 0, 2, 2, True, "adaln"), 2, 5, 3)


def unrolled_loss(model, x0, ib, tgt, n_steps):
    """sum over k of MSE(last row of model(window_k, ib[:, :T + k]), tgt[:, k]); window_{k+1} = [window_k | that row]."""
    T = x0.shape[1]
    inp, loss = x0, 0.0
    for k in range(n_steps):
        out = model(inp, ib[:, :T + k])
        nxt = out[:, -1:]
        loss = loss + ((nxt - tgt[:, k:k + 1]) ** 2).mean()
        inp = torch.cat([inp, nxt], dim=1)
    return loss


def main():
    for name, (cfg, B, T) in CASES.items():
        print(name)
        m = mf.build_reference(cfg).double().eval()
        x, tgt, ib = recipe_inputs(B, T, cfg, seed=7)
        xd, ibd = x.double().requires_grad_(True), ib.double().requires_grad_(True)
        loss = ((m(xd, ibd) - tgt.double()) ** 2).mean()
        dx, dib = torch.autograd.grad(loss, [xd, ibd])
        mf.save(name, cfg=mf.cfg_meta(cfg), x=mf.n(x), tgt=mf.n(tgt), ib=mf.n(ib), loss=mf.n(loss), dx=mf.n(dx), dib=mf.n(dib))
    name, cfg, B, T, K = UNROLL
    print(name)
    m = mf.build_reference(cfg).double().eval()
    x, _, ib = recipe_inputs(B, T + K, cfg, seed=11)
    _, tgt, _ = recipe_inputs(B, K, cfg, seed=12)
    x0 = x[:, :T].double().requires_grad_(True)
    ibd = ib.double().requires_grad_(True)
    loss = unrolled_loss(m, x0, ibd, tgt.double(), K)
    loss.backward()
    arrs = dict(cfg=mf.cfg_meta(cfg), x0=mf.n(x[:, :T]), ib=mf.n(ib), tgt=mf.n(tgt), steps=mf.np.array(K), loss=mf.n(loss), dx0=mf.n(x0.grad),
                dib=mf.n(ibd.grad))
    for k, p in m.named_parameters():
        if p.grad is not None:
            arrs["grad:" + k] = mf.n(p.grad)
    mf.save(name, **arrs)


if __name__ == "__main__":
    main()
