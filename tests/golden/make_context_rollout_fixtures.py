"""Generate the context-rollout fixtures tests/golden/context_rollout_*.npz by RUNNING THE REFERENCE on CPU in fp64 (as make_fixtures.py does, with its
helpers): the reference's TemporalModel in the reference's own evaluation loop (utils/train_utils.py:202-209), started from the first k states of a
trajectory instead of one: a = data[:, :k]; out = model(a, ib[:, :k + i]); a = cat(a, out[:, -1:]).

  context_rollout_adaln_f3   cfg2-structured (AdaLN, info-bottleneck after the exchange, F = 3), small widths, k in {3, 9}
  context_rollout_ln_f2      multiphase-structured (LayerNorm, F = 2), small widths, k in {3, 9}

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_context_rollout_fixtures.py
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
    "context_rollout_adaln_f3": (OracleConfig(1, 64, 4, 40, 8, 0, 3, 2, True, "adaln"), 2, 12),
    "context_rollout_ln_f2": (OracleConfig(1, 64, 4, 40, 4, 0, 2, 2, True, "ln"), 2, 12),
}
KS = (3, 9)


def main():
    for name, (cfg, B, n) in CASES.items():
        print(name)
        m = mf.build_reference(cfg).double().eval()
        x, _, ib = recipe_inputs(B, max(KS) + n, cfg, seed=21)
        arrs = dict(cfg=mf.cfg_meta(cfg), x=mf.n(x), ib=mf.n(ib), steps=mf.np.array(n), ks=mf.np.array(KS))
        with torch.no_grad():
            for k in KS:
                a = x[:, :k].double()
                for i in range(n):
                    out = m(a, ib[:, :k + i].double())
                    a = torch.cat((a, out[:, -1:]), dim=1)
                arrs[f"pred_k{k}"] = mf.n(a[:, k:].float())
        mf.save(name, **arrs)


if __name__ == "__main__":
    main()
