"""Generate the head-dim fixtures tests/golden/model_hd48_*.npz by RUNNING THE REFERENCE on CPU (as make_fixtures.py does, with its helpers).

A model of embed_dim 384 over 8 heads: self-attention head dim 48 and, with down_proj 2, cross-attention head dim 24 — widths that are not powers of
two.  Forward only, and a recompute rollout; weights come from oracle/recipe.py on both sides.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_headdim_fixtures.py
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_fixtures as mf  # noqa: E402
from oracle.sea_oracle import OracleConfig  # noqa: E402


def main():
    cfg = OracleConfig(1, 384, 8, 24, 2, 0, 3, 2, True, "adaln")
    mf.model_case("model_hd48_adaln_f3", cfg, 2, 16)
    mf.rollout_case("model_hd48_rollout6_adaln_f3", cfg, 2, 6)


if __name__ == "__main__":
    main()
