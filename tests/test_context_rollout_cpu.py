"""CPU side of the rollout from a multi-step context: the limits are refused before anything runs, the fill entry point validates its table without a
GPU, and the fp64 oracle reproduces the reference's own loop from a context (tests/golden/context_rollout_*.npz)."""
import ctypes as C

import pytest
import torch

from oracle import sea_oracle as O
from oracle.recipe import recipe_params
from tests.conftest import cfg_from_meta, load_golden, rel_l2


def _model():
    from sea_amd.models.temporal import TemporalModel

    return TemporalModel(1, 64, 4, 24, 8, 0, 2, 2, 0.0, "sea", "learnable", "mlp", "add", 1, 1, True, "adaln")


@pytest.mark.parametrize("mode", ["kv", "recompute"])
def test_context_limits_raise_value_error(mode):
    from sea_amd.utils.train_utils import rollout

    m = _model()
    x, ib = torch.zeros(2, 24, 2, 64), torch.zeros(2, 24, 1)
    with pytest.raises(ValueError, match="max_len"):
        rollout(m, x[:, :10], ib, 16, mode=mode)          # k + n - 1 = 25 > 24
    with pytest.raises(ValueError, match="too short"):
        rollout(m, x[:, :10], ib[:, :13], 5, mode=mode)   # needs 14 conditions
    with pytest.raises(ValueError, match="k >= 1"):
        rollout(m, x[:, :0], ib, 3, mode=mode)
    with pytest.raises(RuntimeError, match="no CPU"):     # inside the limits (k + n - 1 = max_len): on to the device path, which refuses CPU tensors
        rollout(m, x[:, :10], ib, 15, mode=mode)


def test_cache_fill_validates_without_gpu():
    from sea_amd import build, _native as N

    build.build(verbose=False)
    L = N.lib()
    arr = (N.SeaKvFill * 2)()
    assert L.sea_kv_cache_fill(arr, 1, N.SEA_BF16, None) == -1 and b"null" in L.sea_last_error()
    assert L.sea_kv_cache_fill(None, 1, N.SEA_BF16, None) == -1
    assert L.sea_kv_cache_fill(arr, 0, N.SEA_BF16, None) == -1
    assert C.sizeof(N.SeaKvFill) == 64 and N.KV_FILL_MAX == 32


@pytest.mark.parametrize("name", ["context_rollout_adaln_f3", "context_rollout_ln_f2"])
def test_oracle_reproduces_reference_context_rollout(name):
    g = load_golden(name)
    cfg = cfg_from_meta(g["cfg"])
    p = {k: v.double() for k, v in recipe_params(cfg).items()}
    x, ib, n = torch.from_numpy(g["x"]).double(), torch.from_numpy(g["ib"]).double(), int(g["steps"])
    for k in [int(v) for v in g["ks"]]:
        a = x[:, :k]
        with torch.no_grad():
            for i in range(n):
                out = O.model_forward(a, ib[:, :k + i], p, cfg)
                a = torch.cat((a, out[:, -1:]), dim=1)
        assert rel_l2(a[:, k:].numpy(), g[f"pred_k{k}"]) < 1e-6, k
