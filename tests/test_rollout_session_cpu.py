"""CPU side of the rollout session (sea_amd/rollout_session.py, utils/train_utils.py open_rollout): sea_kv_cache_fork is exported, its struct layout
matches, every host-side refusal returns -1 with its message, and the argument checks of open_rollout raise before the device guard."""
import ctypes as C

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from sea_amd import build, _native

    build.build(verbose=False)
    return _native.lib()


def _model(*tail):
    from sea_amd.models.temporal import TemporalModel

    args = [1, 64, 4, 24, 8, 0, 2, 2, 0.0, "sea", "learnable", "mlp", "add", 1, 1, True, "adaln"]
    for i, v in tail:
        args[i] = v
    return TemporalModel(*args)


def test_fork_symbol_and_struct(lib):
    from sea_amd import _native as N

    assert hasattr(lib, "sea_kv_cache_fork") and "sea_kv_cache_fork" in N.EXPORTED_SYMBOLS
    assert N.ABI_STRUCTS[-1] is N.SeaKvFork and N.ABI_STRUCTS[-2] is N.SeaKvFill
    out = (C.c_int * 48)()
    n = lib.sea_struct_sizes(out, 48)
    assert n == len(N.ABI_STRUCTS) and out[n - 1] == C.sizeof(N.SeaKvFork) == 48
    assert N.KV_FORK_MAX == 32 and lib.sea_abi_version() == 8


def _entry(arr, **over):
    e = arr[0]
    e.src, e.dst = 0x1000, 0x2000       # never dereferenced: every call below is refused on the host
    e.B_src, e.H, e.hd, e.n_pos, e.cap_src, e.cap_dst, e.n_rep, e.transposed = 2, 3, 16, 5, 8, 16, 4, 0
    for k, v in over.items():
        setattr(e, k, v)


def test_fork_refusals_without_gpu(lib):
    from sea_amd import _native as N

    arr = (N.SeaKvFork * 2)()
    assert lib.sea_kv_cache_fork(None, 1, N.SEA_BF16, None) == -1 and b"sea_kv_cache_fork: bad arguments" in lib.sea_last_error()
    assert lib.sea_kv_cache_fork(arr, 0, N.SEA_BF16, None) == -1 and b"bad arguments" in lib.sea_last_error()
    _entry(arr)
    assert lib.sea_kv_cache_fork(arr, 1, 7, None) == -1 and b"bad dtype 7" in lib.sea_last_error()
    for over in (dict(src=None), dict(dst=None)):
        _entry(arr, **over)
        assert lib.sea_kv_cache_fork(arr, 1, N.SEA_F32, None) == -1 and b"entry 0: null or misaligned" in lib.sea_last_error(), over
    for over in (dict(src=0x1004), dict(dst=0x2008)):
        _entry(arr, **over)
        assert lib.sea_kv_cache_fork(arr, 1, N.SEA_BF16, None) == -1 and b"entry 0: null or misaligned" in lib.sea_last_error(), over
    for over in (dict(B_src=0), dict(H=0), dict(hd=12), dict(hd=0), dict(hd=264), dict(n_pos=0), dict(n_pos=9), dict(n_pos=17, cap_src=24), dict(cap_src=12),
                 dict(cap_dst=20), dict(n_rep=0), dict(n_rep=-1), dict(transposed=2)):
        _entry(arr, **over)
        assert lib.sea_kv_cache_fork(arr, 1, N.SEA_BF16, None) == -1, over
        assert b"sea_kv_cache_fork: entry 0: bad sizes" in lib.sea_last_error(), over
    # the message names the entry that is wrong
    _entry(arr)
    arr[1].src, arr[1].dst = 0x1000, None
    assert lib.sea_kv_cache_fork(arr, 2, N.SEA_F32, None) == -1 and b"entry 1: null" in lib.sea_last_error()
    # more workgroups than a launch grid holds
    _entry(arr, B_src=1 << 20, H=1 << 10, n_rep=1, hd=256, n_pos=8192, cap_src=8192, cap_dst=8192)
    assert lib.sea_kv_cache_fork(arr, 1, N.SEA_F32, None) == -1 and b"workgroups" in lib.sea_last_error()


def test_open_rollout_checks_arguments_before_the_device_guard():
    from sea_amd.utils.train_utils import open_rollout

    m = _model()
    x, ib = torch.zeros(2, 24, 2, 64), torch.zeros(2, 24, 1)
    with pytest.raises(ValueError, match="k >= 1"):
        open_rollout(m, x[:, :0], ib[:, :0])
    with pytest.raises(ValueError, match=r"k - 1 = 4"):
        open_rollout(m, x[:, :5], ib[:, :5])                 # one condition too many: the newest state's arrives with the step
    with pytest.raises(ValueError, match=r"k - 1 = 4"):
        open_rollout(m, x[:, :5], ib[:, :3])
    with pytest.raises(ValueError, match=r"k - 1 = 4"):
        open_rollout(m, x[:, :5], ib[:, :4, 0])              # [B, k-1] is not [B, k-1, 1]
    with pytest.raises(ValueError, match=r"k - 1 = 4"):
        open_rollout(m, x[:, :5], ib[:1, :4])                # another batch size
    with pytest.raises(ValueError, match=r"F=2, E=64"):
        open_rollout(m, x[:, :5, :1], ib[:, :4])
    with pytest.raises(ValueError, match=r"F=2, E=64"):
        open_rollout(m, x[:, 0], ib[:, :0])
    with pytest.raises(ValueError, match="max_len"):
        open_rollout(m, torch.zeros(2, 25, 2, 64), torch.zeros(2, 24, 1))
    with pytest.raises(RuntimeError, match="CPU"):           # a well-formed history: on to the device path, which refuses a CPU model
        open_rollout(m, x[:, :5], ib[:, :4])
    with pytest.raises(RuntimeError, match="CPU"):
        open_rollout(m, x[:, :1], ib[:, :0])


@pytest.mark.parametrize("tail,match", [
    (((5, 2),), "exact only for src_len == 0"),
    (((9, "pool"),), "does not cover exchange_mode='pool'"),
    (((12, "attention"),), "does not cover ib_addition_mode='attention'"),
])
def test_open_rollout_refuses_models_without_an_exact_cache(tail, match):
    from sea_amd.utils.train_utils import open_rollout

    m = _model(*tail)
    with pytest.raises(NotImplementedError, match=match):
        open_rollout(m, torch.zeros(2, 5, 2, 64), torch.zeros(2, 4, 1))
