"""Host validation of the attention entry points at head dims that are not powers of two (no GPU): every multiple of 8 in 8..256 passes the head-dim
check and reaches the per-problem checks, anything else is refused as an unsupported head dim."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from sea_amd import build, _native

    build.build(verbose=False)
    return _native.lib()


def fwd_params(hd, H=8):
    from sea_amd import _native as N

    P = N.SeaAttnParams()   # problem pointers stay null
    P.n_problems, P.B, P.H, P.hd, P.Tq, P.Tk, P.cap, P.q_pos0, P.src_len, P.ldo = 1, 2, H, hd, 16, 16, 16, 0, 0, H * hd
    return P


def bwd_params(hd, H=8):
    from sea_amd import _native as N

    P = N.SeaAttnBwdParams()
    P.n_problems, P.B, P.H, P.hd, P.Tq, P.Tk, P.cap, P.q_pos0, P.src_len = 1, 2, H, hd, 16, 16, 16, 0, 0
    P.ldo = P.lddo = P.lddq = P.lddk = P.lddv = H * hd
    P.q_scale = 1.0
    P.rope = 16   # any non-null address: validation fails on the problem pointers before anything is read
    return P


def call(lib, which, P, dtype):
    from sea_amd import _native as N

    fn = lib.sea_attention_fwd if which == "fwd" else lib.sea_attention_bwd
    rc = fn(C.byref(P), N.dtype_code(dtype), None)
    return rc, lib.sea_last_error().decode()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("hd", [24, 48, 96, 120, 200, 248])
def test_new_head_dims_reach_the_pointer_checks(lib, hd, dtype):
    import torch

    dt = torch.float32 if dtype == "fp32" else torch.bfloat16
    rc, msg = call(lib, "fwd", fwd_params(hd), dt)
    assert rc == -1 and "sea_attention_fwd[0]: null pointer" in msg, msg
    rc, msg = call(lib, "bwd", bwd_params(hd), dt)
    assert rc == -1 and "sea_attention_bwd[0]: null pointer" in msg, msg


@pytest.mark.parametrize("hd", [12, 4, 20, 264, 512])
def test_other_head_dims_are_refused(lib, hd):
    import torch

    for which, P in (("fwd", fwd_params(hd)), ("bwd", bwd_params(hd))):
        rc, msg = call(lib, which, P, torch.bfloat16)
        assert rc == -1 and f"unsupported head dim {hd}" in msg and "multiple of 8" in msg, msg
