"""The condition-gradient entry points (sea_silu_outer_bwd_dc, sea_ib_bwd_dc) refuse bad arguments with -1 before anything is launched, so these
checks run without a GPU."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from sea_amd import build, _native

    build.build(verbose=False)
    return _native.lib()


FAKE = 1 << 40   # a 16-byte aligned address that is never dereferenced: every call below is refused first


def _silu_groups(n, K2=64):
    from sea_amd import _native as N

    g = (N.SeaSiluBwdGroup * n)()
    for x in g:
        x.dHid = x.w1 = x.b1 = x.dw1 = x.db1 = FAKE
        x.K2, x.ld = K2, K2
    return g


def test_silu_outer_bwd_dc_refuses_bad_arguments(lib):
    g = _silu_groups(1)
    M = 3
    need = lib.sea_silu_outer_bwd_dc_ws_floats(g, 1, M)
    assert need == 1 * M + 2 * 64
    assert lib.sea_silu_outer_bwd_dc(g, 1, FAKE, None, M, 0, FAKE, need, None) == -1 and b"sea_silu_outer_bwd_dc" in lib.sea_last_error()  # null dc
    assert lib.sea_silu_outer_bwd_dc(g, 1, None, FAKE, M, 0, FAKE, need, None) == -1                                                   # null c
    assert lib.sea_silu_outer_bwd_dc(g, 1, FAKE, FAKE, M, 0, None, need, None) == -1                                                   # null workspace
    assert lib.sea_silu_outer_bwd_dc(g, 1, FAKE, FAKE, 0, 0, FAKE, need, None) == -1                                                   # M = 0
    assert lib.sea_silu_outer_bwd_dc(g, 1, FAKE, FAKE, M, 7, FAKE, need, None) == -1 and b"dtype" in lib.sea_last_error()
    assert lib.sea_silu_outer_bwd_dc(g, 1, FAKE, FAKE, M, 0, FAKE, need - 1, None) == -1 and b"workspace" in lib.sea_last_error()
    many = _silu_groups(25)
    assert lib.sea_silu_outer_bwd_dc(many, 25, FAKE, FAKE, M, 0, FAKE, 1 << 30, None) == -1                                            # > one launch's groups
    assert lib.sea_silu_outer_bwd_dc_ws_floats(many, 25, M) == -1
    for K2 in (2, 6, 4096):                                                                                                          # K2 % 4, > 2048
        bad = _silu_groups(1, K2)
        assert lib.sea_silu_outer_bwd_dc(bad, 1, FAKE, FAKE, M, 0, FAKE, 1 << 30, None) == -1 and b"bad group" in lib.sea_last_error()
    mis = _silu_groups(1)
    mis[0].w1 = FAKE + 4
    assert lib.sea_silu_outer_bwd_dc(mis, 1, FAKE, FAKE, M, 0, FAKE, 1 << 30, None) == -1 and b"aligned" in lib.sea_last_error()
    nodw = _silu_groups(1)
    nodw[0].dw1 = None
    assert lib.sea_silu_outer_bwd_dc(nodw, 1, FAKE, FAKE, M, 0, FAKE, 1 << 30, None) == -1


def _ib(mode, E=64, h=4, fields=1):
    from sea_amd import _native as N

    P = N.SeaIbBwdParams()
    for f in range(fields):
        P.dX[f] = FAKE
    P.n_fields, P.ldx, P.M, P.E, P.h, P.mode = fields, E, 5, E, h, mode
    P.c = P.w1 = P.b1 = P.lnw = P.lnb = P.w2 = FAKE
    return P


def test_ib_bwd_dc_refuses_bad_arguments(lib):
    assert lib.sea_ib_bwd_dc(None, FAKE, None) == -1 and b"sea_ib_bwd_dc" in lib.sea_last_error()
    assert lib.sea_ib_bwd_dc(C.byref(_ib(0)), None, None) == -1                     # null dc
    assert lib.sea_ib_bwd_dc(C.byref(_ib(3)), FAKE, None) == -1 and b"mode" in lib.sea_last_error()
    for bad in (dict(n_fields=0), dict(n_fields=9), dict(M=0), dict(ldx=32), dict(c=None), dict(w1=None)):
        P = _ib(1)
        for k, v in bad.items():
            setattr(P, k, v)
        assert lib.sea_ib_bwd_dc(C.byref(P), FAKE, None) == -1, bad
    P = _ib(1, fields=2)
    P.dX[1] = None
    assert lib.sea_ib_bwd_dc(C.byref(P), FAKE, None) == -1 and b"dX[1]" in lib.sea_last_error()
    for bad in (dict(h=0), dict(h=65), dict(E=6, ldx=6), dict(w2=None), dict(lnw=None)):   # 'mlp': h <= 64, E % 4, its parameters
        P = _ib(0)
        for k, v in bad.items():
            setattr(P, k, v)
        assert lib.sea_ib_bwd_dc(C.byref(P), FAKE, None) == -1, bad
    P = _ib(0)
    P.dX[0] = FAKE + 4
    assert lib.sea_ib_bwd_dc(C.byref(P), FAKE, None) == -1 and b"misaligned" in lib.sea_last_error()
    P = _ib(2, E=63, h=0)
    assert lib.sea_ib_bwd_dc(C.byref(P), FAKE, None) == -1 and b"fourier" in lib.sea_last_error()   # [sin | cos]: E even
    P = _ib(2, h=0)
    P.dw1 = FAKE                                                                                   # the Fourier matrix is fixed: no gradient
    assert lib.sea_ib_bwd_dc(C.byref(P), FAKE, None) == -1
    for mode in (1, 2):                                                                            # dropout is on the 'mlp' output only
        P = _ib(mode, h=0)
        P.drop.thr = 26
        assert lib.sea_ib_bwd_dc(C.byref(P), FAKE, None) == -1 and b"dropout" in lib.sea_last_error()
    P = _ib(1)
    P.dw1 = FAKE                                                                                   # parameter gradients asked for: sea_ib_bwd's checks (db1)
    assert lib.sea_ib_bwd_dc(C.byref(P), FAKE, None) == -1 and b"sea_ib_bwd" in lib.sea_last_error()

