"""The packed form of the CRPS loss launch without a device: sea_decode_member_crps_grad_packed's symbol, binding and argument checks (the unpacked entry
point's, under its own name), the shapes it carries as include/sea_hip.h documents them, the pack=None rule as a pure function, and the pack
argument's validation in Decode.member_crps_loss and EnsembleCRPSLoss."""
import ctypes as C
import os
import re

import pytest
import torch

from tests.test_crps_loss_cpu import BREAKS, _loss_args, _tables, lib  # noqa: F401  (lib: the module's fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_and_binding(lib):
    from sea_amd import _native as N

    assert hasattr(lib, "sea_decode_member_crps_grad_packed") and "sea_decode_member_crps_grad_packed" in N.EXPORTED_SYMBOLS
    assert lib.sea_decode_member_crps_grad_packed.restype is C.c_int and len(lib.sea_decode_member_crps_grad_packed.argtypes) == 5
    assert C.sizeof(N.SeaDecodeMemberCrpsGrad) == 152 and lib.sea_abi_version() == 8               # the same struct, an addition to the current ABI version
    assert N.CRPS_PACK_MAX_N == 32


@pytest.mark.parametrize("what", sorted(BREAKS) + ["bad dtype", "no groups", "group null dH", "group overlap", "lddh short"])
def test_packed_entry_refuses_bad_arguments_under_its_own_name(lib, what):
    """The unpacked entry point's checks and messages: every table it refuses is refused here with the same text after the entry point's name."""
    from sea_amd import _native as N

    def broken():
        arr, p = _tables()
        dt, ng = N.SEA_BF16, 2
        if what in BREAKS:
            setattr(p, *BREAKS[what])
        elif what == "bad dtype":
            dt = 5
        elif what == "no groups":
            ng = 0
        elif what == "group null dH":
            arr[0].dH = None
        elif what == "group overlap":
            arr[1].field0 = 1
        else:
            arr[1].lddh = 32
        return arr, ng, p, dt

    arr, ng, p, dt = broken()
    assert lib.sea_decode_member_crps_grad(arr, ng, C.byref(p), dt, None) == -1
    plain = lib.sea_last_error().decode()
    arr, ng, p, dt = broken()
    assert lib.sea_decode_member_crps_grad_packed(arr, ng, C.byref(p), dt, None) == -1, what
    packed = lib.sea_last_error().decode()
    assert packed.startswith("sea_decode_member_crps_grad_packed: ")
    assert packed == plain.replace("sea_decode_member_crps_grad: ", "sea_decode_member_crps_grad_packed: ", 1), (plain, packed)


def test_packed_entry_unsupported_shapes(lib):
    from sea_amd import _native as N, ops

    def widened(S, members):
        arr, p = _tables()
        p.S, p.members, p.M = S, members, 2 * members * 9
        for g in range(2):
            arr[g].ldh = arr[g].ldw = arr[g].lddh = arr[g].ldz = S
        return arr, p

    arr, p = _tables()
    assert lib.sea_decode_member_crps_grad_packed(arr, 2, C.byref(p), N.SEA_F32, None) == -3 and b"sea_decode_member_crps_grad_packed: unsupported: bf16 only" in lib.sea_last_error()
    arr, p = widened(648, 4)
    assert lib.sea_decode_member_crps_grad_packed(arr, 2, C.byref(p), N.SEA_BF16, None) == -3 and b"S=648 above 640" in lib.sea_last_error()
    arr, p = widened(40, 33)
    assert lib.sea_decode_member_crps_grad_packed(arr, 2, C.byref(p), N.SEA_BF16, None) == -3
    assert b"sea_decode_member_crps_grad_packed: unsupported: members=33 above 32" in lib.sea_last_error()
    assert lib.sea_decode_member_crps_grad_packed(None, 2, C.byref(p), N.SEA_BF16, None) == -1 and lib.sea_decode_member_crps_grad_packed(arr, 2, None, N.SEA_BF16, None) == -1
    arr, p = _tables()                                                                           # a short workspace: the unpacked form's size function is the packed form's
    p.work_bytes = 38015
    assert lib.sea_decode_member_crps_grad_packed(arr, 2, C.byref(p), N.SEA_BF16, None) == -1 and b"work_bytes=38015 below the 38016" in lib.sea_last_error()
    assert not ops.last_form()[0].startswith("decode.member_crps_grad.pk")                       # a refused call notes nothing


def test_supported_shapes_agree_with_the_header():
    """include/sea_hip.h: 1 .. 32 members at S up to 640; NP the member count rounded up to a power of two, at least 2; 64 / NP histories per workgroup,
    16 at NP = 2 above S = 512."""
    from sea_amd import ops

    text = open(os.path.join(ROOT, "include", "sea_hip.h")).read()
    doc = text[text.rindex("/* ---", 0, text.index("int sea_decode_member_crps_grad_packed(")):text.index("int sea_decode_member_crps_grad_packed(")]
    assert re.search(r"1 \.\. 32 members", doc) and "S above 640" in doc and "members above 32" in doc and "decode.member_crps_grad.pk" in doc
    assert "16 at NP = 2 above S = 512" in doc and "An addition to ABI version 8" in doc
    for S in (8, 40, 128, 136, 264, 384, 392, 512, 520, 640):
        for n in range(1, 33):
            assert ops.decode_member_crps_pack_supported(S, n), (S, n)
            NP, HG = ops.decode_member_crps_pack_shape(S, n)
            assert NP >= max(n, 2) and NP < 2 * max(n, 2) and NP & (NP - 1) == 0
            assert HG == (16 if NP == 2 and S > 512 else 64 // NP)
    for S, n in ((40, 0), (40, 33), (40, 64), (648, 4), (0, 4), (36, 4)):
        assert not ops.decode_member_crps_pack_supported(S, n), (S, n)
        with pytest.raises(ValueError, match="not carried"):
            ops.decode_member_crps_pack_shape(S, n)


def test_pack_rule_is_a_pure_function_of_the_shape():
    from sea_amd.models import encoder_decoder as ed

    rule = ed.crps_loss_pack_rule
    bf, f32 = torch.bfloat16, torch.float32
    assert ed.CRPS_LOSS_PACK_MEMBERS == (2, 32) and ed.CRPS_LOSS_PACK_MIN_PAIRS == 4096          # the measured member counts; 64 histories x 64 patches
    for n in (2, 3, 4, 8, 9, 16, 32):
        for hidden in (480, 624, 40):
            assert rule(n, 4096 * n, hidden, bf) is True and rule(n, 1 << 22, hidden, bf) is True   # the measured sizes and beyond
            assert rule(n, 4096 * n - 1, hidden, bf) is False and rule(n, 24, hidden, bf) is False  # below the measured row counts
            assert rule(n, 1 << 22, hidden, f32) is False                                           # fp32
        assert rule(n, 1 << 22, 648, bf) is False and rule(n, 1 << 22, 644, bf) is False            # widths the form does not carry
    for n in (0, 1, 33, 64, 65, 128):
        assert rule(n, 1 << 22, 480, bf) is False                                                # 1 member was not measured; above 32 the form does not exist
    assert rule(4, 1 << 20, 480, bf) is rule(4, 1 << 20, 480, bf)                                # no state


def test_pack_argument_validation():
    from sea_amd.utils.train_utils import EnsembleCRPSLoss

    dec, z, obs, P, F, C_ = _loss_args()
    with pytest.raises(ValueError, match="pack must be None, True or False"):
        dec.member_crps_loss(z, obs, 2, pack=1)
    with pytest.raises(ValueError, match="pack=True is a form of the fused launches"):
        dec.member_crps_loss(z, obs, 2, fused=False, pack=True)
    with pytest.raises(ValueError, match="bf16 only"):                                           # pack=True asks for the fused launches: an fp32 decoder raises as fused=True does
        dec.member_crps_loss(z, obs, 2, pack=True)
    dec.set_compute_dtype("bf16")
    big = torch.zeros(2 * 33, P, z.shape[2], z.shape[3])
    with pytest.raises(ValueError, match=r"the packed form carries 1 \.\. 32 members"):
        dec.member_crps_loss(big, obs, 33, pack=True)
    with pytest.raises(ValueError, match=r"the packed form carries 1 \.\. 32 members"):
        dec.member_crps_loss(big, obs, 33, fused=True, pack=True)
    for pack in (None, False):                                                                   # well-formed: past every check, to the device check
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            dec.member_crps_loss(big, obs, 33, pack=pack)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dec.member_crps_loss(z, obs, 2, pack=True)
    crit = EnsembleCRPSLoss(dec, P, 2, pack=True)
    assert crit.pack is True and EnsembleCRPSLoss(dec, P, 2).pack is None
    out = torch.zeros(2 * 2, 1, z.shape[2], P * z.shape[3])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(out, obs.view(2, 1, P, F, C_))
    with pytest.raises(ValueError, match=r"the packed form carries 1 \.\. 32 members"):
        EnsembleCRPSLoss(dec, P, 33, pack=True)(torch.zeros(33, 1, z.shape[2], P * z.shape[3]), obs[:1].view(1, 1, P, F, C_))
