"""ctypes binding of libsea_hip.so (C ABI: include/sea_hip.h).

The library is the product's only compute path: if it is missing or cannot be loaded, every operator raises —
there is no CPU or eager-PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch  # imported first so that the HIP runtime torch ships is the one the library binds to

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libsea_hip.so")

SEA_F32, SEA_BF16 = 0, 1
ABI_VERSION = 8   # include/sea_hip.h SEA_ABI_VERSION
MAX_GROUPS = 16
# the step control block of sea_grad_norm_ctl / sea_adamw_flat_ctl (include/sea_hip.h, SEA_CTL_*): word indices
CTL_GRAD_NORM, CTL_CLIP, CTL_INV_BC1, CTL_INV_SQRT_BC2, CTL_APPLIED, CTL_STEP, CTL_SKIPPED, CTL_CLIPPED, CTL_WORDS = range(9)
MAX_ATTN_PROBLEMS = 8
MAX_NORM_GROUPS = 16
MAX_SILU_GROUPS = 24

_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float


class SeaDropout(C.Structure):
    _fields_ = [("seed", C.c_uint32), ("stream", C.c_uint32), ("thr", _i32), ("mode", _i32)]


class SeaGemmGroup(C.Structure):
    _fields_ = [("A", _vp), ("W", _vp), ("bias", _vp), ("R", _vp), ("C32", _vp), ("Cact", _vp), ("Z", _vp),
                ("a_seg_stride", _i64),
                ("lda", _i32), ("ldw", _i32), ("ldr", _i32), ("ldc32", _i32), ("ldcact", _i32), ("ldz", _i32),
                ("M", _i32), ("N", _i32), ("K", _i32), ("n_seg", _i32),
                ("act", _i32), ("bias_scale", _f32), ("drop", SeaDropout),
                ("silu_c", _vp), ("silu_w1", _vp), ("silu_b1", _vp)]


class SeaQkvGroup(C.Structure):
    _fields_ = [("A", _vp), ("W", _vp), ("bias", _vp), ("Qout", _vp), ("Kout", _vp), ("Vtout", _vp), ("Vout", _vp),
                ("lda", _i32), ("ldw", _i32), ("M", _i32), ("N", _i32), ("K", _i32), ("col0", _i32)]


class SeaQkvCommon(C.Structure):
    _fields_ = [("rope", _vp), ("H", _i32), ("hd", _i32), ("T", _i32), ("pos0", _i32), ("cap", _i32), ("q_scale", _f32)]


class SeaAttnProblem(C.Structure):
    _fields_ = [("Q", _vp), ("K", _vp), ("Vt", _vp), ("O", _vp), ("LSE", _vp)]


class SeaAttnParams(C.Structure):
    _fields_ = [("p", SeaAttnProblem * MAX_ATTN_PROBLEMS), ("n_problems", _i32),
                ("B", _i32), ("H", _i32), ("hd", _i32), ("Tq", _i32), ("Tk", _i32), ("cap", _i32),
                ("q_pos0", _i32), ("src_len", _i32), ("ldo", _i32), ("drop", SeaDropout)]


class SeaNormGroup(C.Structure):
    _fields_ = [("X", _vp), ("mod", _vp), ("gamma", _vp), ("beta", _vp), ("Y32", _vp), ("Yact", _vp),
                ("mean", _vp), ("rstd", _vp),
                ("ldx", _i32), ("ldmod", _i32), ("ldy32", _i32), ("ldyact", _i32),
                ("addend", _vp), ("Xout", _vp), ("ldadd", _i32), ("ldxout", _i32)]


class SeaSiluGroup(C.Structure):
    _fields_ = [("w1", _vp), ("b1", _vp), ("Hid", _vp), ("K2", _i32), ("ld", _i32)]


class SeaIbParams(C.Structure):
    _fields_ = [("X", _vp * 8), ("n_fields", _i32), ("ldx", _i32),
                ("c", _vp), ("w1", _vp), ("b1", _vp), ("lnw", _vp), ("lnb", _vp), ("w2", _vp), ("b2", _vp),
                ("M", _i32), ("E", _i32), ("h", _i32), ("drop", SeaDropout), ("mode", _i32), ("pad_", _i32)]


class SeaWgradGroup(C.Structure):
    _fields_ = [("dY", _vp), ("X", _vp), ("dW", _vp), ("db", _vp), ("lddy", _i32), ("ldx", _i32), ("lddw", _i32),
                ("M", _i32), ("N", _i32), ("K", _i32), ("overwrite", _i32), ("pad_", _i32)]


class SeaNormBwdGroup(C.Structure):
    _fields_ = [("dY", _vp), ("X", _vp), ("mod", _vp), ("gamma", _vp), ("beta", _vp), ("mean", _vp), ("rstd", _vp),
                ("dX32", _vp), ("dXact", _vp), ("dmod", _vp), ("dgamma", _vp), ("dbeta", _vp),
                ("lddy", _i32), ("ldx", _i32), ("ldmod", _i32), ("lddx32", _i32), ("lddxact", _i32), ("lddmod", _i32)]


class SeaSiluBwdGroup(C.Structure):
    _fields_ = [("dHid", _vp), ("w1", _vp), ("b1", _vp), ("dw1", _vp), ("db1", _vp), ("K2", _i32), ("ld", _i32)]


class SeaIbBwdParams(C.Structure):
    _fields_ = [("dX", _vp * 8), ("n_fields", _i32), ("ldx", _i32),
                ("c", _vp), ("w1", _vp), ("b1", _vp), ("lnw", _vp), ("lnb", _vp), ("w2", _vp),
                ("dw1", _vp), ("db1", _vp), ("dlnw", _vp), ("dlnb", _vp), ("dw2", _vp), ("db2", _vp),
                ("M", _i32), ("E", _i32), ("h", _i32), ("drop", SeaDropout), ("mode", _i32), ("pad_", _i32),
                ("ws", _vp), ("ws_floats", _i64), ("dhid", _vp)]


class SeaAttnBwdProblem(C.Structure):
    _fields_ = [("Q", _vp), ("K", _vp), ("V", _vp), ("O", _vp), ("dO", _vp), ("LSE", _vp), ("delta", _vp), ("dQ", _vp), ("dK", _vp),
                ("dV", _vp)]


class SeaAttnBwdParams(C.Structure):
    _fields_ = [("p", SeaAttnBwdProblem * MAX_ATTN_PROBLEMS), ("rope", _vp), ("n_problems", _i32),
                ("B", _i32), ("H", _i32), ("hd", _i32), ("Tq", _i32), ("Tk", _i32), ("cap", _i32), ("q_pos0", _i32), ("src_len", _i32),
                ("ldo", _i32), ("lddo", _i32), ("lddq", _i32), ("lddk", _i32), ("lddv", _i32), ("q_scale", _f32), ("drop", SeaDropout)]


OP_GEMM, OP_QKV, OP_ATTN, OP_NORM, OP_SILU, OP_IB, OP_CONVERT, OP_GEMM_NORM, OP_XTAIL, OP_MLP1, OP_MLP2, OP_GEMM_FEW, OP_QKV_FEW, OP_CHAIN, OP_ADALN, OP_MLPB, OP_AQKV, OP_SPLITK = 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18, 19, 20
FEW_MAX_GROUPS = 8     # sea_gemm_fewrows / sea_qkv_rope_fewrows (gemv.hip)
FEW_K = (512, 1024, 2048, 4096, 8192, 16384)


class SeaLaunchRec(C.Structure):
    _fields_ = [("op", _i32), ("n", _i32), ("dtype", _i32), ("i0", _i32), ("i1", _i32), ("i2", _i32), ("i3", _i32), ("f0", _f32),
                ("p0", _vp), ("p1", _vp), ("l0", _i64), ("l1", _i64), ("l2", _i64), ("l3", _i64)]

MAX_GEMM_NORM_GROUPS = 8


class SeaGemmNormGroup(C.Structure):
    _fields_ = [("A", _vp), ("W", _vp), ("bias", _vp), ("R", _vp), ("C32", _vp), ("mod", _vp), ("gamma", _vp), ("beta", _vp),
                ("Y32", _vp), ("Yact", _vp), ("mean", _vp), ("rstd", _vp),
                ("lda", _i32), ("ldw", _i32), ("ldr", _i32), ("ldc32", _i32), ("ldmod", _i32), ("ldy32", _i32), ("ldyact", _i32),
                ("M", _i32), ("N", _i32), ("K", _i32),
                ("n_seg", _i32), ("a_seg_stride", _i64), ("bias_scale", _f32), ("ldcact", _i32), ("Cact", _vp),
                ("ib_c", _vp), ("ib_w1", _vp), ("ib_b1", _vp), ("ib_lnw", _vp), ("ib_lnb", _vp), ("ib_w2", _vp), ("ib_b2", _vp),
                ("ib_h", _i32), ("pad_", _i32)]


XTAIL_MAX_SEG = 4
XTAIL_MAX_GROUPS = 4
MAX_SILU_IB = 4


class SeaExchangeTail(C.Structure):
    _fields_ = [("att", _vp * XTAIL_MAX_SEG), ("Wp", _vp * XTAIL_MAX_SEG), ("Wup", _vp), ("bup", _vp), ("X", _vp), ("Xact", _vp),
                ("n_seg", _i32), ("ldatt", _i32), ("ldwp", _i32), ("ldwup", _i32), ("ldx", _i32), ("ldxact", _i32),
                ("M", _i32), ("D", _i32), ("E", _i32), ("has_down", _i32), ("bias_scale", _f32),
                ("down", SeaGemmNormGroup)]


CHAIN_MAX_PROJ = 6
CHAIN_MAX_GROUPS = 3
CHAIN_MAX_RIDERS = 8


class SeaRowChain(C.Structure):
    _fields_ = [("att", _vp * XTAIL_MAX_SEG), ("Wp", _vp * XTAIL_MAX_SEG), ("a2", _vp), ("W2", _vp), ("b2", _vp), ("Xin", _vp), ("X", _vp), ("Xact", _vp),
                ("n_seg", _i32), ("ldatt", _i32), ("ldwp", _i32), ("lda2", _i32), ("ldw2", _i32), ("ldxin", _i32), ("ldx", _i32), ("ldxact", _i32),
                ("M", _i32), ("D", _i32), ("E", _i32), ("has_down", _i32), ("n_proj", _i32), ("bias_scale", _f32),
                ("down", SeaGemmNormGroup), ("proj", SeaQkvGroup * CHAIN_MAX_PROJ),
                ("tile_stamps", _vp), ("tile_cond", _vp), ("tile_epoch", _vp), ("tile_count", _vp), ("tile_sets", _i32), ("pad_", _i32)]   # the rider tiles' condition memo (group 0; NULL: none)


MAX_ADALN_GROUPS = 16


class SeaAdalnGroup(C.Structure):
    _fields_ = [("A", _vp), ("W", _vp), ("bias", _vp), ("X", _vp), ("gamma", _vp), ("beta", _vp), ("Yact", _vp), ("Y32", _vp), ("mean", _vp), ("rstd", _vp),
                ("lda", _i32), ("ldw", _i32), ("ldx", _i32), ("ldyact", _i32), ("ldy32", _i32), ("M", _i32), ("d", _i32), ("K", _i32)]


MAX_SPLITK_GROUPS = 8


class SeaEncBlock(C.Structure):
    _fields_ = [(n, _vp) for n in ("Zin", "Zout", "wqkv", "bqkv", "wo", "w1", "b1", "lnw", "lnb", "w2", "b2", "g1", "g2", "dZout", "dZin",
                                   "n1", "dqkv", "att", "dz1", "n2", "dh", "hg", "dz2", "u1", "u2", "u3w", "u3b", "ws")] + \
                [("ws_floats", _i64), ("B", _i32), ("P", _i32), ("W", _i32), ("H", _i32), ("eps", _f32), ("pad_", _i32)]


class SeaSplitkGroup(C.Structure):
    _fields_ = [("P", _vp), ("bias", _vp), ("R", _vp), ("C32", _vp), ("Cact", _vp), ("p_stride", _i64), ("S", _i32), ("M", _i32), ("N", _i32), ("ldp", _i32),
                ("ldr", _i32), ("ldc32", _i32), ("ldcact", _i32), ("bias_scale", _f32)]


MAX_AQKV_GROUPS = 4
AQKV_MAX_SILU = 8


class SeaAdalnQkv(C.Structure):
    _fields_ = [("X", _vp), ("cond", _vp), ("w1", _vp), ("b1", _vp), ("W2c", _vp), ("b2c", _vp), ("gamma", _vp), ("beta", _vp), ("Wqkv", _vp), ("bqkv", _vp),
                ("Q", _vp), ("K", _vp), ("Vt", _vp), ("ldx", _i32), ("ldw2c", _i32), ("ldw", _i32), ("M", _i32), ("E", _i32), ("N3", _i32),
                ("w13", _vp), ("b13", _vp), ("W3", _vp), ("b3", _vp), ("mod3", _vp), ("ldw3", _i32), ("ldmod3", _i32),
                ("memo_stamps", _vp), ("memo_mods", _vp), ("memo_epoch", _vp), ("memo_count", _vp), ("memo_rows", _vp), ("ldmemo", _i32), ("pad_", _i32)]   # the condition memo (NULL: none)


MAX_MLP_GROUPS = 8


class SeaMlpGroup(C.Structure):
    _fields_ = [("A", _vp), ("W1", _vp), ("b1", _vp), ("lnw", _vp), ("lnb", _vp), ("Hg", _vp),
                ("lda", _i32), ("ldw", _i32), ("ldh", _i32), ("M", _i32), ("E", _i32), ("S", _i32),
                ("X32", _vp), ("addend", _vp), ("Xout", _vp), ("mod", _vp), ("gamma", _vp), ("beta", _vp),
                ("ldx32", _i32), ("ldadd", _i32), ("ldxout", _i32), ("ldmod", _i32), ("norm_eps", _f32), ("pad_", _i32)]


class SeaMlp2Group(C.Structure):
    _fields_ = [("Hg", _vp), ("W2", _vp), ("b2", _vp), ("R", _vp), ("Wproj", _vp), ("bproj", _vp), ("gamma", _vp), ("beta", _vp), ("mod", _vp),
                ("Y32", _vp), ("Yact", _vp),
                ("ldh", _i32), ("ldw2", _i32), ("ldr", _i32), ("ldwp", _i32), ("ldmod", _i32), ("ldy32", _i32), ("ldyact", _i32),
                ("M", _i32), ("E", _i32), ("S", _i32)]


class SeaStepPatch(C.Structure):
    _fields_ = [("addr", _vp), ("kind", _i32), ("pad_", _i32), ("base", C.c_int64), ("stride", C.c_int64)]


KV_MAX_FIELDS = 4


class SeaKvNorm(C.Structure):
    _fields_ = [("gamma", _vp), ("beta", _vp), ("mod", _vp), ("ldmod", _i32), ("pad_", _i32)]


class SeaKvField(C.Structure):
    _fields_ = [("ln0", SeaKvNorm), ("ln_cross", SeaKvNorm), ("ln2", SeaKvNorm),
                ("Wqkv", _vp), ("bqkv", _vp), ("Wo", _vp), ("Wdown", _vp), ("bdown", _vp), ("Wup", _vp), ("bup", _vp),
                ("W1", _vp), ("b1", _vp), ("lnw", _vp), ("lnb", _vp), ("W2", _vp), ("b2", _vp), ("Wproj", _vp), ("bproj", _vp),
                ("Ks", _vp), ("Vs", _vp)]


class SeaKvPair(C.Structure):
    _fields_ = [("Wq", _vp), ("bq", _vp), ("Wkv", _vp), ("bkv", _vp), ("Wp", _vp), ("Kc", _vp), ("Vc", _vp)]


class SeaKvLayer(C.Structure):
    _fields_ = [("f", SeaKvField * KV_MAX_FIELDS), ("p", (SeaKvPair * KV_MAX_FIELDS) * KV_MAX_FIELDS), ("ib", _vp)]


class SeaKvGlobal(C.Structure):
    _fields_ = [("F", _i32), ("E", _i32), ("D", _i32), ("S", _i32), ("H", _i32), ("B", _i32), ("L", _i32), ("cap", _i32),
                ("exchange", _i32), ("ib_after_cross", _i32), ("final_ln", SeaKvNorm * KV_MAX_FIELDS),
                ("rope_self", _vp), ("rope_cross", _vp), ("traj", _vp), ("xl", _vp * 2),
                ("att_e", _vp), ("xr", _vp), ("xq", _vp), ("x3", _vp), ("hbuf", _vp), ("nd_old", _vp), ("oc", _vp), ("qc", _vp), ("ml", _vp),
                ("handoff", _vp), ("err", _vp), ("handoff_words", _i64)]


KV_FILL_MAX = 32


class SeaKvFill(C.Structure):
    _fields_ = [("K", _vp), ("Vt", _vp), ("Kd", _vp), ("Vd", _vp), ("B", _i32), ("H", _i32), ("hd", _i32), ("n_pos", _i32), ("cap_src", _i32),
                ("cap_dst", _i32), ("v_rows", _i32), ("pad_", _i32)]


KV_FORK_MAX = 32


class SeaKvFork(C.Structure):
    _fields_ = [("src", _vp), ("dst", _vp), ("B_src", _i32), ("H", _i32), ("hd", _i32), ("n_pos", _i32), ("cap_src", _i32), ("cap_dst", _i32),
                ("n_rep", _i32), ("transposed", _i32)]


KV_GATHER_MAX = 32


class SeaKvGather(C.Structure):
    # (not in ABI_STRUCTS: sea_struct_sizes() keeps SeaKvFork as its last entry; tests/test_session_select_cpu.py checks this layout through the library)
    _fields_ = [("src", _vp), ("dst", _vp), ("index", _vp), ("B_src", _i32), ("B_dst", _i32), ("H", _i32), ("hd", _i32), ("n_pos", _i32),
                ("cap_src", _i32), ("cap_dst", _i32), ("src_transposed", _i32), ("dst_transposed", _i32), ("pad_", _i32)]


DECODE_MSE_MAX_GROUPS = 16
DECODE_MSE_ROWS = 64       # rows per workgroup of sea_decode_mse: its partial workspace holds ceil(M / 64) * n_groups floats
DECODE_MSE_MAX_S = 640


class SeaDecodeMseGroup(C.Structure):
    # (not in ABI_STRUCTS, like SeaKvGather; tests/test_decode_loss_cpu.py checks the layouts through the library's argument checks)
    _fields_ = [("H", _vp), ("W2", _vp), ("bias", _vp), ("dH", _vp), ("Z", _vp), ("ldh", _i32), ("ldw", _i32), ("lddh", _i32), ("ldz", _i32),
                ("n_fields", _i32), ("field0", _i32)]


class SeaDecodeMse(C.Structure):
    _fields_ = [("target", _vp), ("counts", _vp), ("loss", _vp), ("partial", _vp), ("ld_row", _i64), ("ld_field", _i64),
                ("M", _i32), ("S", _i32), ("C", _i32), ("Cp", _i32), ("P", _i32), ("n_partial_cap", _i32), ("inv_n", _f32), ("grad_scale", _f32)]


class SeaDecodeMemberSse(C.Structure):
    # sea_decode_member_sse (not in ABI_STRUCTS either; tests/test_ensemble_cpu.py checks the layout through the library's argument checks)
    _fields_ = [("target", _vp), ("counts", _vp), ("sse", _vp), ("work", _vp), ("ld_row", _i64), ("ld_field", _i64), ("work_cap", _i64),
                ("M", _i32), ("S", _i32), ("C", _i32), ("Cp", _i32), ("P", _i32), ("members", _i32), ("n_fields_total", _i32), ("pad_", _i32)]


class SeaDecodeMemberMoments(C.Structure):
    # sea_decode_member_moments (not in ABI_STRUCTS, like its siblings: sea_struct_sizes() keeps SeaKvFork as its last entry and the existing tests hold
    # that table at 33 entries; tests/test_ensemble_moments_cpu.py checks the layout through the library's argument checks)
    _fields_ = [("w", _vp), ("var_scale", _vp), ("counts", _vp), ("mean", _vp), ("var", _vp), ("work", _vp), ("work_cap", _i64),
                ("M", _i32), ("S", _i32), ("C", _i32), ("Cp", _i32), ("P", _i32), ("members", _i32), ("n_fields_total", _i32), ("ld", _i32)]


class SeaDecodeMemberGram(C.Structure):
    # sea_decode_member_gram (not in ABI_STRUCTS, like its siblings; tests/test_field_enkf_cpu.py checks the layout through the library's argument checks)
    _fields_ = [("obs", _vp), ("prec_field", _vp), ("prec", _vp), ("counts", _vp), ("gram", _vp), ("proj", _vp), ("count", _vp),
                ("ld_row", _i64), ("ld_field", _i64), ("ld_prow", _i64), ("ld_pfield", _i64),
                ("M", _i32), ("S", _i32), ("C", _i32), ("Cp", _i32), ("P", _i32), ("members", _i32), ("n_fields_total", _i32), ("pad_", _i32)]


class SeaDecodeSensorSse(C.Structure):
    # sea_decode_sensor_sse (not in ABI_STRUCTS, like its siblings; tests/test_sensor_cpu.py checks the layout through the library's argument checks)
    _fields_ = [("obs", _vp), ("prec", _vp), ("live", _vp), ("wrow", _vp), ("seg", _vp), ("wsse", _vp), ("pred", _vp), ("work", _vp),
                ("ld_obs", _i64), ("ld_prec", _i64), ("work_cap", _i64),
                ("Bm", _i32), ("members", _i32), ("S", _i32), ("Cp", _i32), ("Q", _i32), ("K_pad", _i32)]


class SeaDecodeSensorGrad(C.Structure):
    # sea_decode_sensor_grad: SeaDecodeSensorSse's fields, then grad_scale (not in ABI_STRUCTS, like its siblings; tests/test_sensor_grad_cpu.py checks the
    # layout through the library's argument checks)
    _fields_ = SeaDecodeSensorSse._fields_ + [("grad_scale", _f32), ("pad_", _i32)]


class SeaDerivedSensorTables(C.Structure):
    # sea_decode_derived_sensor_sse / _grad: the pair tables of a DerivedSensorSet (not in ABI_STRUCTS; tests/test_derived_sensor_cpu.py checks the size)
    _fields_ = [("op", _vp), ("scale", _vp), ("shift", _vp)]


class SeaDecodeFieldGrad(C.Structure):
    # sea_decode_field_grad, 104 bytes (not in ABI_STRUCTS, like its siblings; tests/test_field_grad_cpu.py checks the layout through the library's argument checks)
    _fields_ = [("obs", _vp), ("prec", _vp), ("field_prec", _vp), ("counts", _vp), ("wsse", _vp), ("work", _vp),
                ("ld_row", _i64), ("ld_field", _i64), ("work_cap", _i64),
                ("M", _i32), ("S", _i32), ("C", _i32), ("Cp", _i32), ("P", _i32), ("members", _i32), ("n_fields_total", _i32), ("grad_scale", _f32)]


class SeaEnkfTransform(C.Structure):
    # sea_enkf_transform (not in ABI_STRUCTS, like its siblings; tests/test_enkf_cpu.py checks the layout through the library's argument checks)
    _fields_ = [("pred", _vp), ("obs", _vp), ("prec", _vp), ("taper", _vp), ("D", _vp), ("status", _vp),
                ("ld_pred", _i64), ("ld_obs", _i64), ("ld_prec", _i64), ("ld_taper", _i64), ("rho", C.c_double), ("alpha", C.c_double),
                ("B", _i32), ("N", _i32), ("K", _i32), ("Ld", _i32)]


class SeaEnkfTransformGram(C.Structure):
    # sea_enkf_transform_gram (not in ABI_STRUCTS either; tests/test_field_enkf_cpu.py checks the layout through the library's argument checks)
    _fields_ = [("gram", _vp), ("proj", _vp), ("count", _vp), ("taper", _vp), ("D", _vp), ("status", _vp), ("ld_taper", _i64),
                ("rho", C.c_double), ("alpha", C.c_double), ("B", _i32), ("N", _i32), ("Q", _i32), ("Ld", _i32)]


class SeaEnsembleMix(C.Structure):
    # sea_ensemble_mix (not in ABI_STRUCTS either)
    _fields_ = [("y", _vp), ("D", _vp), ("out", _vp), ("inc", _vp), ("Bm", _i32), ("N", _i32), ("G", _i32), ("P", _i32), ("Dl", _i32), ("Ld", _i32)]


class SeaEnsembleVerify(C.Structure):
    # sea_ensemble_verify (not in ABI_STRUCTS, like its siblings; tests/test_verify_cpu.py checks the layout through the library's argument checks)
    _fields_ = [("pred", _vp), ("obs", _vp), ("prec", _vp), ("logw", _vp), ("mean", _vp), ("spread", _vp), ("crps", _vp), ("pit", _vp), ("rank", _vp),
                ("sums", _vp), ("hist", _vp), ("status", _vp), ("work", _vp),
                ("ld_pred", _i64), ("ld_obs", _i64), ("ld_prec", _i64), ("ld_out", _i64), ("work_bytes", _i64),
                ("B", _i32), ("N", _i32), ("K", _i32), ("unbiased", _i32), ("accumulate", _i32), ("pad_", _i32)]


class SeaDecodeMemberVerify(C.Structure):
    # sea_decode_member_verify (not in ABI_STRUCTS, like its siblings; tests/test_field_verify_cpu.py checks the layout and the library's argument checks)
    _fields_ = [("obs", _vp), ("prec_field", _vp), ("prec", _vp), ("counts", _vp), ("logw", _vp), ("mean", _vp), ("spread", _vp), ("crps", _vp), ("pit", _vp),
                ("rank", _vp), ("sums", _vp), ("hist", _vp), ("status", _vp), ("work", _vp),
                ("ld_row", _i64), ("ld_field", _i64), ("ld_prow", _i64), ("ld_pfield", _i64), ("ld_out", _i64), ("work_bytes", _i64),
                ("M", _i32), ("S", _i32), ("C", _i32), ("Cp", _i32), ("P", _i32), ("members", _i32), ("n_fields_total", _i32), ("unbiased", _i32),
                ("accumulate", _i32), ("pad_", _i32)]


class SeaDecodeMemberCrpsGrad(C.Structure):
    # sea_decode_member_crps_grad, 152 bytes (not in ABI_STRUCTS, like its siblings; tests/test_crps_loss_cpu.py checks the layout and the library's argument checks)
    _fields_ = [("obs", _vp), ("prec_field", _vp), ("prec", _vp), ("field_weight", _vp), ("counts", _vp), ("logw", _vp), ("loss", _vp), ("sums", _vp),
                ("status", _vp), ("work", _vp),
                ("ld_row", _i64), ("ld_field", _i64), ("ld_prow", _i64), ("ld_pfield", _i64), ("work_bytes", _i64),
                ("M", _i32), ("S", _i32), ("C", _i32), ("Cp", _i32), ("P", _i32), ("members", _i32), ("n_fields_total", _i32), ("unbiased", _i32)]


QUANTILE_MAX_LEVELS = 8      # levels, and thresholds, one launch of sea_decode_member_quantiles carries


class SeaDecodeMemberQuantiles(C.Structure):
    # sea_decode_member_quantiles (not in ABI_STRUCTS, like its siblings; tests/test_ensemble_quantiles_cpu.py checks the size the header states)
    _fields_ = [("w", _vp), ("counts", _vp), ("thr", _vp), ("quant", _vp), ("exceed", _vp), ("level", C.c_float * QUANTILE_MAX_LEVELS),
                ("ld", _i64), ("ld_map", _i64),
                ("n_levels", _i32), ("n_thr", _i32), ("M", _i32), ("S", _i32), ("C", _i32), ("Cp", _i32), ("P", _i32), ("members", _i32),
                ("n_fields_total", _i32), ("pad_", _i32)]


BRIER_MAX_T = QUANTILE_MAX_LEVELS   # thresholds one launch of sea_decode_member_brier / sea_ensemble_brier carries
BRIER_SUMS = 5               # fp64 sums per (history, field, threshold): count, sum (p - o)^2, sum p, sum o, count of bad readings
BRIER_MAX_N = 128            # members per history of sea_decode_member_brier / sea_ensemble_brier


class SeaDecodeMemberBrier(C.Structure):
    # sea_decode_member_brier, 200 bytes (not in ABI_STRUCTS, like its siblings; tests/test_brier_cpu.py checks the size the header states and the argument checks)
    _fields_ = [("obs", _vp), ("prec_field", _vp), ("prec", _vp), ("counts", _vp), ("logw", _vp), ("thr", _vp), ("prob", _vp), ("brier", _vp),
                ("sums", _vp), ("hist", _vp), ("hits", _vp), ("status", _vp), ("work", _vp),
                ("ld_row", _i64), ("ld_field", _i64), ("ld_prow", _i64), ("ld_pfield", _i64), ("ld_out", _i64), ("ld_map", _i64), ("work_bytes", _i64),
                ("M", _i32), ("S", _i32), ("C", _i32), ("Cp", _i32), ("P", _i32), ("members", _i32), ("n_fields_total", _i32), ("n_thr", _i32),
                ("accumulate", _i32), ("pad_", _i32)]


DERIVED_MAX = 8              # derived fields one launch of sea_decode_derived_quantiles / sea_decode_derived_brier / sea_decode_derived_verify carries
DERIVED_OPS = {"magnitude": 0, "energy": 1, "difference": 2}   # SEA_DERIVED_MAGNITUDE, SEA_DERIVED_ENERGY, SEA_DERIVED_DIFFERENCE


class SeaDerivedField(C.Structure):
    # a derived field of sea_decode_derived_quantiles / sea_decode_derived_brier, 32 bytes (not in ABI_STRUCTS; tests/test_derived_fields_cpu.py checks the size)
    _fields_ = [("op", _i32), ("a", _i32), ("b", _i32), ("pad_", _i32), ("scale_a", C.c_float), ("shift_a", C.c_float), ("scale_b", C.c_float),
                ("shift_b", C.c_float)]


class SeaEnsembleBrier(C.Structure):
    # sea_ensemble_brier, 176 bytes (not in ABI_STRUCTS either)
    _fields_ = [("pred", _vp), ("obs", _vp), ("prec", _vp), ("logw", _vp), ("thr", _vp), ("prob", _vp), ("brier", _vp), ("sums", _vp), ("hist", _vp),
                ("hits", _vp), ("status", _vp), ("work", _vp),
                ("ld_pred", _i64), ("ld_obs", _i64), ("ld_prec", _i64), ("ld_thr", _i64), ("ld_out", _i64), ("ld_map", _i64), ("work_bytes", _i64),
                ("B", _i32), ("N", _i32), ("K", _i32), ("n_thr", _i32), ("accumulate", _i32), ("pad_", _i32)]


ENKF_MAX_N = 128             # members per history of sea_enkf_transform / sea_ensemble_mix
SENSOR_TILE = 32             # sensors per W2 tile of sea_decode_sensor_sse: every (group, patch) segment of a SensorSet is padded to a multiple of it
SENSOR_MAX_PATCHES = 65535   # observed patches one launch of sea_decode_sensor_sse carries (a grid dimension)
MEMBER_MOMENTS_CHUNK = 128   # members one workgroup of sea_decode_member_moments finishes; above it the launch needs its workspace
VERIFY_MAX_N = 128           # members per history of sea_ensemble_verify
VERIFY_SUMS = 8              # fp64 sums per history of sea_ensemble_verify
FIELD_VERIFY_MAX_N = 128     # members per history of sea_decode_member_verify
CRPS_GRAD_W8_MAX_S = 384     # sea_decode_member_crps_grad: above 64 members the hidden width it carries (beyond: SEA_EUNSUPPORTED, the composed path)
CRPS_PACK_MAX_N = 32         # sea_decode_member_crps_grad_packed: members per history (above: SEA_EUNSUPPORTED; sea_decode_member_crps_grad serves)
SEA_EUNSUPPORTED = -3
QUANTILE_MAX_N = 128         # members per history of sea_decode_member_quantiles
RESAMPLE_MAX_N = 4096      # members per history of sea_resample_systematic

MAX_WGRAD_GROUPS = 32
MAX_NORM_BWD_GROUPS = 8
MAX_SILU_BWD_GROUPS = 24

_lib: Optional[C.CDLL] = None


class NativeLibraryError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load (once) and return the shared library; raise loudly if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            f"{LIB_PATH} is missing: build it with `python -m sea_amd.build` (hipcc, gfx950). "
            "sea_amd has no CPU or eager fallback.")
    try:
        L = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise NativeLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    L.sea_abi_version.restype = C.c_int
    L.sea_last_error.restype = C.c_char_p
    L.sea_last_form.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.sea_last_form.restype = C.c_char_p
    L.sea_struct_sizes.argtypes = [C.POINTER(C.c_int), C.c_int]
    L.sea_struct_sizes.restype = C.c_int
    L.sea_device_info.argtypes = [C.POINTER(C.c_int), C.c_char_p, C.c_int]
    L.sea_gemm_grouped.argtypes = [C.POINTER(SeaGemmGroup), C.c_int, C.c_int, _vp]
    L.sea_qkv_rope_grouped.argtypes = [C.POINTER(SeaQkvGroup), C.c_int, C.POINTER(SeaQkvCommon), C.c_int, _vp]
    L.sea_attention_fwd.argtypes = [C.POINTER(SeaAttnParams), C.c_int, _vp]
    L.sea_rownorm.argtypes = [C.POINTER(SeaNormGroup), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _vp]
    L.sea_gemm_fewrows.argtypes = [C.POINTER(SeaGemmGroup), C.POINTER(SeaNormGroup), C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _vp]
    L.sea_gemm_fewrows.restype = C.c_int
    L.sea_qkv_rope_fewrows.argtypes = [C.POINTER(SeaQkvGroup), C.POINTER(SeaNormGroup), C.c_int, C.POINTER(SeaQkvCommon), C.c_float, C.c_int, _vp]
    L.sea_qkv_rope_fewrows.restype = C.c_int
    L.sea_silu_outer.argtypes = [C.POINTER(SeaSiluGroup), C.c_int, _vp, C.c_int, C.c_int, _vp]
    L.sea_ib_add.argtypes = [C.POINTER(SeaIbParams), _vp]
    L.sea_convert_f32_to_act.argtypes = [_vp, _i64, _vp, _i64, _i64, _i64, C.c_int, _vp]
    L.sea_selftest_mfma.restype = C.c_int
    L.sea_wgrad_grouped.argtypes = [C.POINTER(SeaWgradGroup), C.c_int, C.c_int, _vp]
    L.sea_transpose_weights.argtypes = [_vp, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int, _vp]
    L.sea_rownorm_bwd.argtypes = [C.POINTER(SeaNormBwdGroup), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _i64, _vp]
    L.sea_silu_outer_bwd.argtypes = [C.POINTER(SeaSiluBwdGroup), C.c_int, _vp, C.c_int, C.c_int, _vp, _i64, _vp]
    L.sea_ib_bwd.argtypes = [C.POINTER(SeaIbBwdParams), _vp]
    L.sea_silu_outer_bwd_dc.argtypes = [C.POINTER(SeaSiluBwdGroup), C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, _i64, _vp]
    L.sea_silu_outer_bwd_dc_ws_floats.argtypes = [C.POINTER(SeaSiluBwdGroup), C.c_int, C.c_int]
    L.sea_silu_outer_bwd_dc_ws_floats.restype = _i64
    L.sea_ib_bwd_dc.argtypes = [C.POINTER(SeaIbBwdParams), _vp, _vp]
    L.sea_attention_bwd.argtypes = [C.POINTER(SeaAttnBwdParams), C.c_int, _vp]
    L.sea_dropout_mask.argtypes = [_vp, _i64, _i64, C.c_uint32, C.c_uint32, _i32, _vp]
    L.sea_dropout_mask.restype = C.c_int
    L.sea_unpatchify.argtypes = [_vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp]
    L.sea_unpatchify.restype = C.c_int
    L.sea_gemm_rownorm.argtypes = [C.POINTER(SeaGemmNormGroup), C.c_int, C.c_float, C.c_int, _vp]
    L.sea_gemm_rownorm.restype = C.c_int
    L.sea_exchange_tail.argtypes = [C.POINTER(SeaExchangeTail), C.c_int, C.c_float, C.c_int, _vp]
    L.sea_exchange_tail.restype = C.c_int
    L.sea_gemm_adaln.argtypes = [C.POINTER(SeaAdalnGroup), C.c_int, C.c_float, C.c_int, _vp]
    L.sea_gemm_adaln.restype = C.c_int
    L.sea_row_chain.argtypes = [C.POINTER(SeaRowChain), C.c_int, C.POINTER(SeaQkvCommon), C.c_float, C.c_int, _vp]
    L.sea_row_chain.restype = C.c_int
    L.sea_row_chain_riders.argtypes = [C.POINTER(SeaRowChain), C.c_int, C.POINTER(SeaQkvCommon), C.POINTER(SeaGemmGroup), C.c_int, C.c_int, C.c_int, C.POINTER(SeaIbParams), C.c_float, C.c_int, _vp]
    L.sea_row_chain_riders.restype = C.c_int
    L.sea_patchify.argtypes = [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _vp]
    L.sea_patchify.restype = C.c_int
    L.sea_silu_outer_ib.argtypes = [C.POINTER(SeaSiluGroup), C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp]
    L.sea_silu_outer_ib.restype = C.c_int
    L.sea_mlp_fc1_ln_gelu.argtypes = [C.POINTER(SeaMlpGroup), C.c_int, C.c_float, C.c_int, _vp]
    L.sea_mlp_fc1_ln_gelu.restype = C.c_int
    L.sea_mlp_fc2_proj_norm.argtypes = [C.POINTER(SeaMlp2Group), C.c_int, C.c_float, C.c_int, _vp]
    L.sea_mlp_fc2_proj_norm.restype = C.c_int
    L.sea_mlp_block.argtypes = [C.POINTER(SeaMlpGroup), C.POINTER(SeaMlp2Group), C.c_int, C.c_float, C.c_int, _vp]
    L.sea_mlp_block.restype = C.c_int
    L.sea_adaln_qkv.argtypes = [C.POINTER(SeaAdalnQkv), C.c_int, C.POINTER(SeaQkvCommon), C.POINTER(SeaGemmGroup), C.c_int, C.POINTER(SeaSiluGroup), C.c_int, _vp, C.c_int,
                                C.POINTER(SeaIbParams), C.c_float, C.c_int, _vp]
    L.sea_adaln_qkv.restype = C.c_int
    L.sea_splitk_finish.argtypes = [C.POINTER(SeaSplitkGroup), C.c_int, C.c_int, _vp]
    L.sea_splitk_finish.restype = C.c_int
    L.sea_encoder_block_ws_floats.argtypes = [C.c_int, C.c_int, C.c_int]
    L.sea_encoder_block_ws_floats.restype = _i64
    for name in ("sea_encoder_block_fwd", "sea_encoder_block_bwd"):
        getattr(L, name).argtypes = [C.POINTER(SeaEncBlock), C.c_int, _vp]
        getattr(L, name).restype = C.c_int
    L.sea_run_list.argtypes = [C.POINTER(SeaLaunchRec), C.c_int, _vp]
    L.sea_run_list.restype = C.c_int
    L.sea_run_list_steps.argtypes = [C.POINTER(SeaLaunchRec), C.c_int, C.POINTER(SeaStepPatch), C.c_int, C.c_int, C.c_int, _vp]
    L.sea_run_list_steps.restype = C.c_int
    L.sea_kv_rollout.argtypes = [C.POINTER(SeaKvGlobal), C.POINTER(SeaKvLayer), C.c_int, C.c_int, C.c_uint32, C.c_int, _vp]
    L.sea_kv_rollout.restype = C.c_int
    L.sea_kv_arena_words.argtypes = [C.POINTER(SeaKvGlobal)]
    L.sea_kv_arena_words.restype = C.c_int64
    L.sea_kv_debug_stamps.argtypes = [_vp]
    L.sea_kv_debug_stamps.restype = None
    L.sea_kv_cache_fill.argtypes = [C.POINTER(SeaKvFill), C.c_int, C.c_int, _vp]
    L.sea_kv_cache_fill.restype = C.c_int
    L.sea_kv_cache_fork.argtypes = [C.POINTER(SeaKvFork), C.c_int, C.c_int, _vp]
    L.sea_kv_cache_fork.restype = C.c_int
    L.sea_kv_cache_gather.argtypes = [C.POINTER(SeaKvGather), C.c_int, C.c_int, _vp]
    L.sea_kv_cache_gather.restype = C.c_int
    L.sea_decode_mse.argtypes = [C.POINTER(SeaDecodeMseGroup), C.c_int, C.POINTER(SeaDecodeMse), C.c_int, _vp]
    L.sea_decode_mse.restype = C.c_int
    L.sea_decode_member_sse.argtypes = [C.POINTER(SeaDecodeMseGroup), C.c_int, C.POINTER(SeaDecodeMemberSse), C.c_int, _vp]
    L.sea_decode_member_sse.restype = C.c_int
    L.sea_decode_sensor_sse.argtypes = [C.POINTER(SeaDecodeMseGroup), C.c_int, C.POINTER(SeaDecodeSensorSse), C.c_int, _vp]
    L.sea_decode_sensor_sse.restype = C.c_int
    L.sea_decode_sensor_grad.argtypes = [C.POINTER(SeaDecodeMseGroup), C.c_int, C.POINTER(SeaDecodeSensorGrad), C.c_int, _vp]
    L.sea_decode_sensor_grad.restype = C.c_int
    L.sea_decode_derived_sensor_sse.argtypes = [C.POINTER(SeaDecodeMseGroup), C.c_int, C.POINTER(SeaDecodeSensorSse), C.POINTER(SeaDerivedSensorTables), C.c_int, _vp]
    L.sea_decode_derived_sensor_sse.restype = C.c_int
    L.sea_decode_derived_sensor_grad.argtypes = [C.POINTER(SeaDecodeMseGroup), C.c_int, C.POINTER(SeaDecodeSensorGrad), C.POINTER(SeaDerivedSensorTables), C.c_int, _vp]
    L.sea_decode_derived_sensor_grad.restype = C.c_int
    L.sea_decode_field_grad.argtypes = [C.POINTER(SeaDecodeMseGroup), C.c_int, C.POINTER(SeaDecodeFieldGrad), C.c_int, _vp]
    L.sea_decode_field_grad.restype = C.c_int
    L.sea_decode_member_moments.argtypes = [C.POINTER(SeaDecodeMseGroup), C.c_int, C.POINTER(SeaDecodeMemberMoments), C.c_int, _vp]
    L.sea_decode_member_moments.restype = C.c_int
    L.sea_resample_systematic.argtypes = [_vp, _vp, C.c_float, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]
    L.sea_resample_systematic.restype = C.c_int
    L.sea_enkf_transform.argtypes = [C.POINTER(SeaEnkfTransform), _vp]
    L.sea_enkf_transform.restype = C.c_int
    L.sea_decode_member_gram.argtypes = [C.POINTER(SeaDecodeMseGroup), C.c_int, C.POINTER(SeaDecodeMemberGram), C.c_int, _vp]
    L.sea_decode_member_gram.restype = C.c_int
    L.sea_enkf_transform_gram.argtypes = [C.POINTER(SeaEnkfTransformGram), _vp]
    L.sea_enkf_transform_gram.restype = C.c_int
    L.sea_ensemble_mix.argtypes = [C.POINTER(SeaEnsembleMix), C.c_int, _vp]
    L.sea_ensemble_mix.restype = C.c_int
    L.sea_ensemble_verify.argtypes = [C.POINTER(SeaEnsembleVerify), _vp]
    L.sea_ensemble_verify.restype = C.c_int
    L.sea_ensemble_verify_ws_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    L.sea_ensemble_verify_ws_bytes.restype = _i64
    L.sea_decode_member_verify.argtypes = [C.POINTER(SeaDecodeMseGroup), C.c_int, C.POINTER(SeaDecodeMemberVerify), C.c_int, _vp]
    L.sea_decode_member_verify.restype = C.c_int
    L.sea_decode_member_verify_ws_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.sea_decode_member_verify_ws_bytes.restype = _i64
    L.sea_decode_member_crps_grad.argtypes = [C.POINTER(SeaDecodeMseGroup), C.c_int, C.POINTER(SeaDecodeMemberCrpsGrad), C.c_int, _vp]
    L.sea_decode_member_crps_grad.restype = C.c_int
    L.sea_decode_member_crps_grad_ws_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.sea_decode_member_crps_grad_ws_bytes.restype = _i64
    L.sea_decode_member_crps_grad_packed.argtypes = [C.POINTER(SeaDecodeMseGroup), C.c_int, C.POINTER(SeaDecodeMemberCrpsGrad), C.c_int, _vp]
    L.sea_decode_member_crps_grad_packed.restype = C.c_int
    L.sea_decode_member_quantiles.argtypes = [C.POINTER(SeaDecodeMseGroup), C.c_int, C.POINTER(SeaDecodeMemberQuantiles), C.c_int, _vp]
    L.sea_decode_member_quantiles.restype = C.c_int
    L.sea_decode_member_brier.argtypes = [C.POINTER(SeaDecodeMseGroup), C.c_int, C.POINTER(SeaDecodeMemberBrier), C.c_int, _vp]
    L.sea_decode_member_brier.restype = C.c_int
    L.sea_decode_member_brier_ws_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.sea_decode_member_brier_ws_bytes.restype = _i64
    L.sea_decode_derived_quantiles.argtypes = [C.POINTER(SeaDecodeMseGroup), C.c_int, C.POINTER(SeaDerivedField), C.c_int, C.POINTER(SeaDecodeMemberQuantiles), C.c_int, _vp]
    L.sea_decode_derived_quantiles.restype = C.c_int
    L.sea_decode_derived_brier.argtypes = [C.POINTER(SeaDecodeMseGroup), C.c_int, C.POINTER(SeaDerivedField), C.c_int, C.POINTER(SeaDecodeMemberBrier), C.c_int, _vp]
    L.sea_decode_derived_brier.restype = C.c_int
    L.sea_decode_derived_verify.argtypes = [C.POINTER(SeaDecodeMseGroup), C.c_int, C.POINTER(SeaDerivedField), C.c_int, C.POINTER(SeaDecodeMemberVerify), C.c_int, _vp]
    L.sea_decode_derived_verify.restype = C.c_int
    L.sea_ensemble_brier.argtypes = [C.POINTER(SeaEnsembleBrier), _vp]
    L.sea_ensemble_brier.restype = C.c_int
    L.sea_ensemble_brier_ws_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    L.sea_ensemble_brier_ws_bytes.restype = _i64
    for name in ("sea_attention_bwd", "sea_wgrad_grouped", "sea_transpose_weights", "sea_rownorm_bwd", "sea_silu_outer_bwd", "sea_ib_bwd",
                 "sea_silu_outer_bwd_dc", "sea_ib_bwd_dc"):
        getattr(L, name).restype = C.c_int
    L.sea_mse_fwd_bwd.argtypes = [_vp, _vp, _vp, _vp, _vp, C.c_int, _i64, C.c_float, _vp]
    L.sea_relative_mse.argtypes = [_vp, _vp, _vp, _i64, C.c_int, _vp]
    L.sea_adamw_flat.argtypes = [_vp, _vp, _vp, _vp, _vp, C.c_int, _i64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                 C.c_int, C.c_float, _vp]
    L.sea_grad_norm_ctl.argtypes = [_vp, _i64, C.c_float, C.c_float, C.c_int, C.c_float, C.c_float, _vp, C.c_int, _vp, _vp]
    L.sea_adamw_flat_ctl.argtypes = [_vp, _vp, _vp, _vp, _vp, C.c_int, _i64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                     C.c_float, _vp, _vp]
    for name in ("sea_gemm_grouped", "sea_qkv_rope_grouped", "sea_attention_fwd", "sea_rownorm", "sea_silu_outer",
                 "sea_ib_add", "sea_convert_f32_to_act", "sea_device_info", "sea_mse_fwd_bwd", "sea_relative_mse",
                 "sea_adamw_flat", "sea_grad_norm_ctl", "sea_adamw_flat_ctl"):
        getattr(L, name).restype = C.c_int
    if L.sea_abi_version() != ABI_VERSION:
        raise NativeLibraryError(f"{LIB_PATH}: ABI version {L.sea_abi_version()} != {ABI_VERSION}; rebuild (python -m sea_amd.build --force)")
    _lib = L
    return L


ABI_STRUCTS = (SeaGemmGroup, SeaQkvGroup, SeaQkvCommon, SeaAttnProblem, SeaAttnParams, SeaNormGroup, SeaSiluGroup,
               SeaIbParams, SeaWgradGroup, SeaNormBwdGroup, SeaSiluBwdGroup, SeaIbBwdParams, SeaAttnBwdProblem, SeaAttnBwdParams,
               SeaDropout, SeaLaunchRec, SeaGemmNormGroup, SeaExchangeTail, SeaMlpGroup, SeaMlp2Group, SeaKvNorm, SeaKvField, SeaKvPair, SeaKvLayer, SeaKvGlobal, SeaStepPatch, SeaRowChain, SeaAdalnGroup, SeaAdalnQkv, SeaSplitkGroup, SeaEncBlock,
               SeaKvFill, SeaKvFork)

EXPORTED_SYMBOLS = (
    "sea_abi_version", "sea_last_error", "sea_last_form", "sea_struct_sizes", "sea_device_info", "sea_gemm_grouped", "sea_qkv_rope_grouped",
    "sea_attention_fwd", "sea_rownorm", "sea_silu_outer", "sea_ib_add", "sea_convert_f32_to_act", "sea_selftest_mfma",
    "sea_mse_fwd_bwd", "sea_relative_mse", "sea_adamw_flat", "sea_grad_norm_ctl", "sea_adamw_flat_ctl",
    "sea_wgrad_grouped", "sea_transpose_weights", "sea_rownorm_bwd", "sea_silu_outer_bwd", "sea_ib_bwd",
    "sea_attention_bwd", "sea_dropout_mask", "sea_run_list", "sea_run_list_steps", "sea_unpatchify", "sea_gemm_rownorm", "sea_exchange_tail", "sea_patchify", "sea_silu_outer_ib", "sea_mlp_fc1_ln_gelu", "sea_mlp_fc2_proj_norm", "sea_kv_rollout", "sea_kv_arena_words", "sea_kv_debug_stamps",
    "sea_kv_cache_fill", "sea_kv_cache_fork", "sea_kv_cache_gather", "sea_decode_mse", "sea_decode_member_sse", "sea_decode_member_moments", "sea_decode_sensor_sse", "sea_decode_sensor_grad", "sea_decode_field_grad", "sea_resample_systematic", "sea_enkf_transform", "sea_enkf_transform_gram", "sea_decode_member_gram", "sea_ensemble_mix", "sea_ensemble_verify", "sea_ensemble_verify_ws_bytes", "sea_decode_member_verify", "sea_decode_member_verify_ws_bytes", "sea_decode_member_quantiles",
    "sea_decode_member_crps_grad", "sea_decode_member_crps_grad_ws_bytes", "sea_decode_member_crps_grad_packed",
    "sea_decode_member_brier", "sea_decode_member_brier_ws_bytes", "sea_ensemble_brier", "sea_ensemble_brier_ws_bytes",
    "sea_decode_derived_quantiles", "sea_decode_derived_brier", "sea_decode_derived_verify", "sea_decode_derived_sensor_sse", "sea_decode_derived_sensor_grad",
    "sea_gemm_fewrows", "sea_qkv_rope_fewrows", "sea_row_chain", "sea_row_chain_riders", "sea_gemm_adaln", "sea_mlp_block", "sea_adaln_qkv", "sea_splitk_finish",
    "sea_encoder_block_ws_floats", "sea_encoder_block_fwd", "sea_encoder_block_bwd",
    "sea_silu_outer_bwd_dc", "sea_silu_outer_bwd_dc_ws_floats", "sea_ib_bwd_dc",
)


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().sea_last_error()
        raise RuntimeError(f"libsea_hip {what} failed (code {rc}): {msg.decode() if msg else '?'}")


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return SEA_F32
    if dt == torch.bfloat16:
        return SEA_BF16
    raise ValueError(f"sea_amd: activation dtype must be float32 or bfloat16, got {dt}")


def require_gpu(t: torch.Tensor, name: str = "tensor") -> None:
    if not t.is_cuda:
        raise RuntimeError(
            f"sea_amd: {name} is on {t.device}; this path runs only on an MI355X through libsea_hip.so "
            "(no CPU fallback — the CPU oracle lives under oracle/ for tests only)")


def require_same_operand(out: torch.Tensor, target: torch.Tensor, what: str, f32: bool = False) -> None:
    """A loss reads `out.numel()` elements of the target through its raw pointer: refuse, before any launch, a target of another shape or
    device, or (f32=True: the caller converts nothing) of a dtype other than float32."""
    if target.shape != out.shape:
        raise ValueError(f"sea_amd: {what}: target shape {tuple(target.shape)} does not match output shape {tuple(out.shape)}")
    if target.device != out.device:
        raise ValueError(f"sea_amd: {what}: target is on {target.device}, output on {out.device}")
    if f32 and target.dtype != torch.float32:
        raise ValueError(f"sea_amd: {what}: target dtype {target.dtype} must be torch.float32 (output shape {tuple(out.shape)})")


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()
