"""The package's environment switches, all of them (defaults are the measured best):

  SEA_AMD_DTYPE   fp32 | bf16            compute dtype of new models (TemporalModel.set_compute_dtype overrides)
  SEA_CHECK_PTRS  1                      audit every launch plan's device pointers at EVERY bind (default: at a plan's first bind) — sea_amd/ptrcheck.py
  SEA_DP_OVERLAP  0                      data-parallel step: ONE gradient all-reduce after the backward instead of slices under it
  SEA_DP_REHEARSE 1                      a process group of ONE rank issues the data-parallel step's collectives instead of skipping them (sea_amd/parallel.py:
                                           how the RCCL path runs on a one-GPU box: tests/test_parallel_gpu.py, `SEA_DP_REHEARSE=1 python bench.py --mode train`)
  SEA_PLAN        key=value,...          forms of the launch plans (what the tests force to compare every form with the default one).  Every key but the last two is read in ONE
                                         place, plan_forms.resolve_forms, once per plan build; the measurements behind the defaults are the comments of plan_forms.PlanForms:
                                           lanes=none|cond|all   parallel graph branches            norm=0                Linear + row norm as two launches
                                           xtail=0               a field's exchange tail as three launches               xtail_max_rows=N      ... from N rows up
                                           chain=0               the 18-launch plan instead of the row chains            chain_max_rows=N      row chains up to N rows (4096)
                                           riders=0              whole-model condition launches instead of riders        rider_caps=a:b:c      rider tiles per chain launch (tuning aid)
                                           front=0               silu + sea_gemm_adaln + QKV instead of sea_adaln_qkv    front3=0              ... keeps the silu launch
                                           front_big=1           sea_adaln_qkv at long launches too                      adaln_gemm=0          cond_mlp.2 GEMM + norm launch in front
                                           silu=0|1              generated GEMM operand off / on    fold_ib=0             the info-bottleneck add as a launch of its own
                                           fold_ib_gen=1         ... folded at long launches too    mlp1 / mlpnorm / mlp2=0|1   the fused MLP halves off / forced
                                           mlpblock=0            the field MLP as two launches      projnorm=0            the last proj and the final norm as two launches
                                           splitk=0              no split-K form of skinny GEMMs with a long contraction
                                           cond_memo=0           the one-launch front recomputes its condition-only work at every forward (and the rider tiles theirs)
                                           rider_memo=0          the chain launches' rider tiles recompute at every forward; the front's memo stays
                                           graph_lanes=0         a captured graph replays its lanes in record order (engine.forward_graphed)
                                           enc=composed|fused    spatial encoder training: every EncoderBlock composed from the generic launches (default, measured
                                                                   faster) or as the fused sea_encoder_block_fwd / _bwd (bf16, width 32 or 64; other shapes always compose)
  SEA_KV          key=value,...          KV-cache rollout: fast=0 (generic step plan), hoist=0 (condition work per step), gemv=0 (step plan without the few-row launches of gemv.hip),
                                           loop=python (step loop in Python),
                                           force_err=1 (test hook: the persistent launch "reports" a hand-off that gave up)
  SEA_TUNE        key=value,...          native tuning aids read by libsea_hip.so (sea_tune() in core.hip: one getenv, which returns at once when the variable is unset).
                                         Read at EVERY call, because the tests force one form after another in one process — a key held in a function-local static
                                         is fixed by the first call of the process, long before the forcing test starts —: gemm_tile (64 | 128), gemm256 (0 | 1),
                                         gemm_ws (0 off, 2 also short launches), gemm_norm_rows (16 | 64), attn_split4 (0 | 1), attn_paired, attnb_mode (attention
                                         backward: 1 XCD-local order, 2 paired causal tiles, 3 both, 0 neither), chain_rows, kv_persist, kv_pre, sse_rows, wgrad_tile
                                         (64 | 128 | 256), wgrad_stage, memo_count (1: the condition memo's workgroups count hits / misses into Plan.memo_count, the chain launches' rider tiles into Plan.memo_tile_count).  Every other key (gemm_skinny, gemm_dma_*, gemm_n_major, gemm_norm_dma, attn_row, wgrad_target,
                                         wgrad_xcd, normbwd_*, ...) is a measurement aid read once per process: set it before the first launch; no test may force
                                         one (tests/test_tune_keys_cpu.py).  Which kernel a launch took: ops.last_form() (sea_last_form, include/sea_hip.h).
  SEA_EXTRA_FLAGS "..."                  extra hipcc flags for `python -m sea_amd.build` (A/B builds)
(tests only: SEA_TEST_DP_BACKEND=nccl runs the data-parallel tests one rank per GPU over RCCL.)
"""
from __future__ import annotations

import os
from typing import Dict, Optional


def parse(var: str) -> Dict[str, str]:
    """Every key=value token of a switch variable (plan_forms.resolve_forms reads SEA_PLAN / SEA_KV through this, once per plan build)."""
    out: Dict[str, str] = {}
    for tok in os.environ.get(var, "").split(","):
        if "=" in tok:
            k, v = tok.split("=", 1)
            out[k.strip()] = v.strip()
    return out


def plan(key: str, default: Optional[str] = None) -> Optional[str]:
    """SEA_PLAN token (read at every plan build: tests change it between builds)."""
    return parse("SEA_PLAN").get(key, default)


def kv(key: str, default: Optional[str] = None) -> Optional[str]:
    return parse("SEA_KV").get(key, default)
