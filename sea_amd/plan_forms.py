"""Which launches a plan consists of, decided ONCE per plan build by one pure function.

`resolve_forms` maps plain facts — the model's structural attributes, (B, T, mode), the activation dtype, the plan kind, whether the condition buffers
are hoisted, the SEA_PLAN / SEA_KV switches — to a `PlanForms`; it touches no tensor, no device and not the native library, so the form a shape gets
can be read off (and tested) without a GPU.  engine.Plan stores the result as `plan.forms`; the code that emits the launches only reads it."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import torch

from . import _native as N
from . import _switches
from . import ops

INFERENCE, TRAINING, CONDITION = "inference", "training", "condition"   # engine.Plan / train_engine.TrainPlan / kv_engine.CondPlan


@dataclass(frozen=True)
class PlanForms:
    # Optional lanes (parallel graph branches) for independent work — SEA_PLAN=lanes: "cond" = the condition MLPs the first launch does
    # not need, "all" = also every finished field's MLP beside the remaining exchange stages.  At one trajectory the
    # cross-branch dependencies of a captured HIP graph cost more than the overlap gains; from 8192 rows up the condition lane pays (1 %).
    # With the current 21-launch plan: cfg2 0.252 ms none / 0.284 cond / 0.358 all; B=8 1.166 none / 1.154 cond / 1.245 all
    lanes: bool          # every finished field's MLP on a lane of its own
    split_cond: bool     # the condition MLPs the first launch does not need on lane 1
    # The row-local chains between the attention launches as ONE launch each (sea_row_chain, round 4): self-attention out-projection + residual ->
    # cross_down + ln_cross -> every q of the field and the k / v of the pairs that read its PRE-exchange rows; per field, its exchange tail ->
    # cross_down + ln_cross of the updated rows -> the k / v of the pairs that read them.  No cross-attention QKV launch, no out-projection launch, no
    # down + norm launch: 18 launches -> 14 at cfg2.  bf16, the widths the kernel instantiates, at most 3 fields (the segments' weights share an LDS
    # half), short launches (a workgroup owns most of a CU's LDS: beyond a round or two of workgroups the tiled launches win; SEA_PLAN=chain_max_rows).
    # SEA_PLAN=chain=0 keeps the 18-launch plan (the reference form of tests/test_model_gpu.py::test_optional_plans_match_default_plan).
    chain: bool
    # ... and with them RIDERS (sea_row_chain_riders): the AdaLN condition MLPs are functions of the condition alone, and only AdaLN_0 / ln_cross of the first
    # layer are needed in front of the first attention — the modules the field MLP and the final norm read (62 % of the condition GEMM's work at cfg2)
    # and the information-bottleneck rows are computed by extra workgroups of the chain launches, on the CUs those leave idle (127-192 workgroups on 256
    # CUs): the condition GEMM in front of the step covers 6 of the 12 modules.  One layer, AdaLN, the ib add behind the exchange.
    # SEA_PLAN=riders=0 keeps the whole-model condition launches.
    riders: bool
    # SEA_PLAN=rider_caps, a tuning aid: "a:b:c" = tiles for the first, second, third host.  Measured at cfg2 (tools/chain_probe.py replay): 128:128:128 tiles
    # under the three hosts 0.2153 ms per step, 192:96:96 0.2178, 256:64:64 0.2201, 384:0:0 0.2233, 0:192:192 0.2250, no riders 0.2214 — equal shares (a rider
    # tile, alone on its CU beside 127-192 chain workgroups, takes ~9 us; the hosts last 24 / 16 / 12 us).  None: equal shares.  These figures say that the
    # tiles are ON the hosts' critical path (190 chain workgroups + 128 tiles on 256 CUs: the first host's tiles run in two rounds behind its chain workgroups,
    # and moving tiles between hosts moves the step by up to 10 us).  With the tiles' condition memo (rider_memo below) the split matters on MISS steps only:
    # a tile that hits loads its stamps and leaves
    rider_caps: Optional[Tuple[int, ...]]
    # cond_mlp.0 + SiLU evaluated inside the GEMM of cond_mlp.2 (generated A operand): no hidden matrix, no silu launch.  Inference plans
    # only (the weight gradient of cond_mlp.2 reads the hidden matrix).  The operand is recomputed by every column tile of a row panel (4x at
    # N = 512), VALU work that pays only once the hidden matrix's HBM round trip is the larger cost: measured 0.2685 against 0.2671 ms at cfg2
    # (M = 2024: not used), 1.215 against 1.241 ms at B = 8 (used).  SEA_PLAN=silu=1|0 forces.
    gen_a: bool
    # the info-bottleneck add without a launch of its own: its MLP depends on the condition only, so it is EVALUATED by extra row passes of the silu
    # launch (into ibuf) and ADDED by the AdaLN_2 pass that follows it anyway (SeaNormGroup.addend).  Needs the silu launch (adaln, short launches)
    # and the add after the exchange; SEA_PLAN=fold_ib=0 keeps sea_ib_add.
    # Where the condition GEMMs generate their operand (long launches) there is no silu launch for the ib rows to ride on.  SEA_PLAN=fold_ib_gen=1 gives them a launch of
    # their own (sea_silu_outer_ib without silu rows) and folds the add into the norm pass — measured at B = 8: 29 + 40 us against 30 (ib_add) + 30 (norm): not the default
    fold_ib: bool        # the add rides in the norm pass in front of the MLP
    hoist_ib: bool       # ... and its rows of all steps exist already (hoisted condition buffers): AdaLN or LayerNorm alike
    ib_rows_here: bool   # ... and this plan evaluates them itself (fold_ib and not hoist_ib)
    # the exchange tail of a field (projections + GELU, up-projection + residual, down-projection + norm) as ONE launch: bf16, the widths the
    # kernel instantiates, short launches (SEA_PLAN=xtail=0 keeps the three-launch form; SEA_PLAN=xtail_max_rows bounds M)
    # measured: cfg2 0.281 -> 0.254 ms, B = 2 0.414 -> 0.404, B = 4 0.679 -> 0.675, B = 8 a tie (1.191)
    xtail: bool
    # KV-cache step at the shipped widths (one row per trajectory and field, embed_dim 1024 / 2048): the Linear layers as sea_gemm_fewrows /
    # sea_qkv_rope_fewrows launches with the row norms in front of them folded in (gemv.hip) — 18 launches instead of 22.  SEA_KV=gemv=0 keeps the generic launches.
    few: bool
    few_fold_ln: bool    # ... LayerNorm + GELU of the hidden rows as the prologue of fc2 while re-reading the row and its gains / shifts per workgroup stays below the weight stream
    # hidden rows of the MLP: S is a power of two (4 KiB rows at cfg2) — a 32-row workgroup's stores, and the next launch's 32-row operand tiles, would sit
    # at one 4 KiB stride and crowd a few memory channels; 128 B of padding per row spreads them (fc1 + LN + GELU 27.0 -> 25.4 us stand-alone)
    hidden_pad: int
    # The front of the block as ONE launch (sea_adaln_qkv, round 4): the condition MLP of AdaLN_0 with its hidden rows generated in the launch, AdaLN_0 and the
    # self-attention's q / k / v + rotary epilogue — no hidden rows, no modulation matrix and no normalised rows of these modules in memory, no QKV launch;
    # cond_mlp.2 of ln_cross rides on the CUs it leaves idle.  SEA_PLAN=front=0 keeps silu + sea_gemm_adaln + QKV.
    front_chain: bool
    # ... and with D = 128 the ln_cross modulation of a field is that launch's third layer (hidden rows generated in the launch, 2 D = 256 columns), the hidden
    # rows of the modules further down and the information-bottleneck rows its row riders: no silu launch at all.  SEA_PLAN=front3=0 keeps the silu launch.
    front3: bool
    # cond_mlp.2 of the rider plan's front modules: AdaLN_0's as the GEMM whose epilogue IS the normalisation (sea_gemm_adaln: no modulation matrix, no norm launch),
    # ln_cross's as plain groups of the same launch.  SEA_PLAN=adaln_gemm=0 keeps GEMM + norm launch.
    adaln_front: bool
    # Long launches (B = 8): AdaLN_0 of the first layer, its condition MLP and the self-attention's q / k / v as ONE launch too (sea_adaln_qkv without riders)
    # — opt-in (SEA_PLAN=front_big=1): measured at B = 8 the launch takes 171 us against 67 (condition GEMM) + 31 (norm) + 60 (QKV) as tiled launches, the forward
    # 1.070 against 1.047 ms: with several rounds of workgroups the tiled GEMMs keep three workgroups per CU busy, the row-owning workgroup one.
    front_big: bool
    # Linear + nn.LayerNorm + GELU in one launch where the kernel is instantiated (bf16; SEA_PLAN=mlp1=0 keeps the two launches, =1 forces
    # the one launch).  Every workgroup of that kernel streams the whole of W1, so it needs enough 32-row tiles to pay: with the few rows
    # of a KV-cache step the two launches are faster (0.143 vs 0.163 ms per step at cfg2), hence the row threshold.
    mlp_fc1: bool
    # ... and the row pass in front of it (info-bottleneck add + AdaLN_2 / LayerNorm) as that launch's prologue: a workgroup owns its 32 rows from the
    # fp32 residual stream to the activated hidden rows.  Measured (graph replay): cfg2 0.2472 -> 0.2440 ms (the launch itself 27.4 -> 31.2-32.2 us: its
    # loads sit in front of the weight stream; the row pass it replaces is 7.8 us), B = 8 1.127 -> 1.138 ms (142 -> 171 us per launch against a 32 us row
    # pass that runs at HBM speed) — used for short launches only.  SEA_PLAN=mlpnorm=0 / 1 forces.
    mlp_norm_in: bool
    # The two fused launches as ONE (sea_mlp_block: the activated hidden rows stay in the owning workgroup's registers; no hg matrix, one launch boundary less, the
    # x + ib rows are not written back — the block's residual is formed from x and ib again).  Short launches, where both halves are fused.  SEA_PLAN=mlpblock=0 keeps two launches.
    # Long launches too (B = 8, M = 16192: 262 us against ib_add 30 + AdaLN_2 30 + fc1 + LN + GELU 160 + fc2 88 + proj + norm 55), there always with the norm
    # prologue: the row pass it replaces and the hidden rows it keeps to itself are 0.6 GB of traffic.
    mlp_block: bool
    # fc2 + residual, proj and — after the last layer — the model's final norm in one launch where the kernel is instantiated (the same shapes as the
    # fc1 kernel): a workgroup owns 32 complete rows through both Linear layers.  Measured (plain replay, same box): cfg2 0.2373 -> 0.2358 ms (the launch
    # 30.8 us against 19.8 + 7.1 + 5.6 with two boundaries less: a 32-row workgroup per CU streams W2 at a third of the rate three co-resident 64 x 64
    # tiles do), B = 8 1.108 -> 1.18 ms (200 us against 76 + 21 + 31) — short launches only.  SEA_PLAN=mlp2=0 / 1 forces.
    mlp_fc2_proj: bool
    # Linear + the row norm that follows it in one launch (sea_gemm_rownorm) where a tile can span the whole output row: cross_down + ln_cross,
    # the last layer's proj + the model's final norm.  SEA_PLAN=norm=0 keeps the two-launch form (A/B measurements).
    down_norm: bool      # cross_down + ln_cross (inference and training plans)
    # the last layer's proj + the model's final norm in one launch (sea_gemm_rownorm: a tile spans the whole output row): at B = 8 two launches of 23 + 31 us
    # (the norm re-reads the rows the proj has just written: 100 MB) -> one.  SEA_PLAN=norm=0 / projnorm=0 keep the two launches.
    proj_norm: bool
    splitk: bool         # SEA_PLAN=splitk=0 keeps the single launch where engine.Plan._gemm_splitk would split a long contraction
    # The condition memo of the one-launch front: the AdaLN modulation rows are functions of one condition scalar per row and the weights, and
    # in a rollout's recompute loop, a repeated window or a graph replay the conditions of (nearly) all rows are those of the forward before.  The plan keeps the
    # AdaLN_0 modulation rows, a stamp {condition bits, weight epoch} per row and the ln_cross modulation between forwards; a workgroup of sea_adaln_qkv whose 32
    # stamps match what it sees skips cond_mlp.2 of AdaLN_0 and of ln_cross (two thirds of the launch's weight stream).  Decided on the device, by value.
    # Where front_chain and riders; SEA_PLAN=cond_memo=0 switches it off (the reference form of tests/test_cond_memo_gpu.py).  Not part of a PlanForms'
    # equality: it changes no launch, only optional pointers of one.
    cond_memo: bool = field(default=False, compare=False)
    # ... taken down to the RIDER TILES of the chain launches: every 128 x 128 tile of cond_mlp.2 of AdaLN_2 and of the final norm keeps a
    # stamp set of its own and exits when the conditions of its rows and the weight epoch are those it stamped; the modulation and hidden-row buffers of these
    # modules persist between forwards.  In force only together with cond_memo (SEA_PLAN=cond_memo=0 switches off both); SEA_PLAN=rider_memo=0 leaves the tiles'
    # pointers NULL and keeps the front memo (the A/B lever).  Like cond_memo it changes no launch and is not part of a PlanForms' equality.
    rider_memo: bool = field(default=False, compare=False)

    @property
    def one_launch_front(self) -> bool:
        return self.front_big or self.front_chain


def resolve_forms(model, B: int, T: int, mode: str, dt: torch.dtype, kind: str = INFERENCE, hoisted: bool = False, hoisted_ib: bool = False,
                  plan_switches: Optional[Dict[str, str]] = None, kv_switches: Optional[Dict[str, str]] = None) -> PlanForms:
    """The forms of one plan.  `model`: anything with TemporalModel's structural attributes; `hoisted`: the condition MLPs of all steps were evaluated up
    front (a step plan over a kv_engine.CondPlan), `hoisted_ib`: ... and the info-bottleneck rows of every layer too; the switches default to the
    environment's SEA_PLAN / SEA_KV, read here once per plan build (tests change them between builds)."""
    assert kind in (INFERENCE, TRAINING, CONDITION)
    sw = (_switches.parse("SEA_PLAN") if plan_switches is None else plan_switches).get
    kvsw = (_switches.parse("SEA_KV") if kv_switches is None else kv_switches).get
    inference = kind == INFERENCE
    F, H, L = model.num_variables, model.n_heads, model.num_layers
    Eo, E, D, S, M = model.embed_dim, model.internal_embed_dim, model.down_dim, model.mlp_hidden, B * T
    xmode, ib_add = model.exchange_mode, model.ib_addition_mode.lower()
    has_ib, ib_attn, concat = ib_add == "add", ib_add == "attention", ib_add == "concat"
    after, adaln = bool(model.add_info_after_cross), model.LN_type.lower() == "adaln"

    lane_mode = sw("lanes", "auto") if inference and xmode == "sea" and has_ib else "none"
    if lane_mode == "auto":
        lane_mode = "cond" if M >= 8192 else "none"
    lanes = lane_mode == "all" and F >= 2 and after
    split_cond = lane_mode in ("cond", "all") and adaln
    fuse_norm = inference and sw("norm", "1") != "0"
    chain = (inference and mode == "full" and xmode == "sea" and 1 < F <= 3 and fuse_norm and not lanes and not concat
             and sw("chain", "1") != "0" and sw("xtail", "1") != "0" and ops.row_chain_supported(dt, D, E, F - 1, D // H)
             and M <= int(sw("chain_max_rows", "4096")))
    riders = (chain and adaln and L == 1 and not split_cond and sw("riders", "1") != "0"
              and (not has_ib or (after and E <= 2048)) and not ib_attn and F + F <= N.CHAIN_MAX_RIDERS)
    caps = sw("rider_caps", "") if riders else ""
    want = sw("silu", "auto")
    gen_a = inference and 2 * max(E, D) <= 1024 and (want == "1" or (want == "auto" and M >= 8192))   # (every module is E, D or Eo <= E wide)
    fold_ib = (inference and has_ib and after and adaln and not lanes and L <= N.MAX_SILU_IB and E <= 2048 and sw("fold_ib", "1") != "0"
               and (riders or (gen_a and sw("fold_ib_gen", "0") != "0") or (not gen_a and not split_cond)))
    hoist_ib = hoisted and hoisted_ib and has_ib and after and E <= 2048
    ib_rows_here = fold_ib and not hoist_ib
    xtail = (fuse_norm and not lanes and xmode == "sea" and F > 1 and sw("xtail", "1") != "0"
             and ops.exchange_tail_supported(dt, D, E, F - 1) and M <= int(sw("xtail_max_rows", "1000000000")))
    few = (inference and mode == "step" and T == 1 and xmode == "sea" and not concat and not ib_attn
           and kvsw("gemv", "1") != "0" and 2 * (F - 1) <= N.FEW_MAX_GROUPS and F <= N.FEW_MAX_GROUPS
           and ops.fewrows_supported(dt, M, [E], qkv=True, pre=True) and ops.fewrows_supported(dt, M, [S])
           and (F == 1 or ops.fewrows_supported(dt, M, [D], qkv=True, pre=True)))

    # the one-launch fronts: full-context plans that evaluate their condition MLPs themselves (never together with `few`, a step plan's form)
    aqkv = ops.adaln_qkv_supported(dt, E, H) and F <= N.MAX_AQKV_GROUPS and not concat
    adaln_front = riders and not hoisted and sw("adaln_gemm", "1") != "0"
    front_chain = adaln_front and sw("front", "1") != "0" and aqkv
    front3 = (front_chain and D == 128 and F + F <= N.AQKV_MAX_SILU and (L if ib_rows_here else 0) <= 1   # (the modules further down: AdaLN_2 and the final norm of every field)
              and sw("front3", "1") != "0")
    front_big = (inference and adaln and not hoisted and not riders and mode == "full" and sw("front_big", "0") == "1" and aqkv and M >= 1024)

    # the field MLP: one call for all fields, or — lanes — one per field
    mlp_ok = ops.mlp_fc1_supported(dt, E, S) and (1 if lanes else F) <= N.MAX_MLP_GROUPS
    w1, wn, w2 = sw("mlp1", "auto"), sw("mlpnorm", "auto"), sw("mlp2", "auto")
    mlp_fc1 = inference and w1 != "0" and (w1 == "1" or M >= 1024) and mlp_ok
    mlp_norm_in = mlp_fc1 and (wn == "1" or (wn == "auto" and M <= 4096))
    mlp_block = (mlp_fc1 and inference and (w2 == "1" or (w2 == "auto" and 1024 <= M)) and mlp_ok and Eo == E and sw("mlpblock", "1") != "0")
    if mlp_block:
        mlp_norm_in = mlp_norm_in or (M > 4096 and wn != "0")
    mlp_fc2_proj = not mlp_block and inference and (w2 == "1" or (w2 == "auto" and 1024 <= M <= 4096)) and mlp_ok and Eo == E

    return PlanForms(
        lanes=lanes, split_cond=split_cond, chain=chain, riders=riders, rider_caps=(tuple(int(v) for v in caps.split(":")) if caps else None),
        gen_a=gen_a, fold_ib=fold_ib or hoist_ib, hoist_ib=hoist_ib, ib_rows_here=ib_rows_here, xtail=xtail, few=few, few_fold_ln=S <= 8192,
        hidden_pad=(64 if inference and S % 1024 == 0 else 0), front_chain=front_chain, front3=front3, adaln_front=adaln_front, front_big=front_big,
        mlp_fc1=mlp_fc1, mlp_norm_in=mlp_norm_in, mlp_block=mlp_block, mlp_fc2_proj=mlp_fc2_proj,
        down_norm=(fuse_norm if inference else kind == TRAINING and sw("norm", "1") != "0") and D <= 256 and D % 16 == 0,
        proj_norm=fuse_norm and Eo <= 256 and Eo % 16 == 0 and Eo == E and sw("projnorm", "1") != "0", splitk=sw("splitk", "1") != "0",
        cond_memo=front_chain and riders and sw("cond_memo", "1") != "0", rider_memo=front_chain and riders and sw("rider_memo", "1") != "0")
