"""Whole-model execution engine for TemporalModel on MI355X.

The reference runs TemporalModel.forward (models/temporal.py:405-416) as ~130 eager ATen calls per layer from Python
loops.  Here the same computation is a PLAN: a fixed list of ~30 grouped kernel launches per layer over
pre-allocated HBM workspaces, with every ABI struct filled once (include/sea_hip.h).  A plan is replayed either launch by
launch (a few microseconds of ctypes per launch) or, for the hot loops, as a captured HIP graph.

Memory layout (all in HBM, allocated through torch):
  * parameters: ONE fp32 buffer `flat32`; every nn.Parameter of the model is a view into it (the reference's state_dict
    schema is unchanged).  Live parameters first, the ~12 % that never receive a gradient at the tail, so
    the optimizer and the gradient all-reduce run over one contiguous prefix.  q/k/v weights of an attention module are
    adjacent in q,k,v order, so the fused [3E, E] projection is a plain view.
  * `flat_act`: the same layout in the activation dtype (bf16 shadow; aliases flat32 in fp32 mode).
  * residual stream: fp32 [M, E] per field (M = B*T rows); matrix-operand activations in the activation dtype.
  * Q [B,H,T,hd], K [B,H,cap,hd], V^T [B,H,hd,cap] per attention problem (written by the QKV epilogue).
"""
from __future__ import annotations

import os

import ctypes as C
import re
from typing import Dict, List, Optional, Tuple

import torch

from . import _native as N
from . import _switches
from . import ops
from . import ptrcheck
from .plan_forms import INFERENCE, resolve_forms

_QKV = re.compile(r"^(.*\.)(k|q|v)\.(weight|bias)$")
_QKV_RANK = {("q", "weight"): 0, ("k", "weight"): 1, ("v", "weight"): 2, ("q", "bias"): 3, ("k", "bias"): 4, ("v", "bias"): 5}


# Plan-only keys of a group dict (Plan._bind): the byte offset of a struct field into the caller's x / out / dout tensor, patched at bind time
_BIND_KEYS = {"X_is_x": ("_x_patches", "X"), "R_is_x": ("_x_patches", "R"), "Xin_is_x": ("_x_patches", "Xin"), "Y_is_out": ("_out_patches", "Y32"),
              "dY_is_dout": ("_dout_patches", "dY")}


# what the KV-cache rollout refuses (TemporalEngine.plan / rollout_kv, and a rollout session before it is opened: rollout_session.check_open)
KV_NO_POOL = ("sea_amd: the KV-cache rollout does not cover exchange_mode='pool' (its sinusoidal positions are relative to the window); "
              "use the recompute rollout")
KV_NO_IB_ATTENTION = ("sea_amd: the KV-cache rollout does not cover ib_addition_mode='attention' (every row attends to the info-bottleneck rows "
                      "of ALL positions of the window, later ones included: rows already produced change as the window grows); use the recompute rollout")
KV_NO_SRC_LEN = "sea_amd: the KV-cache rollout is exact only for src_len == 0; use the recompute rollout (rollout(..., mode='recompute'))"


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def dead_prefixes(model) -> List[str]:
    """Parameter-name prefixes that never receive a gradient on this path: the unused middle AdaLN of every field, `ln.cross`, the
    diagonal cross-attention modules, the info-bottleneck's residual projection — and, per variant, the whole info-bottleneck layer when its output is
    not added (ib_addition_mode 'none': the reference still evaluates it, models/temporal.py:112-114) and the fixed random matrix of the Fourier form
    (models/base_blocks.py:147: requires_grad=False)."""
    out = []
    ib_none = model.ib_addition_mode.lower() == "none"
    for layer in range(model.num_layers):
        pre = f"blocks.{layer}."
        out += [pre + "ln.cross.", pre + "ib.residual_projection."]
        if ib_none:
            out.append(pre + "ib.")
        elif model.ib_scale_mode.lower() == "fourier":
            out.append(pre + "ib.W")
        for i in range(model.num_variables):
            out += [f"{pre}ln.exp.{i}.1.", f"{pre}cross_attn.{i}.{i}."]
        if model.exchange_mode == "pool":   # the 'mlp' pool update ignores its token argument (models/temporal.py:244-249): the token and its norm are never used
            out += [pre + "pool_token", pre + "ln_pool."]
    return out


def grad_phase(model, name: str) -> int:
    """When a parameter's gradient is FINAL in the hand-written backward, as an ordinal (lower = earlier): per layer, last layer first —
    0: the field MLP + proj; 1: everything between them and the self-attention (exchange, ln_cross, the norm in front of the MLP, the info-bottleneck step
    behind the exchange; with the last layer: the model's final norms); 2: self-attention, the norm in front of it, an info-bottleneck step in front of
    the block.  The flat buffers are laid out in this order, so that what a data-parallel step can reduce early is ONE contiguous slice per phase
    (train_engine.TrainPlan.grad_buckets)."""
    L = model.num_layers
    m = re.match(r"^blocks\.(\d+)\.(.*)$", name)
    if not m:
        return 1   # ln.{i}.*: with the last layer's middle phase
    l, rest = int(m.group(1)), m.group(2)
    if rest.startswith("mlp.") or rest.startswith("proj."):
        sub = 0
    elif rest.startswith("attn.self.") or re.match(r"^ln\.exp\.\d+\.0\.", rest):
        sub = 2
    elif (rest.startswith("ib.") or rest.startswith("cross_attn_ib.")) and not model.add_info_after_cross:
        sub = 2
    else:
        sub = 1
    return (L - 1 - l) * 3 + sub


def _kv_pairs(src: dict, dst: dict):
    """((K, V^T) of plan `src`, (K, V^T) of plan `dst`) for every self-attention module and cross-attention pair of the model (Plan.kv)."""
    for l in range(len(src["Ks"])):
        for i in range(len(src["Ks"][l])):
            yield (src["Ks"][l][i], src["Vs"][l][i]), (dst["Ks"][l][i], dst["Vs"][l][i])
            if src["Kc"] is not None:
                for j in range(len(src["Kc"][l][i])):
                    if j != i:
                        yield (src["Kc"][l][i][j], src["Vc"][l][i][j]), (dst["Kc"][l][i][j], dst["Vc"][l][i][j])


class _WatchedParameter(torch.nn.Parameter):
    """The class FlatParams gives the model's parameters: `p.data` hands out a tensor with a version counter of its own, so an in-place write through it
    (`p.data.mul_(s)`, `p.data.copy_(w)`: the usual way to edit a weight) moves neither flat32._version nor p._version and nothing on the host could see
    it.  Here every READ of `.data` is counted, process-wide; a FlatParams whose count is behind takes the weights as possibly changed: its next sync()
    refreshes the shadow and moves the weight epoch on.  A read that wrote nothing costs one redundant conversion (in every engine of the process: the
    parameter holds no reference to its store, so it pickles and copies like any other).  Nothing in this package reads `.data`."""
    reads = 0

    @property
    def data(self):
        _WatchedParameter.reads += 1
        return torch.Tensor.data.__get__(self)

    @data.setter
    def data(self, value):
        torch.Tensor.data.__set__(self, value)


class FlatParams:
    """One contiguous fp32 buffer holding every parameter of the model (+ the activation-dtype shadow)."""

    def __init__(self, model: torch.nn.Module, device: torch.device, act_dtype: torch.dtype):
        named = list(model.named_parameters())
        first_idx: Dict[str, int] = {}
        keyed = []
        for idx, (name, p) in enumerate(named):
            m = _QKV.match(name)
            if m:
                base = first_idx.setdefault(m.group(1), idx)
                keyed.append(((base, _QKV_RANK[(m.group(2), m.group(3))]), name, p))
            else:
                keyed.append(((idx, 0), name, p))
        dead = dead_prefixes(model)
        is_dead = lambda n: any(n.startswith(d) for d in dead)  # noqa: E731
        keyed.sort(key=lambda t: (is_dead(t[1]), grad_phase(model, t[1]), t[0]))
        self.offsets: Dict[str, Tuple[int, Tuple[int, ...]]] = {}
        off = 0
        self.n_live = 0
        for _, name, p in keyed:
            if is_dead(name) and self.n_live == 0 and off > 0:
                self.n_live = off
            self.offsets[name] = (off, tuple(p.shape))
            off += _round_up(p.numel(), 8)
        if self.n_live == 0:
            self.n_live = off
        self.n_total = off
        self.device, self.act_dtype = device, act_dtype
        self.flat32 = torch.zeros(self.n_total, device=device, dtype=torch.float32)
        with torch.no_grad():
            for _, name, p in keyed:
                o, shp = self.offsets[name]
                view = self.flat32[o:o + p.numel()].view(shp)
                view.copy_(p.detach().to(device=device, dtype=torch.float32))
                p.data = view  # the module's parameter now aliases the flat buffer
                if type(p) is torch.nn.Parameter:
                    p.__class__ = _WatchedParameter
        self._data_reads = _WatchedParameter.reads   # reads of a parameter's `.data` seen by the last sync
        self.live_names = [n for _, n, _ in keyed if not is_dead(n)]
        self.phase_of = {n: grad_phase(model, n) for _, n, _ in keyed if not is_dead(n)}
        self.flat_act = self.flat32 if act_dtype == torch.float32 else torch.empty(self.n_total, device=device, dtype=act_dtype)
        self.flat_actT: Optional[torch.Tensor] = None   # transposed weight shadow, built on first training use
        self._t_desc = self._t_tiles = None
        self._t_total = 0
        self._synced_version = -1
        self._synced_T_version = -1
        # the weight epoch of the condition memo (plan_forms.PlanForms.cond_memo): a DEVICE word the kernels read themselves — a captured graph bakes kernel
        # arguments in, not what a pointer leads to.  Starts at 1: a zeroed stamp matches no epoch.  weights_changed() is its only writer
        self.memo_epoch = torch.ones(1, device=device, dtype=torch.int32)
        self.sync()

    # -- views
    def f32(self, name: str) -> torch.Tensor:
        o, shp = self.offsets[name]
        n = 1
        for s in shp:
            n *= s
        return self.flat32[o:o + n].view(shp)

    def act(self, name: str, rows: Optional[int] = None) -> torch.Tensor:
        """Activation-dtype view of a 2-D weight; rows > shape[0] extends over the adjacent tensors (fused q|k|v)."""
        o, shp = self.offsets[name]
        r = shp[0] if rows is None else rows
        return self.flat_act[o:o + r * shp[1]].view(r, shp[1])

    def f32_vec(self, name: str, n: Optional[int] = None) -> torch.Tensor:
        o, shp = self.offsets[name]
        k = shp[0] if n is None else n
        return self.flat32[o:o + k]

    # -- transposed shadow (operand of the data-gradient GEMMs: dX = dY . W needs W^T in the K-contiguous [N,K] form)
    def enable_transposed_shadow(self) -> None:
        if self.flat_actT is not None:
            return
        rows = []
        fused_done = set()
        for name, (o, shp) in self.offsets.items():
            if len(shp) != 2 or shp[1] == 1 or ".ib." in name:
                continue
            m = _QKV.match(name)
            if m and m.group(3) == "weight":
                pre, which = m.group(1), m.group(2)
                is_self = ".attn.self." in pre
                if is_self:
                    if which == "q":
                        rows.append((o, o, 3 * shp[0], shp[1]))      # [q;k;v] as one [3E, E] matrix
                    continue
                if which == "q":
                    rows.append((o, o, shp[0], shp[1]))
                elif which == "k":
                    rows.append((o, o, 2 * shp[0], shp[1]))          # [k;v] as one [2D, D] matrix
                continue
            rows.append((o, o, shp[0], shp[1]))
        desc = torch.tensor(rows, dtype=torch.int64)
        tiles = ((desc[:, 2] + 31) // 32) * ((desc[:, 3] + 31) // 32)
        ts = torch.zeros(len(rows) + 1, dtype=torch.int32)
        ts[1:] = torch.cumsum(tiles, 0).to(torch.int32)
        self._t_total = int(ts[-1])
        self._t_desc, self._t_tiles = desc.to(self.device), ts.to(self.device)
        self.flat_actT = torch.zeros(self.n_total, device=self.device, dtype=self.act_dtype)
        self.sync_transposed(force=True)

    def sync_transposed(self, force: bool = False) -> None:
        if self.flat_actT is None:
            return
        v = self.flat32._version
        if force or v != self._synced_T_version:
            N.check(N.lib().sea_transpose_weights(self.flat32.data_ptr(), self.flat_actT.data_ptr(), N.dtype_code(self.act_dtype),
                                                  self._t_desc.data_ptr(), self._t_tiles.data_ptr(), self._t_desc.shape[0], self._t_total,
                                                  N.stream_ptr()), "weight transpose")
            self._synced_T_version = v

    def actT(self, name: str, rows: Optional[int] = None) -> torch.Tensor:
        """Activation-dtype view of W^T for the weight `name` ([rows, cols] in the model, possibly fused over adjacent tensors)."""
        o, shp = self.offsets[name]
        r = shp[0] if rows is None else rows
        return self.flat_actT[o:o + r * shp[1]].view(shp[1], r)

    def sync(self, force: bool = False) -> None:
        """Refresh the activation-dtype shadow if any parameter view was modified in place since the last sync."""
        if self.act_dtype == torch.float32:
            return
        v = self.flat32._version
        if force or v != self._synced_version or self._data_reads != _WatchedParameter.reads:
            self._data_reads = _WatchedParameter.reads
            N.check(N.lib().sea_convert_f32_to_act(self.flat32.data_ptr(), self.n_total, self.flat_act.data_ptr(), self.n_total, 1,
                                                   self.n_total, N.dtype_code(self.act_dtype), N.stream_ptr()), "weight shadow")
            self._synced_version = v
            self.weights_changed()   # (the fp32 vectors the kernels read from flat32 itself moved the version too)

    def weights_changed(self) -> None:
        """Every writer of the activation shadow `flat_act` calls this behind its write, on the launch stream: sync() above when it converts, and the two AdamW
        launches of optim.FlatAdamW.step, which write the shadow through raw pointers.  One tiny device write moves the weight epoch on; a row stamped under
        an older epoch no longer matches (adaln_qkv.hip), so every memoised condition product is computed again from the new weights.  (The word wraps to 0,
        the epoch of a zeroed stamp, after 2^32 updates.)"""
        self.memo_epoch.add_(1)


class _Rec:
    """One pre-built launch: C function + argument list (the stream is appended at run time).  `lane` selects the stream of a
    concurrent replay (0 = the caller's stream); fn None marks a lane fork / join (name "fork" / "join")."""
    __slots__ = ("fn", "args", "name", "keep", "lane")

    def __init__(self, fn, args, name, keep=None, lane=0):
        self.fn, self.args, self.name, self.keep, self.lane = fn, list(args), name, keep, lane


class _Riders:
    """The rider work of a plan's chain launches (sea_row_chain_riders): cond_mlp.2 of the modules the field MLP and the final norm read, as 128 x 128 tiles of one
    grouped GEMM handed out to the `hosts` chain launches that may carry riders (the one behind the self-attention and the tails of the fields that are not
    last: their results are read by the MLP)."""

    def __init__(self, arr, tiles: int, hosts: int, caps: Optional[Tuple[int, ...]], memo: Optional[dict] = None):
        self.arr, self.tiles, self.done = arr, tiles, 0
        self.memo = memo                      # forms.rider_memo: the tiles' condition memo (ops.fill_row_chain's tile_memo), one stamp set per tile of the rider GEMM
        self.hosts_total = self.hosts_left = hosts
        self.caps, self.host_no = caps, 0     # PlanForms.rider_caps: tiles for the first, second, third host instead of equal shares

    def take(self):
        """The share of the next chain launch, (group array, groups, first tile, tiles): as many tiles of the rider GEMM as its idle CUs take in about the launch's
        own duration (a chain workgroup owns a CU; two tile rounds under the three-field launch behind the self-attention, one under a field's tail) — equal
        shares, the last host takes what is left.  None when nothing is left."""
        left = self.tiles - self.done
        if left <= 0:
            return None
        if self.caps is not None:
            take = min(left, self.caps[self.host_no] if self.host_no < len(self.caps) else 0)
            self.host_no += 1
        else:
            take = left if self.hosts_left <= 1 else min(left, (self.tiles + self.hosts_total - 1) // self.hosts_total)
            self.hosts_left -= 1
        t0, self.done = self.done, self.done + take
        return self.arr, len(self.arr), t0, take


class Plan:
    """Launch list for one (B, T, mode) of TemporalModel.forward."""
    kind = INFERENCE   # what plan_forms.resolve_forms decides for: the subclasses (TrainPlan, CondPlan) turn the inference-only forms off

    def __init__(self, eng: "TemporalEngine", B: int, T: int, mode: str = "full", save_for_backward: bool = False, cond=None):
        assert mode in ("full", "step")
        self.eng, self.B, self.T, self.mode = eng, B, T, mode
        # `cond` (step mode): a kv_engine.CondPlan that has evaluated what depends on the condition only — every AdaLN modulation, the
        # info-bottleneck term — for ALL steps of a rollout (row s * B + b): the step plan then carries no condition launch at all and reads row
        # block s of those buffers, its pointers into them advanced per step (self._hoisted, step_patch_table)
        self._cond_src = cond
        self._hoisted: List[Tuple[object, str, int, int]] = []   # (struct, field, address at step 0, bytes per step)
        m = eng.model
        self.F, self.H, self.L = m.num_variables, m.n_heads, m.num_layers
        # E: the row width INSIDE a block; Eo: the width of the model's input / output rows and of every block's proj output.  They differ only with
        # ib_addition_mode 'concat' (models/temporal.py:48: rows widened by ib_dim_concat = 64 info-bottleneck columns, `ib_dim` wide layer)
        self.Eo, self.E = m.embed_dim, m.internal_embed_dim
        self.concat = m.ib_addition_mode.lower() == "concat"
        self.ib_dim = self.E - self.Eo if self.concat else self.E
        self.D = m.down_dim
        self.S = m.mlp_hidden
        self.M = B * T
        self.dt = eng.act_dtype
        self.code = N.dtype_code(self.dt)
        self.adaln = m.LN_type.lower() == "adaln"
        self.cap = _round_up(m.max_len, 8) if mode == "step" else _round_up(T, 8)
        self.pos0 = 0
        self.records: List[_Rec] = []
        self._cur: List[_Rec] = self.records   # list the record builders append to (forward or backward)
        self._keep: List[object] = []
        self._x_patches: List[Tuple[object, str, int]] = []   # (struct, field, byte offset from x base)
        self._out_patches: List[Tuple[object, str, int]] = []
        self._c_patches: List[Tuple[object, object]] = []      # (container, key) receiving the condition pointer
        self._pos_structs: List[object] = []                   # SeaQkvCommon / SeaAttnParams to update per step
        self._drop_structs: List[object] = []                  # structs whose .drop.seed is re-keyed every training step
        self._bound = (None, None, None)
        self._bound_tensors = None        # (x, ib, out) of the last bind(): held until the next one (see bind)
        self._audited = False             # the pointer audit has run on this plan (ptrcheck)
        self._lane = 0                    # lane the record builders tag new records with
        self._lane_streams: Dict[int, torch.cuda.Stream] = {}
        self._zero_ib: Optional[torch.Tensor] = None   # 'concat': the zeros the info-bottleneck columns are reset to
        self.forms = resolve_forms(m, B, T, mode, self.dt, self.kind, hoisted=cond is not None, hoisted_ib=cond is not None and len(cond.ibufs) == self.L)
        self._mods: Dict[str, torch.Tensor] = {}        # AdaLN modulations, prefix -> [M, 2d] (_cond_mods)
        self._riders: Optional[_Riders] = None          # rider work of the chain launches (forms.riders)
        self._front = None                              # rider plans: (cond_mlp.2 operands of the front modules, row riders of the one-launch front), see _cond_mods
        self.memo_count: Optional[torch.Tensor] = None  # forms.cond_memo: int32 [2], hits / misses of the condition memo's workgroups (SEA_TUNE=memo_count=1)
        self.memo_tile_count: Optional[torch.Tensor] = None   # forms.rider_memo: int32 [2], hits / misses of the chain launches' rider tiles (SEA_TUNE=memo_count=1)
        self._build()
        self._find_hoisted()
        self._clist = None          # (SeaLaunchRec array, [(rec index, field, args list, args index)]) for sea_run_list
        self._compile_list()

    def _find_hoisted(self) -> None:
        """Every pointer field of the launch structs that points into row block 0 of a hoisted condition buffer (self._cond_src): (struct, field,
        address, bytes per step) — found by address, so that no record builder has to know about the hoisting."""
        src = self._cond_src
        if src is None:
            return
        spans = []   # (lo, hi, bytes per step)
        for t in list(src.mods.values()) + list(src.ibufs):
            step = self.M * t.stride(0) * t.element_size()
            spans.append((t.data_ptr(), t.data_ptr() + step, step))
        for r in self.records:
            if r.fn is None:
                continue
            roots = [a for a in r.args if isinstance(a, (C.Structure, C.Array))] + ([r.keep] if r.keep is not None else [])
            seen = set()
            for root in roots:
                for st in ptrcheck._walk_structs(root):
                    for path, pval in ptrcheck.iter_pointers(st):
                        name = path[1:]
                        if "[" in name or (C.addressof(st), name) in seen:
                            continue
                        for lo, hi, step in spans:
                            if lo <= pval < hi:
                                seen.add((C.addressof(st), name))
                                self._hoisted.append((st, name, pval, step))
                                break
        self._keep.append(src)   # the buffers live as long as this plan

    def set_hoisted_step(self, s: int) -> None:
        """Point the plan at row block s of the hoisted condition buffers (the native step loop does the same through its patch table)."""
        for st, field, base, step in self._hoisted:
            setattr(st, field, base + s * step)

    # ------------------------------------------------------------------ allocation helpers
    def _buf(self, *shape, dtype=None, zero=False) -> torch.Tensor:
        dt = self.dt if dtype is None else dtype
        t = (torch.zeros if zero else torch.empty)(*shape, device=self.eng.device, dtype=dt)
        self._keep.append(t)
        return t

    # ------------------------------------------------------------------ lanes (concurrent replay)
    def _rec(self, fn, args, name, keep=None) -> _Rec:
        return _Rec(fn, args, name, keep, self._lane)

    def _fork(self, lane: int) -> None:
        """Records built until the matching _join run on `lane`: in a concurrent replay that stream first waits for everything
        the main stream has been given so far, then runs beside it."""
        assert self._lane == 0 and lane > 0
        self._cur.append(_Rec(None, [], "fork", None, lane))
        self._lane = lane

    def _end_lane(self) -> None:
        self._lane = 0

    def _join(self, lane: int) -> None:
        """The main stream waits for everything given to `lane`."""
        assert self._lane == 0
        self._cur.append(_Rec(None, [], "join", None, lane))

    # ------------------------------------------------------------------ record builders
    def _bind(self, g, d: dict) -> dict:
        """d without its plan-only keys (_BIND_KEYS), each registered as a bind-time patch of struct g; a generated operand (`silu`), an
        info-bottleneck addend (`ib`) and dropout (`drop`) register g for the condition pointer and the per-step seed."""
        d = dict(d)
        for key, (patches, field) in _BIND_KEYS.items():
            off = d.pop(key, None)
            if off is not None:
                getattr(self, patches).append((g, field, off))
        if d.get("silu") is not None:
            self._c_patches.append((g, "silu_c"))
        if d.get("ib") is not None:
            self._c_patches.append((g, "ib_c"))
        if d.get("drop") is not None:
            self._drop_structs.append(g)
        return d

    def _array(self, struct, groups: List[dict], fill):
        """One launch's struct array: fill(g, **d) per group dict (see _bind)."""
        arr = (struct * len(groups))()
        for g, d in zip(arr, groups):
            fill(g, **self._bind(g, d))
        return arr

    def _grouped(self, fn, struct, groups: List[dict], limit: int, fill, name: str, *tail) -> None:
        """Launches fn(arr, n, *tail) over the groups, at most `limit` per launch."""
        for s in range(0, len(groups), limit):
            arr = self._array(struct, groups[s:s + limit], fill)
            self._cur.append(self._rec(fn, [arr, len(arr), *tail], name, arr))

    def _gemm_splitk(self, chunk: List[dict], name: str) -> bool:
        """Split-K form of a launch of skinny-M Linear layers with a very long contraction (the MLP of configs/multiphase_flow.py:112-141 at M = B T = 796: fc2 forward and
        fc1's data gradient, 2048 x 16384): at 128 x 128 tiles such a launch is 224 workgroups each walking K = 16384 alone; four K-quarters as groups of ONE
        sea_gemm_grouped launch (fp32 partial matrices, two workgroups per CU on the two-stage ring) + sea_splitk_finish: 161 -> 128 + 10 us (tools/skinny_probe.py).
        bf16, plain epilogue (bias / residual / outputs only).  SEA_PLAN=splitk=0 keeps the single launch."""
        S = 4
        if self.dt != torch.bfloat16 or not self.forms.splitk or len(chunk) * S > N.MAX_GROUPS or len(chunk) > N.MAX_SPLITK_GROUPS:
            return False
        tiles = 0
        for d in chunk:
            A, W = d.get("A"), d["W"]
            if (A is None or d.get("silu") is not None or d.get("act", 0) != 0 or d.get("drop") is not None or d.get("n_seg", 1) != 1 or d.get("Z") is not None
                    or d.get("R_is_x") is not None or d.get("ldr") is not None or d.get("ldc32") is not None or d.get("M") is not None):
                return False
            Mg, Ng, Kg = A.shape[-2], W.shape[0], W.shape[1]
            if Kg < 8192 or Kg % (S * 64) != 0 or Mg > 1024 or Ng % 4 != 0 or A.dim() != 2:
                return False
            tiles += ((Mg + 127) // 128) * ((Ng + 127) // 128)
        if tiles >= 384:
            return False
        parts, fin = [], []
        for d in chunk:
            A, W = d["A"], d["W"]
            ks = W.shape[1] // S
            P = self._buf(S, A.shape[0], W.shape[0], dtype=torch.float32)
            for q in range(S):
                parts.append(dict(A=A[:, q * ks:(q + 1) * ks], W=W[:, q * ks:(q + 1) * ks], C32=P[q]))
            fin.append(dict(P=P, bias=d.get("bias"), bias_scale=d.get("bias_scale", 1.0), R=d.get("R"), C32=d.get("C32"), Cact=d.get("Cact")))
        L = N.lib()
        self._grouped(L.sea_gemm_grouped, N.SeaGemmGroup, parts, N.MAX_GROUPS, ops.fill_gemm_group, name + ".splitk", self.code)
        self._grouped(L.sea_splitk_finish, N.SeaSplitkGroup, fin, N.MAX_SPLITK_GROUPS, ops.fill_splitk_group, name, self.code)
        return True

    def _gemm(self, groups: List[dict], name: str) -> None:
        """Group dicts: the arguments of ops.fill_gemm_group, plus `R_is_x`; a dropout's seed (drop[0]) is re-keyed every step (set_dropout_seed)."""
        for s in range(0, len(groups), N.MAX_GROUPS):
            chunk = groups[s:s + N.MAX_GROUPS]
            if not self._gemm_splitk(chunk, name):
                self._grouped(N.lib().sea_gemm_grouped, N.SeaGemmGroup, chunk, N.MAX_GROUPS, ops.fill_gemm_group, name, self.code)

    def _norm(self, groups: List[dict], d: int, name: str, x_is_act=False, gelu=False) -> None:
        """Group dicts: those of ops.fill_norm_group, plus `X_is_x` and `Y_is_out`."""
        self._grouped(N.lib().sea_rownorm, N.SeaNormGroup, groups, N.MAX_NORM_GROUPS, lambda g, **gd: ops.fill_norm_group(g, gd), name,
                      self.M, d, int(x_is_act), int(gelu), 1e-5, self.code)

    def _norm_specs(self, specs, n: int):
        """SeaNormGroup array of the `pre` specs of a few-row launch (None entries: no norm for that group), with the bind-time patches of _norm."""
        if specs is None or all(sp is None for sp in specs):
            return None
        arr = (N.SeaNormGroup * n)()
        for g, sp in zip(arr, specs):
            if sp is not None:
                ops.fill_norm_group(g, self._bind(g, sp))
        return arr

    def _gemm_few(self, groups: List[dict], name: str, pre=None, pre_act: bool = False, pre_gelu: bool = False) -> None:
        """sea_gemm_fewrows (step plans at the shipped widths): group dicts as _gemm; pre[i]: the _norm group dict (or None) of the row norm in front of the layer.
        Groups with pre[i] carry no A."""
        n = len(groups)
        assert n <= N.FEW_MAX_GROUPS
        arr = self._array(N.SeaGemmGroup, groups, lambda g, A=None, **d: ops.fill_gemm_group(g, A, M=self.M, **d))
        pa = self._norm_specs(pre, n)
        self._cur.append(self._rec(N.lib().sea_gemm_fewrows, [arr, pa, n, int(pre_act), int(pre_gelu), 1e-5, self.code], name, (arr, pa)))

    def _qkv_common(self, rope: torch.Tensor, hd: int):
        """The SeaQkvCommon of a launch of this plan, its position updated per step (set_position)."""
        common = N.SeaQkvCommon(rope.data_ptr(), self.H, hd, self.T, self.pos0, self.cap, ops.q_scale(hd))
        self._pos_structs.append(common)
        return common

    def _qkv_few(self, groups: List[dict], rope: torch.Tensor, hd: int, name: str, pre=None) -> None:
        """sea_qkv_rope_fewrows: group dicts as _qkv; pre[i]: the _norm group dict of the row norm in front of the projection (or None)."""
        n = len(groups)
        assert n <= N.FEW_MAX_GROUPS
        arr = self._array(N.SeaQkvGroup, groups, lambda g, A=None, **d: ops.fill_qkv_group(g, A, M=self.M, **d))
        pa = self._norm_specs(pre, n)
        common = self._qkv_common(rope, hd)
        self._cur.append(self._rec(N.lib().sea_qkv_rope_fewrows, [arr, pa, n, C.byref(common), 1e-5, self.code], name, (arr, pa, common)))

    def _gemm_norm(self, groups: List[dict], name: str) -> None:
        """Linear + row normalisation in one launch (sea_gemm_rownorm): group dicts as ops.fill_gemm_norm_group, plus `Y_is_out`."""
        self._grouped(N.lib().sea_gemm_rownorm, N.SeaGemmNormGroup, groups, N.MAX_GEMM_NORM_GROUPS, ops.fill_gemm_norm_group, name, 1e-5, self.code)

    def _xtail(self, att, Wp, Wup, bup, bias_scale, X, down, name: str) -> None:
        """One field's exchange tail in one launch (sea_exchange_tail): projections + GELU, up-projection of their sum + residual, and — `down` —
        the down-projection + row norm of the updated rows."""
        P = (N.SeaExchangeTail * 1)()
        ops.fill_exchange_tail(P[0], att, Wp, Wup, bup, bias_scale, X, None, down)
        self._cur.append(self._rec(N.lib().sea_exchange_tail, [P, 1, 1e-5, self.code], name, P))

    def _adaln(self, groups: List[dict], name: str) -> None:
        """AdaLN as the epilogue of cond_mlp.2's GEMM, and plain cond_mlp.2 groups, in one launch (sea_gemm_adaln): dicts as ops.fill_adaln_group, plus `X_is_x`
        (byte offset into the caller's tensor: the rows of the first layer are read from it, strided) and `Y_is_out`."""
        self._grouped(N.lib().sea_gemm_adaln, N.SeaAdalnGroup, groups, N.MAX_ADALN_GROUPS, ops.fill_adaln_group, name, 1e-5, self.code)

    def _chain(self, groups: List[dict], rope: torch.Tensor, hd: int, name: str) -> None:
        """A row-local chain between two attention launches (sea_row_chain): group dicts as ops.fill_row_chain, plus `Xin_is_x` (byte offset into the caller's
        tensor: the residual rows of the first layer are read from it, strided)."""
        for s in range(0, len(groups), N.CHAIN_MAX_GROUPS):
            chunk = groups[s:s + N.CHAIN_MAX_GROUPS]
            rd = self._riders.take() if s == 0 and self._riders is not None else None
            memo = self._riders.memo if rd is not None and rd[3] > 0 else None   # the tiles' condition memo travels in group 0 (forms.rider_memo)
            if memo is not None:
                chunk = [dict(chunk[0], tile_memo=memo)] + chunk[1:]
            arr = self._array(N.SeaRowChain, chunk, ops.fill_row_chain)
            if memo is not None:
                self._c_patches.append((arr[0], "tile_cond"))   # the condition pointer, patched at every bind as the front's row riders' is
            common = self._qkv_common(rope, hd)
            if rd is None:
                self._cur.append(self._rec(N.lib().sea_row_chain, [arr, len(chunk), C.byref(common), 1e-5, self.code], name, (arr, common)))
            else:
                rarr, n_r, t0, nt = rd   # (the launch's information-bottleneck rider is not used: those rows ride in the silu launch / the one-launch front)
                self._cur.append(self._rec(N.lib().sea_row_chain_riders, [arr, len(chunk), C.byref(common), rarr, n_r, t0, nt, None, 1e-5, self.code], name, (arr, common, rarr, None)))

    def _qkv(self, groups: List[dict], rope: torch.Tensor, hd: int, name: str) -> None:
        """Group dicts: the arguments of ops.fill_qkv_group."""
        arr = self._array(N.SeaQkvGroup, groups, lambda g, **d: ops.fill_qkv_group(g, M=self.M, **d))
        common = self._qkv_common(rope, hd)
        self._cur.append(self._rec(N.lib().sea_qkv_rope_grouped, [arr, len(groups), C.byref(common), self.code], name, (arr, common)))

    def _attn(self, problems: List[dict], hd: int, ldo: int, name: str, drop=None, src_len: Optional[int] = None) -> None:
        """drop: (thr, first stream); the seed is re-keyed every step (set_dropout_seed)."""
        for s in range(0, len(problems), N.MAX_ATTN_PROBLEMS):
            P = N.SeaAttnParams()
            ops.fill_attn_params(P, problems[s:s + N.MAX_ATTN_PROBLEMS], self.B, self.H, hd, self.T, self.pos0 + self.T, self.cap, self.pos0,
                                 (self.eng.model.src_len if src_len is None else src_len), ldo, drop=((0, drop[1] + s, drop[0]) if drop is not None else None))
            if drop is not None:
                self._drop_structs.append(P)
            self._pos_structs.append(P)
            self._cur.append(self._rec(N.lib().sea_attention_fwd, [C.byref(P), self.code], name, P))

    def _cond_mods(self, ib_fold=()) -> Dict[str, torch.Tensor]:
        """AdaLN condition MLPs for the WHOLE model: silu launch + grouped GEMM (cond_mlp.2); returns prefix -> [M, 2d] (w | b).
        forms.split_cond: the modules the first launch of the layer needs (AdaLN_0 of layer 0) go first on the main stream, all the others run
        on lane 1 beside the self-attention and are joined by the caller (self._join(1)) before their first use.
        `ib_fold`: (layer prefix, ibuf) — info-bottleneck MLPs evaluated by extra row passes of the first silu launch."""
        P, F, E, D, M, L, fm = self.eng.params, self.F, self.E, self.D, self.M, N.lib(), self.forms
        mods: Dict[str, torch.Tensor] = {}
        if not self.adaln:
            return mods
        if self._cond_src is not None:   # evaluated for all steps up front: row block 0 here, advanced per step
            return {pre: t[:M] for pre, t in self._cond_src.mods.items()}
        first, rest = [], []
        for l in range(self.L):
            pre = f"blocks.{l}."
            for i in range(F):
                (first if l == 0 else rest).append((f"{pre}ln.exp.{i}.0.", E))
                rest.append((f"{pre}ln.exp.{i}.2.", E))
            if self.eng.model.exchange_mode != "simple":
                for i in range(F):
                    rest.append((f"{pre}ln_cross.{i}.", D))
        for i in range(F):
            rest.append((f"ln.{i}.", self.Eo))

        ib_todo = list(ib_fold)

        def silu_launch(chunk, tag):   # sea_silu_outer_ib: the hidden rows of `chunk` (dicts as ops.fill_silu_group) and the info-bottleneck rows still to do
            arr = self._array(N.SeaSiluGroup, chunk, ops.fill_silu_group) if chunk else None
            ibs, n_ib = None, len(ib_todo)
            if ib_todo:
                ibs = (N.SeaIbParams * n_ib)()
                for ibp, (lpre, ibuf) in zip(ibs, ib_todo):
                    ops.fill_ib_params(ibp, [ibuf], None, **self._ib_layer(lpre))
                ib_todo.clear()
            rec = self._rec(L.sea_silu_outer_ib, [arr, len(chunk), None, M, self.code, ibs, n_ib], tag, (arr, ibs) if chunk else (ibs,))
            self._c_patches.append((rec.args, 2))
            self._cur.append(rec)
        if fm.riders:
            # the silu launch as it is (hidden rows of every module + the information-bottleneck rows); cond_mlp.2 of AdaLN_0 and ln_cross of the (only) layer in
            # front; cond_mlp.2 of every other module as rider tiles of the chain launches
            front = first + [(pre_, d) for pre_, d in rest if "ln_cross." in pre_]
            later = [(pre_, d) for pre_, d in rest if (pre_, d) not in front]
            silu_groups, hids = [], {}
            for pre_, d in front + later:
                mods[pre_] = self._buf(M, 2 * d)
                if fm.front_chain and ((pre_, d) in first or (fm.front3 and "ln_cross." in pre_)):
                    continue   # generated inside sea_adaln_qkv
                hids[pre_] = self._buf(M, 2 * d)
                silu_groups.append(dict(w1=P.f32_vec(pre_ + "cond_mlp.0.weight", 2 * d), b1=P.f32_vec(pre_ + "cond_mlp.0.bias"), Hid=hids[pre_]))
            front_rows = None
            if fm.front3:   # the silu / ib rows as row riders of sea_adaln_qkv (emitted by _build)
                sarr = (N.SeaSiluGroup * max(len(silu_groups), 1))()
                for g, gd in zip(sarr, silu_groups):
                    ops.fill_silu_group(g, **gd)
                ibp = None
                if ib_todo:
                    ibp = N.SeaIbParams()
                    lpre, ibuf = ib_todo[0]
                    ops.fill_ib_params(ibp, [ibuf], None, **self._ib_layer(lpre))
                    ib_todo.clear()
                front_rows = (sarr, len(silu_groups), ibp)
                silu_groups = []
            for s_ in range(0, len(silu_groups), N.MAX_SILU_GROUPS):
                silu_launch(silu_groups[s_:s_ + N.MAX_SILU_GROUPS], "adaln.silu")
            # cond_mlp.2 of the front modules: emitted by _build where the AdaLN_0 launch used to be (forms.adaln_front), else as a GEMM here
            if fm.adaln_front:
                self._front = ({pre_: hids.get(pre_) for pre_, _ in front}, front_rows)
            else:
                self._gemm([dict(A=hids[pre_], W=P.act(pre_ + "cond_mlp.2.weight"), bias=P.f32_vec(pre_ + "cond_mlp.2.bias"), Cact=mods[pre_]) for pre_, _ in front], "adaln.cond_gemm.front")
            arr = self._array(N.SeaGemmGroup, [dict(A=hids[pre_], W=P.act(pre_ + "cond_mlp.2.weight"), bias=P.f32_vec(pre_ + "cond_mlp.2.bias"),
                                                    Cact=mods[pre_]) for pre_, _ in later], ops.fill_gemm_group)
            tiles = sum(((M + 127) // 128) * ((2 * d + 127) // 128) for _, d in later)
            memo = None
            if fm.cond_memo and fm.rider_memo:
                # the rider tiles' condition memo: a stamp set per TILE, zeroed once (epoch 0 matches nothing).  A hit leaves the tile's
                # modulation where the last miss stored it and a miss of SOME rows re-reads the hidden rows of all 128: mods[pre_] and hids[pre_] of the later
                # modules are buffers of their own (_buf above), written by the rider tiles / the front's row riders only, and live as long as the plan
                self.memo_tile_count = self._buf(2, dtype=torch.int32, zero=True)
                memo = dict(stamps=self._buf(tiles, 128, 2, dtype=torch.int32, zero=True), epoch=P.memo_epoch, count=self.memo_tile_count)
            self._riders = _Riders(arr, tiles, F, fm.rider_caps, memo)
            self._keep.append(arr)
            return mods

        def emit(inst, tag):
            silu_groups, gemm_groups = [], []
            if fm.gen_a:
                if ib_todo:   # no silu rows to ride on: the information-bottleneck rows as a launch of their own (added by the norm pass in front of the MLP)
                    silu_launch([], "ib.rows")
                for pre, d in inst:
                    mod = self._buf(M, 2 * d)
                    mods[pre] = mod
                    gemm_groups.append(dict(A=None, M=M, W=P.act(pre + "cond_mlp.2.weight"), bias=P.f32_vec(pre + "cond_mlp.2.bias"), Cact=mod,
                                            silu=dict(w1=P.f32_vec(pre + "cond_mlp.0.weight", 2 * d), b1=P.f32_vec(pre + "cond_mlp.0.bias"))))
                self._gemm(gemm_groups, "adaln.cond_gemm" + tag)
                return
            for pre, d in inst:
                hid = self._buf(M, 2 * d)
                mod = self._buf(M, 2 * d)
                mods[pre] = mod
                silu_groups.append(dict(w1=P.f32_vec(pre + "cond_mlp.0.weight", 2 * d), b1=P.f32_vec(pre + "cond_mlp.0.bias"), Hid=hid))
                gemm_groups.append(dict(A=hid, W=P.act(pre + "cond_mlp.2.weight"), bias=P.f32_vec(pre + "cond_mlp.2.bias"), Cact=mod))
            for s in range(0, len(silu_groups), N.MAX_SILU_GROUPS):
                silu_launch(silu_groups[s:s + N.MAX_SILU_GROUPS], "adaln.silu" + tag)
            self._gemm(gemm_groups, "adaln.cond_gemm" + tag)

        if fm.front_big:   # AdaLN_0 of the first layer and its condition MLP are part of the one-launch front (emitted by _build)
            first = []
        if not fm.split_cond:
            emit(first + rest, "")
            return mods
        if first:
            emit(first, ".first")
        self._fork(1)
        emit(rest, ".rest")
        self._end_lane()
        return mods

    # ------------------------------------------------------------------ the plan
    def _build(self) -> None:
        eng, P = self.eng, self.eng.params
        F, E, D, S, M, B, T, H = self.F, self.E, self.D, self.S, self.M, self.B, self.T, self.H
        L = N.lib()
        hd_s, hd_c = E // H, D // H
        cap = self.cap
        f32 = torch.float32

        xmode = eng.model.exchange_mode                                   # 'sea' | 'addition' | 'simple' (models/temporal.py:314-324)
        has_ib = eng.model.ib_addition_mode.lower() == "add"              # 'none': _add_info returns x (models/temporal.py:113-114)
        ib_attn = eng.model.ib_addition_mode.lower() == "attention"       # x_i += cross_attn_ib_i(x_i, ib rows) (models/temporal.py:117-118)
        fm = self.forms                                                   # which launches the plan consists of: decided in plan_forms.resolve_forms
        lanes, chain, few, fold_ib = fm.lanes, fm.chain, fm.few, fm.fold_ib
        if fm.hoist_ib:    # the info-bottleneck rows of all steps exist already: added by the norm pass in front of the MLP (AdaLN or LayerNorm alike)
            ibufs = [t[:M] for t in self._cond_src.ibufs]
        else:
            ibufs = [self._buf(M, E, dtype=f32) for _ in range(self.L)] if fold_ib else None
        mods = self._mods = self._cond_mods([(f"blocks.{l}.", ibufs[l]) for l in range(self.L)] if fm.ib_rows_here else ())
        cond_joined = not fm.split_cond
        rope_s, rope_c = eng.rope_self, eng.rope_cross
        Eo, concat = self.Eo, self.concat
        FE = F * Eo                                             # row stride of the caller's [B, T, F, Eo] tensors
        xr = [self._buf(M, E, dtype=f32) for _ in range(F)]     # fp32 residual stream
        xa = [self._buf(M, E) for _ in range(F)]                # act-dtype copy (GEMM A operand)
        n_e = [self._buf(M, E) for _ in range(F)]               # normalised rows, dim E
        att_e = [self._buf(M, E) for _ in range(F)]
        Qs = [self._buf(B, H, T, hd_s) for _ in range(F)]
        Ks = [[self._buf(B, H, cap, hd_s, zero=True) for _ in range(F)] for _ in range(self.L)]
        Vs = [[self._buf(B, H, hd_s, cap, zero=True) for _ in range(F)] for _ in range(self.L)]
        dn = [self._buf(M, D, dtype=f32) for _ in range(F)]
        if xmode == "sea":   # cross-attention workspaces
            nd_old = [self._buf(M, D) for _ in range(F)]
            nd_new = [self._buf(M, D) for _ in range(F)]
            Qc = [self._buf(B, H, T, hd_c) for _ in range(max(F - 1, 1))]
            Qc2 = [[self._buf(B, H, T, hd_c) for _ in range(F - 1)] for _ in range(F)] if chain else None   # every field's q rows exist at once
            Kc = [[[self._buf(B, H, cap, hd_c, zero=True) for _ in range(F)] for _ in range(F)] for _ in range(self.L)]
            Vc = [[[self._buf(B, H, hd_c, cap, zero=True) for _ in range(F)] for _ in range(F)] for _ in range(self.L)]
            att_c = [self._buf(M, D) for _ in range(max(F - 1, 1))]
            gp = self._buf(max(F - 1, 1), M, D)
        pad = fm.hidden_pad   # (a power-of-two row stride would crowd a few memory channels)
        hbuf = [self._buf(M, S + pad)[:, :S] for _ in range(F)]
        hg = [self._buf(M, S + pad)[:, :S] for _ in range(F)]
        self.ws = dict(xr=xr, xa=xa, n_e=n_e, att_e=att_e, hbuf=hbuf, hg=hg)
        # the keys / values of every self-attention module and cross-attention pair, per layer: the full-context plan leaves positions 0 .. T-1 here, the
        # source of a context rollout's cache prefill (kv_engine.CacheFill); a step plan's are the caches themselves
        self.kv = dict(Ks=Ks, Vs=Vs, Kc=(Kc if xmode == "sea" else None), Vc=(Vc if xmode == "sea" else None))

        xm = [self._buf(M, E) for _ in range(F)] if lanes else xa
        first = True  # the residual stream still lives in the caller's x [B,T,F,E]
        for l in range(self.L):
            pre = f"blocks.{l}."
            last = l == self.L - 1
            if first and not eng.model.add_info_after_cross and (has_ib or ib_attn or concat):
                # the info-bottleneck add comes first and must not modify the caller's tensor: copy x into xr
                for i in range(F):
                    rec = _Rec(L.sea_convert_f32_to_act, [None, FE, xr[i].data_ptr(), E, M, Eo, N.SEA_F32], "x.copy")
                    self._x_patches.append((rec.args, 0, i * Eo * 4))
                    self.records.append(rec)
                first = False
            if concat:
                # x_i := [x_i | ib rows] (models/temporal.py:115-116): columns Eo .. E-1 of the residual rows are zeroed, then the usual info-bottleneck add
                # runs on them (columns 0 .. Eo-1 hold the caller's rows / the previous block's proj output)
                if self._zero_ib is None:
                    self._zero_ib = self._buf(M, self.ib_dim, dtype=f32, zero=True)
                for i in range(F):
                    self._cur.append(self._rec(L.sea_convert_f32_to_act, [self._zero_ib.data_ptr(), self.ib_dim, xr[i][:, Eo:].data_ptr(), E, M, self.ib_dim, N.SEA_F32],
                                               "ib.concat.zero"))
                self._ib(pre, [xr[i][:, Eo:] for i in range(F)])
            if not eng.model.add_info_after_cross and has_ib:
                self._ib(pre, xr)
            if not eng.model.add_info_after_cross and ib_attn:
                self._ib_attn(pre, xr)
            # -- self attention: x_i += proj(attn(AdaLN_0(x_i)))
            def norm0():   # AdaLN_0 / LayerNorm of every field (`few`: as the prologue of the projection, no output rows)
                groups = []
                for i in range(F):
                    g = dict(**self._norm_params(f"{pre}ln.exp.{i}.0.")) if few else dict(Yact=n_e[i], **self._norm_params(f"{pre}ln.exp.{i}.0."))
                    if first:
                        g.update(X=xr[i], ldx=FE, X_is_x=i * Eo * 4)
                    else:
                        g.update(X=xr[i])
                    groups.append(g)
                return groups
            qkv_groups = [dict(W=P.act(f"{pre}attn.self.{i}.q.weight", 3 * E), bias=P.f32_vec(f"{pre}attn.self.{i}.q.bias", 3 * E),
                               col0=0, Q=Qs[i], K=Ks[l][i], Vt=Vs[l][i]) for i in range(F)]
            if few:
                self._qkv_few(qkv_groups, rope_s, hd_s, "self.qkv_rope", pre=norm0())
            elif l == 0 and fm.one_launch_front:   # (reads the module's parameters itself: its modulation matrix does not exist)
                self._front_launch(pre, first, xr, Qs, Ks[l], Vs[l])
            else:
                if l == 0 and fm.adaln_front:
                    hid = self._front[0]
                    ag = []
                    for i in range(F):
                        mp = f"{pre}ln.exp.{i}.0."
                        g = dict(A=hid[mp], W=P.act(mp + "cond_mlp.2.weight"), bias=P.f32_vec(mp + "cond_mlp.2.bias"), X=xr[i], gamma=P.f32_vec(mp + "weight"), beta=P.f32_vec(mp + "bias"), Yact=n_e[i])
                        if first:
                            g.update(ldx=FE, X_is_x=i * Eo * 4)
                        ag.append(g)
                    for key, hid_ in hid.items():
                        if "ln_cross." in key:
                            ag.append(dict(A=hid_, W=P.act(key + "cond_mlp.2.weight"), bias=P.f32_vec(key + "cond_mlp.2.bias"), Yact=mods[key]))
                    self._adaln(ag, "self.cond_adaln0")
                else:
                    self._norm(norm0(), E, "self.adaln0")
                self._qkv([dict(A=n_e[i], **g) for i, g in enumerate(qkv_groups)], rope_s, hd_s, "self.qkv_rope")
            self._attn([dict(Q=Qs[i], K=Ks[l][i], Vt=Vs[l][i], O=att_e[i]) for i in range(F)], hd_s, E, "self.attention")
            groups = []
            for i in range(F):
                g = dict(A=att_e[i], W=P.act(f"{pre}attn.self.{i}.projection.weight"), C32=xr[i], Cact=xa[i])
                if first:
                    g.update(R=xr[i], ldr=FE, R_is_x=i * Eo * 4)
                else:
                    g.update(R=xr[i])
                groups.append(g)
            if chain:
                # out-projection + residual, cross_down + ln_cross of the PRE-exchange rows, and from those normalised rows (never stored): q_ij for every
                # j != i, and k / v of the pairs (a, i), a < i — field a runs its cross-attention before field i is updated (models/temporal.py:187-192)
                groups = []
                for i in range(F):
                    proj = []
                    for s_, j in enumerate([j for j in range(F) if j != i]):
                        ca = f"{pre}cross_attn.{i}.{j}."
                        proj.append(dict(W=P.act(ca + "q.weight"), bias=P.f32_vec(ca + "q.bias"), col0=0, Q=Qc2[i][s_]))
                    for a in range(i):
                        ca = f"{pre}cross_attn.{a}.{i}."
                        proj.append(dict(W=P.act(ca + "k.weight", 2 * D), bias=P.f32_vec(ca + "k.bias", 2 * D), col0=D, K=Kc[l][a][i], Vt=Vc[l][a][i]))
                    g = dict(a2=att_e[i], W2=P.act(f"{pre}attn.self.{i}.projection.weight"), Xin=xr[i], X=xr[i], proj=proj,
                             down=dict(W=P.act(f"{pre}cross_down.{i}.weight"), bias=P.f32_vec(f"{pre}cross_down.{i}.bias"), **self._norm_params(f"{pre}ln_cross.{i}.")))
                    if first:
                        g.update(ldxin=FE, Xin_is_x=i * Eo * 4)
                    groups.append(g)
                self._chain(groups, rope_c, hd_c, "self.out_proj_down_qkv")
            else:
                (self._gemm_few if few else self._gemm)(groups, "self.out_proj")
            first = False
            if not cond_joined:  # everything below reads modulations computed on lane 1
                self._join(1)
                cond_joined = True
            if xmode == "addition":
                # -- 'addition' exchange (models/temporal.py:291-301; Jacobi: every field read at its pre-exchange value): down-projection + norm of all
                # fields in one launch, s = GELU(sum_j n_j) as an identity-weight GEMM over F segments, x_i += cross_up_i(s) in one grouped launch
                ndall = self._buf(F, M, D)
                self._down_norm(pre, range(F), xa, dn, ndall, "add")
                sg = self._buf(M, D)
                self._gemm([dict(A=ndall[0], W=eng.eye(D), n_seg=F, a_seg_stride=M * D, Cact=sg, act=1)], "add.sum_gelu")
                self._gemm([dict(A=sg, W=P.act(f"{pre}cross_up.{i}.weight"), bias=P.f32_vec(f"{pre}cross_up.{i}.bias"), R=xr[i], C32=xr[i])
                            for i in range(F)], "add.up")
            if xmode == "pool":
                # -- 'pool' exchange (models/temporal.py:255-277, pool_update_method 'mlp'; Jacobi): n_j = ln_cross_j(cross_down_j(x_j)) + pe; pool =
                # MLP(cat_j n_j); a_i = cross_attn_i(n_i, pool); x_i += cross_up_i(GELU(n_i + a_i)).  `big` holds [n_0 .. n_{F-1} | a_0 .. a_{F-1}] side by
                # side, so that cat(n) is a view and (n_i, a_i) are two segments of one identity-weight GEMM
                FD = F * D
                big = self._buf(M, 2 * FD)
                nrm = [self._buf(M, D) for _ in range(F)]
                pe_t = self._buf(M, D, dtype=f32)
                pe_t.copy_(blk_pe(eng, l)[:T].repeat(B, 1))
                self._down_norm(pre, range(F), xa, dn, nrm, "pool")
                self._gemm([dict(A=nrm[j], W=eng.eye(D), R=pe_t, Cact=big[:, j * D:(j + 1) * D]) for j in range(F)], "pool.pe_add")
                hp, pool = self._buf(M, 2 * D), self._buf(M, D)
                self._gemm([dict(A=big[:, :FD], W=P.act(f"{pre}pool_update.0.weight"), bias=P.f32_vec(f"{pre}pool_update.0.bias"), Cact=hp, act=1)], "pool.update0")
                self._gemm([dict(A=hp, W=P.act(f"{pre}pool_update.2.weight"), bias=P.f32_vec(f"{pre}pool_update.2.bias"), Cact=pool)], "pool.update2")
                Qp = [self._buf(B, H, T, hd_c) for _ in range(F)]
                Kp = [self._buf(B, H, cap, hd_c, zero=True) for _ in range(F)]
                Vp = [self._buf(B, H, hd_c, cap, zero=True) for _ in range(F)]
                att_p = [self._buf(M, D) for _ in range(F)]
                qg = []
                for i in range(F):
                    ca = f"{pre}cross_attn.{i}."
                    qg.append(dict(A=big[:, i * D:(i + 1) * D], W=P.act(ca + "q.weight"), bias=P.f32_vec(ca + "q.bias"), col0=0, Q=Qp[i]))
                    qg.append(dict(A=pool, W=P.act(ca + "k.weight", 2 * D), bias=P.f32_vec(ca + "k.bias", 2 * D), col0=D, K=Kp[i], Vt=Vp[i]))
                self._qkv(qg, rope_c, hd_c, "pool.qkv_rope")
                self._attn([dict(Q=Qp[i], K=Kp[i], Vt=Vp[i], O=att_p[i]) for i in range(F)], hd_c, D, "pool.attention")
                self._gemm([dict(A=att_p[i], W=P.act(f"{pre}cross_attn.{i}.projection.weight"), Cact=big[:, FD + i * D:FD + (i + 1) * D]) for i in range(F)], "pool.proj")
                sg = [self._buf(M, D) for _ in range(F)]
                self._gemm([dict(A=big[:, i * D:(i + 1) * D], W=eng.eye(D), n_seg=2, a_seg_stride=FD, Cact=sg[i], act=1) for i in range(F)], "pool.sum_gelu")
                self._gemm([dict(A=sg[i], W=P.act(f"{pre}cross_up.{i}.weight"), bias=P.f32_vec(f"{pre}cross_up.{i}.bias"), R=xr[i], C32=xr[i])
                            for i in range(F)], "pool.up")
            # -- state exchange (Gauss-Seidel over i, models/temporal.py:187-192)
            if F > 1 and xmode == "sea" and few:
                # the same Gauss-Seidel sweep with ln_cross evaluated by its consumers: dn[j] holds cross_down_j(x_j) of the CURRENT x_j (rewritten by down_new once
                # field j has been updated), every q / k,v projection normalises the rows it reads itself
                self._gemm_few([dict(A=xa[j], W=P.act(f"{pre}cross_down.{j}.weight"), bias=P.f32_vec(f"{pre}cross_down.{j}.bias"), C32=dn[j]) for j in range(F)], "cross.down_old")
                for i in range(F):
                    others = [j for j in range(F) if j != i]
                    qkv_groups, qkv_pre, probs, proj_groups = [], [], [], []
                    for s, j in enumerate(others):
                        ca = f"{pre}cross_attn.{i}.{j}."
                        qkv_groups.append(dict(W=P.act(ca + "q.weight"), bias=P.f32_vec(ca + "q.bias"), col0=0, Q=Qc[s]))
                        qkv_pre.append(dict(X=dn[i], **self._norm_params(f"{pre}ln_cross.{i}.")))
                        qkv_groups.append(dict(W=P.act(ca + "k.weight", 2 * D), bias=P.f32_vec(ca + "k.bias", 2 * D), col0=D, K=Kc[l][i][j], Vt=Vc[l][i][j]))
                        qkv_pre.append(dict(X=dn[j], **self._norm_params(f"{pre}ln_cross.{j}.")))
                        probs.append(dict(Q=Qc[s], K=Kc[l][i][j], Vt=Vc[l][i][j], O=att_c[s]))
                        proj_groups.append(dict(A=att_c[s], W=P.act(ca + "projection.weight"), Cact=gp[s], act=1))
                    self._qkv_few(qkv_groups, rope_c, hd_c, f"cross{i}.qkv_rope", pre=qkv_pre)
                    self._attn(probs, hd_c, D, f"cross{i}.attention")
                    self._gemm_few(proj_groups, f"cross{i}.proj_gelu")
                    up = dict(A=gp[0], W=P.act(f"{pre}cross_up.{i}.weight"), bias=P.f32_vec(f"{pre}cross_up.{i}.bias"),
                              bias_scale=float(F - 1), n_seg=F - 1, a_seg_stride=M * D, R=xr[i], C32=xr[i], Cact=(xa[i] if i < F - 1 else None))
                    (self._gemm_few if F == 2 else self._gemm)([up], f"cross{i}.up_sum")   # (F > 2: the sum over the F - 1 projections needs sea_gemm_grouped's segments)
                    if i < F - 1:
                        self._gemm_few([dict(A=xa[i], W=P.act(f"{pre}cross_down.{i}.weight"), bias=P.f32_vec(f"{pre}cross_down.{i}.bias"), C32=dn[i])], f"cross{i}.down_new")
            elif F > 1 and xmode == "sea" and chain:
                for i in range(F):
                    others = [j for j in range(F) if j != i]
                    self._attn([dict(Q=Qc2[i][s_], K=Kc[l][i][j], Vt=Vc[l][i][j], O=att_c[s_]) for s_, j in enumerate(others)], hd_c, D, f"cross{i}.attention")
                    # the field's tail; from its UPDATED rows: cross_down + ln_cross, then k / v of the pairs (b, i), b > i (fields that run after it)
                    proj = []
                    for b_ in range(i + 1, F):
                        ca = f"{pre}cross_attn.{b_}.{i}."
                        proj.append(dict(W=P.act(ca + "k.weight", 2 * D), bias=P.f32_vec(ca + "k.bias", 2 * D), col0=D, K=Kc[l][b_][i], Vt=Vc[l][b_][i]))
                    down = None
                    if i < F - 1:
                        down = dict(W=P.act(f"{pre}cross_down.{i}.weight"), bias=P.f32_vec(f"{pre}cross_down.{i}.bias"), **self._norm_params(f"{pre}ln_cross.{i}."))
                    self._chain([dict(att=[att_c[s_] for s_ in range(len(others))], Wp=[P.act(f"{pre}cross_attn.{i}.{j}.projection.weight") for j in others],
                                      W2=P.act(f"{pre}cross_up.{i}.weight"), b2=P.f32_vec(f"{pre}cross_up.{i}.bias"), bias_scale=float(F - 1), Xin=xr[i], X=xr[i],
                                      down=down, proj=proj)], rope_c, hd_c, f"cross{i}.tail")
            elif F > 1 and xmode == "sea":
                self._down_norm(pre, range(F), xa, dn, nd_old, "cross", "_old")
                for i in range(F):
                    others = [j for j in range(F) if j != i]
                    qkv_groups, probs, proj_groups = [], [], []
                    for s, j in enumerate(others):
                        src = nd_new[j] if j < i else nd_old[j]
                        ca = f"{pre}cross_attn.{i}.{j}."
                        qkv_groups.append(dict(A=nd_old[i], W=P.act(ca + "q.weight"), bias=P.f32_vec(ca + "q.bias"), col0=0, Q=Qc[s]))
                        qkv_groups.append(dict(A=src, W=P.act(ca + "k.weight", 2 * D), bias=P.f32_vec(ca + "k.bias", 2 * D), col0=D,
                                               K=Kc[l][i][j], Vt=Vc[l][i][j]))
                        probs.append(dict(Q=Qc[s], K=Kc[l][i][j], Vt=Vc[l][i][j], O=att_c[s]))
                        proj_groups.append(dict(A=att_c[s], W=P.act(ca + "projection.weight"), Cact=gp[s], act=1))
                    self._qkv(qkv_groups, rope_c, hd_c, f"cross{i}.qkv_rope")
                    self._attn(probs, hd_c, D, f"cross{i}.attention")
                    if fm.xtail:
                        # everything between this field's cross-attention and the next field's: projections + GELU, up-projection of the sum + residual,
                        # down-projection + ln_cross of the updated field, in one launch (a workgroup carries 16 rows through the three layers)
                        down = None
                        if i < F - 1:
                            down = dict(W=P.act(f"{pre}cross_down.{i}.weight"), bias=P.f32_vec(f"{pre}cross_down.{i}.bias"), Yact=nd_new[i],
                                        **self._norm_params(f"{pre}ln_cross.{i}."))
                        self._xtail([att_c[s] for s in range(len(others))], [P.act(f"{pre}cross_attn.{i}.{j}.projection.weight") for j in others],
                                    P.act(f"{pre}cross_up.{i}.weight"), P.f32_vec(f"{pre}cross_up.{i}.bias"), float(F - 1), xr[i], down, f"cross{i}.tail")
                        continue
                    self._gemm(proj_groups, f"cross{i}.proj_gelu")
                    up = dict(A=gp[0], W=P.act(f"{pre}cross_up.{i}.weight"), bias=P.f32_vec(f"{pre}cross_up.{i}.bias"),
                              bias_scale=float(F - 1), n_seg=F - 1, a_seg_stride=M * D, R=xr[i], C32=xr[i],
                              Cact=(xa[i] if i < F - 1 else None))
                    self._gemm([up], f"cross{i}.up_sum")
                    if lanes:
                        # x_i is final for the exchange: its info-bottleneck add, MLP, proj (and final norm) run on their own lane beside the
                        # remaining Gauss-Seidel stages; the last field stays on the main stream.  fc2 writes xm, not xa: the main stream
                        # still reads xa[i] (down_new) while the lane runs.
                        if i < F - 1:
                            self._fork(2 + i)
                        self._ib(pre, [xr[i]])
                        self._mlp_proj(pre, [i], xr, xm, n_e, hbuf, hg, last, tag=f".f{i}")
                        if i < F - 1:
                            self._end_lane()
                    if i < F - 1:
                        self._down_norm(pre, [i], xa, dn, nd_new, f"cross{i}", "_new")
            if lanes:
                for i in range(F - 1):
                    self._join(2 + i)
                continue
            if eng.model.add_info_after_cross and has_ib and not fold_ib:
                self._ib(pre, xr)
            if eng.model.add_info_after_cross and ib_attn:
                self._ib_attn(pre, xr)
            self._mlp_proj(pre, list(range(F)), xr, xa, n_e, hbuf, hg, last, addend=(ibufs[l] if fold_ib else None))

    def _norm_params(self, pre: str) -> dict:
        """The gains of the row norm `pre` (AdaLN: with the module's modulation rows) as arguments of ops.fill_norm_group and its kin."""
        P = self.eng.params
        if self.adaln:
            return dict(mod=self._mods[pre], gamma=P.f32_vec(pre + "weight"), beta=P.f32_vec(pre + "bias"))
        return dict(gamma=P.f32_vec(pre + "weight"))

    def _down_norm(self, pre, fields, xa, dn, Y, stem: str, suffix: str = "") -> None:
        """Y_j = ln_cross_j(cross_down_j(xa_j)) for the listed fields: one sea_gemm_rownorm launch (forms.down_norm), else GEMM (into dn_j) + row norm."""
        P = self.eng.params
        lin = lambda j: dict(A=xa[j], W=P.act(f"{pre}cross_down.{j}.weight"), bias=P.f32_vec(f"{pre}cross_down.{j}.bias"))  # noqa: E731
        if self.forms.down_norm:
            self._gemm_norm([dict(Yact=Y[j], **lin(j), **self._norm_params(f"{pre}ln_cross.{j}.")) for j in fields], f"{stem}.down_norm{suffix}")
        else:
            self._gemm([dict(C32=dn[j], **lin(j)) for j in fields], f"{stem}.down{suffix}")
            self._norm([dict(X=dn[j], Yact=Y[j], **self._norm_params(f"{pre}ln_cross.{j}.")) for j in fields], self.D, f"{stem}.norm{suffix}")

    def _front_launch(self, pre, first, xr, Qs, Ks, Vs) -> None:
        """The front of the first block as ONE launch (sea_adaln_qkv): the condition MLP of AdaLN_0 with its hidden rows generated in the launch, AdaLN_0 and the
        self-attention's q / k / v + rotary epilogue.  A rider plan's (forms.front_chain) also carries cond_mlp.2 of ln_cross: as plain GEMM groups on the CUs the
        launch leaves idle, or — forms.front3 — as every field's third layer, the silu / information-bottleneck rows of _cond_mods then being its row riders."""
        P, F, E, D, M, Eo, fm = self.eng.params, self.F, self.E, self.D, self.M, self.Eo, self.forms
        hid, rows = self._front if fm.front_chain else (None, None)
        if fm.cond_memo and self.memo_count is None:
            self.memo_count = self._buf(2, dtype=torch.int32, zero=True)   # (hits, misses) in workgroups, counted where SEA_TUNE=memo_count=1
        arr = (N.SeaAdalnQkv * F)()
        for g_, i in zip(arr, range(F)):
            mp, lc = f"{pre}ln.exp.{i}.0.", f"{pre}ln_cross.{i}."
            third = dict(w1=P.f32_vec(lc + "cond_mlp.0.weight", 2 * D), b1=P.f32_vec(lc + "cond_mlp.0.bias"), W=P.act(lc + "cond_mlp.2.weight"), bias=P.f32_vec(lc + "cond_mlp.2.bias"),
                         out=self._mods[lc]) if fm.front3 else None   # ln_cross_i's modulation as the launch's third layer
            # the condition memo: a stamp per row, zeroed once (epoch 0 matches nothing); the table is the [M, 2E] modulation buffer _cond_mods keeps for the module.
            # Both, and the third layer's output, are written by this launch only and live as long as the plan: what a forward leaves is there for the next
            memo = dict(stamps=self._buf(M, 2, dtype=torch.int32, zero=True), mods=self._mods[mp], epoch=P.memo_epoch, count=self.memo_count) if fm.cond_memo else None
            if memo is not None and i == 0 and rows is not None:   # the row riders' stamps: a set per silu group and one for the information-bottleneck rows
                memo["rows"] = self._buf(rows[1] + 1, M, 2, dtype=torch.int32, zero=True)
            ops.fill_adaln_qkv(g_, X=xr[i], cond=None, w1=P.f32_vec(mp + "cond_mlp.0.weight", 2 * E), b1=P.f32_vec(mp + "cond_mlp.0.bias"), W2c=P.act(mp + "cond_mlp.2.weight"),
                               b2c=P.f32_vec(mp + "cond_mlp.2.bias"), gamma=P.f32_vec(mp + "weight"), beta=P.f32_vec(mp + "bias"), Wqkv=P.act(f"{pre}attn.self.{i}.q.weight", 3 * E),
                               bqkv=P.f32_vec(f"{pre}attn.self.{i}.q.bias", 3 * E), Q=Qs[i], K=Ks[i], Vt=Vs[i], ldx=(F * Eo if first else None), third=third, memo=memo)
            g_.M = M
            self._c_patches.append((g_, "cond"))
            if first:
                self._x_patches.append((g_, "X", i * Eo * 4))
        rg = [key for key in hid if "ln_cross." in key] if fm.front_chain and not fm.front3 else []   # plain rider groups
        rarr = (N.SeaGemmGroup * max(len(rg), 1))() if fm.front_chain else None
        for g_, key in zip(rarr or (), rg):
            ops.fill_gemm_group(g_, hid[key], P.act(key + "cond_mlp.2.weight"), P.f32_vec(key + "cond_mlp.2.bias"), Cact=self._mods[key])
        common = self._qkv_common(self.eng.rope_self, E // self.H)
        sarr, n_s, ibp = rows if rows is not None else (None, 0, None)   # row riders
        rec = self._rec(N.lib().sea_adaln_qkv, [arr, F, C.byref(common), (rarr if rg else None), len(rg), (sarr if n_s else None), n_s, None, (M if (n_s or ibp is not None) else 0),
                                                (C.byref(ibp) if ibp is not None else None), 1e-5, self.code], "self.cond_adaln0_qkv_rope", (arr, common, rarr, sarr, ibp))
        if n_s or ibp is not None:
            self._c_patches.append((rec.args, 7))
        self._cur.append(rec)

    def _mlp_proj(self, pre, fields, xr, xm, n_e, hbuf, hg, final_norm, tag="", addend=None) -> bool:
        """x_i += W2 gelu(LN(W1 AdaLN_2(x_i))) ; x_i = proj_i(x_i) for the listed fields (models/temporal.py:143-146), optionally followed
        by the model's final per-field norm written straight into out (models/temporal.py:412-415)."""
        P, E, S, Eo, FE = self.eng.params, self.E, self.S, self.Eo, self.F * self.Eo
        xo = xr if Eo == E else [t[:, :Eo] for t in xr]   # the proj output / the next block's input rows ('concat': the first Eo columns of the widened rows)

        fm = self.forms
        if fm.few:
            # KV-cache step at the shipped widths: [ib add + AdaLN_2 / LayerNorm] fc1 | [LayerNorm + GELU] fc2 + residual | proj | final norm.
            # x + ib goes to rows of its own (xq): the prologue runs in every workgroup of fc1, so it must not update the rows it reads
            xq = [self._buf(self.M, E, dtype=torch.float32) for _ in fields] if addend is not None else None
            res = xq if addend is not None else [xr[i] for i in fields]
            pre_n = [dict(X=xr[i], **(dict(addend=addend, Xout=xq[k]) if addend is not None else {}), **self._norm_params(f"{pre}ln.exp.{i}.2.")) for k, i in enumerate(fields)]
            self._gemm_few([dict(W=P.act(f"{pre}mlp.{i}.layers.0.weight"), bias=P.f32_vec(f"{pre}mlp.{i}.layers.0.bias"), Cact=hbuf[i]) for i in fields], "mlp.fc1" + tag, pre=pre_n)
            ln_h = [dict(X=hbuf[i], gamma=P.f32_vec(f"{pre}mlp.{i}.layers.1.weight"), beta=P.f32_vec(f"{pre}mlp.{i}.layers.1.bias")) for i in fields]
            fold_ln = fm.few_fold_ln   # LayerNorm + GELU of the hidden rows as the prologue of fc2
            if not fold_ln:
                self._norm([dict(Yact=hg[i], **g_) for i, g_ in zip(fields, ln_h)], S, "mlp.ln_gelu" + tag, x_is_act=True, gelu=True)
            self._gemm_few([dict(A=(None if fold_ln else hg[i]), W=P.act(f"{pre}mlp.{i}.layers.3.weight"), bias=P.f32_vec(f"{pre}mlp.{i}.layers.3.bias"), R=res[k], Cact=xm[i])
                            for k, i in enumerate(fields)], "mlp.fc2" + tag, pre=(ln_h if fold_ln else None), pre_act=fold_ln, pre_gelu=fold_ln)
            self._gemm_few([dict(A=xm[i], W=P.act(f"{pre}proj.{i}.weight"), bias=P.f32_vec(f"{pre}proj.{i}.bias"), C32=xo[i]) for i in fields], "proj" + tag)
            if final_norm:
                self._norm([dict(X=xo[i], Y32=xo[i], ldy32=FE, Y_is_out=i * Eo * 4, **self._norm_params(f"ln.{i}.")) for i in fields], Eo, "final.norm" + tag)
            return final_norm
        fused, norm_in = fm.mlp_fc1, fm.mlp_norm_in   # fc1 + LayerNorm + GELU as one launch; ... with the row pass in front of it as its prologue
        extra = (lambda i: dict(addend=addend, Xout=xr[i])) if addend is not None else (lambda i: {})   # x_i += ib rides in this pass
        if not norm_in:
            self._norm([dict(X=xr[i], Yact=n_e[i], **extra(i), **self._norm_params(f"{pre}ln.exp.{i}.2.")) for i in fields], E, ("mlp.ib_adaln2" if addend is not None else "mlp.adaln2") + tag)
        if fm.mlp_block:   # the whole field MLP + proj (+ final norm) as ONE launch (sea_mlp_block)
            a1, a2 = (N.SeaMlpGroup * len(fields))(), (N.SeaMlp2Group * len(fields))()
            for g1, g2, i in zip(a1, a2, fields):
                nrm = dict(X32=xr[i], **(dict(addend=addend) if addend is not None else {}), **self._norm_params(f"{pre}ln.exp.{i}.2.")) if norm_in else None
                ops.fill_mlp_group(g1, None if norm_in else n_e[i], P.act(f"{pre}mlp.{i}.layers.0.weight"), P.f32_vec(f"{pre}mlp.{i}.layers.0.bias"),
                                   P.f32_vec(f"{pre}mlp.{i}.layers.1.weight"), P.f32_vec(f"{pre}mlp.{i}.layers.1.bias"), None, nrm)
                fin = self._norm_params(f"ln.{i}.") if final_norm else {}
                ops.fill_mlp2_group(g2, None, P.act(f"{pre}mlp.{i}.layers.3.weight"), P.f32_vec(f"{pre}mlp.{i}.layers.3.bias"), (None if norm_in else xr[i]),
                                    P.act(f"{pre}proj.{i}.weight"), P.f32_vec(f"{pre}proj.{i}.bias"), Y32=xr[i], ldy32=(FE if final_norm else None), M=g1.M, **fin)
                if final_norm:
                    self._out_patches.append((g2, "Y32", i * E * 4))
            self._cur.append(self._rec(N.lib().sea_mlp_block, [a1, a2, len(fields), 1e-5, self.code], ("mlp.block_norm" if final_norm else "mlp.block") + tag, (a1, a2)))
            return final_norm
        if fused:
            arr = (N.SeaMlpGroup * len(fields))()
            for g_, i in zip(arr, fields):
                nrm = dict(X32=xr[i], **extra(i), **self._norm_params(f"{pre}ln.exp.{i}.2.")) if norm_in else None
                ops.fill_mlp_group(g_, None if norm_in else n_e[i], P.act(f"{pre}mlp.{i}.layers.0.weight"), P.f32_vec(f"{pre}mlp.{i}.layers.0.bias"),
                                   P.f32_vec(f"{pre}mlp.{i}.layers.1.weight"), P.f32_vec(f"{pre}mlp.{i}.layers.1.bias"), hg[i], nrm)
            self._cur.append(self._rec(N.lib().sea_mlp_fc1_ln_gelu, [arr, len(fields), 1e-5, self.code], "mlp.fc1_ln_gelu" + tag, arr))   # (with or without the norm prologue: one name for the profiles)
        else:
            self._gemm([dict(A=n_e[i], W=P.act(f"{pre}mlp.{i}.layers.0.weight"), bias=P.f32_vec(f"{pre}mlp.{i}.layers.0.bias"), Cact=hbuf[i])
                        for i in fields], "mlp.fc1" + tag)
            self._norm([dict(X=hbuf[i], gamma=P.f32_vec(f"{pre}mlp.{i}.layers.1.weight"), beta=P.f32_vec(f"{pre}mlp.{i}.layers.1.bias"), Yact=hg[i])
                        for i in fields], S, "mlp.ln_gelu" + tag, x_is_act=True, gelu=True)
        if fm.mlp_fc2_proj:   # fc2 + residual, proj and — after the last layer — the model's final norm in one launch (sea_mlp_fc2_proj_norm)
            arr = (N.SeaMlp2Group * len(fields))()
            for g_, i in zip(arr, fields):
                nrm = self._norm_params(f"ln.{i}.") if final_norm else {}
                ops.fill_mlp2_group(g_, hg[i], P.act(f"{pre}mlp.{i}.layers.3.weight"), P.f32_vec(f"{pre}mlp.{i}.layers.3.bias"), xr[i],
                                    P.act(f"{pre}proj.{i}.weight"), P.f32_vec(f"{pre}proj.{i}.bias"), Y32=xr[i], ldy32=(FE if final_norm else None), **nrm)
                if final_norm:
                    self._out_patches.append((g_, "Y32", i * E * 4))
            self._cur.append(self._rec(N.lib().sea_mlp_fc2_proj_norm, [arr, len(fields), 1e-5, self.code], ("mlp.fc2_proj_norm" if final_norm else "mlp.fc2_proj") + tag, arr))
            return final_norm
        self._gemm([dict(A=hg[i], W=P.act(f"{pre}mlp.{i}.layers.3.weight"), bias=P.f32_vec(f"{pre}mlp.{i}.layers.3.bias"), R=xr[i], Cact=xm[i])
                    for i in fields], "mlp.fc2" + tag)
        if final_norm and fm.proj_norm:   # the last layer's proj + the model's final norm in one launch (sea_gemm_rownorm)
            self._gemm_norm([dict(A=xm[i], W=P.act(f"{pre}proj.{i}.weight"), bias=P.f32_vec(f"{pre}proj.{i}.bias"), Y32=xo[i], ldy32=FE, Y_is_out=i * Eo * 4,
                                  **self._norm_params(f"ln.{i}.")) for i in fields], "proj_norm" + tag)
            return final_norm
        self._gemm([dict(A=xm[i], W=P.act(f"{pre}proj.{i}.weight"), bias=P.f32_vec(f"{pre}proj.{i}.bias"), C32=xo[i]) for i in fields], "proj" + tag)
        if final_norm:
            self._norm([dict(X=xo[i], Y32=xo[i], ldy32=FE, Y_is_out=i * Eo * 4, **self._norm_params(f"ln.{i}.")) for i in fields], Eo, "final.norm" + tag)
        return final_norm

    def _ib_params(self, pre: str) -> dict:
        P = self.eng.params
        return dict(w1=P.f32_vec(pre + "ib.layers.0.weight"), b1=P.f32_vec(pre + "ib.layers.0.bias"), lnw=P.f32_vec(pre + "ib.layers.1.weight"),
                    lnb=P.f32_vec(pre + "ib.layers.1.bias"), w2=P.f32(pre + "ib.layers.3.weight"), b2=P.f32_vec(pre + "ib.layers.3.bias"),
                    h=self.eng.model.ib_hidden)

    def _ib_layer(self, pre: str) -> dict:
        """ops.fill_ib_params's layer arguments for the block's ib_scale_mode (models/temporal.py:103-109), on this plan's rows."""
        P, mode = self.eng.params, self.eng.ib_mode
        if mode == 0:
            w = {k: v for k, v in self._ib_params(pre).items() if k != "h"}
        elif mode == 1:   # nn.Linear(1, E): weight [E, 1], bias [E]
            w = dict(w1=P.f32_vec(pre + "ib.weight"), b1=P.f32_vec(pre + "ib.bias"))
        else:             # GaussianFourierProjection: W [1, E/2]
            w = dict(w1=P.f32(pre + "ib.W"))
        return dict(w, mode=mode, M=self.M, E=self.ib_dim)

    def _ib(self, pre: str, xr: List[torch.Tensor], drop=None) -> None:
        """drop: (thr, first stream); the seed is re-keyed every step (set_dropout_seed)."""
        ib = N.SeaIbParams()
        ops.fill_ib_params(ib, xr, None, drop=((0, drop[1], drop[0]) if drop is not None else None), **self._ib_layer(pre))
        if drop is not None:
            self._drop_structs.append(ib)
        self._c_patches.append((ib, "c"))
        self._cur.append(self._rec(N.lib().sea_ib_add, [C.byref(ib)], "ib_add", ib))

    def _ib_rows(self, pre: str, drop=None):
        """The info-bottleneck rows ib(cond) [M, E] as a buffer of their own (fp32, and in the activation dtype): a copy of zeros, the usual ib add on top."""
        L, M, E, f32 = N.lib(), self.M, self.E, torch.float32
        zeros, ib32 = self._buf(M, E, dtype=f32, zero=True), self._buf(M, E, dtype=f32)
        self._cur.append(self._rec(L.sea_convert_f32_to_act, [zeros.data_ptr(), E, ib32.data_ptr(), E, M, E, N.SEA_F32], "ib.rows.zero", zeros))
        self._ib(pre, [ib32], drop=drop)
        if self.dt == f32:
            return ib32, ib32
        ibact = self._buf(M, E)
        self._cur.append(self._rec(L.sea_convert_f32_to_act, [ib32.data_ptr(), E, ibact.data_ptr(), E, M, E, self.code], "ib.rows.act"))
        return ib32, ibact

    def _ib_rows_multi(self, pre: str, n: int, drop) -> List[torch.Tensor]:
        """n sets of info-bottleneck rows ib(cond) [M, E] in the activation dtype, each with its OWN dropout mask (streams drop[1] .. drop[1] + n - 1 of one
        sea_ib_add over n zeroed buffers): what the reference's n evaluations of self.ib in train() produce (models/temporal.py:110-118)."""
        L, M, E, f32 = N.lib(), self.M, self.E, torch.float32
        zeros = self._buf(M, E, dtype=f32, zero=True)
        rows32 = [self._buf(M, E, dtype=f32) for _ in range(n)]
        for t in rows32:
            self._cur.append(self._rec(L.sea_convert_f32_to_act, [zeros.data_ptr(), E, t.data_ptr(), E, M, E, N.SEA_F32], "ib.rows.zero", zeros))
        self._ib(pre, rows32, drop=drop)
        if self.dt == f32:
            return rows32
        out = [self._buf(M, E) for _ in range(n)]
        for a, b in zip(rows32, out):
            self._cur.append(self._rec(L.sea_convert_f32_to_act, [a.data_ptr(), E, b.data_ptr(), E, M, E, self.code], "ib.rows.act"))
        return out

    def _act_copy(self, x32: torch.Tensor, name: str, keep: bool = False) -> torch.Tensor:
        """Activation-dtype copy of an fp32 [M, E] (possibly strided) matrix — the operand of a GEMM that reads the residual stream directly.  `keep`: a
        real copy in fp32 too (training: the rows are updated in place afterwards and the weight gradient needs them as they were)."""
        if self.dt == torch.float32 and not keep:
            return x32
        y = self._buf(self.M, x32.shape[1])
        self._cur.append(self._rec(N.lib().sea_convert_f32_to_act, [x32.data_ptr(), x32.stride(0), y.data_ptr(), y.stride(0), self.M, x32.shape[1], self.code], name))
        return y

    def _ib_attn(self, pre: str, xr: List[torch.Tensor]) -> None:
        """ib_addition_mode 'attention' (models/temporal.py:117-118; MultiHeadCrossAttention, models/base_blocks.py:205-243): x_i += proj_i(softmax(q_i(x_i)
        k_i(ib)^T / sqrt(hd)) v_i(ib)) — no mask, no rotary embedding: the usual QKV / attention launches with a zero-angle rotation table and a visibility
        window (src_len) as long as the sequence."""
        eng, P, B, H, T, E, M, cap = self.eng, self.eng.params, self.B, self.H, self.T, self.E, self.M, self.cap
        F, hd = len(xr), E // H
        _, ibact = self._ib_rows(pre)
        xq = [self._act_copy(xr[i], "ib.attn.x_act") for i in range(F)]
        Q = [self._buf(B, H, T, hd) for _ in range(F)]
        K = [self._buf(B, H, cap, hd, zero=True) for _ in range(F)]
        Vt = [self._buf(B, H, hd, cap, zero=True) for _ in range(F)]
        att = [self._buf(M, E) for _ in range(F)]
        qg = []
        for i in range(F):
            ca = f"{pre}cross_attn_ib.{i}."
            qg.append(dict(A=xq[i], W=P.act(ca + "q.weight"), bias=P.f32_vec(ca + "q.bias"), col0=0, Q=Q[i]))
            qg.append(dict(A=ibact, W=P.act(ca + "k.weight", 2 * E), bias=P.f32_vec(ca + "k.bias", 2 * E), col0=E, K=K[i], Vt=Vt[i]))
        self._qkv(qg, eng.rope_identity(hd), hd, "ib.attn.qkv")
        self._attn([dict(Q=Q[i], K=K[i], Vt=Vt[i], O=att[i]) for i in range(F)], hd, E, "ib.attn.attention", src_len=self.cap)
        self._gemm([dict(A=att[i], W=P.act(f"{pre}cross_attn_ib.{i}.projection.weight"), R=xr[i], C32=xr[i]) for i in range(F)], "ib.attn.proj")

    # ------------------------------------------------------------------ binding and replay
    def bind(self, x: torch.Tensor, ib: torch.Tensor, out: torch.Tensor) -> None:
        """Point the plan at the caller's tensors.  The plan knows them by raw address only, so it HOLDS them until the next bind: a launch list that is
        still executing (the host runs several steps ahead of the device) must never see its output block returned to the allocator — and possibly
        unmapped, e.g. by the cache flush a graph capture starts with — because the caller dropped the tensor."""
        self._bound_tensors = (x, ib, out)
        self.bind_ptrs(x.data_ptr(), ib.data_ptr(), out.data_ptr())
        if not self._audited or ptrcheck.always():
            self.audit()

    def _known_ranges(self, owners=()) -> "ptrcheck.Ranges":
        eng, R = self.eng, ptrcheck.Ranges()
        for t in self._keep:
            R.add_tensor(t, "plan workspace")
        P = eng.params
        for t, label in ((P.flat32, "flat32"), (P.flat_act, "flat_act"), (P.flat_actT, "flat_actT"), (P.memo_epoch, "weight epoch"), (eng.grads, "grads"), (eng.rope_self, "rope_self"),
                         (eng.rope_cross, "rope_cross"), (getattr(self, "_ws_colsum", None), "column-sum workspace"), (self._zero_ib, "zero rows")):
            R.add_tensor(t, label)
        for t in eng._eyes.values():
            R.add_tensor(t, "identity / rotation table")
        if self._cond_src is not None:
            for t in self._cond_src._keep:
                R.add_tensor(t, "hoisted condition buffers")
        for t, label in zip(getattr(self, "_bound_tensors", ()) or (), ("x", "condition", "out")):
            R.add_tensor(t, "bound " + label)
        R.add_tensor(getattr(self, "_bound_dout", None), "bound dout")
        for t in getattr(self, "_bound_input_grads", None) or ():
            R.add_tensor(t, "bound input gradient")
        for t in (eng._loss_ws or ()):
            R.add_tensor(t, "loss workspace")
        for t in owners:
            R.add_tensor(t, "caller buffer")
        return R

    def audit(self, owners=()) -> int:
        """Every device pointer of every launch record lies inside a buffer this plan knows, operands with their full extent (sea_amd/ptrcheck.py).
        Runs at the first bind of a plan and at every bind under SEA_CHECK_PTRS=1."""
        esz = 4 if self.dt == torch.float32 else 2
        n = ptrcheck.check_records(self._all_records(), self._known_ranges(owners), esz, f"{type(self).__name__} B={self.B} T={self.T} {self.mode}")
        self._audited = True
        return n

    def _all_records(self):
        return self.records

    def bind_ptrs(self, xp: int, cp: int, op: int) -> None:
        """Point the plan at the caller's buffers: x [M, F, E] fp32, condition [M] fp32, out [M, F, E] fp32 (row m = b*T + t)."""
        key = (xp, cp, op)
        if key == self._bound:
            return
        for tgt, field, off in self._x_patches:
            if isinstance(tgt, list):
                tgt[field] = xp + off
            else:
                setattr(tgt, field, xp + off)
        for tgt, field, off in self._out_patches:
            setattr(tgt, field, op + off)
        for tgt, field in self._c_patches:
            if isinstance(tgt, list):
                tgt[field] = cp
            else:
                setattr(tgt, field, cp)
        self._bound = key
        self._relink()

    def set_dropout_seed(self, seed: int) -> None:
        for st in self._drop_structs:
            st.drop.seed = seed & 0xFFFFFFFF

    def set_position(self, pos0: int) -> None:
        """Step mode: the T rows of this call sit at absolute positions pos0 .. pos0 + T - 1 of the K/V caches."""
        assert pos0 + self.T <= self.cap
        self.pos0 = pos0
        for s in self._pos_structs:
            if isinstance(s, N.SeaQkvCommon):
                s.pos0 = pos0
            else:
                s.q_pos0, s.Tk = pos0, pos0 + self.T

    def step_patch_table(self, x_base: int, x_stride: int, c_base: int, c_stride: int, out_base: int, out_stride: int, pos0: int = 0):
        """The per-step edits of a KV-cache rollout (set_position + bind_ptrs) as a SeaStepPatch array for sea_run_list_steps: step s reads its rows at
        x_base + s * x_stride, its condition values at c_base + s * c_stride, writes its rows at out_base + s * out_stride and sits at position pos0 + s of
        the caches.  None when the plan has no native launch list."""
        if self._clist is None:
            return None
        arr, _, relink = self._clist
        rows = []   # (address, kind, base, stride)

        def field_addr(tgt, field):
            if isinstance(tgt, list):   # a pointer argument kept in a record's Python args list: its native copy is a field of the SeaLaunchRec
                for i, rf, args, k in relink:
                    if args is tgt and k == field:
                        return C.addressof(arr[i]) + getattr(N.SeaLaunchRec, rf).offset
                raise KeyError("patched argument without a native copy")
            return C.addressof(tgt) + getattr(type(tgt), field).offset

        for st in self._pos_structs:
            if isinstance(st, N.SeaQkvCommon):
                rows.append((field_addr(st, "pos0"), 0, pos0, 1))
            else:
                rows.append((field_addr(st, "q_pos0"), 0, pos0, 1))
                rows.append((field_addr(st, "Tk"), 0, pos0 + self.T, 1))
        for tgt, field, off in self._x_patches:
            rows.append((field_addr(tgt, field), 1, x_base + off, x_stride))
        for tgt, field, off in self._out_patches:
            rows.append((field_addr(tgt, field), 1, out_base + off, out_stride))
        for tgt, field in self._c_patches:
            rows.append((field_addr(tgt, field), 1, c_base, c_stride))
        for st, field, base, step in self._hoisted:
            rows.append((field_addr(st, field), 1, base, step))
        tab = (N.SeaStepPatch * max(len(rows), 1))()
        for t, (a_, k_, b_, s_) in zip(tab, rows):
            t.addr, t.kind, t.base, t.stride = a_, k_, b_, s_
        return tab, len(rows)

    def run_steps(self, n_steps: int, x_base: int, x_stride: int, c_base: int, c_stride: int, out_base: int, out_stride: int, pos0: int = 0) -> bool:
        """n_steps consecutive KV-cache steps from position pos0 in ONE native call (sea_run_list_steps); False when the plan has no native list."""
        pt = self.step_patch_table(x_base, x_stride, c_base, c_stride, out_base, out_stride, pos0)
        if pt is None:
            return False
        assert pos0 + n_steps <= self.cap
        rc = N.lib().sea_run_list_steps(self._clist[0], self._clist[1], pt[0], pt[1], 0, n_steps, N.stream_ptr())
        self._bound = (None, None, None)   # the structs now hold the last step's pointers / position
        self.pos0 = pos0 + n_steps - 1 if n_steps > 0 else self.pos0
        if rc != 0:
            N.check(rc, "KV-cache rollout (sea_run_list_steps)")
        return True

    def _compile_list(self) -> None:
        """Lower self.records to one SeaLaunchRec array (include/sea_hip.h): a sequential replay is then ONE native call instead of a
        Python/ctypes round trip per launch.  Pointers into the argument structs are stable (the structs are patched in place)."""
        L = N.lib()
        recs = [r for r in self.records if r.fn is not None]
        arr = (N.SeaLaunchRec * max(len(recs), 1))()
        relink = []   # records whose pointer arguments live in the Python args list (patched by bind): copied again at bind time
        addr = lambda o: C.addressof(o)
        for i, r in enumerate(recs):
            c, a = arr[i], r.args
            if r.fn is L.sea_gemm_grouped:
                c.op, c.p0, c.n, c.dtype = N.OP_GEMM, addr(a[0]), a[1], a[2]
            elif r.fn is L.sea_qkv_rope_grouped:
                c.op, c.p0, c.n, c.p1, c.dtype = N.OP_QKV, addr(a[0]), a[1], addr(r.keep[1]), a[3]
            elif r.fn is L.sea_gemm_fewrows:
                c.op, c.p0, c.n, c.i0, c.i1, c.f0, c.dtype = N.OP_GEMM_FEW, addr(a[0]), a[2], a[3], a[4], a[5], a[6]
                c.p1 = addr(a[1]) if a[1] is not None else None
            elif r.fn is L.sea_qkv_rope_fewrows:
                c.op, c.p0, c.n, c.p1, c.f0, c.dtype = N.OP_QKV_FEW, addr(a[0]), a[2], addr(r.keep[2]), a[4], a[5]
                c.l0 = addr(a[1]) if a[1] is not None else 0
            elif r.fn is L.sea_attention_fwd:
                c.op, c.p0, c.dtype = N.OP_ATTN, addr(r.keep), a[1]
            elif r.fn is L.sea_mlp_fc1_ln_gelu:
                c.op, c.p0, c.n, c.f0, c.dtype = N.OP_MLP1, addr(a[0]), a[1], a[2], a[3]
            elif r.fn is L.sea_mlp_fc2_proj_norm:
                c.op, c.p0, c.n, c.f0, c.dtype = N.OP_MLP2, addr(a[0]), a[1], a[2], a[3]
            elif r.fn is L.sea_adaln_qkv:
                c.op, c.p0, c.n, c.p1, c.f0, c.dtype = N.OP_AQKV, addr(a[0]), a[1], addr(r.keep[1]), a[10], a[11]
                c.l0, c.i0 = (addr(a[3]) if a[3] is not None else 0), a[4]
                c.l1, c.i1 = (addr(a[5]) if a[5] is not None else 0), a[6]
                c.l2, c.i2 = (a[7] or 0), a[8]
                if a[8]:
                    relink.append((i, "l2", a, 7))   # the condition pointer of the row riders, patched at every bind
                c.l3 = addr(r.keep[4]) if r.keep[4] is not None else 0
            elif r.fn is L.sea_splitk_finish:
                c.op, c.p0, c.n, c.dtype = N.OP_SPLITK, addr(a[0]), a[1], a[2]
            elif r.fn is L.sea_mlp_block:
                c.op, c.p0, c.p1, c.n, c.f0, c.dtype = N.OP_MLPB, addr(a[0]), addr(a[1]), a[2], a[3], a[4]
            elif r.fn is L.sea_exchange_tail:
                c.op, c.p0, c.n, c.f0, c.dtype = N.OP_XTAIL, addr(r.keep), a[1], a[2], a[3]
            elif r.fn is L.sea_gemm_adaln:
                c.op, c.p0, c.n, c.f0, c.dtype = N.OP_ADALN, addr(a[0]), a[1], a[2], a[3]
            elif r.fn is L.sea_row_chain:
                c.op, c.p0, c.n, c.p1, c.f0, c.dtype = N.OP_CHAIN, addr(a[0]), a[1], addr(r.keep[1]), a[3], a[4]
            elif r.fn is L.sea_row_chain_riders:
                c.op, c.p0, c.n, c.p1, c.f0, c.dtype = N.OP_CHAIN, addr(a[0]), a[1], addr(r.keep[1]), a[8], a[9]
                c.l0, c.i0, c.i1, c.i2 = addr(a[3]), a[4], a[5], a[6]
                c.l1 = addr(r.keep[3]) if r.keep[3] is not None else 0
            elif r.fn is L.sea_gemm_rownorm:
                c.op, c.p0, c.n, c.f0, c.dtype = N.OP_GEMM_NORM, addr(a[0]), a[1], a[2], a[3]
            elif r.fn is L.sea_rownorm:
                c.op, c.p0, c.n, c.i0, c.i1, c.i2, c.i3, c.f0, c.dtype = N.OP_NORM, addr(a[0]), a[1], a[2], a[3], a[4], a[5], a[6], a[7]
            elif r.fn is L.sea_silu_outer or r.fn is L.sea_silu_outer_ib:
                c.op, c.p0, c.n, c.i0, c.dtype = N.OP_SILU, (addr(a[0]) if a[0] is not None else None), a[1], a[3], a[4]
                if r.fn is L.sea_silu_outer_ib and a[5] is not None:
                    c.l0, c.l1 = addr(a[5]), a[6]
                relink.append((i, "p1", a, 2))
            elif r.fn is L.sea_ib_add:
                c.op, c.p0 = N.OP_IB, addr(r.keep)
            elif r.fn is L.sea_convert_f32_to_act:
                c.op, c.l0, c.p1, c.l1, c.l2, c.l3, c.dtype = N.OP_CONVERT, a[1], a[2], a[3], a[4], a[5], a[6]
                relink.append((i, "p0", a, 0))
            else:
                return  # a record the list runner does not know (training plans): keep the per-launch replay
        self._clist = (arr, len(recs), relink)
        self._relink()

    def _relink(self) -> None:
        if self._clist is not None:
            arr, _, relink = self._clist
            for i, field, args, k in relink:
                setattr(arr[i], field, args[k] if (args[k] is not None or field[0] == "p") else 0)   # (l0..l3 are integers: an unbound pointer is 0)

    def run(self, concurrent: bool = False) -> None:
        """Replay the launch list.  Sequentially on the current stream (record order is a valid order), or — `concurrent` — with every
        lane on its own stream, forked from / joined to the current stream by events; inside a graph capture the lanes become
        parallel branches of the graph."""
        main = torch.cuda.current_stream()
        stream = main.cuda_stream
        if not concurrent and self._clist is not None:
            rc = N.lib().sea_run_list(self._clist[0], self._clist[1], stream)
            if rc != 0:
                N.check(rc, "plan replay (sea_run_list)")
            return
        if not concurrent:
            for r in self.records:
                if r.fn is None:
                    continue
                rc = r.fn(*r.args, stream)
                if rc != 0:
                    N.check(rc, r.name)
            return
        open_lanes = set()
        for r in self.records:
            if r.fn is None:
                st = self._lane_streams.get(r.lane)
                if st is None:
                    st = self._lane_streams[r.lane] = torch.cuda.Stream(device=self.eng.device)
                if r.name == "fork":
                    st.wait_stream(main)
                    open_lanes.add(r.lane)
                else:
                    main.wait_stream(st)
                    open_lanes.discard(r.lane)
                continue
            rc = r.fn(*r.args, stream if r.lane == 0 else self._lane_streams[r.lane].cuda_stream)
            if rc != 0:
                N.check(rc, r.name)
        for lane in open_lanes:  # every lane rejoins (a graph capture requires it)
            main.wait_stream(self._lane_streams[lane])

    def time_records(self, iters: int = 10) -> List[Tuple[str, float]]:
        """Average device time of every launch of the plan, in milliseconds, from HIP events recorded on the launch stream
        around each launch (diagnostics / bench roofline)."""
        stream = N.stream_ptr()
        recs = [r for r in self.records if r.fn is not None]
        n = len(recs)
        tot = [0.0] * n
        for _ in range(iters):
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
            evs[0].record()
            for k, r in enumerate(recs):
                rc = r.fn(*r.args, stream)
                if rc != 0:
                    N.check(rc, r.name)
                evs[k + 1].record()
            torch.cuda.synchronize()
            for k in range(n):
                tot[k] += evs[k].elapsed_time(evs[k + 1])
        return [(r.name, t / iters) for r, t in zip(recs, tot)]


def blk_pe(eng: "TemporalEngine", layer: int) -> torch.Tensor:
    """The block's sinusoidal table [max_len, D] (PositionalEncoding buffer `pe`, models/base_blocks.py:355-368) on the device."""
    return eng.model.blocks[layer].pos_encoder.pe[0].to(device=eng.device, dtype=torch.float32)


def _require_gpu(device: torch.device) -> None:
    """The engine's device guard (a seam: tests/test_plan_forms_cpu.py builds plans in host memory past it; nothing can RUN there)."""
    if device.type != "cuda":
        raise RuntimeError("sea_amd: TemporalModel runs only on an MI355X (no CPU fallback)")


class TemporalEngine:
    """Owns the flat parameter buffers of one TemporalModel on one GPU and the plans built over them."""

    def __init__(self, model: torch.nn.Module, device: torch.device, act_dtype: torch.dtype):
        N.lib()
        _require_gpu(device)
        m = model
        self.ib_mode = {"mlp": 0, "linear": 1, "fourier": 2}.get(m.ib_scale_mode.lower(), -1)
        if (m.exchange_mode not in ("sea", "addition", "simple", "pool") or self.ib_mode < 0 or m.ib_addition_mode.lower() not in ("add", "none", "attention", "concat")
                or (self.ib_mode == 0 and m.ib_mlp_layers != 1) or m.ib_num != 1 or (self.ib_mode != 0 and m.embed_dim % 8 and m.ib_addition_mode.lower() != "concat")):
            raise NotImplementedError(
                "sea_amd native path covers exchange_mode in {'sea', 'addition', 'simple', 'pool'}, ib_scale_mode in {'mlp', 'linear', 'fourier'}, ib_addition_mode in "
                "{'add', 'attention', 'concat', 'none'}, ib_mlp_layers=1, ib_num=1; got "
                f"{m.exchange_mode}/{m.ib_scale_mode}/{m.ib_addition_mode}/{m.ib_mlp_layers}/{m.ib_num}")
        if m.ib_addition_mode.lower() == "concat" and m.add_info_after_cross:
            raise NotImplementedError("sea_amd: ib_addition_mode='concat' needs add_info_after_cross=False (with the info-bottleneck step after the exchange the "
                                      "reference's own forward fails: its attention modules are built for rows that are already widened, models/temporal.py:48,74-76,126-139)")
        E, H, D = m.internal_embed_dim, m.n_heads, m.down_dim
        for hd, what in ((E // H, "self"),) + (((D // H, "cross"),) if m.exchange_mode in ("sea", "pool") else ()):
            if hd % 8 or not 8 <= hd <= 256 or hd * H != (E if what == "self" else D):   # (the attention kernels' set: sea_attention_fwd / _bwd)
                raise NotImplementedError(f"sea_amd: unsupported {what}-attention head dim {(E if what == 'self' else D) / H:g} (supported: multiples of 8 from 8 to 256)")
        if m.src_len < 0:
            raise NotImplementedError("sea_amd: src_len must be >= 0")
        if self.ib_mode == 0 and m.ib_hidden > 64:
            raise NotImplementedError("sea_amd: info-bottleneck hidden width (scale_ratio) must be <= 64")
        self.model, self.device, self.act_dtype = model, device, act_dtype
        self.params = FlatParams(model, device, act_dtype)
        # load_state_dict copies into the parameters, which alias flat32 but count their versions themselves (flat32._version does not move): the shadow is
        # refreshed — and the condition memo's weight epoch moved on — right behind the load.  (A write through `p.data` moves no version at all:
        # _WatchedParameter reports the read of `.data` instead.)
        model.register_load_state_dict_post_hook(lambda module, incompatible: self.params.sync(force=True))
        blk = model.blocks[0]
        self.rope_self = torch.view_as_real(blk.attn["self"][0].freqs_cis.to(device)).contiguous()
        self.rope_cross = None
        if m.exchange_mode == "sea":
            self.rope_cross = torch.view_as_real(blk.cross_attn[0][0].freqs_cis.to(device)).contiguous()
        elif m.exchange_mode == "pool":
            self.rope_cross = torch.view_as_real(blk.cross_attn[0].freqs_cis.to(device)).contiguous()
        self._eyes: Dict[int, torch.Tensor] = {}
        self._plans: Dict[Tuple, Plan] = {}
        self._graphs: Dict[Tuple, Tuple] = {}
        self._train_plans: Dict[Tuple, object] = {}
        self._kv_fast: Dict[int, object] = {}          # B -> kv_engine.KvFast
        self.grads: Optional[torch.Tensor] = None      # flat fp32 gradient buffer, same layout as params.flat32
        self.grads_dirty = False                       # True once a backward has accumulated into it since the last zero
        self._drop_step = 0                            # dropout streams are re-keyed every training forward
        self._dp_overlap: Optional[Tuple[int, bool]] = None   # (world size, slices under the backward?) — see dp_overlap()
        self._loss_ws: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None

    def eye(self, n: int) -> torch.Tensor:
        """Identity in the activation dtype: W of the GEMM that sums A segments and applies GELU ('addition' exchange)."""
        e = self._eyes.get(n)
        if e is None:
            e = self._eyes[n] = torch.eye(n, device=self.device, dtype=self.act_dtype)
        return e

    def rope_identity(self, hd: int) -> torch.Tensor:
        """A rotation table of zero angles for the un-rotated attention of ib_addition_mode 'attention' (models/base_blocks.py:222-243)."""
        t = self._eyes.get(("rope", hd))
        if t is None:
            t = torch.zeros(_round_up(self.model.max_len, 8), hd // 2, 2, device=self.device, dtype=torch.float32)
            t[..., 0] = 1.0
            self._eyes[("rope", hd)] = t
        return t

    def plan(self, B: int, T: int, mode: str = "full", cond=None) -> Plan:
        if mode == "step" and self.model.exchange_mode == "pool":
            raise NotImplementedError(KV_NO_POOL)
        if mode == "step" and self.model.ib_addition_mode.lower() == "attention":
            raise NotImplementedError(KV_NO_IB_ATTENTION)
        key = (B, T, mode) if cond is None else (B, T, mode, id(cond))
        p = self._plans.get(key)
        if p is None:
            if T > self.model.max_len:
                raise ValueError(f"sequence length {T} exceeds max_len {self.model.max_len}")
            if cond is not None:   # one hoisted step plan at a time per batch size: its predecessor's condition buffers are released with it
                for k in [k for k in self._plans if len(k) == 4 and k[:3] == (B, T, mode)]:
                    del self._plans[k]
            p = Plan(self, B, T, mode, cond=cond)
            self._plans[key] = p
        return p

    # ------------------------------------------------------------------ training
    def ensure_grads(self) -> None:
        if self.grads is None:
            self.grads = torch.zeros(self.params.n_total, device=self.device, dtype=torch.float32)

    def grad_view(self, name: str) -> torch.Tensor:
        o, shp = self.params.offsets[name]
        n = 1
        for s in shp:
            n *= s
        return self.grads[o:o + n].view(shp)

    def grad_vec(self, name: str, n: Optional[int] = None) -> torch.Tensor:
        o, shp = self.params.offsets[name]
        return self.grads[o:o + (shp[0] if n is None else n)]

    def grad_mat(self, name: str, rows: Optional[int] = None) -> torch.Tensor:
        o, shp = self.params.offsets[name]
        r = shp[0] if rows is None else rows
        return self.grads[o:o + r * shp[1]].view(r, shp[1])

    def zero_grads(self) -> None:
        if self.grads is not None:
            self.grads.zero_()
        self.grads_dirty = False

    def train_plan(self, B: int, T: int, want_dx: bool = False, want_dc: bool = False):
        """want_dx / want_dc: the backward also writes d loss / d x and d loss / d condition (TrainPlan.bind_input_grads); a plan of its own."""
        from .train_engine import TrainPlan

        m = self.model
        thr = int(round(256 * m.dropout_p)) if (m.training and m.dropout_p > 0) else 0
        if thr > 255:
            raise ValueError("dropout probability too close to 1")
        dp = self.dp_overlap()
        key = (B, T, thr, dp, bool(want_dx), bool(want_dc))
        p = self._train_plans.get(key)
        if p is None:
            if T > m.max_len:
                raise ValueError(f"sequence length {T} exceeds max_len {m.max_len}")
            p = TrainPlan(self, B, T, drop_thr=thr, dp=dp, want_dx=want_dx, want_dc=want_dc)
            self._train_plans[key] = p
        return p

    def dp_overlap(self) -> bool:
        """Reduce the gradient buffer in slices under the backward (parallel.OverlappedGradientReduce)?  Decided ONCE per engine and process group, and
        AGREED between the ranks (a MIN all-reduce of each rank's SEA_DP_OVERLAP switch): the number of collectives a step issues follows from it, so ranks
        that disagreed, or a switch flipped between two steps, would deadlock.  False without a process group / at world size 1; a group initialised later
        is seen at the next step (the training plans are keyed on the answer)."""
        import torch.distributed as dist

        world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
        if world == 1:
            from .parallel import rehearse

            if not (rehearse() and dist.is_available() and dist.is_initialized()):   # (SEA_DP_REHEARSE=1: one rank issues the collectives of a larger world)
                return False
        if self._dp_overlap is None or self._dp_overlap[0] != world:
            want = torch.tensor([0 if os.environ.get("SEA_DP_OVERLAP", "1") == "0" else 1], device=self.device, dtype=torch.int32)
            dist.all_reduce(want, op=dist.ReduceOp.MIN)
            self._dp_overlap = (world, bool(int(want.item())))
        return self._dp_overlap[1]

    def forward_train(self, x: torch.Tensor, ib: torch.Tensor, want_dx: bool = False, want_dc: bool = False):
        """Forward that keeps the activations the backward needs.  Returns (out, plan).  want_dx / want_dc: see train_plan."""
        B, T, F, E = x.shape
        x, ib = x.contiguous(), ib.contiguous()
        out = torch.empty_like(x)
        self.params.sync()
        self.params.sync_transposed()
        p = self.train_plan(B, T, want_dx, want_dc)
        p.bind(x, ib, out)
        p.held = (x, ib)  # the backward list reads the inputs again: keep them alive until the next forward
        p.generation = getattr(p, "generation", 0) + 1   # identifies the activation set now in the plan's workspace (autograd.py checks it)
        if p.drop_thr > 0:
            self._drop_step += 1
            from .parallel import rank as _dp_rank   # data parallel: every rank draws its own masks (the shards are different trajectories of one batch)
            p.set_dropout_seed((torch.initial_seed() * 0x9E3779B1 + self._drop_step * 0x85EBCA77 + _dp_rank() * 0xC2B2AE35) & 0xFFFFFFFF)
        p.run()
        return out, p

    def backward(self, plan, dout: torch.Tensor, on_bucket=None, dx: Optional[torch.Tensor] = None, dc: Optional[torch.Tensor] = None) -> None:
        """Accumulate d loss / d parameters into self.grads from dout = d loss / d out ([B,T,F,E] fp32, contiguous).  `on_bucket(lo, hi)`: called
        as soon as self.grads[lo:hi] is final (TrainPlan.grad_buckets), while later launches are still being issued.  A plan built with want_dx /
        want_dc also stores d loss / d x into dx ([B,T,F,E] fp32, contiguous) and ADDS d loss / d condition into dc ([B*T] fp32, zeroed by the caller)."""
        assert dout.is_contiguous() and dout.dtype == torch.float32
        for t, shape in ((dx, dout.shape), (dc, (plan.M,))):
            assert t is None or (t.is_contiguous() and t.dtype == torch.float32 and t.numel() == torch.Size(shape).numel() and t.device == dout.device)
        plan.bind_dout(dout.data_ptr())
        plan.bind_input_grads(N.ptr(dx), N.ptr(dc))
        plan._bound_dout = dout          # held until the next backward: the launch list knows it by address only
        plan._bound_input_grads = (dx, dc)
        if ptrcheck.always():
            plan.audit(owners=tuple(t for t in (dout, dx, dc) if t is not None))
        plan.set_grads_fresh(not self.grads_dirty)   # a backward into zeros (the usual step) lets the big weight-gradient launches store instead of add
        plan.run_backward(on_bucket)
        self.grads_dirty = True

    def mse_loss_and_grad(self, out: torch.Tensor, target: torch.Tensor, grad_scale: float = 1.0):
        """loss = mean((out - target)^2) and dout = grad_scale * d loss / d out in one kernel pass.  `target`: out's shape, float32."""
        N.require_same_operand(out, target, "mse_loss_and_grad", f32=True)
        if self._loss_ws is None or self._loss_ws[0].numel() != out.numel():
            self._loss_ws = (torch.empty_like(out), torch.zeros(1, device=self.device), torch.empty(1024, device=self.device))
        dout, loss, partial = self._loss_ws
        target = target.contiguous()
        N.check(N.lib().sea_mse_fwd_bwd(out.data_ptr(), target.data_ptr(), dout.data_ptr(), loss.data_ptr(), partial.data_ptr(), 1024,
                                        out.numel(), grad_scale, N.stream_ptr()), "sea_mse_fwd_bwd")
        return loss, dout

    def train_step(self, x: torch.Tensor, target: torch.Tensor, ib: torch.Tensor, optimizer, allreduce: bool = True, loss_weight: float = 1.0) -> torch.Tensor:
        """One fused train step (train/train_temporal.py:254-258): zero grads, forward, MSE + its gradient, backward, the gradient
        all-reduce when torch.distributed is initialised (the MLP slice as soon as it is final, the rest after the backward: sea_amd/parallel.py) (`allreduce=False`: a rank-local step, e.g. to time the step without the collective),
        AdamW.  Returns the local loss as a device scalar (no host sync).  `loss_weight` scales this rank's loss gradient (an uneven data-parallel
        shard: rows * world / global rows, train/train_temporal.py)."""
        from .parallel import OverlappedGradientReduce

        optimizer.zero_grad(set_to_none=False)
        out, plan = self.forward_train(x, ib)
        loss, dout = self.mse_loss_and_grad(out, target, grad_scale=float(loss_weight))
        red = OverlappedGradientReduce(self.grads, self.params.n_live, overlap=plan.dp) if allreduce else None
        self.backward(plan, dout, red.on_bucket if (red is not None and red.active) else None)
        scale = red.finish() if red is not None else 1.0
        self.last_allreduce_calls = red.calls if red is not None else 0
        if hasattr(optimizer, "mark_reduced"):
            optimizer.mark_reduced(scale)       # FlatAdamW.step() would otherwise all-reduce the buffer itself
        else:
            optimizer.grad_scale = scale
        optimizer.step()
        return loss

    def forward(self, x: torch.Tensor, ib: torch.Tensor) -> torch.Tensor:
        """TemporalModel.forward: x [B,T,F,E] fp32, ib [B,T,1] fp32 -> [B,T,F,E] fp32."""
        B, T, F, E = x.shape
        x = x.contiguous()
        ib = ib.contiguous()
        out = torch.empty_like(x)
        self.params.sync()
        p = self.plan(B, T, "full")
        p.bind(x, ib, out)
        p.run()
        return out

    def forward_graphed(self, x: torch.Tensor, ib: torch.Tensor) -> torch.Tensor:
        """Same forward replayed as ONE captured HIP graph (launch-bound regime: ~30 short kernels per layer).  The graph is
        keyed on the input tensors' addresses: write new data INTO x / ib, the returned tensor is reused between calls."""
        B, T, F, E = x.shape
        assert x.is_contiguous() and ib.is_contiguous()
        self.params.sync()
        key = (B, T, x.data_ptr(), ib.data_ptr())
        hit = self._graphs.get(key)
        if hit is None:
            out = torch.empty_like(x)
            p = Plan(self, B, T, "full")  # a private plan: its workspace addresses are baked into the graph
            p.bind(x, ib, out)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                p.run()  # warm-up outside capture (one-time function attributes, lazy module loading)
            torch.cuda.current_stream().wait_stream(side)
            # A capture begins with a flush of the caching allocator (freed blocks are UNMAPPED): everything issued so far — plain replays of other plans
            # that may still write tensors the caller has since dropped — has to be complete before that, or those launches fault (seen in round 2 as a
            # "Memory access fault" when bench.py captured a graph behind 200 plain forwards).  Once per (shape, inputs): not on the replay path.
            torch.cuda.synchronize(self.device)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                p.run(concurrent=_switches.plan("graph_lanes", "1") != "0")
            hit = (graph, out, p, x, ib)
            self._graphs[key] = hit
        hit[0].replay()
        return hit[1]

    def rollout_kv(self, x0: torch.Tensor, ib: torch.Tensor, n_steps: int) -> torch.Tensor:
        """Exact KV-cache rollout (the loop of utils/train_utils.py:202-209 without recomputing the prefix): step s feeds the row
        at position s, appends its K/V to the per-layer caches and attends over positions <= s.  x0 [B,k,F,E] holds the known states at positions
        0 .. k-1, ib [B,>=k+n_steps-1,1] -> the predictions of positions k .. k+n_steps-1 [B, n_steps, F, E].  k > 1: one full-context forward over the
        context (the prefill) predicts position k and leaves the keys / values of positions 0 .. k-1, which one sea_kv_cache_fill launch moves into the
        caches; the decode continues from position k.  The trajectory is kept time-major [steps+1, B, F, E] so that every step reads and writes
        contiguous [B, F, E] slabs with no copies."""
        from . import kv_engine

        B, k, F, E = x0.shape
        kv_engine.check_context(self.model, x0, ib, n_steps)
        if self.model.src_len > 0:
            # the reference masks with tril(diagonal=src_len) (models/base_blocks.py:173, 265): in its recompute loop the rows already produced re-attend
            # to the src_len rows appended after them, so their K/V and everything downstream change from step to step — a cache is not exact
            raise NotImplementedError(KV_NO_SRC_LEN)
        if kv_engine.supported(self, B):
            # small models: seven launches per layer and step, condition-only work batched over all steps up front (sea_kv_rollout)
            kf = self._kv_fast.get(B)
            if kf is None:
                kf = self._kv_fast[B] = kv_engine.KvFast(self, B)
            return kf.rollout(x0, ib, n_steps)
        self.params.sync()
        first = 0 if k == 1 else k                        # position of the step loop's first step (k > 1: the prefill predicts position k)
        full = None
        if k > 1:
            if n_steps == 0:
                return torch.empty(B, 0, F, E, device=self.device, dtype=torch.float32)
            pred, full = kv_engine.prefill(self, x0, ib)
            n_steps -= 1
            if n_steps == 0:
                return pred.unsqueeze(1).contiguous()
        traj = torch.empty(n_steps + 1, B, F, E, device=self.device, dtype=torch.float32)
        traj[0].copy_(x0[:, 0] if k == 1 else pred)
        cond = ib[:, first:first + n_steps, 0].t().contiguous()  # [n_steps, B]
        # What depends on the condition only (the AdaLN modulations of every module, the info-bottleneck term) is evaluated for ALL steps by one batched
        # pass before the loop — the full-context plan's own silu / grouped-GEMM / ib launches on n_steps * B rows — instead of once per step on B rows:
        # at the shipped cylinder width (embed_dim 1024) that is two launches and 31 % of the weight bytes of every step.  SEA_KV=hoist=0: per step.
        cp = None
        m = self.model
        if _switches.kv("hoist", "1") != "0" and (m.LN_type.lower() == "adaln" or (m.ib_addition_mode.lower() == "add" and m.add_info_after_cross)) \
                and m.ib_addition_mode.lower() in ("add", "none"):
            cp = kv_engine.cond_plan_for(self, n_steps * B)
            for t in cp.ibufs:
                t.zero_()
            cp.bind_ptrs(0, cond.data_ptr(), 0)
            if not cp._audited or ptrcheck.always():
                cp.audit(owners=(cond,))
            cp.run()
        p = self.plan(B, 1, "step", cond=cp)
        if full is not None:   # the context's keys / values -> the step plan's caches (positions 0 .. k-1)
            kv_engine.cache_fill_for(p, full, lambda: kv_engine.CacheFill(
                full, [dict(K=src[0], Vt=src[1], Kd=dst[0], Vd=dst[1]) for src, dst in _kv_pairs(full.kv, p.kv)],
                [t for _, dst in _kv_pairs(full.kv, p.kv) for t in dst], False, f"step plan B={B}")).run()
        slab = B * F * E * 4
        base, cbase = traj.data_ptr(), cond.data_ptr()
        if not p._audited or ptrcheck.always():   # the step plan is bound by raw address: audit it once against the buffers it will walk
            p.set_position(first)
            p.bind_ptrs(base, cbase, base + slab)
            p.set_hoisted_step(0)
            p.audit(owners=(traj, cond))
        # the step loop in native code (the plan's launch list + a table of the per-step edits); SEA_KV=loop=python: one Python round trip per step
        if _switches.kv("loop", "native") == "python" or not p.run_steps(n_steps, base, slab, cbase, B * 4, base + slab, slab, first):
            for s in range(n_steps):
                p.set_position(first + s)
                p.bind_ptrs(base + s * slab, cbase + s * B * 4, base + (s + 1) * slab)
                p.set_hoisted_step(s)
                p.run()
        return (traj[1:] if k == 1 else traj).permute(1, 0, 2, 3).contiguous()

    def open_rollout(self, x0: torch.Tensor, ib: torch.Tensor):
        """A stateful KV-cache rollout (rollout_session.RolloutSession) from the known states x0 [B, k, F, E] and the conditions ib [B, k-1, 1] of
        positions 0 .. k-2: the session owns its caches between calls (step / advance / rewind / fork)."""
        from . import rollout_session

        with torch.no_grad():   # gradients through a session are not covered: the history is taken by value
            return rollout_session.RolloutSession(self, x0, ib)
