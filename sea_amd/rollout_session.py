"""A stateful KV-cache rollout: the loop of utils/train_utils.py:202-209 taken one call at a time.  `rollout()` / `engine.rollout_kv` need every future
condition up front and forget their caches when they return; a RolloutSession owns the caches between calls, so that the next condition can be chosen
after the last state has been seen (closed loops, co-simulation), the fed-back state can be replaced (data assimilation), the rollout can go back
(`rewind`) and many futures can branch off one shared history (`fork`: one sea_kv_cache_fork launch per 32 cache tensors instead of a prefill of the
repeated history) or be kept, dropped, repeated and reordered afterwards (`select`, `resample`: one sea_kv_cache_gather launch per 32 cache tensors, which
also converts between the two value-cache layouts, instead of a prefill of the selected histories).

Positions: `position` p is the index of the newest known state.  The caches hold the keys / values of positions < p; a step feeds position p — its
state (stored, or replaced through `state=`) and its condition, which arrives with the step — and predicts position p + 1, exactly as the reference's
`model(a, ib[:, :len(a)])` does with len(a) = p + 1 states.  So opening on k states needs the k - 1 conditions of positions 0 .. k-2 only.

What a session holds: the trajectory [max_len + 1, B, F, E] and the conditions [max_len, B] (fp32, time-major: every step reads and writes contiguous
slabs), and per decode form
  * sea_kv_rollout (kv_engine.supported): a private kv_engine.KvFast — caches, workspace, hand-off words — and its condition plans;
  * the generic step plan: a private engine.Plan(B, 1, 'step') kept out of the engine's plan cache — its K / V^T buffers are the caches — built over
    the session's single-step condition plan; a longer `advance` points the plan's hoisted condition pointers at its own, larger condition plan.
The single-step condition plan (M = B rows) lives as long as the session, the `advance` one is kept for one row count at a time.

Gradients through a session are not covered: step / advance / fork / select / resample run under torch.no_grad(), so a condition or state that requires grad is
taken by value and no autograd graph is kept alive by the session's buffers.

Weights are read through the engine's flat buffers (`params.sync()` at every call): a weight changed in mid-session takes effect from the next step
on while the caches still hold keys / values computed with the old ones — re-open the session after an optimizer step.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch

from . import _native as N
from . import _switches
from . import kv_engine
from . import ops
from . import ptrcheck
from .engine import KV_NO_IB_ATTENTION, KV_NO_POOL, KV_NO_SRC_LEN, Plan, _Rec, _kv_pairs


def check_open(model, x0: torch.Tensor, ib: torch.Tensor) -> Tuple[int, int]:
    """(B, k) of a session opened on x0 [B, k, F, E] and ib [B, k-1, 1]; raises — on the host, before any device is touched — NotImplementedError for the
    models the KV-cache rollout refuses (a session has no recompute fallback: its point is the cache) and ValueError for bad shapes."""
    if getattr(model, "src_len", 0) > 0:
        raise NotImplementedError(KV_NO_SRC_LEN)
    if getattr(model, "exchange_mode", "sea") == "pool":
        raise NotImplementedError(KV_NO_POOL)
    if str(getattr(model, "ib_addition_mode", "add")).lower() == "attention":
        raise NotImplementedError(KV_NO_IB_ATTENTION)
    F, E = model.num_variables, model.embed_dim
    if x0.dim() != 4 or x0.shape[2] != F or x0.shape[3] != E or x0.shape[0] < 1:
        raise ValueError(f"open_rollout: x0 {tuple(x0.shape)} must be [B, k, F={F}, E={E}]")
    B, k = x0.shape[0], x0.shape[1]
    if k < 1:
        raise ValueError("open_rollout: the history x0 [B, k, F, E] needs k >= 1 known states")
    if k > model.max_len:
        raise ValueError(f"open_rollout: a history of {k} states leaves no step to take: its newest position {k - 1} is not below max_len {model.max_len}")
    if ib.dim() != 3 or tuple(ib.shape) != (B, k - 1, 1):
        raise ValueError(f"open_rollout: ib {tuple(ib.shape)} must be [B={B}, k - 1 = {k - 1}, 1]: the conditions of positions 0 .. k-2 (the condition of the "
                         "newest state arrives with the first step)")
    return B, k


class CacheFork:
    """The sea_kv_cache_fork launch (include/sea_hip.h) from one session's caches into those of a session with n times the trajectories; audited by
    sea_amd/ptrcheck.py against the cache tensors of both."""

    def __init__(self, entries: List[dict], dtype: torch.dtype, what: str):
        self.dtype, self.what = dtype, what
        self.owners = [d[k] for d in entries for k in ("src", "dst")]
        self.arr = (N.SeaKvFork * len(entries))()
        for g, d in zip(self.arr, entries):
            ops.fill_kv_fork(g, **d)
        self.rec = _Rec(N.lib().sea_kv_cache_fork, [self.arr, len(entries), N.dtype_code(dtype)], "kv.cache_fork", self.arr)
        self.audit()

    def audit(self) -> int:
        R = ptrcheck.Ranges()
        for t in self.owners:
            R.add_tensor(t, "session cache")
        return ptrcheck.check_records([self.rec], R, 4 if self.dtype == torch.float32 else 2, f"CacheFork {self.what}")

    def run(self) -> None:
        N.check(N.lib().sea_kv_cache_fork(self.arr, len(self.arr), N.dtype_code(self.dtype), N.stream_ptr()), "sea_kv_cache_fork")


class CacheGather:
    """The sea_kv_cache_gather launch (include/sea_hip.h) from one session's caches into those of a session whose trajectory j is the source's
    trajectory index[j]; an entry converts between value rows and V^T where the two sessions decode from different layouts.  Audited by
    sea_amd/ptrcheck.py against the cache tensors of both sessions and the index tensor (int32, on the device, shared by every entry)."""

    def __init__(self, entries: List[dict], index: torch.Tensor, dtype: torch.dtype, what: str):
        self.dtype, self.what, self.index = dtype, what, index
        self.owners = [d[k] for d in entries for k in ("src", "dst")] + [index]
        self.arr = (N.SeaKvGather * len(entries))()
        for g, d in zip(self.arr, entries):
            ops.fill_kv_gather(g, index=index, **d)
        self.rec = _Rec(N.lib().sea_kv_cache_gather, [self.arr, len(entries), N.dtype_code(dtype)], "kv.cache_gather", self.arr)
        self.audit()

    def audit(self) -> int:
        R = ptrcheck.Ranges()
        for t in self.owners:
            R.add_tensor(t, "session cache")
        return ptrcheck.check_records([self.rec], R, 4 if self.dtype == torch.float32 else 2, f"CacheGather {self.what}")

    def run(self) -> None:
        N.check(N.lib().sea_kv_cache_gather(self.arr, len(self.arr), N.dtype_code(self.dtype), N.stream_ptr()), "sea_kv_cache_gather")


def check_select(B: int, index) -> List[int]:
    """The index of select / resample on a session of B trajectories as a list of ints: a 1-D list, tuple or integer tensor (host or device: a device
    tensor is copied to the host here, which synchronises) of length >= 1 with values in [0, B), duplicates allowed.  Raises ValueError."""
    what = "rollout session: select"
    if torch.is_tensor(index):
        if index.dim() != 1 or index.dtype == torch.bool or index.is_floating_point() or index.is_complex():
            raise ValueError(f"{what}: index must be a 1-D integer tensor, got {tuple(index.shape)} {index.dtype}")
        index = index.detach().cpu()
    elif not isinstance(index, (list, tuple)):
        raise ValueError(f"{what}: index must be a list, a tuple or an integer tensor, got {type(index).__name__}")
    return ops.check_gather_index(index, [B], [], what)


def _own(view: torch.Tensor) -> torch.Tensor:
    """A contiguous tensor of its own.  (`.contiguous()` is no copy where it finds nothing to move — a permuted view whose moved dimension has
    size 1, i.e. B = 1 or one step — and would hand out session storage that a later call overwrites.)"""
    return view.clone(memory_format=torch.contiguous_format)


def _hoists(m) -> bool:
    """Does the generic step plan read condition-only work from a condition plan?  (engine.rollout_kv's own rule.)"""
    return (_switches.kv("hoist", "1") != "0" and (m.LN_type.lower() == "adaln" or (m.ib_addition_mode.lower() == "add" and m.add_info_after_cross))
            and m.ib_addition_mode.lower() in ("add", "none"))


class RolloutSession:
    """See the module docstring.  Built by TemporalEngine.open_rollout / utils.train_utils.open_rollout."""

    def __init__(self, eng, x0: torch.Tensor, ib: torch.Tensor, forked_by: Optional[str] = None):
        m = eng.model
        B, k = check_open(m, x0, ib)
        self.eng, self.B, self.F, self.E, self.max_len = eng, B, m.num_variables, m.embed_dim, m.max_len
        self.forked_by = forked_by          # None: opened; 'copy' / 'prefill': how fork() filled this session's caches; 'gather': select()
        self._closed = False
        self._alloc()
        self.traj[:k].copy_(x0.to(device=eng.device, dtype=torch.float32).permute(1, 0, 2, 3))
        if k > 1:
            self.conds[:k - 1].copy_(ib.to(device=eng.device, dtype=torch.float32)[:, :, 0].t())
            # positions 0 .. k-2: one full-context forward + one sea_kv_cache_fill launch (its prediction of position k-1 is not needed: that state is known)
            _, full = kv_engine.prefill(eng, self.traj[:k - 1].permute(1, 0, 2, 3).contiguous(), self.conds[:k - 1].t().unsqueeze(-1).contiguous())
            self._fill(full).run()
        else:
            eng.params.sync()
        self.position = k - 1

    # ------------------------------------------------------------------ construction
    def _alloc(self) -> None:
        """Buffers and decode objects of a session of self.B trajectories (nothing is launched)."""
        eng, B = self.eng, self.B
        f32 = torch.float32
        self.traj = torch.empty(self.max_len + 1, B, self.F, self.E, device=eng.device, dtype=f32)   # indexed by absolute position
        self.conds = torch.zeros(self.max_len, B, device=eng.device, dtype=f32)                      # row p: the condition of position p
        self.slab = B * self.F * self.E * 4
        self.fast = kv_engine.supported(eng, B)
        self.kv_fast: Optional[kv_engine.KvFast] = None
        self.step_plan: Optional[Plan] = None
        self._cond_step: Optional[kv_engine.CondPlan] = None       # M = B rows: kept for the session's lifetime
        self._cond_adv: Dict[int, kv_engine.CondPlan] = {}         # M = n * B rows of the last advance(n): one row count at a time
        self._bound_cond = None                                    # the condition plan the decode's pointers look at
        self._hoist_tabs: Dict[int, list] = {}                     # id(condition plan) -> the step plan's hoisted-pointer table over its buffers
        self._plan_audited = set()
        m = eng.model
        if self.fast:
            kf = self.kv_fast = kv_engine.KvFast(eng, B)           # private: the engine's own (eng._kv_fast) is shared by every rollout_kv of this B
            kf.G.traj = self.traj.data_ptr()
            self._need_cond = kf.adaln or kf.has_ib
        else:
            self._need_cond = _hoists(m)
        if self._need_cond:
            self._cond_step = kv_engine.CondPlan(eng, B)
        if not self.fast:
            self.step_plan = Plan(eng, B, 1, "step", cond=self._cond_step)   # private: not in eng._plans
            if self._cond_step is not None:
                self._hoist_tabs[id(self._cond_step)] = list(self.step_plan._hoisted)

    def _fill(self, full: Plan) -> kv_engine.CacheFill:
        if self.fast:
            return self.kv_fast._fill(full)
        p = self.step_plan
        return kv_engine.cache_fill_for(p, full, lambda: kv_engine.CacheFill(
            full, [dict(K=src[0], Vt=src[1], Kd=dst[0], Vd=dst[1]) for src, dst in _kv_pairs(full.kv, p.kv)],
            [t for _, dst in _kv_pairs(full.kv, p.kv) for t in dst], False, f"session step plan B={self.B}"))

    def _caches(self) -> List[Tuple[torch.Tensor, bool]]:
        """Every cache tensor of the decode, in a fixed order, with its layout (True: [B, H, hd, cap], the generic step plan's V^T)."""
        out: List[Tuple[torch.Tensor, bool]] = []
        if self.fast:
            kf = self.kv_fast
            for l in range(kf.L):
                Ly = kf.layers[l]
                for i in range(kf.F):
                    out += [(kf._cache(Ly.f[i].Ks), False), (kf._cache(Ly.f[i].Vs), False)]
                    if kf.exchange:
                        for j in range(kf.F):
                            if j != i:
                                out += [(kf._cache(Ly.p[i][j].Kc), False), (kf._cache(Ly.p[i][j].Vc), False)]
        else:
            kv = self.step_plan.kv
            for (K, Vt), _ in _kv_pairs(kv, kv):
                out += [(K, False), (Vt, True)]
        return out

    # ------------------------------------------------------------------ the decode
    def _cond_plan(self, n: int) -> Optional[kv_engine.CondPlan]:
        if not self._need_cond:
            return None
        if n == 1:
            return self._cond_step
        M = n * self.B
        cp = self._cond_adv.get(M)
        if cp is None:
            for old in self._cond_adv.values():      # one row count at a time: the modulation buffers are ~12 M x 2d elements
                self._hoist_tabs.pop(id(old), None)
                self._plan_audited.discard(id(old))
                if self._bound_cond is old:
                    self._bound_cond = None
            self._cond_adv.clear()
            cp = self._cond_adv[M] = kv_engine.CondPlan(self.eng, M)
        return cp

    def _run_cond(self, cp: kv_engine.CondPlan, first: int) -> None:
        """The condition-only work of the rows conds[first : first + M / B] (the same launches rollout_kv runs before its step loop)."""
        for t in cp.ibufs:
            t.zero_()
        cp.bind_ptrs(0, self.conds.data_ptr() + first * self.B * 4, 0)
        if not cp._audited or ptrcheck.always():
            cp.audit(owners=(self.conds,))
        cp.run()

    def _hoist_table(self, cp: kv_engine.CondPlan) -> list:
        """The step plan's hoisted pointers (Plan._find_hoisted, found over the single-step condition plan) re-based on the buffers of `cp`: the same
        offset inside row block 0 of the same module's buffer."""
        tab = self._hoist_tabs.get(id(cp))
        if tab is None:
            c1 = self._cond_step
            pairs = [(c1.mods[key], cp.mods[key]) for key in c1.mods] + list(zip(c1.ibufs, cp.ibufs))
            tab = []
            for st, field, base, step in self._hoist_tabs[id(c1)]:
                t1, t2 = next((a, b) for a, b in pairs if a.data_ptr() <= base < a.data_ptr() + step)
                assert t1.stride(0) == t2.stride(0) and t1.dtype == t2.dtype
                tab.append((st, field, t2.data_ptr() + (base - t1.data_ptr()), step))
            self._hoist_tabs[id(cp)] = tab
        return tab

    def _decode(self, first: int, n: int) -> None:
        """n steps from position `first`: reads traj[first] and conds[first : first + n], writes traj[first + 1 : first + n + 1] and cache rows
        first .. first + n - 1."""
        eng, B = self.eng, self.B
        eng.params.sync()
        cp = self._cond_plan(n)
        if cp is not None:
            self._run_cond(cp, first)
        if self.fast:
            self._decode_fast(cp, first, n)
            return
        p = self.step_plan
        base, cbase, slab = self.traj.data_ptr(), self.conds.data_ptr() + first * B * 4, self.slab
        if cp is not None and cp is not self._bound_cond:
            p._hoisted = self._hoist_table(cp)
            self._bound_cond = cp
        key = id(cp) if cp is not None else 0
        if key not in self._plan_audited or ptrcheck.always():   # the plan is bound by raw address: audit it once against the buffers it will walk
            p.set_position(first)
            p.bind_ptrs(base + first * slab, cbase, base + (first + 1) * slab)
            p.set_hoisted_step(0)
            p.audit(owners=(self.traj, self.conds) + (tuple(t for t in cp._keep if isinstance(t, torch.Tensor)) if cp is not None else ()))
            self._plan_audited.add(key)
        if _switches.kv("loop", "native") == "python" or not p.run_steps(n, base + first * slab, slab, cbase, B * 4, base + (first + 1) * slab, slab, first):
            for s in range(n):
                p.set_position(first + s)
                p.bind_ptrs(base + (first + s) * slab, cbase + s * B * 4, base + (first + s + 1) * slab)
                p.set_hoisted_step(s)
                p.run()

    def _decode_fast(self, cp, first: int, n: int) -> None:
        kf, B = self.kv_fast, self.B
        if cp is not self._bound_cond:
            for nm, pre in kf._norms:
                mod = cp.mods.get(pre) if (cp is not None and kf.adaln) else None
                nm.mod, nm.ldmod = (mod.data_ptr(), mod.stride(0)) if mod is not None else (None, 0)
            for l in range(kf.L):
                kf.layers[l].ib = cp.ibufs[l].data_ptr() if (cp is not None and kf.has_ib) else None
            self._bound_cond = cp
        small = B * kf.F * max(kf.D, 1)      # hand-off words of the seven-launch form; more: the persistent form's arena
        for attempt in (0, 1):
            N.check(N.lib().sea_kv_rollout(C.byref(kf.G), kf.layers, first, n, kf._tag, N.dtype_code(self.eng.act_dtype), N.stream_ptr()), "sea_kv_rollout")
            kf._tag = (kf._tag + n * kf.L) & 0xFFFFFFFF or 1
            if attempt == 0 and _switches.kv("force_err") == "1" and kf.G.handoff_words > small:
                kf.err.fill_(1)              # test hook, as KvFast.rollout's: behave as if a hand-off wait of the persistent launch had given up
            if int(kf.err.item()) == 0:      # (synchronises)
                return
            # A hand-off wait of the persistent launch gave up (KvFast.rollout explains why that can happen): fall back once, for good, to the seven
            # launches per step and recompute this call's steps from its first position — traj[first] and the cache rows < first are untouched.
            kf.err.zero_()
            if attempt == 0 and kf.G.handoff_words > small:
                kf.G.handoff_words = small
                continue
            raise RuntimeError("sea_kv_rollout: a hand-off wait inside the exchange tails gave up (results invalid)")

    # ------------------------------------------------------------------ the interface
    def _live(self) -> None:
        if self._closed:
            raise ValueError("rollout session: used after close()")

    def _room(self, n: int) -> None:
        if self.position + n > self.max_len:
            raise ValueError(f"rollout session: {n} step(s) from position {self.position} would feed position {self.position + n - 1} >= max_len {self.max_len}")

    @torch.no_grad()
    def step(self, c: torch.Tensor, state: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Feed position `position` — its condition c [B, 1] or [B], and, with `state` [B, F, E], a replacement of its stored state — and return the
        prediction of the next position [B, F, E] (fp32, a tensor of its own), which becomes the newest known state."""
        self._live()
        B = self.B
        if not torch.is_tensor(c) or tuple(c.shape) not in ((B, 1), (B,)):
            raise ValueError(f"rollout session: step condition {tuple(c.shape) if torch.is_tensor(c) else type(c).__name__} must be [B={B}, 1] or [B={B}]")
        if state is not None and tuple(state.shape) != (B, self.F, self.E):
            raise ValueError(f"rollout session: state {tuple(state.shape)} must be [B={B}, F={self.F}, E={self.E}]")
        self._room(1)
        p = self.position
        if state is not None:
            self.traj[p].copy_(state)       # the caches hold positions < p only: nothing else depends on the state at p
        self.conds[p].copy_(c.reshape(B))
        self._decode(p, 1)
        self.position = p + 1
        return self.traj[p + 1].clone()

    @torch.no_grad()
    def advance(self, conds: torch.Tensor) -> torch.Tensor:
        """n steps in the native step loop: conds [B, n, 1] are the conditions of positions position .. position + n - 1; returns the predictions of
        positions position + 1 .. position + n [B, n, F, E] (fp32, a tensor of its own)."""
        self._live()
        B = self.B
        if not torch.is_tensor(conds) or conds.dim() != 3 or conds.shape[0] != B or conds.shape[2] != 1:
            raise ValueError(f"rollout session: advance conditions {tuple(conds.shape) if torch.is_tensor(conds) else type(conds).__name__} must be [B={B}, n, 1]")
        n = conds.shape[1]
        self._room(n)
        p = self.position
        if n == 0:
            return torch.empty(B, 0, self.F, self.E, device=self.eng.device, dtype=torch.float32)
        self.conds[p:p + n].copy_(conds[:, :, 0].t())
        self._decode(p, n)
        self.position = p + n
        return _own(self.traj[p + 1:p + n + 1].permute(1, 0, 2, 3))

    @torch.no_grad()
    def states(self) -> torch.Tensor:
        """The trajectory so far, history included: [B, position + 1, F, E] fp32 (a copy)."""
        self._live()
        return _own(self.traj[:self.position + 1].permute(1, 0, 2, 3))

    @torch.no_grad()
    def conditions(self) -> torch.Tensor:
        """The conditions of positions 0 .. position - 1 as given: [B, position, 1] fp32 (a copy)."""
        self._live()
        return _own(self.conds[:self.position].t().unsqueeze(-1))

    def rewind(self, p: int) -> None:
        """Position p (0 <= p <= position) becomes the newest known state; later states are forgotten.  No launch: cache rows >= p are overwritten by
        the steps that follow."""
        self._live()
        if not 0 <= p <= self.position:
            raise ValueError(f"rollout session: rewind({p}) is outside 0 .. position = {self.position}")
        self.position = int(p)

    @torch.no_grad()
    def fork(self, n: int) -> "RolloutSession":
        """A new, independent session of B * n trajectories at the same position: row b * n + j is branch j of trajectory b.  The cache positions below
        `position` are copied by sea_kv_cache_fork (`forked_by == 'copy'`); where the wider batch decodes from another cache layout (sea_kv_rollout's
        value rows against the generic step plan's V^T, e.g. B * n > 64) the new session prefills from the stored states instead ('prefill')."""
        self._live()
        if not isinstance(n, int) or n < 1:
            raise ValueError(f"rollout session: fork({n}) needs n >= 1 branches")
        pos = self.position
        if kv_engine.supported(self.eng, self.B * n) != self.fast:
            return RolloutSession(self.eng, self.states().repeat_interleave(n, dim=0), self.conditions().repeat_interleave(n, dim=0), forked_by="prefill")
        t = RolloutSession.__new__(RolloutSession)
        t.eng, t.B, t.F, t.E, t.max_len = self.eng, self.B * n, self.F, self.E, self.max_len
        t.forked_by, t._closed = "copy", False
        t._alloc()
        assert t.fast == self.fast
        t.traj[:pos + 1].copy_(self.traj[:pos + 1].repeat_interleave(n, dim=1))
        if pos > 0:
            t.conds[:pos].copy_(self.conds[:pos].repeat_interleave(n, dim=1))
            entries = [dict(src=a, dst=b, n_pos=pos, transposed=tr) for (a, tr), (b, _) in zip(self._caches(), t._caches())]
            CacheFork(entries, self.eng.act_dtype, f"B={self.B} x {n} at position {pos}").run()
        t.position = pos
        return t

    def _gathered(self, idx: List[int]) -> "RolloutSession":
        """A new session whose trajectory j is trajectory idx[j] of this one (idx already checked): states and conditions through index_select, the
        cache positions below `position` through ONE sea_kv_cache_gather launch per 32 cache tensors, which also converts value rows <-> V^T where
        the new batch decodes from the other layout."""
        pos = self.position
        t = RolloutSession.__new__(RolloutSession)
        t.eng, t.B, t.F, t.E, t.max_len = self.eng, len(idx), self.F, self.E, self.max_len
        t.forked_by, t._closed = "gather", False
        t._alloc()
        index = torch.tensor(idx, dtype=torch.int32, device=self.eng.device)
        t.traj[:pos + 1].copy_(self.traj[:pos + 1].index_select(1, index))
        if pos > 0:
            t.conds[:pos].copy_(self.conds[:pos].index_select(1, index))
            mine, theirs = self._caches(), t._caches()
            assert len(mine) == len(theirs)
            entries = [dict(src=a, dst=b, n_pos=pos, src_transposed=ta, dst_transposed=tb) for (a, ta), (b, tb) in zip(mine, theirs)]
            CacheGather(entries, index, self.eng.act_dtype, f"B={self.B} -> {t.B} at position {pos}").run()
        t.position = pos
        return t

    @torch.no_grad()
    def select(self, index) -> "RolloutSession":
        """A new, independent session of len(index) trajectories at the same position: trajectory j has the states, conditions and cache positions
        below `position` of trajectory index[j] of this session, which is left untouched.  index: a 1-D list, tuple or integer tensor with values in
        [0, B), duplicates allowed (a device tensor is brought to the host once for validation: select then synchronises).  The caches are copied by
        sea_kv_cache_gather (`forked_by == 'gather'`), never prefilled: where the new batch decodes from the other cache layout (kv_engine.supported
        of len(index) against this session's form) the same launch converts the value caches.  At position 0 nothing is launched."""
        self._live()
        return self._gathered(check_select(self.B, index))

    @torch.no_grad()
    def resample(self, index) -> None:
        """select(index) in place, len(index) == B: trajectory j becomes a copy of what trajectory index[j] was.  The selection is built in fresh
        buffers (copying in place would read rows it has already overwritten), the device is synchronised as in close(), then this session adopts
        them and releases its old ones.  Position, B and the decode form are unchanged; an identity index copies."""
        self._live()
        idx = check_select(self.B, index)
        if len(idx) != self.B:
            raise ValueError(f"rollout session: resample needs one index per trajectory (B = {self.B}), got {len(idx)}")
        t = self._gathered(idx)
        assert t.fast == self.fast and t.B == self.B
        torch.cuda.synchronize(self.eng.device)   # the gather, and launches still in flight, read the old buffers by raw address
        forked_by = self.forked_by
        self.__dict__.update(t.__dict__)
        self.forked_by = forked_by
        t._closed = True

    def close(self) -> None:
        """Release the session's buffers (caches, workspace, trajectory).  Every later use raises ValueError."""
        if self._closed:
            return
        torch.cuda.synchronize(self.eng.device)   # launches still in flight read these buffers by raw address
        self._closed = True
        self.traj = self.conds = self.kv_fast = self.step_plan = self._cond_step = self._bound_cond = None
        self._cond_adv, self._hoist_tabs = {}, {}

    def __enter__(self) -> "RolloutSession":
        self._live()
        return self

    def __exit__(self, *exc) -> None:
        self.close()
