"""AdamW over the model's flat parameter buffer: one kernel launch per step (sea_adamw_flat), which also refreshes the
activation-dtype weight shadow.  Semantics follow torch.optim.AdamW as the reference configures it
(utils/train_utils.py:33-34): decoupled weight decay, bias-corrected moments; parameters that never receive a gradient are not
touched and get no state (they sit beyond the live prefix of the flat buffer).

Data parallel (one process per GPU, torch.distributed initialised): `step()` SUM-all-reduces the live prefix of the flat gradient buffer
itself when nothing has reduced it since the last `zero_grad()` — so the reference's loop `loss.backward(); optimizer.step()`
(train/train_temporal.py:256-257) is correct on N ranks as written — and folds the 1/world mean into the kernel's grad_scale.  The fused step
(engine.train_step) reduces in slices under the backward and tells the optimizer so (`mark_reduced`).

Clipping and skipping (`max_grad_norm`, `skip_nonfinite`): with either set, `step()` issues sea_grad_norm_ctl + sea_adamw_flat_ctl instead of
sea_adamw_flat — the global 2-norm of the mean gradient (after the reduce, so identical on every rank), torch.nn.utils.clip_grad_norm_'s factor
and the decision to drop a step whose norm is not finite are all taken on the device and handed to the AdamW launch through an 8-word control
block: no host sync, no further collective.  The clip lives in the AdamW launch: the `.grad` views read after `step()` hold the UNCLIPPED gradients.
`step_control` restates the rule in plain Python."""
from __future__ import annotations

import math
import numbers
from typing import Optional

import torch

from . import _native as N


def _f32(x: float) -> float:
    return float(torch.tensor(x, dtype=torch.float64).float())


def step_control(norm: float, max_norm: float, skip_nonfinite: bool, step: int = 0, skipped: int = 0, clipped: int = 0) -> dict:
    """What the finish of sea_grad_norm_ctl decides (include/sea_hip.h), in plain Python.  `norm`: the 2-norm of the scaled gradients as a
    Python float (fp64); `max_norm` <= 0: no clipping; step / skipped / clipped: the counters before this step.  Returns the control words after
    it: {"grad_norm", "clip", "applied", "step", "skipped", "clipped"} — grad_norm and clip rounded to fp32 as the device stores them."""
    norm32 = _f32(norm)
    finite = math.isfinite(norm32)
    if not finite and skip_nonfinite:
        return dict(grad_norm=norm32, clip=0.0, applied=0, step=step, skipped=skipped + 1, clipped=clipped)
    clip = _f32(min(1.0, max_norm / (norm + 1e-6))) if (max_norm > 0 and finite) else 1.0
    return dict(grad_norm=norm32, clip=clip, applied=1, step=step + 1, skipped=skipped, clipped=clipped + (1 if clip < 1.0 else 0))


class FlatAdamW(torch.optim.Optimizer):
    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, skip_nonfinite=False):
        if max_grad_norm is not None:
            if not isinstance(max_grad_norm, numbers.Real) or isinstance(max_grad_norm, bool) or not (math.isfinite(max_grad_norm) and max_grad_norm > 0):
                raise ValueError(f"FlatAdamW: max_grad_norm = {max_grad_norm!r} must be a positive finite number (None: no clipping)")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._ctl: Optional[torch.Tensor] = None       # the step control block (8 x int32, include/sea_hip.h SEA_CTL_*), when `controlled`
        self._norm_ws: Optional[torch.Tensor] = None   # partial sums of the norm pass (1024 x float64)
        params = list(model.parameters())
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.model = model
        self._m: Optional[torch.Tensor] = None
        self._v: Optional[torch.Tensor] = None
        self._step = 0
        self._eng = None
        self.grad_scale = 1.0   # data parallel: 1 / world_size after the SUM all-reduce
        self._reduced = False   # True once this step's gradients have been all-reduced (by engine.train_step or by step() itself)
        self.allreduce_calls = 0   # collectives issued by step() over the optimizer's lifetime (the bench line reports it)
        self.process_group = None

    def _buffers(self):
        eng = self.model.engine()
        if self._eng is not eng:  # first use, or the model moved / changed dtype: (re)allocate the moments
            n = eng.params.n_live
            self._m = torch.zeros(n, device=eng.device, dtype=torch.float32)
            self._v = torch.zeros(n, device=eng.device, dtype=torch.float32)
            self._eng = eng
            eng.ensure_grads()
            if self.controlled:
                self._new_ctl(self._ctl)
                self._norm_ws = torch.empty(1024, device=eng.device, dtype=torch.float64)
        return eng

    # ------------------------------------------------------------------ clipping / skipping: the device-side step control
    @property
    def controlled(self) -> bool:
        """True when step() runs the sea_grad_norm_ctl + sea_adamw_flat_ctl pair (clipping or skipping asked for)."""
        return self.max_grad_norm is not None or self.skip_nonfinite

    def _new_ctl(self, words: Optional[torch.Tensor]) -> None:
        """The control block on the engine's device: `words` (a saved or an earlier block) or zeros with the applied-step count taken from _step."""
        if words is None:
            words = torch.zeros(N.CTL_WORDS, dtype=torch.int32)
            words[N.CTL_STEP] = self._step
        self._ctl = words.detach().to(device=self._eng.device, dtype=torch.int32, copy=True)

    @property
    def last_grad_norm(self) -> Optional[torch.Tensor]:
        """2-norm of the last step's mean gradient (before clipping; of a skipped step too) as a 0-d fp32 DEVICE view of the control block: no sync.
        None without clipping / skipping."""
        if not self.controlled:
            return None
        self._buffers()
        return self._ctl[N.CTL_GRAD_NORM:N.CTL_GRAD_NORM + 1].view(torch.float32)[0]

    @property
    def last_applied(self) -> Optional[torch.Tensor]:
        """0-d int32 device view: 1 if the last step updated the parameters, 0 if it was skipped.  None without clipping / skipping."""
        if not self.controlled:
            return None
        self._buffers()
        return self._ctl[N.CTL_APPLIED]

    def step_control_words(self) -> torch.Tensor:
        """The control block itself (8 x int32 on the device, _native.CTL_*), for a caller that folds it into a copy of its own."""
        if not self.controlled:
            raise RuntimeError("FlatAdamW.step_control_words(): the optimizer was built without max_grad_norm / skip_nonfinite")
        self._buffers()
        return self._ctl

    def step_stats(self) -> dict:
        """The control block on the host (ONE small device-to-host copy, which waits for the stream)."""
        if not self.controlled:
            raise RuntimeError("FlatAdamW.step_stats(): the optimizer was built without max_grad_norm / skip_nonfinite")
        self._buffers()
        w = self._ctl.cpu()
        f = w.view(torch.float32)
        return {"grad_norm": float(f[N.CTL_GRAD_NORM]), "clip": float(f[N.CTL_CLIP]), "applied": int(w[N.CTL_APPLIED]),
                "applied_steps": int(w[N.CTL_STEP]), "skipped_steps": int(w[N.CTL_SKIPPED]), "clipped_steps": int(w[N.CTL_CLIPPED])}

    def zero_grad(self, set_to_none: bool = True):
        eng = self._buffers()
        eng.zero_grads()
        self._reduced = False
        if set_to_none:
            for p in self.model._live_params():
                p.grad = None

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        eng = self._buffers()
        if not eng.grads_dirty:
            return loss  # no backward since the last zero_grad: like torch, parameters without gradients are skipped
        if not self._reduced:
            # data parallel: ONE all-reduce of the live prefix (a no-op returning 1.0 without a process group or at world size 1)
            from .parallel import allreduce_flat_gradients, world_size

            if world_size(self.process_group) > 1:
                self.grad_scale = allreduce_flat_gradients(eng.grads, eng.params.n_live, self.process_group)
                self.allreduce_calls += 1
            else:
                self.grad_scale = 1.0
            self._reduced = True
        g = self.param_groups[0]
        P = eng.params
        n = P.n_live
        shadow = P.flat_act if P.act_dtype != torch.float32 else None
        if self.controlled:
            # the norm of the summed-and-scaled gradients decides clip and skip ON THE DEVICE (the same on every rank); the host does not learn
            # whether the step was applied: the applied-step count lives in the control block (state_dict() reads it)
            L = N.lib()
            N.check(L.sea_grad_norm_ctl(eng.grads.data_ptr(), n, float(self.grad_scale), float(self.max_grad_norm or 0.0), int(self.skip_nonfinite),
                                        float(g["betas"][0]), float(g["betas"][1]), self._norm_ws.data_ptr(), self._norm_ws.numel(),
                                        self._ctl.data_ptr(), N.stream_ptr()), "sea_grad_norm_ctl")
            N.check(L.sea_adamw_flat_ctl(P.flat32.data_ptr(), eng.grads.data_ptr(), self._m.data_ptr(), self._v.data_ptr(),
                                         None if shadow is None else shadow.data_ptr(), N.dtype_code(P.act_dtype), n, float(g["lr"]),
                                         float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                                         float(self.grad_scale), self._ctl.data_ptr(), N.stream_ptr()), "sea_adamw_flat_ctl")
            P._synced_version = P.flat32._version   # as below (a skipped step wrote nothing: the refresh is then redundant, not wrong)
            if shadow is not None:
                P.weights_changed()                 # (the kernel wrote the shadow through raw pointers: the condition memo's weight epoch moves on)
            P.sync_transposed(force=True)
            return loss
        self._step += 1
        N.check(N.lib().sea_adamw_flat(P.flat32.data_ptr(), eng.grads.data_ptr(), self._m.data_ptr(), self._v.data_ptr(),
                                       None if shadow is None else shadow.data_ptr(), N.dtype_code(P.act_dtype), n, float(g["lr"]),
                                       float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]), self._step,
                                       float(self.grad_scale), N.stream_ptr()), "sea_adamw_flat")
        # the kernel wrote through raw pointers: mark both shadows as current for the row-major one, stale for the transposed one
        P._synced_version = P.flat32._version
        if shadow is not None:
            P.weights_changed()
        P.sync_transposed(force=True)
        return loss

    def mark_reduced(self, grad_scale: float) -> None:
        """engine.train_step: the gradients of this step are already summed over the ranks; `grad_scale` turns the sum into the mean."""
        self.grad_scale, self._reduced = grad_scale, True

    def state_dict(self):
        sd = super().state_dict()
        ctl = None
        if self.controlled and self._ctl is not None:
            ctl = self._ctl.cpu()
            self._step = int(ctl[N.CTL_STEP])   # the APPLIED steps: a resume without clipping continues the bias correction from here
        sd["sea_flat"] = dict(step=self._step, m=None if self._m is None else self._m.cpu(), v=None if self._v is None else self._v.cpu())
        if ctl is not None:
            sd["sea_flat"]["ctl"] = ctl
        return sd

    def load_state_dict(self, state_dict):
        flat = state_dict.get("sea_flat")
        super().load_state_dict({k: v for k, v in state_dict.items() if k != "sea_flat"})
        if flat is not None and flat["m"] is not None:
            self._buffers()
            self._step = flat["step"]
            self._m.copy_(flat["m"])
            self._v.copy_(flat["v"])
            if self.controlled:   # a state saved without the options has no block: the applied-step count starts from its step
                self._new_ctl(flat.get("ctl"))
