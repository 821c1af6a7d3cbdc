"""Weighting and resampling an ensemble of rollout trajectories on the device: the two steps between what RolloutSession.step returns and what
RolloutSession.resample takes.

    ens = open_rollout(model, x0, ib).fork(n)                     # n members per history
    like = FieldLikelihood(decoder, n_patches, members=n, counts=counts, sigma=sigma)
    y = ens.step(perturbed_conditions())                          # [B * n, n_groups, P * D]
    logw = like(y, obs)                                           # [B * n] log-weights: one fused launch over the decoder's second layer
    index, logw, ess, resampled = systematic_resample(logw, n, ess_threshold=0.5, prior=logw_prev)
    ens.resample(index)                                           # the int32 device index goes in as it is
    mean, var = EnsembleFields(decoder, n_patches, members=n, counts=counts)(y, logw=logw)   # the forecast: posterior mean and spread of the decoded fields

FieldLikelihood is Decode.member_sse behind the latent -> z re-layout of FieldSpaceLoss: from 8192 rows (members x patches) on, or with
fused=True, one fused launch over the decoder's second layer (sea_decode_member_sse: the decoded fields are never written); below that, by
measurement, the decoder's forward plus reductions (Decode.member_sse states the rule); systematic_resample is sea_resample_systematic: normalisation, cumulative sum, effective sample size, the decision whether to
resample and the searches in one launch.  Neither function reads anything back from the device (no .item(), no .cpu()): the decision lives in the
index itself (the identity where a history was not resampled) and in the returned `resampled` tensor.  EnsembleFields is the product of the
ensemble: the weighted mean and the centred variance of the members' decoded fields (Decode.member_moments; fused: sea_decode_member_moments, the
members' fields are never written), from the log-weights as they are — normalised with tensor ops, nothing read back.

A GAPPY snapshot — a frame with masked regions, a field known on some cells only — comes with a precision map in obs's shape (0: missing cell,
neutral by a select whatever obs holds there), and the same object also moves states towards it (Decode.field_loss: sea_decode_field_grad, one
fused launch for the score and its gradient; members = 1 pulls single trajectories, which neither FieldKalman nor the encoder can):

    logw = like(y, obs, precision)                                # [B * n]: -0.5 * sum_f wsse_f, sigma as a per-field precision
    logw, dlogw_dy = like.score_and_grad(y, obs, precision)       # ... and the gradient of every member's own log-weight, in y's layout
    y = ens.step(c_next, state=like.nudge(y, obs, precision, rate=0.25))   # one gradient step towards the frame as the corrected state

Sparse observations — K point sensors, each reading one field at one cell of one patch, with a precision per reading (0: missing) — take the place of
the dense snapshot through SensorSet and SensorLikelihood:

    sensors = unpatcher.sensor_set(decoder, points, fields)       # or SensorSet(decoder, n_patches, patch, cell, field): tables built and uploaded once
    like = SensorLikelihood(decoder, n_patches, members=n, sensors=sensors, sigma=sensors.scale_sigma(sigma_phys))
    logw = like(y, sensors.scale_values(readings), precision)     # [B * n]: Decode.sensor_sse — the first layer over the observed patches only, then ONE
                                                                  # launch (sea_decode_sensor_sse) over the sensors' rows of the second layer
    logw, dlogw_dy = like.score_and_grad(y, obs, precision)       # the same log-weights and the gradient of every member's own log-weight, in y's layout:
                                                                  # Decode.sensor_loss's launches (sea_decode_sensor_grad), no autograd graph
    y = ens.step(c_next, state=like.nudge(y, obs, precision, rate=0.25))   # one gradient step towards the readings as the corrected state

The ensemble Kalman analysis moves all members at once (SensorKalman: sea_enkf_transform + sea_ensemble_mix behind sensor_sse's predictions):

    kalman = SensorKalman(decoder, n_patches, members=n, sensors=sensors, sigma=sensors.scale_sigma(sigma_phys), inflation=1.05,
                          taper=unpatcher.sensor_taper(sensors, radius))      # taper=None: one analysis domain for all patches
    y = ens.step(c_next, state=kalman.analyse(y, sensors.scale_values(readings), precision))

A dense snapshot takes the same analysis through FieldKalman (sea_decode_member_gram + sea_enkf_transform_gram + sea_ensemble_mix: the members' decoded
fields are reduced to one N x N Gram matrix per (history, patch) while they are decoded; a [P, P] taper between patch centroids localises):

    kalman = FieldKalman(decoder, n_patches, members=n, counts=counts, sigma=sigma_cell, inflation=1.05, taper=unpatcher.patch_taper(radius))
    y = ens.step(c_next, state=kalman.analyse(y, obs, precision))             # obs [B, P, n_fields, C]; precision: a map of obs's shape, 0 = missing

Whether the ensemble is any good is read at the same sensors (SensorVerification: sea_ensemble_verify behind the same predictions):

    verify = SensorVerification(decoder, n_patches, members=n, sensors=sensors, sigma=sensors.scale_sigma(sigma_phys))
    D, status, pred = kalman.transform(y, obs, precision)
    forecast = verify.from_predictions(pred, obs, precision, into=forecast)   # CRPS, PIT, rank, mean, spread per sensor; sums and rank histogram add up
    forecast.spread_skill, forecast.suggested_inflation, forecast.hist         # [B] tensors and the histogram, on the device

... or on the whole mesh against a dense snapshot (FieldVerification: sea_decode_member_verify, the members' fields never written):

    verify = FieldVerification(decoder, n_patches, members=n, counts=counts, sigma=sigma_cell)
    scores = verify(y, snapshot, precision, into=scores)                       # crps, pit, rank, mean, spread maps [B, P, n_fields, n_inp]
    scores.spread_skill, scores.pooled().suggested_inflation                    # [B, n_fields] per field; pooled(): [B] over the mesh

What is published as the forecast besides mean and variance (EnsembleQuantiles: sea_decode_member_quantiles, one launch, the members' fields never written):

    products = EnsembleQuantiles(decoder, n_patches, members=n, levels=(0.05, 0.5, 0.95), thresholds=unpatcher.scale_thresholds([[0.5, 2.0]]), counts=counts)
    quant, exceed = products(y, logw)                                           # [3, B, P, n_fields, n_inp] quantile maps, [1, B, P, n_fields, n_inp] P(field > threshold)

Whether those exceedance probabilities are any good (FieldThresholdVerification: sea_decode_member_brier, two launches, the members' fields never
written; SensorThresholdVerification: sea_ensemble_brier on predictions that exist already):

    check = FieldThresholdVerification(decoder, n_patches, members=n, thresholds=unpatcher.scale_thresholds([[0.5, 2.0]]), counts=counts)
    scores = check(y, snapshot, precision, into=scores)                         # Brier sums, reliability histograms and ROC hit counts add up over the cycles
    scores.brier, scores.brier_skill, scores.reliability, scores.roc_area       # [B, n_fields, T] tensors on the device; scores.reliability_curve(), scores.roc()

The same CRPS TRAINS the temporal model as an ensemble generator (EnsembleCRPSLoss: Decode.member_crps_loss, sea_decode_member_crps_grad — the
CRPS sums of FieldVerification with their gradient to the latent states, the members' fields and their gradient never written):

    loss = EnsembleCRPSLoss(decoder, n_patches, members=n, counts=counts)(model(x_members, perturbed_conditions), truth_fields)
    loss.backward()                                                             # to the parameters, and to x.grad / cond.grad of TemporalModel
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional

import torch

from . import _native as N
from . import ops

try:   # numpy integers are accepted in sensor index sequences where numpy is installed
    import numpy as _np
except ImportError:   # pragma: no cover
    _np = None


class FieldLikelihood:
    """Gaussian log-likelihood of an observation of the decoded fields, per ensemble member: like(y, obs) -> log-weights [B * members] (f32, device).

    y: what RolloutSession.step returns for a session of B * members trajectories, [B * members, n_groups, P * D] (member j of history b at row
    b * members + j, the order of fork()); obs: float32 [B, P, n_fields, C >= n_inp] (what patchify_and_scale(..., layout="BPFC") writes for one
    snapshot) or, with layout="BPCF", the reference's [B, P, C, n_fields].  logw = -0.5 * sum_f sse_f / sigma_f^2 with sse_f the member's squared
    error of field f over its patches and valid cells (Decode.member_sse); sigma: None (1), a positive number, or n_fields positive numbers (a
    sequence or tensor) — applied with tensor ops on the [B * members, n_fields] result.  counts: valid cells per patch (None: all), as in
    Decode.mse_loss.  fused: None (Decode.member_sse's measured rule), True (the fused launch at any size; bf16 only) or False (the composed path).
    `decoder` is a sea_amd Decode; no autograd graph is built.
    like(y, obs, precision) takes a precision map for a gappy snapshot — float32 in obs's shape and layout on y's device, >= 0, 0 marking a missing
    cell — and scores through Decode.field_loss (its measured fused=None rule): logw = -0.5 * sum_f wsse_f with sigma as field_precision = 1 / sigma_f^2.
    score_and_grad(y, obs, precision) adds the gradient of every member's own log-weight with respect to its state, and nudge(y, obs, precision,
    rate) takes one gradient step along it; members = 1 is legal (single trajectories pulled towards a gappy frame)."""

    def __init__(self, decoder, n_patches: int, members: int, counts=None, layout: str = "BPFC", sigma=None, fused: Optional[bool] = None):
        if layout not in ("BPFC", "BPCF"):
            raise ValueError(f"FieldLikelihood: layout must be 'BPFC' or 'BPCF', got {layout!r}")
        if not isinstance(n_patches, int) or isinstance(n_patches, bool) or n_patches < 1:
            raise ValueError(f"FieldLikelihood: n_patches = {n_patches!r} must be a positive integer")
        if not isinstance(members, int) or isinstance(members, bool) or members < 1:
            raise ValueError(f"FieldLikelihood: members = {members!r} must be a positive integer")
        self.decoder, self.n_patches, self.members, self.counts, self.layout, self.fused = decoder, n_patches, members, counts, layout, fused
        n_fields = sum(len(g) for g in decoder.field_groups)
        if sigma is None:
            self._scale_host = None
        else:
            s = torch.as_tensor(sigma, dtype=torch.float64).detach().cpu()   # a tensor given on the device comes to the host once, here
            if s.dim() > 1 or (s.dim() == 1 and s.numel() != n_fields):
                raise ValueError(f"FieldLikelihood: sigma must be None, a number or {n_fields} numbers (one per field), got shape {tuple(s.shape)}")
            if not bool(torch.isfinite(s).all()) or not bool((s > 0).all()):
                raise ValueError(f"FieldLikelihood: sigma must be finite and positive, got {s.tolist()}")
            self._scale_host = [float(v) for v in (-0.5 / (s * s)).expand(n_fields)]
        self._scale = None

    def _field_scale(self, device):
        """-0.5 / sigma_f^2 as an f32 [n_fields] tensor on the device, built once per device by fills (an upload from the host would synchronise)."""
        if self._scale is None or self._scale.device != device:
            n_fields = sum(len(g) for g in self.decoder.field_groups)
            scale = torch.full((n_fields,), -0.5, device=device, dtype=torch.float32)
            if self._scale_host is not None:
                for f, v in enumerate(self._scale_host):
                    scale[f].fill_(v)
            self._scale = scale
        return self._scale

    def _field_prec(self, device):
        """1 / sigma_f^2 as an f32 [n_fields] tensor on the device (None without sigma): the field_precision of Decode.field_loss, from the same numbers
        as _field_scale, built once per device with tensor ops."""
        if self._scale_host is None:
            return None
        cur = getattr(self, "_fprec", None)
        if cur is None or cur.device != device:
            cur = self._fprec = (self._field_scale(device) * -2.0).contiguous()
        return cur

    def _operands(self, y, obs, precision, layout):
        """Checked (Bm, G, E, z view, obs and precision in "BPFC" order)."""
        if isinstance(precision, str) and layout is None:   # the call's third positional argument used to be the layout
            precision, layout = None, precision
        layout = self.layout if layout is None else layout
        if layout not in ("BPFC", "BPCF"):
            raise ValueError(f"FieldLikelihood: layout must be 'BPFC' or 'BPCF', got {layout!r}")
        P = self.n_patches
        if not torch.is_tensor(y) or y.dim() != 3 or y.shape[-1] % P or y.shape[0] < 1:
            raise ValueError(f"FieldLikelihood: y must be [B * members, n_groups, n_patches * D] with n_patches = {P}, got "
                             f"{tuple(y.shape) if torch.is_tensor(y) else type(y).__name__}")
        Bm, G, E = y.shape
        if Bm % self.members:
            raise ValueError(f"FieldLikelihood: the {Bm} trajectories of y are not a multiple of members = {self.members}")
        B = Bm // self.members
        if not torch.is_tensor(obs) or obs.dim() != 4 or tuple(obs.shape[:2]) != (B, P):
            raise ValueError(f"FieldLikelihood: the observation must be [{B}, {P}, ...] in layout {layout} (one per history), got "
                             f"{tuple(obs.shape) if torch.is_tensor(obs) else type(obs).__name__}")
        if precision is not None:
            if not torch.is_tensor(precision) or tuple(precision.shape) != tuple(obs.shape):
                raise ValueError(f"FieldLikelihood: precision must be None or a map of obs's shape {tuple(obs.shape)}, got "
                                 f"{tuple(precision.shape) if torch.is_tensor(precision) else type(precision).__name__}")
            if precision.dtype != torch.float32:
                raise ValueError(f"FieldLikelihood: precision must be float32, got {precision.dtype}")
            if precision.device.type == "cpu" and (not bool(torch.isfinite(precision).all()) or not bool((precision >= 0).all())):
                raise ValueError("FieldLikelihood: precision must be finite and >= 0")
            if precision.device != y.device:
                raise ValueError(f"FieldLikelihood: precision is on {precision.device}, the states on {y.device}")
        perm = (lambda t: t) if layout == "BPFC" else (lambda t: t.permute(0, 1, 3, 2))
        z = y.reshape(Bm, G, P, E // P).permute(0, 2, 1, 3)          # the re-layout of inverse_transform_processed_data, one snapshot per member
        return Bm, G, E, z, perm(obs), None if precision is None else perm(precision)

    def __call__(self, y: torch.Tensor, obs: torch.Tensor, precision: Optional[torch.Tensor] = None, layout: Optional[str] = None) -> torch.Tensor:
        """Log-weights [B * members].  precision: None — the squared error over the valid cells (Decode.member_sse) — or a float32 map of obs's shape
        on y's device, >= 0, 0 marking a missing cell (neutral by a select, NaN in obs there included): logw = -0.5 * sum_f wsse_f with sigma entering
        as field_precision = 1 / sigma_f^2 (Decode.field_loss, score-only)."""
        Bm, G, E, z, tgt, prec = self._operands(y, obs, precision, layout)
        if prec is None:
            sse = self.decoder.member_sse(z, tgt, counts=self.counts, members=self.members, fused=self.fused)
            return (sse * self._field_scale(sse.device)).sum(1)
        with torch.no_grad():
            wsse = self.decoder.field_loss(z.detach(), tgt.detach(), members=self.members, counts=self.counts, precision=prec.detach(),
                                           field_precision=self._field_prec(y.device), fused=self.fused)
            return -0.5 * wsse.sum(1)

    def score_and_grad(self, y: torch.Tensor, obs: torch.Tensor, precision: Optional[torch.Tensor] = None, layout: Optional[str] = None):
        """(logw [Bm], dlogw_dy [Bm, n_groups, P * D] fp32): the log-weights logw = -0.5 * sum_f wsse_f (sigma as field_precision = 1 / sigma_f^2; with
        a precision map the bits of __call__ on the same path) and the gradient of every member's OWN log-weight with respect to its state, in y's
        layout (the inverse of the re-layout __call__ applies) — Decode.field_loss's one pass.  precision as in __call__; None: every valid cell with
        weight 1.  members = 1 is the pull of single trajectories towards a gappy frame.  The graph is local to the call (y is detached); nothing is
        read back."""
        Bm, G, E, z, tgt, prec = self._operands(y, obs, precision, layout)
        dec = self.decoder
        pf = self._field_prec(y.device)
        tgt, prec = tgt.detach(), None if prec is None else prec.detach()
        with torch.enable_grad():
            zz = z.detach().to(torch.float32).contiguous().requires_grad_(True)
            wsse = dec.field_loss(zz, tgt, members=self.members, counts=self.counts, precision=prec, field_precision=pf, fused=self.fused)
            (dz,) = torch.autograd.grad(wsse.sum(), zz)
            wsse = wsse.detach()
        return -0.5 * wsse.sum(1), (-0.5 * dz.to(torch.float32)).permute(0, 2, 1, 3).reshape(Bm, G, E)

    def nudge(self, y: torch.Tensor, obs: torch.Tensor, precision: Optional[torch.Tensor] = None, rate=1.0, layout: Optional[str] = None) -> torch.Tensor:
        """y + rate * dlogw_dy, in y's dtype: one gradient step on every member's log-likelihood of the snapshot — a corrected state for
        RolloutSession.step(c, state=...).  rate: a number, or a float32 [Bm] tensor on y's device (one step length per member)."""
        if torch.is_tensor(rate):
            if not torch.is_tensor(y) or rate.dim() != 1 or rate.shape[0] != y.shape[0] or rate.dtype != torch.float32 or rate.device != y.device:
                raise ValueError(f"FieldLikelihood.nudge: a rate tensor must be float32 [{y.shape[0] if torch.is_tensor(y) else 'Bm'}] on the states' device, got "
                                 f"{tuple(rate.shape)} {rate.dtype} on {rate.device}")
            rate = rate.detach().view(-1, 1, 1)
        elif isinstance(rate, bool) or not isinstance(rate, (int, float)) or not math.isfinite(rate):
            raise ValueError(f"FieldLikelihood.nudge: rate must be a finite number or a float32 [Bm] tensor, got {rate!r}")
        _, grad = self.score_and_grad(y, obs, precision, layout=layout)
        return (y.detach().to(torch.float32) + rate * grad).to(y.dtype)


def normalised_weights(logw: torch.Tensor, members: int) -> torch.Tensor:
    """Log-weights [B * members] (unnormalised, or a `logw_out` of systematic_resample) -> float32 weights [B * members] that sum to 1 per history, with
    tensor ops only.  A NaN or infinite log-weight is a dead member: weight exactly 0; the maximum over the live members is subtracted first; a
    history without a live member gets equal weights (what `resampled == -1` means in the resampler: the ensemble is kept as it is)."""
    lw = logw.detach().reshape(-1, members).to(torch.float32)
    live = torch.isfinite(lw)
    mx = torch.where(live, lw, torch.full_like(lw, float("-inf"))).max(dim=1, keepdim=True).values
    w = torch.where(live, (torch.where(live, lw, mx) - mx).exp(), torch.zeros_like(lw))
    W = w.sum(dim=1, keepdim=True)
    return torch.where(W > 0, w / W.clamp_min(torch.finfo(torch.float32).tiny), torch.full_like(w, 1.0 / members)).reshape(-1).contiguous()


class EnsembleFields:
    """The forecast of an ensemble: fields(y, logw=None, unbiased=False) -> (mean, var), the weighted mean and the centred variance of the members'
    decoded fields, each fp32 [B, P, n_fields, n_inp] (layout "BPFC": views of n_inp_p-wide buffers that sea_unpatchify reads in place —
    MeshUnpatcher.inverse_scale_and_unpatch(mean, layout="BPFC") and unpatch_spread(var.sqrt())) or, with layout="BPCF", permuted views in the
    reference's [B, P, n_inp, n_fields].

    y: what RolloutSession.step returns for B * members trajectories, [B * members, n_groups, P * D], member j of history b at row b * members + j;
    logw: None (equal weights) or [B * members] log-weights on y's device, unnormalised or the `logw_out` of systematic_resample (normalised_weights
    states the rules: dead members get weight 0 and are passed over — NaN in their states reaches nothing; a history without a live member gets equal
    weights); nothing is read back.  unbiased: multiply var by 1 / (1 - sum_j w_j^2).  counts: valid cells per patch (None: all), as in
    Decode.mse_loss; invalid cells are exactly 0 in both results.  fused: None (Decode.member_moments' rule), True (the fused launch at any size;
    bf16 only) or False (the composed path).  `decoder` is a sea_amd Decode; no autograd graph is built."""

    def __init__(self, decoder, n_patches: int, members: int, counts=None, layout: str = "BPFC", fused: Optional[bool] = None):
        if layout not in ("BPFC", "BPCF"):
            raise ValueError(f"EnsembleFields: layout must be 'BPFC' or 'BPCF', got {layout!r}")
        if not isinstance(n_patches, int) or isinstance(n_patches, bool) or n_patches < 1:
            raise ValueError(f"EnsembleFields: n_patches = {n_patches!r} must be a positive integer")
        if not isinstance(members, int) or isinstance(members, bool) or members < 1:
            raise ValueError(f"EnsembleFields: members = {members!r} must be a positive integer")
        self.decoder, self.n_patches, self.members, self.counts, self.layout, self.fused = decoder, n_patches, members, counts, layout, fused

    def __call__(self, y: torch.Tensor, logw: Optional[torch.Tensor] = None, unbiased: bool = False, layout: Optional[str] = None):
        layout = self.layout if layout is None else layout
        if layout not in ("BPFC", "BPCF"):
            raise ValueError(f"EnsembleFields: layout must be 'BPFC' or 'BPCF', got {layout!r}")
        P = self.n_patches
        if y.dim() != 3 or y.shape[-1] % P or y.shape[0] < 1:
            raise ValueError(f"EnsembleFields: y must be [B * members, n_groups, n_patches * D] with n_patches = {P}, got {tuple(y.shape)}")
        Bm, G, E = y.shape
        if Bm % self.members:
            raise ValueError(f"EnsembleFields: the {Bm} trajectories of y are not a multiple of members = {self.members}")
        if logw is not None:
            if not torch.is_tensor(logw) or not logw.is_floating_point() or logw.numel() != Bm or logw.dim() not in (1, 2) \
                    or (logw.dim() == 2 and logw.shape[1] != self.members):
                raise ValueError(f"EnsembleFields: logw must be None or a floating-point [{Bm}] (or [{Bm // self.members}, {self.members}]) tensor of log-weights, got "
                                 f"{tuple(logw.shape) if torch.is_tensor(logw) else type(logw).__name__}")
            if logw.device != y.device:
                raise ValueError(f"EnsembleFields: logw is on {logw.device}, y on {y.device}")
        N.require_gpu(y, "EnsembleFields states")
        z = y.reshape(Bm, G, P, E // P).permute(0, 2, 1, 3)          # the re-layout of FieldLikelihood
        with torch.no_grad():
            w = None if logw is None else normalised_weights(logw, self.members)
            mean, var = self.decoder.member_moments(z, self.members, weights=w, counts=self.counts, unbiased=bool(unbiased), fused=self.fused)
        return (mean, var) if layout == "BPFC" else (mean.permute(0, 1, 3, 2), var.permute(0, 1, 3, 2))


def systematic_resample(logw: torch.Tensor, members: int, u: Optional[torch.Tensor] = None, ess_threshold: Optional[float] = None,
                        prior: Optional[torch.Tensor] = None):
    """Systematic resampling of G histories with `members` members each, one launch (sea_resample_systematic), nothing read back.

    logw: log-weights [G * members] (or [G, members]) on the device, member j of history g at g * members + j; prior: log-weights carried from steps
    that did not resample (the `logw_out` of the call before), added first; u: float32 [G] offsets in [0, 1) (None: torch.rand(G) on the device);
    ess_threshold: None — always resample; a fraction f in [0, 1] — only the histories whose effective sample size is below f * members.
    Returns (index, logw_out, ess, resampled):
      index      int32 [G * members] on the device, for RolloutSession.resample / select as it is: global trajectory numbers, never outside their own
                 history, non-decreasing within it; the identity for a history that was not resampled;
      logw_out   float32 [G * members]: 0 where a history was resampled (equal weights), the normalised log-weights otherwise (carry them as `prior`);
      ess        float32 [G]: the effective sample size before resampling;
      resampled  int32 [G]: 1 resampled, 0 kept, -1 no live member (every log-weight NaN or infinite: identity index, zero log-weights).
    A member with a NaN or infinite log-weight is dead: weight 0, never selected."""
    if not isinstance(members, int) or isinstance(members, bool) or members < 1 or members > N.RESAMPLE_MAX_N:
        raise ValueError(f"systematic_resample: members = {members!r} must be an integer in 1 .. {N.RESAMPLE_MAX_N}")
    if not torch.is_tensor(logw) or not logw.is_floating_point() or logw.dim() not in (1, 2) or logw.numel() < 1 or logw.numel() % members \
            or (logw.dim() == 2 and logw.shape[1] != members):
        raise ValueError(f"systematic_resample: logw must be a floating-point [G * {members}] or [G, {members}] tensor, got "
                         f"{tuple(logw.shape) if torch.is_tensor(logw) else type(logw).__name__}")
    G = logw.numel() // members
    if prior is not None and (not torch.is_tensor(prior) or prior.numel() != logw.numel() or prior.device != logw.device or not prior.is_floating_point()):
        raise ValueError(f"systematic_resample: prior must be a floating-point tensor of {logw.numel()} log-weights on {logw.device}")
    if u is not None and (not torch.is_tensor(u) or u.dtype != torch.float32 or u.dim() != 1 or u.shape[0] != G or u.device != logw.device):
        raise ValueError(f"systematic_resample: u must be a float32 [{G}] tensor on {logw.device} (one offset in [0, 1) per history)")
    if ess_threshold is None:
        frac = -1.0
    else:
        frac = float(ess_threshold)
        if not 0.0 <= frac <= 1.0:
            raise ValueError(f"systematic_resample: ess_threshold = {ess_threshold} must be None or a fraction in [0, 1]")
    N.require_gpu(logw, "systematic_resample log-weights")
    with torch.no_grad():
        lw = logw.detach().reshape(-1).to(torch.float32)
        if prior is not None:
            lw = lw + prior.detach().reshape(-1).to(torch.float32)
        lw = lw.contiguous()
        if u is None:
            u = torch.rand(G, device=lw.device, dtype=torch.float32)
        return ops.resample_systematic(lw, u.contiguous(), members, frac)


# ------------------------------------------------------------------------------------------------ sparse observations
def _int_list(x, name: str, what: str):
    """A 1-D sequence or tensor of integers as a list of Python ints; bool, float, empty, nested or ragged input is refused."""
    if torch.is_tensor(x):
        if x.dtype == torch.bool or x.is_floating_point() or x.is_complex() or x.dim() != 1 or x.numel() < 1:
            raise ValueError(f"{what}: {name} must be a non-empty 1-D integer sequence or tensor, got a {tuple(x.shape)} {x.dtype} tensor")
        return [int(v) for v in x.detach().cpu().tolist()]       # a tensor given on the device comes to the host once, here
    try:
        vals = list(x)
    except TypeError:
        raise ValueError(f"{what}: {name} must be a non-empty 1-D integer sequence or tensor, got {type(x).__name__}") from None
    if not vals:
        raise ValueError(f"{what}: {name} is empty")
    out = []
    for v in vals:
        if torch.is_tensor(v) and v.dim() == 0 and v.dtype != torch.bool and not v.is_floating_point() and not v.is_complex():
            v = int(v)
        if isinstance(v, bool) or not isinstance(v, int):
            if _np is None or not isinstance(v, _np.integer):
                raise ValueError(f"{what}: {name} must hold integers only (no bool, float or nested sequence), got {type(v).__name__}")
        out.append(int(v))
    return out


class SensorSet:
    """K >= 1 point sensors shared by all histories of a call: sensor k reads decoded field field[k] at cell cell[k] of patch patch[k].

    patch, cell, field: integer sequences or tensors of equal length (a device tensor comes to the host once, here), checked on the host:
    0 <= patch < n_patches, 0 <= cell < decoder.n_inp, field one of the decoder's fields.  Duplicates are allowed (two instruments at one point).
    The launch tables of sea_decode_sensor_sse are built here, once, and uploaded once per device (at construction for the decoder's device when
    that is a GPU, otherwise at the first call on a device):
      order   the sensors sorted by (group, patch, given order), every (group, observed patch) segment padded to a multiple of 32 entries: K_pad
      perm    int32 [K_pad]: sorted position -> sensor (pad entries point at sensor 0)
      wrow    int32 [K_pad]: the row of the group's second-layer weights, (position of the field in its group) * Cp + cell with Cp = the decoder's
              PADDED cell width (pad entries: 0)
      live    int32 [K_pad]: 1 a sensor, 0 a pad entry
      Q       the observed patches: the sorted union over all groups (`patches`, int64 [Q] on the device)
      seg     int32 [n_groups, Q + 1]: the CSR table of the segments in the sorted list (a (group, patch) pair without sensors: an empty segment)
      inv     int64 [K]: sensor -> sorted position (un-permutes the predictions)
    perm and wrow are range-checked before the upload: the kernel trusts them.  A set belongs to the decoder geometry it was built for (n_patches,
    n_inp, padded width, field grouping); Decode.sensor_sse refuses another.  affine: None, or (scales [K], shifts [K]) — the forward scaling x * a + b of
    every sensor's field into the decoder's scaled units, which scale_values / scale_sigma apply (they raise without it); points: None, or the K mesh
    point ids the sensors sit at, kept for the caller.  MeshUnpatcher.sensor_set passes both."""

    def __init__(self, decoder, n_patches: int, patch, cell, field, affine=None, points=None):
        what = "SensorSet"
        if not isinstance(n_patches, int) or isinstance(n_patches, bool) or n_patches < 1:
            raise ValueError(f"{what}: n_patches = {n_patches!r} must be a positive integer")
        patch, cell, field = _int_list(patch, "patch", what), _int_list(cell, "cell", what), _int_list(field, "field", what)
        K = len(patch)
        if len(cell) != K or len(field) != K:
            raise ValueError(f"{what}: patch, cell and field must have equal lengths, got {K}, {len(cell)}, {len(field)}")
        groups = tuple(tuple(int(f) for f in g) for g in decoder.field_groups)
        where = {}                      # field id -> (group, position in the group, position in the decoder's output)
        pos = 0
        for g, grp in enumerate(groups):
            for j, f in enumerate(grp):
                where[f] = (g, j, pos)
                pos += 1
        C_, Cp = int(decoder.n_inp), int(decoder._n_inp_p)
        for k in range(K):
            if not 0 <= patch[k] < n_patches:
                raise ValueError(f"{what}: sensor {k}: patch {patch[k]} outside 0 .. {n_patches - 1}")
            if not 0 <= cell[k] < C_:
                raise ValueError(f"{what}: sensor {k}: cell {cell[k]} outside 0 .. n_inp - 1 = {C_ - 1}")
            if field[k] not in where:
                raise ValueError(f"{what}: sensor {k}: field {field[k]} is not one of the decoder's fields {sorted(where)}")
        self.n_patches, self.n_inp, self.Cp, self.groups, self.K = n_patches, C_, Cp, groups, K
        self.patch, self.cell, self.field = patch, cell, field
        self.out_field = [where[f][2] for f in field]            # the field's position in the decoder's output (and in a per-field sigma)
        G, T = len(groups), N.SENSOR_TILE
        buckets = {}
        for k in range(K):
            buckets.setdefault((where[field[k]][0], patch[k]), []).append(k)
        self.patches = sorted(set(patch))
        Q = len(self.patches)
        if Q > N.SENSOR_MAX_PATCHES:
            raise ValueError(f"{what}: {Q} observed patches; a set carries at most {N.SENSOR_MAX_PATCHES}")
        perm, wrow, live, seg = [], [], [], []
        for g in range(G):
            row = []
            for p in self.patches:
                row.append(len(perm))
                ks = buckets.get((g, p), [])
                for k in ks:
                    perm.append(k)
                    wrow.append(where[field[k]][1] * Cp + cell[k])
                    live.append(1)
                pad = -len(ks) % T
                perm += [0] * pad
                wrow += [0] * pad
                live += [0] * pad
            row.append(len(perm))
            seg.append(row)
        self.K_pad, self.Q = len(perm), Q
        inv = [0] * K
        for s, (k, l) in enumerate(zip(perm, live)):
            if l:
                inv[k] = s
        # the kernel trusts these: check them here
        for g in range(G):
            for qi in range(Q):
                a, b = seg[g][qi], seg[g][qi + 1]
                if not 0 <= a <= b <= self.K_pad or (b - a) % T:
                    raise ValueError(f"{what}: internal error: segment ({g}, {qi}) = [{a}, {b}) is not a multiple of {T} inside 0 .. {self.K_pad}")
                for s in range(a, b):
                    if not 0 <= wrow[s] < len(groups[g]) * Cp or not 0 <= perm[s] < K:
                        raise ValueError(f"{what}: internal error: entry {s}: W2 row {wrow[s]} or sensor {perm[s]} out of range")
        if self.K_pad < T or self.K_pad >= 2 ** 31 or sum(live) != K:
            raise ValueError(f"{what}: internal error: K_pad = {self.K_pad}, {sum(live)} live entries for {K} sensors")
        self.perm, self.wrow, self.live, self.seg, self.inv = perm, wrow, live, seg, inv
        self._finish_init(what, decoder, affine, points)

    def _finish_init(self, what: str, decoder, affine, points) -> None:
        """The end of the constructor, shared with DerivedSensorSet: the affine and the mesh points (one per sensor), the per-device caches, and the
        upload of the tables when the decoder sits on a GPU."""
        K = self.K
        self._dev = {}
        if affine is not None and (len(affine) != 2 or len(affine[0]) != K or len(affine[1]) != K):
            raise ValueError(f"{what}: affine must be a pair of {K} scales and {K} shifts (one per sensor)")
        if points is not None and len(points) != K:
            raise ValueError(f"{what}: points must name one mesh point per sensor ({K}), got {len(points)}")
        self._affine = None if affine is None else ([float(v) for v in affine[0]], [float(v) for v in affine[1]])
        self.points = None if points is None else [int(v) for v in points]
        self._affine_dev = {}
        dev = next(iter(decoder.parameters())).device
        if dev.type == "cuda":
            self.tables(dev)

    def matches(self, decoder, n_patches: int) -> bool:
        return (self.n_patches == n_patches and self.n_inp == int(decoder.n_inp) and self.Cp == int(decoder._n_inp_p)
                and self.groups == tuple(tuple(int(f) for f in g) for g in decoder.field_groups))

    def tables(self, device):
        """The tables on `device` (uploaded once per device): a dict perm, wrow, live, seg (int32), patches, inv, patch, cell, out_field (int64)."""
        device = torch.device(device)
        t = self._dev.get(device)
        if t is None:
            i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=device)   # noqa: E731
            i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=device)   # noqa: E731
            t = dict(perm=i32(self.perm), wrow=i32(self.wrow), live=i32(self.live), seg=i32(self.seg), patches=i64(self.patches), inv=i64(self.inv),
                     patch=i64(self.patch), cell=i64(self.cell), out_field=i64(self.out_field))
            self._dev[device] = t
        return t

    def _coeffs(self, device):
        if self._affine is None:
            raise ValueError("SensorSet: this set was not built from a mesh (MeshUnpatcher.sensor_set): it has no field scaling")
        device = torch.device(device)
        t = self._affine_dev.get(device)
        if t is None:
            t = (torch.tensor(self._affine[0], dtype=torch.float32, device=device), torch.tensor(self._affine[1], dtype=torch.float32, device=device))
            self._affine_dev[device] = t
        return t

    def scale_values(self, v: torch.Tensor) -> torch.Tensor:
        """Physical sensor readings [..., K] -> the decoder's scaled units: v * a_f + b_f with the forward affine of sensor k's field, the coefficients
        patchify_and_scale applies (float32)."""
        if not torch.is_tensor(v) or v.dim() < 1 or v.shape[-1] != self.K:
            raise ValueError(f"SensorSet.scale_values: need a tensor [..., {self.K}], got {tuple(v.shape) if torch.is_tensor(v) else type(v).__name__}")
        a, b = self._coeffs(v.device)
        return v.to(torch.float32) * a + b

    def scale_sigma(self, s: torch.Tensor) -> torch.Tensor:
        """Physical standard deviations [..., K] -> scaled units: s * |a_f|."""
        if not torch.is_tensor(s) or s.dim() < 1 or s.shape[-1] != self.K:
            raise ValueError(f"SensorSet.scale_sigma: need a tensor [..., {self.K}], got {tuple(s.shape) if torch.is_tensor(s) else type(s).__name__}")
        a, _ = self._coeffs(s.device)
        return s.to(torch.float32) * a.abs()


class SensorLikelihood:
    """Gaussian log-likelihood of sparse sensor readings, per ensemble member: like(y, obs, precision=None) -> log-weights [B * members] (f32, device),
    ready for systematic_resample.

    y: what RolloutSession.step returns for B * members trajectories, [B * members, n_groups, P * D] (member j of history b at row b * members + j);
    obs: float32 [B, K] on y's device, the readings in the sensors' given order, in the decoder's scaled units (SensorSet.scale_values);
    precision: None (1), or float32 [K] or [B, K] on y's device, finite and >= 0 — a weight per reading; 0 marks a missing reading: it is neutral
    whatever obs holds there, NaN and Inf included.  A precision on the device is not read back (a negative or NaN entry there counts as 0); one on
    the host is checked.  sigma: None (1), a positive number, n_fields numbers (one per field in the decoder's output order; taken so when K equals
    n_fields) or K numbers (one per sensor), folded once into a per-sensor precision 1 / sigma^2 that multiplies the call's precision; a sigma given
    on the device is read when the object is built.  logw = -0.5 * sum_k w_k (y_k - obs_k)^2 (Decode.sensor_sse).  fused: None (Decode.sensor_sse's
    rule), True (the fused launch; bf16 only) or False (the composed path).  A call reads nothing back from the device and uploads nothing, once the
    sensor set's tables and the folded sigma are on the device (the first call on a device uploads them).  `decoder` is a sea_amd Decode; no
    autograd graph is built.  score_and_grad(y, obs, precision) adds the gradient of every member's own log-weight with respect to its state, and
    nudge(y, obs, precision, rate) takes one gradient step along it."""

    def __init__(self, decoder, n_patches: int, members: int, sensors: SensorSet, sigma=None, fused: Optional[bool] = None):
        if not isinstance(n_patches, int) or isinstance(n_patches, bool) or n_patches < 1:
            raise ValueError(f"SensorLikelihood: n_patches = {n_patches!r} must be a positive integer")
        if not isinstance(members, int) or isinstance(members, bool) or members < 1:
            raise ValueError(f"SensorLikelihood: members = {members!r} must be a positive integer")
        if not isinstance(sensors, SensorSet):
            raise ValueError(f"SensorLikelihood: sensors must be a SensorSet, got {type(sensors).__name__}")
        if not sensors.matches(decoder, n_patches):
            raise ValueError("SensorLikelihood: the SensorSet was built for another decoder geometry (n_patches, n_inp, padded cell width or field grouping)")
        self.decoder, self.n_patches, self.members, self.sensors, self.fused = decoder, n_patches, members, sensors, fused
        n_fields, K = sum(len(g) for g in decoder.field_groups), sensors.K
        if sigma is None:
            self._prec_host = None
        else:
            s = torch.as_tensor(sigma, dtype=torch.float64).detach().cpu()   # a tensor given on the device comes to the host once, here
            if isinstance(sensors, DerivedSensorSet) and s.dim() == 1 and s.numel() != K:
                raise ValueError(f"SensorLikelihood: with a DerivedSensorSet sigma must be None, a number or {K} numbers (one per reading: a derived reading has "
                                 f"no field of its own), got shape {tuple(s.shape)}")
            if s.dim() > 1 or (s.dim() == 1 and s.numel() not in (n_fields, K)):
                raise ValueError(f"SensorLikelihood: sigma must be None, a number, {n_fields} numbers (one per field) or {K} numbers (one per sensor), "
                                 f"got shape {tuple(s.shape)}")
            if not bool(torch.isfinite(s).all()) or not bool((s > 0).all()):
                raise ValueError(f"SensorLikelihood: sigma must be finite and positive, got {s.tolist()}")
            p = 1.0 / (s * s)
            if p.dim() == 0:
                self._prec_host = [float(p)] * K
            elif p.numel() == n_fields and not isinstance(sensors, DerivedSensorSet):
                self._prec_host = [float(p[f]) for f in sensors.out_field]
            else:
                self._prec_host = [float(v) for v in p]
        self._prec = {}
        dev = next(iter(decoder.parameters())).device
        if dev.type == "cuda":
            self._sigma_precision(dev)

    def _sigma_precision(self, device):
        if self._prec_host is None:
            return None
        t = self._prec.get(device)
        if t is None:
            t = self._prec[device] = torch.tensor(self._prec_host, dtype=torch.float32, device=device)
        return t

    def __call__(self, y: torch.Tensor, obs: torch.Tensor, precision: Optional[torch.Tensor] = None) -> torch.Tensor:
        P = self.n_patches
        if not torch.is_tensor(y) or y.dim() != 3 or y.shape[-1] % P or y.shape[0] < 1:
            raise ValueError(f"SensorLikelihood: y must be [B * members, n_groups, n_patches * D] with n_patches = {P}, got "
                             f"{tuple(y.shape) if torch.is_tensor(y) else type(y).__name__}")
        Bm, G, E = y.shape
        if Bm % self.members:
            raise ValueError(f"SensorLikelihood: the {Bm} trajectories of y are not a multiple of members = {self.members}")
        z = y.reshape(Bm, G, P, E // P).permute(0, 2, 1, 3)          # the re-layout of FieldLikelihood
        _check_sensor_operands("SensorLikelihood", obs, precision, Bm // self.members, self.sensors.K, y.device)
        sp = self._sigma_precision(y.device) if y.is_cuda else None
        if sp is not None:
            precision = sp if precision is None else precision * sp
        wsse = self.decoder.sensor_sse(z, self.sensors, obs, precision=precision, members=self.members, fused=self.fused)
        return -0.5 * wsse


    def score_and_grad(self, y: torch.Tensor, obs: torch.Tensor, precision: Optional[torch.Tensor] = None):
        """(logw [Bm], dlogw_dy [Bm, n_groups, P * D] fp32): __call__'s log-weights (the same bits on the fused path) and the gradient of every member's
        OWN log-weight with respect to its state, in y's layout (the inverse of the re-layout __call__ applies) — Decode.sensor_loss's one pass.  On the
        fused path no graph is built; nothing is read back, and nothing is uploaded after the first call on a device."""
        P = self.n_patches
        if not torch.is_tensor(y) or y.dim() != 3 or y.shape[-1] % P or y.shape[0] < 1:
            raise ValueError(f"SensorLikelihood: y must be [B * members, n_groups, n_patches * D] with n_patches = {P}, got "
                             f"{tuple(y.shape) if torch.is_tensor(y) else type(y).__name__}")
        Bm, G, E = y.shape
        if Bm % self.members:
            raise ValueError(f"SensorLikelihood: the {Bm} trajectories of y are not a multiple of members = {self.members}")
        _check_sensor_operands("SensorLikelihood", obs, precision, Bm // self.members, self.sensors.K, y.device)
        sp = self._sigma_precision(y.device) if y.is_cuda else None
        if sp is not None:
            precision = sp if precision is None else precision * sp
        dec = self.decoder
        fused = self.fused if self.fused is not None else dec._act_dtype() == torch.bfloat16 and (not isinstance(self.sensors, DerivedSensorSet) or self.sensors.fusable)
        z = y.detach().reshape(Bm, G, P, E // P).permute(0, 2, 1, 3)
        if fused:
            if dec._act_dtype() != torch.bfloat16:
                raise ValueError("SensorLikelihood: the fused launch is bf16 only (set_compute_dtype('bf16'), or fused=False)")
            if isinstance(self.sensors, DerivedSensorSet):
                self.sensors._require_fusable("SensorLikelihood")
            N.require_gpu(y, "SensorLikelihood.score_and_grad input")
            wsse, _, dz = dec._sensor_grad_fused(z, self.sensors, obs.detach(), None if precision is None else precision.detach(), self.members, False, True)
        else:
            with torch.enable_grad():
                zz = z.to(torch.float32).contiguous().requires_grad_(True)
                wsse = dec.sensor_loss(zz, self.sensors, obs, precision=precision, members=self.members, fused=False)
                (dz,) = torch.autograd.grad(wsse.sum(), zz)
                wsse = wsse.detach()
        return -0.5 * wsse, (-0.5 * dz.to(torch.float32)).permute(0, 2, 1, 3).reshape(Bm, G, E)

    def nudge(self, y: torch.Tensor, obs: torch.Tensor, precision: Optional[torch.Tensor] = None, rate=1.0) -> torch.Tensor:
        """y + rate * dlogw_dy, in y's dtype: one gradient step on every member's log-likelihood of the readings — a corrected state for
        RolloutSession.step(c, state=...).  rate: a number, or a float32 [Bm] tensor on y's device (one step length per member)."""
        if torch.is_tensor(rate):
            if not torch.is_tensor(y) or rate.dim() != 1 or rate.shape[0] != y.shape[0] or rate.dtype != torch.float32 or rate.device != y.device:
                raise ValueError(f"SensorLikelihood.nudge: a rate tensor must be float32 [{y.shape[0] if torch.is_tensor(y) else 'Bm'}] on the states' device, got "
                                 f"{tuple(rate.shape)} {rate.dtype} on {rate.device}")
            rate = rate.detach().view(-1, 1, 1)
        elif isinstance(rate, bool) or not isinstance(rate, (int, float)) or not math.isfinite(rate):
            raise ValueError(f"SensorLikelihood.nudge: rate must be a finite number or a float32 [Bm] tensor, got {rate!r}")
        _, grad = self.score_and_grad(y, obs, precision)
        return (y.detach().to(torch.float32) + rate * grad).to(y.dtype)


def _check_sensor_operands(what: str, obs, precision, B: int, K: int, device) -> None:
    """obs float32 [B, K] and precision None / float32 [K] / [B, K], both on `device`; a precision on the host is also checked for finite, non-negative values
    (one on the device is not read back)."""
    if not torch.is_tensor(obs) or obs.dim() != 2 or tuple(obs.shape) != (B, K):
        raise ValueError(f"{what}: obs must be a [{B}, {K}] tensor (one row of readings per history, in the sensors' given order), got "
                         f"{tuple(obs.shape) if torch.is_tensor(obs) else type(obs).__name__}")
    if obs.dtype != torch.float32 or obs.device != device:
        raise ValueError(f"{what}: obs must be float32 on {device}, got {obs.dtype} on {obs.device}")
    if precision is not None:
        if not torch.is_tensor(precision) or tuple(precision.shape) not in ((K,), (B, K)):
            raise ValueError(f"{what}: precision must be None or a [{K}] or [{B}, {K}] tensor, got "
                             f"{tuple(precision.shape) if torch.is_tensor(precision) else type(precision).__name__}")
        if precision.dtype != torch.float32:
            raise ValueError(f"{what}: precision must be float32, got {precision.dtype}")
        if precision.device.type == "cpu" and (not bool(torch.isfinite(precision).all()) or not bool((precision >= 0).all())):
            raise ValueError(f"{what}: precision must be finite and >= 0")
        if precision.device != device:
            raise ValueError(f"{what}: precision is on {precision.device}, the states on {device}")


# ------------------------------------------------------------------------------------------------ the ensemble Kalman analysis
def gaspari_cohn(dist: torch.Tensor, radius) -> torch.Tensor:
    """The fifth-order, compactly supported correlation function of Gaspari & Cohn (1999, eq. 4.10) as a localisation taper: 1 at distance 0,
    monotonically down to exactly 0 at 2 * radius and beyond.  dist: a tensor of distances (any shape, any sign); radius: a positive number, the
    half-width c of the function.  Returns a tensor of dist's shape (float32 unless dist is float64)."""
    if not torch.is_tensor(dist) or dist.is_complex():
        raise ValueError(f"gaspari_cohn: dist must be a real tensor of distances, got {type(dist).__name__}")
    if isinstance(radius, bool) or not isinstance(radius, (int, float)) or not math.isfinite(radius) or radius <= 0:
        raise ValueError(f"gaspari_cohn: radius = {radius!r} must be a positive finite number")
    z = dist.to(torch.float64 if dist.dtype == torch.float64 else torch.float32).abs() / float(radius)
    zi = z.clamp(max=1.0)                                             # each branch is evaluated inside its own interval only
    zo = z.clamp(min=1.0, max=2.0)
    inner = (((-0.25 * zi + 0.5) * zi + 0.625) * zi - 5.0 / 3.0) * zi * zi + 1.0
    outer = ((((zo / 12.0 - 0.5) * zo + 0.625) * zo + 5.0 / 3.0) * zo - 5.0) * zo + 4.0 - 2.0 / (3.0 * zo)
    return torch.where(z <= 1.0, inner, torch.where(z < 2.0, outer.clamp(min=0.0), torch.zeros_like(z)))


def _composed_transform(pred, obs, prec, taper, members: int, rho: float, alpha: float):
    """sea_enkf_transform's formulas (include/sea_hip.h) as fp64 torch ops on pred's device: (D f32 [B, Ld, N, N], status int32 [B, Ld]).  Needs
    torch.linalg's Cholesky on that device."""
    f64 = torch.float64
    n = members
    B, K = obs.shape
    zero = torch.zeros((), device=pred.device, dtype=f64)
    p = pred.to(f64).view(B, 1, n, K)
    w = torch.ones(B, 1, K, device=pred.device, dtype=f64) if prec is None else prec.to(f64).expand(B, K).unsqueeze(1)
    w = torch.where(w > 0, w, zero)
    if taper is not None:
        t = taper.to(f64).unsqueeze(0)                                 # [1, Ld, K]
        w = w * torch.where(t > 0, t, zero)
    live = w > 0                                                       # [B, Ld, K]
    ybar = p.mean(dim=2)                                               # [B, 1, K]
    S = torch.where(live.unsqueeze(2), rho * (p - ybar.unsqueeze(2)) * (w / (n - 1)).sqrt().unsqueeze(2), zero)     # [B, Ld, N, K]
    dl = torch.where(live, w.sqrt() * (obs.to(f64).unsqueeze(1) - ybar), zero)                                       # [B, Ld, K]
    C_ = S @ S.transpose(-1, -2)
    v = (S @ dl.unsqueeze(-1)).squeeze(-1)
    eye = torch.eye(n, device=pred.device, dtype=f64)
    bad = ~(torch.isfinite(C_).all(-1).all(-1) & torch.isfinite(v).all(-1))                                          # [B, Ld]
    Msafe = torch.where(bad[..., None, None], eye, eye + C_)
    L, _ = torch.linalg.cholesky_ex(Msafe, check_errors=False)      # its info is not used: measured unreliable for large batches; a failed factor is not finite
    bad = bad | ~torch.isfinite(L).all(-1).all(-1)
    W = torch.cholesky_solve(eye.expand_as(Msafe).contiguous(), torch.where(bad[..., None, None], eye, L))
    G = (W @ torch.where(bad[..., None], zero, v).unsqueeze(-1)) / math.sqrt(n - 1) - alpha * (eye - W)
    Pi = eye - 1.0 / n
    D = (rho - 1.0) * Pi + rho * (G - G.mean(dim=-2, keepdim=True))
    D = torch.where(bad[..., None, None], zero, D)
    count = live.sum(-1).to(torch.int32)
    status = torch.where(bad, torch.full_like(count, -1), count)
    return D.to(torch.float32).contiguous(), status


def _composed_mix(y, D, n_patches: int):
    """sea_ensemble_mix's increment with batched fp32 matrix products: f32, y's shape."""
    B, Ld, n, _ = D.shape
    Bm, G, E = y.shape
    yf = y.to(torch.float32).view(B, n, G, n_patches, E // n_patches)
    if Ld == 1:
        return torch.bmm(D[:, 0].transpose(1, 2), yf.reshape(B, n, -1)).view(Bm, G, E)
    yp = yf.permute(0, 3, 1, 2, 4).reshape(B, n_patches, n, -1)       # [B, P, N, G * Dl]
    inc = torch.matmul(D.transpose(2, 3), yp)                          # [B, P, N, G * Dl]
    return inc.view(B, n_patches, n, G, E // n_patches).permute(0, 2, 3, 1, 4).reshape(Bm, G, E)


class SensorKalman:
    """The ensemble Kalman analysis of an ensemble's latent states from sparse sensor readings — the deterministic EnKF of Sakov & Oke (2008) in
    ensemble space, two launches behind the predictions: kalman.analyse(y, obs, precision=None) -> y_a in y's layout and dtype, a corrected state
    for RolloutSession.step(c, state=y_a).  No random numbers, no step length to tune, and the ensemble keeps its N distinct members.

    y: what RolloutSession.step returns for B * members trajectories, [B * members, n_groups, P * D]; obs, precision, sigma: exactly SensorLikelihood's
    (readings float32 [B, K] in the decoder's scaled units; a precision 0 marks a missing reading — neutral whatever obs holds there).  The members'
    predictions at the sensors come from Decode.sensor_sse(..., predictions=True) (the fused launch in bf16, the composed path in fp32); from them
    sea_enkf_transform forms, per history and analysis domain, the [N, N] matrix D of include/sea_hip.h in fp64 (the mean moves by K (obs - H xbar),
    the anomalies by -anomaly_gain K H A, K the Kalman gain of the forecast inflated by `inflation` >= 1), and sea_ensemble_mix applies
    y_a[j] = y[j] + sum_i D[i, j] y[i] to every latent element.  taper: None — one domain: every patch takes the same D; or float32 [P, K] weights in
    [0, 1] (MeshUnpatcher.sensor_taper) — patch p's latent slice is analysed by its own problem, whose precisions are multiplied by taper[p]
    (LETKF-style domain localisation; a patch is the natural domain of a latent state stored per patch).  A taper on the host is uploaded once per
    device.  transform(y, obs, precision) -> (D [B, Ld, N, N], status [B, Ld], pred [B * N, K]); status is the number of live readings of a problem,
    or -1 where a live operand was not finite: that problem's D is 0 and its states pass through unchanged.  analyse(..., increment=True) also returns
    the fp32 increment y_a - y before rounding.  fused: None or True — the two launches; False — the same formulas as fp64 torch ops on the device and
    batched fp32 matrix products, for comparison (it needs torch.linalg's Cholesky on the device; the predictions are sensor_sse's either way).
    fused=None is the measured rule (tools/enkf_bench.py, profiles/enkf_bench.txt): the two launches, except for ONE problem (one
    history, one domain) with 4096 sensors or more, the only measured rows with the composed path ahead (a single workgroup then carries all the fp64
    work of C = S S^T).  A call reads nothing back from
    the device and uploads nothing after the first call on a device.  2 <= members <= 128.  `decoder` is a sea_amd Decode; no autograd graph is built."""

    def __init__(self, decoder, n_patches: int, members: int, sensors: SensorSet, sigma=None, inflation: float = 1.0, anomaly_gain: float = 0.5,
                 taper=None, fused: Optional[bool] = None):
        if not isinstance(members, int) or isinstance(members, bool) or members < 2 or members > N.ENKF_MAX_N:
            raise ValueError(f"SensorKalman: members = {members!r} must be an integer in 2 .. {N.ENKF_MAX_N}")
        self._like = SensorLikelihood(decoder, n_patches, members, sensors, sigma=sigma)   # its checks, its folding of sigma
        for name, v, lo, hi in (("inflation", inflation, 1.0, float("inf")), ("anomaly_gain", anomaly_gain, 0.0, 1.0)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not lo <= v <= hi:
                raise ValueError(f"SensorKalman: {name} = {v!r} must be a finite number in [{lo}, {hi}]")
        self.decoder, self.n_patches, self.members, self.sensors, self.fused = decoder, n_patches, members, sensors, fused
        self.inflation, self.anomaly_gain = float(inflation), float(anomaly_gain)
        self._taper = {}
        if taper is None:
            self._taper_src = None
        else:
            t = taper if torch.is_tensor(taper) else torch.as_tensor(taper)
            if t.dim() != 2 or tuple(t.shape) != (n_patches, sensors.K) or not t.is_floating_point():
                raise ValueError(f"SensorKalman: taper must be None or a float32 [{n_patches}, {sensors.K}] array (one row of weights per patch), got "
                                 f"{tuple(t.shape)} {t.dtype}")
            t = t.detach().to(torch.float32).contiguous()
            if t.device.type == "cpu" and (not bool(torch.isfinite(t).all()) or not bool(((t >= 0) & (t <= 1)).all())):
                raise ValueError("SensorKalman: taper weights must lie in [0, 1]")
            self._taper_src = t
            self._taper[t.device] = t
            dev = next(iter(decoder.parameters())).device
            if dev.type == "cuda":
                self._taper_on(dev)

    def _taper_on(self, device):
        if self._taper_src is None:
            return None
        t = self._taper.get(device)
        if t is None:
            t = self._taper[device] = self._taper_src.to(device)
        return t

    def _fused_for(self, histories: int) -> bool:
        if self.fused is not None:
            return bool(self.fused)
        domains = 1 if self._taper_src is None else self.n_patches
        return not (histories * domains == 1 and self.sensors.K >= 4096)

    def _operands(self, y, obs, precision):
        P, n = self.n_patches, self.members
        if not torch.is_tensor(y) or y.dim() != 3 or y.shape[-1] % P or y.shape[0] < 1:
            raise ValueError(f"SensorKalman: y must be [B * members, n_groups, n_patches * D] with n_patches = {P}, got "
                             f"{tuple(y.shape) if torch.is_tensor(y) else type(y).__name__}")
        Bm, G, E = y.shape
        if Bm % n:
            raise ValueError(f"SensorKalman: the {Bm} trajectories of y are not a multiple of members = {n}")
        _check_sensor_operands("SensorKalman", obs, precision, Bm // n, self.sensors.K, y.device)
        sp = self._like._sigma_precision(y.device) if y.is_cuda else None
        if sp is not None:
            precision = sp if precision is None else precision * sp
        return y.detach(), obs.detach(), None if precision is None else precision.detach()

    def transform(self, y: torch.Tensor, obs: torch.Tensor, precision: Optional[torch.Tensor] = None):
        """(D f32 [B, Ld, N, N], status int32 [B, Ld], pred f32 [B * N, K]): the ensemble-space matrix of the analysis, the live readings per problem
        (-1: no update) and the members' predictions at the sensors (the innovation of member j is pred[j] - obs)."""
        y, obs, prec = self._operands(y, obs, precision)
        Bm, G, E = y.shape
        P, n = self.n_patches, self.members
        z = y.reshape(Bm, G, P, E // P).permute(0, 2, 1, 3)          # the re-layout of SensorLikelihood
        _, pred = self.decoder.sensor_sse(z, self.sensors, obs, precision=prec, members=n, predictions=True)
        taper = self._taper_on(y.device)
        with torch.no_grad():
            if self._fused_for(obs.shape[0]):
                D, status = ops.enkf_transform(pred, obs, n, prec=prec, taper=taper, rho=self.inflation, alpha=self.anomaly_gain)
            else:
                D, status = _composed_transform(pred, obs, prec, taper, n, self.inflation, self.anomaly_gain)
        return D, status, pred

    def analyse(self, y: torch.Tensor, obs: torch.Tensor, precision: Optional[torch.Tensor] = None, increment: bool = False):
        """y_a in y's layout and dtype — or (y_a, increment f32) with increment=True — from one set of readings."""
        D, _, _ = self.transform(y, obs, precision)
        yc = y.detach().contiguous()
        with torch.no_grad():
            if self._fused_for(obs.shape[0]):
                return ops.ensemble_mix(yc, D, self.n_patches, output=True, increment=bool(increment))
            inc = _composed_mix(yc, D, self.n_patches)
            out = (yc.to(torch.float32) + inc).to(y.dtype)
        return (out, inc) if increment else out


def _composed_transform_gram(gram, proj, count, taper, members: int, rho: float, alpha: float):
    """sea_enkf_transform_gram's formulas (include/sea_hip.h) as fp64 torch ops on gram's device: (D f32 [B, Ld, N, N], status int32 [B, Ld])."""
    f64 = torch.float64
    n = members
    B, Q = count.shape
    zero = torch.zeros((), device=gram.device, dtype=f64)
    t = torch.ones(1, Q, device=gram.device, dtype=f64) if taper is None else taper.to(f64)
    t = torch.where(t > 0, t, zero)                                                                  # [Ld, Q]
    use = (t > 0).unsqueeze(0) & (count != 0).unsqueeze(1)                                           # [B, Ld, Q]
    tw = torch.where(use & (count > 0).unsqueeze(1), t.unsqueeze(0), zero)
    ok = (count > 0)
    g = torch.where(ok[..., None, None], gram, zero)
    pr = torch.where(ok[..., None], proj, zero)
    C_ = (rho * rho / (n - 1)) * torch.einsum("bdq,bqij->bdij", tw, g)
    v = (rho / math.sqrt(n - 1)) * torch.einsum("bdq,bqi->bdi", tw, pr)
    eye = torch.eye(n, device=gram.device, dtype=f64)
    bad = (use & (count < 0).unsqueeze(1)).any(-1) | ~(torch.isfinite(C_).all(-1).all(-1) & torch.isfinite(v).all(-1))    # [B, Ld]
    Msafe = torch.where(bad[..., None, None], eye, eye + C_)
    L, _ = torch.linalg.cholesky_ex(Msafe, check_errors=False)
    bad = bad | ~torch.isfinite(L).all(-1).all(-1)
    W = torch.cholesky_solve(eye.expand_as(Msafe).contiguous(), torch.where(bad[..., None, None], eye, L))
    G = (W @ torch.where(bad[..., None], zero, v).unsqueeze(-1)) / math.sqrt(n - 1) - alpha * (eye - W)
    Pi = eye - 1.0 / n
    D = (rho - 1.0) * Pi + rho * (G - G.mean(dim=-2, keepdim=True))
    D = torch.where(bad[..., None, None], zero, D)
    live = torch.where(use, count.unsqueeze(1).expand_as(use), torch.zeros_like(count).unsqueeze(1).expand_as(use)).sum(-1).to(torch.int32)
    status = torch.where(bad, torch.full_like(live, -1), live)
    return D.to(torch.float32).contiguous(), status


class _FieldObserver:
    """What FieldKalman and FieldVerification share: the checks of (y, obs, precision) against a dense snapshot, the layout, and sigma folded into an f32
    [n_fields] precision on the device.  _what names the class in the messages."""
    _what = "FieldObserver"

    def _set_sigma(self, sigma, n_fields: int) -> None:
        if sigma is None:
            self._prec_host = None
        else:
            s = torch.as_tensor(sigma, dtype=torch.float64).detach().cpu()   # a tensor given on the device comes to the host once, here
            if s.dim() > 1 or (s.dim() == 1 and s.numel() != n_fields):
                raise ValueError(f"{self._what}: sigma must be None, a number or {n_fields} numbers (one per field), got shape {tuple(s.shape)}")
            if not bool(torch.isfinite(s).all()) or not bool((s > 0).all()):
                raise ValueError(f"{self._what}: sigma must be finite and positive, got {s.tolist()}")
            self._prec_host = [float(v) for v in (1.0 / (s * s)).expand(n_fields)]
        self._prec = None

    def _field_precision(self, device):
        """1 / sigma_f^2 as an f32 [n_fields] tensor on the device (None without sigma), built once per device by fills."""
        if self._prec_host is None:
            return None
        if self._prec is None or self._prec.device != device:
            prec = torch.empty(len(self._prec_host), device=device, dtype=torch.float32)
            for f, v in enumerate(self._prec_host):
                prec[f].fill_(v)
            self._prec = prec
        return self._prec

    def _operands(self, y, obs, precision, gpu: bool = True):
        P, n, what = self.n_patches, self.members, self._what
        if not torch.is_tensor(y) or y.dim() != 3 or y.shape[-1] % P or y.shape[0] < 1:
            raise ValueError(f"{what}: y must be [B * members, n_groups, n_patches * D] with n_patches = {P}, got "
                             f"{tuple(y.shape) if torch.is_tensor(y) else type(y).__name__}")
        Bm = y.shape[0]
        if Bm % n:
            raise ValueError(f"{what}: the {Bm} trajectories of y are not a multiple of members = {n}")
        B = Bm // n
        if not torch.is_tensor(obs) or obs.dim() != 4 or tuple(obs.shape[:2]) != (B, P):
            raise ValueError(f"{what}: the observation must be [{B}, {P}, ...] in layout {self.layout} (one snapshot per history), got "
                             f"{tuple(obs.shape) if torch.is_tensor(obs) else type(obs).__name__}")
        if obs.dtype != torch.float32 or obs.device != y.device:
            raise ValueError(f"{what}: obs must be float32 on {y.device}, got {obs.dtype} on {obs.device}")
        if precision is not None:
            if not torch.is_tensor(precision) or tuple(precision.shape) != tuple(obs.shape):
                raise ValueError(f"{what}: precision must be None or a map of obs's shape {tuple(obs.shape)}, got "
                                 f"{tuple(precision.shape) if torch.is_tensor(precision) else type(precision).__name__}")
            if precision.dtype != torch.float32:
                raise ValueError(f"{what}: precision must be float32, got {precision.dtype}")
            if precision.device.type == "cpu" and (not bool(torch.isfinite(precision).all()) or not bool((precision >= 0).all())):
                raise ValueError(f"{what}: precision must be finite and >= 0")
            if precision.device != y.device:
                raise ValueError(f"{what}: precision is on {precision.device}, the states on {y.device}")
        if gpu:
            N.require_gpu(y, f"{what} states")
        perm = (lambda t: t) if self.layout == "BPFC" else (lambda t: t.permute(0, 1, 3, 2))
        return y.detach(), perm(obs.detach()), None if precision is None else perm(precision.detach())


class FieldKalman(_FieldObserver):
    """The ensemble Kalman analysis of an ensemble's latent states from a DENSE snapshot of the decoded fields — a PIV frame, a coarse solver's field, a
    reanalysis — by the deterministic EnKF of Sakov & Oke (2008) in ensemble space: kalman.analyse(y, obs, precision=None) -> y_a in y's layout and
    dtype, a corrected state for RolloutSession.step(c, state=y_a).  All members move, none is duplicated; no random numbers.

    y, obs, layout, counts and sigma mean what they mean in FieldLikelihood: y [B * members, n_groups, P * D] as RolloutSession.step returns it (member j
    of history b at row b * members + j); obs float32 [B, P, n_fields, C >= n_inp] (layout "BPFC") or the reference's [B, P, C, n_fields] ("BPCF"), one
    snapshot per history, in the decoder's scaled units; counts: valid cells per patch (None: all); sigma: None (1), a positive number or n_fields
    positive numbers — the precision of a cell of field f is 1 / sigma_f^2.  precision: an optional float32 map in obs's layout and shape, >= 0, that
    multiplies it; 0 marks a missing cell, neutral whatever obs holds there (NaN included).  A dense snapshot makes the ensemble-space matrix large:
    choose sigma as the error of one CELL, not of a field.
    Three launches behind the decoder's first layer: sea_decode_member_gram (per (history, patch) the N x N Gram matrix of the members' weighted decoded
    anomalies and its product with the innovation; the members' fields and a [B * N, cells] prediction matrix never exist), sea_enkf_transform_gram
    (the weighted sum of the patches' matrices per analysis domain, then SensorKalman's factorisation: D [B, Ld, N, N], include/sea_hip.h), and
    sea_ensemble_mix (y_a[j] = y[j] + sum_i D[i, j] y[i]).  taper: None — one domain, every patch takes the same D; or a float [P, P] array in [0, 1]
    (MeshUnpatcher.patch_taper) — patch p's latent slice is analysed by its own problem in which the cells of patch q weigh taper[p, q]; uploaded once
    per device.  Because a domain's matrix is a weighted sum of patch matrices, localisation costs P small sums per domain, not a pass over the cells.
    transform(y, obs, precision) -> (D, status): status int32 [B, Ld] is the number of live cells of a problem, or -1 where an operand of a contributing
    patch was not finite: that problem's D is 0 and its states pass through unchanged.  analyse(..., increment=True) also returns the fp32 increment.
    fused: True — the launches above (bf16 only); False — Decode.forward plus the same formulas as fp64 torch ops and batched fp32 products, for
    comparison (it holds the members' decoded fields in float64 and needs torch.linalg's Cholesky on the device, whose factor at 128 members came back
    wrong in one of three runs in the torch build this was developed on: DESIGN.md section 7j).  fused=None decides the DECODE (fused launch or
    Decode.forward plus fp64 reductions, the only form in fp32) and always takes the transform and mix launches, which do not depend on the
    decoder's dtype and are ahead of the torch formulas in every measured row (0.14 - 0.15 against 0.42 - 0.73 ms).  It is the measured rule
    (tools/field_enkf_bench.py, profiles/field_enkf_bench.txt; 64 members x 64 patches, n_inp 1628, cylinder and multiphase
    decoder, every column valid and the mesh's counts, device time per analyse call): one history, one domain 0.87 - 0.94 ms fused against 1.44 -
    1.47 ms composed; one history, 64 domains 0.83 - 0.90 against 1.79 - 1.92 ms; four histories 0.85 - 0.96 against 4.15 - 4.28 ms; 7 launches against
    152 - 168; 11 - 54 MB of extra memory against 0.5 - 2.5 GB; SensorKalman with every valid cell a sensor: 18.5 ms (90 000 cells) and 63.1 ms (312 576).
    So: the fused decode in bf16 from 4096 rows (B * members * P) on — every measured row — and the composed decode below, where nothing was measured.
    A call reads nothing back from the device and uploads nothing after the first call on a device.  2 <= members <= 128.  `decoder` is a sea_amd
    Decode; no autograd graph is built."""

    _what = "FieldKalman"

    def __init__(self, decoder, n_patches: int, members: int, counts=None, layout: str = "BPFC", sigma=None, inflation: float = 1.0,
                 anomaly_gain: float = 0.5, taper=None, fused: Optional[bool] = None):
        if layout not in ("BPFC", "BPCF"):
            raise ValueError(f"FieldKalman: layout must be 'BPFC' or 'BPCF', got {layout!r}")
        if not isinstance(n_patches, int) or isinstance(n_patches, bool) or n_patches < 1:
            raise ValueError(f"FieldKalman: n_patches = {n_patches!r} must be a positive integer")
        if not isinstance(members, int) or isinstance(members, bool) or members < 2 or members > N.ENKF_MAX_N:
            raise ValueError(f"FieldKalman: members = {members!r} must be an integer in 2 .. {N.ENKF_MAX_N}")
        for name, v, lo, hi in (("inflation", inflation, 1.0, float("inf")), ("anomaly_gain", anomaly_gain, 0.0, 1.0)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not lo <= v <= hi:
                raise ValueError(f"FieldKalman: {name} = {v!r} must be a finite number in [{lo}, {hi}]")
        if fused not in (None, True, False):
            raise ValueError(f"FieldKalman: fused must be None, True or False, got {fused!r}")
        self.decoder, self.n_patches, self.members, self.counts, self.layout, self.fused = decoder, n_patches, members, counts, layout, fused
        self.inflation, self.anomaly_gain = float(inflation), float(anomaly_gain)
        n_fields = sum(len(g) for g in decoder.field_groups)
        self._set_sigma(sigma, n_fields)
        self._taper = {}
        if taper is None:
            self._taper_src = None
        else:
            t = taper if torch.is_tensor(taper) else torch.as_tensor(taper)
            if t.dim() != 2 or tuple(t.shape) != (n_patches, n_patches) or not t.is_floating_point():
                raise ValueError(f"FieldKalman: taper must be None or a float [{n_patches}, {n_patches}] array (row p: the weights of the patches in patch p's "
                                 f"analysis), got {tuple(t.shape)} {t.dtype}")
            t = t.detach().to(torch.float32).contiguous()
            if t.device.type == "cpu" and (not bool(torch.isfinite(t).all()) or not bool(((t >= 0) & (t <= 1)).all())):
                raise ValueError("FieldKalman: taper weights must lie in [0, 1]")
            self._taper_src = t
            self._taper[t.device] = t
            dev = next(iter(decoder.parameters())).device
            if dev.type == "cuda":
                self._taper_on(dev)

    def _taper_on(self, device):
        if self._taper_src is None:
            return None
        t = self._taper.get(device)
        if t is None:
            t = self._taper[device] = self._taper_src.to(device)
        return t

    def _fused_for(self, y) -> bool:
        """Whether the decode and reduction run as the fused launch (sea_decode_member_gram)."""
        if self.fused is not None:
            return bool(self.fused)
        return self.decoder._act_dtype() == torch.bfloat16 and y.shape[0] * self.n_patches >= 4096

    def _native_tail(self) -> bool:
        """Whether the transform and the mix run as sea_enkf_transform_gram and sea_ensemble_mix: always, except with fused=False (all torch ops, for
        comparison).  The two launches take fp64 partials and fp32 or bf16 states whatever the decoder computed in."""
        return self.fused is not False

    def transform(self, y: torch.Tensor, obs: torch.Tensor, precision: Optional[torch.Tensor] = None):
        """(D f32 [B, Ld, N, N], status int32 [B, Ld]): the ensemble-space matrix of the analysis and the live cells per problem (-1: no update)."""
        y, tgt, prec = self._operands(y, obs, precision)
        Bm, G, E = y.shape
        P, n = self.n_patches, self.members
        fused = self._fused_for(y)
        z = y.reshape(Bm, G, P, E // P).permute(0, 2, 1, 3)          # the re-layout of FieldLikelihood
        gram, proj, count = self.decoder.member_gram(z, tgt, n, counts=self.counts, precision=prec, field_precision=self._field_precision(y.device), fused=fused)
        taper = self._taper_on(y.device)
        with torch.no_grad():
            if self._native_tail():
                return ops.enkf_transform_gram(gram, proj, count, taper=taper, rho=self.inflation, alpha=self.anomaly_gain)
            return _composed_transform_gram(gram, proj, count, taper, n, self.inflation, self.anomaly_gain)

    def analyse(self, y: torch.Tensor, obs: torch.Tensor, precision: Optional[torch.Tensor] = None, increment: bool = False):
        """y_a in y's layout and dtype — or (y_a, increment f32) with increment=True — from one snapshot: the correct(y, observation) of a rollout."""
        D, _ = self.transform(y, obs, precision)
        yc = y.detach().contiguous()
        with torch.no_grad():
            if self._native_tail():
                return ops.ensemble_mix(yc, D, self.n_patches, output=True, increment=bool(increment))
            inc = _composed_mix(yc, D, self.n_patches)
            out = (yc.to(torch.float32) + inc).to(y.dtype)
        return (out, inc) if increment else out


# ------------------------------------------------------------------------------------------------ verification at the sensors
@dataclasses.dataclass(frozen=True)
class EnsembleScores:
    """What SensorVerification returns, all on the predictions' device.  Per (history, sensor), [B, K]: crps, pit, mean, spread (float32) and rank
    (int32: live members below the reading; -1 a reading without weight, -2 a bad sensor — a live reading or a live member's prediction that is not
    finite; its floats are NaN).  Per history: sums float64 [B, 8] (count of live good sensors, sum crps, sum (y - mean)^2, sum spread^2,
    sum (y - mean)^2 / (spread^2 + 1 / precision), sum (mean - y), count of bad sensors, sum 1 / precision), hist int64 [B, members + 1] (the rank
    histogram over the same sensors) and status int32 [B] (the live members; -1: the history's log-weights hold a NaN, +inf or no finite entry, and
    it was not scored).  sums and hist add up over calls (into=).  The derived properties are float64 [B] tensor expressions of sums: nothing is read
    back; a history without a live good sensor gives NaN."""
    crps: torch.Tensor
    pit: torch.Tensor
    rank: torch.Tensor
    mean: torch.Tensor
    spread: torch.Tensor
    sums: torch.Tensor
    hist: torch.Tensor
    status: torch.Tensor

    @property
    def count(self):
        return self.sums[:, 0]

    @property
    def mean_crps(self):
        return self.sums[:, 1] / self.sums[:, 0]

    @property
    def rmse(self):
        """The root-mean-square error of the ensemble mean at the sensors."""
        return (self.sums[:, 2] / self.sums[:, 0]).sqrt()

    @property
    def mean_spread(self):
        """The root of the mean ensemble variance at the sensors (what the error of the mean is to be compared with)."""
        return (self.sums[:, 3] / self.sums[:, 0]).sqrt()

    @property
    def spread_skill(self):
        """mean_spread / rmse: below 1 the ensemble is under-dispersive (raise the inflation), above 1 over-dispersive."""
        return (self.sums[:, 3] / self.sums[:, 2]).sqrt()

    @property
    def consistency(self):
        """The mean of (y - mean)^2 / (spread^2 + 1 / precision): about 1 for a calibrated ensemble with honest observation errors."""
        return self.sums[:, 4] / self.sums[:, 0]

    @property
    def bias(self):
        """The mean of (ensemble mean - reading)."""
        return self.sums[:, 5] / self.sums[:, 0]

    @property
    def suggested_inflation(self):
        """sqrt(max(1, (sum (y - mean)^2 - sum 1 / precision) / sum spread^2)): the moment estimate of the inflation that would make the spread
        consistent with the error of the mean (Wang & Bishop 2003; Desroziers et al. 2005)."""
        return ((self.sums[:, 2] - self.sums[:, 7]) / self.sums[:, 3]).clamp_min(1.0).sqrt()


def _composed_verify(pred, obs, prec, logw, members: int, unbiased: bool, out_dtype=torch.float32):
    """sea_ensemble_verify's formulas (include/sea_hip.h) as fp64 torch ops on pred's device — a stable sort, a cumulative sum, gathers — for any
    member count: a dict with ops.ensemble_verify's keys (out_dtype: the dtype of the per-sensor floats).  Nothing is read back."""
    f64 = torch.float64
    n = members
    B, K = obs.shape
    dev = pred.device
    zero = torch.zeros((), device=dev, dtype=f64)
    x = pred.to(f64).view(B, n, K)
    y = obs.to(f64)
    lw = torch.zeros(B, n, device=dev, dtype=f64) if logw is None else logw.to(f64).view(B, n)
    invalid = (torch.isnan(lw) | (lw == float("inf"))).any(1) | ~torch.isfinite(lw).any(1)            # [B]
    lw = torch.where(invalid.unsqueeze(1), zero, lw)
    alive = lw != float("-inf")                                                                      # [B, N]
    e = torch.where(alive, (lw - lw.max(dim=1, keepdim=True).values).exp(), zero)
    w = e / e.sum(dim=1, keepdim=True)
    c = 1.0 - (w * w).sum(dim=1, keepdim=True) if unbiased else torch.ones(B, 1, device=dev, dtype=f64)
    pos = c > 0
    c_safe = torch.where(pos, c, torch.ones_like(c))
    p = torch.ones(B, K, device=dev, dtype=f64) if prec is None else prec.to(f64).expand(B, K)
    live = (p > 0) & ~invalid.unsqueeze(1)                                                           # [B, K]
    finite = torch.isfinite(y) & torch.isfinite(p) & (torch.isfinite(x) | ~alive.unsqueeze(2)).all(1)
    bad = live & ~finite
    good = live & finite
    use = good.unsqueeze(1) & alive.unsqueeze(2)                                                     # [B, N, K]: what enters a sum
    xs = torch.where(use, x, zero)
    ys = torch.where(good, y, zero)
    rvar = 1.0 / torch.where(good, p, torch.ones_like(p))
    wv = torch.where(use, w.unsqueeze(2), zero)
    mean = (wv * xs).sum(1)
    sp2 = torch.where(pos, (wv * (xs - mean.unsqueeze(1)) ** 2).sum(1) / c_safe, zero)
    d = xs - ys.unsqueeze(1)
    order = torch.sort(xs, dim=1, stable=True).indices                                                # ties keep the member order
    ws, ds = torch.gather(wv, 1, order), torch.gather(d, 1, order)
    below = ws.cumsum(1) - ws
    pair = (ws * ds * (2.0 * below + ws - 1.0)).sum(1)
    crps = (wv * d.abs()).sum(1) - torch.where(pos, pair / c_safe, zero)
    lt, eq = xs < ys.unsqueeze(1), xs == ys.unsqueeze(1)
    pit = (wv * (lt.to(f64) + 0.5 * eq.to(f64))).sum(1)
    rank = (lt & use).sum(1)
    err = ys - mean
    terms = torch.stack([good.to(f64), crps, err * err, sp2, err * err / (sp2 + rvar), mean - ys, zero.expand(B, K), rvar], dim=2)   # [B, K, 8]
    sums = torch.where(good.unsqueeze(2), terms, zero).sum(1)
    sums[:, 6] = bad.sum(1).to(f64)
    hist = torch.zeros(B, n + 1, device=dev, dtype=torch.int64).scatter_add_(1, torch.where(good, rank, torch.zeros_like(rank)), good.to(torch.int64))
    nan = torch.full((), float("nan"), device=dev, dtype=f64)
    f32 = lambda t: torch.where(bad, nan, torch.where(good, t, zero)).to(out_dtype)   # noqa: E731
    rank = torch.where(bad, torch.full_like(rank, -2), torch.where(good, rank, torch.full_like(rank, -1))).to(torch.int32)
    status = torch.where(invalid, torch.full_like(invalid, -1, dtype=torch.int64), alive.sum(1)).to(torch.int32)
    return dict(mean=f32(mean), spread=f32(sp2.sqrt()), crps=f32(crps), pit=f32(pit), rank=rank, sums=sums, hist=hist, status=status)


class SensorVerification:
    """Verification of an ensemble against sparse sensor readings — is the ensemble any good: verify(y, obs, precision=None, logw=None, into=None) ->
    EnsembleScores.  Per (history, sensor) the continuous ranked probability score, the probability integral transform, the rank of the reading among
    the members, the ensemble mean and spread; per history the fp64 sums behind rmse, mean_spread, spread_skill, consistency, bias, mean_crps and
    suggested_inflation, and the rank histogram — what inflation, anomaly_gain, sigma and a taper radius of SensorKalman are tuned by.

    y, obs, precision, sigma: exactly SensorLikelihood's (that object's checks and its folding of sigma into the precision; 1 / precision is the
    reading's observation-error variance; precision 0 marks a missing reading — neutral whatever obs and the predictions hold there).  logw: None
    (equal weights) or [B * members] (or [B, members]) unnormalised log-weights; a member with -inf is dead: weight 0, not ranked.  unbiased=True
    divides the spread's and the CRPS's member-pair terms by 1 - sum w^2 (N / (N - 1) for equal weights: the fair CRPS).  The predictions come from
    Decode.sensor_sse(..., predictions=True); from_predictions(pred, obs, ...) skips the decode — the pred that SensorKalman.transform returned is
    scored as the forecast without decoding twice.  into: an earlier result; this call's sums and histogram are added onto ITS sums and hist (in
    place), so a run aggregates its cycles without host work.  fused: True — the two launches of sea_ensemble_verify (include/sea_hip.h; up to 128
    members, GPU tensors); False — the same formulas as fp64 torch ops (a sort, a cumulative sum, gathers), for comparison, for more than 128 members
    and for CPU tensors through from_predictions.  fused=None is the measured rule (tools/verify_bench.py, profiles/verify_bench.txt, DESIGN.md
    section 7i): the two launches up to 128 members — every measured row has them ahead of the composed path (64 members, 16 to 4096 sensors, one
    and four histories, with and without log-weights: 0.035 - 0.050 ms against 0.76 - 1.00 ms per from_predictions call; 128 members at 256 and 4096
    sensors: 0.047 - 0.093 against 0.69 - 0.87 ms); other member counts were not measured and follow the same rule.  A call reads nothing
    back from the device and uploads nothing after the first call on a device.  `decoder` is a sea_amd Decode; no autograd graph is built."""

    def __init__(self, decoder, n_patches: int, members: int, sensors: SensorSet, sigma=None, unbiased: bool = True, fused: Optional[bool] = None):
        if not isinstance(members, int) or isinstance(members, bool) or members < 1:
            raise ValueError(f"SensorVerification: members = {members!r} must be a positive integer")
        if fused is not None and not isinstance(fused, bool):
            raise ValueError(f"SensorVerification: fused = {fused!r} must be None, True or False")
        if fused and members > N.VERIFY_MAX_N:
            raise ValueError(f"SensorVerification: the fused launches carry up to {N.VERIFY_MAX_N} members, got {members} (fused=False, or None)")
        self._like = SensorLikelihood(decoder, n_patches, members, sensors, sigma=sigma)   # its checks, its folding of sigma
        self.decoder, self.n_patches, self.members, self.sensors, self.fused, self.unbiased = decoder, n_patches, members, sensors, fused, bool(unbiased)

    def _fused_for(self, device) -> bool:
        if self.fused is not None:
            return bool(self.fused)
        return self.members <= N.VERIFY_MAX_N and device.type == "cuda"

    def _operands(self, obs, precision, logw, into, B: int, device):
        n, K = self.members, self.sensors.K
        _check_sensor_operands("SensorVerification", obs, precision, B, K, device)
        sp = self._like._sigma_precision(device)
        if sp is not None:
            precision = sp if precision is None else precision * sp
        if logw is not None:
            if not torch.is_tensor(logw) or not logw.is_floating_point() or logw.numel() != B * n or logw.dim() not in (1, 2) \
                    or (logw.dim() == 2 and logw.shape[1] != n) or logw.device != device:
                raise ValueError(f"SensorVerification: logw must be None or a floating-point [{B * n}] (or [{B}, {n}]) tensor of log-weights on {device}, got "
                                 f"{(tuple(logw.shape), str(logw.device)) if torch.is_tensor(logw) else type(logw).__name__}")
            logw = logw.detach().reshape(-1).to(torch.float32).contiguous()
        if into is not None:
            if not isinstance(into, EnsembleScores) or tuple(into.sums.shape) != (B, N.VERIFY_SUMS) or tuple(into.hist.shape) != (B, n + 1) \
                    or into.sums.device != device or into.sums.dtype != torch.float64 or into.hist.dtype != torch.int64 \
                    or not into.sums.is_contiguous() or not into.hist.is_contiguous():
                raise ValueError(f"SensorVerification: into must be an earlier EnsembleScores for {B} histories of {n} members on {device}")
        return obs.detach(), None if precision is None else precision.detach(), logw

    def _verify(self, pred, obs, prec, logw, into) -> EnsembleScores:
        with torch.no_grad():
            if self._fused_for(pred.device):
                out = None if into is None else dict(sums=into.sums, hist=into.hist)
                r = ops.ensemble_verify(pred, obs, self.members, prec=prec, logw=logw, unbiased=self.unbiased, accumulate=into is not None, out=out)
            else:
                r = _composed_verify(pred, obs, prec, logw, self.members, self.unbiased)
                if into is not None:
                    r["sums"], r["hist"] = into.sums.add_(r["sums"]), into.hist.add_(r["hist"])
        return EnsembleScores(**r)

    def from_predictions(self, pred: torch.Tensor, obs: torch.Tensor, precision: Optional[torch.Tensor] = None, logw: Optional[torch.Tensor] = None,
                         into: Optional[EnsembleScores] = None) -> EnsembleScores:
        """The scores of predictions that exist already: pred float32 [B * members, K] in the sensors' given order (Decode.sensor_sse's predictions, the
        third result of SensorKalman.transform)."""
        n, K = self.members, self.sensors.K
        if not torch.is_tensor(pred) or pred.dim() != 2 or pred.dtype != torch.float32 or pred.shape[0] < 1 or pred.shape[0] % n or pred.shape[1] != K:
            raise ValueError(f"SensorVerification: pred must be a float32 [B * {n}, {K}] tensor, got "
                             f"{(tuple(pred.shape), pred.dtype) if torch.is_tensor(pred) else type(pred).__name__}")
        obs, prec, logw = self._operands(obs, precision, logw, into, pred.shape[0] // n, pred.device)
        pred = pred.detach()
        return self._verify(pred if pred.stride(1) == 1 and pred.stride(0) >= K else pred.contiguous(), obs, prec, logw, into)

    def __call__(self, y: torch.Tensor, obs: torch.Tensor, precision: Optional[torch.Tensor] = None, logw: Optional[torch.Tensor] = None,
                 into: Optional[EnsembleScores] = None) -> EnsembleScores:
        P, n = self.n_patches, self.members
        if not torch.is_tensor(y) or y.dim() != 3 or y.shape[-1] % P or y.shape[0] < 1:
            raise ValueError(f"SensorVerification: y must be [B * members, n_groups, n_patches * D] with n_patches = {P}, got "
                             f"{tuple(y.shape) if torch.is_tensor(y) else type(y).__name__}")
        Bm, G, E = y.shape
        if Bm % n:
            raise ValueError(f"SensorVerification: the {Bm} trajectories of y are not a multiple of members = {n}")
        obs, prec, logw = self._operands(obs, precision, logw, into, Bm // n, y.device)
        z = y.detach().reshape(Bm, G, P, E // P).permute(0, 2, 1, 3)          # the re-layout of SensorLikelihood
        _, pred = self.decoder.sensor_sse(z, self.sensors, obs, precision=prec, members=n, predictions=True)
        return self._verify(pred, obs, prec, logw, into)


# ------------------------------------------------------------------------------------------------ verification on dense fields
FIELD_MAPS = ("mean", "spread", "crps", "pit", "rank")
FIELD_VERIFY_FUSED_MIN_ROWS = 4096   # fused=None: the fused launches from this many decoder rows (B * members * n_patches) on — the smallest measured size


def _field_sums_property(fn):
    return property(lambda self: fn(self.sums))


@dataclasses.dataclass(frozen=True)
class FieldScores:
    """What FieldVerification returns, all on the states' device.  Per cell, [B, P, n_fields, n_inp] views: crps, pit, mean, spread (float32) and rank
    (int32: live members below the observed value; -1 a cell without weight, -2 a bad cell — a live cell whose observation, weight or a live
    member's value is not finite; its floats are NaN); None for a map that was not asked for.  Per (history, field): sums float64 [B, F, 8] and hist
    int64 [B, F, members + 1] with EnsembleScores' entries, status int32 [B].  sums and hist add up over calls (into=).  The derived properties are
    float64 [B, F] tensor expressions of sums: nothing is read back; a field without a live good cell gives NaN.  pooled() adds the fields up."""
    crps: Optional[torch.Tensor]
    pit: Optional[torch.Tensor]
    rank: Optional[torch.Tensor]
    mean: Optional[torch.Tensor]
    spread: Optional[torch.Tensor]
    sums: torch.Tensor
    hist: torch.Tensor
    status: torch.Tensor

    count = _field_sums_property(lambda s: s[..., 0])
    mean_crps = _field_sums_property(lambda s: s[..., 1] / s[..., 0])
    rmse = _field_sums_property(lambda s: (s[..., 2] / s[..., 0]).sqrt())
    mean_spread = _field_sums_property(lambda s: (s[..., 3] / s[..., 0]).sqrt())
    spread_skill = _field_sums_property(lambda s: (s[..., 3] / s[..., 2]).sqrt())
    consistency = _field_sums_property(lambda s: s[..., 4] / s[..., 0])
    bias = _field_sums_property(lambda s: s[..., 5] / s[..., 0])
    suggested_inflation = _field_sums_property(lambda s: ((s[..., 2] - s[..., 7]) / s[..., 3]).clamp_min(1.0).sqrt())

    def pooled(self) -> EnsembleScores:
        """The scores over all fields: an EnsembleScores whose sums [B, 8] and hist [B, members + 1] are this object's added over the fields (new
        tensors), with the same maps and status — its derived properties are the mesh-wide rmse, spread_skill, suggested_inflation, ..."""
        return EnsembleScores(crps=self.crps, pit=self.pit, rank=self.rank, mean=self.mean, spread=self.spread, sums=self.sums.sum(1), hist=self.hist.sum(1),
                              status=self.status)


def _field_cell_weights(shape, prec_field, prec, counts, device):
    """w f32 [B, P, F, C] of sea_decode_member_verify: valid ? max(pf, 0) * max(prec, 0) : 0, by selects (a NaN counts as 0), the product in fp32."""
    B, P, F, C_ = shape
    zero = torch.zeros((), device=device, dtype=torch.float32)
    w = torch.ones(B, P, F, C_, device=device, dtype=torch.float32)
    if prec_field is not None:
        pf = prec_field.to(torch.float32).view(1, 1, F, 1)
        w = w * torch.where(pf > 0, pf, zero)
    if prec is not None:
        pm = prec[..., :C_].to(torch.float32)
        w = w * torch.where(pm > 0, pm, zero)
    if counts is not None:
        w = torch.where((torch.arange(C_, device=device) < counts.to(device)[:, None]).view(1, P, 1, C_), w, zero)
    return torch.where(w > 0, w, zero)   # false for NaN


def _composed_field_verify(Y, obs, w, logw, members: int, unbiased: bool, maps=FIELD_MAPS, out_dtype=torch.float32):
    """sea_decode_member_verify's outputs from decoded members, with every cell a sensor of _composed_verify and every (history, field) a history of
    it: Y [B * members, P, F, C] (any float dtype, compared as given), obs [B, P, F, >= C], w [B, P, F, C] the cells' weights (0: dead), logw None or
    [B * members].  Returns a dict: the maps asked for [B, P, F, C], sums [B, F, 8], hist [B, F, members + 1], status [B].  Nothing is read back."""
    n = members
    Bm, P, F, C_ = Y.shape
    B = Bm // n
    pred = Y.reshape(B, n, P, F, C_).permute(0, 3, 1, 2, 4).reshape(B * F * n, P * C_)
    cells = lambda t: t[..., :C_].permute(0, 2, 1, 3).reshape(B * F, P * C_)   # noqa: E731
    lw = None if logw is None else logw.reshape(B, 1, n).expand(B, F, n).reshape(-1)
    r = _composed_verify(pred, cells(obs), cells(w), lw, n, unbiased, out_dtype=out_dtype)
    res = {k: r[k].view(B, F, P, C_).permute(0, 2, 1, 3).contiguous() for k in FIELD_MAPS if k in maps}
    res.update(sums=r["sums"].view(B, F, N.VERIFY_SUMS), hist=r["hist"].view(B, F, n + 1), status=r["status"].view(B, F)[:, 0].contiguous())
    return res


class FieldVerification(_FieldObserver):
    """Verification of an ensemble against a DENSE snapshot of the decoded fields — SensorVerification's scores with every cell of the mesh a reading:
    verify(y, obs, precision=None, logw=None, into=None, maps=...) -> FieldScores.  Per cell the continuous ranked probability score, the probability
    integral transform, the rank of the observed value among the members, the ensemble mean and spread (maps on the mesh: MeshUnpatcher.unpatch_spread
    for crps and spread, unpatch_map for pit and rank); per (history, field) the fp64 sums behind rmse, mean_spread, spread_skill, consistency, bias,
    mean_crps and suggested_inflation, and the rank histogram — what inflation, anomaly_gain, sigma and a taper radius of FieldKalman are tuned by.

    y, obs, layout, counts, sigma and precision mean what they mean in FieldKalman (its checks, its folding of sigma into a per-field precision): the
    weight of a cell is precision / sigma_f^2, 1 / weight is the observation-error variance that `consistency` and `suggested_inflation` use, and a
    cell without weight is neutral whatever obs holds there.  logw: None (equal weights) or [B * members] (or [B, members]) unnormalised log-weights;
    a member with -inf is dead.  unbiased=True: the fair CRPS and the N / (N - 1) spread.  maps: the per-cell outputs to produce, a subset of
    ("mean", "spread", "crps", "pit", "rank"); the others are None in the result.  into: an earlier FieldScores; this call's sums and histograms are
    added onto ITS sums and hist (in place).
    fused: True — the decoder's first layer plus the two launches of sea_decode_member_verify (include/sea_hip.h; bf16, up to 128 members): neither the
    members' decoded fields nor a prediction matrix are written; False — Decode.forward plus the formulas as fp64 torch ops with every cell a sensor
    (the composed path: fp32, more than 128 members, comparison; it holds the members' fields several times over).  fused=None takes the fused launches
    in bf16 up to 128 members from 4096 decoder rows (B * members * n_patches) on, and the composed path everywhere else — the measured rule
    (tools/field_verify_bench.py, profiles/field_verify_bench.txt; P = 64 patches, n_inp 1628, cylinder and multiphase decoder,
    every column valid and the mesh's counts, maps on and off, device time per call): 64 members, one history (4096 rows) 0.62 - 1.01 ms fused
    against 6.3 - 6.7 ms composed; 64 members, four histories (16384 rows) 1.78 - 3.20 against 23.5 - 25.1 ms; 128 members, one history (8192
    rows) 1.33 - 2.20 against 8.8 - 9.7 ms; 128 members, four histories (32768 rows) 3.90 - 7.03 against 34.8 - 37.8 ms; 6 launches against 170;
    16 - 119 MB of extra memory (9 - 95 MB without maps; the members' fp32 fields alone would be 76 - 611 MB) against 1.9 - 15.2 GB.  Nothing was
    measured below 4096 rows, so the composed path stays the default there.  (SensorVerification with every valid cell a sensor, cylinder, 64 members,
    one history: 0.87 ms at the mesh's 90 000 cells, 2.05 ms at all 312 576.)
    A call reads nothing back from the device and uploads nothing after the first call on a device.  `decoder` is a sea_amd Decode; no autograd graph
    is built."""
    _what = "FieldVerification"

    def __init__(self, decoder, n_patches: int, members: int, counts=None, layout: str = "BPFC", sigma=None, unbiased: bool = True,
                 fused: Optional[bool] = None):
        if layout not in ("BPFC", "BPCF"):
            raise ValueError(f"FieldVerification: layout must be 'BPFC' or 'BPCF', got {layout!r}")
        if not isinstance(n_patches, int) or isinstance(n_patches, bool) or n_patches < 1:
            raise ValueError(f"FieldVerification: n_patches = {n_patches!r} must be a positive integer")
        if not isinstance(members, int) or isinstance(members, bool) or members < 1:
            raise ValueError(f"FieldVerification: members = {members!r} must be a positive integer")
        if fused is not None and not isinstance(fused, bool):
            raise ValueError(f"FieldVerification: fused = {fused!r} must be None, True or False")
        if fused and members > N.FIELD_VERIFY_MAX_N:
            raise ValueError(f"FieldVerification: the fused launches carry up to {N.FIELD_VERIFY_MAX_N} members, got {members} (fused=False, or None)")
        self.decoder, self.n_patches, self.members, self.counts, self.layout, self.fused = decoder, n_patches, members, counts, layout, fused
        self.unbiased = bool(unbiased)
        self._set_sigma(sigma, sum(len(g) for g in decoder.field_groups))

    def _fused_for(self, y) -> bool:
        """Whether a call on y runs the fused launches (sea_decode_member_verify): the class docstring's rule when fused is None."""
        if self.fused is not None:
            return bool(self.fused)
        return (self.decoder._act_dtype() == torch.bfloat16 and self.members <= N.FIELD_VERIFY_MAX_N
                and y.shape[0] * self.n_patches >= FIELD_VERIFY_FUSED_MIN_ROWS)

    def __call__(self, y: torch.Tensor, obs: torch.Tensor, precision: Optional[torch.Tensor] = None, logw: Optional[torch.Tensor] = None,
                 into: Optional[FieldScores] = None, maps=FIELD_MAPS) -> FieldScores:
        y, tgt, prec = self._operands(y, obs, precision, gpu=False)
        Bm, G, E = y.shape
        P, n = self.n_patches, self.members
        B = Bm // n
        n_fields = sum(len(g) for g in self.decoder.field_groups)
        maps = tuple(maps)
        if any(k not in FIELD_MAPS for k in maps) or len(set(maps)) != len(maps):
            raise ValueError(f"FieldVerification: maps must be distinct names among {FIELD_MAPS}, got {maps!r}")
        if logw is not None:
            if not torch.is_tensor(logw) or not logw.is_floating_point() or logw.numel() != Bm or logw.dim() not in (1, 2) \
                    or (logw.dim() == 2 and logw.shape[1] != n) or logw.device != y.device:
                raise ValueError(f"FieldVerification: logw must be None or a floating-point [{Bm}] (or [{B}, {n}]) tensor of log-weights on {y.device}, got "
                                 f"{(tuple(logw.shape), str(logw.device)) if torch.is_tensor(logw) else type(logw).__name__}")
            logw = logw.detach().reshape(-1).to(torch.float32).contiguous()
        if into is not None:
            if not isinstance(into, FieldScores) or tuple(into.sums.shape) != (B, n_fields, N.VERIFY_SUMS) or tuple(into.hist.shape) != (B, n_fields, n + 1) \
                    or into.sums.device != y.device or into.sums.dtype != torch.float64 or into.hist.dtype != torch.int64 \
                    or not into.sums.is_contiguous() or not into.hist.is_contiguous():
                raise ValueError(f"FieldVerification: into must be an earlier FieldScores for {B} histories of {n} members and {n_fields} fields on {y.device}")
        N.require_gpu(y, "FieldVerification states")
        z = y.reshape(Bm, G, P, E // P).permute(0, 2, 1, 3)          # the re-layout of FieldLikelihood
        r = self.decoder.member_verify(z, tgt, n, counts=self.counts, precision=prec, field_precision=self._field_precision(y.device), logw=logw,
                                       unbiased=self.unbiased, fused=self._fused_for(y), maps=maps, into=None if into is None else dict(sums=into.sums, hist=into.hist))
        return FieldScores(**{k: r.get(k) for k in FIELD_MAPS}, sums=r["sums"], hist=r["hist"], status=r["status"])

    verify = __call__


# ------------------------------------------------------------------------------------------------ quantile and exceedance maps
QUANTILES_FUSED_MIN_ROWS = 4096   # fused=None: the fused launch from this many decoder rows (B * members * n_patches) on — the smallest measured size


def _composed_quantiles(Y, w, levels, thr):
    """sea_decode_member_quantiles' maps from decoded members, by a stable sort and cumulative weights in fp64 (include/sea_hip.h states the definitions):
    Y [B, members, P, F, C] (any float dtype, compared as given; CPU or device), w None (equal weights) or [B, members] (a member with w <= 0 or NaN
    is dead), levels a sequence of numbers in [0, 1] (rounded to float32 first, as the launch carries them), thr None or [T, F].  Returns (quant
    [Q, B, P, F, C] in Y's dtype or None, exceed float32 [T, B, P, F, C] or None).  Nothing is read back."""
    B, n, P, F, C_ = Y.shape
    dev, f64 = Y.device, torch.float64
    w64 = torch.ones(B, n, device=dev, dtype=f64) if w is None else w.detach().reshape(B, n).to(f64)
    live = w64 > 0                                                       # false for NaN
    w64 = torch.where(live, w64, torch.zeros((), device=dev, dtype=f64))
    W = w64.sum(1)
    some = (W > 0).view(1, B, 1, 1, 1)
    lv = live.view(B, n, 1, 1, 1)
    bad = (lv & ~torch.isfinite(Y)).any(1).unsqueeze(0)                  # [1, B, P, F, C]: a live member's value is not finite
    quant = exceed = None
    if len(levels):
        x = torch.where(lv, Y, torch.full((), float("inf"), device=dev, dtype=Y.dtype))   # dead members go behind every live one
        xs, idx = torch.sort(x, dim=1, stable=True)                      # the order (value, member index)
        cum = w64.view(B, n, 1, 1, 1).expand(B, n, P, F, C_).gather(1, idx).cumsum(1)
        ok_live = lv.expand(B, n, P, F, C_).gather(1, idx)
        pos_all = torch.arange(n, device=dev).view(1, n, 1, 1, 1)
        last = (live.sum(1) - 1).clamp_min(0).view(B, 1, 1, 1)
        tau = torch.tensor([float(v) for v in levels], dtype=torch.float32).to(f64).tolist()   # host floats: the float32 levels, exactly
        maps = []
        for k in range(len(levels)):
            tw = (tau[k] * W).view(B, 1, 1, 1, 1)
            pos = torch.where(ok_live & (cum >= tw), pos_all, torch.full((), n, device=dev, dtype=pos_all.dtype)).amin(1)
            pos = torch.where(pos == n, last.expand_as(pos), pos)        # nobody qualifies (rounding at tau = 1): the largest live value
            maps.append(xs.gather(1, pos.unsqueeze(1)).squeeze(1))
        quant = torch.stack(maps)
        quant = torch.where(bad, torch.full((), float("nan"), device=dev, dtype=quant.dtype), quant)
        quant = torch.where(some, quant, torch.zeros((), device=dev, dtype=quant.dtype))
    if thr is not None:
        t = thr.detach().to(dev)
        over = lv.unsqueeze(0) & (Y.unsqueeze(0) > t.to(Y.dtype).view(-1, 1, 1, 1, F, 1))
        e = torch.where(over, w64.view(1, B, n, 1, 1, 1), torch.zeros((), device=dev, dtype=f64)).sum(2) / W.clamp_min(1e-300).view(1, B, 1, 1, 1)
        e = torch.where(bad | torch.isnan(t).view(-1, 1, 1, F, 1), torch.full((), float("nan"), device=dev, dtype=f64), e)
        exceed = torch.where(some, e, torch.zeros((), device=dev, dtype=f64)).to(torch.float32)
    return quant, exceed


class EnsembleQuantiles:
    """The forecast products of an ensemble beyond mean and variance: quantiles(y, logw=None) -> (quant, exceed).  quant float32 [Q, B, P, n_fields,
    n_inp]: the weighted quantile maps of the members' decoded fields at `levels` (the median, a 5 % / 95 % band, with levels 0 and 1 the envelope) —
    each value is the decoded value of one member, so it stays in the physical range and on a mode where the mean of a bimodal cell is on neither;
    the maps are non-decreasing in the level.  exceed float32 [T, B, P, n_fields, n_inp]: the probability (the weight of the live members) that a field
    exceeds a threshold, strictly.  A product that was not asked for is None.  include/sea_hip.h (sea_decode_member_quantiles) states the definitions:
    the inverted weighted empirical distribution function — numpy's method="inverted_cdf" for equal weights, with the level rounded to float32.

    y, logw, counts and layout mean what they mean in EnsembleFields (normalised_weights: a dead member is passed over, NaN in its states reaches
    nothing; a history without a live member gets equal weights); invalid cells are exactly 0 in every map; a live cell where a live member's value
    is not finite is NaN.  levels: up to 8 numbers in [0, 1], checked here.  thresholds: None, [T] (the same for every field) or [T, n_fields], T <= 8,
    in the decoder's SCALED units (MeshUnpatcher.scale_thresholds maps physical thresholds there); numbers or a tensor.  With layout="BPCF" the maps
    are permuted views [.., B, P, n_inp, n_fields].  Quantile maps go back to the mesh with MeshUnpatcher.inverse_scale_and_unpatch(quant[k],
    layout="BPFC"), exceedance maps with unpatch_map(exceed[t]).
    fused: True — the decoder's first layer plus the ONE launch of sea_decode_member_quantiles (bf16, up to 128 members): the members' decoded fields
    are never written; False — Decode.forward plus a sort in fp64 torch ops (the composed path: fp32, more than 128 members, comparison); None —
    Decode.member_quantiles' rule: the fused launch in bf16 up to 128 members from 4096 decoder rows (B * members * n_patches) on — every measured row
    (tools/quantile_bench.py, profiles/ensemble_quantiles_bench.txt) — and the composed path everywhere else.  A call reads nothing back from the device and uploads nothing after the first call on a device.  `decoder` is a
    sea_amd Decode; no autograd graph is built."""

    def __init__(self, decoder, n_patches: int, members: int, levels=(0.05, 0.5, 0.95), thresholds=None, counts=None, layout: str = "BPFC",
                 fused: Optional[bool] = None):
        from . import ops

        if layout not in ("BPFC", "BPCF"):
            raise ValueError(f"EnsembleQuantiles: layout must be 'BPFC' or 'BPCF', got {layout!r}")
        if not isinstance(n_patches, int) or isinstance(n_patches, bool) or n_patches < 1:
            raise ValueError(f"EnsembleQuantiles: n_patches = {n_patches!r} must be a positive integer")
        if not isinstance(members, int) or isinstance(members, bool) or members < 1:
            raise ValueError(f"EnsembleQuantiles: members = {members!r} must be a positive integer")
        if fused is not None and not isinstance(fused, bool):
            raise ValueError(f"EnsembleQuantiles: fused = {fused!r} must be None, True or False")
        if fused and members > N.QUANTILE_MAX_N:
            raise ValueError(f"EnsembleQuantiles: the fused launch carries up to {N.QUANTILE_MAX_N} members, got {members} (fused=False, or None)")
        self.levels = ops.check_quantile_levels(() if levels is None else levels, "EnsembleQuantiles")
        n_fields = sum(len(g) for g in decoder.field_groups)
        self._thr_src = None
        if thresholds is not None:
            t = thresholds.detach() if torch.is_tensor(thresholds) else torch.as_tensor(thresholds, dtype=torch.float32)
            if t.dim() not in (1, 2) or not 1 <= t.shape[0] <= N.QUANTILE_MAX_LEVELS or (t.dim() == 2 and t.shape[1] != n_fields) or not t.is_floating_point():
                raise ValueError(f"EnsembleQuantiles: thresholds must be None, [T] or [T, {n_fields}] numbers with 1 <= T <= {N.QUANTILE_MAX_LEVELS}, got shape "
                                 f"{tuple(t.shape)} {t.dtype}")
            self._thr_src = (t.view(-1, 1).expand(t.shape[0], n_fields) if t.dim() == 1 else t).to(torch.float32).contiguous()
        if not self.levels and self._thr_src is None:
            raise ValueError("EnsembleQuantiles: neither levels nor thresholds: there is nothing to compute")
        self._thr = {}
        self.decoder, self.n_patches, self.members, self.counts, self.layout, self.fused = decoder, n_patches, members, counts, layout, fused

    def _thresholds_on(self, device):
        """The thresholds f32 [T, n_fields] on the device (None without): moved there once per device."""
        if self._thr_src is None:
            return None
        t = self._thr.get(device)
        if t is None:
            t = self._thr[device] = self._thr_src.to(device)
        return t

    def __call__(self, y: torch.Tensor, logw: Optional[torch.Tensor] = None, layout: Optional[str] = None):
        layout = self.layout if layout is None else layout
        if layout not in ("BPFC", "BPCF"):
            raise ValueError(f"EnsembleQuantiles: layout must be 'BPFC' or 'BPCF', got {layout!r}")
        P = self.n_patches
        if not torch.is_tensor(y) or y.dim() != 3 or y.shape[-1] % P or y.shape[0] < 1:
            raise ValueError(f"EnsembleQuantiles: y must be [B * members, n_groups, n_patches * D] with n_patches = {P}, got "
                             f"{tuple(y.shape) if torch.is_tensor(y) else type(y).__name__}")
        Bm, G, E = y.shape
        if Bm % self.members:
            raise ValueError(f"EnsembleQuantiles: the {Bm} trajectories of y are not a multiple of members = {self.members}")
        if logw is not None:
            if not torch.is_tensor(logw) or not logw.is_floating_point() or logw.numel() != Bm or logw.dim() not in (1, 2) \
                    or (logw.dim() == 2 and logw.shape[1] != self.members):
                raise ValueError(f"EnsembleQuantiles: logw must be None or a floating-point [{Bm}] (or [{Bm // self.members}, {self.members}]) tensor of log-weights, got "
                                 f"{tuple(logw.shape) if torch.is_tensor(logw) else type(logw).__name__}")
            if logw.device != y.device:
                raise ValueError(f"EnsembleQuantiles: logw is on {logw.device}, y on {y.device}")
        N.require_gpu(y, "EnsembleQuantiles states")
        z = y.detach().reshape(Bm, G, P, E // P).permute(0, 2, 1, 3)          # the re-layout of FieldLikelihood
        with torch.no_grad():
            w = None if logw is None else normalised_weights(logw, self.members)
            quant, exceed = self.decoder.member_quantiles(z, self.members, levels=self.levels, thresholds=self._thresholds_on(y.device), weights=w,
                                                          counts=self.counts, fused=self.fused)
        if layout == "BPCF":
            quant = None if quant is None else quant.permute(0, 1, 2, 4, 3)
            exceed = None if exceed is None else exceed.permute(0, 1, 2, 4, 3)
        return quant, exceed

    quantiles = __call__


# ------------------------------------------------------------------------------------------------ verification of exceedance forecasts
BRIER_MAPS = ("prob", "brier")
BRIER_FUSED_MIN_ROWS = 4096   # fused=None: the fused launches from this many decoder rows (B * members * n_patches) on — the smallest measured size


def _check_thresholds(what: str, thresholds, n_fields: int) -> torch.Tensor:
    """thresholds — numbers or a tensor, [T] (the same for every field) or [T, n_fields], 1 <= T <= 8, finite — as a contiguous float32 [T, n_fields]
    tensor on the host (a tensor given on the device comes to the host once, here)."""
    try:
        t = thresholds.detach().cpu() if torch.is_tensor(thresholds) else torch.as_tensor(thresholds, dtype=torch.float32)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{what}: thresholds must be [T] or [T, {n_fields}] numbers, got {thresholds!r}") from None
    if t.dim() not in (1, 2) or not 1 <= t.shape[0] <= N.BRIER_MAX_T or (t.dim() == 2 and t.shape[1] != n_fields) or not t.is_floating_point():
        raise ValueError(f"{what}: thresholds must be [T] or [T, {n_fields}] floating-point numbers with 1 <= T <= {N.BRIER_MAX_T}, got shape {tuple(t.shape)} {t.dtype}")
    t = (t.view(-1, 1).expand(t.shape[0], n_fields) if t.dim() == 1 else t).to(torch.float32).contiguous()
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"{what}: every threshold must be finite, got {t.tolist()}")
    return t


@dataclasses.dataclass(frozen=True)
class ThresholdScores:
    """What FieldThresholdVerification and SensorThresholdVerification return, all on the states' device.  Per reading and threshold, float32
    [T, B, P, n_fields, n_inp] (sensors: [T, B, K]) or None when not asked for: prob, the forecast probability of exceedance p, and brier_map, (p - o)^2
    with o = [reading > threshold]; 0 at a reading without weight, NaN at a bad one.  Per (history, field, threshold) — [B, F, T, ..]; sensors: per
    (history, threshold), [B, T, ..]: sums float64 [.., 5] (count of live good readings, sum (p - o)^2, sum p, sum o, count of bad readings), hist int64
    [.., members + 1] (the readings by the number m of members above the threshold) and hits (those of them where the reading was above it).  status
    int32 [B]: the live members L, or -1 (the history's log-weights are invalid: not scored).  thresholds: the float32 table the scores were made
    with.  weighted: whether a call that went into sums was given log-weights.  sums, hist and hits add up over calls (into=).
    The derived properties are float64 tensor expressions of shape [B, F, T] ([B, T] for sensors): nothing is read back; a field without a live good
    reading gives NaN.  (The per-reading map is the field brier_map, so that `brier` is the score, as in every verification suite.)"""
    prob: Optional[torch.Tensor]
    brier_map: Optional[torch.Tensor]
    sums: torch.Tensor
    hist: torch.Tensor
    hits: torch.Tensor
    status: torch.Tensor
    thresholds: torch.Tensor
    weighted: bool = False

    @property
    def count(self):
        return self.sums[..., 0]

    @property
    def brier(self):
        """The Brier score: the mean of (p - o)^2 over the live, good readings.  Defined for weighted and unweighted ensembles."""
        return self.sums[..., 1] / self.sums[..., 0]

    @property
    def base_rate(self):
        """The observed frequency of exceedance, the mean of o."""
        return self.sums[..., 3] / self.sums[..., 0]

    @property
    def mean_probability(self):
        """The mean forecast probability: above base_rate the forecasts over-predict the event."""
        return self.sums[..., 2] / self.sums[..., 0]

    @property
    def uncertainty(self):
        """base_rate (1 - base_rate): the Brier score of the constant forecast p = base_rate."""
        return self.base_rate * (1.0 - self.base_rate)

    @property
    def brier_skill(self):
        """1 - brier / uncertainty: 1 a perfect forecast, 0 no better than the base rate."""
        return 1.0 - self.brier / self.uncertainty

    def _bins(self, what: str):
        """(probability m / L, cells n_m, hits o_m) per bin as float64 [.., members + 1] — for equal weights only."""
        if self.weighted:
            raise ValueError(f"ThresholdScores.{what} is defined for equal weights only: the bins are by the NUMBER of members above the threshold, and with "
                             "unequal weights the readings of one bin carry different forecast probabilities, so a bin has no single probability to be "
                             "reliable against (brier, brier_skill and roc() are defined in every case)")
        f64 = torch.float64
        n = self.hist.shape[-1] - 1
        L = self.status.to(f64).view((-1,) + (1,) * (self.hist.dim() - 1))
        prob = torch.arange(n + 1, device=self.hist.device, dtype=f64) / L            # m / L; bins above L are empty
        return prob.expand(self.hist.shape), self.hist.to(f64), self.hits.to(f64)

    @property
    def reliability(self):
        """sum_m n_m (m / L - o_m / n_m)^2 / count over the bins m = the number of members above the threshold: 0 for a reliable forecast.  With equal
        weights brier = reliability - resolution + uncertainty exactly (Murphy 1973), since every reading of bin m was forecast p = m / L.  Raises
        ValueError on a result made with log-weights: the bins are by member count, and with unequal weights a bin has no single probability."""
        prob, n_m, o_m = self._bins("reliability")
        zero = torch.zeros((), device=n_m.device, dtype=torch.float64)
        freq = o_m / torch.where(n_m > 0, n_m, torch.ones_like(n_m))
        return torch.where(n_m > 0, n_m * (prob - freq) ** 2, zero).sum(-1) / self.count

    @property
    def resolution(self):
        """sum_m n_m (o_m / n_m - base_rate)^2 / count: how far the bins' observed frequencies lie from the base rate (larger is better).  Equal weights
        only, as reliability."""
        _, n_m, o_m = self._bins("resolution")
        zero = torch.zeros((), device=n_m.device, dtype=torch.float64)
        freq = o_m / torch.where(n_m > 0, n_m, torch.ones_like(n_m))
        return torch.where(n_m > 0, n_m * (freq - self.base_rate.unsqueeze(-1)) ** 2, zero).sum(-1) / self.count

    def reliability_curve(self):
        """The reliability diagram: (probability m / L, observed frequency o_m / n_m — NaN for an empty bin —, cells n_m), float64 [.., members + 1].
        Equal weights only, as reliability."""
        prob, n_m, o_m = self._bins("reliability_curve()")
        return prob, o_m / n_m, n_m

    def roc(self):
        """The relative operating characteristic over the decision rules "warn when at least k members exceed", k = 0 .. members + 1: (hit_rate,
        false_alarm_rate), float64 [.., members + 2], from (1, 1) at k = 0 down to (0, 0).  Defined for weighted ensembles too (the rules count members)."""
        f64 = torch.float64
        ev, ne = self.hits.to(f64), (self.hist - self.hits).to(f64)
        tail = lambda t: torch.cat([t.flip(-1).cumsum(-1).flip(-1), torch.zeros_like(t[..., :1])], dim=-1)   # noqa: E731   sum over m >= k
        return tail(ev) / ev.sum(-1, keepdim=True), tail(ne) / ne.sum(-1, keepdim=True)

    @property
    def roc_area(self):
        """The area under roc() by the trapezoid rule: 1 a perfect discrimination, 0.5 none."""
        hr, far = self.roc()
        return ((far[..., :-1] - far[..., 1:]) * (hr[..., :-1] + hr[..., 1:])).sum(-1) * 0.5


def _composed_brier(pred, obs, prec, logw, members: int, thr, out_dtype=torch.float32):
    """sea_ensemble_brier's formulas (include/sea_hip.h) as fp64 torch ops on pred's device, for any member count and on CPU tensors: pred [B * members,
    K] (any float dtype, compared as given), obs [B, K], prec None, [K] or [B, K], logw None or [B * members], thr [T, K] (or [T, B, K]: a table per
    history).  Returns a dict with ops.ensemble_brier's keys: prob, brier [T, B, K] (out_dtype), sums f64 [B, T, 5], hist, hits int64 [B, T, members +
    1], status int32 [B].  Nothing is read back."""
    f64 = torch.float64
    n = members
    B, K = obs.shape
    dev = pred.device
    zero = torch.zeros((), device=dev, dtype=f64)
    x = pred.view(B, n, K)
    y = obs
    lw = torch.zeros(B, n, device=dev, dtype=f64) if logw is None else logw.to(f64).view(B, n)
    invalid = (torch.isnan(lw) | (lw == float("inf"))).any(1) | ~torch.isfinite(lw).any(1)            # [B]
    lw = torch.where(invalid.unsqueeze(1), zero, lw)
    alive = lw != float("-inf")                                                                      # [B, N]
    e = torch.where(alive, (lw - lw.max(dim=1, keepdim=True).values).exp(), zero)
    W = e.sum(dim=1)
    p_ = torch.ones(B, K, device=dev, dtype=f64) if prec is None else prec.to(f64).expand(B, K)
    live = (p_ > 0) & ~invalid.unsqueeze(1)                                                          # [B, K]
    finite = torch.isfinite(y) & torch.isfinite(p_) & (torch.isfinite(x) | ~alive.unsqueeze(2)).all(1)
    bad, good = (live & ~finite).unsqueeze(0), (live & finite).unsqueeze(0)                          # [1, B, K]
    t = thr.detach().to(dev)
    T = t.shape[0]
    t = t.view(T, 1, K) if t.dim() == 2 else t                                                        # [T, 1 | B, K]
    over = alive.view(1, B, n, 1) & (x.unsqueeze(0) > t.to(x.dtype).unsqueeze(2))                      # [T, B, N, K]: strict, as the values they are
    m = over.sum(2)
    p = torch.where(over, e.view(1, B, n, 1), zero).sum(2) / W.view(1, B, 1)
    o = y.unsqueeze(0) > t.to(y.dtype)                                                                # [T, B, K]
    d = p - o.to(f64)
    br = d * d
    hit = good & o
    sums = torch.stack([good.expand(T, B, K).to(f64).sum(2), torch.where(good, br, zero).sum(2), torch.where(good, p, zero).sum(2), hit.to(f64).sum(2),
                        bad.expand(T, B, K).to(f64).sum(2)], dim=2).permute(1, 0, 2).contiguous()  # [B, T, 5]
    idx = torch.where(good, m, torch.zeros_like(m))
    hist = torch.zeros(T, B, n + 1, device=dev, dtype=torch.int64).scatter_add_(2, idx, good.expand(T, B, K).to(torch.int64)).permute(1, 0, 2).contiguous()
    hits = torch.zeros(T, B, n + 1, device=dev, dtype=torch.int64).scatter_add_(2, idx, hit.to(torch.int64)).permute(1, 0, 2).contiguous()
    nan = torch.full((), float("nan"), device=dev, dtype=f64)
    out = lambda v: torch.where(bad, nan, torch.where(good, v, zero)).to(out_dtype)   # noqa: E731
    status = torch.where(invalid, torch.full_like(invalid, -1, dtype=torch.int64), alive.sum(1)).to(torch.int32)
    return dict(prob=out(p), brier=out(br), sums=sums, hist=hist, hits=hits, status=status)


def _composed_field_brier(Y, obs, w, logw, members: int, thr, maps=BRIER_MAPS, out_dtype=torch.float32):
    """sea_decode_member_brier's outputs from decoded members, with every cell a sensor of _composed_brier and every (history, field) a history of it,
    mirroring _composed_field_verify: Y [B * members, P, F, C] (any float dtype, compared as given), obs [B, P, F, >= C], w [B, P, F, C] the cells'
    weights (0: dead), logw None or [B * members], thr [T, F].  Returns a dict: the maps asked for [T, B, P, F, C], sums [B, F, T, 5], hist and hits
    [B, F, T, members + 1], status [B].  Nothing is read back."""
    n = members
    Bm, P, F, C_ = Y.shape
    B = Bm // n
    T = thr.shape[0]
    pred = Y.reshape(B, n, P, F, C_).permute(0, 3, 1, 2, 4).reshape(B * F * n, P * C_)
    cells = lambda t: t[..., :C_].permute(0, 2, 1, 3).reshape(B * F, P * C_)   # noqa: E731
    lw = None if logw is None else logw.reshape(B, 1, n).expand(B, F, n).reshape(-1)
    tk = thr.to(Y.device).view(T, 1, F, 1).expand(T, B, F, P * C_).reshape(T, B * F, P * C_)
    r = _composed_brier(pred, cells(obs), cells(w), lw, n, tk, out_dtype=out_dtype)
    res = {k: r[k].view(T, B, F, P, C_).permute(0, 1, 3, 2, 4).contiguous() for k in BRIER_MAPS if k in maps}
    res.update(sums=r["sums"].view(B, F, T, N.BRIER_SUMS), hist=r["hist"].view(B, F, T, n + 1), hits=r["hits"].view(B, F, T, n + 1),
               status=r["status"].view(B, F)[:, 0].contiguous())
    return res


def _check_brier_call(what: str, maps, logw, into, shape, Bm: int, n: int, device):
    """maps, logw and into of a threshold-verification call, checked; returns (maps, logw as a contiguous float32 [Bm] or None)."""
    maps = tuple(maps)
    if any(k not in BRIER_MAPS for k in maps) or len(set(maps)) != len(maps):
        raise ValueError(f"{what}: maps must be distinct names among {BRIER_MAPS}, got {maps!r}")
    if logw is not None:
        if not torch.is_tensor(logw) or not logw.is_floating_point() or logw.numel() != Bm or logw.dim() not in (1, 2) \
                or (logw.dim() == 2 and logw.shape[1] != n) or logw.device != device:
            raise ValueError(f"{what}: logw must be None or a floating-point [{Bm}] (or [{Bm // n}, {n}]) tensor of log-weights on {device}, got "
                             f"{(tuple(logw.shape), str(logw.device)) if torch.is_tensor(logw) else type(logw).__name__}")
        logw = logw.detach().reshape(-1).to(torch.float32).contiguous()
    if into is not None:
        if not isinstance(into, ThresholdScores) or tuple(into.sums.shape) != shape + (N.BRIER_SUMS,) or tuple(into.hist.shape) != shape + (n + 1,) \
                or tuple(into.hits.shape) != shape + (n + 1,) or into.sums.device != device or into.sums.dtype != torch.float64 \
                or into.hist.dtype != torch.int64 or into.hits.dtype != torch.int64 or not into.sums.is_contiguous() or not into.hist.is_contiguous() \
                or not into.hits.is_contiguous():
            raise ValueError(f"{what}: into must be an earlier ThresholdScores with sums {list(shape + (N.BRIER_SUMS,))} for {n} members on {device}")
    return maps, logw


class FieldThresholdVerification(_FieldObserver):
    """Verification of EXCEEDANCE forecasts against a dense snapshot of the decoded fields — are EnsembleQuantiles' probability maps any good:
    verify(y, obs, precision=None, logw=None, into=None, maps=()) -> ThresholdScores.  Per (history, field, threshold) the Brier score with its
    reliability / resolution / uncertainty decomposition, the reliability diagram (is 0.8 observed 80 % of the time?) and the ROC curve, from fp64 sums
    and integer histograms that add up over calls (into=: an earlier result whose sums, hist and hits this call's are added onto, in place); per cell,
    when asked for (maps: a subset of ("prob", "brier")), the forecast probability and (p - o)^2 (MeshUnpatcher.unpatch_map takes them to the mesh).
    include/sea_hip.h (sea_decode_member_brier) states the definitions; exceedance is strict, of the forecast and of the observation.

    thresholds: [T] (the same for every field) or [T, n_fields], T <= 8, finite, in the decoder's SCALED units as in EnsembleQuantiles
    (MeshUnpatcher.scale_thresholds maps physical thresholds there); checked here.  y, obs, layout, counts, precision and logw are checked exactly as
    FieldVerification checks them; the precision only decides which cells are read (a cell with precision 0, or beyond counts, is neutral whatever obs
    holds there): no score is weighted by it.
    fused: True — the decoder's first layer plus the two launches of sea_decode_member_brier (bf16, up to 128 members): the thresholds-only decode of
    sea_decode_member_quantiles plus one comparison with the observation; the members' decoded fields are never written.  False — Decode.forward plus
    the formulas as fp64 torch ops (the composed path: fp32, more than 128 members, comparison; it holds the members' fields and a boolean and an fp64
    temporary per threshold).  fused=None takes the fused launches in bf16 up to 128 members from 4096 decoder rows (B * members * n_patches) on and the
    composed path everywhere else — the measured rule (tools/brier_bench.py, profiles/brier_bench.txt, DESIGN.md section 7o: every measured row, 4096 -
    32768 rows, has the fused launches ahead); nothing was measured below 4096 rows, so the composed path stays the default there.
    A call reads nothing back from the device and uploads nothing after the first call on a device.  `decoder` is a sea_amd Decode; no autograd graph
    is built."""
    _what = "FieldThresholdVerification"

    def __init__(self, decoder, n_patches: int, members: int, thresholds, counts=None, layout: str = "BPFC", fused: Optional[bool] = None):
        what = self._what
        if layout not in ("BPFC", "BPCF"):
            raise ValueError(f"{what}: layout must be 'BPFC' or 'BPCF', got {layout!r}")
        if not isinstance(n_patches, int) or isinstance(n_patches, bool) or n_patches < 1:
            raise ValueError(f"{what}: n_patches = {n_patches!r} must be a positive integer")
        if not isinstance(members, int) or isinstance(members, bool) or members < 1:
            raise ValueError(f"{what}: members = {members!r} must be a positive integer")
        if fused is not None and not isinstance(fused, bool):
            raise ValueError(f"{what}: fused = {fused!r} must be None, True or False")
        if fused and members > N.BRIER_MAX_N:
            raise ValueError(f"{what}: the fused launches carry up to {N.BRIER_MAX_N} members, got {members} (fused=False, or None)")
        n_fields = sum(len(g) for g in decoder.field_groups)
        self.thresholds = _check_thresholds(what, thresholds, n_fields)
        self._thr = {}
        self.decoder, self.n_patches, self.members, self.counts, self.layout, self.fused = decoder, n_patches, members, counts, layout, fused
        self._set_sigma(None, n_fields)

    def _thresholds_on(self, device):
        """The thresholds f32 [T, n_fields] on the device: moved there once per device."""
        t = self._thr.get(device)
        if t is None:
            t = self._thr[device] = self.thresholds.to(device)
        return t

    def _fused_for(self, y) -> bool:
        """Whether a call on y runs the fused launches (sea_decode_member_brier): the class docstring's rule when fused is None."""
        if self.fused is not None:
            return bool(self.fused)
        return (self.decoder._act_dtype() == torch.bfloat16 and self.members <= N.BRIER_MAX_N
                and y.shape[0] * self.n_patches >= BRIER_FUSED_MIN_ROWS)

    def __call__(self, y: torch.Tensor, obs: torch.Tensor, precision: Optional[torch.Tensor] = None, logw: Optional[torch.Tensor] = None,
                 into: Optional[ThresholdScores] = None, maps=()) -> ThresholdScores:
        y, tgt, prec = self._operands(y, obs, precision, gpu=False)
        Bm, G, E = y.shape
        P, n = self.n_patches, self.members
        B = Bm // n
        n_fields, T = self.thresholds.shape[1], self.thresholds.shape[0]
        maps, logw = _check_brier_call(self._what, maps, logw, into, (B, n_fields, T), Bm, n, y.device)
        N.require_gpu(y, f"{self._what} states")
        thr = self._thresholds_on(y.device)
        z = y.reshape(Bm, G, P, E // P).permute(0, 2, 1, 3)          # the re-layout of FieldLikelihood
        r = self.decoder.member_brier(z, tgt, n, thr, counts=self.counts, precision=prec, logw=logw, fused=self._fused_for(y), maps=maps,
                                      into=None if into is None else dict(sums=into.sums, hist=into.hist, hits=into.hits))
        return ThresholdScores(prob=r.get("prob"), brier_map=r.get("brier"), sums=r["sums"], hist=r["hist"], hits=r["hits"], status=r["status"], thresholds=thr,
                               weighted=logw is not None or (into is not None and into.weighted))

    verify = __call__


class SensorThresholdVerification:
    """Verification of EXCEEDANCE forecasts against sparse sensor readings: verify(y, obs, precision=None, logw=None, into=None, maps=()) ->
    ThresholdScores with [B, T] scores — FieldThresholdVerification's with a sensor for a cell (include/sea_hip.h, sea_ensemble_brier).
    thresholds: [T] or [T, n_fields] in the decoder's scaled units, T <= 8, finite; a sensor takes the threshold of its field (the set's field index), so
    the launch carries a [T, K] table.  y, obs, precision and logw exactly as in SensorVerification (precision 0 marks a missing reading; no score is
    weighted by it).  The predictions come from Decode.sensor_sse(..., predictions=True); from_predictions(pred, obs, ...) skips the decode — the pred
    that SensorKalman.transform returned is scored without decoding twice — and serves CPU tensors through the composed path.
    fused: True — the two launches of sea_ensemble_brier (up to 128 members, GPU tensors); False — the same formulas as fp64 torch ops.  fused=None
    follows SensorVerification's rule, which this form's bench confirms (tools/brier_bench.py, profiles/brier_bench.txt): the two
    launches up to 128 members on the GPU — every measured row, 16 to 4096 sensors, has them ahead of the composed path —, the composed path above 128
    members and on the CPU.  A call reads nothing back from the device and uploads nothing after the first call on a device."""

    def __init__(self, decoder, n_patches: int, members: int, sensors: SensorSet, thresholds, fused: Optional[bool] = None):
        what = "SensorThresholdVerification"
        if not isinstance(members, int) or isinstance(members, bool) or members < 1:
            raise ValueError(f"{what}: members = {members!r} must be a positive integer")
        if fused is not None and not isinstance(fused, bool):
            raise ValueError(f"{what}: fused = {fused!r} must be None, True or False")
        if fused and members > N.BRIER_MAX_N:
            raise ValueError(f"{what}: the fused launches carry up to {N.BRIER_MAX_N} members, got {members} (fused=False, or None)")
        self._like = SensorLikelihood(decoder, n_patches, members, sensors)   # its checks
        n_fields = sum(len(g) for g in decoder.field_groups)
        if isinstance(sensors, DerivedSensorSet):   # a derived reading has no field of its own: [T] (every reading) or [T, K] (one column per reading)
            self.thresholds = _check_thresholds(what, thresholds, sensors.K)
        else:
            tf = _check_thresholds(what, thresholds, n_fields)
            self.thresholds = tf[:, torch.as_tensor(list(sensors.out_field), dtype=torch.long)].contiguous()   # [T, K] through the set's field index
        self._thr = {}
        self.decoder, self.n_patches, self.members, self.sensors, self.fused = decoder, n_patches, members, sensors, fused

    def _thresholds_on(self, device):
        t = self._thr.get(device)
        if t is None:
            t = self._thr[device] = self.thresholds.to(device)
        return t

    def _fused_for(self, device) -> bool:
        if self.fused is not None:
            return bool(self.fused)
        return self.members <= N.BRIER_MAX_N and device.type == "cuda"

    def _score(self, pred, obs, precision, logw, into, maps) -> ThresholdScores:
        what = "SensorThresholdVerification"
        n, K, T = self.members, self.sensors.K, self.thresholds.shape[0]
        B, dev = pred.shape[0] // n, pred.device
        _check_sensor_operands(what, obs, precision, B, K, dev)
        maps, logw = _check_brier_call(what, maps, logw, into, (B, T), B * n, n, dev)
        obs, prec = obs.detach(), None if precision is None else precision.detach()
        thr = self._thresholds_on(dev)
        with torch.no_grad():
            if self._fused_for(dev):
                out = None if into is None else dict(sums=into.sums, hist=into.hist, hits=into.hits)
                r = ops.ensemble_brier(pred, obs, n, thr, prec=prec, logw=logw, accumulate=into is not None, maps=maps, out=out)
            else:
                r = _composed_brier(pred, obs, prec, logw, n, thr)
                if into is not None:
                    r["sums"], r["hist"], r["hits"] = into.sums.add_(r["sums"]), into.hist.add_(r["hist"]), into.hits.add_(r["hits"])
        return ThresholdScores(prob=r.get("prob") if "prob" in maps else None, brier_map=r.get("brier") if "brier" in maps else None, sums=r["sums"],
                               hist=r["hist"], hits=r["hits"], status=r["status"], thresholds=thr, weighted=logw is not None or (into is not None and into.weighted))

    def from_predictions(self, pred: torch.Tensor, obs: torch.Tensor, precision: Optional[torch.Tensor] = None, logw: Optional[torch.Tensor] = None,
                         into: Optional[ThresholdScores] = None, maps=()) -> ThresholdScores:
        """The scores of predictions that exist already: pred float32 [B * members, K] in the sensors' given order (Decode.sensor_sse's predictions, the
        third result of SensorKalman.transform).  CPU tensors are served by the composed path."""
        n, K = self.members, self.sensors.K
        if not torch.is_tensor(pred) or pred.dim() != 2 or pred.dtype != torch.float32 or pred.shape[0] < 1 or pred.shape[0] % n or pred.shape[1] != K:
            raise ValueError(f"SensorThresholdVerification: pred must be a float32 [B * {n}, {K}] tensor, got "
                             f"{(tuple(pred.shape), pred.dtype) if torch.is_tensor(pred) else type(pred).__name__}")
        pred = pred.detach()
        return self._score(pred if pred.stride(1) == 1 and pred.stride(0) >= K else pred.contiguous(), obs, precision, logw, into, maps)

    def __call__(self, y: torch.Tensor, obs: torch.Tensor, precision: Optional[torch.Tensor] = None, logw: Optional[torch.Tensor] = None,
                 into: Optional[ThresholdScores] = None, maps=()) -> ThresholdScores:
        P, n = self.n_patches, self.members
        if not torch.is_tensor(y) or y.dim() != 3 or y.shape[-1] % P or y.shape[0] < 1:
            raise ValueError(f"SensorThresholdVerification: y must be [B * members, n_groups, n_patches * D] with n_patches = {P}, got "
                             f"{tuple(y.shape) if torch.is_tensor(y) else type(y).__name__}")
        Bm, G, E = y.shape
        if Bm % n:
            raise ValueError(f"SensorThresholdVerification: the {Bm} trajectories of y are not a multiple of members = {n}")
        _check_sensor_operands("SensorThresholdVerification", obs, precision, Bm // n, self.sensors.K, y.device)
        _check_brier_call("SensorThresholdVerification", maps, logw, into, (Bm // n, self.thresholds.shape[0]), Bm, n, y.device)
        z = y.detach().reshape(Bm, G, P, E // P).permute(0, 2, 1, 3)          # the re-layout of SensorLikelihood
        _, pred = self.decoder.sensor_sse(z, self.sensors, obs.detach(), precision=None if precision is None else precision.detach(), members=n, predictions=True)
        return self._score(pred, obs, precision, logw, into, maps)

    verify = __call__


# ------------------------------------------------------------------------------------------------ CRPS of the decoded fields as a loss
def _composed_crps(Y, obs, w, logw, members: int, unbiased: bool, field_weight=None):
    """sea_decode_member_crps_grad's formulas (include/sea_hip.h) as fp64 torch ops on _composed_verify's conventions: Y [B * members, P, F, C] decoded
    members (any float dtype, compared as given), obs [B, P, F, >= C], w [B, P, F, C] the cells' weights (0: dead), logw None or [B * members],
    field_weight None or [F].  Returns (loss f32 [B, F] = fw * the sum of the live, good cells' CRPS, count f64 [B, F], G f64 [B * members, P, F, C] =
    d sum_f loss / d Y, coded explicitly: fw w_m (sign(x_m - y) - (2 below_m + w_m - 1) / c) with below_m from a STABLE sort, which is the order
    (value, member index) — not torch.abs's subgradient; exactly 0 for a dead member, a dead or bad cell, an unscored history).  Nothing is read back."""
    f64 = torch.float64
    n = members
    Bm, P, F, C_ = Y.shape
    B = Bm // n
    dev = Y.device
    zero = torch.zeros((), device=dev, dtype=f64)
    x = Y.detach().to(f64).view(B, n, P, F, C_)
    y = obs[..., :C_].to(f64)
    lw = torch.zeros(B, n, device=dev, dtype=f64) if logw is None else logw.to(f64).view(B, n)
    invalid = (torch.isnan(lw) | (lw == float("inf"))).any(1) | ~torch.isfinite(lw).any(1)            # [B]
    lw = torch.where(invalid.unsqueeze(1), zero, lw)
    alive = lw != float("-inf")                                                                      # [B, n]
    e = torch.where(alive, (lw - lw.max(dim=1, keepdim=True).values).exp(), zero)
    wm = e / e.sum(dim=1, keepdim=True)
    c = (1.0 - (wm * wm).sum(dim=1) if unbiased else torch.ones(B, device=dev, dtype=f64)).view(B, 1, 1, 1)
    pos = c > 0
    c_safe = torch.where(pos, c, torch.ones_like(c))
    p = w.to(f64)
    al = alive.view(B, n, 1, 1, 1)
    live = (p > 0) & ~invalid.view(B, 1, 1, 1)
    finite = torch.isfinite(y) & torch.isfinite(p) & (torch.isfinite(x) | ~al).all(1)
    good = live & finite                                                                             # [B, P, F, C]
    use = good.unsqueeze(1) & al                                                                     # [B, n, P, F, C]: what enters a sum
    xs = torch.where(use, x, zero)
    ys = torch.where(good, y, zero)
    wv = torch.where(use, wm.view(B, n, 1, 1, 1), zero)
    d = xs - ys.unsqueeze(1)
    order = torch.sort(xs, dim=1, stable=True).indices                                                # ties keep the member order
    ws, ds = torch.gather(wv, 1, order), torch.gather(d, 1, order)
    below_sorted = ws.cumsum(1) - ws
    pair = (ws * ds * (2.0 * below_sorted + ws - 1.0)).sum(1)
    crps = (wv * d.abs()).sum(1) - torch.where(pos, pair / c_safe, zero)
    below = torch.zeros_like(below_sorted).scatter_(1, order, below_sorted)
    G = wv * (torch.sign(d) - torch.where(pos.unsqueeze(1), (2.0 * below + wv - 1.0) / c_safe.unsqueeze(1), zero))
    G = torch.where(use, G, zero)
    sums1 = torch.where(good, crps, zero).sum(dim=(1, 3))                                             # [B, F]
    count = good.to(f64).sum(dim=(1, 3))
    if field_weight is not None:
        fw = field_weight.to(device=dev, dtype=f64)
        fw = torch.where(fw > 0, fw, zero)
        sums1, G = fw.view(1, F) * sums1, G * fw.view(1, 1, 1, F, 1)
    return sums1.to(torch.float32), count, G.view(Bm, P, F, C_)


class _CrpsComposedFn(torch.autograd.Function):
    """_composed_crps behind autograd: (loss [B, F], count [B, F]) from the decoded members Y; the backward multiplies the saved explicit gradient by the
    upstream factor of its (history, field) — exact for any upstream gradient."""

    @staticmethod
    def forward(ctx, Y, obs, w, logw, members, unbiased, field_weight):
        loss, count, G = _composed_crps(Y, obs, w, logw, members, unbiased, field_weight)
        ctx.members = members
        ctx.save_for_backward(G.to(Y.dtype))
        ctx.mark_non_differentiable(count)
        return loss, count

    @staticmethod
    def backward(ctx, g, _unused):
        (G,) = ctx.saved_tensors
        Bm, P, F, C_ = G.shape
        n = ctx.members
        gy = G.view(Bm // n, n, P, F, C_) * g.to(G.dtype).view(Bm // n, 1, 1, F, 1)
        return gy.view(Bm, P, F, C_), None, None, None, None, None, None


class EnsembleCRPSLoss(torch.nn.Module):
    """The CRPS of the DECODED fields of an ensemble as a training loss: loss = EnsembleCRPSLoss(decoder, n_patches, members)(out, target_fields).

    out: the temporal model's output [B * members, T, n_groups, P * D] in fork order (row b * members + j is member j of history b — members that differ
    by perturbed conditions, noisy inputs or dropout); target_fields: float32 [B, T, P, n_fields, C] (layout "BPFC"; C >= the decoder's n_inp) or, with
    layout="BPCF", [B, T, P, C, n_fields]: ONE truth per (b, t).  precision: None or a float32 map of target_fields' shape (0: a missing cell);
    logw: None (equal weights) or float32 [B * members] log-weights of the members, constants.  The latent -> z re-layout of
    inverse_transform_processed_data is applied as torch views and permutes with (b, t) as the history and j as the member, so autograd carries the
    gradient back to the temporal model's hand-written backward; the loss itself is Decode.member_crps_loss (fused: sea_decode_member_crps_grad — neither
    the members' decoded fields nor their gradient are written).  Returns the 0-dim tensor sum(loss) / max(sum(count), 1) — the mean CRPS per live
    cell (the fair CRPS with unbiased=True; field_weight scales a field's share) — on the device; nothing is read back.  `decoder` is a frozen sea_amd
    Decode (decoder.requires_grad_(False)); it is not registered as a sub-module, so the loss has no parameters."""

    def __init__(self, decoder, n_patches: int, members: int, counts=None, layout: str = "BPFC", unbiased: bool = True, field_weight=None, fused=None,
                 pack=None):
        super().__init__()
        if layout not in ("BPFC", "BPCF"):
            raise ValueError(f"EnsembleCRPSLoss: layout must be 'BPFC' or 'BPCF', got {layout!r}")
        if not isinstance(n_patches, int) or isinstance(n_patches, bool) or n_patches < 1:
            raise ValueError(f"EnsembleCRPSLoss: n_patches = {n_patches!r} must be a positive integer")
        if not isinstance(members, int) or isinstance(members, bool) or members < 1:
            raise ValueError(f"EnsembleCRPSLoss: members = {members!r} must be a positive integer")
        n_fields = sum(len(g) for g in decoder.field_groups)
        if field_weight is not None:
            field_weight = torch.as_tensor(field_weight, dtype=torch.float32)
            if tuple(field_weight.shape) != (n_fields,) or not bool(torch.isfinite(field_weight).all()) or bool((field_weight < 0).any()):
                raise ValueError(f"EnsembleCRPSLoss: field_weight must be {n_fields} finite numbers >= 0, got {field_weight.tolist()}")
        object.__setattr__(self, "decoder", decoder)
        self.n_patches, self.members, self.counts, self.layout, self.unbiased, self.fused = n_patches, members, counts, layout, bool(unbiased), fused
        self.pack = pack   # Decode.member_crps_loss's pack: None (its rule), True (the packed form, 1 .. 32 members) or False
        self._fw_src, self._fw = field_weight, {}

    def _field_weight_on(self, device):
        if self._fw_src is None:
            return None
        t = self._fw.get(device)
        if t is None:
            t = self._fw[device] = self._fw_src.to(device)
            t._sea_checked_field_weight = True   # checked on the host at construction: Decode.member_crps_loss does not read it back
        return t

    def forward(self, output: torch.Tensor, target_fields: torch.Tensor, precision: Optional[torch.Tensor] = None, logw: Optional[torch.Tensor] = None,
                layout: Optional[str] = None) -> torch.Tensor:
        layout = self.layout if layout is None else layout
        if layout not in ("BPFC", "BPCF"):
            raise ValueError(f"EnsembleCRPSLoss: layout must be 'BPFC' or 'BPCF', got {layout!r}")
        P, n = self.n_patches, self.members
        if not torch.is_tensor(output) or output.dim() != 4 or output.shape[-1] % P or output.shape[0] < 1:
            raise ValueError(f"EnsembleCRPSLoss: output must be [B * members, T, n_groups, n_patches * D] with n_patches = {P}, got "
                             f"{tuple(output.shape) if torch.is_tensor(output) else type(output).__name__}")
        Bm, T, G, E = output.shape
        if Bm % n:
            raise ValueError(f"EnsembleCRPSLoss: the {Bm} trajectories of output are not a multiple of members = {n}")
        B = Bm // n
        for name, t in (("target_fields", target_fields), ("precision", precision)):
            if t is None and name == "precision":
                continue
            if not torch.is_tensor(t) or t.dim() != 5 or tuple(t.shape[:3]) != (B, T, P):
                raise ValueError(f"EnsembleCRPSLoss: {name} must be [{B}, {T}, {P}, ...] in layout {layout} (one truth per history and step), got "
                                 f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
        if precision is not None and precision.shape != target_fields.shape:
            raise ValueError(f"EnsembleCRPSLoss: precision must have target_fields' shape {tuple(target_fields.shape)}, got {tuple(precision.shape)}")
        if logw is not None and (not torch.is_tensor(logw) or logw.dtype != torch.float32 or tuple(logw.shape) != (Bm,) or logw.device != output.device):
            raise ValueError(f"EnsembleCRPSLoss: logw must be None or a float32 [{Bm}] tensor on {output.device}, got "
                             f"{(tuple(logw.shape), logw.dtype, str(logw.device)) if torch.is_tensor(logw) else type(logw).__name__}")
        D = E // P
        # [B, n, T, G, P, D] -> [B, T, n, P, G, D]: the history is (b, t), the member j
        z = output.reshape(B, n, T, G, P, D).permute(0, 2, 1, 4, 3, 5).reshape(B * T * n, P, G, D)
        rel = (lambda t: t) if layout == "BPFC" else (lambda t: t.permute(0, 1, 2, 4, 3))   # noqa: E731
        tgt = rel(target_fields)
        tgt = tgt.reshape((B * T,) + tuple(tgt.shape[2:]))
        prec = None
        if precision is not None:
            prec = rel(precision)
            prec = prec.reshape((B * T,) + tuple(prec.shape[2:]))
        lw = None if logw is None else logw.detach().view(B, 1, n).expand(B, T, n).reshape(-1)
        kw = {} if self.pack is None else {"pack": self.pack}   # None: the decoder's own rule, whatever decoder this is
        loss, count = self.decoder.member_crps_loss(z, tgt, n, counts=self.counts, precision=prec, field_weight=self._field_weight_on(output.device), logw=lw,
                                                    unbiased=self.unbiased, fused=self.fused, **kw)
        return loss.sum() / count.sum().clamp_min(1.0).to(loss.dtype)


# ------------------------------------------------------------------------------------------------ derived fields: |u|, energy, differences
DERIVED_OPS = ("magnitude", "energy", "difference")
DERIVED_FUSED_MIN_ROWS = 4096   # fused=None: the fused launches from this many decoder rows (B * members * n_patches) on — the smallest measured size


class DerivedField:
    """A derived field of two decoded fields, formed per member and cell in float32 with every operation rounded once (include/sea_hip.h,
    sea_decode_derived_quantiles):  a' = y_a * scale_a + shift_a,  b' = y_b * scale_b + shift_b,  then
        "magnitude"   sqrt(a' a' + b' b')       the speed |u| of two velocity components (a correctly rounded root)
        "energy"      0.5 (a' a' + b' b')
        "difference"  a' - b'
    a != b index the decoder's fields in output order; scale and shift carry the mesh's inverse scaling so that the value is in PHYSICAL units
    (MeshUnpatcher.derived_fields builds them: a magnitude of min-max-scaled components means nothing).  Immutable; validated here, on the host."""
    __slots__ = ("op", "a", "b", "scale_a", "shift_a", "scale_b", "shift_b", "name")

    def __init__(self, op: str, a: int, b: int, scale_a: float = 1.0, shift_a: float = 0.0, scale_b: float = 1.0, shift_b: float = 0.0, name: Optional[str] = None):
        if op not in DERIVED_OPS:
            raise ValueError(f"DerivedField: op must be one of {DERIVED_OPS}, got {op!r}")
        for k, v in (("a", a), ("b", b)):
            if not isinstance(v, int) or isinstance(v, bool) or v < 0:
                raise ValueError(f"DerivedField: {k} = {v!r} must be a field index >= 0")
        if a == b:
            raise ValueError(f"DerivedField: a == b = {a}: two different source fields are needed")
        coeff = []
        for k, v in (("scale_a", scale_a), ("shift_a", shift_a), ("scale_b", scale_b), ("shift_b", shift_b)):
            try:
                v = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"DerivedField: {k} = {v!r} must be a number") from None
            v32 = float(torch.tensor(v, dtype=torch.float32))   # the float32 the launch carries
            if not math.isfinite(v32):
                raise ValueError(f"DerivedField: {k} = {v!r} must be finite in float32")
            coeff.append(v32)
        for k, v in zip(self.__slots__, (op, a, b, *coeff, f"{op}({a},{b})" if name is None else str(name))):
            object.__setattr__(self, k, v)

    def __setattr__(self, k, v):
        raise AttributeError("DerivedField is immutable")

    def __repr__(self):
        return (f"DerivedField({self.op!r}, {self.a}, {self.b}, scale_a={self.scale_a}, shift_a={self.shift_a}, scale_b={self.scale_b}, shift_b={self.shift_b}, "
                f"name={self.name!r})")

    def _key(self):
        return tuple(getattr(self, k) for k in self.__slots__)

    def __eq__(self, other):
        return isinstance(other, DerivedField) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())


def _check_derived(what: str, derived, n_fields: int) -> tuple:
    """derived as a tuple of DerivedField whose sources lie in 0 .. n_fields - 1 (ValueError otherwise)."""
    try:
        derived = tuple(derived)
    except TypeError:
        raise ValueError(f"{what}: derived must be a sequence of DerivedField, got {type(derived).__name__}") from None
    if not derived or any(not isinstance(d, DerivedField) for d in derived):
        raise ValueError(f"{what}: derived must be a non-empty sequence of DerivedField, got {derived!r}")
    for i, d in enumerate(derived):
        if d.a >= n_fields or d.b >= n_fields:
            raise ValueError(f"{what}: derived field {i} ({d.name}): sources a = {d.a}, b = {d.b} outside the {n_fields} fields")
    return derived


def _composed_derived(Y, derived):
    """The derived fields of decoded members as separate float32 torch ops in the stated order — the composed path and the restatement's front end
    (include/sea_hip.h, sea_decode_derived_quantiles): Y [..., F, C] (members' decoded fields [B, members, P, F, C], or an observation [B, P, F, C];
    any float dtype, converted to float32 first; CPU or device) -> float32 [..., n_derived, C].  Every product and sum is ONE float32 torch op: nothing
    is fused and nothing reassociated.  The root is the float64 root rounded once to float32 — the correctly rounded float32 root (a float64 root is
    never close enough to the middle of two float32 values for the second rounding to matter); torch.sqrt on float32 tensors is NOT always that (its
    CPU form differs from numpy's float32 root by one unit in the last place in about 0.7 % of random arguments)."""
    y = Y.to(torch.float32)
    out = []
    for d in derived:
        a = y.select(-2, d.a) * d.scale_a + d.shift_a      # python floats that are float32 values: one multiply, one add
        b = y.select(-2, d.b) * d.scale_b + d.shift_b
        if d.op == "difference":
            out.append(a - b)
            continue
        q = a * a + b * b
        out.append(q * 0.5 if d.op == "energy" else torch.sqrt(q.to(torch.float64)).to(torch.float32))
    return torch.stack(out, dim=-2)


def _composed_derived_readings(ya, yb, op, sa, ha, sb, hb):
    """_composed_derived's float32 arithmetic per READING: ya, yb float32 [..., K], the decoded values of the two sources; op int64 [K] (-1 plain, else
    the index into DERIVED_OPS); sa, ha, sb, hb float32 [K].  One torch op per product and sum, the float64 root rounded once.  Differentiable: the root
    is taken of 1 where the sum of squares is 0 and the value selected to 0 there, so the gradient at a zero speed is exactly 0, as on the fused path."""
    a = ya * sa + ha
    b = yb * sb + hb
    q = a * a + b * b
    pos = q > 0
    root = torch.sqrt(torch.where(pos, q, torch.ones_like(q)).to(torch.float64)).to(torch.float32)
    mag = torch.where(pos, root, q)          # q == 0: the root of 0 (NaN stays NaN: q > 0 is false and q itself is returned)
    x = torch.where(op == 2, a - b, torch.where(op == 1, q * 0.5, mag))
    return torch.where(op < 0, ya, x)


class DerivedSensorSet(SensorSet):
    """K >= 1 point sensors of which some read a DERIVED quantity — a speed (hot-wire, Pitot tube, cup anemometer), an energy, a difference of two
    fields (a differential tap) — at cell cell[k] of patch patch[k].  reading[k] is a field id (a plain sensor, exactly as in SensorSet: scaled units;
    scale_values / scale_sigma apply to it) or a DerivedField (its a, b index the decoder's fields in output order; the reading is in the PHYSICAL
    units of the derived quantity, and scale_values / scale_sigma pass it through).  Every consumer of a SensorSet takes this set with the same calls.
    The launch tables of sea_decode_derived_sensor_sse (include/sea_hip.h) are built here, once, and uploaded once per device.  A reading occupies TWO
    adjacent entries of the sorted, padded list — entry 2 i the W2 row of source a, entry 2 i + 1 that of source b (a plain reading: its field, and row
    0) — so a (group, patch) segment of n readings takes 2 n entries padded to a multiple of 32:
      perm    int32 [K_pad]: sorted entry -> reading (both entries of a pair; pad entries point at reading 0)
      wrow    int32 [K_pad]: the rows of the group's second-layer weights
      live    int32 [K_pad]: 1 at the first entry of a reading's pair, 0 elsewhere
      op      int32 [K_pad]: -1 (plain) or the op code at the first entry of a pair; scale, shift float32 [K_pad]: (scale_a, shift_a) at 2 i, (scale_b,
              shift_b) at 2 i + 1 (1, 0 elsewhere)
      seg, Q, patches as in SensorSet; inv int64 [K]: reading -> the sorted position of its first entry
    A derived reading whose sources lie in different decoder groups cannot be paired inside one segment: the set accepts it, `fusable` is False, no
    launch tables exist (K_pad is None) and only the composed path serves it (fused=True raises, fused=None takes the composed path)."""

    def __init__(self, decoder, n_patches: int, patch, cell, reading, affine=None, points=None):
        what = "DerivedSensorSet"
        if not isinstance(n_patches, int) or isinstance(n_patches, bool) or n_patches < 1:
            raise ValueError(f"{what}: n_patches = {n_patches!r} must be a positive integer")
        patch, cell = _int_list(patch, "patch", what), _int_list(cell, "cell", what)
        if torch.is_tensor(reading):
            reading = _int_list(reading, "reading", what)
        try:
            reading = list(reading)
        except TypeError:
            raise ValueError(f"{what}: reading must be a sequence of field ids and DerivedField, got {type(reading).__name__}") from None
        K = len(patch)
        if len(cell) != K or len(reading) != K:
            raise ValueError(f"{what}: patch, cell and reading must have equal lengths, got {K}, {len(cell)}, {len(reading)}")
        groups = tuple(tuple(int(f) for f in g) for g in decoder.field_groups)
        where, bypos = {}, []           # field id -> (group, position in the group, position in the output); output position -> (group, position in the group)
        for g, grp in enumerate(groups):
            for j, f in enumerate(grp):
                where[f] = (g, j, len(bypos))
                bypos.append((g, j))
        C_, Cp = int(decoder.n_inp), int(decoder._n_inp_p)
        src = []                        # per reading: (op code, group a, row a, group b, row b, out a, out b, sa, ha, sb, hb)
        for k in range(K):
            if not 0 <= patch[k] < n_patches:
                raise ValueError(f"{what}: sensor {k}: patch {patch[k]} outside 0 .. {n_patches - 1}")
            if not 0 <= cell[k] < C_:
                raise ValueError(f"{what}: sensor {k}: cell {cell[k]} outside 0 .. n_inp - 1 = {C_ - 1}")
            r = reading[k]
            if isinstance(r, DerivedField):
                if r.a >= len(bypos) or r.b >= len(bypos):
                    raise ValueError(f"{what}: sensor {k} ({r.name}): sources a = {r.a}, b = {r.b} outside the {len(bypos)} fields")
                (ga, ja), (gb, jb) = bypos[r.a], bypos[r.b]
                src.append((DERIVED_OPS.index(r.op), ga, ja * Cp + cell[k], gb, jb * Cp + cell[k], r.a, r.b, r.scale_a, r.shift_a, r.scale_b, r.shift_b))
                continue
            if torch.is_tensor(r) and r.dim() == 0 and r.dtype != torch.bool and not r.is_floating_point() and not r.is_complex():
                r = int(r)
            if isinstance(r, bool) or not (isinstance(r, int) or (_np is not None and isinstance(r, _np.integer))):
                raise ValueError(f"{what}: sensor {k}: a reading must be a field id (an integer) or a DerivedField, got {type(r).__name__}")
            r = reading[k] = int(r)
            if r not in where:
                raise ValueError(f"{what}: sensor {k}: field {r} is not one of the decoder's fields {sorted(where)}")
            g, j, pos = where[r]
            src.append((-1, g, j * Cp + cell[k], g, 0, pos, pos, 1.0, 0.0, 1.0, 0.0))
        self.n_patches, self.n_inp, self.Cp, self.groups, self.K = n_patches, C_, Cp, groups, K
        self.patch, self.cell, self.reading = patch, cell, reading
        self.field = [r if isinstance(r, int) else None for r in reading]
        self.out_field = [s[5] if s[0] < 0 else None for s in src]    # a derived reading has no field of its own (a per-field sigma is refused)
        self.plain = [s[0] < 0 for s in src]
        self._src = src
        self.fusable = all(s[1] == s[3] for s in src)
        self.patches = sorted(set(patch))
        G, T, Q = len(groups), N.SENSOR_TILE, len(self.patches)
        if Q > N.SENSOR_MAX_PATCHES:
            raise ValueError(f"{what}: {Q} observed patches; a set carries at most {N.SENSOR_MAX_PATCHES}")
        self.Q, self.K_pad = Q, None
        self.perm = self.wrow = self.live = self.seg = self.inv = self.op = self.scale = self.shift = None
        if self.fusable:
            buckets = {}
            for k in range(K):
                buckets.setdefault((src[k][1], patch[k]), []).append(k)
            perm, wrow, live, op, scale, shift, seg = [], [], [], [], [], [], []
            for g in range(G):
                row = []
                for p in self.patches:
                    row.append(len(perm))
                    ks = buckets.get((g, p), [])
                    for k in ks:
                        o, _, ra, _, rb, _, _, sa, ha, sb, hb = src[k]
                        perm += [k, k]
                        wrow += [ra, rb]
                        live += [1, 0]
                        op += [o, -1]
                        scale += [sa, sb]
                        shift += [ha, hb]
                    pad = -(2 * len(ks)) % T
                    perm += [0] * pad
                    wrow += [0] * pad
                    live += [0] * pad
                    op += [-1] * pad
                    scale += [1.0] * pad
                    shift += [0.0] * pad
                row.append(len(perm))
                seg.append(row)
            K_pad = len(perm)
            inv = [0] * K
            for s_, (k, l) in enumerate(zip(perm, live)):
                if l:
                    inv[k] = s_
            # the kernels trust these: check them here
            for g in range(G):
                for qi in range(Q):
                    a, b = seg[g][qi], seg[g][qi + 1]
                    if not 0 <= a <= b <= K_pad or (b - a) % T:
                        raise ValueError(f"{what}: internal error: segment ({g}, {qi}) = [{a}, {b}) is not a multiple of {T} inside 0 .. {K_pad}")
                    for s_ in range(a, b):
                        if not 0 <= wrow[s_] < len(groups[g]) * Cp or not 0 <= perm[s_] < K or not -1 <= op[s_] < len(DERIVED_OPS):
                            raise ValueError(f"{what}: internal error: entry {s_}: W2 row {wrow[s_]}, reading {perm[s_]} or op {op[s_]} out of range")
                        if s_ % 2 and (op[s_] != -1 or live[s_]):
                            raise ValueError(f"{what}: internal error: entry {s_}: the second entry of a pair carries an op or is live")
            if K_pad < T or K_pad >= 2 ** 31 or sum(live) != K or any(inv[k] % 2 for k in range(K)):
                raise ValueError(f"{what}: internal error: K_pad = {K_pad}, {sum(live)} live entries for {K} readings")
            self.K_pad, self.perm, self.wrow, self.live, self.seg, self.inv = K_pad, perm, wrow, live, seg, inv
            self.op, self.scale, self.shift = op, scale, shift
        self._finish_init(what, decoder, affine, points)   # the affine holds 1 and 0 at a derived reading

    def tables(self, device):
        """The tables on `device` (uploaded once per device): the composed path's patch, cell, out_a, out_b, cop (int64 [K]) and csa, cha, csb, chb
        (float32 [K]) and, for a fusable set, SensorSet's perm, wrow, live, seg, patches, inv plus op (int32), scale, shift (float32), each [K_pad]."""
        device = torch.device(device)
        t = self._dev.get(device)
        if t is None:
            i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=device)     # noqa: E731
            i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=device)     # noqa: E731
            f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=device)   # noqa: E731
            col = lambda i: [s[i] for s in self._src]                             # noqa: E731
            t = dict(patches=i64(self.patches), patch=i64(self.patch), cell=i64(self.cell), out_a=i64(col(5)), out_b=i64(col(6)), cop=i64(col(0)),
                     csa=f32(col(7)), cha=f32(col(8)), csb=f32(col(9)), chb=f32(col(10)))
            if self.fusable:
                t.update(perm=i32(self.perm), wrow=i32(self.wrow), live=i32(self.live), seg=i32(self.seg), inv=i64(self.inv), op=i32(self.op),
                         scale=f32(self.scale), shift=f32(self.shift))
            self._dev[device] = t
        return t

    def composed_predictions(self, y: torch.Tensor) -> torch.Tensor:
        """The readings of decoded fields y [Bm, P, n_fields, C] as float32 [Bm, K]: a gather of both source values and _composed_derived's float32
        arithmetic (the composed path; differentiable)."""
        T = self.tables(y.device)
        ya = y[:, T["patch"], T["out_a"], T["cell"]].to(torch.float32)
        yb = y[:, T["patch"], T["out_b"], T["cell"]].to(torch.float32)
        return _composed_derived_readings(ya, yb, T["cop"], T["csa"], T["cha"], T["csb"], T["chb"])

    def _require_fusable(self, what: str) -> None:
        if not self.fusable:
            raise ValueError(f"{what}: this DerivedSensorSet has a derived reading whose sources lie in different decoder groups: the fused launches pair "
                             f"two rows of ONE group's weights (fused=False, or None)")

    def _coeffs(self, device):
        if self._affine is None:
            raise ValueError("DerivedSensorSet: this set was not built from a mesh (MeshUnpatcher.derived_sensor_set): it has no field scaling")
        return SensorSet._coeffs(self, device)


def _derived_thresholds(what: str, thresholds, nd: int, max_t: int, finite: bool) -> torch.Tensor:
    """thresholds — numbers or a tensor, [T] (the same for every derived field) or [T, n_derived], 1 <= T <= max_t — as a contiguous float32 [T, n_derived]
    tensor on the host."""
    try:
        t = thresholds.detach().cpu() if torch.is_tensor(thresholds) else torch.as_tensor(thresholds, dtype=torch.float32)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{what}: thresholds must be [T] or [T, {nd}] numbers, got {thresholds!r}") from None
    if t.dim() not in (1, 2) or not 1 <= t.shape[0] <= max_t or (t.dim() == 2 and t.shape[1] != nd) or not t.is_floating_point():
        raise ValueError(f"{what}: thresholds must be [T] or [T, {nd}] floating-point numbers (one column per derived field) with 1 <= T <= {max_t}, got shape "
                         f"{tuple(t.shape)} {t.dtype}")
    t = (t.view(-1, 1).expand(t.shape[0], nd) if t.dim() == 1 else t).to(torch.float32).contiguous()
    if finite and not bool(torch.isfinite(t).all()):
        raise ValueError(f"{what}: every threshold must be finite")
    return t


class _DerivedBase:
    """What DerivedQuantiles, DerivedThresholdVerification and DerivedVerification share: the constructor's checks, the thresholds per device, the states'
    re-layout, the valid-cell mask and (the two verifying classes, which set self.observed) the observation brought to derived readings."""
    _what = "Derived"

    def _init_common(self, decoder, n_patches, members, derived, counts, layout, fused, max_n: int):
        what = self._what
        if layout not in ("BPFC", "BPCF"):
            raise ValueError(f"{what}: layout must be 'BPFC' or 'BPCF', got {layout!r}")
        if not isinstance(n_patches, int) or isinstance(n_patches, bool) or n_patches < 1:
            raise ValueError(f"{what}: n_patches = {n_patches!r} must be a positive integer")
        if not isinstance(members, int) or isinstance(members, bool) or members < 1:
            raise ValueError(f"{what}: members = {members!r} must be a positive integer")
        if fused is not None and not isinstance(fused, bool):
            raise ValueError(f"{what}: fused = {fused!r} must be None, True or False")
        if fused and members > max_n:
            raise ValueError(f"{what}: the fused launches carry up to {max_n} members, got {members} (fused=False, or None)")
        self.n_fields = sum(len(g) for g in decoder.field_groups)
        self.derived = _check_derived(what, derived, self.n_fields)
        if fused and len(self.derived) > N.DERIVED_MAX:
            raise ValueError(f"{what}: the fused launches carry up to {N.DERIVED_MAX} derived fields, got {len(self.derived)} (fused=False, or None)")
        self._thr = {}
        self.decoder, self.n_patches, self.members, self.counts, self.layout, self.fused = decoder, n_patches, members, counts, layout, fused

    def _thresholds_on(self, device):
        """The thresholds f32 [T, n_derived] on the device (None without): moved there once per device."""
        if self._thr_src is None:
            return None
        t = self._thr.get(device)
        if t is None:
            t = self._thr[device] = self._thr_src.to(device)
        return t

    def _states(self, y):
        """y [B * members, n_groups, n_patches * D] checked -> (z [Bm, P, G, D], Bm): the re-layout of FieldLikelihood."""
        P, what = self.n_patches, self._what
        if not torch.is_tensor(y) or y.dim() != 3 or y.shape[-1] % P or y.shape[0] < 1:
            raise ValueError(f"{what}: y must be [B * members, n_groups, n_patches * D] with n_patches = {P}, got "
                             f"{tuple(y.shape) if torch.is_tensor(y) else type(y).__name__}")
        Bm, G, E = y.shape
        if Bm % self.members:
            raise ValueError(f"{what}: the {Bm} trajectories of y are not a multiple of members = {self.members}")
        return y.detach().reshape(Bm, G, P, E // P).permute(0, 2, 1, 3), Bm

    def _valid(self, P: int, C_: int, device):
        """The valid-cell mask [1, P, 1, C] from counts (None: every cell)."""
        if self.counts is None:
            return None
        cnt = torch.as_tensor(self.counts, dtype=torch.int64).to(device).clamp(0, C_)
        return (torch.arange(C_, device=device) < cnt[:, None]).view(1, P, 1, C_)

    def _observation(self, obs, precision, B: int, device):
        """obs and precision checked and brought to derived readings: (obs [B, P, n_derived, W], precision [B, P, n_derived, W] or None)."""
        what, P, nd = self._what, self.n_patches, len(self.derived)
        width = self.n_fields if self.observed == "fields" else nd
        if not torch.is_tensor(obs) or obs.dim() != 4 or tuple(obs.shape[:2]) != (B, P):
            raise ValueError(f"{what}: the observation must be [{B}, {P}, ...] in layout {self.layout} (one snapshot per history), got "
                             f"{tuple(obs.shape) if torch.is_tensor(obs) else type(obs).__name__}")
        if obs.dtype != torch.float32 or obs.device != device:
            raise ValueError(f"{what}: obs must be float32 on {device}, got {obs.dtype} on {obs.device}")
        if precision is not None:
            if not torch.is_tensor(precision) or tuple(precision.shape) != tuple(obs.shape):
                raise ValueError(f"{what}: precision must be None or a map of obs's shape {tuple(obs.shape)}, got "
                                 f"{tuple(precision.shape) if torch.is_tensor(precision) else type(precision).__name__}")
            if precision.dtype != torch.float32 or precision.device != device:
                raise ValueError(f"{what}: precision must be float32 on {device}, got {precision.dtype} on {precision.device}")
            if precision.device.type == "cpu" and (not bool(torch.isfinite(precision).all()) or not bool((precision >= 0).all())):
                raise ValueError(f"{what}: precision must be finite and >= 0")
        perm = (lambda t: t) if self.layout == "BPFC" else (lambda t: t.permute(0, 1, 3, 2))
        obs, precision = perm(obs.detach()), None if precision is None else perm(precision.detach())
        if obs.shape[2] != width:
            raise ValueError(f"{what}: observed={self.observed!r}: the observation must carry {width} fields in layout {self.layout}, got shape {tuple(obs.shape)}")
        if self.observed == "derived":
            return obs, precision
        with torch.no_grad():
            x = _composed_derived(obs, self.derived)
            if precision is not None:   # live where both source cells are: the product of two 0 / 1 flags
                on = (precision > 0).to(torch.float32)
                precision = torch.stack([on.select(2, d.a) * on.select(2, d.b) for d in self.derived], dim=2)
        return x, precision


class DerivedQuantiles(_DerivedBase):
    """EnsembleQuantiles for DERIVED fields — "the 5 % / 95 % band of the speed", "P(speed > 1.2 U) here": quantiles(y, logw=None) -> (quant float32
    [Q, B, P, n_derived, n_inp], exceed float32 [T, B, P, n_derived, n_inp]).  A quantile of |u| is not a function of the quantiles of u and v: the derived
    value is formed per member (DerivedField; include/sea_hip.h, sea_decode_derived_quantiles) and the maps are read out of those values exactly as
    EnsembleQuantiles reads its maps out of a decoded field: each quantile is the derived value of one member, exceedance is strict.

    derived: a sequence of DerivedField (MeshUnpatcher.derived_fields builds them with the mesh's inverse scaling, so the values, the quantile maps and the
    thresholds are in PHYSICAL units); thresholds: None, [T] (the same for every derived field) or [T, n_derived], T <= 8, in the derived fields' own units.
    y, logw, counts, layout, levels and the conventions for dead members, invalid cells (0) and non-finite values (NaN) are EnsembleQuantiles'; the maps go
    to the mesh with MeshUnpatcher.unpatch_derived (they are in physical units already).
    fused: True — the decoder's first layer plus the ONE launch of sea_decode_derived_quantiles (bf16, up to 128 members, up to 8 derived fields whose two
    sources share a decoder group): neither the members' decoded fields nor the derived fields are written; raises where the launch refuses.  False —
    Decode.forward plus _composed_derived plus _composed_quantiles (the composed path: fp32, any member count, sources in different groups).  None — the
    fused launch where it serves, from 4096 decoder rows (B * members * n_patches) on — the measured rows (tools/derived_fields_bench.py,
    profiles/derived_fields_bench.txt) — and the composed path everywhere else, and wherever nothing was measured.
    from_fields(Y, logw=None) runs the composed arithmetic on members' decoded fields [B, members, P, F, n_inp] that already exist (CPU or device).
    A call reads nothing back from the device.  `decoder` is a sea_amd Decode; no autograd graph is built."""
    _what = "DerivedQuantiles"

    def __init__(self, decoder, n_patches: int, members: int, derived, levels=(0.05, 0.5, 0.95), thresholds=None, counts=None, layout: str = "BPFC",
                 fused: Optional[bool] = None):
        from . import ops

        self._init_common(decoder, n_patches, members, derived, counts, layout, fused, N.QUANTILE_MAX_N)
        self.levels = ops.check_quantile_levels(() if levels is None else levels, self._what)
        self._thr_src = None if thresholds is None else _derived_thresholds(self._what, thresholds, len(self.derived), N.QUANTILE_MAX_LEVELS, finite=False)
        if not self.levels and self._thr_src is None:
            raise ValueError(f"{self._what}: neither levels nor thresholds: there is nothing to compute")

    def _weights(self, logw, Bm: int, device):
        if logw is None:
            return None
        if not torch.is_tensor(logw) or not logw.is_floating_point() or logw.numel() != Bm or logw.dim() not in (1, 2) \
                or (logw.dim() == 2 and logw.shape[1] != self.members):
            raise ValueError(f"{self._what}: logw must be None or a floating-point [{Bm}] (or [{Bm // self.members}, {self.members}]) tensor of log-weights, got "
                             f"{tuple(logw.shape) if torch.is_tensor(logw) else type(logw).__name__}")
        if logw.device != device:
            raise ValueError(f"{self._what}: logw is on {logw.device}, the states on {device}")
        return normalised_weights(logw, self.members)

    def _permuted(self, quant, exceed, layout):
        layout = self.layout if layout is None else layout
        if layout not in ("BPFC", "BPCF"):
            raise ValueError(f"{self._what}: layout must be 'BPFC' or 'BPCF', got {layout!r}")
        if layout == "BPCF":
            quant = None if quant is None else quant.permute(0, 1, 2, 4, 3)
            exceed = None if exceed is None else exceed.permute(0, 1, 2, 4, 3)
        return quant, exceed

    def from_fields(self, Y: torch.Tensor, logw: Optional[torch.Tensor] = None, layout: Optional[str] = None):
        """The composed path on members' decoded fields Y [B, members, P, n_fields, n_inp] (scaled units, any float dtype, CPU or device)."""
        if not torch.is_tensor(Y) or Y.dim() != 5 or Y.shape[1] != self.members or Y.shape[2] != self.n_patches or Y.shape[3] != self.n_fields:
            raise ValueError(f"{self._what}: Y must be [B, {self.members}, {self.n_patches}, {self.n_fields}, n_inp], got "
                             f"{tuple(Y.shape) if torch.is_tensor(Y) else type(Y).__name__}")
        B, n, P, _, C_ = Y.shape
        with torch.no_grad():
            w = self._weights(logw, B * n, Y.device)
            q, e = _composed_quantiles(_composed_derived(Y.detach(), self.derived), None if w is None else w.view(B, n), self.levels, self._thresholds_on(Y.device))
            valid = self._valid(P, C_, Y.device)
            if valid is not None:
                zero = torch.zeros((), device=Y.device, dtype=torch.float32)
                q = None if q is None else torch.where(valid.unsqueeze(0), q, zero)
                e = None if e is None else torch.where(valid.unsqueeze(0), e, zero)
        return self._permuted(q, e, layout)

    def __call__(self, y: torch.Tensor, logw: Optional[torch.Tensor] = None, layout: Optional[str] = None):
        self._permuted(None, None, layout)
        z, Bm = self._states(y)
        w = self._weights(logw, Bm, y.device)
        N.require_gpu(y, f"{self._what} states")
        with torch.no_grad():
            quant, exceed = self.decoder.member_derived_quantiles(z, self.members, self.derived, levels=self.levels, thresholds=self._thresholds_on(y.device),
                                                                  weights=w, counts=self.counts, fused=self.fused)
        return self._permuted(quant, exceed, layout)

    quantiles = __call__


class DerivedThresholdVerification(_DerivedBase):
    """FieldThresholdVerification for DERIVED fields — is "P(speed > 1.2 U)" any good: verify(y, obs, precision=None, logw=None, into=None, maps=()) ->
    ThresholdScores with n_derived where that class has n_fields (include/sea_hip.h, sea_decode_derived_brier).  derived and thresholds ([T] or
    [T, n_derived], finite, in the derived fields' own units) as in DerivedQuantiles.
    observed="fields": obs (and precision) is the snapshot of the SOURCE fields that FieldThresholdVerification takes — [B, P, n_fields, >= n_inp] in layout
    "BPFC", scaled units; the observed derived values are formed from it with _composed_derived's arithmetic, on the device, and a derived cell is live
    only where both of its source cells are (precision > 0 in both).  observed="derived": obs and precision are [B, P, n_derived, >= n_inp] readings of the
    derived quantities themselves (a PIV speed map), in their own units.  The precision only decides which cells are read.
    fused as in DerivedQuantiles (True: the first layer plus the two launches of sea_decode_derived_brier; None: from 4096 decoder rows on where the launch
    serves, the composed path elsewhere).  from_fields(Y, obs, ...) runs the composed arithmetic on members' decoded fields [B, members, P, F, n_inp] that
    already exist (CPU or device).  Nothing is read back.  `decoder` is a sea_amd Decode; no autograd graph is built."""
    _what = "DerivedThresholdVerification"

    def __init__(self, decoder, n_patches: int, members: int, derived, thresholds, counts=None, layout: str = "BPFC", observed: str = "fields",
                 fused: Optional[bool] = None):
        if observed not in ("fields", "derived"):
            raise ValueError(f"{self._what}: observed must be 'fields' or 'derived', got {observed!r}")
        self._init_common(decoder, n_patches, members, derived, counts, layout, fused, N.BRIER_MAX_N)
        self.thresholds = self._thr_src = _derived_thresholds(self._what, thresholds, len(self.derived), N.BRIER_MAX_T, finite=True)
        self.observed = observed

    def from_fields(self, Y: torch.Tensor, obs: torch.Tensor, precision: Optional[torch.Tensor] = None, logw: Optional[torch.Tensor] = None,
                    into: Optional["ThresholdScores"] = None, maps=()) -> "ThresholdScores":
        """The composed path on members' decoded fields Y [B, members, P, n_fields, n_inp] (scaled units, any float dtype, CPU or device)."""
        if not torch.is_tensor(Y) or Y.dim() != 5 or Y.shape[1] != self.members or Y.shape[2] != self.n_patches or Y.shape[3] != self.n_fields:
            raise ValueError(f"{self._what}: Y must be [B, {self.members}, {self.n_patches}, {self.n_fields}, n_inp], got "
                             f"{tuple(Y.shape) if torch.is_tensor(Y) else type(Y).__name__}")
        B, n, P, _, C_ = Y.shape
        nd, T = len(self.derived), self.thresholds.shape[0]
        x_obs, prec = self._observation(obs, precision, B, Y.device)
        maps, logw = _check_brier_call(self._what, maps, logw, into, (B, nd, T), B * n, n, Y.device)
        thr = self._thresholds_on(Y.device)
        with torch.no_grad():
            cnt = None if self.counts is None else torch.as_tensor(self.counts, dtype=torch.int64).to(Y.device)
            w = _field_cell_weights((B, P, nd, C_), None, prec, cnt, Y.device)
            r = _composed_field_brier(_composed_derived(Y.detach(), self.derived).view(B * n, P, nd, C_), x_obs, w, logw, n, thr, maps=maps)
            if into is not None:
                r["sums"], r["hist"], r["hits"] = into.sums.add_(r["sums"]), into.hist.add_(r["hist"]), into.hits.add_(r["hits"])
        return ThresholdScores(prob=r.get("prob"), brier_map=r.get("brier"), sums=r["sums"], hist=r["hist"], hits=r["hits"], status=r["status"], thresholds=thr,
                               weighted=logw is not None or (into is not None and into.weighted))

    def __call__(self, y: torch.Tensor, obs: torch.Tensor, precision: Optional[torch.Tensor] = None, logw: Optional[torch.Tensor] = None,
                 into: Optional["ThresholdScores"] = None, maps=()) -> "ThresholdScores":
        z, Bm = self._states(y)
        n = self.members
        B = Bm // n
        nd, T = len(self.derived), self.thresholds.shape[0]
        x_obs, prec = self._observation(obs, precision, B, y.device)
        maps, logw = _check_brier_call(self._what, maps, logw, into, (B, nd, T), Bm, n, y.device)
        N.require_gpu(y, f"{self._what} states")
        thr = self._thresholds_on(y.device)
        r = self.decoder.member_derived_brier(z, x_obs, n, self.derived, thr, counts=self.counts, precision=prec, logw=logw, fused=self.fused, maps=maps,
                                              into=None if into is None else dict(sums=into.sums, hist=into.hist, hits=into.hits))
        return ThresholdScores(prob=r.get("prob"), brier_map=r.get("brier"), sums=r["sums"], hist=r["hist"], hits=r["hits"], status=r["status"], thresholds=thr,
                               weighted=logw is not None or (into is not None and into.weighted))

    verify = __call__


# ------------------------------------------------------------------------------------------------ derived fields: CRPS, rank and spread of the speed
# fused=None: the fused launches from this many decoder rows (B * members * n_patches) on — the smallest measured size (None would mean "nothing
# measured": the composed path everywhere)
DERIVED_VERIFY_FUSED_MIN_ROWS = 4096


def _check_verify_call(what: str, maps, logw, into, shape, Bm: int, n: int, device):
    """maps, logw and into of a field-verification call, checked (FieldVerification's checks); returns (maps, logw as a contiguous float32 [Bm] or None)."""
    maps = tuple(maps)
    if any(k not in FIELD_MAPS for k in maps) or len(set(maps)) != len(maps):
        raise ValueError(f"{what}: maps must be distinct names among {FIELD_MAPS}, got {maps!r}")
    if logw is not None:
        if not torch.is_tensor(logw) or not logw.is_floating_point() or logw.numel() != Bm or logw.dim() not in (1, 2) \
                or (logw.dim() == 2 and logw.shape[1] != n) or logw.device != device:
            raise ValueError(f"{what}: logw must be None or a floating-point [{Bm}] (or [{Bm // n}, {n}]) tensor of log-weights on {device}, got "
                             f"{(tuple(logw.shape), str(logw.device)) if torch.is_tensor(logw) else type(logw).__name__}")
        logw = logw.detach().reshape(-1).to(torch.float32).contiguous()
    if into is not None:
        if not isinstance(into, FieldScores) or tuple(into.sums.shape) != shape + (N.VERIFY_SUMS,) or tuple(into.hist.shape) != shape + (n + 1,) \
                or into.sums.device != device or into.sums.dtype != torch.float64 or into.hist.dtype != torch.int64 \
                or not into.sums.is_contiguous() or not into.hist.is_contiguous():
            raise ValueError(f"{what}: into must be an earlier FieldScores for {shape[0]} histories of {n} members and {shape[1]} derived fields on {device}")
    return maps, logw


class DerivedVerification(_DerivedBase, _FieldObserver):
    """FieldVerification for DERIVED fields — is the ensemble of the SPEED calibrated, is its spread the size of its error, what is its CRPS, is its rank
    histogram flat, what inflation does it suggest: verify(y, obs, precision=None, logw=None, into=None, maps=...) -> FieldScores with n_derived where
    FieldVerification has n_fields (include/sea_hip.h, sea_decode_derived_verify).  None of this follows from the scores of u and v: the derived value is
    formed per member (DerivedField), before the scoring.  pooled(), rmse, spread_skill, consistency, suggested_inflation and the rest of FieldScores work
    as they are; the maps go to the mesh with MeshUnpatcher.unpatch_derived (they are in physical units already).

    derived, counts, layout, y and logw as in DerivedThresholdVerification; unbiased, maps and into as in FieldVerification.  sigma: None, a number or
    n_derived numbers — the observation-error standard deviation in the derived field's own (physical) units, folded into a per-derived-field precision
    1 / sigma_d^2 as FieldVerification folds its sigma; 1 / weight is the observation-error variance that `consistency` and `suggested_inflation` use.
    observed="fields": obs (and precision) is the snapshot of the SOURCE fields that FieldVerification takes — [B, P, n_fields, >= n_inp] in layout
    "BPFC", scaled units; the observed derived value is formed from it with _composed_derived's arithmetic, on the device; a derived cell is live only
    where both of its source cells are (precision > 0 in both), and its weight is 1 / sigma_d^2: a source precision map has no defined image under a
    nonlinear op, it only decides liveness.  observed="derived": obs and precision are [B, P, n_derived, >= n_inp] readings of the derived quantities
    themselves (a PIV speed map), in their own units; the weight of a cell is precision / sigma_d^2, as in FieldVerification.
    fused: True — the decoder's first layer plus the two launches of sea_decode_derived_verify (bf16, up to 128 members, up to 8 derived fields whose two
    sources share a decoder group): neither the members' decoded fields nor the derived fields are written; raises where the launch refuses.  False —
    Decode.forward plus _composed_derived plus _composed_field_verify (the composed path: fp32, any member count, sources in different groups; it holds the
    members' fields several times over).  None — the fused launches where they serve (bf16, up to 128 members, up to 8 derived fields, both sources in one
    decoder group) from 4096 decoder rows (B * members * n_patches, DERIVED_VERIFY_FUSED_MIN_ROWS) on, and the composed path everywhere else — the measured
    rule (tools/derived_verify_bench.py, profiles/derived_verify_bench.txt; the speed of the cylinder decoder, P = 64 patches, n_inp
    1628, the mesh's counts, observed="fields", maps on and off, device time per call): 64 members, one history (4096 rows) 0.43 ms fused against 2.56 ms
    composed; 64 members, four histories (16384 rows) 0.82 against 8.8 ms; 128 members, one history (8192 rows) 0.82 against 3.45 ms; 128 members, four
    histories (32768 rows) 1.60 against 12.8 ms; 16 launches against 177; 9 - 70 MB of extra memory against 0.7 - 5.5 GB.  Nothing was measured below
    4096 rows, so the composed path stays the default there.
    from_fields(Y, obs, ...) runs the composed arithmetic on members' decoded fields [B, members, P, F, n_inp] that already exist (CPU or device).
    A call reads nothing back from the device.  `decoder` is a sea_amd Decode; no autograd graph is built."""
    _what = "DerivedVerification"

    def __init__(self, decoder, n_patches: int, members: int, derived, counts=None, layout: str = "BPFC", sigma=None, unbiased: bool = True,
                 observed: str = "fields", fused: Optional[bool] = None):
        if observed not in ("fields", "derived"):
            raise ValueError(f"{self._what}: observed must be 'fields' or 'derived', got {observed!r}")
        self._init_common(decoder, n_patches, members, derived, counts, layout, fused, N.FIELD_VERIFY_MAX_N)
        self._thr_src = None
        self.observed, self.unbiased = observed, bool(unbiased)
        self._set_sigma(sigma, len(self.derived))

    def _scores(self, r) -> FieldScores:
        return FieldScores(**{k: r.get(k) for k in FIELD_MAPS}, sums=r["sums"], hist=r["hist"], status=r["status"])

    def from_fields(self, Y: torch.Tensor, obs: torch.Tensor, precision: Optional[torch.Tensor] = None, logw: Optional[torch.Tensor] = None,
                    into: Optional[FieldScores] = None, maps=FIELD_MAPS) -> FieldScores:
        """The composed path on members' decoded fields Y [B, members, P, n_fields, n_inp] (scaled units, any float dtype, CPU or device)."""
        if not torch.is_tensor(Y) or Y.dim() != 5 or Y.shape[1] != self.members or Y.shape[2] != self.n_patches or Y.shape[3] != self.n_fields:
            raise ValueError(f"{self._what}: Y must be [B, {self.members}, {self.n_patches}, {self.n_fields}, n_inp], got "
                             f"{tuple(Y.shape) if torch.is_tensor(Y) else type(Y).__name__}")
        B, n, P, _, C_ = Y.shape
        nd = len(self.derived)
        x_obs, prec = self._observation(obs, precision, B, Y.device)
        if x_obs.shape[3] < C_:
            raise ValueError(f"{self._what}: the observation carries {x_obs.shape[3]} cells per patch, the members' fields {C_}")
        maps, logw = _check_verify_call(self._what, maps, logw, into, (B, nd), B * n, n, Y.device)
        with torch.no_grad():
            cnt = None if self.counts is None else torch.as_tensor(self.counts, dtype=torch.int64).to(Y.device)
            w = _field_cell_weights((B, P, nd, C_), self._field_precision(Y.device), prec, cnt, Y.device)
            r = _composed_field_verify(_composed_derived(Y.detach(), self.derived).view(B * n, P, nd, C_), x_obs, w, logw, n, self.unbiased, maps=maps)
            if into is not None:
                r["sums"], r["hist"] = into.sums.add_(r["sums"]), into.hist.add_(r["hist"])
        return self._scores(r)

    def __call__(self, y: torch.Tensor, obs: torch.Tensor, precision: Optional[torch.Tensor] = None, logw: Optional[torch.Tensor] = None,
                 into: Optional[FieldScores] = None, maps=FIELD_MAPS) -> FieldScores:
        z, Bm = self._states(y)
        n = self.members
        B = Bm // n
        x_obs, prec = self._observation(obs, precision, B, y.device)
        maps, logw = _check_verify_call(self._what, maps, logw, into, (B, len(self.derived)), Bm, n, y.device)
        N.require_gpu(y, f"{self._what} states")
        r = self.decoder.member_derived_verify(z, x_obs, n, self.derived, counts=self.counts, precision=prec, field_precision=self._field_precision(y.device),
                                               logw=logw, unbiased=self.unbiased, fused=self.fused, maps=maps,
                                               into=None if into is None else dict(sums=into.sums, hist=into.hist))
        return self._scores(r)

    verify = __call__
