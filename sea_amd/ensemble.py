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
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _native as N
from . import ops


class FieldLikelihood:
    """Gaussian log-likelihood of an observation of the decoded fields, per ensemble member: like(y, obs) -> log-weights [B * members] (f32, device).

    y: what RolloutSession.step returns for a session of B * members trajectories, [B * members, n_groups, P * D] (member j of history b at row
    b * members + j, the order of fork()); obs: float32 [B, P, n_fields, C >= n_inp] (what patchify_and_scale(..., layout="BPFC") writes for one
    snapshot) or, with layout="BPCF", the reference's [B, P, C, n_fields].  logw = -0.5 * sum_f sse_f / sigma_f^2 with sse_f the member's squared
    error of field f over its patches and valid cells (Decode.member_sse); sigma: None (1), a positive number, or n_fields positive numbers (a
    sequence or tensor) — applied with tensor ops on the [B * members, n_fields] result.  counts: valid cells per patch (None: all), as in
    Decode.mse_loss.  fused: None (Decode.member_sse's measured rule), True (the fused launch at any size; bf16 only) or False (the composed path).
    `decoder` is a sea_amd Decode; no autograd graph is built."""

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

    def __call__(self, y: torch.Tensor, obs: torch.Tensor, layout: Optional[str] = None) -> torch.Tensor:
        layout = self.layout if layout is None else layout
        if layout not in ("BPFC", "BPCF"):
            raise ValueError(f"FieldLikelihood: layout must be 'BPFC' or 'BPCF', got {layout!r}")
        P = self.n_patches
        if y.dim() != 3 or y.shape[-1] % P or y.shape[0] < 1:
            raise ValueError(f"FieldLikelihood: y must be [B * members, n_groups, n_patches * D] with n_patches = {P}, got {tuple(y.shape)}")
        Bm, G, E = y.shape
        if Bm % self.members:
            raise ValueError(f"FieldLikelihood: the {Bm} trajectories of y are not a multiple of members = {self.members}")
        B = Bm // self.members
        if obs.dim() != 4 or tuple(obs.shape[:2]) != (B, P):
            raise ValueError(f"FieldLikelihood: the observation must be [{B}, {P}, ...] in layout {layout} (one per history), got {tuple(obs.shape)}")
        z = y.reshape(Bm, G, P, E // P).permute(0, 2, 1, 3)          # the re-layout of inverse_transform_processed_data, one snapshot per member
        tgt = obs if layout == "BPFC" else obs.permute(0, 1, 3, 2)
        sse = self.decoder.member_sse(z, tgt, counts=self.counts, members=self.members, fused=self.fused)
        return (sse * self._field_scale(sse.device)).sum(1)


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
