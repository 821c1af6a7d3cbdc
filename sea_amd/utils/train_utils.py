"""Host-side mirror of the hot-path half of the reference's utils/train_utils.py.

Mirrored (same names and argument meaning): initialize_optimizer (:33-39), calculate_R2 (:42-48), relativeMSE (:112-116),
relativeMSE_with_time (:124-150), autoregressive_validation (:154-184), full_autoregressive_evaluation (:186-212, the
encoded half; decoding through the spatial autoencoder, CSV and plots are out of scope — SURVEY.md §2), the
error-tracker duck type (:50-110).  `rollout` is the loop both evaluation functions share (:202-209), with the
reference-equivalent recompute mode and an exact KV-cache mode.
"""
from __future__ import annotations

import os
from typing import Any, Dict

import torch

from .. import _native as N


# ------------------------------------------------------------------------------------------------ metrics
def relativeMSE(predictions: torch.Tensor, truth: torch.Tensor, dim: int = -1) -> torch.Tensor:
    """sum((p - t)^2, dim) / (sum(t^2, dim) + 1e-8) through sea_relative_mse (reference :112-116)."""
    N.require_gpu(predictions, "predictions")
    assert predictions.shape == truth.shape, "Predictions and truth must have the same shape"
    nd = predictions.dim()
    dim = dim % nd
    p, t = predictions.float(), truth.float()
    if dim != nd - 1:
        p, t = p.movedim(dim, -1), t.movedim(dim, -1)
    p, t = p.contiguous(), t.contiguous()
    d = p.shape[-1]
    rows = p.numel() // d
    y = torch.empty(p.shape[:-1], device=p.device, dtype=torch.float32)
    N.check(N.lib().sea_relative_mse(p.data_ptr(), t.data_ptr(), y.data_ptr(), rows, d, N.stream_ptr()), "sea_relative_mse")
    return y


def relativeMSE_with_time(predictions: torch.Tensor, truth: torch.Tensor, dim=2) -> torch.Tensor:
    """Same ratio, summed over `dim` (reference :124-150)."""
    return relativeMSE(predictions, truth, dim=dim)


def calculate_R2(prediction: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """1 - sum((p - y)^2) / sum((y - mean(y))^2) over all elements (reference :42-48); a 0-d tensor on the inputs' device."""
    prediction, labels = prediction.reshape(-1), labels.reshape(-1)
    residual = torch.sum((prediction - labels) ** 2)
    total = torch.sum((labels - torch.mean(labels)) ** 2)
    return 1 - residual / total


class SeaMSELoss(torch.nn.Module):
    """nn.MSELoss() replacement whose forward AND backward are one fused kernel (sea_mse_fwd_bwd)."""

    def forward(self, output: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        from ..autograd import MSELossFn

        return MSELossFn.apply(output, target)


class FieldSpaceLoss(torch.nn.Module):
    """Mean squared error of the DECODED fields: loss = FieldSpaceLoss(decoder, n_patches, counts)(out, target_fields).

    out: the temporal model's output [B, T, n_groups, P * D]; target_fields: float32 patch fields [B, T, P, n_fields, C] (what
    patchify_and_scale(..., layout="BPFC") writes; C >= the decoder's n_inp) or, with layout="BPCF", the reference's [B, T, P, C, n_fields].
    The latent -> z re-layout of inverse_transform_processed_data / decode_rollout is applied as torch views, so autograd carries the gradient
    back to the temporal model's hand-written backward; the loss itself is Decode.mse_loss (one fused launch in bf16; the decoded fields are
    never written).  `decoder` is a frozen sea_amd Decode (decoder.requires_grad_(False)); it is not registered as a sub-module, so the loss
    has no parameters.  counts: valid cells per patch (None: all), see Decode.mse_loss."""

    def __init__(self, decoder, n_patches: int, counts=None, layout: str = "BPFC", fused=None):
        super().__init__()
        if layout not in ("BPFC", "BPCF"):
            raise ValueError(f"FieldSpaceLoss: layout must be 'BPFC' or 'BPCF', got {layout!r}")
        if int(n_patches) < 1:
            raise ValueError(f"FieldSpaceLoss: n_patches = {n_patches} must be positive")
        object.__setattr__(self, "decoder", decoder)
        self.n_patches, self.counts, self.layout, self.fused = int(n_patches), counts, layout, fused

    def forward(self, output: torch.Tensor, target_fields: torch.Tensor, layout=None) -> torch.Tensor:
        layout = self.layout if layout is None else layout
        if output.dim() != 4 or output.shape[-1] % self.n_patches:
            raise ValueError(f"FieldSpaceLoss: output must be [B, T, n_groups, n_patches * D] with n_patches = {self.n_patches}, got {tuple(output.shape)}")
        B, T, G, _ = output.shape
        if target_fields.dim() != 5 or tuple(target_fields.shape[:3]) != (B, T, self.n_patches):
            raise ValueError(f"FieldSpaceLoss: target fields must be [{B}, {T}, {self.n_patches}, ...] in layout {layout}, got {tuple(target_fields.shape)}")
        z = inverse_transform_processed_data(output, B, T, self.n_patches, G)
        tgt = target_fields if layout == "BPFC" else target_fields.permute(0, 1, 2, 4, 3)
        tgt = tgt.reshape((B * T,) + tuple(tgt.shape[2:]))
        return self.decoder.mse_loss(z, tgt, counts=self.counts, fused=self.fused)


# ------------------------------------------------------------------------------------------------ ensembles (sea_amd/ensemble.py)
from ..ensemble import DerivedField, DerivedQuantiles, DerivedSensorSet, DerivedThresholdVerification, DerivedVerification, EnsembleCRPSLoss, EnsembleFields, EnsembleQuantiles, EnsembleScores, FieldKalman, FieldLikelihood, FieldScores, FieldThresholdVerification, FieldVerification, SensorKalman, SensorLikelihood, SensorSet, SensorThresholdVerification, SensorVerification, ThresholdScores, gaspari_cohn, systematic_resample  # noqa: E402,F401  (re-exported: the particle-filter steps around a RolloutSession)


# ------------------------------------------------------------------------------------------------ optimizer
def initialize_optimizer(model, config):
    """AdamW(lr=config['learning_rate'], betas=(0.9, 0.999), eps=1e-8, weight_decay=config.get('weight_decay', 0.0)) as one fused
    kernel over the model's flat parameter buffer (reference :33-39).  Returns (optimizer, scheduler) when
    config['scheduler'] == 'linear', like the reference.  Two optional keys beyond the reference's: config['max_grad_norm'] (clip the gradients
    by their global 2-norm) and config['skip_nonfinite_steps'] (drop a step whose gradient norm is inf or NaN), both decided on the device
    (sea_amd/optim.py)."""
    from ..optim import FlatAdamW

    opt = FlatAdamW(model, lr=config['learning_rate'], betas=(0.9, 0.999), eps=1e-8, weight_decay=config.get('weight_decay', 0.0),
                    max_grad_norm=config.get('max_grad_norm'), skip_nonfinite=config.get('skip_nonfinite_steps', False))
    if config.get('scheduler', None) == 'linear':
        sched = torch.optim.lr_scheduler.LinearLR(opt, start_factor=0.1, end_factor=1.0, total_iters=config['epoch_num'])
        return opt, sched
    return opt


# ------------------------------------------------------------------------------------------------ rollout
_KV_FALLBACK_WARNED: set = set()


def rollout(model, x0: torch.Tensor, ib: torch.Tensor, n_steps: int, mode: str = "kv") -> torch.Tensor:
    """Autoregressive rollout (reference :202-209) from a known history: x0 [B,k,F,E] holds the states at positions 0 .. k-1 (k >= 1; the
    reference starts from k = 1), ib [B, >= k+n_steps-1, 1] one condition per position 0 .. k+n_steps-2.  Returns the n_steps predictions of
    positions k .. k+n_steps-1 [B, n_steps, F, E].

    mode='recompute' — what the reference does: the full forward over the growing prefix every step (O(N^2) token-forwards);
    mode='kv'        — exact incremental decode with per-layer K/V caches (the model is strictly causal and
                        prefix-consistent), O(N) token-forwards; a context of k > 1 states is prefilled by one
                        full-context forward (engine.rollout_kv).
    ValueError, before anything runs: k = 0, k + n_steps - 1 > max_len, or fewer than k + n_steps - 1 conditions.
    """
    assert mode in ("recompute", "kv")
    from ..kv_engine import check_context

    k = check_context(model, x0, ib, n_steps)
    if mode == "kv" and (getattr(model, "src_len", 0) > 0 or getattr(model, "exchange_mode", "sea") == "pool"
                         or str(getattr(model, "ib_addition_mode", "add")).lower() == "attention"):
        # a cache is exact only for strictly causal attention (src_len == 0, no un-masked info-bottleneck attention) and absolute positions (not 'pool'):
        # see engine.rollout_kv.  The caller asked for 'kv' (the shipped configs do): say once that the O(N^2) loop runs instead.
        why = ("src_len > 0" if getattr(model, "src_len", 0) > 0 else
               "exchange_mode='pool'" if getattr(model, "exchange_mode", "sea") == "pool" else "ib_addition_mode='attention'")
        if why not in _KV_FALLBACK_WARNED:
            _KV_FALLBACK_WARNED.add(why)
            import warnings

            warnings.warn(f"sea_amd.rollout: mode='kv' is not exact for this model ({why}); running the recompute rollout instead", RuntimeWarning, stacklevel=2)
        mode = "recompute"
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            if mode == "recompute":
                a = x0
                for i in range(n_steps):
                    out = model(a, ib[:, : k + i])
                    a = torch.cat((a, out[:, -1:]), dim=1)
                return a[:, k:]
            return model.engine(x0.device).rollout_kv(x0.float(), ib.float(), n_steps)
    finally:
        model.train(was_training)


def open_rollout(model, x0: torch.Tensor, ib: torch.Tensor):
    """A stateful KV-cache rollout (sea_amd/rollout_session.py) from a known history: x0 [B, k, F, E] holds the states of positions 0 .. k-1 (k >= 1),
    ib [B, k-1, 1] the conditions of positions 0 .. k-2 (may be empty) — the condition of the newest state arrives with the first step, which is
    what lets a controller or a coupled solver choose it after seeing that state.

        s = open_rollout(model, x0, ib)
        y = s.step(c)                 # c [B, 1] or [B] -> the next state [B, F, E]; s.step(c, state=z) first replaces the current state by z
        ys = s.advance(conds)         # conds [B, n, 1] -> [B, n, F, E]: n steps in the native loop
        s.position, s.states()        # index of the newest known state; the trajectory so far [B, position + 1, F, E]
        s.rewind(p)                   # go back to position p
        t = s.fork(n)                 # B * n independent trajectories (row b * n + j: branch j of b) that share the history so far
        s.close()                     # or `with open_rollout(...) as s:`

    open(...).advance(ib[:, k-1:k-1+n]) is the trajectory of rollout(model, x0, ib, n, mode='kv').  The session owns its caches: rollout(), model(x, ib)
    and other sessions on the same model do not disturb it.  It reads the weights as they are at every call; after an optimizer step the caches are
    stale — open a new session.  NotImplementedError for the models the KV-cache rollout does not cover (src_len > 0, exchange_mode='pool',
    ib_addition_mode='attention': a session has no recompute fallback); ValueError, before anything runs, for a malformed history."""
    from ..rollout_session import check_open

    check_open(model, x0, ib)
    with torch.no_grad():
        return model.engine(x0.device).open_rollout(x0, ib)


def autoregressive_validation(model, validationLoader, loss_fn, device):
    """Autoregressive validation on the first sample of the first batch (reference :154-184)."""
    model.eval()
    with torch.no_grad():
        data, target, _, ib = next(iter(validationLoader))
        data, target, ib = data[0:1].to(device), target[0:1].to(device), ib[0:1].to(device)
        pred = rollout(model, data[:, 0:1].contiguous(), ib, target.shape[1], mode=_rollout_mode(model))
        v_loss = loss_fn(pred, target)
        v_rel_mse = relativeMSE_with_time(pred, target, dim=3).mean()
    return v_loss.item(), v_rel_mse.item()


def full_autoregressive_evaluation(model, dataLoader, loss_fn, device, processor, mesh_processor, config, epoch, plot_traj=True):
    """The reference's evaluation (:186-312) on the device: roll every batch out from its first step, relativeMSE in the encoded space; then —
    when `processor` (ProcessData: the frozen spatial decoder) and `mesh_processor` (MeshProcessor) are given — decode the rollout
    (inverse_transform_processed_data -> processor.decode_data), undo the SEA_isolate / SEA_mixed layout switch, un-patchify + inverse-scale
    (mesh_processor.inverse_scale_and_unpatch) and take relativeMSE_with_time over the mesh points per step and field.  The per-step table goes to
    `{save_dir}/rollout_error_{case_name}_{run_name}.csv` as in the reference (rewritten for every batch, so — like the reference's, :249-262 — the file
    holds the LAST batch's table); its contour plots are not produced.  Returns the reference's dict
    {'encoded_rel_mse', 'decoded_rel_mse'} (None for an empty loader); decoded_rel_mse is NaN without the two processors."""
    model.eval()
    enc_sum, dec_sum, n_batches = 0.0, 0.0, 0
    decode = processor is not None and mesh_processor is not None
    with torch.no_grad():
        for data, target, original_data, ib in dataLoader:
            data, target, ib = data.to(device), target.to(device), ib.to(device)
            pred = rollout(model, data[:, 0:1].contiguous(), ib, target.shape[1], mode=_rollout_mode(model, config))
            enc_sum += relativeMSE(pred, target).mean().item()
            if decode:
                tr, T = pred.shape[0], pred.shape[1]
                if config['dimension'] == '3D':
                    n_patches = (config['m'] - 1) * (config['n'] - 1) * (config['k'] - 1)
                else:
                    n_patches = (config['m'] - 1) * (config['n'] - 1)
                z = inverse_transform_processed_data(pred, tr, T, n_patches, len(config['field_groups']))
                fused = config.get('SEA_isolate') and not config.get('SEA_mixed') and hasattr(processor, 'decoder') and hasattr(mesh_processor, 'decode_and_unpatch')
                dec = None if fused else processor.decode_data(z)   # [tr*T, P, F, C]
                if fused:   # the decoder over a cell's mesh points only, then the scatter: the same fields as the two calls below, without the padding
                    fields = mesh_processor.decode_and_unpatch(processor.decoder(), z)
                elif config.get('SEA_mixed'):
                    B_, P_, F_, C_ = dec.shape
                    fields = mesh_processor.inverse_scale_and_unpatch(dec.reshape(B_, P_, C_, F_))
                elif config.get('SEA_isolate'):
                    fields = mesh_processor.inverse_scale_and_unpatch(dec, layout="BPFC")     # the permute(0, 1, 3, 2) of :225 is read in place
                else:
                    assert False, "Invalid SEA data configuration"
                fields = fields.reshape(tr, T, fields.shape[1], fields.shape[2])
                per_step = relativeMSE_with_time(fields, original_data.to(device).float(), dim=2).mean(dim=0)       # [T, F]
                dec_sum += per_step.mean().item()
                if config.get('save_dir') and os.path.isdir(config['save_dir']):
                    import csv

                    with open(f"{config['save_dir']}/rollout_error_{config.get('case_name', 'case')}_{config.get('run_name', 'run')}.csv", 'w', newline='') as f:
                        w = csv.writer(f)
                        w.writerow(['Time Step'] + [f'Field {i + 1}' for i in range(per_step.shape[1])])
                        for i, row in enumerate(per_step.cpu().numpy()):
                            w.writerow([i + 1] + list(row))
            else:
                dec_sum = float("nan")
            n_batches += 1
    if n_batches == 0:
        return None
    return {"encoded_rel_mse": enc_sum / n_batches, "decoded_rel_mse": dec_sum / n_batches}


def _rollout_mode(model, config=None) -> str:
    if config is not None and config.get('rollout_mode'):
        return config['rollout_mode']
    return getattr(model, "rollout_mode", "kv")


# ------------------------------------------------------------------------------------------------ error trackers (duck type, :50-110)
class NoOpErrorTracker:
    def __init__(self, *args, **kwargs):
        pass

    def record_error(self, phase, epoch, metrics):
        pass

    def log_model(self, model, criterion, optimizer):
        pass

    def finish(self):
        pass


def create_error_tracker(use_wandb, project_name, run_name=None, config: Dict[str, Any] = None):
    """wandb is not part of this build: always the no-op tracker (the reference falls back to it when wandb is missing)."""
    return NoOpErrorTracker()


def transform_processed_data(processed_data: torch.Tensor, tr: int, T: int, n_patches: int, num_field_groups: int) -> torch.Tensor:
    """[tr*T, P, num_field_groups, D] -> [tr, T, num_field_groups, P*D] (reference utils/train_utils.py:315-337, same signature)."""
    D = processed_data.shape[-1]
    return processed_data.reshape(tr, T, n_patches, num_field_groups, D).permute(0, 1, 3, 2, 4).reshape(tr, T, num_field_groups, -1)


def inverse_transform_processed_data(transformed_data: torch.Tensor, tr: int, T: int, n_patches: int, num_field_groups: int) -> torch.Tensor:
    """[tr, T, num_field_groups, P*D] -> [tr*T, P, num_field_groups, D] (reference utils/train_utils.py:339-362, same signature)."""
    D = transformed_data.shape[-1] // n_patches
    return transformed_data.reshape(tr, T, num_field_groups, n_patches, D).permute(0, 1, 3, 2, 4).reshape(tr * T, n_patches, num_field_groups, D)


def decode_rollout(decoder, rollout_out: torch.Tensor, n_patches: int) -> torch.Tensor:
    """The decode leg of full_autoregressive_evaluation (reference utils/train_utils.py:214-222): rollout output [tr, T, G, P*D] ->
    decoded patches [tr*T, P, n_fields, n_inp], on the device (the reference round-trips through `processor.decode_data`)."""
    tr, T, G, _ = rollout_out.shape
    return decoder(inverse_transform_processed_data(rollout_out, tr, T, n_patches, G))
