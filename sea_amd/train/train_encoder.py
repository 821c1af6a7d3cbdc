"""Training of the spatial autoencoder: the hot-path half of the reference's train/train_encoder.py (get_model :148-175, train :186-316) on the
SpatialModel training path (sea_amd/spatial_train.py: composed forward / backward launches, the fused AdamW over the flat parameter buffer).

Loaders come in ready-made through config['loaders'] = (train, val, test), as for sea_amd.train.train_temporal; building them from files
(get_datasets) is not part of this module.  One process; the variational encoder is not provided.
"""
from __future__ import annotations

import time
from typing import Any, Dict, Tuple

import torch

from ..models.encoder_decoder import SpatialModel
from ..utils.train_utils import SeaMSELoss, calculate_R2, initialize_optimizer


def get_model(config: Dict[str, Any], device: torch.device) -> Tuple[SpatialModel, torch.nn.Module, torch.optim.Optimizer]:
    """(model, loss_fn, optimizer) with the reference's constructor keys (:148-175).  config['compute_dtype'] ('fp32' | 'bf16', default fp32)
    selects the matrix-operand dtype."""
    if config.get('variational', False):
        raise NotImplementedError("sea_amd.train_encoder: the variational encoder is not provided (both shipped configs use variational=False)")
    model = SpatialModel(field_groups=config['field_groups'], n_inp=config['n_inp'], MLP_hidden=config['MLP_hidden'], num_layers=config['num_layers'],
                         embed_dim=config['embed_dim'], n_heads=config['n_heads'], max_len=config['block_size'], src_len=config.get('src_len', 0),
                         variational=False, dropout=config['dropout'])
    if config.get('load_pretrained', False):
        model.load_state_dict(torch.load(config['pretrained_model_path'], map_location='cpu'))
        print(f"Loaded pre-trained model from {config['pretrained_model_path']}")
    model.set_compute_dtype(config.get('compute_dtype', 'fp32'))
    model = model.to(device)
    optimizer = initialize_optimizer(model, config)
    return model, SeaMSELoss(), optimizer


def train(config: Dict[str, Any], error_tracker):
    """The reference's epoch loop (:186-316): MSE against the masked input, R^2, validation every config['validation_interval'] epochs and at the last,
    best-by-validation-loss checkpoint {save_dir}/encoder_decoder_{case_name}_{run_name}.pt (the model's state_dict, reference keys)."""
    if 'loaders' not in config:
        raise RuntimeError("sea_amd.train_encoder: pass config['loaders'] = (trainLoader, validationLoader, testLoader); building them from "
                           "files is not part of this package")
    trainLoader, validationLoader, _ = config['loaders']
    device = torch.device(config['device'])
    model, loss_fn, optimizer = get_model(config, device)
    if isinstance(optimizer, tuple):
        optimizer = optimizer[0]
    model.train()
    start_time = time.time()
    prev_error = float('inf')
    error_tracker.log_model(model, loss_fn, optimizer)
    # clipping / skipping (config['max_grad_norm'], config['skip_nonfinite_steps']): the loop reads the loss on the host every step, and reads
    # the step's control block with it; a skipped step counts for neither the loss nor R^2
    controlled = bool(getattr(optimizer, 'controlled', False))
    grad_norm, stats = 0.0, None

    for epoch in range(1, config['epoch_num'] + 1):
        model.train()
        train_loss, train_r2_sum, n_batches = 0.0, 0.0, 0
        for data in trainLoader:
            data = data.to(device, dtype=torch.float32)
            optimizer.zero_grad()
            outputs = model(data)          # masks data in place: the loss target is the masked input, as in the reference
            loss = loss_fn(outputs, data)
            loss.backward()
            optimizer.step()
            if controlled:
                stats = optimizer.step_stats()
                if not stats["applied"]:
                    continue
                grad_norm = stats["grad_norm"]
            train_loss += loss.item()
            train_r2_sum += calculate_R2(outputs.detach(), data).item()
            n_batches += 1
        if controlled and n_batches == 0:   # no step of the epoch was applied: there is nothing to average
            train_loss = train_r2 = float('nan')
        else:
            train_loss /= n_batches
            train_r2 = train_r2_sum / n_batches
        record = {"Loss": train_loss, "Recon_Loss": train_loss, "R2": train_r2}
        if controlled and stats is not None:
            record.update({"GradNorm": grad_norm, "SkippedSteps": stats["skipped_steps"], "ClippedSteps": stats["clipped_steps"]})
        error_tracker.record_error("train", epoch, record)

        if epoch % config.get('validation_interval', 1) == 0 or epoch == config['epoch_num']:
            model.eval()
            val_loss, val_r2_sum, n_val = 0.0, 0.0, 0
            with torch.no_grad():
                for v_data in validationLoader:
                    v_data = v_data.to(device, dtype=torch.float32)
                    v_outputs = model(v_data)
                    val_loss += loss_fn(v_outputs, v_data).item()
                    val_r2_sum += calculate_R2(v_outputs, v_data).item()
                    n_val += 1
            val_loss /= n_val
            val_r2 = val_r2_sum / n_val
            error_tracker.record_error("val", epoch, {"Loss": val_loss, "Recon_Loss": val_loss, "R2": val_r2})
            print(f"\nEpoch: {epoch}/{config['epoch_num']}")
            print(f"Train - Loss: {train_loss:.8f}, R^2: {train_r2:.8f}")
            print(f"Val   - Loss: {val_loss:.8f}, R^2: {val_r2:.8f}")
            if val_loss < prev_error:
                prev_error = val_loss
                print("--- New Best Model Saved ---")
                path = f"{config['save_dir']}/encoder_decoder_{config['case_name']}_{config['run_name']}.pt"
                # copied to the host without moving the model: .to('cpu') would drop the flat parameter buffer and the optimizer's moments
                torch.save({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, path)
            else:
                print("--- No Improvement, Best Model Retained ---")

    print(f"Total training time: {time.time() - start_time:.2f} seconds")
    error_tracker.finish()
    return model
