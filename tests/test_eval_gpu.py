"""The entry points north_star names, executed: `train(config, tracker)` / `get_model` (train/train_temporal.py:190-348) on synthetic loaders, and the
`temporal test` evaluation (main.py:101-123 -> full_autoregressive_evaluation / autoregressive_validation, utils/train_utils.py:154-312) on a
synthetic mesh against the numbers the REFERENCE's own MeshProcessor / ProcessData / TemporalDataset / evaluation loop produced
(tests/golden/eval_synth.npz, tests/golden/make_fixtures.py::eval_case)."""
import os

import numpy as np
import pytest
import torch

from oracle.recipe import decode_schema, encoder_schema, recipe_params, recipe_tensor
from tests.conftest import cfg_from_meta, load_golden, rel_l2
from tests.test_model_gpu import build, gpu

pytestmark = pytest.mark.gpu


def _eval_setup(tmp_path, dtype="fp32", n_points=None):
    """n_points: keep only the first n_points mesh points of the fixture (a ragged mesh; the fixture's own z / enc then no longer apply)."""
    from sea_amd.utils.data_processors import MeshProcessor, ProcessData, TemporalDataset
    from sea_amd.utils.train_utils import transform_processed_data

    g = load_golden("eval_synth")
    m_, n_, D, hidden, layers, Hs, n_inp, tr, T = (int(v) for v in g["dims"])
    groups, f0 = [], 0
    for n_f in g["groups"]:
        groups.append(list(range(f0, f0 + int(n_f))))
        f0 += int(n_f)
    sd = {}
    for k, (shp, kind) in {**encoder_schema(groups, n_inp, hidden, layers, D, pre="encode."), **decode_schema(groups, n_inp, hidden, D, pre="decode.decoders.")}.items():
        sd[k] = torch.from_numpy(recipe_tensor(k, shp, kind))
    from sea_amd.models.encoder_decoder import SpatialModel

    # the checkpoint of the reference also holds the sinusoidal table buffer (deterministic: taken from a fresh module)
    sd["encode.spatial_pos_encoder.pe"] = SpatialModel(groups, n_inp, hidden, layers, D, Hs, 64, 0, dropout=0.0).state_dict()["encode.spatial_pos_encoder.pe"]
    config = dict(device="cuda", save_dir=str(tmp_path), dimension="2D", field_groups=groups, scale_feature_range=None, csv_scale_name="scaler", m=m_, n=n_,
                  k=None, pad_id=-1, pad_field_value=0, MLP_hidden_spatial=hidden, num_layers_spatial=layers, embed_dim_spatial=D, n_heads_spatial=Hs,
                  block_size_spatial=64, dropout_spatial=0.0, variational_spatial=False, src_len_spatial=0, encoder_decoder_path=sd, spatial_batch_size=1000,
                  random_seed=42, SEA_isolate=True, SEA_mixed=False, case_name="synth", run_name="fixture", dtype_spatial=dtype)
    fields, xy = gpu(g["fields"]), gpu(g["xy"])                                   # [tr, T+1, N, F], [2, N]
    if n_points is not None:
        fields, xy = fields[:, :, :n_points].contiguous(), xy[:, :n_points].contiguous()
    mp_ = MeshProcessor(config, xy)
    _, scaled = mp_.patchify_and_scale(fields.reshape(tr * (T + 1), fields.shape[2], fields.shape[3]), train_indices=np.arange(1))
    if n_points is None:
        assert scaled.shape[2] == n_inp and torch.equal(scaled.cpu(), torch.from_numpy(g["scaled"]))   # no scaling in the shipped configs: a pure gather
    proc = ProcessData(n_inp, config)
    z = proc.initialize_and_process_data(scaled.permute(0, 1, 3, 2).contiguous())
    P = (m_ - 1) * (n_ - 1)
    enc = transform_processed_data(z, tr, T + 1, P, len(groups))
    cond = gpu(g["cond"])
    ds = TemporalDataset([enc[i] for i in range(tr)], [fields[i] for i in range(tr)], [cond[i] for i in range(tr)], src_len=T, overlap=0)
    loader = [ds.batch(range(len(ds)))]
    return g, config, mp_, proc, z, enc, loader


@pytest.mark.parametrize("mode", ["recompute", "kv"])
def test_temporal_test_verb_matches_reference_golden(tmp_path, mode):
    from sea_amd.utils.train_utils import SeaMSELoss, autoregressive_validation, full_autoregressive_evaluation

    g, config, mp_, proc, z, enc, loader = _eval_setup(tmp_path)
    assert rel_l2(z.cpu().numpy(), g["z"]) < 1e-4 and rel_l2(enc.cpu().numpy(), g["enc"]) < 1e-4
    cfg = cfg_from_meta(g["cfg"])
    model = build(cfg, "fp32")
    config["rollout_mode"] = model.rollout_mode = mode
    res = full_autoregressive_evaluation(model, loader, SeaMSELoss(), torch.device("cuda"), proc, mp_, config, 0, plot_traj=False)
    assert abs(res["encoded_rel_mse"] - float(g["encoded_rel_mse"])) < 2e-4 * float(g["encoded_rel_mse"])
    assert abs(res["decoded_rel_mse"] - float(g["decoded_rel_mse"])) < 5e-4 * float(g["decoded_rel_mse"])
    table = np.loadtxt(os.path.join(str(tmp_path), "rollout_error_synth_fixture.csv"), delimiter=",", skiprows=1)[:, 1:]
    assert rel_l2(table, g["decoded_per_step"]) < 5e-4
    v_loss, v_rel = autoregressive_validation(model, loader, SeaMSELoss(), torch.device("cuda"))
    assert abs(v_loss - float(g["val_loss"])) < 2e-4 * float(g["val_loss"]) and abs(v_rel - float(g["val_rel_mse_time"])) < 2e-4 * float(g["val_rel_mse_time"])
    # without the processors the decoded figure is NaN, the encoded one unchanged
    res2 = full_autoregressive_evaluation(model, loader, SeaMSELoss(), torch.device("cuda"), None, None, config, 0, plot_traj=False)
    assert res2["encoded_rel_mse"] == res["encoded_rel_mse"] and res2["decoded_rel_mse"] != res2["decoded_rel_mse"]


def test_temporal_test_verb_bf16_within_stated_tolerance(tmp_path):
    from sea_amd.utils.train_utils import SeaMSELoss, full_autoregressive_evaluation

    g, config, mp_, proc, z, enc, loader = _eval_setup(tmp_path, dtype="bf16")
    assert rel_l2(z.cpu().numpy(), g["z"]) < 3e-2
    model = build(cfg_from_meta(g["cfg"]), "bf16")
    res = full_autoregressive_evaluation(model, loader, SeaMSELoss(), torch.device("cuda"), proc, mp_, config, 0, plot_traj=False)
    assert abs(res["encoded_rel_mse"] - float(g["encoded_rel_mse"])) < 0.1 * float(g["encoded_rel_mse"])
    assert abs(res["decoded_rel_mse"] - float(g["decoded_rel_mse"])) < 0.1 * float(g["decoded_rel_mse"])


@pytest.mark.parametrize("n_points", [417, 418, 419])
def test_temporal_test_verb_on_ragged_mesh(tmp_path, n_points):
    """A mesh whose point count is not a multiple of 4: the evaluation takes relativeMSE over the points (dim=2) of the decoded fields.  It returns
    finite numbers, and decoded_rel_mse is the fp64 formula applied to the same decoded fields, taken from the mesh processor outside the loop."""
    from oracle.sea_oracle import relative_mse
    from sea_amd.utils.train_utils import SeaMSELoss, full_autoregressive_evaluation, inverse_transform_processed_data, rollout

    g, config, mp_, proc, z, enc, loader = _eval_setup(tmp_path, n_points=n_points)
    model = build(cfg_from_meta(g["cfg"]), "fp32")
    config["rollout_mode"] = model.rollout_mode = "kv"
    res = full_autoregressive_evaluation(model, loader, SeaMSELoss(), torch.device("cuda"), proc, mp_, config, 0, plot_traj=False)
    assert np.isfinite(res["encoded_rel_mse"]) and np.isfinite(res["decoded_rel_mse"])
    data, target, original, ib = loader[0]
    tr, T = target.shape[0], target.shape[1]
    with torch.no_grad():
        pred = rollout(model, data[:, 0:1].contiguous(), ib, T, mode="kv")
        zz = inverse_transform_processed_data(pred, tr, T, (config["m"] - 1) * (config["n"] - 1), len(config["field_groups"]))
        fields = mp_.decode_and_unpatch(proc.decoder(), zz)
    fields = fields.reshape(tr, T, fields.shape[1], fields.shape[2])
    assert fields.shape[2] == n_points
    want = float(relative_mse(fields.double(), original.double(), dim=2).mean(dim=0).mean())
    assert abs(res["decoded_rel_mse"] - want) <= 1e-5 * want, (res["decoded_rel_mse"], want)


@pytest.mark.parametrize("name", ["rollout8_adaln_f3", "rollout100_ln_f2"])
def test_autoregressive_validation_matches_reference_golden(name):
    """The reference's own scalars of its validation loop (first sample of the first batch, utils/train_utils.py:154-184) stored with the rollout goldens."""
    from sea_amd.utils.train_utils import SeaMSELoss, autoregressive_validation

    g = load_golden(name)
    model = build(cfg_from_meta(g["cfg"]), "fp32")
    x0, tgt, ib = gpu(g["x0"]), gpu(g["tgt"]), gpu(g["ib"])
    data = torch.cat((x0, tgt[:, :-1]), dim=1)          # only data[:, 0] is read by the loop
    v_loss, v_rel = autoregressive_validation(model, [(data, tgt, None, ib)], SeaMSELoss(), torch.device("cuda"))
    assert abs(v_loss - float(g["val_loss"])) < 5e-4 * float(g["val_loss"])
    assert abs(v_rel - float(g["val_rel_mse_time"])) < 5e-4 * float(g["val_rel_mse_time"])


def test_train_entry_point_on_synthetic_loaders(tmp_path):
    """train(config, error_tracker) with the config mirror's keys (get_model consumes the reference's 17 positional keys), DataLoader-like lists of
    (data, target, original, ib) batches: the loss falls, both checkpoints are written under the reference's file names in the reference's
    state_dict schema (a fresh TemporalModel loads them strictly and reproduces the trained model's output)."""
    from sea_amd.configs import get_config
    from sea_amd.models.temporal import TemporalModel
    from sea_amd.train.train_temporal import get_model, train
    from sea_amd.utils.train_utils import NoOpErrorTracker

    config = get_config("cylinder_flow", "temporal")
    config.update(device="cuda", save_dir=str(tmp_path), embed_dim=64, n_heads=4, block_size=32, num_fields=3, dropout=0.0, dtype="fp32", learning_rate=2e-3,
                  epoch_num=8, validation_interval=2, full_eval_interval=4, run_name="t", rollout_mode="kv")
    torch.manual_seed(3)
    base = torch.randn(4, 13, 3, 64).cumsum(dim=1) * 0.1
    ib = torch.rand(4, 13, 1)
    batch = lambda sl: (base[sl, :-1].cuda(), base[sl, 1:].cuda(), base[sl, 1:].cuda(), ib[sl, :-1].cuda())   # noqa: E731
    config["loaders"] = ([batch(slice(0, 2)), batch(slice(2, 3))], [batch(slice(3, 4))], [batch(slice(3, 4))])

    class Tracker(NoOpErrorTracker):
        def __init__(self):
            self.rows = []

        def record_error(self, phase, epoch, metrics):
            self.rows.append((phase, epoch, dict(metrics)))

    tr = Tracker()
    model = train(config, tr)
    train_losses = [m["Loss"] for ph, _, m in tr.rows if ph == "train"]
    assert len(train_losses) == 8 and train_losses[-1] < 0.8 * train_losses[0], train_losses
    assert any("Full_Encoded_Rel_MSE" in m for ph, _, m in tr.rows if ph == "val")
    for fname in ("temporal_cylinder_flow_t.pt", "temporal_Checkpoint_cylinder_flow_t.pt"):
        path = os.path.join(str(tmp_path), fname)
        assert os.path.exists(path), fname
        sd = torch.load(path, map_location="cpu")
        fresh = TemporalModel(1, 64, 4, 32, 8, 0, 3, 2, 0.0, "sea", "learnable", "mlp", "add", 1, 1, True, "adaln")
        fresh.load_state_dict(sd, strict=True)
    m2, loss_fn, opt = get_model(dict(config, load_pretrained=True, pretrained_model_path=os.path.join(str(tmp_path), "temporal_cylinder_flow_t.pt")), torch.device("cuda"))
    x, _, _, c = config["loaders"][1][0]
    with torch.no_grad():
        # the best-validation checkpoint is an earlier or equal state of `model`: compare with a model that loads the same file
        m3, _, _ = get_model(dict(config, load_pretrained=True, pretrained_model_path=os.path.join(str(tmp_path), "temporal_cylinder_flow_t.pt")), torch.device("cuda"))
        assert torch.equal(m2.eval()(x, c), m3.eval()(x, c))
    assert type(opt).__name__ == "FlatAdamW" and callable(loss_fn)
