"""Training path on the MI355X: hand-written backward + flat AdamW against the gradients and post-step parameters the REFERENCE
produced (tests/golden/model_tiny_*.npz) and against the CPU oracle's autograd at a larger shape."""
import numpy as np
import pytest
import torch

from oracle import sea_oracle as O
from oracle.recipe import recipe_inputs, recipe_params
from tests.conftest import cfg_from_meta, grad_err, load_golden, rel_l2
from tests.test_model_gpu import build, gpu

pytestmark = pytest.mark.gpu

TRAIN_CASES = ["model_tiny_adaln_f3", "model_tiny_ln_f2", "model_tiny_adaln_f2_pre"]
# the ablation variants of the block (reference models/temporal.py:285-312, 103-116): 'addition' / 'simple' exchange, the info-bottleneck
# layer not added ('none'), as nn.Linear ('linear') or as fixed Fourier features ('fourier'), the 'pool' exchange (a pooled token per row; also with one field), the info-bottleneck rows attended to instead of added ('attention') or concatenated to the block's rows ('concat'; the second case also has ONE field in 'addition' mode)
VARIANT_TRAIN_CASES = ["train_addition_adaln_f3", "train_simple_ln_f2", "train_sea_noib_adaln_f2", "train_sea_linear_ln_f2_pre", "train_addition_fourier_adaln_f3",
                       "train_pool_adaln_f3", "train_pool_ln_f1", "train_ibattn_adaln_f3", "train_ibattn_ln_f2_pre",
                       "train_ibconcat_ln_f2", "train_ibconcat_adaln_f1"]


@pytest.mark.parametrize("name", TRAIN_CASES + VARIANT_TRAIN_CASES)
def test_gradients_match_reference_golden_fp32(name):
    """The reference's own train-step sequence (zero_grad, forward, MSELoss, backward) through the drop-in surface."""
    from sea_amd.utils.train_utils import SeaMSELoss

    g = load_golden(name)
    cfg = cfg_from_meta(g["cfg"])
    m = build(cfg, "fp32").train()
    x, tgt, ib = gpu(g["x"]), gpu(g["tgt"]), gpu(g["ib"])
    out = m(x, ib)
    assert rel_l2(out.detach().cpu().numpy(), g["out_train"]) < 1e-4
    loss = SeaMSELoss()(out, tgt)
    assert abs(loss.item() - float(g["losses"][0])) < 1e-5 * abs(float(g["losses"][0]))
    loss.backward()
    dead = set(str(k) for k in g["dead_keys"])
    worst, worst_k = 0.0, None
    for k, p in m.named_parameters():
        if k in dead:
            assert p.grad is None, k  # exactly the reference's set of gradient-less parameters
            continue
        assert p.grad is not None, k
        e = grad_err(p.grad.cpu().numpy(), g["grad:" + k])
        if e > worst:
            worst, worst_k = e, k
    assert worst < 1e-4, (worst_k, worst)


@pytest.mark.parametrize("name", TRAIN_CASES)
def test_adamw_steps_match_reference_golden_fp32(name):
    from sea_amd.utils.train_utils import SeaMSELoss, initialize_optimizer

    g = load_golden(name)
    cfg = cfg_from_meta(g["cfg"])
    m = build(cfg, "fp32").train()
    opt = initialize_optimizer(m, {"learning_rate": float(g["lr"])})
    loss_fn = SeaMSELoss()
    x, tgt, ib = gpu(g["x"]), gpu(g["tgt"]), gpu(g["ib"])
    dead = set(str(k) for k in g["dead_keys"])
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    losses = []
    for step in range(1, 4):
        opt.zero_grad()
        loss = loss_fn(m(x, ib), tgt)
        loss.backward()
        opt.step()
        losses.append(loss.item())
        if step in (1, 3):
            for k, p in m.named_parameters():
                if k in dead:
                    assert torch.equal(p, before[k]), k
                else:
                    # compare the UPDATE (param - initial): the parameters themselves barely move in 3 steps.
                    # Key biases are excluded: softmax is invariant to a per-row constant, so d loss / d k.bias is exactly zero in
                    # exact arithmetic and Adam turns its rounding noise (~1e-9) into +-lr steps, in the reference as much as here.
                    if not k.endswith(".k.bias"):
                        ref_delta = g[f"param{step}:" + k] - before[k].cpu().numpy()
                        delta = (p.detach() - before[k]).cpu().numpy()
                        # step 1 of Adam is lr * g / (|g| + eps): elements whose gradient is of the order of eps (1e-8) turn fp32 rounding of
                        # the gradient into O(lr) differences, hence 5e-3 and not the gradients' own 1e-4
                        assert rel_l2(delta, ref_delta) < (5e-3 if step == 1 else 2e-2), (k, step)
                    assert rel_l2(p.detach().cpu().numpy(), g[f"param{step}:" + k]) < (2e-5 if not k.endswith(".k.bias") else 5e-2), (k, step)
    assert np.allclose(losses, g["losses"], rtol=1e-4)


def test_fused_train_step_equals_autograd_path():
    from sea_amd.utils.train_utils import SeaMSELoss, initialize_optimizer

    g = load_golden("model_tiny_adaln_f3")
    cfg = cfg_from_meta(g["cfg"])
    x, tgt, ib = gpu(g["x"]), gpu(g["tgt"]), gpu(g["ib"])
    ma, mb = build(cfg, "fp32").train(), build(cfg, "fp32").train()
    oa, ob = initialize_optimizer(ma, {"learning_rate": 1e-3}), initialize_optimizer(mb, {"learning_rate": 1e-3})
    for _ in range(2):
        oa.zero_grad()
        SeaMSELoss()(ma(x, ib), tgt).backward()
        oa.step()
        loss_b = mb.engine().train_step(x, tgt, ib, ob)
    for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        # .k.bias has a mathematically zero gradient (softmax is shift-invariant per query): Adam normalises the atomics-order
        # rounding noise to O(lr), so the two paths agree only to that noise there.
        assert rel_l2(pb.detach().cpu().numpy(), pa.detach().cpu().numpy()) < (1e-6 if not k.endswith(".k.bias") else 1e-4), k
    assert np.isfinite(loss_b.item())


@pytest.mark.parametrize("dtype,tol", [("fp32", 2e-4), ("bf16", 6e-2)])
def test_gradients_match_oracle_larger_shape(dtype, tol):
    """E=128, F=3, L=2, B=3, T=70 (multi-tile attention, two layers) against the CPU oracle's autograd."""
    cfg = O.OracleConfig(2, 128, 4, 96, 8, 0, 3, 2, True, "adaln")
    p = recipe_params(cfg)
    x, tgt, ib = recipe_inputs(3, 70, cfg, seed=77)
    _, loss_ref, grads_ref = O.loss_and_grads(x, ib, tgt, p, cfg)
    m = build(cfg, dtype).train()
    eng = m.engine()
    out, plan = eng.forward_train(x.cuda(), ib.cuda())
    loss, dout = eng.mse_loss_and_grad(out, tgt.cuda())
    eng.zero_grads()
    eng.backward(plan, dout)
    assert abs(loss.item() - float(loss_ref)) < tol * float(loss_ref)
    num = den = 0.0
    worst, worst_k = 0.0, None
    for k, gr in grads_ref.items():
        mine = eng.grad_view(k).cpu()
        num += float((mine.double() - gr.double()).pow(2).sum())
        den += float(gr.double().pow(2).sum())
        e = rel_l2(mine.numpy(), gr.numpy())
        if e > worst:
            worst, worst_k = e, k
    assert (num / den) ** 0.5 < tol, ((num / den) ** 0.5)
    assert worst < 10 * tol, (worst_k, worst)


@pytest.mark.parametrize("dtype,tol", [("bf16", 6e-2), ("fp32", 1e-4)])
def test_gradients_at_multiphase_width_head_dim_256(dtype, tol):
    """embed_dim 2048, 8 heads (the shipped multiphase_flow dims: self-attention head dim 256, cross 128, MLP hidden 16384), LayerNorm without
    modulation, two fields: forward + backward against the CPU oracle's fp32 autograd (T = 40: one key tile, every width-dependent path of
    the row passes and GEMMs).  bf16 <= 6e-2 / fp32 <= 1e-4 over all parameters together, each within 10x of that."""
    cfg = O.OracleConfig(1, 2048, 8, 48, 8, 0, 2, 2, True, "ln")
    p = recipe_params(cfg)
    x, tgt, ib = recipe_inputs(1, 40, cfg, seed=5)
    _, loss_ref, grads_ref = O.loss_and_grads(x, ib, tgt, p, cfg)
    m = build(cfg, dtype).train()
    eng = m.engine()
    out, plan = eng.forward_train(x.cuda(), ib.cuda())
    loss, dout = eng.mse_loss_and_grad(out, tgt.cuda())
    eng.zero_grads()
    eng.backward(plan, dout)
    assert abs(loss.item() - float(loss_ref)) < tol * float(loss_ref)
    num = den = 0.0
    worst, worst_k = 0.0, None
    for k, gr in grads_ref.items():
        mine = eng.grad_view(k).cpu()
        num += float((mine.double() - gr.double()).pow(2).sum())
        den += float(gr.double().pow(2).sum())
        e = rel_l2(mine.numpy(), gr.numpy())
        if e > worst:
            worst, worst_k = e, k
    print(f"multiphase width {dtype} gradients: overall rel-L2 {(num / den) ** 0.5:.3e}, worst {worst_k} {worst:.3e}")
    assert (num / den) ** 0.5 < tol
    assert worst < 10 * tol, (worst_k, worst)
    assert sorted(eng.params.live_names) == sorted(grads_ref.keys())


@pytest.mark.parametrize("dtype,tol", [("bf16", 6e-2), ("fp32", 1e-4)])
def test_gradients_at_cylinder_width(dtype, tol):
    """embed_dim 1024, 8 heads, AdaLN, two field groups, two trajectories (the shipped cylinder_flow dims and batch: self-attention head dim 128, cross 64, MLP hidden
    8192, condition MLPs of 2048 / 1024 columns), T = 72 (two key tiles): forward + backward against the CPU oracle's fp32 autograd — the widths at which the
    round-3 backward kernels take their wide forms (rows of 8192 through rownorm_bwd_wide_kernel, the column-block backward of cond_mlp.0 + SiLU and of the
    info-bottleneck MLP with four column blocks).  bf16 <= 6e-2 / fp32 <= 1e-4 over all parameters together, each within 10x of that."""
    cfg = O.OracleConfig(1, 1024, 8, 80, 8, 0, 2, 2, True, "adaln")
    p = recipe_params(cfg)
    x, tgt, ib = recipe_inputs(2, 72, cfg, seed=15)
    _, loss_ref, grads_ref = O.loss_and_grads(x, ib, tgt, p, cfg)
    m = build(cfg, dtype).train()
    eng = m.engine()
    out, plan = eng.forward_train(x.cuda(), ib.cuda())
    loss, dout = eng.mse_loss_and_grad(out, tgt.cuda())
    eng.zero_grads()
    eng.backward(plan, dout)
    assert abs(loss.item() - float(loss_ref)) < tol * float(loss_ref)
    num = den = 0.0
    worst, worst_k = 0.0, None
    for k, gr in grads_ref.items():
        mine = eng.grad_view(k).cpu()
        num += float((mine.double() - gr.double()).pow(2).sum())
        den += float(gr.double().pow(2).sum())
        e = rel_l2(mine.numpy(), gr.numpy())
        if e > worst:
            worst, worst_k = e, k
    print(f"cylinder width {dtype} gradients: overall rel-L2 {(num / den) ** 0.5:.3e}, worst {worst_k} {worst:.3e}")
    assert (num / den) ** 0.5 < tol
    assert worst < 10 * tol, (worst_k, worst)
    assert sorted(eng.params.live_names) == sorted(grads_ref.keys())


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-4), ("bf16", 6e-2)])
def test_cfg3_shape_gradients_match_reference_golden(dtype, tol):
    """BASELINE.json configs[2] at one trajectory (E=256, H=8, F=3, T=2024: every multi-tile path of the backward — 128-row weight-gradient
    tiles, multi-tile attention backward, grid-capped row passes) against the REFERENCE's train step (tests/golden/cfg3_train.npz:
    train/train_temporal.py:254-258 run on CPU): loss, train-mode output, the set of gradient-less parameters, and every live parameter's
    gradient by its L2 norm and a strided sub-sample.  fp32 <= 1e-4 (north_star); bf16 <= 6e-2 relative L2 over all sub-samples together
    (bf16 operands, fp32 accumulation), each parameter within 10x of that."""
    from tests.conftest import grad_sub_stride

    g = load_golden("cfg3_train")
    cfg = cfg_from_meta(g["cfg"])
    x, tgt, ib = recipe_inputs(1, 2024, cfg, seed=int(g["seed"]))
    m = build(cfg, dtype).train()
    eng = m.engine()
    out, plan = eng.forward_train(x.cuda(), ib.cuda())
    loss, dout = eng.mse_loss_and_grad(out, tgt.cuda())
    eng.zero_grads()
    eng.backward(plan, dout)
    assert abs(loss.item() - float(g["loss"])) < tol * float(g["loss"])
    assert rel_l2(out[:, ::97, :, ::13].cpu().numpy(), g["out_sub"]) < (tol if dtype == "fp32" else 3e-2)
    dead = set(str(k) for k in g["dead_keys"])
    assert dead == set(k for k, _ in m.named_parameters()) - set(eng.params.live_names)
    num = den = 0.0
    worst, worst_k = 0.0, None
    for k, l2 in zip((str(k) for k in g["grad_keys"]), g["grad_l2"]):
        mine = eng.grad_view(k).reshape(-1)
        ref = g["gsub:" + k]
        sub = mine[:: grad_sub_stride(mine.numel())].cpu().double().numpy()
        num += float(((sub - ref) ** 2).sum())
        den += float((ref.astype(np.float64) ** 2).sum())
        assert abs(float(mine.double().norm()) - l2) < (2e-4 if dtype == "fp32" else 6e-2) * l2, (k, float(mine.double().norm()), l2)
        e = rel_l2(sub, ref)
        if e > worst:
            worst, worst_k = e, k
    assert (num / den) ** 0.5 < tol, (num / den) ** 0.5
    assert worst < 10 * tol, (worst_k, worst)
    # the AdamW step on those gradients (fp32): parameters after one step against the reference's, on the same sub-sample
    if dtype == "fp32":
        from sea_amd.utils.train_utils import initialize_optimizer

        opt = initialize_optimizer(m, {"learning_rate": 1e-4})
        opt.step()
        for k in (str(k) for k in g["grad_keys"]):
            q = eng.params.f32(k).reshape(-1)
            assert rel_l2(q[:: grad_sub_stride(q.numel())].cpu().numpy(), g["p1sub:" + k]) < 2e-4, k


_CFG3_ORACLE = {}


def _cfg3_oracle_b8():
    """BASELINE.json configs[2] at ITS OWN batch on the host: loss and gradients of the CPU oracle for B = 8 trajectories of T = 2024 (E=256, H=8, F=3, AdaLN).
    The loss is a mean over all elements, so the batch gradient is the mean of the per-trajectory gradients: one trajectory at a time keeps the oracle's
    materialised [H, T, T] score tensors at 5 GB instead of 40 (about a minute of CPU on the box's cores).  Cached for both dtypes."""
    if not _CFG3_ORACLE:
        cfg = O.OracleConfig(1, 256, 8, 2024, 8, 0, 3, 2, True, "adaln")
        x, tgt, ib = recipe_inputs(8, 2024, cfg, seed=808)
        p = recipe_params(cfg)
        loss, grads = 0.0, {}
        for b in range(8):
            _, lb, gb = O.loss_and_grads(x[b:b + 1], ib[b:b + 1], tgt[b:b + 1], p, cfg)
            loss += float(lb) / 8
            for k, g in gb.items():
                grads[k] = grads.get(k, 0) + g.double() / 8
        _CFG3_ORACLE.update(cfg=cfg, x=x, tgt=tgt, ib=ib, loss=loss, grads=grads)
    return _CFG3_ORACLE


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-4), ("bf16", 6e-2)])
def test_cfg3_own_batch_gradients_match_oracle(dtype, tol):
    """BASELINE.json configs[2] at its own size — B = 8 trajectories, T = 2024 — against the ORACLE (not against another driver of the same kernels): the
    fused step's forward + MSE + backward (engine.forward_train / mse_loss_and_grad / backward: what engine.train_step runs in front of the optimizer)
    gives the oracle's loss and, on the golden files' strided sub-samples (tests/conftest.py::grad_sub_stride), the oracle's gradient of every live
    parameter: fp32 <= 1e-4 relative L2 over all sub-samples together (north_star's bar), bf16 <= 6e-2; every single parameter within 10x of that; the
    norm of every gradient within the same bar.  Reference step: train/train_temporal.py:254-258."""
    from tests.conftest import grad_sub_stride

    R = _cfg3_oracle_b8()
    cfg = R["cfg"]
    m = build(cfg, dtype).train()
    eng = m.engine()
    out, plan = eng.forward_train(R["x"].cuda(), R["ib"].cuda())
    loss, dout = eng.mse_loss_and_grad(out, R["tgt"].cuda())
    eng.zero_grads()
    eng.backward(plan, dout)
    assert abs(loss.item() - R["loss"]) < tol * R["loss"]
    assert set(R["grads"]) == set(eng.params.live_names)
    num = den = 0.0
    worst, worst_k = 0.0, None
    for k, ref_full in R["grads"].items():
        mine = eng.grad_view(k).reshape(-1).cpu().double()
        ref_full = ref_full.reshape(-1)
        st = grad_sub_stride(mine.numel())
        sub, ref = mine[::st].numpy(), ref_full[::st].numpy()
        num += float(((sub - ref) ** 2).sum())
        den += float((ref ** 2).sum())
        assert abs(float(mine.norm()) - float(ref_full.norm())) < (2e-4 if dtype == "fp32" else 6e-2) * float(ref_full.norm()), k
        e = rel_l2(sub, ref)
        if e > worst:
            worst, worst_k = e, k
    assert (num / den) ** 0.5 < tol, (num / den) ** 0.5
    assert worst < 10 * tol, (worst_k, worst)


def test_cfg3_full_size_fused_step_equals_autograd_path_and_replays():
    """cfg3 at its own size (B=8 trajectories, T=2024, bf16): the fused train_step against the autograd path (same kernels, different driver),
    and two replays of forward + backward on the same inputs: outputs bit-identical, gradients equal up to the order of the fp32 atomics of
    the weight-gradient kernel."""
    from sea_amd.utils.train_utils import SeaMSELoss, initialize_optimizer

    cfg = O.OracleConfig(1, 256, 8, 2024, 8, 0, 3, 2, True, "adaln")
    x, tgt, ib = recipe_inputs(8, 2024, cfg, seed=808)
    x, tgt, ib = x.cuda(), tgt.cuda(), ib.cuda()
    ma, mb = build(cfg, "bf16").train(), build(cfg, "bf16").train()
    oa, ob = initialize_optimizer(ma, {"learning_rate": 1e-4}), initialize_optimizer(mb, {"learning_rate": 1e-4})
    oa.zero_grad()
    la = SeaMSELoss()(ma(x, ib), tgt)
    la.backward()
    ga = ma.engine().grads.clone()
    oa.step()
    lb = mb.engine().train_step(x, tgt, ib, ob)
    gb = mb.engine().grads.clone()
    assert abs(la.item() - lb.item()) < 1e-6 * abs(la.item())
    n_live = ma.engine().params.n_live
    assert rel_l2(gb[:n_live].cpu().numpy(), ga[:n_live].cpu().numpy()) < 1e-5
    for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        # one Adam step moves every element by about +-lr whatever the gradient's size: elements whose gradient is rounding noise may flip sign
        # between two orders of the atomics, so the parameters are compared through the update's size (lr = 1e-4 against weights of ~2e-2)
        assert float((pa.detach() - pb.detach()).abs().max()) <= 2.5e-4, k
    eng = mb.engine()
    outs, grads = [], []
    for _ in range(2):
        out, plan = eng.forward_train(x, ib)
        loss, dout = eng.mse_loss_and_grad(out, tgt)
        eng.zero_grads()
        eng.backward(plan, dout)
        torch.cuda.synchronize()
        outs.append(out.clone())
        grads.append(eng.grads[:n_live].clone())
    assert torch.equal(outs[0], outs[1])
    assert rel_l2(grads[1].cpu().numpy(), grads[0].cpu().numpy()) < 1e-5


def test_bf16_training_reduces_loss():
    from sea_amd.utils.train_utils import initialize_optimizer

    cfg = O.OracleConfig(1, 64, 4, 48, 8, 0, 3, 2, True, "adaln")
    m = build(cfg, "bf16").train()
    opt = initialize_optimizer(m, {"learning_rate": 2e-3})
    x, tgt, ib = recipe_inputs(4, 40, cfg, seed=5)
    x, tgt, ib = x.cuda(), tgt.cuda(), ib.cuda()
    eng = m.engine()
    losses = [eng.train_step(x, tgt, ib, opt).item() for _ in range(30)]
    assert losses[-1] < 0.7 * losses[0], losses[::5]


def _doubled_gradients_agree(names, g1, g2, dtype):
    """g2 = 2 g1 for every live parameter, by name, to the noise of the atomics' order; .k.bias (a mathematically zero gradient: see the comment in
    test_fused_train_step_equals_autograd_path) absolutely, against the largest gradient norm in the model."""
    top = max(float(g1[k].double().norm()) for k in names)
    for k in names:
        a, b = g2[k].double(), 2 * g1[k].double()
        if k.endswith(".k.bias"):
            assert float((a - b).norm()) <= 2e-5 * top, (dtype, k, float((a - b).norm()), top)
        else:
            assert float((a - b).norm()) <= 2e-5 * float(b.norm()), (dtype, k, float((a - b).norm() / b.norm()))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_second_backward_without_zeroing_adds(dtype):
    """Gradient accumulation: a backward into a buffer that already holds a microbatch's gradients must ADD everywhere.  The field MLP's weight-gradient
    launches store instead of adding when the buffer holds zeros (SeaWgradGroup.overwrite, set per run from grads_dirty): a flag left on would silently
    discard the first microbatch's fc1 / fc2 gradients.  Through the engine and through the module surface (two loss.backward() without zero_grad())."""
    from sea_amd.utils.train_utils import SeaMSELoss

    cfg = O.OracleConfig(2, 128, 4, 96, 8, 0, 3, 2, True, "adaln")
    x, tgt, ib = recipe_inputs(2, 70, cfg, seed=78)
    x, tgt, ib = x.cuda(), tgt.cuda(), ib.cuda()
    m = build(cfg, dtype).train()
    eng = m.engine()
    names = list(eng.params.live_names)

    def fwd_bwd():
        out, plan = eng.forward_train(x, ib)
        _, dout = eng.mse_loss_and_grad(out, tgt)
        eng.backward(plan, dout)
        sole = plan.__dict__.get("_sole_wgrads", [])
        assert len(sole) > 0
        return [int(g.overwrite) for g in sole]

    eng.zero_grads()
    assert set(fwd_bwd()) == {1}
    g1 = {k: eng.grad_view(k).clone() for k in names}
    assert any(k.endswith(".k.bias") for k in names) and all(torch.isfinite(v).all() for v in g1.values())
    eng.zero_grads()
    assert set(fwd_bwd()) == {1}
    assert set(fwd_bwd()) == {0}
    _doubled_gradients_agree(names, g1, {k: eng.grad_view(k).clone() for k in names}, dtype)

    m2 = build(cfg, dtype).train()
    for _ in range(2):
        SeaMSELoss()(m2(x, ib), tgt).backward()
    named = dict(m2.named_parameters())
    assert list(m2.engine().params.live_names) == names and all(named[k].grad is not None for k in names)
    _doubled_gradients_agree(names, g1, {k: named[k].grad for k in names}, dtype)
    sole = m2.engine().train_plan(2, 70).__dict__.get("_sole_wgrads", [])
    assert len(sole) > 0 and {int(g.overwrite) for g in sole} == {0}
