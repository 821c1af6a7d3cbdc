"""Attention at head dims that are multiples of 8 but not powers of two (the masked kernels of attention.hip / attention_bwd.hip), from the op level up to the
whole model: forward, dropout and backward against plain fp32 PyTorch, TemporalModel at embed_dim 384 / 768 over 8 heads (self head dims 48 / 96, cross 24 / 48)
against the CPU oracle and a reference-generated golden, the KV-cache rollout, HIP-graph replay, the optional plan forms and the data-parallel step."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import sea_oracle as O
from oracle.recipe import recipe_inputs, recipe_params
from tests.conftest import cfg_from_meta, grad_err, load_golden, rel_l2
from tests.test_bwd_ops_gpu import _attention_backward_case
from tests.test_dropout_gpu import test_attention_dropout_forward_backward as _dropout_case
from tests.test_model_gpu import BF16_TOL, FP32_TOL, build, gpu
from tests.test_ops_gpu import attention_ref, dev, rel, rnd, tol

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
HDS = [24, 40, 48, 56, 80, 96, 120, 160, 192, 224, 248]


# ---------------------------------------------------------------------------------------------------- op level
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("Tq,Tk,q_pos0,src_len,cap", [(70, 70, 0, 0, 72), (130, 130, 0, 3, 136), (5, 77, 72, 0, 80), (1, 40, 39, 0, 48), (65, 65, 0, 0, 96)])
def test_attention_forward(dtype, hd, Tq, Tk, q_pos0, src_len, cap):
    """Causal with and without src_len, Tq != Tk with q_pos0 > 0 (a cache step of 5 rows; Tq = 1: the tiled kernel), cap > Tk, T not a multiple of 64.  The key / value
    padding past Tk is poisoned, and O is a column slice of a wider buffer whose trailing columns must stay untouched."""
    from sea_amd import ops

    B, H = 2, 3
    Q = rnd(B, H, Tq, hd, dtype=dtype, scale=hd ** -0.25, seed=60)
    K = rnd(B, H, cap, hd, dtype=dtype, scale=hd ** -0.25, seed=61)
    Vt = rnd(B, H, hd, cap, dtype=dtype, seed=62)
    K[:, :, Tk:] = float("nan")
    Vt[:, :, :, Tk:] = float("nan")
    wide = torch.full((B, Tq, H * hd + 8), 7.0, device=dev(), dtype=dtype)
    O = wide[:, :, : H * hd]
    O.fill_(float("nan"))
    LSE = torch.empty(B, H, Tq, device=dev())
    ops.attention_fwd([dict(Q=Q, K=K, Vt=Vt, O=O, LSE=LSE)], B, H, hd, Tq, Tk, cap, q_pos0, src_len, dtype)
    Oref, lse_ref = attention_ref(Q, K, Vt, q_pos0, src_len, Tk)
    assert torch.isfinite(O.float()).all()
    assert torch.all(wide[:, :, H * hd:] == 7.0)
    assert rel(O.float(), Oref) < tol(dtype, f32=2e-5, bf16=8e-3)
    assert rel(LSE, lse_ref) < tol(dtype, f32=1e-5, bf16=1e-3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", [48, 96])
def test_attention_forward_full_length(dtype, hd):
    """T = 2024 (cfg3's sequence length), and B * H * 32 query tiles = 4096 workgroups at hd 48: the paired, XCD-local form of compute width 64."""
    from sea_amd import ops

    B, H, T = 2, 8, 2024
    Q = rnd(B, H, T, hd, dtype=dtype, scale=hd ** -0.25, seed=1)
    K = rnd(B, H, T, hd, dtype=dtype, scale=hd ** -0.25, seed=2)
    Vt = rnd(B, H, hd, T, dtype=dtype, seed=3)
    O = torch.empty(B, T, H * hd, device=dev(), dtype=dtype)
    LSE = torch.empty(B, H, T, device=dev())
    ops.attention_fwd([dict(Q=Q, K=K, Vt=Vt, O=O, LSE=LSE)], B, H, hd, T, T, T, 0, 0, dtype)
    Oref, lse_ref = attention_ref(Q, K, Vt, 0, 0, T)
    assert rel(O.float(), Oref) < tol(dtype, f32=2e-5, bf16=8e-3)
    assert rel(LSE, lse_ref) < tol(dtype, f32=1e-5, bf16=1e-3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd,T", [(24, 70), (48, 130), (96, 70), (200, 70)])
def test_attention_dropout(dtype, hd, T):
    """The dropout forms (both kernels), masks reproduced through sea_dropout_mask: the checks of tests/test_dropout_gpu.py at the new widths."""
    _dropout_case(dtype, hd, T)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("T,src_len", [(1, 0), (70, 0), (200, 3)])
def test_attention_backward(dtype, hd, T, src_len):
    """dQ / dK / dV in [M, H*hd] with RoPE and the q scale undone, against torch autograd in fp32 (tests/test_bwd_ops_gpu.py's check)."""
    _attention_backward_case(dtype, hd, T, src_len, B=2, H=3)


@pytest.mark.parametrize("mode", [0, 3])
def test_attention_backward_full_length_both_orders(mode, monkeypatch):
    monkeypatch.setenv("SEA_TUNE", f"attnb_mode={mode}")
    _attention_backward_case(torch.bfloat16, 48, 2024, 0, B=1, H=2)


# ---------------------------------------------------------------------------------------------------- model level
MODELS = {"e384": (1, 384, 8, 40, 8, 0, 3, 2, True, "adaln"), "e768": (1, 768, 8, 40, 8, 0, 3, 2, True, "adaln"),
          "e384_pool": (1, 384, 8, 40, 8, 0, 3, 2, True, "ln", "pool")}


@pytest.mark.parametrize("name", list(MODELS))
def test_model_forward_gradients_and_rollouts(name):
    from sea_amd.utils.train_utils import rollout

    cfg = O.OracleConfig(*MODELS[name])
    p = recipe_params(cfg)
    x, _, ib = recipe_inputs(2, 24, cfg, seed=11)
    ref = O.model_forward(x, ib, p, cfg)
    for dtype, t in (("fp32", FP32_TOL), ("bf16", BF16_TOL)):
        with torch.no_grad():
            out = build(cfg, dtype)(x.cuda(), ib.cuda())
        assert rel_l2(out.cpu().numpy(), ref.numpy()) < t, dtype
    m = build(cfg, "fp32")
    a = rollout(m, x[:, :1].cuda(), ib.cuda(), 8, mode="recompute")
    assert rel_l2(a.cpu().numpy(), O.rollout(x[:, :1], ib, 8, p, cfg).numpy()) < FP32_TOL
    if cfg.exchange_mode == "pool":
        with pytest.raises(NotImplementedError, match="KV-cache"):
            m.engine().rollout_kv(x[:, :1].cuda(), ib.cuda(), 8)
    else:
        b = rollout(m, x[:, :1].cuda(), ib.cuda(), 8, mode="kv")
        assert rel_l2(b.cpu().numpy(), a.cpu().numpy()) < 1e-5
    m.train()
    _, loss_ref, grads_ref = O.loss_and_grads(x, ib, x * 0.5, p, cfg)
    eng = m.engine()
    out, plan = eng.forward_train(x.cuda(), ib.cuda())
    loss, dout = eng.mse_loss_and_grad(out, (x * 0.5).cuda())
    eng.zero_grads()
    eng.backward(plan, dout)
    assert abs(loss.item() - float(loss_ref)) < 1e-4 * float(loss_ref)
    for k, gr in grads_ref.items():
        assert grad_err(eng.grad_view(k).cpu().numpy(), gr.numpy()) < 2e-4, k


def test_model_matches_reference_golden():
    """tests/golden/make_headdim_fixtures.py: the reference's forward and recompute rollout at self / cross head dims 48 / 24."""
    from sea_amd.utils.train_utils import rollout

    g = load_golden("model_hd48_adaln_f3")
    m = build(cfg_from_meta(g["cfg"]), "fp32")
    with torch.no_grad():
        out = m(gpu(g["x"]), gpu(g["ib"]))
    assert rel_l2(out.cpu().numpy(), g["out"]) < FP32_TOL
    g = load_golden("model_hd48_rollout6_adaln_f3")
    m = build(cfg_from_meta(g["cfg"]), "fp32")
    n = g["tgt"].shape[1]
    for mode in ("recompute", "kv"):
        pred = rollout(m, gpu(g["x0"]), gpu(g["ib"]), n, mode=mode)
        assert rel_l2(pred.cpu().numpy(), g["pred"]) < 2e-4, mode


def test_graph_replay_and_kv_step_plan_forms(monkeypatch):
    """HIP-graph replay equals the plain replay; the KV-cache rollout through the generic step plan with and without the few-row launches."""
    from sea_amd.utils.train_utils import rollout

    cfg = O.OracleConfig(*MODELS["e384"])
    x, _, ib = recipe_inputs(2, 30, cfg, seed=5)
    x, ib = x.cuda(), ib.cuda()
    m = build(cfg, "bf16")
    eng = m.engine()
    with torch.no_grad():
        a = eng.forward(x, ib).clone()
        b = eng.forward_graphed(x, ib).clone()
    assert torch.equal(a, b)
    m32 = build(cfg, "fp32")
    ref = rollout(m32, x[:, :1], ib, 8, mode="kv")
    for env in ("gemv=0", "fast=0"):
        monkeypatch.setenv("SEA_KV", env)
        got = rollout(build(cfg, "fp32"), x[:, :1], ib, 8, mode="kv")
        assert rel_l2(got.cpu().numpy(), ref.cpu().numpy()) < 1e-5, env


@pytest.mark.parametrize("env,graphed", [("lanes=all", True), ("lanes=cond", True), ("norm=0", False), ("xtail=0", False), ("chain=0", False), ("silu=1", False),
                                         ("fold_ib=0", False), ("mlp1=1,mlp2=1", False), ("mlp1=1,mlp2=1,mlpblock=0", False), ("front=0", False)])
@pytest.mark.parametrize("dtype,t", [("fp32", 2e-6), ("bf16", 2e-2)])
def test_optional_plans_match_default_plan(env, graphed, dtype, t, monkeypatch):
    cfg = O.OracleConfig(2, 384, 8, 96, 8, 0, 3, 2, True, "adaln")
    x, _, ib = recipe_inputs(2, 70, cfg, seed=5)
    xg, ibg = x.cuda().contiguous(), ib.cuda().contiguous()
    with torch.no_grad():
        ref = build(cfg, dtype)(xg, ibg)
    monkeypatch.setenv("SEA_PLAN", env)
    m = build(cfg, dtype)
    with torch.no_grad():
        out = m.engine().forward_graphed(xg, ibg).clone() if graphed else m(xg, ibg)
    assert rel_l2(out.cpu().numpy(), ref.cpu().numpy()) < t


def test_model_training_with_attention_dropout():
    """Attention dropout in the training plan at hd 48 / 24: the hand-written backward matches a central finite difference with the step's seed held."""
    from sea_amd.models.temporal import TemporalModel

    cfg = O.OracleConfig(*MODELS["e384"])
    m = TemporalModel(1, 384, 8, 40, 8, 0, 3, 2, 0.1, "sea", "learnable", "mlp", "add", 1, 1, True, "adaln")
    p = recipe_params(cfg)
    with torch.no_grad():
        for k, prm in m.named_parameters():
            prm.copy_(p[k])
    m = m.to("cuda:0").train()
    x, tgt, ib = (t_.cuda() for t_ in recipe_inputs(2, 24, cfg, seed=3))
    eng = m.engine()

    def loss_at(s, direction):
        eng._drop_step = 1000
        with torch.no_grad():
            eng.params.flat32[: eng.params.n_live].add_(direction, alpha=s)
            out, plan = eng.forward_train(x, ib)
            loss, dout = eng.mse_loss_and_grad(out, tgt)
            eng.params.flat32[: eng.params.n_live].add_(direction, alpha=-s)
        return float(loss.double()), plan, dout

    torch.manual_seed(0)
    direction = torch.randn(eng.params.n_live, device="cuda:0")
    direction /= direction.norm()
    _, plan, dout = loss_at(0.0, direction)
    eng.zero_grads()
    eng.backward(plan, dout)
    analytic = float((eng.grads[: eng.params.n_live].double() * direction.double()).sum())
    eps = 2e-2
    numeric = (loss_at(eps, direction)[0] - loss_at(-eps, direction)[0]) / (2 * eps)
    assert abs(analytic - numeric) < 3e-2 * max(abs(numeric), 1e-3), (analytic, numeric)


def _dp_steps(world, rank):
    from sea_amd.parallel import shard_batch
    from sea_amd.utils.train_utils import initialize_optimizer

    cfg = O.OracleConfig(*MODELS["e384"])
    x, tgt, ib = recipe_inputs(4, 24, cfg, seed=31)
    m = build(cfg, "fp32").train()
    eng = m.engine()
    opt = initialize_optimizer(m, {"learning_rate": 1e-3})
    xs, ts, cs = (shard_batch(t_, rank, world).cuda().contiguous() for t_ in (x, tgt, ib))
    for _ in range(2):
        eng.train_step(xs, ts, cs, opt)
    return eng.params.flat32[: eng.params.n_live].cpu().numpy()


def _dp_worker(rank, world, port, ret):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ret[rank] = _dp_steps(world, rank)
    except Exception as e:  # pragma: no cover
        ret[rank] = repr(e)
    finally:
        dist.destroy_process_group()


def test_data_parallel_step_equals_single_process():
    from tests.test_parallel_gpu import _free_port

    ref = _dp_steps(1, 0)
    ret = mp.Manager().dict()
    mp.spawn(_dp_worker, args=(2, _free_port(), ret), nprocs=2, join=True)
    got = dict(ret)
    assert all(not isinstance(v, str) for v in got.values()), got
    for r in range(2):
        assert np.abs(got[r] - ref).max() <= 2e-5, r
    assert np.array_equal(got[0], got[1])


@pytest.mark.parametrize("E,H,hd", [(96, 8, 12), (264, 1, 264), (160, 8, 20)])
def test_unsupported_head_dims_are_refused(E, H, hd):
    from sea_amd.models.temporal import TemporalModel

    m = TemporalModel(1, E, H, 16, 8, 0, 1, 2, 0.0, "sea", "learnable", "mlp", "add", 1, 1, True, "adaln").to("cuda:0")
    with pytest.raises(NotImplementedError, match=f"self-attention head dim {hd} .*multiples of 8 from 8 to 256"):
        m.engine()
