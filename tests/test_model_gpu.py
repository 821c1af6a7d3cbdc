"""Whole-model parity on the MI355X: sea_amd.TemporalModel (HIP kernels through the C ABI) against the golden vectors the
reference produced and against the CPU oracle on the same seeded inputs.

Tolerances (relative L2 over the whole output tensor):
  fp32 compute  : 1e-4  (north_star's bar; measured ~1e-6)
  bf16 compute  : 3e-2  for a single forward (bf16 operands, fp32 accumulation/statistics/residual stream)
"""
import numpy as np
import pytest
import torch

from oracle import sea_oracle as O
from oracle.recipe import recipe_inputs, recipe_params
from tests.conftest import cfg_from_meta, grad_err, load_golden, rel_l2

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4
BF16_TOL = 3e-2


def build(cfg, dtype="fp32"):
    from sea_amd.models.temporal import TemporalModel

    m = TemporalModel(cfg.num_layers, cfg.embed_dim, cfg.n_heads, cfg.max_len, cfg.scale_ratio, cfg.src_len, cfg.num_variables,
                      cfg.down_proj, 0.0, cfg.exchange_mode, "learnable", cfg.ib_scale_mode, cfg.ib_addition_mode, 1, 1, cfg.add_info_after_cross, cfg.LN_type)
    p = recipe_params(cfg)
    with torch.no_grad():
        for k, prm in m.named_parameters():
            prm.copy_(p[k])
    m.set_compute_dtype(dtype)
    return m.to("cuda:0").eval()


def gpu(a):
    return torch.from_numpy(np.asarray(a)).to("cuda:0")


MODEL_CASES = ["model_tiny_adaln_f3", "model_tiny_ln_f2", "model_tiny_adaln_f2_pre", "model_small_srclen2",
               "model_small_adaln_f3_T1", "model_small_adaln_f3_T7", "model_small_adaln_f3_T16", "model_small_adaln_f3_T65",
               # ablation variants: exchange_mode 'addition' / 'simple', ib_addition_mode 'none'
               "model_addition_adaln_f3", "model_addition_ln_f2_pre", "model_simple_adaln_f3", "model_sea_noib_adaln_f2",
               # ib_scale_mode 'fourier' (the constructor's default) and 'linear'
               "model_sea_fourier_adaln_f3", "model_sea_linear_ln_f2_pre",
               "model_pool_adaln_f3", "model_pool_ln_f2",
               # ib_addition_mode 'attention': un-masked cross-attention from the field rows to the info-bottleneck rows (after / before the exchange)
               "model_ibattn_adaln_f3", "model_ibattn_ln_f2_pre",
               # ib_addition_mode 'concat': every block works on rows widened by 64 info-bottleneck columns (embed_dim 64 -> 128)
               "model_ibconcat_adaln_f3", "model_ibconcat_ln_f2"]


@pytest.mark.parametrize("chain", [True, False])
@pytest.mark.parametrize("F,ln,after", [(2, "ln", True), (2, "adaln", False), (3, "ln", True)])
def test_bf16_fused_launches_at_shipped_widths(F, ln, after, chain, monkeypatch):
    """E = 256 / D = 128 (the widths sea_row_chain, sea_exchange_tail and the 16-row Linear + norm launches instantiate) with the configurations the golden
    fixtures do not reach in bf16: F = 2 (one segment per tail), LayerNorm without modulation, the info-bottleneck add in front of the block;
    forward against the fp32 oracle, and the KV-cache rollout (M = 2 rows per launch) against the recompute rollout — with the row chains of round 4
    (default) and with round 3's launches (SEA_PLAN=chain=0)."""
    from sea_amd.utils.train_utils import rollout

    if not chain:
        monkeypatch.setenv("SEA_PLAN", "chain=0")
    cfg = O.OracleConfig(2, 256, 8, 64, 8, 0, F, 2, after, ln)
    x, _, ib = recipe_inputs(2, 50, cfg, seed=21)
    ref = O.model_forward(x, ib, recipe_params(cfg), cfg)
    m = build(cfg, "bf16")
    with torch.no_grad():
        out = m(x.cuda(), ib.cuda())
        names = [r.name for r in m.engine().plan(2, 50, "full").records]
    assert "cross0.tail" in names and ("cross.down_norm_old" in names) == (not chain) and ("self.out_proj_down_qkv" in names) == chain
    assert rel_l2(out.cpu().numpy(), ref.numpy()) < BF16_TOL
    a = rollout(m, x[:, :1].cuda(), ib.cuda(), 10, mode="recompute")
    b = rollout(m, x[:, :1].cuda(), ib.cuda(), 10, mode="kv")
    assert rel_l2(b.cpu().numpy(), a.cpu().numpy()) < 2e-2


@pytest.mark.parametrize("xmode,ibmode,ibscale", [("addition", "add", "mlp"), ("simple", "add", "mlp"), ("sea", "none", "mlp"), ("sea", "add", "fourier"), ("addition", "add", "linear"), ("pool", "add", "mlp"),
                                                  ("sea", "attention", "mlp")])
def test_ablation_variants_rollout_bf16_and_training(xmode, ibmode, ibscale):
    """The ablation variants through the same plan machinery: bf16 forward within the stated tolerance of the fp32 oracle, KV-cache rollout
    equal to the recompute rollout, and the hand-written backward against the oracle's autograd."""
    from sea_amd.utils.train_utils import rollout

    cfg = O.OracleConfig(2, 128, 4, 96, 8, 0, 3, 2, True, "adaln", xmode, ibmode, ibscale)
    x, _, ib = recipe_inputs(2, 40, cfg, seed=11)
    ref = O.model_forward(x, ib, recipe_params(cfg), cfg)
    m = build(cfg, "bf16")
    with torch.no_grad():
        out = m(x.cuda(), ib.cuda())
    assert rel_l2(out.cpu().numpy(), ref.numpy()) < BF16_TOL
    m32 = build(cfg, "fp32")
    a = rollout(m32, x[:, :1].cuda(), ib.cuda(), 12, mode="recompute")
    if xmode == "pool" or ibmode == "attention":
        # 'pool': window-relative sinusoidal positions; ib 'attention': rows attend to the info-bottleneck rows of LATER positions of the window — neither is
        # a cache-able recurrence: the engine refuses loudly, the rollout front end (what the evaluation loops call) falls back to the recompute loop
        with pytest.raises(NotImplementedError, match="KV-cache"):
            m32.engine().rollout_kv(x[:, :1].cuda(), ib.cuda(), 12)
        assert torch.equal(rollout(m32, x[:, :1].cuda(), ib.cuda(), 12, mode="kv"), a)
    else:
        b = rollout(m32, x[:, :1].cuda(), ib.cuda(), 12, mode="kv")
        assert rel_l2(b.cpu().numpy(), a.cpu().numpy()) < 1e-5
    assert rel_l2(a.cpu().numpy(), O.rollout(x[:, :1], ib, 12, recipe_params(cfg), cfg).numpy()) < FP32_TOL
    m32.train()
    # gradients against the CPU oracle's autograd (the reference-generated goldens are in tests/test_train_gpu.py)
    _, loss_ref, grads_ref = O.loss_and_grads(x, ib, x * 0.5, recipe_params(cfg), cfg)
    eng = m32.engine()
    out, plan = eng.forward_train(x.cuda(), ib.cuda())
    loss, dout = eng.mse_loss_and_grad(out, (x * 0.5).cuda())
    eng.zero_grads()
    eng.backward(plan, dout)
    assert abs(loss.item() - float(loss_ref)) < 1e-4 * float(loss_ref)
    for k, gr in grads_ref.items():
        assert grad_err(eng.grad_view(k).cpu().numpy(), gr.numpy()) < 2e-4, k
    assert sorted(eng.params.live_names) == sorted(grads_ref.keys())


def test_ib_concat_rollouts_bf16_and_constructor_rules():
    """ib_addition_mode 'concat' (models/temporal.py:48,115-116): embed_dim 192 -> block rows of 256 (head dims 32 / 16, the widths of the fused bf16 launches).
    KV-cache rollout (generic step plan: the concatenation is per position, so the cache is exact) against the recompute rollout and the oracle; bf16 forward
    within the stated tolerance; add_info_after_cross=True is refused (the reference's own forward fails there)."""
    from sea_amd.models.temporal import TemporalModel
    from sea_amd.utils.train_utils import rollout

    cfg = O.OracleConfig(2, 192, 8, 96, 8, 0, 3, 2, False, "adaln", "sea", "concat")
    x, _, ib = recipe_inputs(2, 40, cfg, seed=12)
    p = recipe_params(cfg)
    ref = O.model_forward(x, ib, p, cfg)
    m = build(cfg, "bf16")
    with torch.no_grad():
        out = m(x.cuda(), ib.cuda())
    assert out.shape == (2, 40, 3, 192)
    assert rel_l2(out.cpu().numpy(), ref.numpy()) < BF16_TOL
    m32 = build(cfg, "fp32")
    with torch.no_grad():
        assert rel_l2(m32(x.cuda(), ib.cuda()).cpu().numpy(), ref.numpy()) < FP32_TOL
    a = rollout(m32, x[:, :1].cuda(), ib.cuda(), 12, mode="recompute")
    b = rollout(m32, x[:, :1].cuda(), ib.cuda(), 12, mode="kv")
    assert len(m32.engine()._kv_fast) == 0          # rows of two widths: the generic step plan, not sea_kv_rollout
    assert rel_l2(b.cpu().numpy(), a.cpu().numpy()) < 1e-5
    assert rel_l2(a.cpu().numpy(), O.rollout(x[:, :1], ib, 12, p, cfg).numpy()) < FP32_TOL
    bad = TemporalModel(1, 64, 4, 32, 8, 0, 2, 2, 0.0, "sea", "learnable", "mlp", "concat", 1, 1, True, "ln").to("cuda:0")
    with pytest.raises(NotImplementedError, match="add_info_after_cross"):
        bad(x[:, :8, :2, :64].contiguous().cuda(), ib[:, :8].cuda())


def test_kv_rollout_with_src_len_is_refused_and_falls_back_to_recompute():
    """src_len > 0: the reference's recompute loop lets rows already produced attend to the src_len rows appended after them (mask
    tril(diagonal=src_len), models/base_blocks.py:173), so a K/V cache is not exact: the engine refuses, rollout() recomputes, and that
    recompute rollout matches the CPU oracle's restatement of the reference loop."""
    from sea_amd.utils.train_utils import rollout

    g = load_golden("model_small_srclen2")
    cfg = cfg_from_meta(g["cfg"])
    assert cfg.src_len == 2
    m = build(cfg, "fp32")
    x, ib = gpu(g["x"]), gpu(g["ib"])
    with pytest.raises(NotImplementedError, match="src_len"):
        m.engine().rollout_kv(x[:, :1].contiguous(), ib, 6)
    a = rollout(m, x[:, :1].contiguous(), ib, 6, mode="kv")
    b = rollout(m, x[:, :1].contiguous(), ib, 6, mode="recompute")
    assert torch.equal(a, b)
    ref = O.rollout(torch.from_numpy(g["x"])[:, :1], torch.from_numpy(g["ib"]), 6, recipe_params(cfg), cfg)
    assert rel_l2(a.cpu().numpy(), ref.numpy()) < FP32_TOL


def test_backward_after_second_forward_of_same_shape_raises():
    """One activation set per (batch, length) lives in the training plan's workspace: a backward whose activations were replaced by a later
    grad-enabled forward must fail loudly instead of returning wrong gradients (torch itself would handle the pattern)."""
    from sea_amd.utils.train_utils import SeaMSELoss

    g = load_golden("model_tiny_adaln_f3")
    cfg = cfg_from_meta(g["cfg"])
    m = build(cfg, "fp32").train()
    x, tgt, ib = gpu(g["x"]), gpu(g["tgt"]), gpu(g["ib"])
    out1 = m(x, ib)
    out2 = m(x * 0.5, ib)
    with pytest.raises(RuntimeError, match="overwritten"):
        SeaMSELoss()(out1, tgt).backward()
    SeaMSELoss()(out2, tgt).backward()          # the latest forward's backward is fine
    out3 = m(x, ib)
    with torch.no_grad():
        m(x * 0.5, ib)                          # an eval-style forward between forward and backward does not touch the training plan
    SeaMSELoss()(out3, tgt).backward()


@pytest.mark.parametrize("name", MODEL_CASES)
def test_forward_fp32_matches_reference_golden(name):
    g = load_golden(name)
    cfg = cfg_from_meta(g["cfg"])
    m = build(cfg, "fp32")
    with torch.no_grad():
        out = m(gpu(g["x"]), gpu(g["ib"]))
    assert out.shape == g["out"].shape
    assert rel_l2(out.cpu().numpy(), g["out"]) < FP32_TOL


@pytest.mark.parametrize("name", ["model_small_adaln_f3_T16", "model_small_adaln_f3_T65", "model_tiny_ln_f2"])
def test_forward_bf16_within_stated_tolerance(name):
    g = load_golden(name)
    cfg = cfg_from_meta(g["cfg"])
    m = build(cfg, "bf16")
    with torch.no_grad():
        out = m(gpu(g["x"]), gpu(g["ib"]))
    assert rel_l2(out.cpu().numpy(), g["out"]) < BF16_TOL


def test_forward_is_repeatable_and_does_not_touch_inputs():
    g = load_golden("model_small_adaln_f3_T16")
    cfg = cfg_from_meta(g["cfg"])
    m = build(cfg, "fp32")
    x, ib = gpu(g["x"]), gpu(g["ib"])
    x0 = x.clone()
    with torch.no_grad():
        a = m(x, ib)
        b = m(x, ib)
        x2 = x.clone()
        c = m(x2, ib.clone())  # different tensor addresses: the plan re-binds
    assert torch.equal(x, x0)
    assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("dtype,tol", [("fp32", FP32_TOL), ("bf16", BF16_TOL)])
def test_cfg2_shape_forward(dtype, tol):
    """BASELINE.json configs[1]: E=256, H=8, F=3, T=2024, B=1 — against the reference's strided sample and norms."""
    g = load_golden("cfg2_shape")
    cfg = cfg_from_meta(g["cfg"])
    m = build(cfg, dtype)
    x, _, ib = recipe_inputs(1, 2024, cfg, seed=int(g["seed"]))
    with torch.no_grad():
        out = m(x.cuda(), ib.cuda()).cpu()
    assert rel_l2(out[:, ::97, :, ::13].numpy(), g["out_sub"]) < tol
    assert rel_l2(out[:, -1].numpy(), g["out_last"]) < tol
    assert np.allclose(out.pow(2).sum(dim=(0, 1, 3)).sqrt().numpy(), g["out_l2"], rtol=tol)


def test_forward_matches_oracle_on_fresh_inputs_batch8():
    """Same seeded inputs through the oracle (CPU fp32) and the HIP path, at a shape no fixture covers (B=8, T=130, L=2)."""
    cfg = O.OracleConfig(2, 128, 4, 160, 8, 0, 3, 2, True, "adaln")
    m = build(cfg, "fp32")
    x, _, ib = recipe_inputs(8, 130, cfg, seed=2024)
    with torch.no_grad():
        ref = O.model_forward(x, ib, recipe_params(cfg), cfg)
        out = m(x.cuda(), ib.cuda()).cpu()
    assert rel_l2(out.numpy(), ref.numpy()) < FP32_TOL


def test_causality_and_prefix_consistency():
    """Size-independent properties: perturbing step t leaves outputs < t unchanged; forward on a prefix equals the prefix of
    the forward (what makes recompute rollout and KV-cache rollout equivalent)."""
    cfg = O.OracleConfig(1, 64, 4, 96, 8, 0, 3, 2, True, "adaln")
    m = build(cfg, "fp32")
    x, _, ib = recipe_inputs(2, 90, cfg, seed=5)
    x, ib = x.cuda(), ib.cuda()
    with torch.no_grad():
        a = m(x, ib)
        x2 = x.clone()
        x2[:, 70] += 1.0
        b = m(x2, ib)
        c = m(x[:, :50].contiguous(), ib[:, :50].contiguous())
    assert torch.equal(a[:, :70], b[:, :70]) and not torch.equal(a[:, 70:], b[:, 70:])
    assert rel_l2(c.cpu().numpy(), a[:, :50].cpu().numpy()) < 1e-5


def test_cfg2_full_size_causality_and_prefix_bf16():
    """The same size-independent properties at BASELINE.json configs[1] (E=256, H=8, F=3, T=2024, B=1) in bf16, i.e. through the plan bench.py
    times (fused launches, graph replay included): a perturbation at step 1500 leaves every earlier output bit-identical and changes later ones;
    the forward of the 1000-step prefix equals the prefix of the forward within the bf16 tolerance; the graph replay equals the plain replay bitwise, and so do 25 further replays."""
    g = load_golden("cfg2_shape")
    cfg = cfg_from_meta(g["cfg"])
    m = build(cfg, "bf16")
    x, _, ib = recipe_inputs(1, 2024, cfg, seed=int(g["seed"]))
    x, ib = x.cuda().contiguous(), ib.cuda().contiguous()
    with torch.no_grad():
        a = m(x, ib).clone()
        names = [r.name for r in m.engine().plan(1, 2024, "full").records]
        assert "mlp.block_norm" in names and "cross0.tail" in names and "self.out_proj_down_qkv" in names and "self.cond_adaln0_qkv_rope" in names and len(names) == 10 and "adaln.silu" not in names   # the plan of the bench line
        x2 = x.clone()
        x2[:, 1500] += 1.0
        b = m(x2, ib).clone()
        c = m(x[:, :1000].contiguous(), ib[:, :1000].contiguous()).clone()
        gr = m.engine().forward_graphed(x, ib).clone()
    assert torch.equal(a[:, :1500], b[:, :1500]) and not torch.equal(a[:, 1500:], b[:, 1500:])
    assert rel_l2(c.cpu().numpy(), a[:, :1000].cpu().numpy()) < BF16_TOL
    assert torch.equal(gr, a)
    with torch.no_grad():   # run-to-run determinism of the whole plan (this caught a packed-fp32 code path of the QKV + RoPE launch that was not, sea_amd/build.py)
        for _ in range(25):
            assert torch.equal(m(x, ib), a)


@pytest.mark.parametrize("cfg_args,dtype,B,T", [((1, 64, 4, 96, 8, 0, 3, 2, True, "adaln"), "fp32", 2, 90),
                                                ((2, 128, 4, 160, 8, 0, 3, 2, True, "adaln"), "bf16", 3, 150),
                                                ((2, 256, 8, 640, 8, 0, 2, 2, False, "ln"), "bf16", 1, 600),
                                                ((1, 256, 8, 640, 8, 0, 3, 2, True, "adaln"), "fp32", 1, 600),
                                                ((1, 2048, 8, 64, 8, 0, 2, 2, True, "ln"), "bf16", 1, 40)])
def test_forward_and_kv_rollout_replays_are_bit_identical(cfg_args, dtype, B, T):
    """No launch of the inference plans may depend on timing: 20 replays of the forward and a second KV-cache rollout reproduce the first bit for bit
    (other instantiations than cfg2's: fp32, E = 64 / 128 / 2048, LayerNorm without modulation, two layers, F = 2)."""
    from sea_amd.utils.train_utils import rollout

    cfg = O.OracleConfig(*cfg_args)
    m = build(cfg, dtype)
    x, _, ib = recipe_inputs(B, T, cfg, seed=77)
    x, ib = x.cuda().contiguous(), ib.cuda().contiguous()
    with torch.no_grad():
        a = m(x, ib).clone()
        for _ in range(20):
            assert torch.equal(m(x, ib), a)
        n = min(T, 48)
        r1 = rollout(m, x[:, :1].contiguous(), ib, n, mode="kv").clone()
        r2 = rollout(m, x[:, :1].contiguous(), ib, n, mode="kv")
    assert torch.equal(r1, r2)


@pytest.mark.parametrize("name", ["rollout8_adaln_f3", "rollout100_ln_f2", "rollout100_ln_f2_e256"])
def test_rollout_recompute_matches_reference_golden(name):
    from sea_amd.utils.train_utils import relativeMSE, rollout

    g = load_golden(name)
    cfg = cfg_from_meta(g["cfg"])
    m = build(cfg, "fp32")
    tgt = gpu(g["tgt"])
    pred = rollout(m, gpu(g["x0"]), gpu(g["ib"]), tgt.shape[1], mode="recompute")
    assert rel_l2(pred.cpu().numpy(), g["pred"]) < 2e-4  # autoregressive: per-step noise compounds over up to 100 steps
    rel = relativeMSE(pred, tgt).mean().item()
    assert abs(rel - float(g["rel_mse"])) < 1e-3 * float(g["rel_mse"])


def test_module_forwards_match_reference_golden():
    """The stand-alone module mirrors (AdaLN, LayerNorm, attention, MLP) through the un-fused kernels."""
    from oracle.recipe import recipe_tensor
    from sea_amd.models import base_blocks as bb

    g = load_golden("modules")

    def load(mod, prefix):
        for row in g["kinds:" + prefix]:
            key, kind, shp = str(row).split("|")
            shape = tuple(int(s) for s in shp.split(",")) if shp else ()
            name = key[len(prefix):]
            obj = mod
            parts = name.split(".")
            for p_ in parts[:-1]:
                obj = getattr(obj, p_) if not p_.isdigit() else obj[int(p_)]
            with torch.no_grad():
                getattr(obj, parts[-1]).copy_(torch.from_numpy(recipe_tensor(key, shape, kind)))
        return mod.to("cuda:0").eval()

    for d in (64, 128):
        mod = load(bb.AdaLN(d, 1), f"adaln{d}.")
        y = mod(gpu(g[f"adaln{d}.x"]), gpu(g[f"adaln{d}.c"]))
        assert rel_l2(y.cpu().numpy(), g[f"adaln{d}.y"]) < FP32_TOL
    mod = load(bb.LayerNorm(64), "ln64.")
    assert rel_l2(mod(gpu(g["ln64.x"])).cpu().numpy(), g["ln64.y"]) < FP32_TOL
    for T in (1, 7, 16):
        mod = load(bb.MaskedMultiHeadAttention(4, 64, 32, 0, 0.0), "self64.")
        assert rel_l2(mod(gpu(g[f"self64.T{T}.x"])).cpu().numpy(), g[f"self64.T{T}.y"]) < FP32_TOL
    mod = load(bb.MaskedMultiHeadAttention(4, 64, 32, 3, 0.0), "self64s3.")
    assert rel_l2(mod(gpu(g["self64s3.x"])).cpu().numpy(), g["self64s3.y"]) < FP32_TOL
    mod = load(bb.MaskedMultiHeadCrossAttention(4, 32, 32, 0, 0.0), "cross32.")
    assert rel_l2(mod(gpu(g["cross32.x1"]), gpu(g["cross32.x2"])).cpu().numpy(), g["cross32.y"]) < FP32_TOL
    mod = load(bb.MLP(64, 0.0, 8), "mlp64.")
    assert rel_l2(mod(gpu(g["mlp64.x"])).cpu().numpy(), g["mlp64.y"]) < FP32_TOL
    mod = load(bb.MLP(1, 0.0, 8, 64, 1), "ibmlp.")
    assert rel_l2(mod(gpu(g["ibmlp.c"])).cpu().numpy(), g["ibmlp.y"]) < FP32_TOL


@pytest.mark.parametrize("tag", ["F2adaln", "F3adaln", "F3ln"])
def test_block_forward_unfused_matches_reference_golden(tag):
    """SEABlockTemporal.forward / _apply_exchange through the module kernels (Gauss-Seidel order)."""
    g = load_golden("exchange")
    cfg = cfg_from_meta(g[tag + ".cfg"])
    m = build(cfg, "fp32")
    x, ib = gpu(g[tag + ".x"]), gpu(g[tag + ".ib"])
    F = cfg.num_variables
    with torch.no_grad():
        ys = m.blocks[0]._apply_exchange([x[:, :, i].contiguous() for i in range(F)], ib)
        blk = m.blocks[0](*[x[:, :, i] for i in range(F)], x_add=ib)
    assert rel_l2(torch.stack(ys, 2).cpu().numpy(), g[tag + ".y"]) < FP32_TOL
    assert rel_l2(torch.stack(blk, 2).cpu().numpy(), g[tag + ".block"]) < FP32_TOL


@pytest.mark.parametrize("name", ["rollout8_adaln_f3", "rollout100_ln_f2", "rollout100_ln_f2_e256"])
def test_rollout_kv_cache_matches_reference_golden(name):
    """KV-cache decode is exact: it must reproduce the reference's recompute rollout."""
    from sea_amd.utils.train_utils import rollout

    g = load_golden(name)
    cfg = cfg_from_meta(g["cfg"])
    m = build(cfg, "fp32")
    n = g["tgt"].shape[1]
    pred = rollout(m, gpu(g["x0"]), gpu(g["ib"]), n, mode="kv")
    assert pred.shape == g["pred"].shape
    assert rel_l2(pred.cpu().numpy(), g["pred"]) < 2e-4
    again = rollout(m, gpu(g["x0"]), gpu(g["ib"]), n, mode="kv")  # caches are reused: a second rollout must not see stale keys
    assert torch.equal(pred, again)


@pytest.mark.parametrize("name", ["rollout100_ln_f2_e256", "rollout8_adaln_f3"])
def test_batched_kv_rollout_matches_golden_row_and_oracle(name):
    """The KV-cache rollout over a BATCH of trajectories (what full_autoregressive_evaluation does with a loader batch, utils/train_utils.py:186-209;
    sea_kv_rollout's seven-launch form): the golden trajectory placed in a batch of three next to perturbed copies comes out as the reference computed
    it alone, and every row agrees with the oracle's batched recompute rollout."""
    from oracle.recipe import recipe_params
    from sea_amd.utils.train_utils import rollout

    g = load_golden(name)
    cfg = cfg_from_meta(g["cfg"])
    m = build(cfg, "fp32")
    n = g["tgt"].shape[1]
    gen = torch.Generator().manual_seed(5)
    gx, gib = torch.from_numpy(g["x0"]), torch.from_numpy(g["ib"])
    nb = gx.shape[0]                                                # the golden trajectories sit between a perturbed first and last row
    x0 = torch.cat((gx[:1] + 0.3 * torch.randn(gx[:1].shape, generator=gen), gx, gx[-1:] - 0.2 * torch.randn(gx[:1].shape, generator=gen)))
    ib = torch.cat((torch.rand(gib[:1].shape, generator=gen), gib, gib[-1:]))
    pred = rollout(m, x0.cuda(), ib.cuda(), n, mode="kv").cpu()
    assert rel_l2(pred[1:1 + nb].numpy(), g["pred"]) < 2e-4      # the golden rows, batched
    ref = O.rollout(x0, ib, n, recipe_params(cfg), cfg)
    assert rel_l2(pred.numpy(), ref.numpy()) < 2e-4
    mb = build(cfg, "bf16")
    pb = rollout(mb, x0.cuda(), ib.cuda(), n, mode="kv").cpu()
    assert rel_l2(pb.numpy(), ref.numpy()) < 1e-1


def test_rollout_kv_bf16_error_is_reported_and_bounded():
    """bf16 tolerance over a 100-step autoregressive rollout (north_star: 'stated bf16 tolerance'): rel-L2 <= 1e-1 at 100 steps
    on the E=256 multiphase-like model; the measured value is printed."""
    from sea_amd.utils.train_utils import rollout

    g = load_golden("rollout100_ln_f2_e256")
    cfg = cfg_from_meta(g["cfg"])
    m = build(cfg, "bf16")
    pred = rollout(m, gpu(g["x0"]), gpu(g["ib"]), 100, mode="kv").cpu().numpy()
    e8, e100 = rel_l2(pred[:, :8], g["pred"][:, :8]), rel_l2(pred, g["pred"])
    print(f"bf16 KV rollout rel-L2: 8 steps {e8:.3e}, 100 steps {e100:.3e}")
    assert e8 < 3e-2 and e100 < 1e-1


def test_cfg5_shipped_multiphase_dims_rollout100():
    """BASELINE.json configs[4] at its own size: the shipped multiphase_flow dims (embed_dim 2048, 2 field groups, 'ln', head dims 256 / 128, MLP hidden 16384),
    a 100-step autoregressive rollout.  fp32 KV-cache rollout (few-row kernels at every width of a step: contractions up to 16384, rows of 16384, one-row
    attention at head dims 256 / 128) against the CPU oracle's restatement of the reference's recompute loop at north_star's 1e-4, and against the device's own
    recompute rollout; bf16 within the stated 100-step tolerance (1e-1; the measured value is printed)."""
    from sea_amd.utils.train_utils import rollout

    cfg = O.OracleConfig(1, 2048, 8, 104, 8, 0, 2, 2, True, "ln")
    p = recipe_params(cfg)
    x, _, ib = recipe_inputs(1, 100, cfg, seed=21)
    with torch.no_grad():
        ref = O.rollout(x[:, :1], ib, 100, p, cfg).numpy()
    x0, ibg = x[:, :1].cuda().contiguous(), ib.cuda().contiguous()
    m32 = build(cfg, "fp32")
    kv = rollout(m32, x0, ibg, 100, mode="kv").cpu().numpy()
    rc = rollout(m32, x0, ibg, 100, mode="recompute").cpu().numpy()
    e_kv, e_rc = rel_l2(kv, ref), rel_l2(rc, ref)
    print(f"multiphase dims, 100 steps, fp32 vs oracle: KV {e_kv:.3e}, recompute {e_rc:.3e}")
    assert e_kv < FP32_TOL and e_rc < FP32_TOL
    del m32
    mb = build(cfg, "bf16")
    kb = rollout(mb, x0, ibg, 100, mode="kv").cpu().numpy()
    e8, e100 = rel_l2(kb[:, :8], ref[:, :8]), rel_l2(kb, ref)
    print(f"multiphase dims, bf16 KV rollout rel-L2: 8 steps {e8:.3e}, 100 steps {e100:.3e}")
    assert e8 < 3e-2 and e100 < 1e-1


def test_graph_replay_equals_plain_replay():
    cfg = O.OracleConfig(1, 64, 4, 96, 8, 0, 3, 2, True, "adaln")
    m = build(cfg, "bf16")
    x, _, ib = recipe_inputs(2, 80, cfg, seed=11)
    x, ib = x.cuda(), ib.cuda()
    eng = m.engine()
    with torch.no_grad():
        a = eng.forward(x, ib).clone()
        b = eng.forward_graphed(x, ib).clone()
        x.add_(0.5)  # new data written into the same buffers is picked up by the replay
        c = eng.forward_graphed(x, ib).clone()
        d = eng.forward(x, ib)
    assert torch.equal(a, b) and torch.equal(c, d) and not torch.equal(a, c)


def test_cfg1_shipped_cylinder_dims_rollout8():
    """BASELINE.json configs[0]: the shipped cylinder_flow dims (embed_dim 1024, 2 field groups, head dims 128 / 64, MLP hidden 8192),
    1 trajectory, 8-step rollout — fp32 against the reference's golden sample, recompute and KV-cache modes."""
    from sea_amd.utils.train_utils import rollout

    g = load_golden("cfg1_cylinder_rollout8")
    cfg = cfg_from_meta(g["cfg"])
    m = build(cfg, "fp32")
    x, _, ib = recipe_inputs(1, 8, cfg, seed=int(g["seed"]))
    for mode in ("recompute", "kv"):
        pred = rollout(m, x[:, :1].cuda(), ib.cuda(), 8, mode=mode).cpu()
        assert rel_l2(pred[:, :, :, ::37].numpy(), g["pred_sub"]) < 2e-4, mode
        assert np.allclose(pred.pow(2).sum(dim=(0, 3)).sqrt().numpy(), g["pred_l2"], rtol=2e-4), mode


@pytest.mark.parametrize("dtype,tol", [("bf16", BF16_TOL), ("fp32", 1e-4)])
def test_shipped_multiphase_dims_forward(dtype, tol):
    """configs/multiphase_flow.py dims: embed_dim 2048, 2 field groups, LN_type 'ln' -> head dims 256 / 128, MLP hidden 16384.
    Forward and a short KV rollout against the CPU oracle on the same seeded inputs (rows of 16384 exercise the generic row kernels); fp32 at
    north_star's 1e-4 (head dim 256 in f32: the single-buffer attention instantiation), bf16 at the single-forward bf16 tolerance."""
    from sea_amd.utils.train_utils import rollout

    cfg = O.OracleConfig(1, 2048, 8, 64, 8, 0, 2, 2, True, "ln")
    p = recipe_params(cfg)
    x, _, ib = recipe_inputs(1, 40, cfg, seed=9)
    with torch.no_grad():
        ref = O.model_forward(x, ib, p, cfg)
        ref_roll = O.rollout(x[:, :1], ib, 6, p, cfg)
    m = build(cfg, dtype)
    with torch.no_grad():
        out = m(x.cuda(), ib.cuda()).cpu()
    assert rel_l2(out.numpy(), ref.numpy()) < tol
    roll = rollout(m, x[:, :1].cuda(), ib.cuda(), 6, mode="kv").cpu()
    assert rel_l2(roll.numpy(), ref_roll.numpy()) < 2 * tol


@pytest.mark.parametrize("F,B,T", [(3, 2, 70), (2, 1, 130), (3, 1, 300)])
def test_rider_plan_matches_the_plans_it_replaces(F, B, T, monkeypatch):
    """One-layer AdaLN models in bf16 run round 4's rider plan: the condition GEMM in front covers AdaLN_0 + ln_cross only, the row chains (sea_row_chain_riders)
    carry cond_mlp.2 of the modules the field MLP / final norm read as RIDER tiles on the CUs they leave idle (engine._Riders.take).  Against the oracle, against the same model with SEA_PLAN=riders=0 (whole-model silu + condition launches: same arithmetic ->
    bitwise) and with SEA_PLAN=chain=0 (round 3's launches); rows cross a trajectory boundary (B = 2) and a partial last tile (T = 70, 130, 300)."""
    cfg = O.OracleConfig(1, 128, 4, 320, 8, 0, F, 2, True, "adaln")
    x, _, ib = recipe_inputs(B, T, cfg, seed=9)
    xg, ibg = x.to("cuda:0").contiguous(), ib.to("cuda:0").contiguous()
    m = build(cfg, "bf16")
    with torch.no_grad():
        out = m(xg, ibg).clone()
        out2 = m(xg, ibg).clone()
    names = [r.name for r in m.engine().plan(B, T, "full").records]
    assert "self.cond_adaln0" in names and "adaln.cond_gemm" not in names and "self.adaln0" not in names and "ib_add" not in names
    head = names[:5 + 2 * F]   # silu rows, condition GEMM + AdaLN_0 (sea_gemm_adaln), QKV, self-attention, the chain behind it; per field attention + tail; then the MLP's launches (2 from 1024 rows up)
    assert head == ["adaln.silu", "self.cond_adaln0", "self.qkv_rope", "self.attention", "self.out_proj_down_qkv"] + [f"cross{i}.{k}" for i in range(F) for k in ("attention", "tail")]
    assert torch.equal(out, out2)
    assert rel_l2(out.cpu().numpy(), O.model_forward(x, ib, recipe_params(cfg), cfg).numpy()) < BF16_TOL
    monkeypatch.setenv("SEA_PLAN", "riders=0")
    m2 = build(cfg, "bf16")
    with torch.no_grad():
        ref = m2(xg, ibg)
    names2 = [r.name for r in m2.engine().plan(B, T, "full").records]
    assert "adaln.silu" in names2 and "adaln.cond_gemm" in names2 and "self.out_proj_down_qkv" in names2 and len(names2) == len(names) + 1
    assert rel_l2(out.cpu().numpy(), ref.cpu().numpy()) < 1e-2   # (bf16-level: AdaLN_0's modulation stays fp32 inside sea_gemm_adaln, the two-launch form rounds it to bf16)
    monkeypatch.setenv("SEA_PLAN", "chain=0")
    m3 = build(cfg, "bf16")
    with torch.no_grad():
        ref3 = m3(xg, ibg)
    assert rel_l2(out.cpu().numpy(), ref3.cpu().numpy()) < 2e-2


@pytest.mark.parametrize("env,graphed", [({"SEA_PLAN": "lanes=all"}, True), ({"SEA_PLAN": "lanes=cond"}, True),
                                         ({"SEA_PLAN": "norm=0"}, False), ({"SEA_PLAN": "xtail=0"}, False), ({"SEA_PLAN": "chain=0"}, False), ({"SEA_PLAN": "silu=1"}, False), ({"SEA_PLAN": "fold_ib=0"}, False), ({"SEA_PLAN": "mlp1=1"}, False), ({"SEA_PLAN": "mlp1=1,mlp2=1"}, False), ({"SEA_PLAN": "mlp1=1,mlp2=1,mlpblock=0"}, False), ({"SEA_PLAN": "front=0"}, False), ({"SEA_PLAN": "front3=0"}, False),
                                         ({"SEA_TUNE": "gemm_norm_rows=64"}, False)])
@pytest.mark.parametrize("dtype,tol", [("fp32", 2e-6), ("bf16", 2e-2)])
def test_optional_plans_match_default_plan(env, graphed, dtype, tol, monkeypatch):
    """The opt-in plans (fusion switches; parallel graph branches) compute what the default launch list computes — checked on the oracle too
    (E=128, D=64; two layers; B=2 so rows cross a trajectory)."""
    cfg = O.OracleConfig(2, 128, 4, 96, 8, 0, 3, 2, True, "adaln")
    x, _, ib = recipe_inputs(2, 70, cfg, seed=5)
    xg, ibg = x.to("cuda:0").contiguous(), ib.to("cuda:0").contiguous()
    with torch.no_grad():
        ref = build(cfg, dtype)(xg, ibg)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = build(cfg, dtype)
    with torch.no_grad():
        eng = m.engine()
        out = eng.forward_graphed(xg, ibg).clone() if graphed else m(xg, ibg)
        plan = eng.plan(2, 70, "full")
    names = [r.name for r in plan.records]
    sw = env.get("SEA_PLAN", "") + env.get("SEA_TUNE", "")
    if sw == "mlp1=1":   # Linear + nn.LayerNorm + GELU in one launch, forced (default from 1024 rows up: a KV-cache step keeps two launches)
        assert (dtype == "bf16") == ("mlp.fc1_ln_gelu" in names) and (dtype == "fp32") == ("mlp.fc1" in names)
        monkeypatch.delenv("SEA_PLAN")
        e2 = build(cfg, dtype).engine()
        assert "mlp.fc1" in [r.name for r in e2.plan(2, 70, "full").records]
        assert ("mlp.block" in [r.name for r in e2.plan(16, 70, "full").records]) == (dtype == "bf16")   # (from 1024 rows up both halves are fused, and the two fused launches are one: sea_mlp_block)
    elif sw == "mlp1=1,mlp2=1":   # both halves of the field MLP fused and short launches forced: ONE launch (sea_mlp_block), in the last layer with the final norm
        assert (dtype == "bf16") == ("mlp.block" in names and "mlp.block_norm" in names) and "mlp.fc2_proj_norm" not in names
    elif sw == "mlp1=1,mlp2=1,mlpblock=0":   # ... and the two launches it replaces
        assert (dtype == "bf16") == ("mlp.fc1_ln_gelu" in names and "mlp.fc2_proj_norm" in names) and "mlp.block" not in names
    elif sw == "fold_ib=0":     # the info-bottleneck add as its own launch (default: evaluated in the silu launch, added by the AdaLN_2 pass)
        assert "ib_add" in names and "mlp.adaln2" in names and "mlp.ib_adaln2" not in names
    elif sw == "silu=1":   # AdaLN condition MLPs with the generated operand (default only for long launches)
        assert "adaln.silu" not in names and "adaln.cond_gemm" in names
    elif sw == "xtail=0":  # the three-launch form of a field's exchange tail (bf16: the default plan runs sea_exchange_tail)
        assert "cross0.proj_gelu" in names and "cross0.tail" not in names
        monkeypatch.delenv("SEA_PLAN")
        default_names = [r.name for r in build(cfg, dtype).engine().plan(2, 70, "full").records]
        assert ("cross0.tail" in default_names) == (dtype == "bf16")   # the default plan runs sea_exchange_tail in bf16, the three launches in fp32
    elif sw == "chain=0":   # round 3's 18-launch form (out-projection, down + norm, a QKV launch per field, sea_exchange_tail) as the reference of the row chains
        assert "self.out_proj" in names and "cross.down_norm_old" in names and "cross1.qkv_rope" in names and "self.out_proj_down_qkv" not in names
        monkeypatch.delenv("SEA_PLAN")
        default_names = [r.name for r in build(cfg, dtype).engine().plan(2, 70, "full").records]
        # bf16: the default plan runs sea_row_chain (no cross-attention QKV launch, no out-projection, no down + norm launch: 4 launches per layer less)
        assert ("self.out_proj_down_qkv" in default_names) == (dtype == "bf16") and ("cross1.qkv_rope" in default_names) == (dtype == "fp32")
        assert len(default_names) == len(names) - (8 if dtype == "bf16" else 0)
    elif sw == "gemm_norm_rows=64":   # Linear + row norm with the 64-row tiles the long launches use
        assert ("cross.down_norm_old" in names) == (dtype == "fp32") and ("self.out_proj_down_qkv" in names) == (dtype == "bf16")
    elif sw == "front=0":   # silu + sea_gemm_adaln + the QKV launch in front of the first attention (the one-launch front needs E = 256: test_cfg2_* run it)
        assert "self.cond_adaln0_qkv_rope" not in names and "self.qkv_rope" in names
    elif sw == "front3=0":   # ... with the silu launch and the ln_cross condition GEMM as rider tiles (E = 256 only: here the plan is the default one)
        assert "self.cond_adaln0_qkv_rope" not in names
    elif sw == "norm=0":   # the two-launch form of Linear + row norm
        assert "cross.norm_old" in names and "cross.down_norm_old" not in names
    else:
        assert any(r.fn is None for r in plan.records)  # fork / join markers present
    assert rel_l2(out.cpu().numpy(), ref.cpu().numpy()) < tol
    if dtype == "fp32":
        assert rel_l2(out.cpu().numpy(), O.model_forward(x, ib, recipe_params(cfg), cfg).numpy()) < FP32_TOL
