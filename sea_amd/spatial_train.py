"""Training of the spatial autoencoder (`SpatialModel` = `PointwiseEncode` + `Decode`; reference train/train_encoder.py:186-316).

The forward keeps what the backward needs (per EncoderBlock: its input and mid-block residual rows, both LayerNorm inputs' statistics, q / k / v in the
attention layouts, the attention output and its log-sum-exp, the MLP's hidden rows before and after LayerNorm + GELU; per MLP of the down- and up-scale
stacks the GELU pre-activation) and the backward is composed from the existing entry points of libsea_hip.so:

    Linear dgrad          sea_gemm_grouped with a transposed weight copy (act = 2 multiplies by GELU'(pre-activation) in the same pass)
    Linear wgrad          sea_wgrad_grouped (fp32 accumulation into the flat gradient buffer, so gradients add up until zero_grad())
    LayerNorm (+ GELU)    sea_rownorm_bwd (the residual's gradient is accumulated in place)
    attention             sea_attention_bwd, every key visible (src_len = P) and the identity rotary table, as the forward

Parameters live in one flat fp32 buffer (`SpatialFlatParams`) that the module's parameters alias, with a flat fp32 gradient buffer beside it: the engine
protocol FlatAdamW uses (optim.py), so `initialize_optimizer` returns the one-launch AdamW (sea_adamw_flat) for a SpatialModel too.  After every
optimizer step the activation-dtype weight packs of the encoder and the decoder are dropped (the kernel writes through raw pointers, which does not bump
a tensor's version counter).

Rows m = snapshot * P + patch throughout, as in PointwiseEncode.forward.  The inference path (no_grad / eval) is not touched by anything here.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import _native as N
from . import _switches, ops


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


class SpatialFlatParams:
    """All parameters of a SpatialModel in one fp32 buffer (each padded to 8 elements, so the AdamW kernel's n % 4 holds); the module's parameters
    become views of it.  `act_dtype` is fp32: the activation-dtype copies are the encoder's / decoder's own packs, refreshed by `sync_transposed`."""

    def __init__(self, model: torch.nn.Module, device: torch.device):
        named = list(model.named_parameters())
        self.offsets: Dict[str, tuple] = {}
        off = 0
        for name, p in named:
            self.offsets[name] = (off, tuple(p.shape))
            off += _round_up(p.numel(), 8)
        self.n_total = self.n_live = off
        self.device, self.act_dtype = device, torch.float32
        self.flat32 = torch.zeros(off, device=device, dtype=torch.float32)
        self.flat_act = self.flat32
        with torch.no_grad():
            for name, p in named:
                o, shp = self.offsets[name]
                view = self.flat32[o:o + p.numel()].view(shp)
                view.copy_(p.detach().to(device=device, dtype=torch.float32))
                p.data = view
        self.live_names = [n for n, _ in named]
        self._model = model

    def sync_transposed(self, force: bool = False) -> None:
        """Called by FlatAdamW.step after its raw-pointer update: drop the packs built from the old values (always; `force` is FlatAdamW's argument)."""
        self._model.encode._pack = None
        self._model.decode._shadow = self._model.decode._shadow_T = None


class SpatialEngine:
    """Flat parameter / gradient store + the composed training forward and backward of one SpatialModel on one device."""

    def __init__(self, model, device: torch.device):
        self.model, self.device = model, device
        self.params = SpatialFlatParams(model, device)
        self.grads: Optional[torch.Tensor] = None
        self.grads_dirty = False
        self.launches = 0   # native launches issued by forward_train / backward (tools/encoder_train_bench.py reports them per step)

    # ---------------------------------------------------------------- FlatAdamW protocol
    def ensure_grads(self) -> None:
        if self.grads is None:
            self.grads = torch.zeros(self.params.n_total, device=self.device, dtype=torch.float32)

    def zero_grads(self) -> None:
        if self.grads is not None:
            self.grads.zero_()
        self.grads_dirty = False

    def grad_view(self, name: str) -> torch.Tensor:
        o, shp = self.params.offsets[name]
        n = 1
        for s in shp:
            n *= s
        return self.grads[o:o + n].view(shp)

    # ---------------------------------------------------------------- launch helpers (counted)
    def _gemm(self, groups, dt):
        self.launches += 1
        ops.gemm_grouped(groups, dt)

    def _norm(self, groups, M, d, x_is_act, gelu, eps, dt):
        self.launches += 1
        ops.rownorm(groups, M, d, x_is_act, gelu, eps, dt)

    def _norm_bwd(self, groups, M, d, dy_is_act, x_is_act, gelu, accumulate, dt):
        self.launches += 1
        ops.rownorm_bwd(groups, M, d, dy_is_act, x_is_act, gelu, accumulate, dt)

    def _wgrad(self, groups, dt):
        for s in range(0, len(groups), 32):
            self.launches += 1
            ops.wgrad_grouped(groups[s:s + 32], dt)

    def _act(self, src: torch.Tensor, dt) -> torch.Tensor:
        """Activation-dtype copy of an fp32 [M, n] operand (the operand itself in fp32)."""
        if dt == torch.float32:
            return src
        out = torch.empty(src.shape, device=src.device, dtype=dt)
        self.launches += 1
        ops.convert(src, out)
        return out

    # ---------------------------------------------------------------- transposed weights of the data-gradient GEMMs
    def _enc_T(self, pk):
        t = pk.get("train_T")
        if t is None:
            tr = lambda w: w.t().contiguous()  # noqa: E731
            t = dict(enc=[tr(g["W2"]) for g in pk["enc"]],
                     blocks=[dict(wqkv=tr(b["wqkv"]), wo=tr(b["wo"]), w1=tr(b["w1"]), w2=tr(b["w2"])) for b in pk["blocks"]])
            pk["train_T"] = t
        return t

    def _dec_T(self, dec, W1, W2):
        cur = getattr(dec, "_shadow_T", None)
        if cur is None or cur[0] is not dec._shadow:
            cur = (dec._shadow, [w.t().contiguous() for w in W1], [w.t().contiguous() for w in W2])
            dec._shadow_T = cur
        return cur[1], cur[2]

    # ---------------------------------------------------------------- fused EncoderBlocks (encoder_block.hip)
    def _fused_weights(self, pk, dev):
        """Unpadded bf16 q|k|v and projection weights of every block (sea_encoder_block_* take head dim W / 8 as it is)."""
        fw = pk.get("fused_w")
        if fw is None:
            fw = []
            with torch.no_grad():
                for b, blk in zip(self.model.encode.blocks, pk["blocks"]):
                    a = b.attn_1
                    fw.append(dict(wqkv=torch.cat([a.q.weight, a.k.weight, a.v.weight], 0).to(dev, torch.bfloat16).contiguous(),
                                   bqkv=torch.cat([a.q.bias, a.k.bias, a.v.bias], 0).to(dev, torch.float32).contiguous(),
                                   wo=a.projection.weight.detach().to(dev, torch.bfloat16).contiguous(),
                                   **{k: blk[k] for k in ("w1", "b1", "lnw", "lnb", "w2", "b2", "g1", "g2")}))
            pk["fused_w"] = fw
        return fw

    def _blocks_fwd_fused(self, sv, pk, zs, B, P, W, dt, dev):
        fw = self._fused_weights(pk, dev)
        ws = torch.empty(ops.encoder_block_ws_floats(B, P, W), device=dev, dtype=torch.float32)
        for l, w in enumerate(fw):
            self.launches += 1
            ops.encoder_block_fwd(dict(Zin=zs[l], Zout=zs[l + 1], **w), B, P, W, 8, ws, 1e-5, dt)
        sv.update(layers=None, fused_ws=ws)

    def _blocks_bwd_fused(self, sv, pk, dz, dt):
        """Per block, last to first: sea_encoder_block_bwd (dZin and the wgrad operands) + one sea_wgrad_grouped of all the block's parameter
        gradients.  The operand buffers are reused from block to block (stream order: a block's wgrad launch precedes the next block's backward)."""
        fw = pk["fused_w"]
        B, P, M = sv["B"], sv["P"], sv["M"]
        W = dz.shape[1]
        S = 4 * W
        dev = dz.device
        e = lambda *shape, dtype=dt: torch.empty(*shape, device=dev, dtype=dtype)  # noqa: E731
        op = dict(n1=e(M, W), dqkv=e(M, 3 * W), att=e(M, W), dz1=e(M, W), n2=e(M, W), dh=e(M, S), hg=e(M, S), dz2=e(M, W), u1=e(M, W), u2=e(M, W),
                  u3w=e(M, S), u3b=e(M, S))
        scratch = torch.zeros(S, 8, device=dev, dtype=torch.float32)   # the dW of the column-sum groups: not read
        gv = self.grad_view
        dz_in = torch.empty_like(dz)
        for l in reversed(range(len(fw))):
            pre = f"encode.blocks.{l}."
            self.launches += 1
            ops.encoder_block_bwd(dict(Zin=sv["zs"][l], dZout=dz, dZin=dz_in, **fw[l], **op), B, P, W, 8, sv["fused_ws"], 1e-5, dt)
            x8 = op["n1"][:, :8]
            groups = [dict(dY=op["dqkv"][:, i * W:(i + 1) * W], X=op["n1"], dW=gv(pre + f"attn_1.{c}.weight"), db=gv(pre + f"attn_1.{c}.bias"))
                      for i, c in enumerate("qkv")]
            groups += [dict(dY=op["dz1"], X=op["att"], dW=gv(pre + "attn_1.projection.weight")),
                       dict(dY=op["dh"], X=op["n2"], dW=gv(pre + "mlp_1.layers.0.weight"), db=gv(pre + "mlp_1.layers.0.bias")),
                       dict(dY=op["dz2"], X=op["hg"], dW=gv(pre + "mlp_1.layers.3.weight"), db=gv(pre + "mlp_1.layers.3.bias")),
                       dict(dY=op["u1"], X=x8, dW=scratch[:W], db=gv(pre + "ln_exp1_1.weight")),
                       dict(dY=op["u2"], X=x8, dW=scratch[:W], db=gv(pre + "ln_exp1_2.weight")),
                       dict(dY=op["u3w"], X=x8, dW=scratch, db=gv(pre + "mlp_1.layers.1.weight")),
                       dict(dY=op["u3b"], X=x8, dW=scratch, db=gv(pre + "mlp_1.layers.1.bias"))]
            self._wgrad(groups, dt)
            dz, dz_in = dz_in, dz
        return dz

    # ---------------------------------------------------------------- forward with saved activations
    def forward_train(self, x: torch.Tensor):
        """x [B, P, F, n_inp] (already masked) -> (out [B, P, F, n_inp] strided view of the padded output, saved activations)."""
        enc, dec = self.model.encode, self.model.decode
        dt = torch.float32 if enc.compute_dtype == "fp32" else torch.bfloat16
        if dec.compute_dtype != enc.compute_dtype:
            raise ValueError("sea_amd.SpatialModel: encoder and decoder compute dtypes differ")
        dev = x.device
        B, P, F, C = x.shape
        assert F == sum(len(g) for g in enc.field_groups) and C == enc.n_inp, (x.shape, enc.field_groups, enc.n_inp)
        if P > enc.spatial_pos_encoder.pe.shape[1]:
            raise ValueError(f"{P} patches exceed the positional table ({enc.spatial_pos_encoder.pe.shape[1]})")
        pk = enc._packed(dt, dev)
        T = self._enc_T(pk)
        G, E, H, hdp, Wp = enc.num_groups, enc.embed_dim, enc.n_heads, pk["hdp"], pk["Wp"]
        W, S, Hd = G * E, 4 * G * E, enc.MLP_hidden
        M, cap = B * P, _round_up(P, 8)
        f32 = torch.float32
        e = lambda *shape, dtype=dt: torch.empty(*shape, device=dev, dtype=dtype)  # noqa: E731
        z = lambda *shape, dtype=dt: torch.zeros(*shape, device=dev, dtype=dtype)  # noqa: E731
        sv = dict(dt=dt, B=B, P=P, M=M, cap=cap, pk=pk, T=T)

        # down-scale MLPs + positions
        xf = x.detach().to(f32)
        if enc._n_inp_p != C:
            xf = torch.nn.functional.pad(xf, (0, enc._n_inp_p - C))
        xf = xf.contiguous().view(M, F * enc._n_inp_p)
        A = [z(M, g["Kp"]) for g in pk["enc"]]
        for g, a in zip(pk["enc"], A):
            self.launches += 1
            ops.convert(xf[:, g["col0"]:g["col0"] + g["K"]], a[:, :g["K"]])
        pre = [e(M, Hd) for _ in pk["enc"]]
        hid = [e(M, Hd) for _ in pk["enc"]]
        self._gemm([dict(A=a, W=g["W1"], Cact=h, Z=p, act=1) for g, a, h, p in zip(pk["enc"], A, hid, pre)], dt)
        pe = enc.spatial_pos_encoder.pe[0, :P].to(dev, f32).repeat(B, 1).contiguous()
        zs = [e(M, W, dtype=f32) for _ in range(len(pk["blocks"]) + 1)]
        self._gemm([dict(A=h, W=g["W2"], bias=g["b2"], R=pe[:, i * E:(i + 1) * E], C32=zs[0][:, i * E:(i + 1) * E])
                    for i, (g, h) in enumerate(zip(pk["enc"], hid))], dt)
        sv.update(A=A, enc_pre=pre, enc_hid=hid, zs=zs)

        sv["fused"] = _switches.plan("enc", "composed") == "fused" and ops.encoder_block_supported(dt, W, H, P)   # composed: measured faster
        if sv["fused"]:
            self._blocks_fwd_fused(sv, pk, zs, B, P, W, dt, dev)
        else:
            rope = torch.zeros(cap, hdp // 2, 2, device=dev, dtype=f32)
            rope[..., 0] = 1.0   # identity rotation: this attention has no positional rotation
            sv["rope"] = rope
            layers = []
            for l, blk in enumerate(pk["blocks"]):
                zin, zout = zs[l], zs[l + 1]
                a = dict(zmid=e(M, W, dtype=f32), n1=e(M, W), m1=e(M, dtype=f32), r1=e(M, dtype=f32), Q=e(B, H, P, hdp), K=z(B, H, cap, hdp),
                         Vt=z(B, H, hdp, cap), V=z(B, H, cap, hdp), att=e(B, P, Wp), lse=e(B, H, P, dtype=f32), n2=e(M, W), m2=e(M, dtype=f32),
                         r2=e(M, dtype=f32), h=e(M, S), m3=e(M, dtype=f32), r3=e(M, dtype=f32), hg=e(M, S))
                self._norm([dict(X=zin, gamma=blk["g1"], Yact=a["n1"], mean=a["m1"], rstd=a["r1"])], M, W, False, False, 1e-5, dt)
                self.launches += 1
                ops.qkv_rope_grouped([dict(A=a["n1"], W=blk["wqkv"], bias=blk["bqkv"], col0=0, Q=a["Q"], K=a["K"], Vt=a["Vt"], V=a["V"])], rope, H, hdp, P, 0,
                                     cap, ops.q_scale(pk["hd"]), dt)
                self.launches += 1
                ops.attention_fwd([dict(Q=a["Q"], K=a["K"], Vt=a["Vt"], O=a["att"], LSE=a["lse"])], B, H, hdp, P, P, cap, 0, P, dt)
                a["Vt"] = None   # the backward reads the row-major copy
                self._gemm([dict(A=a["att"].view(M, Wp), W=blk["wo"], R=zin, C32=a["zmid"])], dt)
                self._norm([dict(X=a["zmid"], gamma=blk["g2"], Yact=a["n2"], mean=a["m2"], rstd=a["r2"])], M, W, False, False, 1e-5, dt)
                self._gemm([dict(A=a["n2"], W=blk["w1"], bias=blk["b1"], Cact=a["h"])], dt)
                self._norm([dict(X=a["h"], gamma=blk["lnw"], beta=blk["lnb"], Yact=a["hg"], mean=a["m3"], rstd=a["r3"])], M, S, dt != f32, True, 1e-5, dt)
                self._gemm([dict(A=a["hg"], W=blk["w2"], bias=blk["b2"], R=a["zmid"], C32=zout)], dt)
                layers.append(a)
            sv["layers"] = layers
        zenc = e(M, W, dtype=f32)
        sv["mf"], sv["rf"] = e(M, dtype=f32), e(M, dtype=f32)
        self._norm([dict(X=zs[-1], gamma=pk["fin_w"], beta=pk["fin_b"], Y32=zenc, mean=sv["mf"], rstd=sv["rf"])], M, W, False, False, enc.ln.eps, dt)

        # decoder (the same two grouped launches as Decode.forward, with the GELU pre-activation kept)
        W1d, W2d = dec._weights(dt)
        b2d = dec._shadow[3]
        D, Cp = dec.embed_dim, dec._n_inp_p
        za = self._act(zenc, dt)
        dpre = [e(M, dec.MLP_hidden) for _ in range(G)]
        dhid = [e(M, dec.MLP_hidden) for _ in range(G)]
        self._gemm([dict(A=za[:, g * D:(g + 1) * D], W=W1d[g], Cact=dhid[g], Z=dpre[g], act=1) for g in range(G)], dt)
        out = e(M, F * Cp, dtype=f32)
        groups, off = [], 0
        for g, grp in enumerate(dec.field_groups):
            w = len(grp) * Cp
            groups.append(dict(A=dhid[g], W=W2d[g], bias=b2d[g], C32=out[:, off:off + w]))
            off += w
        self._gemm(groups, dt)
        sv.update(za=za, dec_pre=dpre, dec_hid=dhid, W1d=W1d, W2d=W2d)
        return out.view(B, P, F, Cp)[..., :C], sv

    # ---------------------------------------------------------------- backward
    def backward(self, sv, dout: torch.Tensor) -> None:
        """dout: gradient of the real output columns [B, P, F, n_inp]; parameter gradients are ADDED to the flat gradient buffer."""
        enc, dec = self.model.encode, self.model.decode
        dt, B, P, M, cap, pk, T = sv["dt"], sv["B"], sv["P"], sv["M"], sv["cap"], sv["pk"], sv["T"]
        dev = dout.device
        f32 = torch.float32
        G, E, H, hd, hdp, Wp = enc.num_groups, enc.embed_dim, enc.n_heads, pk["hd"], pk["hdp"], pk["Wp"]
        W, S = G * E, 4 * G * E
        D, Cp, C = dec.embed_dim, dec._n_inp_p, dec.n_inp
        F = sum(len(g) for g in dec.field_groups)
        e = lambda *shape, dtype=dt: torch.empty(*shape, device=dev, dtype=dtype)  # noqa: E731
        gv = self.grad_view
        self.ensure_grads()
        fixups = []   # (gradient view, function returning the real part of its padded temporary): added once the weight-gradient launches are queued

        # ---- decoder
        dpad = torch.zeros(B, P, F, Cp, device=dev, dtype=f32)
        dpad[..., :C] = dout
        da = self._act(dpad.view(M, F * Cp), dt)
        W1T, W2T = self._dec_T(dec, sv["W1d"], sv["W2d"])
        dpre = [e(M, dec.MLP_hidden) for _ in range(G)]
        wg, off = [], 0
        dgemm = []
        for g, grp in enumerate(dec.field_groups):
            w = len(grp) * Cp
            dW2, db2 = gv(f"decode.decoders.{g}.layer2.weight"), gv(f"decode.decoders.{g}.layer2.bias")
            if Cp != C:
                dW2t, db2t = torch.zeros(w, dec.MLP_hidden, device=dev, dtype=f32), torch.zeros(w, device=dev, dtype=f32)
                fixups.append((dW2, lambda t=dW2t, n=len(grp), shp=dW2.shape: t.view(n, Cp, -1)[:, :C].reshape(shp)))
                fixups.append((db2, lambda t=db2t, n=len(grp), shp=db2.shape: t.view(n, Cp)[:, :C].reshape(shp)))
                dW2, db2 = dW2t, db2t
            wg.append(dict(dY=da[:, off:off + w], X=sv["dec_hid"][g], dW=dW2, db=db2))
            dgemm.append(dict(A=da[:, off:off + w], W=W2T[g], act=2, Z=sv["dec_pre"][g], Cact=dpre[g]))
            off += w
        self._gemm(dgemm, dt)
        for g in range(G):
            wg.append(dict(dY=dpre[g], X=sv["za"][:, g * D:(g + 1) * D], dW=gv(f"decode.decoders.{g}.layer1.weight")))
        self._wgrad(wg, dt)
        dzenc = e(M, W, dtype=f32)
        self._gemm([dict(A=dpre[g], W=W1T[g], C32=dzenc[:, g * D:(g + 1) * D]) for g in range(G)], dt)

        # ---- final LayerNorm
        dz = e(M, W, dtype=f32)
        self._norm_bwd([dict(dY=dzenc, X=sv["zs"][-1], gamma=pk["fin_w"], beta=pk["fin_b"], mean=sv["mf"], rstd=sv["rf"], dX32=dz,
                             dgamma=gv("encode.ln.weight"), dbeta=gv("encode.ln.bias"))], M, W, False, False, False, False, dt)

        # ---- EncoderBlocks, last to first: fused (two launches per block) or composed
        if sv["fused"]:
            dz = self._blocks_bwd_fused(sv, pk, dz, dt)
        else:
            pad = hd != hdp
            for l in reversed(range(len(pk["blocks"]))):
                a, blk, bt = sv["layers"][l], pk["blocks"][l], T["blocks"][l]
                pre = f"encode.blocks.{l}."
                zin = sv["zs"][l]
                # MLP: fc2, LayerNorm + GELU, fc1
                dza = self._act(dz, dt)
                dhg, dh = e(M, S), e(M, S)
                self._gemm([dict(A=dza, W=bt["w2"], Cact=dhg)], dt)
                self._norm_bwd([dict(dY=dhg, X=a["h"], gamma=blk["lnw"], beta=blk["lnb"], mean=a["m3"], rstd=a["r3"], dXact=dh,
                                     dgamma=gv(pre + "mlp_1.layers.1.weight"), dbeta=gv(pre + "mlp_1.layers.1.bias"))], M, S, dt != f32, dt != f32, True, False, dt)
                dn = e(M, W, dtype=f32)
                self._gemm([dict(A=dh, W=bt["w1"], C32=dn)], dt)
                self._wgrad([dict(dY=dza, X=a["hg"], dW=gv(pre + "mlp_1.layers.3.weight"), db=gv(pre + "mlp_1.layers.3.bias")),
                             dict(dY=dh, X=a["n2"], dW=gv(pre + "mlp_1.layers.0.weight"), db=gv(pre + "mlp_1.layers.0.bias"))], dt)
                # weight-only ln_exp1_2 (+ the residual)
                self._norm_bwd([dict(dY=dn, X=a["zmid"], gamma=blk["g2"], mean=a["m2"], rstd=a["r2"], dX32=dz, dgamma=gv(pre + "ln_exp1_2.weight"))],
                               M, W, False, False, False, True, dt)
                # projection, attention
                dza = self._act(dz, dt)
                datt = e(B, P, Wp)
                self._gemm([dict(A=dza, W=bt["wo"], Cact=datt.view(M, Wp))], dt)
                dqkv = e(M, 3 * Wp)
                delta = e(B, H, P, dtype=f32)
                self.launches += 1
                ops.attention_bwd([dict(Q=a["Q"], K=a["K"], V=a["V"], O=a["att"], dO=datt, LSE=a["lse"], delta=delta, dQ=dqkv[:, :Wp], dK=dqkv[:, Wp:2 * Wp],
                                        dV=dqkv[:, 2 * Wp:])], sv["rope"], B, H, hdp, P, P, cap, 0, P, ops.q_scale(hd), dt)
                dn = e(M, W, dtype=f32)
                self._gemm([dict(A=dqkv, W=bt["wqkv"], C32=dn)], dt)
                dWo = gv(pre + "attn_1.projection.weight")
                wg = []
                if pad:
                    t = torch.zeros(W, Wp, device=dev, dtype=f32)
                    fixups.append((dWo, lambda t=t: t.view(W, H, hdp)[:, :, :hd].reshape(W, W)))
                    dWo = t
                wg.append(dict(dY=dza, X=a["att"].view(M, Wp), dW=dWo))
                for i, which in enumerate("qkv"):
                    dWq, dbq = gv(pre + f"attn_1.{which}.weight"), gv(pre + f"attn_1.{which}.bias")
                    if pad:
                        tw, tb = torch.zeros(Wp, W, device=dev, dtype=f32), torch.zeros(Wp, device=dev, dtype=f32)
                        fixups.append((dWq, lambda t=tw: t.view(H, hdp, W)[:, :hd].reshape(W, W)))
                        fixups.append((dbq, lambda t=tb: t.view(H, hdp)[:, :hd].reshape(W)))
                        dWq, dbq = tw, tb
                    wg.append(dict(dY=dqkv[:, i * Wp:(i + 1) * Wp], X=a["n1"], dW=dWq, db=dbq))
                self._wgrad(wg, dt)
                # weight-only ln_exp1_1 (+ the residual)
                self._norm_bwd([dict(dY=dn, X=zin, gamma=blk["g1"], mean=a["m1"], rstd=a["r1"], dX32=dz, dgamma=gv(pre + "ln_exp1_1.weight"))],
                               M, W, False, False, False, True, dt)

        # ---- down-scale MLPs (no gradient to the input; the positional table is a buffer)
        dza = self._act(dz, dt)
        dpre = [e(M, enc.MLP_hidden) for _ in pk["enc"]]
        self._gemm([dict(A=dza[:, i * E:(i + 1) * E], W=T["enc"][i], act=2, Z=sv["enc_pre"][i], Cact=dpre[i]) for i in range(G)], dt)
        wg = []
        Cpe = enc._n_inp_p
        for i, (g, grp) in enumerate(zip(pk["enc"], enc.field_groups)):
            wg.append(dict(dY=dza[:, i * E:(i + 1) * E], X=sv["enc_hid"][i], dW=gv(f"encode.encoders.{i}.layer2.weight"), db=gv(f"encode.encoders.{i}.layer2.bias")))
            dW1 = gv(f"encode.encoders.{i}.layer1.weight")
            t = torch.zeros(enc.MLP_hidden, g["Kp"], device=dev, dtype=f32)
            fixups.append((dW1, lambda t=t, K=g["K"], n=len(grp), shp=dW1.shape: t[:, :K].view(enc.MLP_hidden, n, Cpe)[:, :, :enc.n_inp].reshape(shp)))
            wg.append(dict(dY=dpre[i], X=sv["A"][i], dW=t))
        self._wgrad(wg, dt)
        for dst, real_part in fixups:
            dst.add_(real_part())
        self.grads_dirty = True


class _SpatialFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, x, model, eng):
        out, sv = eng.forward_train(x)
        ctx.sv, ctx.eng, ctx.model = sv, eng, model   # every forward keeps its own activations: two forwards before their backwards are fine
        return out

    @staticmethod
    def backward(ctx, dout):
        eng, model = ctx.eng, ctx.model
        if ctx.sv is None:
            raise RuntimeError("sea_amd: backward() through a SpatialModel forward a second time (its saved activations are freed after the first)")
        live = model._live_params()
        # torch semantics: gradients accumulate until zero_grad(); a step that starts from p.grad is None starts from zero
        if eng.grads_dirty and live and live[0].grad is None:
            eng.zero_grads()
        eng.backward(ctx.sv, dout.float())
        for name, p in zip(eng.params.live_names, live):
            if p.grad is None:
                p.grad = eng.grad_view(name)
        ctx.sv = None
        return None, None, None, None


def spatial_forward_with_grad(model, eng, x):
    return _SpatialFn.apply(model._grad_anchor(), x, model, eng)
