"""Spatial decoder of the rollout's consumer side: the reference's `Decode` module
(models/encoder_decoder.py:126-146) and its `upScaleMLP` (models/base_blocks.py:49-63) with the same constructor arguments,
parameter names and shapes, computed by two grouped-GEMM launches of libsea_hip.so (sea_gemm_grouped: Linear + GELU epilogue, then
Linear + bias written straight into the concatenated [B, P, n_fields, n_inp] output) — no per-group Python loop of ATen ops, no cat.

`PointwiseEncode` (models/encoder_decoder.py:75-123) is the inference forward of the 12-layer spatial encoder: the same
constructor, sub-module and parameter names, run as a fixed sequence of libsea_hip.so launches per chunk of snapshots — grouped down-scale
MLPs (GELU epilogue; the sinusoidal patch positions ride as the residual operand of the second Linear), and per EncoderBlock:
weight-only LayerNorm, fused q/k/v projection written in the attention layouts, un-masked flash attention (the causal kernel with the whole
row visible), projection + residual, LayerNorm, Linear, LayerNorm + GELU, Linear + residual.  `SpatialModel` ties encoder and decoder
together as the reference does; under grad its forward is the training path of sea_amd/spatial_train.py (forward with saved activations and a
hand-written backward), with grad disabled it is the inference path above, unchanged.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch
import torch.nn as nn

from .. import _native as N
from .. import ops
from .base_blocks import EncoderBlock, PositionalEncoding, downScaleMLP


class upScaleMLP(nn.Module):  # noqa: N801  (reference name, models/base_blocks.py:49)
    def __init__(self, d_model: int, d_output: int, hidden_dim: int):
        super().__init__()
        self.d_model, self.d_output, self.hidden_dim = d_model, d_output, hidden_dim
        self.layer1 = nn.Linear(d_model, hidden_dim, bias=False)
        self.activation = nn.GELU()
        self.layer2 = nn.Linear(hidden_dim, d_output)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        raise RuntimeError("sea_amd.upScaleMLP is a parameter container; call Decode.forward (grouped native launch)")


class Decode(nn.Module):
    """Decode(field_groups, n_inp, MLP_hidden, embed_dim, dropout=0.1).forward(z [B, P, n_groups, embed_dim]) -> [B, P, n_fields, n_inp].
    `dropout` is accepted and unused, as in the reference (models/encoder_decoder.py:127-136 never applies it)."""

    def __init__(self, field_groups: Sequence[Sequence[int]], n_inp: int, MLP_hidden: int, embed_dim: int, dropout: float = 0.1):
        super().__init__()
        self.field_groups = [list(g) for g in field_groups]
        self.num_groups = len(self.field_groups)
        self.n_inp, self.MLP_hidden, self.embed_dim = n_inp, MLP_hidden, embed_dim
        self.decoders = nn.ModuleList([upScaleMLP(d_model=embed_dim, d_output=n_inp * len(g), hidden_dim=MLP_hidden) for g in self.field_groups])
        self.compute_dtype = "fp32"
        self._shadow = None  # (key, [W1 act], [W2 act])
        if embed_dim % 8 or MLP_hidden % 8:
            raise NotImplementedError("sea_amd.Decode: embed_dim and MLP_hidden must be multiples of 8 (16-byte operand rows)")
        # a field's output columns are padded to whole 128-byte lines inside (n_inp is the padded cell size: data-dependent in the reference): every row and
        # every field of the fp32 output then starts on a cache line — rows at odd multiples of 16 B cost the second layer 12 % (1.48 -> 1.29 ms for the
        # 2.5 GB of a 2024-snapshot rollout: partial lines at both ends of every 512-byte tile row)
        self._n_inp_p = (n_inp + 31) // 32 * 32

    def set_compute_dtype(self, dtype) -> "Decode":
        name = {torch.float32: "fp32", torch.bfloat16: "bf16"}.get(dtype, dtype)
        if name not in ("fp32", "bf16"):
            raise ValueError("compute dtype must be 'fp32' or 'bf16'")
        self.compute_dtype, self._shadow = name, None
        return self

    def _weights(self, dt: torch.dtype):
        """Activation-dtype copies of the Linear weights, refreshed when a parameter was written (version counter) or moved."""
        ps = [d.layer1.weight for d in self.decoders] + [d.layer2.weight for d in self.decoders] + [d.layer2.bias for d in self.decoders]
        key = (dt, tuple((p.data_ptr(), p._version) for p in ps))
        if self._shadow is None or self._shadow[0] != key:
            with torch.no_grad():
                conv = lambda p: p.detach().contiguous() if dt == torch.float32 else p.detach().to(dt).contiguous()
                C, Cp = self.n_inp, self._n_inp_p

                def pad_out(t, grp):   # layer2 rows / bias entries of field f at [f C, (f + 1) C) -> [f Cp, f Cp + C); the pad rows are zero
                    if Cp == C:
                        return t.detach()
                    out = torch.zeros((len(grp), Cp) + tuple(t.shape[1:]), device=t.device, dtype=t.dtype)
                    out[:, :C] = t.detach().view((len(grp), C) + tuple(t.shape[1:]))
                    return out.view((len(grp) * Cp,) + tuple(t.shape[1:]))

                self._shadow = (key, [conv(d.layer1.weight) for d in self.decoders], [conv(pad_out(d.layer2.weight, g)) for d, g in zip(self.decoders, self.field_groups)],
                                [pad_out(d.layer2.bias, g).float().contiguous() for d, g in zip(self.decoders, self.field_groups)])
        return self._shadow[1], self._shadow[2]

    def forward(self, z: torch.Tensor) -> torch.Tensor:
        N.require_gpu(z, "Decode input")
        if z.requires_grad and torch.is_grad_enabled():
            self._require_frozen("forward")
            return _DecodeFn.apply(z, self)
        B, P, G, D = z.shape
        assert G == self.num_groups and D == self.embed_dim, (z.shape, self.num_groups, self.embed_dim)
        dt = torch.float32 if self.compute_dtype == "fp32" else torch.bfloat16
        M = B * P
        zf = z.detach().to(torch.float32).contiguous().view(M, G * D)
        za = zf if dt == torch.float32 else torch.empty(M, G * D, device=z.device, dtype=dt)
        if dt != torch.float32:
            ops.convert(zf, za)
        W1, W2 = self._weights(dt)
        n_fields = sum(len(g) for g in self.field_groups)
        Cp = self._n_inp_p
        out = torch.empty(M, n_fields * Cp, device=z.device, dtype=torch.float32)
        hid: List[torch.Tensor] = [torch.empty(M, self.MLP_hidden, device=z.device, dtype=dt) for _ in range(G)]
        ops.gemm_grouped([dict(A=za[:, g * D:(g + 1) * D], W=W1[g], Cact=hid[g], act=1) for g in range(G)], dt)
        groups, off = [], 0
        for g, grp in enumerate(self.field_groups):
            w = len(grp) * Cp
            groups.append(dict(A=hid[g], W=W2[g], bias=self._shadow[3][g], C32=out[:, off:off + w]))
            off += w
        ops.gemm_grouped(groups, dt)
        out = out.view(B, P, n_fields, Cp)
        return out if Cp == self.n_inp else out[..., :self.n_inp]   # a strided view: sea_unpatchify reads it in place

    # ------------------------------------------------------------------ gradients to z (the decoder as a frozen observation operator)
    def _require_frozen(self, what: str) -> None:
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise ValueError(f"sea_amd.Decode.{what}: gradients flow to z only, but a decoder parameter requires grad and would silently get none: call "
                             "decoder.requires_grad_(False) to use the decoder as a frozen observation operator (training the decoder itself is "
                             "SpatialModel's training path)")

    def _act_dtype(self) -> torch.dtype:
        return torch.float32 if self.compute_dtype == "fp32" else torch.bfloat16

    def _weights_T(self, dt: torch.dtype):
        """W1^T [D, S] and W2^T [S, n_fields * Cp] of every group in the activation dtype: the operands of the two data-gradient launches (kept under the
        attribute the spatial training engine uses, refreshed with the shadow copies)."""
        W1, W2 = self._weights(dt)
        cur = getattr(self, "_shadow_T", None)
        if cur is None or cur[0] is not self._shadow:
            cur = (self._shadow, [w.t().contiguous() for w in W1], [w.t().contiguous() for w in W2])
            self._shadow_T = cur
        return cur[1], cur[2]

    def _first_layer(self, z: torch.Tensor, dt: torch.dtype):
        """forward()'s first grouped launch with the GELU pre-activation kept: (hidden rows, pre-activations), each a list of [M, MLP_hidden] per group."""
        B, P, G, D = z.shape
        assert G == self.num_groups and D == self.embed_dim, (z.shape, self.num_groups, self.embed_dim)
        M = B * P
        zf = z.detach().to(torch.float32).contiguous().view(M, G * D)
        za = zf if dt == torch.float32 else torch.empty(M, G * D, device=z.device, dtype=dt)
        if dt != torch.float32:
            ops.convert(zf, za)
        W1, _ = self._weights(dt)
        hid = [torch.empty(M, self.MLP_hidden, device=z.device, dtype=dt) for _ in range(G)]
        pre = [torch.empty(M, self.MLP_hidden, device=z.device, dtype=dt) for _ in range(G)]
        ops.gemm_grouped([dict(A=za[:, g * D:(g + 1) * D], W=W1[g], Cact=hid[g], Z=pre[g], act=1) for g in range(G)], dt)
        return hid, pre

    def _input_grad(self, dpre: List[torch.Tensor], dt: torch.dtype) -> torch.Tensor:
        """dz [M, G * D] f32 from the pre-activation gradients of the groups: one grouped data-gradient launch against W1^T."""
        W1T, _ = self._weights_T(dt)
        D = self.embed_dim
        dz = torch.empty(dpre[0].shape[0], self.num_groups * D, device=dpre[0].device, dtype=torch.float32)
        ops.gemm_grouped([dict(A=dpre[g], W=W1T[g], C32=dz[:, g * D:(g + 1) * D]) for g in range(self.num_groups)], dt)
        return dz

    def _valid_counts(self, counts, P: int, device: torch.device, allow_empty: bool = False, what: str = "mse_loss"):
        """(device int32 [P] or None, valid cells summed over the patches) for mse_loss and member_sse; checked on the host, cached per counts object.
        allow_empty: counts that leave no valid element are accepted (a sum of squares over nothing is 0; a mean is undefined); what: the caller named in the messages."""
        if counts is None:
            return None, P * self.n_inp
        key = (id(counts), getattr(counts, "_version", None), P, device)
        cur = getattr(self, "_counts_cache", None)
        if cur is not None and cur[0] == key:
            if cur[2] < 1 and not allow_empty:
                raise ValueError(f"sea_amd.Decode.{what}: counts leave no valid element")
            return cur[1], cur[2]
        host = counts.detach().cpu() if torch.is_tensor(counts) else torch.as_tensor(list(counts))
        if host.dim() != 1 or host.shape[0] != P or host.is_floating_point() or host.is_complex() or host.dtype == torch.bool:
            raise ValueError(f"sea_amd.Decode.{what}: counts must be {P} integers (one per patch), got shape {tuple(host.shape)} {host.dtype}")
        if int(host.min()) < 0 or int(host.max()) > self.n_inp:
            raise ValueError(f"sea_amd.Decode.{what}: counts must lie in [0, n_inp = {self.n_inp}], got {int(host.min())} .. {int(host.max())}")
        total = int(host.sum())
        if total < 1 and not allow_empty:
            raise ValueError(f"sea_amd.Decode.{what}: counts leave no valid element")
        dev = host.to(device=device, dtype=torch.int32).contiguous()
        self._counts_cache = (key, dev, total, counts)   # the object is kept so that its id is not reused
        return dev, total

    def mse_loss(self, z: torch.Tensor, target: torch.Tensor, counts=None, fused: Optional[bool] = None) -> torch.Tensor:
        """Mean squared error of the decoded fields against `target` over the valid elements, as a 0-dim fp32 tensor; gradient flows to z only.
        z [B, P, n_groups, embed_dim]; target float32 [B, P, n_fields, C] with C == n_inp or any wider row (e.g. c_out of patchify_and_scale: only the
        first n_inp columns of a row are read); counts: None (every column of a cell is valid: the value equals F.mse_loss(decode(z), target)) or one
        integer per patch in [0, n_inp] — the cell's mesh points are the first counts[p] slots of its rows, the rest is padding that contributes neither
        loss nor gradient.  bf16 compute dtype: ONE fused launch (sea_decode_mse) between the two small-K ends — the decoded fields are never written;
        fp32 compute dtype: forward() + the loss in eager launches.  `fused` forces either path (None: fused in bf16, except at the one measured size where
        the composed path is faster: hidden width above 512, no counts, fewer than 16384 rows — the fused path there is leaner, not faster)."""
        n_fields = sum(len(g) for g in self.field_groups)
        C = self.n_inp
        if z.dim() != 4 or z.shape[2] != self.num_groups or z.shape[3] != self.embed_dim:
            raise ValueError(f"sea_amd.Decode.mse_loss: z must be [B, P, {self.num_groups}, {self.embed_dim}], got {tuple(z.shape)}")
        B, P = z.shape[0], z.shape[1]
        if target.dim() != 4 or tuple(target.shape[:3]) != (B, P, n_fields) or target.shape[3] < C:
            raise ValueError(f"sea_amd.Decode.mse_loss: target must be [{B}, {P}, {n_fields}, >= {C}], got {tuple(target.shape)}")
        if target.dtype != torch.float32 or target.device != z.device:
            raise ValueError(f"sea_amd.Decode.mse_loss: target must be float32 on {z.device}, got {target.dtype} on {target.device}")
        if target.requires_grad and torch.is_grad_enabled():
            raise ValueError("sea_amd.Decode.mse_loss: the target must not require grad (gradients flow to z only)")
        self._require_frozen("mse_loss")
        dt = self._act_dtype()
        if fused is None:
            # measured (tools/decode_loss_bench.py): the fused launch is the faster path everywhere except at the padded hidden width 640 with
            # every column valid and few rows (multiphase decoder, B = 1: 1.10 against 1.05 ms), where the composed path stays the default
            fused = dt == torch.bfloat16 and not (counts is None and self.MLP_hidden > 512 and B * P < 16384)
        if fused and dt != torch.bfloat16:
            raise ValueError("sea_amd.Decode.mse_loss: the fused launch is bf16 only (set_compute_dtype('bf16'), or fused=False)")
        cnt, per_snapshot = self._valid_counts(counts, P, z.device)
        n_valid = B * n_fields * per_snapshot
        N.require_gpu(z, "Decode.mse_loss input")
        if fused:
            return _DecodeMseFn.apply(z, self, target, cnt, n_valid)
        y = self.forward(z)
        t = target[..., :C]
        if cnt is None:
            from ..autograd import MSELossFn

            return MSELossFn.apply(y, t)
        valid = (torch.arange(C, device=z.device) < cnt[:, None]).view(1, P, 1, C)
        d = torch.where(valid, y - t, torch.zeros((), device=z.device))
        return (d * d).sum() / n_valid

    def member_sse(self, z: torch.Tensor, target: torch.Tensor, counts=None, members: int = 1, fused: Optional[bool] = None) -> torch.Tensor:
        """Squared error of the decoded fields of every ensemble member against an observation, summed over a member's patches and valid cells:
        fp32 [Bm, n_fields], no autograd graph.  z [Bm, P, n_groups, embed_dim] holds `members` consecutive members per history (row b * members + j is
        member j of history b, as RolloutSession.fork orders them); target float32 [Bm / members, P, n_fields, C >= n_inp] is one observation per
        history; counts as in mse_loss (counts that leave no valid element are accepted here: every score is then 0).  bf16 compute dtype: the
        first-layer launch plus ONE fused launch (sea_decode_member_sse) — the decoded fields are never written; fp32, or fused=False: forward() plus
        torch reductions over its output (the composed path).  `fused` forces either path; None: fused in bf16 from 8192 rows (Bm * P) on, composed
        below — measured (tools/ensemble_bench.py, DESIGN.md section 7d, 64 members x 64 patches): at 4096 rows the composed path is the faster one
        (0.14 - 0.19 ms against 0.18 - 0.23 ms: the fused path's time there is its launches, not its kernel), except with the mesh's counts at the
        cylinder decoder, where the fused path is ahead by 2 % (0.180 against 0.184 ms) — too little to make the rule depend on counts; at 16384 rows
        the fused path is 2.1 - 3.1x faster; fused=True selects the leaner path (8 - 10 MB of extra memory against 229 MB at 4096 rows) at any size."""
        n_fields = sum(len(g) for g in self.field_groups)
        C = self.n_inp
        if z.dim() != 4 or z.shape[2] != self.num_groups or z.shape[3] != self.embed_dim:
            raise ValueError(f"sea_amd.Decode.member_sse: z must be [Bm, P, {self.num_groups}, {self.embed_dim}], got {tuple(z.shape)}")
        Bm, P = z.shape[0], z.shape[1]
        if not isinstance(members, int) or isinstance(members, bool) or members < 1 or Bm < 1 or Bm % members:
            raise ValueError(f"sea_amd.Decode.member_sse: members = {members!r} must be a positive integer that divides the {Bm} rows of z")
        B = Bm // members
        if target.dim() != 4 or tuple(target.shape[:3]) != (B, P, n_fields) or target.shape[3] < C:
            raise ValueError(f"sea_amd.Decode.member_sse: target must be [{B}, {P}, {n_fields}, >= {C}] (one observation per history of {members} members), "
                             f"got {tuple(target.shape)}")
        if target.dtype != torch.float32 or target.device != z.device:
            raise ValueError(f"sea_amd.Decode.member_sse: target must be float32 on {z.device}, got {target.dtype} on {target.device}")
        dt = self._act_dtype()
        if fused is None:
            fused = dt == torch.bfloat16 and Bm * P >= 8192
        if fused and dt != torch.bfloat16:
            raise ValueError("sea_amd.Decode.member_sse: the fused launch is bf16 only (set_compute_dtype('bf16'), or fused=False)")
        cnt, _ = self._valid_counts(counts, P, z.device, allow_empty=True, what="member_sse")
        N.require_gpu(z, "Decode.member_sse input")
        with torch.no_grad():
            if not fused:
                y = self.forward(z.detach()).view(B, members, P, n_fields, C)
                d = y - target.detach()[..., :C].unsqueeze(1)
                if cnt is not None:
                    valid = (torch.arange(C, device=z.device) < cnt[:, None]).view(1, 1, P, 1, C)
                    d = torch.where(valid, d, torch.zeros((), device=z.device))
                return (d * d).sum(dim=(2, 4)).view(Bm, n_fields)
            M = Bm * P
            t3 = target.detach().reshape(B * P, n_fields, target.shape[3])
            if t3.stride(2) != 1 or t3.stride(0) % 4 or t3.stride(1) % 4 or t3.data_ptr() % 16:
                # a contiguous observation of an odd cell width, or the reference's [.., C, n_fields] layout seen through a permute: one row-aligned copy
                src = t3[..., :C]
                t3 = torch.zeros(B * P, n_fields, (C + 3) // 4 * 4, device=src.device, dtype=torch.float32)
                t3[..., :C] = src
            G, D = self.num_groups, self.embed_dim
            zf = z.detach().to(torch.float32).contiguous().view(M, G * D)
            za = torch.empty(M, G * D, device=z.device, dtype=dt)
            ops.convert(zf, za)
            W1, W2 = self._weights(dt)
            hid = [torch.empty(M, self.MLP_hidden, device=z.device, dtype=dt) for _ in range(G)]
            ops.gemm_grouped([dict(A=za[:, g * D:(g + 1) * D], W=W1[g], Cact=hid[g], act=1) for g in range(G)], dt)
            bias = self._shadow[3]
            return ops.decode_member_sse([dict(H=hid[g], W2=W2[g], bias=bias[g]) for g in range(G)], t3, C, self._n_inp_p, P, members=members, counts=cnt, dtype=dt)

    def sensor_sse(self, z: torch.Tensor, sensors, obs: torch.Tensor, precision: Optional[torch.Tensor] = None, members: int = 1,
                   fused: Optional[bool] = None, predictions: bool = False):
        """Precision-weighted squared error of every ensemble member against SPARSE observations: fp32 [Bm], sum_k w_k (y_k - obs[b, k])^2 over the K
        sensors of `sensors` (a sea_amd.ensemble.SensorSet built for this decoder: sensor k reads decoded field field[k] at cell cell[k] of patch
        patch[k]); no autograd graph.  z [Bm, P, n_groups, embed_dim], member j of history b at row b * members + j; obs float32 [Bm / members, K] on
        z's device in the sensors' given order; precision None (1) or float32 [K] or [Bm / members, K], finite and >= 0: a sensor with w == 0 is
        neutral by a select whatever obs holds there, NaN and Inf included (a precision on the host is checked; one on the device is not read back —
        a negative or NaN entry there counts as 0).  predictions=True: returns (wsse, pred) with pred fp32 [Bm, K], the decoded value of every member
        at every sensor in the given order (the innovation is pred - obs).
        bf16 compute dtype, fused: the z rows of the observed patches gathered patch-major, the first-layer launch over those Q * Bm rows only, ONE
        fused launch (sea_decode_sensor_sse) and its finish launch — neither the decoded fields nor the unobserved patches' hidden rows exist; obs and
        precision come into the sorted, padded order of the set by one index_select each.  fp32, or fused=False: forward(), a gather of its output at
        the sensors, torch reductions (the composed path).  fused=None: the fused path in bf16 — it never does more arithmetic than the composed one
        (K columns against every cell), and no measured size has the composed path ahead (tools/sensor_bench.py, profiles/sensor_bench.txt, DESIGN.md section 7f;
        64 members x 64 patches, 16 - 4096 sensors: one history 0.10 - 0.12 ms fused against 0.12 - 0.14 ms composed, level within the windows' spread in two
        rows; four histories 0.10 - 0.14 against 0.21 - 0.29 ms; 0.5 - 46 MB of extra memory against 84 - 348 MB).  A call with device inputs reads nothing back and
        uploads nothing once the set's tables are on the device.
        `sensors` may be a sea_amd.ensemble.DerivedSensorSet (readings of a speed, an energy or a difference, plain sensors mixed in): obs then holds
        the readings in their own units, the fused launch is sea_decode_derived_sensor_sse (a reading is two adjacent entries of the sorted list), the
        composed path gathers both source values and applies the derived arithmetic in float32 torch ops, and fused=None takes the fused launch in
        bf16 only when every derived reading has its two sources in one decoder group (fused=True raises otherwise)."""
        from ..ensemble import DerivedSensorSet, SensorSet, _check_sensor_operands

        if z.dim() != 4 or z.shape[2] != self.num_groups or z.shape[3] != self.embed_dim:
            raise ValueError(f"sea_amd.Decode.sensor_sse: z must be [Bm, P, {self.num_groups}, {self.embed_dim}], got {tuple(z.shape)}")
        Bm, P = z.shape[0], z.shape[1]
        if not isinstance(members, int) or isinstance(members, bool) or members < 1 or Bm < 1 or Bm % members:
            raise ValueError(f"sea_amd.Decode.sensor_sse: members = {members!r} must be a positive integer that divides the {Bm} rows of z")
        B = Bm // members
        if not isinstance(sensors, SensorSet):
            raise ValueError(f"sea_amd.Decode.sensor_sse: sensors must be a SensorSet, got {type(sensors).__name__}")
        if not sensors.matches(self, P):
            raise ValueError(f"sea_amd.Decode.sensor_sse: the SensorSet was built for n_patches {sensors.n_patches}, n_inp {sensors.n_inp} (padded {sensors.Cp}), "
                             f"field groups {sensors.groups}; this call has n_patches {P}, n_inp {self.n_inp} (padded {self._n_inp_p}), field groups {self.field_groups}")
        K = sensors.K
        _check_sensor_operands("sea_amd.Decode.sensor_sse", obs, precision, B, K, z.device)
        dt = self._act_dtype()
        derived = isinstance(sensors, DerivedSensorSet)   # readings of derived quantities: the pair launch (sea_decode_derived_sensor_sse), or the composed path
        if fused is None:
            fused = dt == torch.bfloat16 and (not derived or sensors.fusable)
        if fused and dt != torch.bfloat16:
            raise ValueError("sea_amd.Decode.sensor_sse: the fused launch is bf16 only (set_compute_dtype('bf16'), or fused=False)")
        if fused and derived:
            sensors._require_fusable("sea_amd.Decode.sensor_sse")
        N.require_gpu(z, "Decode.sensor_sse input")
        T = sensors.tables(z.device)
        with torch.no_grad():
            obs = obs.detach()
            prec = None if precision is None else precision.detach()
            if not fused:
                y = self.forward(z.detach())                                              # [Bm, P, n_fields, C]
                pred = sensors.composed_predictions(y) if derived else y[:, T["patch"], T["out_field"], T["cell"]]   # [Bm, K]
                o = obs.unsqueeze(1).expand(B, members, K).reshape(Bm, K)
                if prec is None:
                    d = pred - o
                    wsse = (d * d).sum(1)
                else:
                    w = prec.view(1, 1, K).expand(B, members, K) if prec.dim() == 1 else prec.unsqueeze(1).expand(B, members, K)
                    w = w.reshape(Bm, K)
                    zero = torch.zeros((), device=z.device)
                    live = w > 0
                    w = torch.where(live, w, zero)
                    d = torch.where(live, pred - o, zero)
                    wsse = (w * d * d).sum(1)
                return (wsse, pred.contiguous()) if predictions else wsse
            G, D, Q = self.num_groups, self.embed_dim, sensors.Q
            zq = z.detach().index_select(1, T["patches"]).to(torch.float32).permute(1, 0, 2, 3).contiguous().view(Q * Bm, G * D)   # patch-major: row q * Bm + bm
            za = torch.empty(Q * Bm, G * D, device=z.device, dtype=dt)
            ops.convert(zq, za)
            W1, W2 = self._weights(dt)
            hid = [torch.empty(Q * Bm, self.MLP_hidden, device=z.device, dtype=dt) for _ in range(G)]
            ops.gemm_grouped([dict(A=za[:, g * D:(g + 1) * D], W=W1[g], Cact=hid[g], act=1) for g in range(G)], dt)
            bias = self._shadow[3]
            obs_s = obs.index_select(1, T["perm"])                                         # [B, K_pad]: sorted, padded (a pad entry repeats sensor 0 and is not live)
            prec_s = None if prec is None else prec.index_select(prec.dim() - 1, T["perm"])
            if derived:   # obs and prec through perm land on both entries of a pair (the launch reads the first); inv points at the first
                out = ops.decode_derived_sensor_sse([dict(H=hid[g], W2=W2[g], bias=bias[g]) for g in range(G)], obs_s, T["live"], T["wrow"], T["seg"], T["op"],
                                                    T["scale"], T["shift"], self._n_inp_p, members=members, prec=prec_s, predictions=predictions, dtype=dt)
            else:
                out = ops.decode_sensor_sse([dict(H=hid[g], W2=W2[g], bias=bias[g]) for g in range(G)], obs_s, T["live"], T["wrow"], T["seg"], self._n_inp_p,
                                            members=members, prec=prec_s, predictions=predictions, dtype=dt)
            if not predictions:
                return out
            return out[0], out[1].index_select(1, T["inv"])

    def sensor_loss(self, z: torch.Tensor, sensors, obs: torch.Tensor, precision: Optional[torch.Tensor] = None, members: int = 1,
                    fused: Optional[bool] = None, predictions: bool = False):
        """sensor_sse WITH a gradient to z: the precision-weighted squared error of every member against sparse observations, fp32 [Bm], as a
        differentiable tensor — gradient flows to z only (the decoder is a frozen observation operator: a parameter that requires grad is refused; obs
        and precision must not require grad).  Arguments as sensor_sse.  predictions=True: returns (wsse, pred) with pred fp32 [Bm, K], which carries
        no gradient.  wsse[bm] depends on z[bm] alone, so d (sum_bm c_bm wsse[bm]) / dz[bm] = c_bm d wsse[bm] / dz[bm]: this is what nudging, a
        3D-Var correction or a gradient move of resampled duplicates differentiates.
        bf16 compute dtype, fused: the z rows of the observed patches gathered patch-major, the first-layer launch over those Q * Bm rows with the
        pre-activation kept, ONE fused launch (sea_decode_sensor_grad: the score — sensor_sse's bits — and the gradient of the pre-activation, the
        weighted residual rounded to bf16 once between the two products) and its finish launch, the data-gradient launch against W1^T over Q * Bm
        rows, and one index_copy_ into a zeroed [Bm, P, n_groups, embed_dim]: the gradient at an unobserved patch, and at the slice of a group without
        sensors in a patch, is exactly 0.  Forward and backward are one pass, as in mse_loss: the backward scales the stored dz by the upstream
        gradient of every member.  fp32, or fused=False: forward() under autograd, a gather at the sensors and torch reductions (the composed path;
        its backward runs over all P patches).  fused=None: the fused path in bf16 — it never does more arithmetic than the composed one, and no
        measured size has the composed path ahead (tools/sensor_grad_bench.py, profiles/sensor_grad_bench.txt; 64 members x 64
        patches, 16 - 4096 sensors over 4 - 64 patches, loss + backward: one history 0.23 - 0.29 ms fused against 0.40 - 0.68 ms composed, four
        histories 0.23 - 0.33 against 0.83 - 0.97 ms, every row outside the windows' spread; 1.5 - 127 MB of extra memory against 206 - 846 MB; the
        score alone, sensor_sse, takes 0.09 - 0.12 ms).  A call with device inputs reads nothing back and uploads nothing once the set's tables
        are on the device.
        A sea_amd.ensemble.DerivedSensorSet is taken as in sensor_sse: the fused launch is sea_decode_derived_sensor_grad (the two partial derivatives
        of a reading weight the residuals of its two entries; exactly 0 at a zero speed), fused=None by the same rule."""
        from ..ensemble import DerivedSensorSet, SensorSet, _check_sensor_operands

        what = "sea_amd.Decode.sensor_loss"
        if z.dim() != 4 or z.shape[2] != self.num_groups or z.shape[3] != self.embed_dim:
            raise ValueError(f"{what}: z must be [Bm, P, {self.num_groups}, {self.embed_dim}], got {tuple(z.shape)}")
        Bm, P = z.shape[0], z.shape[1]
        if not isinstance(members, int) or isinstance(members, bool) or members < 1 or Bm < 1 or Bm % members:
            raise ValueError(f"{what}: members = {members!r} must be a positive integer that divides the {Bm} rows of z")
        B = Bm // members
        if not isinstance(sensors, SensorSet):
            raise ValueError(f"{what}: sensors must be a SensorSet, got {type(sensors).__name__}")
        if not sensors.matches(self, P):
            raise ValueError(f"{what}: the SensorSet was built for n_patches {sensors.n_patches}, n_inp {sensors.n_inp} (padded {sensors.Cp}), "
                             f"field groups {sensors.groups}; this call has n_patches {P}, n_inp {self.n_inp} (padded {self._n_inp_p}), field groups {self.field_groups}")
        K = sensors.K
        _check_sensor_operands(what, obs, precision, B, K, z.device)
        if torch.is_grad_enabled() and (obs.requires_grad or (precision is not None and precision.requires_grad)):
            raise ValueError(f"{what}: obs and precision must not require grad (gradients flow to z only)")
        self._require_frozen("sensor_loss")
        dt = self._act_dtype()
        derived = isinstance(sensors, DerivedSensorSet)
        if fused is None:
            fused = dt == torch.bfloat16 and (not derived or sensors.fusable)
        if fused and dt != torch.bfloat16:
            raise ValueError(f"{what}: the fused launch is bf16 only (set_compute_dtype('bf16'), or fused=False)")
        if fused and derived:
            sensors._require_fusable(what)
        N.require_gpu(z, "Decode.sensor_loss input")
        obs = obs.detach()
        prec = None if precision is None else precision.detach()
        if fused:
            out = _DecodeSensorFn.apply(z, self, sensors, obs, prec, members, predictions)
            return (out[0], out[1]) if predictions else out
        T = sensors.tables(z.device)
        y = _DecodeFn.apply(z, self)                                                  # [Bm, P, n_fields, C]
        pred = sensors.composed_predictions(y) if derived else y[:, T["patch"], T["out_field"], T["cell"]]   # [Bm, K]
        o = obs.unsqueeze(1).expand(B, members, K).reshape(Bm, K)
        if prec is None:
            d = pred - o
            wsse = (d * d).sum(1)
        else:
            w = prec.view(1, 1, K).expand(B, members, K) if prec.dim() == 1 else prec.unsqueeze(1).expand(B, members, K)
            w = w.reshape(Bm, K)
            zero = torch.zeros((), device=z.device)
            live = w > 0
            w = torch.where(live, w, zero)
            d = torch.where(live, pred - o, zero)
            wsse = (w * d * d).sum(1)
        return (wsse, pred.detach().contiguous()) if predictions else wsse

    def _sensor_grad_fused(self, z: torch.Tensor, sensors, obs: torch.Tensor, prec: Optional[torch.Tensor], members: int, predictions: bool, want_grad: bool):
        """The fused bf16 launches of sensor_loss on checked arguments, without autograd: (wsse [Bm], pred [Bm, K] or None, dz f32 [Bm, P, G, D] or None)."""
        from ..ensemble import DerivedSensorSet

        dt = torch.bfloat16
        derived = isinstance(sensors, DerivedSensorSet)
        if derived:
            sensors._require_fusable("sea_amd.Decode.sensor_loss")
        with torch.no_grad():
            Bm, P, G, D = z.shape
            T, Q = sensors.tables(z.device), sensors.Q
            zq = z.detach().index_select(1, T["patches"]).permute(1, 0, 2, 3)            # [Q, Bm, G, D] patch-major: row q * Bm + bm
            hid, pre = self._first_layer(zq, dt)
            _, W2 = self._weights(dt)
            bias = self._shadow[3]
            dpre = [torch.empty(Q * Bm, self.MLP_hidden, device=z.device, dtype=dt) for _ in range(G)]
            obs_s = obs.index_select(1, T["perm"])                                         # [B, K_pad]: sorted, padded (a pad entry repeats sensor 0 and is not live)
            prec_s = None if prec is None else prec.index_select(prec.dim() - 1, T["perm"])
            if derived:   # the pair launch (sea_decode_derived_sensor_grad)
                wsse, pred = ops.decode_derived_sensor_grad([dict(H=hid[g], W2=W2[g], bias=bias[g], dH=dpre[g], Z=pre[g]) for g in range(G)], obs_s, T["live"],
                                                            T["wrow"], T["seg"], T["op"], T["scale"], T["shift"], self._n_inp_p, members=members, prec=prec_s,
                                                            predictions=predictions, dtype=dt)
            else:
                wsse, pred = ops.decode_sensor_grad([dict(H=hid[g], W2=W2[g], bias=bias[g], dH=dpre[g], Z=pre[g]) for g in range(G)], obs_s, T["live"], T["wrow"],
                                                    T["seg"], self._n_inp_p, members=members, prec=prec_s, predictions=predictions, dtype=dt)
            if pred is not None:
                pred = pred.index_select(1, T["inv"])
            dz = None
            if want_grad:
                dz = torch.zeros(Bm, P, G, D, device=z.device, dtype=torch.float32)
                dz.index_copy_(1, T["patches"], self._input_grad(dpre, dt).view(Q, Bm, G, D).permute(1, 0, 2, 3))
            return wsse, pred, dz

    def field_loss(self, z: torch.Tensor, obs: torch.Tensor, members: int = 1, counts=None, precision: Optional[torch.Tensor] = None,
                   field_precision: Optional[torch.Tensor] = None, fused: Optional[bool] = None) -> torch.Tensor:
        """The DENSE-snapshot score with a precision map, per member and field, WITH a gradient to z: wsse fp32 [B * members, n_fields],
        wsse[bm, f] = sum over the member's patches and cells of w (y - obs)^2, as a differentiable tensor — gradient flows to z only (the decoder is a
        frozen observation operator: a parameter that requires grad is refused; obs, precision and field_precision must not require grad).
        z [B * members, P, n_groups, embed_dim] in fork() order (row b * members + j is member j of history b); obs float32 [B, P, n_fields, C >= n_inp]
        on z's device, one snapshot per history; members >= 1 (members = 1: one trajectory per snapshot); counts as in mse_loss (all-zero counts are
        accepted); precision: None or a float32 map of obs's shape, 0 marks a missing cell; field_precision: None or float32 [n_fields] on z's
        device.  The weight of a cell is w = valid && precision > 0 && field_precision > 0 ? field_precision * precision : 0, by selects: a cell
        without weight is neutral whatever obs and precision hold there, NaN included, and a patch without a weighted cell gets a gradient of
        exactly 0 (include/sea_hip.h, sea_decode_field_grad, states the formulas).
        Upstream gradients.  wsse[bm, f] depends on z[bm, :, g, :] alone, g the group of field f, and forward and backward are ONE pass, as in
        mse_loss and sensor_loss: the gradient of sum_f wsse[bm, f] is saved at forward and the backward scales it per member AND group.  An upstream
        gradient may therefore differ between members and between field groups, but must be the same for the fields of one group — a per-field factor
        inside a group cannot be folded into one saved gradient and belongs into field_precision; where the upstream does differ inside a group the
        gradient of that member's group slice is NaN (a select on the device, nothing is read back), never a silently wrong number.
        bf16 compute dtype, fused: the first-layer launch with the pre-activation kept, ONE fused launch (sea_decode_field_grad: score and
        pre-activation gradient; the weighted residual is rounded to bf16 once between the two products; neither the decoded fields nor their gradient
        are written) and its finish launch, the data-gradient launch against W1^T.  Under torch.no_grad(), or when z does not require grad, the
        score-only form of the same launch runs: the same bits, no second product.  fp32, or fused=False: forward() under autograd plus torch ops with
        the same selects (the composed path; it holds the [B * members, P, n_fields, n_inp] fields and their gradient).
        fused=None, read from profiles/field_grad_bench.txt (tools/field_grad_bench.py; cylinder and multiphase decoders, 64 members
        x 64 patches, n_inp 1628, one and four histories; every column valid, the mesh's counts, a 30 %-missing map with and without counts): the fused
        launch is the default exactly where it is ahead in every measured row —
          the score alone (no_grad, or z without grad): in bf16 from 4096 rows (B * members * P) on: 0.20 - 0.27 ms against 0.24 - 0.29 ms composed at 4096
          rows, 0.23 - 0.41 against 0.82 - 0.88 ms at 16384 (8 - 43 MB of extra memory against 307 - 1231 MB);
          with the gradient: in bf16 from 4096 rows on up to hidden width 512 (cylinder: 0.43 - 0.46 ms against 0.52 - 0.65 ms at 4096 rows, 0.67 - 0.71
          against 1.94 - 1.98 ms at 16384), and from 16384 rows on above it (multiphase: 0.87 - 0.91 against 1.96 - 2.01 ms; at 4096 rows the two are level,
          0.55 - 0.58 against 0.55 - 0.60 ms, the fused one behind in two of four rows: the composed path stays the default there; 23 - 117 MB against
          314 - 1266 MB) —
        and the composed path below 4096 rows, where nothing has been measured.  fused=True selects the leaner path at any size (bf16 only)."""
        what = "sea_amd.Decode.field_loss"
        n_fields = sum(len(g) for g in self.field_groups)
        C = self.n_inp
        if not torch.is_tensor(z) or z.dim() != 4 or z.shape[2] != self.num_groups or z.shape[3] != self.embed_dim:
            raise ValueError(f"{what}: z must be [B * members, P, {self.num_groups}, {self.embed_dim}], got {tuple(z.shape) if torch.is_tensor(z) else type(z).__name__}")
        Bm, P = z.shape[0], z.shape[1]
        if not isinstance(members, int) or isinstance(members, bool) or members < 1 or Bm < 1 or Bm % members:
            raise ValueError(f"{what}: members = {members!r} must be a positive integer that divides the {Bm} rows of z")
        B = Bm // members
        for name, t in (("obs", obs), ("precision", precision)):
            if t is None and name == "precision":
                continue
            if not torch.is_tensor(t) or t.dim() != 4 or tuple(t.shape[:3]) != (B, P, n_fields) or t.shape[3] < C:
                raise ValueError(f"{what}: {name} must be [{B}, {P}, {n_fields}, >= {C}] (one per history of {members} members), got "
                                 f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
            if t.dtype != torch.float32 or t.device != z.device:
                raise ValueError(f"{what}: {name} must be float32 on {z.device}, got {t.dtype} on {t.device}")
        if precision is not None and precision.shape[3] != obs.shape[3]:
            raise ValueError(f"{what}: precision must have obs's shape {tuple(obs.shape)}, got {tuple(precision.shape)}")
        if field_precision is not None and (not torch.is_tensor(field_precision) or field_precision.dtype != torch.float32 or tuple(field_precision.shape) != (n_fields,)
                                            or field_precision.device != z.device):
            raise ValueError(f"{what}: field_precision must be None or a float32 [{n_fields}] tensor on {z.device}")
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (obs, precision, field_precision)):
            raise ValueError(f"{what}: obs, precision and field_precision must not require grad (gradients flow to z only)")
        self._require_frozen("field_loss")
        dt = self._act_dtype()
        if fused is None:
            fused = self._field_loss_default(dt, Bm * P, z.requires_grad and torch.is_grad_enabled())
        if fused and dt != torch.bfloat16:
            raise ValueError(f"{what}: the fused launch is bf16 only (set_compute_dtype('bf16'), or fused=False)")
        cnt, _ = self._valid_counts(counts, P, z.device, allow_empty=True, what="field_loss")
        N.require_gpu(z, "Decode.field_loss input")
        obs = obs.detach()
        prec = None if precision is None else precision.detach()
        pf = None if field_precision is None else field_precision.detach().contiguous()
        want_grad = z.requires_grad and torch.is_grad_enabled()
        if fused:
            if want_grad:
                return _DecodeFieldFn.apply(z, self, obs, prec, pf, cnt, members)
            return self._field_grad_fused(z, obs, prec, pf, cnt, members, False)[0]
        zero = torch.zeros((), device=z.device)
        y = (_DecodeFn.apply(z, self) if want_grad else self.forward(z.detach())).view(B, members, P, n_fields, C)
        w = torch.ones(B, P, n_fields, C, device=z.device, dtype=torch.float32)
        live = torch.ones(B, P, n_fields, C, device=z.device, dtype=torch.bool)
        if pf is not None:
            w, live = w * pf.view(1, 1, n_fields, 1), live & (pf > 0).view(1, 1, n_fields, 1)
        if prec is not None:
            w, live = w * prec[..., :C], live & (prec[..., :C] > 0)
        if cnt is not None:
            live = live & (torch.arange(C, device=z.device) < cnt[:, None]).view(1, P, 1, C)
        w = torch.where(live, w, zero)                                            # NaN, negative values and Inf * 0 give no weight
        live = (w > 0).unsqueeze(1)
        d = torch.where(live, y - obs[..., :C].unsqueeze(1), zero)
        return (w.unsqueeze(1) * d * d).sum(dim=(2, 4)).view(Bm, n_fields)

    def _field_loss_default(self, dt: torch.dtype, rows: int, want_grad: bool) -> bool:
        """field_loss's fused=None rule, read from profiles/field_grad_bench.txt (tools/field_grad_bench.py): the fused launch is the
        default exactly where it is ahead in every measured row, and the composed path where it is not or where nothing was measured (below 4096 rows)."""
        if dt != torch.bfloat16 or rows < 4096:
            return False
        return not (want_grad and self.MLP_hidden > 512 and rows < 16384)

    def _field_grad_fused(self, z: torch.Tensor, obs: torch.Tensor, prec: Optional[torch.Tensor], pf: Optional[torch.Tensor], cnt, members: int, want_grad: bool):
        """The fused bf16 launches of field_loss on checked arguments, without autograd: (wsse [Bm, n_fields], dz f32 [Bm, P, G, D] or None)."""
        dt = torch.bfloat16
        with torch.no_grad():
            Bm, P, G, D = z.shape
            B, M, C = Bm // members, Bm * P, self.n_inp
            n_fields = sum(len(g) for g in self.field_groups)

            def rows(t):   # [B * P, n_fields, width]: a view where unit inner stride, strides that are multiples of 4 and a 16-byte base allow it, else None
                t3 = t.reshape(B * P, n_fields, t.shape[3])
                ok = t3.stride(2) == 1 and t3.stride(0) % 4 == 0 and t3.stride(1) % 4 == 0 and t3.stride(0) >= 0 and t3.stride(1) >= C and t3.data_ptr() % 16 == 0
                return t3 if ok else None

            def padded(t):   # one row-aligned copy of the first C columns (an odd cell width, or the reference's [.., C, n_fields] layout seen through a permute)
                out = torch.zeros(B * P, n_fields, (C + 3) // 4 * 4, device=t.device, dtype=torch.float32)
                out[..., :C] = t.reshape(B * P, n_fields, t.shape[3])[..., :C]
                return out

            o3 = rows(obs)
            p3 = None if prec is None else rows(prec)
            if o3 is None or (prec is not None and (p3 is None or p3.stride() != o3.stride())):   # the map is addressed through the observation's strides
                o3, p3 = padded(obs), None if prec is None else padded(prec)
            _, W2 = self._weights(dt)
            if want_grad:
                hid, pre = self._first_layer(z, dt)
                bias = self._shadow[3]
                dpre = [torch.empty(M, self.MLP_hidden, device=z.device, dtype=dt) for _ in range(G)]
                groups = [dict(H=hid[g], W2=W2[g], bias=bias[g], dH=dpre[g], Z=pre[g]) for g in range(G)]
            else:
                zf = z.detach().to(torch.float32).contiguous().view(M, G * D)
                za = torch.empty(M, G * D, device=z.device, dtype=dt)
                ops.convert(zf, za)
                W1, _ = self._weights(dt)
                hid = [torch.empty(M, self.MLP_hidden, device=z.device, dtype=dt) for _ in range(G)]
                ops.gemm_grouped([dict(A=za[:, g * D:(g + 1) * D], W=W1[g], Cact=hid[g], act=1) for g in range(G)], dt)
                bias = self._shadow[3]
                groups = [dict(H=hid[g], W2=W2[g], bias=bias[g]) for g in range(G)]
            wsse = ops.decode_field_grad(groups, o3, C, self._n_inp_p, P, members=members, prec=p3, field_prec=pf, counts=cnt, dtype=dt)
            dz = self._input_grad(dpre, dt).view(Bm, P, G, D) if want_grad else None
            return wsse, dz

    def member_moments(self, z: torch.Tensor, members: int, weights: Optional[torch.Tensor] = None, counts=None, unbiased: bool = False,
                       fused: Optional[bool] = None):
        """The forecast of an ensemble: (mean, var) of the decoded fields over the `members` members of every history, each fp32 [B, P, n_fields, n_inp]
        (a view of an n_inp_p-wide buffer, like forward()'s result: sea_unpatchify reads it in place); no autograd graph.  z [B * members, P, n_groups,
        embed_dim] in fork() order (row b * members + j is member j of history b); weights: None (1 / members) or float32 [B * members] on z's device,
        normalised per history (EnsembleFields builds them from log-weights); a member with weight 0 is dead: it is passed over, NaN in its latents
        reaches nothing.  mean = sum_j w_j y_j, var = sum_j w_j (y_j - mean)^2, centred; unbiased=True multiplies var by 1 / (1 - sum_j w_j^2)
        (members / (members - 1) for equal weights), computed with tensor ops; a history whose weight sits on one member gets variance 0, not Inf.
        counts as in mse_loss (None, or valid cells per patch; all-zero counts are accepted): invalid cells and the pad columns are exactly 0 in both.
        bf16 compute dtype: the first-layer launch plus ONE fused launch (sea_decode_member_moments) — the members' decoded fields are never written;
        fp32, or fused=False: forward() plus torch reductions (mean, then centred squares; the composed path).  `fused` forces either path; None:
        fused in bf16 from 4096 rows (B * members * P) on, composed below — measured (tools/ensemble_bench.py --moments,
        profiles/ensemble_moments_bench.txt; 64 members x 64 patches, n_inp 1628): at 4096 rows, the smallest size measured,
        the fused path is ahead at both decoders (cylinder 0.21 against 0.29 - 0.31 ms; multiphase 0.30 against 0.30 - 0.32 ms: level with every
        column valid, 8 % ahead with the mesh's counts), at 16384 rows 2.5 - 5.0x faster, and it needs 10 - 53 MB of extra memory against 307 -
        1229 MB.  Below 4096 rows nothing has been measured, so the composed path stays the default there."""
        n_fields = sum(len(g) for g in self.field_groups)
        C, Cp = self.n_inp, self._n_inp_p
        if z.dim() != 4 or z.shape[2] != self.num_groups or z.shape[3] != self.embed_dim:
            raise ValueError(f"sea_amd.Decode.member_moments: z must be [B * members, P, {self.num_groups}, {self.embed_dim}], got {tuple(z.shape)}")
        Bm, P = z.shape[0], z.shape[1]
        if not isinstance(members, int) or isinstance(members, bool) or members < 1 or Bm < 1 or Bm % members:
            raise ValueError(f"sea_amd.Decode.member_moments: members = {members!r} must be a positive integer that divides the {Bm} rows of z")
        B = Bm // members
        if weights is not None:
            if not torch.is_tensor(weights) or weights.dim() != 1 or weights.shape[0] != Bm:
                raise ValueError(f"sea_amd.Decode.member_moments: weights must be None or a [{Bm}] tensor (one weight per member), got "
                                 f"{tuple(weights.shape) if torch.is_tensor(weights) else type(weights).__name__}")
            if weights.dtype != torch.float32 or weights.device != z.device:
                raise ValueError(f"sea_amd.Decode.member_moments: weights must be float32 on {z.device}, got {weights.dtype} on {weights.device}")
        dt = self._act_dtype()
        if fused is None:
            fused = dt == torch.bfloat16 and Bm * P >= 4096
        if fused and dt != torch.bfloat16:
            raise ValueError("sea_amd.Decode.member_moments: the fused launch is bf16 only (set_compute_dtype('bf16'), or fused=False)")
        cnt, _ = self._valid_counts(counts, P, z.device, allow_empty=True, what="member_moments")
        N.require_gpu(z, "Decode.member_moments input")
        with torch.no_grad():
            w = None if weights is None else weights.detach().contiguous()
            scale = None
            if unbiased:
                s2 = torch.full((B,), 1.0 / members, device=z.device, dtype=torch.float32) if w is None else (w.view(B, members) ** 2).sum(1)
                den = 1.0 - s2
                scale = torch.where(den > 0, 1.0 / den.clamp_min(torch.finfo(torch.float32).tiny), torch.zeros_like(den)).contiguous()
            if not fused:
                y = self.forward(z.detach()).view(B, members, P, n_fields, C)
                wb = (torch.full((B, members), 1.0 / members, device=z.device, dtype=torch.float32) if w is None else w.view(B, members)).view(B, members, 1, 1, 1)
                live = wb > 0
                zero = torch.zeros((), device=z.device)
                W = torch.where(live, wb, zero).sum(1)
                mean = (wb * torch.where(live, y, zero)).sum(1) / W.clamp_min(torch.finfo(torch.float32).tiny)
                d = torch.where(live, y - mean.unsqueeze(1), zero)
                var = (wb * d * d).sum(1)
                if scale is not None:
                    var = var * scale.view(B, 1, 1, 1)
                if cnt is not None:
                    valid = (torch.arange(C, device=z.device) < cnt[:, None]).view(1, P, 1, C)
                    mean, var = torch.where(valid, mean, zero), torch.where(valid, var, zero)
                out = torch.zeros(2, B, P, n_fields, Cp, device=z.device, dtype=torch.float32)
                out[0, ..., :C], out[1, ..., :C] = mean, var
                return (out[0], out[1]) if Cp == C else (out[0, ..., :C], out[1, ..., :C])
            M = Bm * P
            G, D = self.num_groups, self.embed_dim
            zf = z.detach().to(torch.float32).contiguous().view(M, G * D)
            za = torch.empty(M, G * D, device=z.device, dtype=dt)
            ops.convert(zf, za)
            W1, W2 = self._weights(dt)
            hid = [torch.empty(M, self.MLP_hidden, device=z.device, dtype=dt) for _ in range(G)]
            ops.gemm_grouped([dict(A=za[:, g * D:(g + 1) * D], W=W1[g], Cact=hid[g], act=1) for g in range(G)], dt)
            bias = self._shadow[3]
            mean, var = ops.decode_member_moments([dict(H=hid[g], W2=W2[g], bias=bias[g]) for g in range(G)], C, Cp, P, members=members, weights=w,
                                                  var_scale=scale, counts=cnt, ld=Cp, dtype=dt)
            mean, var = mean.view(B, P, n_fields, Cp), var.view(B, P, n_fields, Cp)
            return (mean, var) if Cp == C else (mean[..., :C], var[..., :C])

    def member_gram(self, z: torch.Tensor, obs: torch.Tensor, members: int, counts=None, precision: Optional[torch.Tensor] = None,
                    field_precision: Optional[torch.Tensor] = None, fused: Optional[bool] = None):
        """What an ensemble Kalman analysis needs from a DENSE observation of the decoded fields: (gram, proj, count) per (history, patch) —
        gram float64 [B, P, members, members] = sum over the live cells of w a_i a_j with a_j = y_j - mean_j y_j the decoded anomaly of member j, proj
        float64 [B, P, members] = sum w a_j (obs - mean_j y_j), count int32 [B, P] the live cells, or -1 where obs or a member's value at a live
        cell, or a sum, is not finite (include/sea_hip.h, sea_decode_member_gram, states the formulas); no autograd graph.  z [B * members, P,
        n_groups, embed_dim] in fork() order; obs float32 [B, P, n_fields, C >= n_inp] on z's device, one snapshot per history; counts as in
        mse_loss (all-zero counts are accepted); precision: None or a float32 map of obs's shape, >= 0, 0 marks a missing cell; field_precision: None
        or float32 [n_fields] on z's device.  The weight of a cell is w = valid ? max(field_precision, 0) * max(precision, 0) : 0, by selects: a
        cell without weight is neutral whatever obs and precision hold there, NaN included.  2 <= members <= 128.
        bf16 compute dtype: the first-layer launch plus ONE fused launch (sea_decode_member_gram) — neither the members' decoded fields nor a
        [B * members, cells] prediction matrix are ever written; fp32, or fused=False: forward() plus float64 torch ops with the same selects (the
        composed path: it holds the members' fields in float64).  fused=None: the fused launch in bf16 from 4096 rows (B * members * P) on — measured
        at 4096 and 16384 rows (tools/field_enkf_bench.py, profiles/field_enkf_bench.txt, DESIGN.md section 7j: 0.64 - 0.72 ms for this call; the
        composed analysis it replaces takes 1.4 - 4.3 ms) — and the composed path below, where nothing has been measured."""
        what = "sea_amd.Decode.member_gram"
        n_fields = sum(len(g) for g in self.field_groups)
        C, Cp = self.n_inp, self._n_inp_p
        if not torch.is_tensor(z) or z.dim() != 4 or z.shape[2] != self.num_groups or z.shape[3] != self.embed_dim:
            raise ValueError(f"{what}: z must be [B * members, P, {self.num_groups}, {self.embed_dim}], got {tuple(z.shape) if torch.is_tensor(z) else type(z).__name__}")
        Bm, P = z.shape[0], z.shape[1]
        if not isinstance(members, int) or isinstance(members, bool) or members < 2 or members > N.ENKF_MAX_N or Bm < 1 or Bm % members:
            raise ValueError(f"{what}: members = {members!r} must be an integer in 2 .. {N.ENKF_MAX_N} that divides the {Bm} rows of z")
        B = Bm // members
        for name, t in (("obs", obs), ("precision", precision)):
            if t is None and name == "precision":
                continue
            if not torch.is_tensor(t) or t.dim() != 4 or tuple(t.shape[:3]) != (B, P, n_fields) or t.shape[3] < C:
                raise ValueError(f"{what}: {name} must be [{B}, {P}, {n_fields}, >= {C}] (one per history of {members} members), got "
                                 f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
            if t.dtype != torch.float32 or t.device != z.device:
                raise ValueError(f"{what}: {name} must be float32 on {z.device}, got {t.dtype} on {t.device}")
        if precision is not None and precision.shape[3] != obs.shape[3]:
            raise ValueError(f"{what}: precision must have obs's shape {tuple(obs.shape)}, got {tuple(precision.shape)}")
        if field_precision is not None and (not torch.is_tensor(field_precision) or field_precision.dtype != torch.float32 or tuple(field_precision.shape) != (n_fields,)
                                            or field_precision.device != z.device):
            raise ValueError(f"{what}: field_precision must be None or a float32 [{n_fields}] tensor on {z.device}")
        dt = self._act_dtype()
        if fused is None:
            fused = dt == torch.bfloat16 and Bm * P >= 4096
        if fused and dt != torch.bfloat16:
            raise ValueError(f"{what}: the fused launch is bf16 only (set_compute_dtype('bf16'), or fused=False)")
        cnt, _ = self._valid_counts(counts, P, z.device, allow_empty=True, what="member_gram")
        N.require_gpu(z, "Decode.member_gram input")
        with torch.no_grad():
            obs = obs.detach()
            prec = None if precision is None else precision.detach()
            pf = None if field_precision is None else field_precision.detach().contiguous()
            if not fused:
                f64 = torch.float64
                zero = torch.zeros((), device=z.device, dtype=f64)
                y = self.forward(z.detach()).view(B, members, P, n_fields, C).to(f64)
                w = torch.ones(B, P, n_fields, C, device=z.device, dtype=f64)
                if pf is not None:
                    pf64 = pf.to(f64).view(1, 1, n_fields, 1)
                    w = w * torch.where(pf64 > 0, pf64, zero)
                if prec is not None:
                    pm = prec[..., :C].to(f64)
                    w = w * torch.where(pm > 0, pm, zero)
                if cnt is not None:
                    w = torch.where((torch.arange(C, device=z.device) < cnt[:, None]).view(1, P, 1, C), w, zero)
                live = w > 0                                                         # false for NaN
                sw = torch.where(live, w, zero).sqrt()
                ybar = y.mean(dim=1)                                                 # [B, P, F, C]
                X = torch.where(live.unsqueeze(1), (y - ybar.unsqueeze(1)) * sw.unsqueeze(1), zero)          # [B, n, P, F, C]
                e = torch.where(live, sw * (obs[..., :C].to(f64) - ybar), zero)
                Xp = X.permute(0, 2, 1, 3, 4).reshape(B, P, members, n_fields * C)
                gram = Xp @ Xp.transpose(-1, -2)
                gram = 0.5 * (gram + gram.transpose(-1, -2))
                proj = (Xp @ e.reshape(B, P, n_fields * C, 1)).squeeze(-1)
                count = live.sum(dim=(2, 3)).to(torch.int32)
                bad = ~(torch.isfinite(X).all(-1).all(-1).all(1) & torch.isfinite(e).all(-1).all(-1)) \
                    | ~(torch.isfinite(gram).all(-1).all(-1) & torch.isfinite(proj).all(-1))
                return gram.contiguous(), proj.contiguous(), torch.where(bad, torch.full_like(count, -1), count)

            def rows(t):   # [B * P, n_fields, width] with unit inner stride: a view where the layout allows it, else one copy of the first C columns
                t3 = t.reshape(B * P, n_fields, t.shape[3])
                return t3 if t3.stride(2) == 1 and t3.stride(1) >= C and t3.stride(0) >= 0 else t3[..., :C].contiguous()

            M = Bm * P
            G, D = self.num_groups, self.embed_dim
            zf = z.detach().to(torch.float32).contiguous().view(M, G * D)
            za = torch.empty(M, G * D, device=z.device, dtype=dt)
            ops.convert(zf, za)
            W1, W2 = self._weights(dt)
            hid = [torch.empty(M, self.MLP_hidden, device=z.device, dtype=dt) for _ in range(G)]
            ops.gemm_grouped([dict(A=za[:, g * D:(g + 1) * D], W=W1[g], Cact=hid[g], act=1) for g in range(G)], dt)
            bias = self._shadow[3]
            return ops.decode_member_gram([dict(H=hid[g], W2=W2[g], bias=bias[g]) for g in range(G)], rows(obs), C, Cp, P, members, prec_field=pf,
                                          prec=None if prec is None else rows(prec), counts=cnt, dtype=dt)

    def member_verify(self, z: torch.Tensor, obs: torch.Tensor, members: int, counts=None, precision: Optional[torch.Tensor] = None,
                      field_precision: Optional[torch.Tensor] = None, logw: Optional[torch.Tensor] = None, unbiased: bool = True,
                      fused: Optional[bool] = None, maps=("mean", "spread", "crps", "pit", "rank"), into: Optional[dict] = None):
        """The verification of an ensemble against a DENSE observation of the decoded fields: a dict with the maps asked for — mean, spread, crps, pit
        float32 and rank int32 [B, P, n_fields, n_inp] — and sums float64 [B, n_fields, 8], hist int64 [B, n_fields, members + 1], status int32 [B]
        (include/sea_hip.h, sea_decode_member_verify, states the formulas: sea_ensemble_verify's with every cell a reading); no autograd graph.  z, obs,
        counts, precision and field_precision as in member_gram: the weight of a cell is w = valid ? max(field_precision, 0) * max(precision, 0) : 0
        by selects (an fp32 product), and 1 / w is its observation-error variance.  logw: None or float32 [B * members] on z's device.  into: a dict
        with earlier "sums" and "hist" tensors that this call's are added onto in place (they are the result's).
        fused=True (bf16 compute dtype, members <= 128): the first-layer launch plus the TWO launches of sea_decode_member_verify — the members'
        decoded fields are never written.  fused=False: forward() plus the formulas as float64 torch ops with every cell a sensor (the composed path:
        fp32, any member count, comparison).  fused=None: the fused launches in bf16 up to 128 members from 4096 rows (B * members * P) on — every row
        of profiles/field_verify_bench.txt (tools/field_verify_bench.py, DESIGN.md section 7k: 0.62 - 7.0 ms against 6.3 - 37.8 ms composed at 4096 -
        32768 rows) — and the composed path elsewhere: below 4096 rows, where nothing was measured, in fp32 and above 128 members."""
        from ..ensemble import FIELD_MAPS, FIELD_VERIFY_FUSED_MIN_ROWS, _composed_field_verify, _field_cell_weights

        what = "sea_amd.Decode.member_verify"
        n_fields = sum(len(g) for g in self.field_groups)
        C, Cp = self.n_inp, self._n_inp_p
        if not torch.is_tensor(z) or z.dim() != 4 or z.shape[2] != self.num_groups or z.shape[3] != self.embed_dim:
            raise ValueError(f"{what}: z must be [B * members, P, {self.num_groups}, {self.embed_dim}], got {tuple(z.shape) if torch.is_tensor(z) else type(z).__name__}")
        Bm, P = z.shape[0], z.shape[1]
        if not isinstance(members, int) or isinstance(members, bool) or members < 1 or Bm < 1 or Bm % members:
            raise ValueError(f"{what}: members = {members!r} must be a positive integer that divides the {Bm} rows of z")
        B = Bm // members
        for name, t in (("obs", obs), ("precision", precision)):
            if t is None and name == "precision":
                continue
            if not torch.is_tensor(t) or t.dim() != 4 or tuple(t.shape[:3]) != (B, P, n_fields) or t.shape[3] < C:
                raise ValueError(f"{what}: {name} must be [{B}, {P}, {n_fields}, >= {C}] (one per history of {members} members), got "
                                 f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
            if t.dtype != torch.float32 or t.device != z.device:
                raise ValueError(f"{what}: {name} must be float32 on {z.device}, got {t.dtype} on {t.device}")
        if precision is not None and precision.shape[3] != obs.shape[3]:
            raise ValueError(f"{what}: precision must have obs's shape {tuple(obs.shape)}, got {tuple(precision.shape)}")
        if field_precision is not None and (not torch.is_tensor(field_precision) or field_precision.dtype != torch.float32 or tuple(field_precision.shape) != (n_fields,)
                                            or field_precision.device != z.device):
            raise ValueError(f"{what}: field_precision must be None or a float32 [{n_fields}] tensor on {z.device}")
        if logw is not None and (not torch.is_tensor(logw) or logw.dtype != torch.float32 or tuple(logw.shape) != (Bm,) or logw.device != z.device):
            raise ValueError(f"{what}: logw must be None or a float32 [{Bm}] tensor on {z.device}")
        maps = tuple(maps)
        if any(k not in FIELD_MAPS for k in maps) or len(set(maps)) != len(maps):
            raise ValueError(f"{what}: maps must be distinct names among {FIELD_MAPS}, got {maps!r}")
        if into is not None and (not isinstance(into, dict) or set(into) != {"sums", "hist"} or any(
                not torch.is_tensor(t) or tuple(t.shape) != sh or t.dtype != dt_ or t.device != z.device or not t.is_contiguous()
                for t, sh, dt_ in ((into.get("sums"), (B, n_fields, N.VERIFY_SUMS), torch.float64), (into.get("hist"), (B, n_fields, members + 1), torch.int64)))):
            raise ValueError(f"{what}: into must be a dict of contiguous sums float64 [{B}, {n_fields}, {N.VERIFY_SUMS}] and hist int64 [{B}, {n_fields}, "
                             f"{members + 1}] on {z.device}")
        dt = self._act_dtype()
        if fused is None:
            fused = dt == torch.bfloat16 and members <= N.FIELD_VERIFY_MAX_N and Bm * P >= FIELD_VERIFY_FUSED_MIN_ROWS
        if fused and dt != torch.bfloat16:
            raise ValueError(f"{what}: the fused launches are bf16 only (set_compute_dtype('bf16'), or fused=False)")
        if fused and members > N.FIELD_VERIFY_MAX_N:
            raise ValueError(f"{what}: the fused launches carry up to {N.FIELD_VERIFY_MAX_N} members, got {members} (fused=False, or None)")
        cnt, _ = self._valid_counts(counts, P, z.device, allow_empty=True, what="member_verify")
        N.require_gpu(z, "Decode.member_verify input")
        with torch.no_grad():
            obs = obs.detach()
            prec = None if precision is None else precision.detach()
            pf = None if field_precision is None else field_precision.detach().contiguous()
            lw = None if logw is None else logw.detach().contiguous()
            if not fused:
                y = self.forward(z.detach()).view(Bm, P, n_fields, C)
                w = _field_cell_weights((B, P, n_fields, C), pf, prec, cnt, z.device)
                r = _composed_field_verify(y, obs, w, lw, members, bool(unbiased), maps=maps)
                if into is not None:
                    r["sums"], r["hist"] = into["sums"].add_(r["sums"]), into["hist"].add_(r["hist"])
                return r

            def rows(t):   # [B * P, n_fields, width] with unit inner stride: a view where the layout allows it, else one copy of the first C columns
                t3 = t.reshape(B * P, n_fields, t.shape[3])
                return t3 if t3.stride(2) == 1 and t3.stride(1) >= C and t3.stride(0) >= 0 else t3[..., :C].contiguous()

            M = Bm * P
            G, D = self.num_groups, self.embed_dim
            zf = z.detach().to(torch.float32).contiguous().view(M, G * D)
            za = torch.empty(M, G * D, device=z.device, dtype=dt)
            ops.convert(zf, za)
            W1, W2 = self._weights(dt)
            hid = [torch.empty(M, self.MLP_hidden, device=z.device, dtype=dt) for _ in range(G)]
            ops.gemm_grouped([dict(A=za[:, g * D:(g + 1) * D], W=W1[g], Cact=hid[g], act=1) for g in range(G)], dt)
            bias = self._shadow[3]
            return ops.decode_member_verify([dict(H=hid[g], W2=W2[g], bias=bias[g]) for g in range(G)], rows(obs), C, Cp, P, members, prec_field=pf,
                                            prec=None if prec is None else rows(prec), counts=cnt, logw=lw, unbiased=bool(unbiased),
                                            accumulate=into is not None, maps=maps, out=into, dtype=dt)

    def member_brier(self, z: torch.Tensor, obs: torch.Tensor, members: int, thresholds: torch.Tensor, counts=None, precision: Optional[torch.Tensor] = None,
                     field_precision: Optional[torch.Tensor] = None, logw: Optional[torch.Tensor] = None, fused: Optional[bool] = None, maps=(),
                     into: Optional[dict] = None):
        """The threshold scores of an ensemble against a DENSE observation of the decoded fields: a dict with the maps asked for — prob, brier float32
        [T, B, P, n_fields, n_inp] — and sums float64 [B, n_fields, T, 5], hist and hits int64 [B, n_fields, T, members + 1], status int32 [B]
        (include/sea_hip.h, sea_decode_member_brier, states the definitions); no autograd graph.  z, obs, counts, precision, field_precision and logw as
        in member_verify (the weight of a cell only decides whether it is read); thresholds: float32 [T <= 8, n_fields] on z's device, in the decoder's
        scaled units (a host tensor is checked for finite values; the classes of sea_amd.ensemble check theirs at construction).  into: a dict with
        earlier "sums", "hist" and "hits" tensors that this call's are added onto in place (they are the result's).
        fused=True (bf16 compute dtype, members <= 128): the first-layer launch plus the TWO launches of sea_decode_member_brier — the members' decoded
        fields are never written.  fused=False: forward() plus the formulas as float64 torch ops (ensemble._composed_field_brier: fp32, any member
        count, comparison).  fused=None: the fused launches in bf16 up to 128 members from 4096 rows (B * members * P) on — every row of
        profiles/brier_bench.txt (tools/brier_bench.py) — and the composed path elsewhere: below 4096 rows, where nothing was
        measured, in fp32 and above 128 members."""
        from ..ensemble import BRIER_FUSED_MIN_ROWS, BRIER_MAPS, _composed_field_brier, _field_cell_weights

        what = "sea_amd.Decode.member_brier"
        n_fields = sum(len(g) for g in self.field_groups)
        C, Cp = self.n_inp, self._n_inp_p
        if not torch.is_tensor(z) or z.dim() != 4 or z.shape[2] != self.num_groups or z.shape[3] != self.embed_dim:
            raise ValueError(f"{what}: z must be [B * members, P, {self.num_groups}, {self.embed_dim}], got {tuple(z.shape) if torch.is_tensor(z) else type(z).__name__}")
        Bm, P = z.shape[0], z.shape[1]
        if not isinstance(members, int) or isinstance(members, bool) or members < 1 or Bm < 1 or Bm % members:
            raise ValueError(f"{what}: members = {members!r} must be a positive integer that divides the {Bm} rows of z")
        B = Bm // members
        for name, t in (("obs", obs), ("precision", precision)):
            if t is None and name == "precision":
                continue
            if not torch.is_tensor(t) or t.dim() != 4 or tuple(t.shape[:3]) != (B, P, n_fields) or t.shape[3] < C:
                raise ValueError(f"{what}: {name} must be [{B}, {P}, {n_fields}, >= {C}] (one per history of {members} members), got "
                                 f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
            if t.dtype != torch.float32 or t.device != z.device:
                raise ValueError(f"{what}: {name} must be float32 on {z.device}, got {t.dtype} on {t.device}")
        if precision is not None and precision.shape[3] != obs.shape[3]:
            raise ValueError(f"{what}: precision must have obs's shape {tuple(obs.shape)}, got {tuple(precision.shape)}")
        if field_precision is not None and (not torch.is_tensor(field_precision) or field_precision.dtype != torch.float32 or tuple(field_precision.shape) != (n_fields,)
                                            or field_precision.device != z.device):
            raise ValueError(f"{what}: field_precision must be None or a float32 [{n_fields}] tensor on {z.device}")
        if logw is not None and (not torch.is_tensor(logw) or logw.dtype != torch.float32 or tuple(logw.shape) != (Bm,) or logw.device != z.device):
            raise ValueError(f"{what}: logw must be None or a float32 [{Bm}] tensor on {z.device}")
        thr = thresholds.detach().contiguous() if torch.is_tensor(thresholds) else thresholds
        ops.check_brier_thresholds(thr, n_fields, z.device, what)
        T = thr.shape[0]
        maps = tuple(maps)
        if any(k not in BRIER_MAPS for k in maps) or len(set(maps)) != len(maps):
            raise ValueError(f"{what}: maps must be distinct names among {BRIER_MAPS}, got {maps!r}")
        shapes = (("sums", (B, n_fields, T, N.BRIER_SUMS), torch.float64), ("hist", (B, n_fields, T, members + 1), torch.int64),
                  ("hits", (B, n_fields, T, members + 1), torch.int64))
        if into is not None and (not isinstance(into, dict) or set(into) != {"sums", "hist", "hits"} or any(
                not torch.is_tensor(into[k]) or tuple(into[k].shape) != sh or into[k].dtype != dt_ or into[k].device != z.device or not into[k].is_contiguous()
                for k, sh, dt_ in shapes)):
            raise ValueError(f"{what}: into must be a dict of contiguous sums float64 [{B}, {n_fields}, {T}, {N.BRIER_SUMS}], hist and hits int64 [{B}, {n_fields}, "
                             f"{T}, {members + 1}] on {z.device}")
        dt = self._act_dtype()
        if fused is None:
            fused = dt == torch.bfloat16 and members <= N.BRIER_MAX_N and Bm * P >= BRIER_FUSED_MIN_ROWS
        if fused and dt != torch.bfloat16:
            raise ValueError(f"{what}: the fused launches are bf16 only (set_compute_dtype('bf16'), or fused=False)")
        if fused and members > N.BRIER_MAX_N:
            raise ValueError(f"{what}: the fused launches carry up to {N.BRIER_MAX_N} members, got {members} (fused=False, or None)")
        cnt, _ = self._valid_counts(counts, P, z.device, allow_empty=True, what="member_brier")
        N.require_gpu(z, "Decode.member_brier input")
        with torch.no_grad():
            obs = obs.detach()
            prec = None if precision is None else precision.detach()
            pf = None if field_precision is None else field_precision.detach().contiguous()
            lw = None if logw is None else logw.detach().contiguous()
            if not fused:
                y = self.forward(z.detach()).view(Bm, P, n_fields, C)
                w = _field_cell_weights((B, P, n_fields, C), pf, prec, cnt, z.device)
                r = _composed_field_brier(y, obs, w, lw, members, thr, maps=maps)
                if into is not None:
                    r["sums"], r["hist"], r["hits"] = into["sums"].add_(r["sums"]), into["hist"].add_(r["hist"]), into["hits"].add_(r["hits"])
                return r

            def rows(t):   # [B * P, n_fields, width] with unit inner stride: a view where the layout allows it, else one copy of the first C columns
                t3 = t.reshape(B * P, n_fields, t.shape[3])
                return t3 if t3.stride(2) == 1 and t3.stride(1) >= C and t3.stride(0) >= 0 else t3[..., :C].contiguous()

            M = Bm * P
            G, D = self.num_groups, self.embed_dim
            zf = z.detach().to(torch.float32).contiguous().view(M, G * D)
            za = torch.empty(M, G * D, device=z.device, dtype=dt)
            ops.convert(zf, za)
            W1, W2 = self._weights(dt)
            hid = [torch.empty(M, self.MLP_hidden, device=z.device, dtype=dt) for _ in range(G)]
            ops.gemm_grouped([dict(A=za[:, g * D:(g + 1) * D], W=W1[g], Cact=hid[g], act=1) for g in range(G)], dt)
            bias = self._shadow[3]
            return ops.decode_member_brier([dict(H=hid[g], W2=W2[g], bias=bias[g]) for g in range(G)], rows(obs), C, Cp, P, members, thr, prec_field=pf,
                                           prec=None if prec is None else rows(prec), counts=cnt, logw=lw, accumulate=into is not None, maps=maps, out=into,
                                           dtype=dt)

    def _field_weight_on(self, field_weight, n_fields: int, device: torch.device, what: str):
        """field_weight checked on the host (float32 [n_fields], finite, >= 0; cached per tensor object and version) -> a contiguous copy on `device`, or None.
        A tensor that EnsembleCRPSLoss made from values it checked at construction carries a mark and is taken as it is: nothing is read back from the device."""
        if field_weight is None:
            return None
        if not torch.is_tensor(field_weight) or field_weight.dtype != torch.float32 or tuple(field_weight.shape) != (n_fields,):
            raise ValueError(f"{what}: field_weight must be None or a float32 [{n_fields}] tensor, got "
                             f"{(tuple(field_weight.shape), field_weight.dtype) if torch.is_tensor(field_weight) else type(field_weight).__name__}")
        if field_weight.requires_grad and torch.is_grad_enabled():
            raise ValueError(f"{what}: field_weight must not require grad (gradients flow to z only)")
        if getattr(field_weight, "_sea_checked_field_weight", False):
            return field_weight.detach().to(device).contiguous()
        key = (id(field_weight), field_weight._version, device)
        cur = getattr(self, "_fw_cache", None)
        if cur is None or cur[0] != key:
            host = field_weight.detach().cpu()
            if not bool(torch.isfinite(host).all()) or bool((host < 0).any()):
                raise ValueError(f"{what}: field_weight must be finite and >= 0, got {host.tolist()}")
            cur = (key, field_weight.detach().to(device).contiguous(), field_weight)   # the object is kept so that its id is not reused
            self._fw_cache = cur
        return cur[1]

    def member_crps_loss(self, z: torch.Tensor, obs: torch.Tensor, members: int, counts=None, precision: Optional[torch.Tensor] = None,
                         field_precision: Optional[torch.Tensor] = None, field_weight: Optional[torch.Tensor] = None, logw: Optional[torch.Tensor] = None,
                         unbiased: bool = True, fused: Optional[bool] = None, pack: Optional[bool] = None):
        """The CRPS of an ensemble's DECODED fields against a dense observation as a loss: (loss, count) with loss float32 [B, n_fields],
        loss[b, f] = field_weight[f] * sum over the patches and the live, good cells of field f of the cell's CRPS (member_verify's sums[..., 1]:
        the fair CRPS with unbiased=True), differentiable with a gradient to z only, and count float64 [B, n_fields] the number of those cells
        (sums[..., 0]; not differentiable).  z, obs, members, counts, precision, field_precision, logw, unbiased and their validation are
        member_verify's (logw is a constant: no gradient reaches it); field_weight: None or float32 [n_fields], finite and >= 0.  The derivative of a
        cell's CRPS with respect to member m's value is w_m (sign(x_m - y) - (2 below_m + w_m - 1) / c) (include/sea_hip.h,
        sea_decode_member_crps_grad): the derivative away from ties, at ties the subgradient that the order (value, member index) selects; exactly 0
        for a dead member, a dead or bad cell and a history that is not scored.
        Upstream gradients.  loss[b, f] depends on the z rows of history b's members in the group g of field f alone, and forward and backward are ONE
        pass, as in field_loss: the gradient of sum_f loss[b, f] is saved at forward and the backward scales it per HISTORY and field GROUP.  Where the
        upstream gradient differs between the fields of one group that history's group slice is NaN (a select on the device), never a silently wrong
        number; per-field factors belong in field_weight.  (The composed path carries per-field upstream gradients exactly.)
        fused=True (bf16; members <= 64, or <= 128 at MLP_hidden <= 384): the first-layer launch with the pre-activation kept, the TWO launches of
        sea_decode_member_crps_grad (member_verify's grid and walk; the scoring lanes hand the derivative to a second MFMA product against the same
        LDS image of the W2 tile; neither the members' decoded fields nor their gradient are written) and the data-gradient launch against W1^T.
        Under torch.no_grad(), or when z does not require grad, it is member_verify without maps: the same loss bits.  fused=False: forward() under
        autograd plus the formulas as float64 torch ops with the gradient coded explicitly in the (value, index) tie order (the composed path: fp32,
        any member count; it holds the [B * members, P, n_fields, n_inp] fields and their gradient).
        fused=None, read from profiles/crps_loss_bench.txt (tools/crps_loss_bench.py; cylinder and multiphase decoders, 64 patches,
        n_inp 1628, the mesh's counts, loss + backward): the fused launches in bf16, where the fused form carries the shape, up to 64 members from 4096
        rows (B * members * P) on, and up to 8 members from 16384 rows on — the smallest measured sizes of the two regimes; the fused path is ahead in
        every measured row of both: 64 members x 1 and 4 histories 1.13 - 3.48 ms against 6.0 - 22.9 ms composed (112 - 584 MB of extra
        memory against 1.9 - 7.8 GB); 4 and 8 members x 64 and 256 histories 23.9 - 104.7 ms against 104.9 - 457.3 ms (0.46 - 4.7 GB against
        8.6 - 65.5 GB).  Member counts between 8 and 64 were not measured: the rule INTERPOLATES between the two regimes there (both ends are ahead by
        4x or more).  The composed path serves elsewhere: below those row counts and above 64 members, where nothing was measured (the bench's
        128-member shapes have hidden widths the fused form refuses), in fp32, and for any shape the fused form refuses (MLP_hidden above 640
        included) — such a shape raises only under fused=True.
        pack (the fused path with a gradient only; under no_grad the path is member_verify whatever pack says): True takes
        sea_decode_member_crps_grad_packed — several histories per workgroup for 1 .. 32 members, every output with the bits of pack=False — and
        raises ValueError for a shape that form refuses (above 32 members) and with fused=False; with fused=None it selects the fused launches, as
        fused=True does.  False is the unpacked form.  None is crps_loss_pack_rule(members, rows, MLP_hidden, dtype), read from
        profiles/crps_pack_bench.txt: the packed form at 2 .. 32 members from 4096 (history, patch) pairs on — ahead in every
        measured row, 2.05x (32 members) to 15 - 16x (4 members) and 17 - 30x (2 members) — and the unpacked form elsewhere, tiny shapes included."""
        from ..ensemble import _CrpsComposedFn, _field_cell_weights

        what = "sea_amd.Decode.member_crps_loss"
        n_fields = sum(len(g) for g in self.field_groups)
        C, Cp = self.n_inp, self._n_inp_p
        if not torch.is_tensor(z) or z.dim() != 4 or z.shape[2] != self.num_groups or z.shape[3] != self.embed_dim:
            raise ValueError(f"{what}: z must be [B * members, P, {self.num_groups}, {self.embed_dim}], got {tuple(z.shape) if torch.is_tensor(z) else type(z).__name__}")
        Bm, P = z.shape[0], z.shape[1]
        if not isinstance(members, int) or isinstance(members, bool) or members < 1 or Bm < 1 or Bm % members:
            raise ValueError(f"{what}: members = {members!r} must be a positive integer that divides the {Bm} rows of z")
        B = Bm // members
        for name, t in (("obs", obs), ("precision", precision)):
            if t is None and name == "precision":
                continue
            if not torch.is_tensor(t) or t.dim() != 4 or tuple(t.shape[:3]) != (B, P, n_fields) or t.shape[3] < C:
                raise ValueError(f"{what}: {name} must be [{B}, {P}, {n_fields}, >= {C}] (one per history of {members} members), got "
                                 f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
            if t.dtype != torch.float32 or t.device != z.device:
                raise ValueError(f"{what}: {name} must be float32 on {z.device}, got {t.dtype} on {t.device}")
        if precision is not None and precision.shape[3] != obs.shape[3]:
            raise ValueError(f"{what}: precision must have obs's shape {tuple(obs.shape)}, got {tuple(precision.shape)}")
        if field_precision is not None and (not torch.is_tensor(field_precision) or field_precision.dtype != torch.float32 or tuple(field_precision.shape) != (n_fields,)
                                            or field_precision.device != z.device):
            raise ValueError(f"{what}: field_precision must be None or a float32 [{n_fields}] tensor on {z.device}")
        if logw is not None and (not torch.is_tensor(logw) or logw.dtype != torch.float32 or tuple(logw.shape) != (Bm,) or logw.device != z.device):
            raise ValueError(f"{what}: logw must be None or a float32 [{Bm}] tensor on {z.device}")
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (obs, precision, field_precision, logw)):
            raise ValueError(f"{what}: obs, precision, field_precision and logw must not require grad (gradients flow to z only)")
        fw = self._field_weight_on(field_weight, n_fields, z.device, what)
        self._require_frozen("member_crps_loss")
        dt = self._act_dtype()
        carried = ops.decode_member_crps_grad_supported(self.MLP_hidden, members)
        if pack is not None and not isinstance(pack, bool):
            raise ValueError(f"{what}: pack must be None, True or False, got {pack!r}")
        if pack:   # an explicit request for a form of the fused launches: a shape it refuses raises, as fused=True does
            if fused is not None and not fused:
                raise ValueError(f"{what}: pack=True is a form of the fused launches; fused=False takes the composed path")
            if not ops.decode_member_crps_pack_supported(self.MLP_hidden, members):
                raise ValueError(f"{what}: the packed form carries 1 .. {N.CRPS_PACK_MAX_N} members at MLP_hidden <= {N.DECODE_MSE_MAX_S}; got {members} members at "
                                 f"MLP_hidden = {self.MLP_hidden} (pack=False, or None, take the unpacked form)")
            fused = True
        if fused is None:
            # profiles/crps_loss_bench.txt: the fused launches are ahead in every measured row of both regimes — 64 members at 4096 and
            # 16384 rows, 4 and 8 members at 16384 - 131072 rows; above 64 members no shape the bench has is carried, below 4096 rows (below 16384 at up to 8
            # members) nothing was measured; a shape the fused form refuses takes the composed path
            fused = dt == torch.bfloat16 and carried and members <= 64 and Bm * P >= (CRPS_LOSS_FUSED_MIN_ROWS if members > 8 else CRPS_LOSS_FUSED_MIN_ROWS_SMALL)
        if fused and dt != torch.bfloat16:
            raise ValueError(f"{what}: the fused launches are bf16 only (set_compute_dtype('bf16'), or fused=False)")
        if fused and not carried:
            raise ValueError(f"{what}: the fused launches carry up to 64 members, or up to {N.FIELD_VERIFY_MAX_N} at MLP_hidden <= {N.CRPS_GRAD_W8_MAX_S}; got "
                             f"{members} members at MLP_hidden = {self.MLP_hidden} (fused=False, or None, take the composed path)")
        if pack is None:
            pack = bool(fused) and crps_loss_pack_rule(members, Bm * P, self.MLP_hidden, dt)
        cnt, _ = self._valid_counts(counts, P, z.device, allow_empty=True, what="member_crps_loss")
        N.require_gpu(z, "Decode.member_crps_loss input")
        want_grad = z.requires_grad and torch.is_grad_enabled()
        obs = obs.detach()
        prec = None if precision is None else precision.detach()
        pf = None if field_precision is None else field_precision.detach().contiguous()
        lw = None if logw is None else logw.detach().contiguous()
        if not fused:
            y = (_DecodeFn.apply(z, self) if want_grad else self.forward(z.detach())).view(Bm, P, n_fields, C)
            w = _field_cell_weights((B, P, n_fields, C), pf, prec, cnt, z.device)
            return _CrpsComposedFn.apply(y, obs, w, lw, members, bool(unbiased), fw)
        if not want_grad:
            r = self.member_verify(z, obs, members, counts=counts, precision=prec, field_precision=pf, logw=lw, unbiased=unbiased, fused=True, maps=())
            s1 = r["sums"][..., 1]
            return (s1 if fw is None else fw.to(torch.float64) * s1).to(torch.float32), r["sums"][..., 0]

        def rows(t):   # [B * P, n_fields, width] with unit inner stride: a view where the layout allows it, else one copy of the first C columns
            t3 = t.reshape(B * P, n_fields, t.shape[3])
            return t3 if t3.stride(2) == 1 and t3.stride(1) >= C and t3.stride(0) >= 0 else t3[..., :C].contiguous()

        return _DecodeCrpsFn.apply(z, self, rows(obs), None if prec is None else rows(prec), pf, fw, cnt, lw, members, bool(unbiased), bool(pack))

    def member_quantiles(self, z: torch.Tensor, members: int, levels=(), thresholds: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None,
                         counts=None, fused: Optional[bool] = None):
        """Quantile and exceedance-probability maps of an ensemble's decoded fields: (quant float32 [Q, B, P, n_fields, n_inp] or None, exceed float32
        [T, B, P, n_fields, n_inp] or None), views of n_inp_p-wide buffers as member_moments returns; no autograd graph (include/sea_hip.h,
        sea_decode_member_quantiles, states the definitions: the inverted weighted empirical distribution function; strict exceedance).  z, weights and
        counts as in member_moments: weights None (equal) or float32 [B * members] on z's device, normalised per history; a member with weight <= 0 or
        NaN is dead.  levels: up to 8 numbers in [0, 1]; thresholds: None or float32 [T <= 8, n_fields] on z's device, in the decoder's scaled units.
        Invalid cells and the pad columns are exactly 0; a live cell where a live member's value is not finite is NaN in every map.
        fused=True (bf16 compute dtype, members <= 128): the first-layer launch plus the ONE launch of sea_decode_member_quantiles — the members'
        decoded fields are never written.  fused=False: forward() plus ensemble._composed_quantiles (a stable sort and cumulative weights in float64
        torch ops: fp32, any member count, comparison).  fused=None: the fused launch in bf16 up to 128 members from 4096 rows (B * members * P) on —
        every row of profiles/ensemble_quantiles_bench.txt (tools/quantile_bench.py, DESIGN.md section 7l: 0.66 - 6.9 ms against 2.6 - 16.2 ms composed at
        4096 - 32768 rows, 13 - 112 MB of extra memory against 0.74 - 5.9 GB; thresholds only 0.20 - 0.99 ms) — and the composed path elsewhere: below
        4096 rows, where nothing was measured, in fp32 and above 128 members."""
        from ..ensemble import QUANTILES_FUSED_MIN_ROWS, _composed_quantiles

        what = "sea_amd.Decode.member_quantiles"
        n_fields = sum(len(g) for g in self.field_groups)
        C, Cp = self.n_inp, self._n_inp_p
        if not torch.is_tensor(z) or z.dim() != 4 or z.shape[2] != self.num_groups or z.shape[3] != self.embed_dim:
            raise ValueError(f"{what}: z must be [B * members, P, {self.num_groups}, {self.embed_dim}], got {tuple(z.shape) if torch.is_tensor(z) else type(z).__name__}")
        Bm, P = z.shape[0], z.shape[1]
        if not isinstance(members, int) or isinstance(members, bool) or members < 1 or Bm < 1 or Bm % members:
            raise ValueError(f"{what}: members = {members!r} must be a positive integer that divides the {Bm} rows of z")
        B = Bm // members
        levels = ops.check_quantile_levels(levels, what)
        if thresholds is not None and (not torch.is_tensor(thresholds) or thresholds.dtype != torch.float32 or thresholds.dim() != 2
                                       or not 1 <= thresholds.shape[0] <= N.QUANTILE_MAX_LEVELS or thresholds.shape[1] != n_fields or thresholds.device != z.device):
            raise ValueError(f"{what}: thresholds must be None or a float32 [1 .. {N.QUANTILE_MAX_LEVELS}, {n_fields}] tensor on {z.device}, got "
                             f"{(tuple(thresholds.shape), thresholds.dtype, str(thresholds.device)) if torch.is_tensor(thresholds) else type(thresholds).__name__}")
        if not levels and thresholds is None:
            raise ValueError(f"{what}: neither levels nor thresholds: there is nothing to compute")
        if weights is not None:
            if not torch.is_tensor(weights) or weights.dim() != 1 or weights.shape[0] != Bm:
                raise ValueError(f"{what}: weights must be None or a [{Bm}] tensor (one weight per member), got "
                                 f"{tuple(weights.shape) if torch.is_tensor(weights) else type(weights).__name__}")
            if weights.dtype != torch.float32 or weights.device != z.device:
                raise ValueError(f"{what}: weights must be float32 on {z.device}, got {weights.dtype} on {weights.device}")
        dt = self._act_dtype()
        if fused is None:
            fused = dt == torch.bfloat16 and members <= N.QUANTILE_MAX_N and Bm * P >= QUANTILES_FUSED_MIN_ROWS
        if fused and dt != torch.bfloat16:
            raise ValueError(f"{what}: the fused launch is bf16 only (set_compute_dtype('bf16'), or fused=False)")
        if fused and members > N.QUANTILE_MAX_N:
            raise ValueError(f"{what}: the fused launch carries up to {N.QUANTILE_MAX_N} members, got {members} (fused=False, or None)")
        cnt, _ = self._valid_counts(counts, P, z.device, allow_empty=True, what="member_quantiles")
        N.require_gpu(z, "Decode.member_quantiles input")
        with torch.no_grad():
            w = None if weights is None else weights.detach().contiguous()
            thr = None if thresholds is None else thresholds.detach().contiguous()
            n_q, n_t = len(levels), 0 if thr is None else thr.shape[0]
            out = {}
            if not fused:
                y = self.forward(z.detach()).view(B, members, P, n_fields, C)
                q, e = _composed_quantiles(y, None if w is None else w.view(B, members), levels, thr)
                valid = None if cnt is None else (torch.arange(C, device=z.device) < cnt[:, None]).view(1, 1, P, 1, C)
                for name, t, k in (("quant", q, n_q), ("exceed", e, n_t)):
                    if t is not None:
                        buf = torch.zeros(k, B, P, n_fields, Cp, device=z.device, dtype=torch.float32)
                        buf[..., :C] = t if valid is None else torch.where(valid, t.to(torch.float32), torch.zeros((), device=z.device))
                        out[name] = buf
            else:
                M = Bm * P
                G, D = self.num_groups, self.embed_dim
                zf = z.detach().to(torch.float32).contiguous().view(M, G * D)
                za = torch.empty(M, G * D, device=z.device, dtype=dt)
                ops.convert(zf, za)
                W1, W2 = self._weights(dt)
                hid = [torch.empty(M, self.MLP_hidden, device=z.device, dtype=dt) for _ in range(G)]
                ops.gemm_grouped([dict(A=za[:, g * D:(g + 1) * D], W=W1[g], Cact=hid[g], act=1) for g in range(G)], dt)
                bias = self._shadow[3]
                bufs = {name: torch.empty(k, B, P, n_fields, Cp, device=z.device, dtype=torch.float32) for name, k in (("quant", n_q), ("exceed", n_t)) if k}
                out = ops.decode_member_quantiles([dict(H=hid[g], W2=W2[g], bias=bias[g]) for g in range(G)], C, Cp, P, members, levels=levels, thr=thr, w=w,
                                                  counts=cnt, out=bufs, dtype=dt)
            quant, exceed = out.get("quant"), out.get("exceed")
            if Cp != C:
                quant = None if quant is None else quant[..., :C]
                exceed = None if exceed is None else exceed[..., :C]
            return quant, exceed

    def _derived_call(self, what: str, z, members, derived, fused, max_n: int, min_rows: int):
        """The checks member_derived_quantiles and member_derived_brier share.  Returns (derived as a tuple, Bm, P, B, fused resolved): fused=None takes
        the fused launches in bf16 up to max_n members, with every derived field's sources in one decoder group, from min_rows rows on."""
        n_fields = sum(len(g) for g in self.field_groups)
        if not torch.is_tensor(z) or z.dim() != 4 or z.shape[2] != self.num_groups or z.shape[3] != self.embed_dim:
            raise ValueError(f"{what}: z must be [B * members, P, {self.num_groups}, {self.embed_dim}], got {tuple(z.shape) if torch.is_tensor(z) else type(z).__name__}")
        Bm, P = z.shape[0], z.shape[1]
        if not isinstance(members, int) or isinstance(members, bool) or members < 1 or Bm < 1 or Bm % members:
            raise ValueError(f"{what}: members = {members!r} must be a positive integer that divides the {Bm} rows of z")
        try:
            derived = tuple(derived)
        except TypeError:
            raise ValueError(f"{what}: derived must be a sequence of DerivedField, got {type(derived).__name__}") from None
        if not derived or any(not all(hasattr(d, k) for k in ("op", "a", "b", "scale_a", "shift_a", "scale_b", "shift_b")) for d in derived):
            raise ValueError(f"{what}: derived must be a non-empty sequence of DerivedField")
        for i, d in enumerate(derived):
            if not (0 <= d.a < n_fields and 0 <= d.b < n_fields) or d.a == d.b:
                raise ValueError(f"{what}: derived field {i}: sources a = {d.a}, b = {d.b} must be two different fields in 0 .. {n_fields - 1}")
        group_of = [g for g, fields in enumerate(self.field_groups) for _ in fields]   # the decoder group of every field, in output order
        one_group = all(group_of[d.a] == group_of[d.b] for d in derived)
        dt = self._act_dtype()
        if fused is None:
            fused = dt == torch.bfloat16 and members <= max_n and one_group and len(derived) <= N.DERIVED_MAX and Bm * P >= min_rows
        if fused and dt != torch.bfloat16:
            raise ValueError(f"{what}: the fused launches are bf16 only (set_compute_dtype('bf16'), or fused=False)")
        if fused and members > max_n:
            raise ValueError(f"{what}: the fused launches carry up to {max_n} members, got {members} (fused=False, or None)")
        if fused and len(derived) > N.DERIVED_MAX:
            raise ValueError(f"{what}: the fused launches carry up to {N.DERIVED_MAX} derived fields, got {len(derived)} (fused=False, or None)")
        return derived, Bm, P, Bm // members, bool(fused)

    def _hidden_groups(self, z: torch.Tensor, dt: torch.dtype):
        """The first decoder layer in one grouped launch: the operand groups [dict(H, W2, bias)] of the fused decode launches."""
        Bm, P = z.shape[0], z.shape[1]
        M = Bm * P
        G, D = self.num_groups, self.embed_dim
        zf = z.detach().to(torch.float32).contiguous().view(M, G * D)
        za = torch.empty(M, G * D, device=z.device, dtype=dt)
        ops.convert(zf, za)
        W1, W2 = self._weights(dt)
        hid = [torch.empty(M, self.MLP_hidden, device=z.device, dtype=dt) for _ in range(G)]
        ops.gemm_grouped([dict(A=za[:, g * D:(g + 1) * D], W=W1[g], Cact=hid[g], act=1) for g in range(G)], dt)
        bias = self._shadow[3]
        return [dict(H=hid[g], W2=W2[g], bias=bias[g]) for g in range(G)]

    def member_derived_quantiles(self, z: torch.Tensor, members: int, derived, levels=(), thresholds: Optional[torch.Tensor] = None,
                                 weights: Optional[torch.Tensor] = None, counts=None, fused: Optional[bool] = None):
        """member_quantiles for DERIVED fields — the magnitude, the energy or the difference of two decoded fields, formed per member (include/sea_hip.h,
        sea_decode_derived_quantiles, states the definitions; sea_amd.ensemble.DerivedField): (quant float32 [Q, B, P, n_derived, n_inp] or None, exceed
        float32 [T, B, P, n_derived, n_inp] or None); no autograd graph.  z, levels, weights and counts as in member_quantiles; derived: a sequence of
        DerivedField; thresholds: None or float32 [T <= 8, n_derived] on z's device, in the derived fields' own (physical) units.
        fused=True (bf16, members <= 128, up to 8 derived fields, each with both sources in one decoder group): the first-layer launch plus the ONE
        launch of sea_decode_derived_quantiles — neither the members' decoded fields nor the derived fields are written; it raises where the launch
        refuses.  fused=False: forward() plus ensemble._composed_derived plus ensemble._composed_quantiles (float32 values, float64 weights: fp32, any
        member count, sources in different groups, comparison).  fused=None: the fused launch where it serves, from 4096 rows (B * members * P) on —
        the rows of profiles/derived_fields_bench.txt (tools/derived_fields_bench.py) — and the composed path elsewhere."""
        from ..ensemble import DERIVED_FUSED_MIN_ROWS, _composed_derived, _composed_quantiles

        what = "sea_amd.Decode.member_derived_quantiles"
        n_fields = sum(len(g) for g in self.field_groups)
        C, Cp = self.n_inp, self._n_inp_p
        derived, Bm, P, B, fused = self._derived_call(what, z, members, derived, fused, N.QUANTILE_MAX_N, DERIVED_FUSED_MIN_ROWS)
        nd = len(derived)
        levels = ops.check_quantile_levels(levels, what)
        if thresholds is not None and (not torch.is_tensor(thresholds) or thresholds.dtype != torch.float32 or thresholds.dim() != 2
                                       or not 1 <= thresholds.shape[0] <= N.QUANTILE_MAX_LEVELS or thresholds.shape[1] != nd or thresholds.device != z.device):
            raise ValueError(f"{what}: thresholds must be None or a float32 [1 .. {N.QUANTILE_MAX_LEVELS}, {nd}] tensor on {z.device}, got "
                             f"{(tuple(thresholds.shape), thresholds.dtype, str(thresholds.device)) if torch.is_tensor(thresholds) else type(thresholds).__name__}")
        if not levels and thresholds is None:
            raise ValueError(f"{what}: neither levels nor thresholds: there is nothing to compute")
        if weights is not None:
            if not torch.is_tensor(weights) or weights.dim() != 1 or weights.shape[0] != Bm:
                raise ValueError(f"{what}: weights must be None or a [{Bm}] tensor (one weight per member), got "
                                 f"{tuple(weights.shape) if torch.is_tensor(weights) else type(weights).__name__}")
            if weights.dtype != torch.float32 or weights.device != z.device:
                raise ValueError(f"{what}: weights must be float32 on {z.device}, got {weights.dtype} on {weights.device}")
        cnt, _ = self._valid_counts(counts, P, z.device, allow_empty=True, what="member_derived_quantiles")
        N.require_gpu(z, "Decode.member_derived_quantiles input")
        with torch.no_grad():
            w = None if weights is None else weights.detach().contiguous()
            thr = None if thresholds is None else thresholds.detach().contiguous()
            n_q, n_t = len(levels), 0 if thr is None else thr.shape[0]
            out = {}
            if not fused:
                y = self.forward(z.detach()).view(B, members, P, n_fields, C)
                q, e = _composed_quantiles(_composed_derived(y, derived), None if w is None else w.view(B, members), levels, thr)
                valid = None if cnt is None else (torch.arange(C, device=z.device) < cnt[:, None]).view(1, 1, P, 1, C)
                for name, t, k in (("quant", q, n_q), ("exceed", e, n_t)):
                    if t is not None:
                        buf = torch.zeros(k, B, P, nd, Cp, device=z.device, dtype=torch.float32)
                        buf[..., :C] = t if valid is None else torch.where(valid, t.to(torch.float32), torch.zeros((), device=z.device))
                        out[name] = buf
            else:
                dt = self._act_dtype()
                bufs = {name: torch.empty(k, B, P, nd, Cp, device=z.device, dtype=torch.float32) for name, k in (("quant", n_q), ("exceed", n_t)) if k}
                out = ops.decode_derived_quantiles(self._hidden_groups(z, dt), derived, C, Cp, P, members, levels=levels, thr=thr, w=w, counts=cnt, out=bufs, dtype=dt)
            quant, exceed = out.get("quant"), out.get("exceed")
            if Cp != C:
                quant = None if quant is None else quant[..., :C]
                exceed = None if exceed is None else exceed[..., :C]
            return quant, exceed

    def member_derived_brier(self, z: torch.Tensor, obs: torch.Tensor, members: int, derived, thresholds: torch.Tensor, counts=None,
                             precision: Optional[torch.Tensor] = None, field_precision: Optional[torch.Tensor] = None, logw: Optional[torch.Tensor] = None,
                             fused: Optional[bool] = None, maps=(), into: Optional[dict] = None):
        """member_brier for DERIVED fields (include/sea_hip.h, sea_decode_derived_brier; sea_amd.ensemble.DerivedField): the dict of member_brier with
        n_derived where that has n_fields; no autograd graph.  z, counts, logw, maps and into as in member_brier; derived: a sequence of DerivedField;
        obs and precision float32 [B, P, n_derived, >= n_inp]: readings of the DERIVED quantities (ensemble.DerivedThresholdVerification forms them from a
        snapshot of the source fields); field_precision float32 [n_derived]; thresholds float32 [T <= 8, n_derived] on z's device, in the derived
        fields' own units.  fused as in member_derived_quantiles: True — the first-layer launch plus the TWO launches of sea_decode_derived_brier; False —
        forward() plus ensemble._composed_derived plus ensemble._composed_field_brier; None — the fused launches where they serve, from 4096 rows on."""
        from ..ensemble import BRIER_MAPS, DERIVED_FUSED_MIN_ROWS, _composed_derived, _composed_field_brier, _field_cell_weights

        what = "sea_amd.Decode.member_derived_brier"
        n_fields = sum(len(g) for g in self.field_groups)
        C, Cp = self.n_inp, self._n_inp_p
        derived, Bm, P, B, fused = self._derived_call(what, z, members, derived, fused, N.BRIER_MAX_N, DERIVED_FUSED_MIN_ROWS)
        nd = len(derived)
        for name, t in (("obs", obs), ("precision", precision)):
            if t is None and name == "precision":
                continue
            if not torch.is_tensor(t) or t.dim() != 4 or tuple(t.shape[:3]) != (B, P, nd) or t.shape[3] < C:
                raise ValueError(f"{what}: {name} must be [{B}, {P}, {nd}, >= {C}] (one per history of {members} members), got "
                                 f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
            if t.dtype != torch.float32 or t.device != z.device:
                raise ValueError(f"{what}: {name} must be float32 on {z.device}, got {t.dtype} on {t.device}")
        if precision is not None and precision.shape[3] != obs.shape[3]:
            raise ValueError(f"{what}: precision must have obs's shape {tuple(obs.shape)}, got {tuple(precision.shape)}")
        if field_precision is not None and (not torch.is_tensor(field_precision) or field_precision.dtype != torch.float32 or tuple(field_precision.shape) != (nd,)
                                            or field_precision.device != z.device):
            raise ValueError(f"{what}: field_precision must be None or a float32 [{nd}] tensor on {z.device}")
        if logw is not None and (not torch.is_tensor(logw) or logw.dtype != torch.float32 or tuple(logw.shape) != (Bm,) or logw.device != z.device):
            raise ValueError(f"{what}: logw must be None or a float32 [{Bm}] tensor on {z.device}")
        thr = thresholds.detach().contiguous() if torch.is_tensor(thresholds) else thresholds
        ops.check_brier_thresholds(thr, nd, z.device, what)
        T = thr.shape[0]
        maps = tuple(maps)
        if any(k not in BRIER_MAPS for k in maps) or len(set(maps)) != len(maps):
            raise ValueError(f"{what}: maps must be distinct names among {BRIER_MAPS}, got {maps!r}")
        shapes = (("sums", (B, nd, T, N.BRIER_SUMS), torch.float64), ("hist", (B, nd, T, members + 1), torch.int64), ("hits", (B, nd, T, members + 1), torch.int64))
        if into is not None and (not isinstance(into, dict) or set(into) != {"sums", "hist", "hits"} or any(
                not torch.is_tensor(into[k]) or tuple(into[k].shape) != sh or into[k].dtype != dt_ or into[k].device != z.device or not into[k].is_contiguous()
                for k, sh, dt_ in shapes)):
            raise ValueError(f"{what}: into must be a dict of contiguous sums float64 [{B}, {nd}, {T}, {N.BRIER_SUMS}], hist and hits int64 [{B}, {nd}, {T}, "
                             f"{members + 1}] on {z.device}")
        cnt, _ = self._valid_counts(counts, P, z.device, allow_empty=True, what="member_derived_brier")
        N.require_gpu(z, "Decode.member_derived_brier input")
        with torch.no_grad():
            obs = obs.detach()
            prec = None if precision is None else precision.detach()
            pf = None if field_precision is None else field_precision.detach().contiguous()
            lw = None if logw is None else logw.detach().contiguous()
            if not fused:
                y = self.forward(z.detach()).view(B, members, P, n_fields, C)
                x = _composed_derived(y, derived).view(Bm, P, nd, C)
                w = _field_cell_weights((B, P, nd, C), pf, prec, cnt, z.device)
                r = _composed_field_brier(x, obs, w, lw, members, thr, maps=maps)
                if into is not None:
                    r["sums"], r["hist"], r["hits"] = into["sums"].add_(r["sums"]), into["hist"].add_(r["hist"]), into["hits"].add_(r["hits"])
                return r

            def rows(t):   # [B * P, n_derived, width] with unit inner stride: a view where the layout allows it, else one copy of the first C columns
                t3 = t.reshape(B * P, nd, t.shape[3])
                return t3 if t3.stride(2) == 1 and t3.stride(1) >= C and t3.stride(0) >= 0 else t3[..., :C].contiguous()

            dt = self._act_dtype()
            return ops.decode_derived_brier(self._hidden_groups(z, dt), derived, rows(obs), C, Cp, P, members, thr, prec_field=pf,
                                            prec=None if prec is None else rows(prec), counts=cnt, logw=lw, accumulate=into is not None, maps=maps, out=into, dtype=dt)

    def member_derived_verify(self, z: torch.Tensor, obs: torch.Tensor, members: int, derived, counts=None, precision: Optional[torch.Tensor] = None,
                              field_precision: Optional[torch.Tensor] = None, logw: Optional[torch.Tensor] = None, unbiased: bool = True,
                              fused: Optional[bool] = None, maps=("mean", "spread", "crps", "pit", "rank"), into: Optional[dict] = None):
        """member_verify for DERIVED fields (include/sea_hip.h, sea_decode_derived_verify; sea_amd.ensemble.DerivedField): the dict of member_verify with
        n_derived where that has n_fields; no autograd graph.  z, counts, logw, unbiased, maps and into as in member_verify; derived: a sequence of
        DerivedField; obs and precision float32 [B, P, n_derived, >= n_inp]: readings of the DERIVED quantities, in their own units
        (ensemble.DerivedVerification forms them from a snapshot of the source fields); field_precision float32 [n_derived]: the weight of a cell is
        w = valid ? max(field_precision, 0) * max(precision, 0) : 0, and 1 / w is its observation-error variance.
        fused=True (bf16, members <= 128, up to 8 derived fields, each with both sources in one decoder group): the first-layer launch plus the TWO
        launches of sea_decode_derived_verify — neither the members' decoded fields nor the derived fields are written; it raises where the launch
        refuses.  fused=False: forward() plus ensemble._composed_derived plus ensemble._composed_field_verify (fp32, any member count, sources in
        different groups, comparison).  fused=None: the fused launches where they serve, from ensemble.DERIVED_VERIFY_FUSED_MIN_ROWS = 4096 rows
        (B * members * P) on — the rows of profiles/derived_verify_bench.txt (tools/derived_verify_bench.py) — and the composed
        path elsewhere (everywhere if that constant is None)."""
        from ..ensemble import DERIVED_VERIFY_FUSED_MIN_ROWS, FIELD_MAPS, _composed_derived, _composed_field_verify, _field_cell_weights

        what = "sea_amd.Decode.member_derived_verify"
        n_fields = sum(len(g) for g in self.field_groups)
        C, Cp = self.n_inp, self._n_inp_p
        min_rows = DERIVED_VERIFY_FUSED_MIN_ROWS
        derived, Bm, P, B, fused = self._derived_call(what, z, members, derived, False if fused is None and min_rows is None else fused, N.FIELD_VERIFY_MAX_N,
                                                      0 if min_rows is None else min_rows)
        nd = len(derived)
        for name, t in (("obs", obs), ("precision", precision)):
            if t is None and name == "precision":
                continue
            if not torch.is_tensor(t) or t.dim() != 4 or tuple(t.shape[:3]) != (B, P, nd) or t.shape[3] < C:
                raise ValueError(f"{what}: {name} must be [{B}, {P}, {nd}, >= {C}] (one per history of {members} members), got "
                                 f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
            if t.dtype != torch.float32 or t.device != z.device:
                raise ValueError(f"{what}: {name} must be float32 on {z.device}, got {t.dtype} on {t.device}")
        if precision is not None and precision.shape[3] != obs.shape[3]:
            raise ValueError(f"{what}: precision must have obs's shape {tuple(obs.shape)}, got {tuple(precision.shape)}")
        if field_precision is not None and (not torch.is_tensor(field_precision) or field_precision.dtype != torch.float32 or tuple(field_precision.shape) != (nd,)
                                            or field_precision.device != z.device):
            raise ValueError(f"{what}: field_precision must be None or a float32 [{nd}] tensor on {z.device}")
        if logw is not None and (not torch.is_tensor(logw) or logw.dtype != torch.float32 or tuple(logw.shape) != (Bm,) or logw.device != z.device):
            raise ValueError(f"{what}: logw must be None or a float32 [{Bm}] tensor on {z.device}")
        maps = tuple(maps)
        if any(k not in FIELD_MAPS for k in maps) or len(set(maps)) != len(maps):
            raise ValueError(f"{what}: maps must be distinct names among {FIELD_MAPS}, got {maps!r}")
        if into is not None and (not isinstance(into, dict) or set(into) != {"sums", "hist"} or any(
                not torch.is_tensor(t) or tuple(t.shape) != sh or t.dtype != dt_ or t.device != z.device or not t.is_contiguous()
                for t, sh, dt_ in ((into.get("sums"), (B, nd, N.VERIFY_SUMS), torch.float64), (into.get("hist"), (B, nd, members + 1), torch.int64)))):
            raise ValueError(f"{what}: into must be a dict of contiguous sums float64 [{B}, {nd}, {N.VERIFY_SUMS}] and hist int64 [{B}, {nd}, {members + 1}] on {z.device}")
        cnt, _ = self._valid_counts(counts, P, z.device, allow_empty=True, what="member_derived_verify")
        N.require_gpu(z, "Decode.member_derived_verify input")
        with torch.no_grad():
            obs = obs.detach()
            prec = None if precision is None else precision.detach()
            pf = None if field_precision is None else field_precision.detach().contiguous()
            lw = None if logw is None else logw.detach().contiguous()
            if not fused:
                y = self.forward(z.detach()).view(B, members, P, n_fields, C)
                x = _composed_derived(y, derived).view(Bm, P, nd, C)
                w = _field_cell_weights((B, P, nd, C), pf, prec, cnt, z.device)
                r = _composed_field_verify(x, obs, w, lw, members, bool(unbiased), maps=maps)
                if into is not None:
                    r["sums"], r["hist"] = into["sums"].add_(r["sums"]), into["hist"].add_(r["hist"])
                return r

            def rows(t):   # [B * P, n_derived, width] with unit inner stride: a view where the layout allows it, else one copy of the first C columns
                t3 = t.reshape(B * P, nd, t.shape[3])
                return t3 if t3.stride(2) == 1 and t3.stride(1) >= C and t3.stride(0) >= 0 else t3[..., :C].contiguous()

            dt = self._act_dtype()
            return ops.decode_derived_verify(self._hidden_groups(z, dt), derived, rows(obs), C, Cp, P, members, prec_field=pf,
                                             prec=None if prec is None else rows(prec), counts=cnt, logw=lw, unbiased=bool(unbiased),
                                             accumulate=into is not None, maps=maps, out=into, dtype=dt)

    def forward_prefix(self, z: torch.Tensor, buckets) -> torch.Tensor:
        """The decoder for a consumer that only reads the first cells of a patch (MeshUnpatcher.decode_and_unpatch: a patch holds as many mesh points as its
        cell has, the rest of its n_inp columns is padding nobody reads — 71 % of the columns on the bench's wake-refined mesh).  z [B, P, n_groups,
        embed_dim] with the patches in the CALLER's order; buckets: [(p_lo, p_hi, n_cols)] covering 0 .. P — for the patches p_lo .. p_hi-1 only the first
        n_cols columns of every field are computed.  Rows are patch-major inside (a bucket is one contiguous row range: one GEMM group per (bucket, field)
        with the first n_cols rows of the field's second-layer weights).  Returns [B, P, n_fields, n_inp] as a strided view; columns >= n_cols of a
        bucket's patches are UNDEFINED."""
        N.require_gpu(z, "Decode input")
        B, P, G, D = z.shape
        assert G == self.num_groups and D == self.embed_dim, (z.shape, self.num_groups, self.embed_dim)
        dt = torch.float32 if self.compute_dtype == "fp32" else torch.bfloat16
        M = B * P
        zf = z.detach().to(torch.float32).permute(1, 0, 2, 3).contiguous().view(M, G * D)      # patch-major rows
        za = zf if dt == torch.float32 else torch.empty(M, G * D, device=z.device, dtype=dt)
        if dt != torch.float32:
            ops.convert(zf, za)
        W1, W2 = self._weights(dt)
        bias = self._shadow[3]
        n_fields = sum(len(g) for g in self.field_groups)
        Cp = self._n_inp_p
        out = torch.empty(M, n_fields * Cp, device=z.device, dtype=torch.float32)
        hid: List[torch.Tensor] = [torch.empty(M, self.MLP_hidden, device=z.device, dtype=dt) for _ in range(G)]
        ops.gemm_grouped([dict(A=za[:, g * D:(g + 1) * D], W=W1[g], Cact=hid[g], act=1) for g in range(G)], dt)
        groups = []
        for p_lo, p_hi, n_cols in buckets:
            nn = min(_round_up(max(int(n_cols), 1), 32), Cp)
            r0, r1 = p_lo * B, p_hi * B
            f = 0
            for g, grp in enumerate(self.field_groups):
                for j in range(len(grp)):
                    groups.append(dict(A=hid[g][r0:r1], W=W2[g][j * Cp:j * Cp + nn], bias=bias[g][j * Cp:j * Cp + nn], C32=out[r0:r1, f * Cp:f * Cp + nn]))
                    f += 1
        for s0 in range(0, len(groups), N.MAX_GROUPS):
            ops.gemm_grouped(groups[s0:s0 + N.MAX_GROUPS], dt)
        return out.view(P, B, n_fields, Cp).permute(1, 0, 2, 3)[..., :self.n_inp]


class _DecodeFn(torch.autograd.Function):
    """Decode.forward with a gradient to z: the launches of the inference forward (the first with the GELU pre-activation kept); the backward is two
    grouped data-gradient launches of sea_gemm_grouped — against W2^T with GELU' of the saved pre-activation in the epilogue, then against W1^T."""

    @staticmethod
    def forward(ctx, z, dec):
        dt = dec._act_dtype()
        B, P, G, _ = z.shape
        M = B * P
        hid, pre = dec._first_layer(z, dt)
        _, W2 = dec._weights(dt)
        n_fields = sum(len(g) for g in dec.field_groups)
        Cp = dec._n_inp_p
        out = torch.empty(M, n_fields * Cp, device=z.device, dtype=torch.float32)
        groups, off = [], 0
        for g, grp in enumerate(dec.field_groups):
            w = len(grp) * Cp
            groups.append(dict(A=hid[g], W=W2[g], bias=dec._shadow[3][g], C32=out[:, off:off + w]))
            off += w
        ops.gemm_grouped(groups, dt)
        ctx.dec, ctx.dt, ctx.zshape, ctx.zdtype = dec, dt, z.shape, z.dtype
        ctx.save_for_backward(*pre)
        out = out.view(B, P, n_fields, Cp)
        return out if Cp == dec.n_inp else out[..., :dec.n_inp]

    @staticmethod
    def backward(ctx, dout):
        dec, dt, pre = ctx.dec, ctx.dt, ctx.saved_tensors
        B, P, G, _ = ctx.zshape
        M, C, Cp = B * P, dec.n_inp, dec._n_inp_p
        n_fields = sum(len(g) for g in dec.field_groups)
        dev = dout.device
        if Cp == C:
            dpad = dout.to(torch.float32).contiguous().view(M, n_fields * Cp)
        else:
            dpad = torch.zeros(B, P, n_fields, Cp, device=dev, dtype=torch.float32)
            dpad[..., :C] = dout
            dpad = dpad.view(M, n_fields * Cp)
        da = dpad
        if dt != torch.float32:
            da = torch.empty(M, n_fields * Cp, device=dev, dtype=dt)
            ops.convert(dpad, da)
        _, W2T = dec._weights_T(dt)
        dpre = [torch.empty(M, dec.MLP_hidden, device=dev, dtype=dt) for _ in range(G)]
        groups, off = [], 0
        for g, grp in enumerate(dec.field_groups):
            w = len(grp) * Cp
            groups.append(dict(A=da[:, off:off + w], W=W2T[g], act=2, Z=pre[g], Cact=dpre[g]))
            off += w
        ops.gemm_grouped(groups, dt)
        return dec._input_grad(dpre, dt).view(ctx.zshape).to(ctx.zdtype), None


class _DecodeMseFn(torch.autograd.Function):
    """Decode.mse_loss on the fused path: first layer (pre-activation kept), sea_decode_mse (second layer, masked MSE and the gradient of the
    pre-activation in one launch; nothing of size [rows, columns] is allocated), data-gradient launch against W1^T.  Forward and backward are one
    pass, as in MSELossFn: the backward scales the stored dz."""

    @staticmethod
    def forward(ctx, z, dec, target, counts, n_valid):
        dt = torch.bfloat16
        B, P, G, _ = z.shape
        M = B * P
        t3 = target.reshape(M, target.shape[2], target.shape[3])
        if t3.stride(2) != 1 or t3.stride(0) % 4 or t3.stride(1) % 4 or t3.data_ptr() % 16:
            # a contiguous target of an odd cell width, or the reference's [.., C, n_fields] layout seen through a permute: one row-aligned copy
            src = t3[..., :dec.n_inp]
            t3 = torch.zeros(M, src.shape[1], (dec.n_inp + 3) // 4 * 4, device=src.device, dtype=torch.float32)
            t3[..., :dec.n_inp] = src
        hid, pre = dec._first_layer(z, dt)
        _, W2 = dec._weights(dt)
        bias = dec._shadow[3]
        dpre = [torch.empty(M, dec.MLP_hidden, device=z.device, dtype=dt) for _ in range(G)]
        loss = ops.decode_mse([dict(H=hid[g], W2=W2[g], bias=bias[g], dH=dpre[g], Z=pre[g]) for g in range(G)], t3, dec.n_inp, dec._n_inp_p,
                              1.0 / n_valid, counts=counts, n_patches=P, dtype=dt)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(dec._input_grad(dpre, dt).view(z.shape).to(z.dtype))
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dz,) = ctx.saved_tensors
        return dz * g, None, None, None, None


class _DecodeSensorFn(torch.autograd.Function):
    """Decode.sensor_loss on the fused path (Decode._sensor_grad_fused): first layer over the observed patches' rows (pre-activation kept),
    sea_decode_sensor_grad (score and pre-activation gradient in one launch), data-gradient launch against W1^T, one index_copy_ into the zeroed dz.
    Forward and backward are one pass, as in _DecodeMseFn: wsse[bm] depends on z[bm] only, so the backward scales the stored dz per member."""

    @staticmethod
    def forward(ctx, z, dec, sensors, obs, prec, members, predictions):
        wsse, pred, dz = dec._sensor_grad_fused(z, sensors, obs, prec, members, predictions, ctx.needs_input_grad[0])
        if dz is not None:
            ctx.save_for_backward(dz.to(z.dtype))
        if not predictions:
            return wsse
        ctx.mark_non_differentiable(pred)
        return wsse, pred

    @staticmethod
    def backward(ctx, g, *unused):
        (dz,) = ctx.saved_tensors
        return (dz * g.view(-1, 1, 1, 1)).to(dz.dtype), None, None, None, None, None, None


class _DecodeFieldFn(torch.autograd.Function):
    """Decode.field_loss on the fused path (Decode._field_grad_fused): first layer (pre-activation kept), sea_decode_field_grad (score and
    pre-activation gradient in one launch), data-gradient launch against W1^T.  Forward and backward are one pass, as in _DecodeMseFn: wsse[bm, f]
    depends on z[bm, :, g, :] only (g the group of field f), so the backward scales the stored dz per member and group; an upstream gradient that
    differs between the fields of one group cannot be represented by the one stored dz and turns that slice into NaN (a select, nothing read back)."""

    @staticmethod
    def forward(ctx, z, dec, obs, prec, pf, cnt, members):
        wsse, dz = dec._field_grad_fused(z, obs, prec, pf, cnt, members, ctx.needs_input_grad[0])
        if dz is not None:
            ctx.save_for_backward(dz.to(z.dtype))
        ctx.groups = [len(g) for g in dec.field_groups]
        return wsse

    @staticmethod
    def backward(ctx, g):
        (dz,) = ctx.saved_tensors
        if g.stride(1) == 0:   # an expanded upstream (wsse.sum(), c[bm] * wsse.sum(1)): the same for every field by construction
            return (dz * g[:, 0].view(-1, 1, 1, 1)).to(dz.dtype), None, None, None, None, None, None
        cols, off = [], 0
        for n in ctx.groups:
            first = g[:, off]
            same = (g[:, off:off + n] == first.unsqueeze(1)).all(dim=1)
            cols.append(torch.where(same, first, torch.full_like(first, float("nan"))))
            off += n
        factor = torch.stack(cols, dim=1).view(dz.shape[0], 1, len(cols), 1)          # [Bm, 1, G, 1]
        return (dz * factor).to(dz.dtype), None, None, None, None, None, None


class _DecodeCrpsFn(torch.autograd.Function):
    """Decode.member_crps_loss on the fused path: first layer (pre-activation kept), sea_decode_member_crps_grad (the CRPS sums and the
    pre-activation gradient in its two launches), data-gradient launch against W1^T.  Forward and backward are one pass, as in _DecodeFieldFn:
    loss[b, f] depends on the rows of history b's members in the group of field f only, so the backward scales the stored dz per history and group; an
    upstream gradient that differs between the fields of one group turns that slice into NaN (a select, nothing read back)."""

    @staticmethod
    def forward(ctx, z, dec, o3, p3, pf, fw, cnt, lw, members, unbiased, pack=False):
        dt = torch.bfloat16
        with torch.no_grad():
            Bm, P, G, D = z.shape
            M = Bm * P
            hid, pre = dec._first_layer(z, dt)
            _, W2 = dec._weights(dt)
            bias = dec._shadow[3]
            dpre = [torch.empty(M, dec.MLP_hidden, device=z.device, dtype=dt) for _ in range(G)]
            groups = [dict(H=hid[g], W2=W2[g], bias=bias[g], dH=dpre[g], Z=pre[g]) for g in range(G)]
            loss, sums, _ = ops.decode_member_crps_grad(groups, o3, dec.n_inp, dec._n_inp_p, P, members, prec=p3, prec_field=pf, field_weight=fw, counts=cnt,
                                                        logw=lw, unbiased=unbiased, dtype=dt, pack=pack)
            ctx.save_for_backward(dec._input_grad(dpre, dt).view(Bm, P, G, D).to(z.dtype))
        ctx.groups, ctx.members = [len(g) for g in dec.field_groups], members
        count = sums[..., 0].contiguous()
        ctx.mark_non_differentiable(count)
        return loss, count

    @staticmethod
    def backward(ctx, g, _unused):
        (dz,) = ctx.saved_tensors
        Bm, P, G, D = dz.shape
        n = ctx.members
        cols, off = [], 0
        for k in ctx.groups:
            first = g[:, off]
            same = (g[:, off:off + k] == first.unsqueeze(1)).all(dim=1)
            cols.append(torch.where(same, first, torch.full_like(first, float("nan"))))
            off += k
        factor = torch.stack(cols, dim=1).view(Bm // n, 1, 1, G, 1)                       # [B, 1, 1, G, 1]
        return (dz.view(Bm // n, n, P, G, D) * factor).view(Bm, P, G, D).to(dz.dtype), None, None, None, None, None, None, None, None, None, None


CRPS_LOSS_FUSED_MIN_ROWS_SMALL = 16384   # ... and with up to 8 members, where the smallest measured size is 64 histories x 4 members x 64 patches
CRPS_LOSS_PACK_MEMBERS = (2, 32)   # member_crps_loss, pack=None: the packed form at these member counts (the measured 2, 4, 8, 16, 32 and between them) ...
CRPS_LOSS_PACK_MIN_PAIRS = 4096    # ... from this many (history, patch) pairs on, i.e. rows >= 4096 * members: the smallest measured size at every member count (64 histories x 64 patches)


def crps_loss_pack_rule(members: int, rows: int, hidden: int, dtype) -> bool:
    """Decode.member_crps_loss's pack=None: whether the fused launches take the packed form (sea_decode_member_crps_grad_packed) at this member count,
    number of decoder rows (B * members * n_patches), MLP_hidden and compute dtype.  A pure function of its arguments, read from
    profiles/crps_pack_bench.txt: at 2, 4, 8, 16 and 32 members x 64 histories (4 and 8 members: x 256 too) x 64 patches the
    packed form is ahead of the unpacked one in EVERY measured row — 17 - 30x at 2 members, 15 - 16x at 4, 8.0 - 8.5x at 8, 4.0x at 16, 2.05x at 32,
    against a run-to-run spread of up to 1.4 % — with the same bits, so it is taken at 2 .. 32 members (the counts between measured ones lie between
    two that are both ahead) from the smallest measured size on: 4096 (history, patch) pairs, rows >= 4096 * members.  Everywhere else — tiny shapes,
    1 member and above 32 members, fp32, widths the form does not carry — the unpacked form."""
    return (dtype == torch.bfloat16 and isinstance(members, int) and CRPS_LOSS_PACK_MEMBERS[0] <= members <= CRPS_LOSS_PACK_MEMBERS[1]
            and rows >= CRPS_LOSS_PACK_MIN_PAIRS * members and ops.decode_member_crps_pack_supported(hidden, members))


CRPS_LOSS_FUSED_MIN_ROWS = 4096   # member_crps_loss, fused=None: the fused launches from this many decoder rows (B * members * n_patches) on — the smallest measured size


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


class PointwiseEncode(nn.Module):
    """PointwiseEncode(field_groups, n_inp, MLP_hidden, num_layers, embed_dim, n_heads, max_len, src_len, dropout=0.1)
    .forward(x [B, P, n_fields, n_inp]) -> z [B, P, n_groups, embed_dim]      (inference; reference models/encoder_decoder.py:75-123)

    Device layout: rows m = snapshot * P + patch; fp32 residual stream [M, W], W = n_groups * embed_dim; matrix operands in the compute dtype.
    Attention heads narrower than 8 (the shipped cylinder model: W = 32, 8 heads) are zero-padded to 8 inside the packed q/k/v and
    projection weights — exact, the pad lanes contribute 0 to every score and every output."""

    CHUNK = 2048   # snapshots per pass (workspace ~ M * 4W act elements)

    def __init__(self, field_groups: Sequence[Sequence[int]], n_inp: int, MLP_hidden: int, num_layers: int, embed_dim: int, n_heads: int,
                 max_len: int, src_len: int, dropout: float = 0.1):
        super().__init__()
        self.field_groups = [list(g) for g in field_groups]
        self.num_groups = len(self.field_groups)
        self.n_inp, self.MLP_hidden, self.embed_dim, self.n_heads = n_inp, MLP_hidden, embed_dim, n_heads
        W = self.num_groups * embed_dim
        self.spatial_pos_encoder = PositionalEncoding(W, dropout)
        self.blocks = nn.ModuleList([EncoderBlock(n_heads=n_heads, max_len=max_len, embed_dim=W, src_len=src_len, dropout=dropout) for _ in range(num_layers)])
        self.ln = nn.LayerNorm(W)
        self.apply(self._init_weights)   # before the down-scale MLPs exist, as in the reference (:90-95): they keep torch's default init
        self.encoders = nn.ModuleList([downScaleMLP(d_input=n_inp * len(g), d_model=embed_dim, hidden_dim=MLP_hidden) for g in self.field_groups])
        self.compute_dtype = "fp32"
        self._pack = None
        for g in self.field_groups:
            if g != list(range(g[0], g[0] + len(g))):
                raise NotImplementedError("sea_amd.PointwiseEncode: a field group must be a run of consecutive field indices (column slice of the [M, F*C] input)")
        if W % n_heads or (W // n_heads) % 4 or W % 8 or MLP_hidden % 8 or embed_dim % 4:
            raise NotImplementedError("sea_amd.PointwiseEncode: need n_groups*embed_dim a multiple of 8 and of n_heads, head dim and embed_dim multiples of 4, "
                                      "MLP_hidden a multiple of 8")
        self._n_inp_p = (n_inp + 3) // 4 * 4   # a field's cell columns are padded to 16 bytes inside (zero weight columns: exact)
        if (W // n_heads) > 128:
            raise NotImplementedError("sea_amd.PointwiseEncode: head dim above 128")

    @staticmethod
    def _init_weights(module):
        if isinstance(module, nn.Linear):
            torch.nn.init.normal_(module.weight, mean=0.0, std=0.02)
            if module.bias is not None:
                torch.nn.init.zeros_(module.bias)
        elif isinstance(module, nn.LayerNorm):
            nn.init.constant_(module.bias, 0)
            nn.init.constant_(module.weight, 1.0)

    def set_compute_dtype(self, dtype) -> "PointwiseEncode":
        name = {torch.float32: "fp32", torch.bfloat16: "bf16"}.get(dtype, dtype)
        if name not in ("fp32", "bf16"):
            raise ValueError("compute dtype must be 'fp32' or 'bf16'")
        self.compute_dtype, self._pack = name, None
        return self

    # ------------------------------------------------------------------ packed weights (refreshed when a parameter was written or moved)
    def _packed(self, dt: torch.dtype, dev: torch.device):
        ps = list(self.parameters())
        key = (dt, dev, tuple((p.data_ptr(), p._version) for p in ps))
        if self._pack is not None and self._pack["key"] == key:
            return self._pack
        W, H = self.num_groups * self.embed_dim, self.n_heads
        hd = W // H
        hdp = min(v for v in (8, 16, 32, 64, 128) if v >= hd)   # the attention kernel's head dims; narrower heads are zero-padded (exact)
        Wp = H * hdp
        f32 = torch.float32
        with torch.no_grad():
            conv = lambda t: t.detach().to(device=dev, dtype=dt).contiguous()  # noqa: E731
            enc = []
            C, Cp = self.n_inp, self._n_inp_p
            for g, m in zip(self.field_groups, self.encoders):
                K = len(g) * Cp
                Kp = _round_up(K, 8)
                w1 = torch.zeros(self.MLP_hidden, Kp, device=dev, dtype=dt)
                w1[:, :K].view(self.MLP_hidden, len(g), Cp)[:, :, :C] = m.layer1.weight.detach().to(dt).view(self.MLP_hidden, len(g), C)
                enc.append(dict(K=K, Kp=Kp, col0=g[0] * Cp, W1=w1, W2=conv(m.layer2.weight), b2=m.layer2.bias.detach().to(dev, f32).contiguous()))

            def pad_rows(w):   # [H*hd, ...] -> [H*hdp, ...], head h at rows h*hdp .. h*hdp + hd - 1
                out = torch.zeros((H, hdp) + tuple(w.shape[1:]), device=dev, dtype=w.dtype)
                out[:, :hd] = w.detach().to(dev).view((H, hd) + tuple(w.shape[1:]))
                return out.view((Wp,) + tuple(w.shape[1:]))

            blocks = []
            for b in self.blocks:
                a = b.attn_1
                wqkv = torch.cat([pad_rows(a.q.weight), pad_rows(a.k.weight), pad_rows(a.v.weight)], 0).to(dt).contiguous()
                bqkv = torch.cat([pad_rows(a.q.bias), pad_rows(a.k.bias), pad_rows(a.v.bias)], 0).to(f32).contiguous()
                wo = pad_rows(a.projection.weight.detach().t().contiguous()).t().to(dt).contiguous()      # [W, Wp]: zero columns at the pad lanes
                fc1, ln, _, fc2 = b.mlp_1.layers
                blocks.append(dict(g1=b.ln_exp1_1.weight.detach().to(dev, f32), g2=b.ln_exp1_2.weight.detach().to(dev, f32), wqkv=wqkv, bqkv=bqkv, wo=wo,
                                   w1=conv(fc1.weight), b1=fc1.bias.detach().to(dev, f32), lnw=ln.weight.detach().to(dev, f32), lnb=ln.bias.detach().to(dev, f32),
                                   w2=conv(fc2.weight), b2=fc2.bias.detach().to(dev, f32)))
            fin_w, fin_b = self.ln.weight.detach().to(dev, f32).contiguous(), self.ln.bias.detach().to(dev, f32).contiguous()
        self._pack = dict(key=key, enc=enc, blocks=blocks, hd=hd, hdp=hdp, Wp=Wp, ws={}, fin_w=fin_w, fin_b=fin_b)
        return self._pack

    def _workspace(self, pk, Bc: int, P: int, dt: torch.dtype, dev: torch.device):
        ws = pk["ws"].get((Bc, P))
        if ws is not None:
            return ws
        W, H, hdp, Wp, S = self.num_groups * self.embed_dim, self.n_heads, pk["hdp"], pk["Wp"], 4 * self.num_groups * self.embed_dim
        M, cap = Bc * P, _round_up(P, 8)
        e = lambda *shape, dtype=dt: torch.empty(*shape, device=dev, dtype=dtype)  # noqa: E731
        z = lambda *shape, dtype=dt: torch.zeros(*shape, device=dev, dtype=dtype)  # noqa: E731
        rope = torch.zeros(cap, hdp // 2, 2, device=dev, dtype=torch.float32)
        rope[..., 0] = 1.0   # (cos, sin) = (1, 0): the projection kernel's rotation is the identity — this attention has no positional rotation
        ws = dict(A=[z(M, g["Kp"]) for g in pk["enc"]], hid=[e(M, self.MLP_hidden) for _ in pk["enc"]], zr=e(M, W, dtype=torch.float32), n=e(M, W),
                  Q=e(Bc, H, P, hdp), K=z(Bc, H, cap, hdp), Vt=z(Bc, H, hdp, cap), att=e(Bc, P, Wp), h=e(M, S), hg=e(M, S), rope=rope,
                  pe=self.spatial_pos_encoder.pe[0, :P].to(dev, torch.float32).repeat(Bc, 1).contiguous(), cap=cap)
        pk["ws"] = {(Bc, P): ws}   # one shape kept: a new chunk shape replaces it
        return ws

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        N.require_gpu(x, "PointwiseEncode input")
        if torch.is_grad_enabled() and x.requires_grad:
            raise NotImplementedError("sea_amd.PointwiseEncode: inference only")
        B, P, F, C = x.shape
        assert F == sum(len(g) for g in self.field_groups) and C == self.n_inp, (x.shape, self.field_groups, self.n_inp)
        if P > self.spatial_pos_encoder.pe.shape[1]:
            raise ValueError(f"{P} patches exceed the positional table ({self.spatial_pos_encoder.pe.shape[1]})")
        dt = torch.float32 if self.compute_dtype == "fp32" else torch.bfloat16
        dev = x.device
        pk = self._packed(dt, dev)
        W, G, H, hdp = self.num_groups * self.embed_dim, self.num_groups, self.n_heads, pk["hdp"]
        xf = x.detach().to(torch.float32)
        if self._n_inp_p != C:   # pad each field's cell columns to 16 bytes (one copy; sea_patchify can write this layout directly: c_out)
            xf = torch.nn.functional.pad(xf, (0, self._n_inp_p - C))
        xf = xf.contiguous().view(B * P, F * self._n_inp_p)
        out = torch.empty(B * P, W, device=dev, dtype=torch.float32)
        x_is_act = dt != torch.float32
        for b0 in range(0, B, self.CHUNK):
            Bc = min(self.CHUNK, B - b0)
            M = Bc * P
            ws = self._workspace(pk, Bc, P, dt, dev)
            rows = slice(b0 * P, b0 * P + M)
            # down-scale MLPs of all groups: (compute-dtype copy of the group's columns) -> Linear + GELU -> Linear + bias + positions
            for g, A in zip(pk["enc"], ws["A"]):
                ops.convert(xf[rows, g["col0"]:g["col0"] + g["K"]], A[:, :g["K"]])
            ops.gemm_grouped([dict(A=A, W=g["W1"], Cact=hid, act=1) for g, A, hid in zip(pk["enc"], ws["A"], ws["hid"])], dt)
            E = self.embed_dim
            ops.gemm_grouped([dict(A=hid, W=g["W2"], bias=g["b2"], R=ws["pe"][:, i * E:(i + 1) * E], C32=ws["zr"][:, i * E:(i + 1) * E])
                              for i, (g, hid) in enumerate(zip(pk["enc"], ws["hid"]))], dt)
            zr = ws["zr"]
            for blk in pk["blocks"]:
                ops.rownorm([dict(X=zr, gamma=blk["g1"], Yact=ws["n"])], M, W, False, False, 1e-5, dt)
                ops.qkv_rope_grouped([dict(A=ws["n"], W=blk["wqkv"], bias=blk["bqkv"], col0=0, Q=ws["Q"], K=ws["K"], Vt=ws["Vt"])], ws["rope"], H, hdp, P, 0,
                                     ws["cap"], ops.q_scale(pk["hd"]), dt)
                ops.attention_fwd([dict(Q=ws["Q"], K=ws["K"], Vt=ws["Vt"], O=ws["att"])], Bc, H, hdp, P, P, ws["cap"], 0, P, dt)   # src_len = P: every key visible
                ops.gemm_grouped([dict(A=ws["att"].view(M, -1), W=blk["wo"], R=zr, C32=zr)], dt)
                ops.rownorm([dict(X=zr, gamma=blk["g2"], Yact=ws["n"])], M, W, False, False, 1e-5, dt)
                ops.gemm_grouped([dict(A=ws["n"], W=blk["w1"], bias=blk["b1"], Cact=ws["h"])], dt)
                ops.rownorm([dict(X=ws["h"], gamma=blk["lnw"], beta=blk["lnb"], Yact=ws["hg"])], M, ws["h"].shape[1], x_is_act, True, 1e-5, dt)
                ops.gemm_grouped([dict(A=ws["hg"], W=blk["w2"], bias=blk["b2"], R=zr, C32=zr)], dt)
            ops.rownorm([dict(X=zr, gamma=pk["fin_w"], beta=pk["fin_b"], Y32=out[rows])], M, W, False, False, self.ln.eps, dt)
        return out.view(B, P, G, self.embed_dim)


class SpatialModel(nn.Module):
    """SpatialModel(field_groups, n_inp, MLP_hidden, num_layers, embed_dim, n_heads, max_len, src_len, dropout=0.1, variational=False): encoder +
    decoder under the reference's attribute names `encode` / `decode` (models/encoder_decoder.py:148-176); the variational encoder
    (`Encode`, sampling) is not provided.

    In train() mode with grad enabled (and parameters requiring grad) forward() is the training forward of sea_amd/spatial_train.py: `loss.backward()` fills
    p.grad of every parameter (gradients accumulate until zero_grad()), and initialize_optimizer returns the fused AdamW over the flat parameter
    buffer the engine keeps.  Under torch.no_grad() or in eval() mode forward() runs the inference launches of PointwiseEncode.forward / Decode.forward."""

    def __init__(self, field_groups, n_inp, MLP_hidden, num_layers, embed_dim, n_heads, max_len, src_len, dropout=0.1, variational=False):
        super().__init__()
        if variational:
            raise NotImplementedError("sea_amd.SpatialModel: the variational encoder is outside the accelerated path (both shipped configs use variational=False)")
        self.variational = False
        self.dropout_p = float(dropout)
        self.encode = PointwiseEncode(field_groups, n_inp, MLP_hidden, num_layers, embed_dim, n_heads, max_len, src_len, dropout)
        self.decode = Decode(field_groups, n_inp, MLP_hidden, embed_dim, dropout)
        object.__setattr__(self, "_engine", None)

    def set_compute_dtype(self, dtype) -> "SpatialModel":
        self.encode.set_compute_dtype(dtype)
        self.decode.set_compute_dtype(dtype)
        return self

    def generate_padding_mask(self, x, pad_idx=-9999):
        """In place, as the reference (:171-174): entries equal to pad_idx become 0."""
        x[x == pad_idx] = 0.0
        return x

    # ------------------------------------------------------------------ training (sea_amd/spatial_train.py)
    def _apply(self, fn, *args, **kwargs):
        # .to()/.cuda()/.cpu() re-create parameter storage: drop the engine (and its flat buffers); it is rebuilt lazily
        object.__setattr__(self, "_engine", None)
        return super()._apply(fn, *args, **kwargs)

    def engine(self, device: Optional[torch.device] = None):
        from ..spatial_train import SpatialEngine

        if self._engine is None:
            dev = device if device is not None else next(self.parameters()).device
            if dev.type != "cuda":
                raise RuntimeError("sea_amd.SpatialModel: parameters are on the CPU; training runs on the MI355X only (model.to('cuda'))")
            object.__setattr__(self, "_engine", SpatialEngine(self, dev))
        return self._engine

    def _grad_anchor(self) -> torch.Tensor:
        """A leaf that requires grad, so that autograd calls the hand-written backward."""
        a = getattr(self, "_anchor", None)
        if a is None or a.device != next(self.parameters()).device:
            a = torch.zeros(1, device=next(self.parameters()).device, requires_grad=True)
            object.__setattr__(self, "_anchor", a)
        return a

    def _live_params(self):
        eng = self._engine
        cache = getattr(self, "_live_cache", None)
        if cache is None or cache[0] is not eng:
            named = dict(self.named_parameters())
            cache = (eng, [named[n] for n in eng.params.live_names])
            object.__setattr__(self, "_live_cache", cache)
        return cache[1]

    def forward(self, x):
        x = self.generate_padding_mask(x)
        if self.training and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            if self.dropout_p > 0.0:
                raise NotImplementedError(f"sea_amd.SpatialModel: training with dropout {self.dropout_p} is not implemented (the shipped spatial configs "
                                          "use dropout 0.0)")
            N.require_gpu(x, "SpatialModel input")
            from ..spatial_train import spatial_forward_with_grad

            return spatial_forward_with_grad(self, self.engine(x.device), x)
        return self.decode(self.encode(x))
