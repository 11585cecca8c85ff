"""RenderFormer on MI355X: the two-stage transformer driven through librfhip.

Public surface mirrors the reference ``RenderFormer`` (renderformer/models/
renderformer.py:13-206): ``RenderFormer(config)``, ``from_pretrained``,
``load_state_dict``/``state_dict``, ``to``/``eval``/``device`` and
``forward(tri_vpos_list, texture_patch_list, valid_mask, vns, rays_o, rays_d,
tri_vpos_view_tf, tf32_view_tf=False)``.

Execution model: every scene is *unpadded* into a packed token
matrix — stage 1 holds ``16 + n_b`` rows per scene (register tokens then the
valid triangles), stage 2 ``R = (H/8) (W/8)`` ray-token rows per (scene, view) of an H x W frame.
All GEMMs run over the packed rows of the whole batch at once; attention
kernels receive per-problem row ranges.  The residual streams are fp32; the
projection GEMMs take fp16 operands (RMSNorm / SwiGLU / attention outputs and
weights; ``operands="bf16"`` selects bf16), attention q/k/v are bf16 with an fp32
softmax, and the DPT convolutions take fp16 operands with fp32 accumulation.
fp16 operands are range-checked on the device (every fp16 writer raises a word of the
frame's own on |x| > 65504; ``range_check``): a frame that overflowed is rendered again
with bf16 operands (bf16x3 DPT planes), or reported as a DeviceError in the deferred mode.
The default ("sync") resolves a frame before ``render`` returns by waiting on that frame's end
event only (no device sync, like the caller's own ``.cpu()``), so a caller that never calls
``resolve`` — the reference README example, its ``infer.py`` — always reads the final frame.
Callers that pipeline frames opt in to "lazy" (read at a later render, ``resolve(out)`` or
``check_range()``: ``batch_infer.py``, ``infer.py``) or "deferred" (``bench.py``).  The range words, the pending
frames and the three modes are ``range_guard.RangeGuard``'s (``_guard``); changing operands (``_fall_back``) stays here.
"""
from __future__ import annotations

import math
import os
import threading
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from . import ops
from ._lib import load as _load_lib
from .config import RenderFormerConfig, named_config
from .dpt import PRECISIONS as DPT_PRECISIONS
from .dpt import DPTHead
from .range_guard import RangeGuard, deferred_error
from .weights import check_state_dict, load_snapshot, synthetic_state_dict

EPS = 1e-6  # layers/attention.py:16
FP8_PROJECTIONS = ("q", "out", "self_in", "self_out", "w13", "w2")  # stage-2 projections the fp8 mode can take
# the subset it takes by default: the two whose MX fp8 error keeps the render inside the 1e-3 bar (measured per
# projection on the reference fixtures, profiles/r3_fp8_study.log: q 2.8e-4, w2 6.6e-4 on the bf16 base's 2.7e-4;
# out 1.8e-3, self_in 2.3e-3, self_out 3.1e-3, w13 1.0e-3, all six 3.2e-3)
FP8_DEFAULT = ("q", "w2")
SWIN_WINDOW, SWIN_SHIFT = 8, 4  # attention.py:604-605


def _bf16(t, device):
    return t.to(device=device, dtype=torch.bfloat16).contiguous()


def _f32(t, device):
    return t.to(device=device, dtype=torch.float32).contiguous()


OPERANDS = {"f16": torch.float16, "bf16": torch.bfloat16}  # 16-bit MFMA operand formats of the projections


def _interleave_swiglu(w1: torch.Tensor, w3: torch.Tensor) -> torch.Tensor:
    """[F, D] x2 -> [2F, D] in 16-row groups (w1 block g, w3 block g) for the SwiGLU GEMM epilogue."""
    f, d = w1.shape
    return torch.stack([w1.view(f // 16, 16, d), w3.view(f // 16, 16, d)], dim=1).reshape(2 * f, d)


class _Layer:
    pass


class _DeviceWeights:
    """Weights packed for the kernels: bf16 GEMM operands, fp32 norms/biases/tokens."""

    def __init__(self, cfg: RenderFormerConfig, sd: Dict[str, torch.Tensor], device, dpt_precision: str = "f16",
                 operands: str = "f16"):
        d = cfg.latent_dim
        # projection GEMM operands (weights, and the activations that feed them: RMSNorm outputs, attention
        # outputs, SwiGLU outputs): fp16 by default; q/k/v of the attention kernels stay bf16
        self.half = OPERANDS[operands]
        hw = lambda t: t.to(device=device, dtype=self.half).contiguous()  # noqa: E731
        self.tri_token = _f32(sd["tri_token"].reshape(-1), device)
        self.reg_tokens = _f32(sd["reg_tokens"].reshape(cfg.num_register_tokens, d), device)
        vn_w = sd["vn_encoding_proj.weight"]
        self.vn_k = ((vn_w.shape[1] + 63) // 64) * 64
        self.vn_w = hw(torch.nn.functional.pad(vn_w, (0, self.vn_k - vn_w.shape[1])))
        self.vn_b = _f32(sd["vn_encoding_proj.bias"], device)
        self.vn_norm = _f32(sd["vn_encoder_norm.weight"], device)
        self.tex_w = _bf16(sd["texture_encoder.weight"], device)
        self.tex_b = _f32(sd["texture_encoder.bias"], device)
        # texture fast path (prologue.hip rf_texture_scan): the encoder weights summed over the to_h5 patch
        # mask {(i, j): i + j <= 32} per channel, [C, D] f32 (from the f32 checkpoint weights, in f64)
        tw = sd["texture_encoder.weight"]
        self.tex_wsum = None
        if cfg.texture_encode_patch_size == 32 and tw.shape[1] == cfg.texture_channels * 1024:
            i, j = torch.meshgrid(torch.arange(32), torch.arange(32), indexing="ij")
            mask = (i + j <= 32).double().reshape(1, 1, 1024)
            ws = (tw.detach().double().reshape(d, cfg.texture_channels, 1024) * mask).sum(-1)
            self.tex_wsum = _f32(ws.t(), device)
        # texture fast-path flags by frame parity: frame i raises tex_flags[i % 2] and its scan clears the other
        # one for frame i + 1 (no reset launch in the frame; rf_texture_scan2)
        self.tex_flags = torch.zeros(2, dtype=torch.int32, device=device)
        # the flag word of compact [B, N, C] textures (ops.texture_rows): never raised, and apart from the parity
        # pair above, so compact and expanded frames alternate on one model in any order
        self.tex_rows_flag = torch.zeros(1, dtype=torch.int32, device=device)
        # identity camera transforms per view count (read-only; built on the host and copied synchronously, so a
        # render on another stream never sees it half-written): no fill kernels between stage 1 and stage 2
        self.eyes: Dict[int, torch.Tensor] = {}
        self.tex_parity = 0
        self.tex_norm = _f32(sd["texture_encoder_norm.weight"], device)
        self.enc_freqs = _f32(sd["transformer.rope_emb.freqs"], device)
        # stage 1's positional encoding fused into the QK path (rf.h ABI 16; RF_QK_FUSE=0 restores the q/k norm +
        # RoPE row kernel): the q and k rows of every in-projection (and their norm weights) are stored in
        # ops.rope_pair_perm order, so the projection's epilogue holds each rotate-half pair in one lane
        self.qk_fused = os.environ.get("RF_QK_FUSE", "1") != "0"
        D = cfg.latent_dim
        perm = ops.rope_pair_perm(D)
        qk_perm = torch.cat([perm, perm + D, torch.arange(2 * D, 3 * D)]) if self.qk_fused else None
        self.enc = []
        for i in range(cfg.num_layers):
            p = f"transformer.layers.{i}."
            L = _Layer()
            w_in = sd[p + "multihead_attn.in_proj.weight"]
            qn = torch.cat([sd[p + "multihead_attn.q_norm.weight"], sd[p + "multihead_attn.k_norm.weight"]])
            if self.qk_fused:
                w_in, qn = w_in[qk_perm], qn[qk_perm[:2 * D]]
            L.w_in = hw(w_in)
            L.w_out = hw(sd[p + "multihead_attn.out_proj.weight"])
            L.qk_norm = _f32(qn, device)
            L.query_norm = _f32(sd[p + "query_norm.weight"], device)
            L.w13 = hw(_interleave_swiglu(sd[p + "ffn.w1.weight"], sd[p + "ffn.w3.weight"]))
            L.w2 = hw(sd[p + "ffn.w2.weight"])
            L.ffn_norm = _f32(sd[p + "ffn_norm.weight"], device)
            self.enc.append(L)
        vt = "view_transformer."
        self.patch_token = _f32(sd[vt + "ray_map_patch_token"].reshape(-1), device)
        self.ray_w = hw(sd[vt + "ray_map_encoder.weight"])
        self.ray_b = _f32(sd[vt + "ray_map_encoder.bias"], device)
        self.ray_norm = _f32(sd[vt + "ray_map_encoder_norm.weight"], device)
        self.dec_freqs = _f32(sd[vt + "transformer.rope_emb.freqs"], device)
        dperm = ops.rope_pair_perm(cfg.view_transformer_latent_dim)
        qk_rows = (lambda t: t[dperm]) if self.qk_fused else (lambda t: t)  # noqa: E731
        self.dec = []
        for i in range(cfg.view_transformer_n_layers):
            p = f"{vt}transformer.layers.{i}."
            a = p + "multihead_attn."
            L = _Layer()
            # (qk_fused: the cross-attention q and k rows in rope_pair_perm order, as stage 1's)
            L.wq = hw(qk_rows(sd[a + "q_proj.weight"]))
            L.wkv = hw(torch.cat([qk_rows(sd[a + "k_proj.weight"]), sd[a + "v_proj.weight"]], 0))
            L.wo = hw(sd[a + "out_proj.weight"])
            L.q_norm = _f32(qk_rows(sd[a + "q_norm.weight"]), device)
            L.k_norm = _f32(qk_rows(sd[a + "k_norm.weight"]), device)
            L.query_norm = _f32(sd[p + "query_norm.weight"], device)
            L.kv_norm = _f32(sd[p + "kv_norm.weight"], device)
            if cfg.view_transformer_include_self_attn:
                s = p + "self_attn."
                L.ws_in = hw(sd[s + "in_proj.weight"])
                L.ws_out = hw(sd[s + "out_proj.weight"])
                L.sqk_norm = _f32(torch.cat([sd[s + "q_norm.weight"], sd[s + "k_norm.weight"]]), device)
                L.self_norm = _f32(sd[p + "self_attn_norm.weight"], device)
            L.w13 = hw(_interleave_swiglu(sd[p + "ffn.w1.weight"], sd[p + "ffn.w3.weight"]))
            L.w2 = hw(sd[p + "ffn.w2.weight"])
            L.ffn_norm = _f32(sd[p + "ffn_norm.weight"], device)
            self.dec.append(L)
        # Cross-attention K/V of every decoder layer in ONE GEMM (their input, the stage-1 output, is the same
        # for all layers): RMSNorm(ctx) W^T = (ctx * inv_rms) (W diag(g))^T, so each layer's kv_norm weight g
        # is folded into its K/V rows (in f32, then rounded to bf16) and ctx is normalised once with unit
        # weights; layer i reads columns [2D i, 2D (i+1)) of the [T1, L*2D] result.
        wkv_all = []
        for i in range(cfg.view_transformer_n_layers):
            p = f"{vt}transformer.layers.{i}."
            a = p + "multihead_attn."
            w = torch.cat([qk_rows(sd[a + "k_proj.weight"]), sd[a + "v_proj.weight"]], 0).float()
            wkv_all.append(w * sd[p + "kv_norm.weight"].float()[None, :])
        self.wkv_all = hw(torch.cat(wkv_all, 0))
        # every layer's k_norm weight, for the one-launch key rotation of all layers (ops.qk_norm_rope_groups)
        self.k_norm_all = _f32(torch.cat([qk_rows(sd[f"{vt}transformer.layers.{i}.multihead_attn.k_norm.weight"])
                                          for i in range(cfg.view_transformer_n_layers)]), device)
        self.ctx_unit = torch.ones(self.wkv_all.shape[1], dtype=torch.float32, device=device)
        self.dpt = DPTHead(sd, vt + "out_dpt", device, precision=dpt_precision)
        self.fp8_ready = False

    @property
    def tex_flag(self) -> torch.Tensor:
        """The texture fast-path flag of the most recent frame (1: the scan rejected the fast path)."""
        return self.tex_flags[1 - self.tex_parity:2 - self.tex_parity]

    def make_fp8(self):
        """MX fp8 copies (e4m3 + E8M0 per 32 K-elements, ops.mx8_quant_ref) of the stage-2 projection weights:
        q_proj, self-attention in/out, cross out_proj, SwiGLU w1/w3 (interleaved) and w2."""
        if self.fp8_ready:
            return
        q = lambda w: ops.MX8(*ops.mx8_quant_ref(w))  # noqa: E731
        for L in self.dec:
            L.wq8, L.wo8, L.w13_8, L.w2_8 = q(L.wq), q(L.wo), q(L.w13), q(L.w2)
            if hasattr(L, "ws_in"):
                L.ws_in8, L.ws_out8 = q(L.ws_in), q(L.ws_out)
        self.fp8_ready = True


@dataclass
class _Plan:
    """Packed-row bookkeeping for one batch (built once per mask pattern / view count / resolution)."""
    B: int
    V: int
    H: int                     # frame height and width in pixels (hp x wp patches)
    W: int
    counts: List[int]
    T_tri: int
    T1: int
    T_kv: int
    R: int
    hp: int
    wp: int
    max_s: int
    valid_flat: torch.Tensor   # int32 [T_tri] rows into [B*N]
    dst_row: torch.Tensor      # int32 [B*N] -> packed triangle index or -1
    tri_rows: torch.Tensor     # int32 [T_tri] -> stage-1 row
    reg_rows: torch.Tensor     # int32 [16 B]
    scene_off: torch.Tensor    # int32 [B+1] into valid_flat
    cu1: torch.Tensor          # int32 [B+1] stage-1 row offsets
    kv_off: torch.Tensor       # int32 [P+1] per-view K row offsets
    kv_src_rows: torch.Tensor  # int32 [T_kv] -> stage-1 row
    prob1: torch.Tensor        # int32 [B, 5]
    prob2: torch.Tensor        # int32 [P, 5]
    prob_self: torch.Tensor    # int32 [P, 5]
    sched1: Optional[torch.Tensor] = None      # int64 [grid + 1] stream-K ranges of prob1 (ops.attn_schedule)
    sched2: Optional[torch.Tensor] = None      # ... of prob2
    view_valid: Optional[torch.Tensor] = None  # for forward(): valid rows into [P*N]
    view_off: Optional[torch.Tensor] = None


def frame_size(cfg: RenderFormerConfig, resolution) -> Tuple[int, int]:
    """``resolution`` (an int r = the square (r, r), or (height, width)) as (H, W), checked per side: each must be
    a positive multiple of the patch size (times the Swin window when the view transformer uses Swin attention)."""
    H, W = ops.frame_hw(resolution)
    unit = cfg.patch_size * (SWIN_WINDOW if cfg.view_transformer_use_swin_attn else 1)
    for side, n in (("height", H), ("width", W)):
        if n <= 0 or n % unit != 0:
            raise ValueError(f"resolution {H} x {W}: {side} {n} incompatible with patch/window size (must be a "
                             f"positive multiple of {unit})")
    return H, W


def frame_layout(cfg: RenderFormerConfig, resolution, overscan: bool = False) -> Tuple[int, int, int, int, int, int]:
    """``(H, W, Hp, Wp, y0, x0)``: the requested frame H x W, the frame Hp x Wp the model renders (what the plan, the
    ray tokens and the DPT see) and where the requested frame sits inside it.

    Without ``overscan`` this is ``frame_size`` plus zeros: Hp = H, Wp = W, and a side that is no multiple of the
    frame unit u (the patch size, times the Swin window with Swin attention: 64 for the released models) raises.
    With ``overscan`` any positive H x W is taken: Hp = ceil(H / u) u, Wp = ceil(W / u) u, and the requested frame is
    centred, y0 = (Hp - H) // 2, x0 = (Wp - W) // 2 (1080 -> 1088 rows, y0 = 4).  A frame whose sides are multiples
    of u already gives what it gives without ``overscan``."""
    if not overscan:
        H, W = frame_size(cfg, resolution)
        return H, W, H, W, 0, 0
    H, W = ops.frame_hw(resolution)
    unit = cfg.patch_size * (SWIN_WINDOW if cfg.view_transformer_use_swin_attn else 1)
    for side, n in (("height", H), ("width", W)):
        if n <= 0:
            raise ValueError(f"resolution {H} x {W}: {side} {n} must be positive")
    Hp, Wp = -(-H // unit) * unit, -(-W // unit) * unit
    return H, W, Hp, Wp, (Hp - H) // 2, (Wp - W) // 2


def _check_camera(c2w, fov, intrinsics):
    """Exactly one of ``fov`` and ``intrinsics``; intrinsics float32 [B, V, 4] (values are not read back: a
    non-positive focal length is the caller's error)."""
    if (fov is None) == (intrinsics is None):
        raise ValueError("pass exactly one of fov and intrinsics" +
                         (" (fov may be None only with intrinsics=)" if fov is None else " (got both)"))
    if intrinsics is None:
        return
    if not isinstance(intrinsics, torch.Tensor) or intrinsics.dtype != torch.float32:
        raise ValueError("intrinsics must be a float32 tensor [B, V, 4] = (fx, fy, cx, cy) in pixels, got "
                         f"{getattr(intrinsics, 'dtype', type(intrinsics))}")
    want = tuple(c2w.shape[:2]) + (4,) if isinstance(c2w, torch.Tensor) and c2w.dim() == 4 else None
    if intrinsics.dim() != 3 or intrinsics.shape[-1] != 4 or (want is not None and tuple(intrinsics.shape) != want):
        raise ValueError(f"intrinsics must be [B, V, 4] = (fx, fy, cx, cy) per camera"
                         f"{'' if want is None else f', here {list(want)}'}, got {list(intrinsics.shape)}")


def _build_plan(mask_host, V: int, res, patch: int, n_reg: int, device, n_heads: int = 0) -> _Plan:
    """The plan of an H x W frame (``res``: (H, W), or an int for a square) from a HOST copy of the mask (numpy bool
    [B, N]): every index table is built with numpy and reaches
    the device in ONE pinned, non-blocking copy (plus one for the two stream-K range tables), so building a plan
    never waits for the device (the frames queued before it keep running).  Only a device-only mask needs a
    read-back first (RenderFormer._plan: like flash_attn's unpad_input)."""
    import numpy as np
    m = np.asarray(mask_host, dtype=bool)
    B, N = m.shape
    counts = [int(c) for c in m.sum(axis=1)]
    valid_flat = np.flatnonzero(m.reshape(-1)).astype(np.int32)
    T_tri = int(valid_flat.size)
    dst_row = np.full(B * N, -1, dtype=np.int32)
    dst_row[valid_flat] = np.arange(T_tri, dtype=np.int32)
    S = [n_reg + c for c in counts]
    cu1 = np.concatenate([[0], np.cumsum(S)]).astype(np.int64)
    tri_rows = np.concatenate([np.arange(cu1[b] + n_reg, cu1[b + 1]) for b in range(B)] or [np.zeros(0)])
    reg_rows = np.concatenate([np.arange(cu1[b], cu1[b] + n_reg) for b in range(B)] or [np.zeros(0)])
    prob1 = [[int(cu1[b]), S[b], int(cu1[b]), S[b], int(cu1[b])] for b in range(B)]
    scene_off = np.concatenate([[0], np.cumsum(counts)])
    H, W = ops.frame_hw(res)
    hp, wp = H // patch, W // patch
    R = hp * wp
    P = B * V
    kv_off, kv_src, prob2, prob_self = [0], [], [], []
    for p in range(P):
        b = p // V
        kv_src.append(np.arange(cu1[b], cu1[b + 1]))
        prob2.append([p * R, R, kv_off[-1], S[b], int(cu1[b])])
        prob_self.append([p * R, R, p * R, R, p * R])
        kv_off.append(kv_off[-1] + S[b])
    parts = {"valid_flat": valid_flat, "dst_row": dst_row, "tri_rows": tri_rows, "reg_rows": reg_rows,
             "scene_off": scene_off, "cu1": cu1, "kv_off": np.asarray(kv_off),
             "kv_src_rows": np.concatenate(kv_src) if kv_src else np.zeros(0), "prob1": np.asarray(prob1).reshape(-1),
             "prob2": np.asarray(prob2).reshape(-1), "prob_self": np.asarray(prob_self).reshape(-1)}
    offs, o = {}, 0
    for k, a in parts.items():
        offs[k] = (o, int(a.size))
        o += int(a.size)
    buf = np.empty(max(o, 1), dtype=np.int32)
    for k, a in parts.items():
        buf[offs[k][0]:offs[k][0] + offs[k][1]] = a
    dbuf = torch.from_numpy(buf)
    if torch.device(device).type == "cuda":  # (a host plan, device "cpu", only lays the tables out: the CPU tests)
        dbuf = dbuf.pin_memory().to(device, non_blocking=True)
    t = {k: dbuf[a:a + n] for k, (a, n) in offs.items()}
    sched1 = sched2 = None
    if n_heads and ops.attn_schedule_enabled():
        grid = ops.attn_grid(device)
        sc = np.concatenate([ops.attn_schedule_host(prob1, n_heads, grid), ops.attn_schedule_host(prob2, n_heads, grid)])
        dsc = torch.from_numpy(sc).pin_memory().to(device, non_blocking=True)
        sched1, sched2 = dsc[:grid + 1], dsc[grid + 1:]
    return _Plan(B=B, V=V, H=H, W=W, counts=counts, T_tri=T_tri, T1=int(cu1[-1]), T_kv=kv_off[-1], R=R, hp=hp, wp=wp,
                 max_s=max(S), valid_flat=t["valid_flat"], dst_row=t["dst_row"], tri_rows=t["tri_rows"],
                 reg_rows=t["reg_rows"], scene_off=t["scene_off"], cu1=t["cu1"], kv_off=t["kv_off"],
                 kv_src_rows=t["kv_src_rows"], prob1=t["prob1"].view(-1, 5), prob2=t["prob2"].view(-1, 5),
                 prob_self=t["prob_self"].view(-1, 5), sched1=sched1, sched2=sched2)


class PrecisionWarning(UserWarning):
    pass


RANGE_CHECKS = ("lazy", "sync", "deferred", "off")


class EncodedScene:
    """The camera-independent state of a batch of scenes (RenderFormer.encode_scene): the stage-1 output ``x1``
    [T1, D] f32, every decoder layer's K/V ``kv_all`` [T1, n_layers * 2 * Dv] bf16 (None when the batched K/V form
    is off: RF_KV_BATCH=0 or above 4 GiB) and the packed triangles ``tris``.  ``render_encoded`` renders any number
    of cameras from it without running stage 1 or the K/V GEMM again.  It costs ``nbytes`` of device memory
    (T1 * (4 * D + n_layers * 4 * Dv)) plus the retained inputs.

    The handle also keeps a host copy of the mask (plans for any view count / resolution are built with no device
    read-back), the input tensors (texture already log-encoded) to encode again after an fp16 fallback, the
    ``precision`` = (operands, dpt_precision) and the weights object it was computed with, and the stream and end
    event of the encode.  It belongs to one model on one device; ``lock`` serialises a re-encode."""
    __slots__ = ("x1", "kv_all", "tris", "mask_host", "inputs", "versions", "precision", "weights", "model",
                 "generation", "device", "stream", "event", "lock")

    def __init__(self, model, generation, device, mask_host, inputs):
        self.model, self.generation, self.device = model, generation, device
        self.mask_host, self.inputs = mask_host, inputs
        self.versions = [t._version for t in inputs]
        self.x1 = self.kv_all = self.tris = self.precision = self.weights = self.stream = self.event = None
        self.lock = threading.RLock()

    @property
    def batch_size(self) -> int:
        return int(self.mask_host.shape[0])

    @property
    def nbytes(self) -> int:
        """Device bytes of the kept state: x1 plus kv_all."""
        return sum(t.numel() * t.element_size() for t in (self.x1, self.kv_all) if t is not None)


def _hf_cache_snapshot(model_id: str) -> Optional[str]:
    """Newest snapshot directory of a hub model id in the local Hugging Face cache that holds config.json and
    model.safetensors (the files PyTorchModelHubMixin downloads), or None."""
    if "/" not in model_id:
        return None
    roots = [os.environ.get("HF_HUB_CACHE"), os.environ.get("HUGGINGFACE_HUB_CACHE"),
             os.path.join(os.environ["HF_HOME"], "hub") if os.environ.get("HF_HOME") else None,
             os.path.join(os.path.expanduser("~"), ".cache", "huggingface", "hub")]
    name = "models--" + model_id.replace("/", "--")
    for root in roots:
        base = os.path.join(root, name, "snapshots") if root else None
        if not base or not os.path.isdir(base):
            continue
        snaps = sorted((os.path.join(base, d) for d in os.listdir(base)), key=os.path.getmtime, reverse=True)
        for d in snaps:
            if os.path.exists(os.path.join(d, "config.json")) and os.path.exists(os.path.join(d, "model.safetensors")):
                return d
    return None


class RenderFormer:
    """Drop-in for renderformer.models.renderformer.RenderFormer (inference only)."""

    def __init__(self, config: RenderFormerConfig, state_dict: Optional[Dict[str, torch.Tensor]] = None,
                 seed: int = 0, dpt_precision: Optional[str] = None, fp8: Optional[bool] = None,
                 view_chunk: Optional[int] = None, operands: Optional[str] = None,
                 range_check: Optional[str] = None):
        self.config = config
        # fp16 range check (RF_RANGE_CHECK).  Every render binds a host-mapped word of its own (rf_range_word_bind)
        # that the fp16-writing kernels raise on |x| > 65504 (inf included): a checkpoint whose activations exceed
        # fp16's range.  Concurrent renders (streams, models, threads) never share a word.
        #   "sync" (default): render waits for its own frame's end event (no device sync) and, if the frame
        #     overflowed, renders it again with bf16 projection operands (code 1/2/4) and/or bf16x3 DPT planes
        #     (code 8) before returning; the model keeps them (PrecisionWarning).  Safe for callers that never call
        #     resolve (the reference's README example and infer.py).
        #   "lazy" (opt-in: batch_infer.py, infer.py): render returns without waiting; the word is read once the
        #     frame's end event has completed — at the start of a later render (non-blocking), in resolve(out) or
        #     check_range() (waiting) — and an overflowed frame is rendered again IN PLACE (same tensor and stream).
        #   "deferred": like lazy, but an overflow raises DeviceError (bench.py's timed loop).   "off": no check.
        # The range-word lists are guarded by a lock: renders of one model from several threads never share a word.
        self.range_check = range_check or os.environ.get("RF_RANGE_CHECK", "sync")
        if self.range_check not in RANGE_CHECKS:
            raise ValueError(f"range_check must be one of {RANGE_CHECKS}")
        self.range_fallbacks = 0  # frames rendered again with bf16 operands after an fp16 overflow
        self._guard = RangeGuard(self)  # the words, the frames whose word is unread, and the lock of both lists
        # render_views: stage 2 + DPT over at most view_chunk views per pass (stage 1 once per scene); None = all
        # views of the batch in one pass.  A fixed chunk makes each view's image independent of the batching.
        self.view_chunk = view_chunk if view_chunk is not None else (int(os.environ.get("RF_VIEW_CHUNK", "0")) or None)
        # fp8 mode (opt-in, RF_FP8=1 or fp8=True): stage-2 projections as MX fp8 GEMMs (rf_gemm_mx8) on activations
        # quantised per 32-element block.  Not config 5's path: the subset inside the 1e-3 bar (FP8_DEFAULT) buys no
        # frame time, and the full set misses the bar 3x
        self.fp8 = (os.environ.get("RF_FP8", "0") != "0") if fp8 is None else bool(fp8)
        # stage 1 as ONE library call (rf_encoder_forward: the same launches in the same order, so the same bits)
        # instead of 8 Python-issued calls per layer; RF_NATIVE_STAGES=0 issues them from Python
        self.native_stages = os.environ.get("RF_NATIVE_STAGES", "1") != "0"
        # which stage-2 projections the fp8 mode quantises (RF_FP8_PROJ, comma list of FP8_PROJECTIONS)
        self.fp8_projections = set(os.environ.get("RF_FP8_PROJ", ",".join(FP8_DEFAULT)).split(","))
        unknown = self.fp8_projections - set(FP8_PROJECTIONS)
        if unknown:
            raise ValueError(f"RF_FP8_PROJ: unknown projections {sorted(unknown)} (choose from {FP8_PROJECTIONS})")
        # DPT operand precision (dpt.py): "f16" (default) or "bf16x3"; RF_DPT_PRECISION overrides the default
        self.dpt_precision = dpt_precision or os.environ.get("RF_DPT_PRECISION", "f16")
        # 16-bit operands of the transformer projections (OPERANDS): fp16 by default (11-bit mantissa at the bf16
        # MFMA rate: ~7x less rounding error end to end, tools/precision_budget.py); "bf16" (RF_OPERANDS=bf16)
        # for checkpoints whose activations exceed fp16's range.  The fp8 mode quantises bf16 activations.
        self.operands = operands or os.environ.get("RF_OPERANDS", "bf16" if self.fp8 else "f16")
        if self.operands not in OPERANDS:
            raise ValueError(f"operands must be one of {tuple(OPERANDS)}")
        if self.fp8 and self.operands != "bf16":
            raise ValueError("the fp8 mode quantises bf16 activations: operands must be 'bf16'")
        if self.dpt_precision not in DPT_PRECISIONS:
            raise ValueError(f"dpt_precision must be one of {DPT_PRECISIONS}")
        cfg = config
        if cfg.latent_dim // cfg.num_heads != 128 or cfg.vt_head_dim != 128:
            raise ValueError("head_dim must be 128 (triangle RoPE constraint, rope.py:91-92)")
        if cfg.vdir_num_freqs != 0 or cfg.vdir_pe_type != "nerf":
            raise ValueError("only vdir_num_freqs=0 ray encoding is supported")
        self._sd = state_dict if state_dict is not None else synthetic_state_dict(cfg, seed)
        check_state_dict(cfg, self._sd, strict=state_dict is None)
        self._device = torch.device("cpu")
        # texture encoder fast path for to_h5-format textures (proven per call on the device; RF_TEX_FAST=0
        # forces the general pack + GEMM path)
        self._tex_fast = os.environ.get("RF_TEX_FAST", "1") != "0"
        # (id(mask), V, (H, W)) -> (mask object, mask version, plan): the no-read-back fast path for a mask tensor seen
        # before (bench.py c4 cycles 64 fixed device masks; a view-chunked render alternates two chunk sizes)
        self._last_plan: Dict = {}
        self._host_masks: Dict = {}  # id(device mask) -> (mask, version, host copy): plan_hint
        self._w: Optional[_DeviceWeights] = None
        self._generation = 0  # bumped by to() / load_state_dict: an EncodedScene made before either is refused
        self._plans: Dict = {}
        self._capture: Optional[dict] = None
        self.skip_token_num = cfg.num_register_tokens

    # ------------------------------------------------------------------ module-like API
    @classmethod
    def from_pretrained(cls, model_id: str, synthetic_seed: Optional[int] = None, dpt_precision: Optional[str] = None,
                        range_check: Optional[str] = None, **_):
        """PyTorchModelHubMixin.from_pretrained (renderformer.py:13) without the network: ``model_id`` is a local
        snapshot directory (config.json + model.safetensors), or a hub id ("microsoft/renderformer-v1.1-swin-
        large") found in the local Hugging Face cache; with ``synthetic_seed`` (or env RF_SYNTHETIC_SEED) a hub
        id or architecture name that is not cached gets deterministic random weights of that architecture."""
        snap = model_id if os.path.isdir(model_id) else _hf_cache_snapshot(model_id)
        if snap is not None:
            return cls(named_config(snap), load_snapshot(snap), dpt_precision=dpt_precision, range_check=range_check)
        if synthetic_seed is None and os.environ.get("RF_SYNTHETIC_SEED"):
            synthetic_seed = int(os.environ["RF_SYNTHETIC_SEED"])
        if synthetic_seed is None:
            raise FileNotFoundError(f"{model_id!r} is neither a local snapshot directory nor in the local Hugging Face "
                                    "cache (no network here); pass synthetic_seed= (or set RF_SYNTHETIC_SEED) for "
                                    "random-init weights of the named architecture")
        return cls(named_config(model_id), seed=synthetic_seed, dpt_precision=dpt_precision, range_check=range_check)

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        check_state_dict(self.config, sd, strict=strict)
        self._sd = {k: v.detach().float().cpu() for k, v in sd.items()}
        self._generation += 1
        if self._w is not None:
            with torch.cuda.device(self._device):
                self._w = _DeviceWeights(self.config, self._sd, self._device, self.dpt_precision, self.operands)
        return self

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return dict(self._sd)

    def eval(self):
        return self

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("renderformer_amd runs on HIP devices only (no CPU path)")
        _load_lib()
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self._device = device
        self._generation += 1
        with torch.cuda.device(device):
            self._w = _DeviceWeights(self.config, self._sd, device, self.dpt_precision, self.operands)
        return self

    cuda = lambda self, i=None: self.to("cuda" if i is None else f"cuda:{i}")  # noqa: E731

    @property
    def device(self):
        return self._device

    def parameters(self):
        return iter(self._sd.values())

    def _require(self):
        if self._w is None:
            raise RuntimeError("call .to('cuda') before running the model")
        _load_lib()

    def plan_hint(self, mask: torch.Tensor, mask_host) -> None:
        """Register the host copy of a device mask (batch_infer.py has it: it uploaded the batch), so the plan for a
        NEW mask pattern is built without reading the mask back (no device sync in front of the frame).  Valid for
        this mask object at its current version (an in-place edit invalidates it)."""
        if len(self._host_masks) > 64:
            self._host_masks.clear()
        self._host_masks[id(mask)] = (mask, mask._version, mask_host)

    def _plan(self, mask, V, res):
        # the same mask tensor object, unmodified since it was planned (torch's version counter): reuse that plan
        # without reading the mask back (the host sync stalls the queue at the start of every frame).  The
        # reference is held, so the object (and its storage) cannot be recycled under the same id.
        res = ops.frame_hw(res)
        ko = (id(mask), V, res)
        last = self._last_plan.get(ko)
        if last is not None and last[0] is mask and last[1] == mask._version:
            return last[2]
        plan = self._plan_host(self._mask_host(mask), V, res)  # (device-only mask: one read-back, like unpad_input)
        if len(self._last_plan) > 128:
            self._last_plan.clear()
        self._last_plan[ko] = (mask, mask._version, plan)
        return plan

    def _plan_host(self, host, V, res):
        """The plan of a host mask (numpy bool [B, N]) from the cache keyed by its pattern: no device read-back."""
        res = ops.frame_hw(res)
        key = (tuple(host.shape), host.tobytes(), V, res)
        plan = self._plans.get(key)
        if plan is None:
            if len(self._plans) > 64:
                self._plans.clear()
            plan = _build_plan(host, V, res, self.config.patch_size, self.config.num_register_tokens, self._device,
                               self.config.num_heads)
            self._plans[key] = plan
        return plan

    def _mask_host(self, mask):
        """Host copy of a device mask: the registered one (plan_hint) or one read-back."""
        import numpy as np
        hint = self._host_masks.get(id(mask))
        if hint is not None and hint[0] is mask and hint[1] == mask._version:
            return np.array(hint[2], dtype=bool)
        return mask.cpu().numpy().astype(bool)

    def capture_taps(self, enc_rows=None, dec_rows=None, dec_views=None) -> dict:
        """Arm a one-shot capture of intermediates for the NEXT render (parity tests at production size): the
        stage-1 output rows `enc_rows` of scene 0 (packed rows: 16 register tokens, then the valid triangles in
        order, = the reference's sequence) and their row norms, and for every decoder layer the ray-token rows
        `dec_rows` of views `dec_views` of scene 0.  Returns the dict the render fills (device fp32 tensors:
        'enc_rows' [n, D], 'enc_rownorm' [S], 'dec_rows' [layers, views, n, D])."""
        if self.view_chunk and any(int(v) >= int(self.view_chunk) for v in (dec_views or [])):
            # the capture is one-shot and filled by the first pass over the views (stage 2 runs per chunk)
            raise ValueError(f"capture_taps: dec_views must be < view_chunk ({self.view_chunk})")
        out: dict = {}
        dev = self._device
        as_idx = lambda x: None if x is None else torch.as_tensor(x, dtype=torch.long).to(dev)  # noqa: E731
        self._capture = {"enc": as_idx(enc_rows), "dec": as_idx(dec_rows), "views": list(dec_views or []),
                         "out": out}
        return out

    # ------------------------------------------------------------------ stages
    def _embed_triangles(self, plan: _Plan, texture: torch.Tensor, vns: torch.Tensor, log_encode: bool):
        cfg, W, dev = self.config, self._w, self._device
        D = cfg.latent_dim
        kt = cfg.texture_channels * cfg.texture_encode_patch_size ** 2
        log_ch = 3 if log_encode else 0
        tex_lin = torch.empty(plan.T_tri, D, dtype=torch.float32, device=dev)
        rows = cfg.texture_encode_patch_size != 1 and texture.dim() == 3
        if rows:
            # material rows [B, N, C]: one constant per triangle and channel, the form the scan below proves of an
            # expanded texture.  Nothing to prove here: the constants go straight to the C-wide product (no pack, no
            # K = C * 1024 GEMM), whatever RF_TEX_FAST says (it chooses between the two paths of expanded textures)
            if texture.shape[2] != cfg.texture_channels:
                raise ValueError(f"a [B, N, C] texture needs C = texture_channels = {cfg.texture_channels}, got "
                                 f"{tuple(texture.shape)}")
            if W.tex_wsum is None:
                raise ValueError("a [B, N, C] texture (one constant per triangle and channel) needs the mask-summed "
                                 f"encoder weights, which exist for texture_encode_patch_size 32 only (this model's is "
                                 f"{cfg.texture_encode_patch_size}): pass the expanded [B, N, C, p, p] texture")
            coef = torch.empty(max(plan.T_tri, 1), 16, dtype=torch.float32, device=dev)  # (no valid row: encode only)
            ops.texture_rows(texture, log_ch, plan.dst_row, coef)
            if plan.T_tri:
                ops.texture_linear(coef, W.tex_wsum, W.tex_b, tex_lin, W.tex_rows_flag)
        tex_in = None if rows else torch.empty(plan.T_tri, kt, dtype=torch.bfloat16, device=dev)
        fast = (not rows and self._tex_fast and plan.T_tri > 0 and W.tex_wsum is not None and texture.dim() == 5
                and tuple(texture.shape[2:]) == (cfg.texture_channels, 32, 32))
        if fast:
            # to_h5-format textures: one scan proves the per-channel-constant form and
            # the C-wide product replaces the K=13,312 GEMM; the general path below it runs only when the
            # scan's device flag says some row is not of that form
            coef = torch.empty(plan.T_tri, 16, dtype=torch.float32, device=dev)
            flag = W.tex_flags[W.tex_parity:W.tex_parity + 1]
            ops.texture_scan(texture, log_ch, plan.dst_row, coef, flag, W.tex_flags[1 - W.tex_parity:2 - W.tex_parity])
            W.tex_parity ^= 1
            ops.texture_linear(coef, W.tex_wsum, W.tex_b, tex_lin, flag)
            ops.texture_pack_if(flag, texture, 0, plan.dst_row, tex_in)
            ops.gemm(tex_in, W.tex_w, tex_lin, W.tex_b, ops.EPI_F32, flag=flag)
        elif not rows:
            ops.texture_pack(texture, log_ch, plan.dst_row, tex_in)
            if plan.T_tri:
                ops.gemm(tex_in, W.tex_w, tex_lin, W.tex_b, ops.EPI_F32)
        vn_in = torch.empty(plan.T_tri, W.vn_k, dtype=W.half, device=dev)
        ops.vn_encode(vns, plan.dst_row, cfg.vn_pe_num_freqs, vn_in)
        vn_lin = torch.empty(plan.T_tri, D, dtype=torch.float32, device=dev)
        if plan.T_tri:
            ops.gemm(vn_in, W.vn_w, vn_lin, W.vn_b, ops.EPI_F32)
        x = torch.empty(plan.T1, D, dtype=torch.float32, device=dev)
        ops.embed(x, plan.tri_rows, plan.T_tri, W.tri_token, 1, tex_lin, W.tex_norm, ops.FLT_EPS, vn_lin, W.vn_norm,
                  ops.FLT_EPS)
        ops.embed(x, plan.reg_rows, plan.B * cfg.num_register_tokens, W.reg_tokens, cfg.num_register_tokens)
        return x

    def _stage1(self, plan: _Plan, x: torch.Tensor, pos1: torch.Tensor):
        """TransformerEncoder (attention.py:579-590): pre-norm MHA with q/k norm + triangle RoPE, SwiGLU."""
        cfg, W, dev = self.config, self._w, self._device
        D, H, F = cfg.latent_dim, cfg.num_heads, cfg.dim_feedforward
        T = plan.T1
        if self._native_ok() and T > 0:
            if getattr(W, "enc_desc", None) is None:  # host array of the layers' device pointers, built once
                W.enc_desc = ops.encoder_layers(W.enc, cfg.view_indep_qk_norm)
            ops.encoder_forward(x, W.enc_desc, len(W.enc), H, F, W.half, EPS, pos1, W.enc_freqs, plan.prob1,
                                schedule=plan.sched1, tag="attn_stage1", qk_fused=W.qk_fused)
            self._capture_stage1(plan, x)
            return x
        h = torch.empty(T, D, dtype=W.half, device=dev)      # GEMM operands: W.half (fp16 by default)
        qkv = torch.empty(T, 3 * D, dtype=torch.bfloat16, device=dev)  # attention operands: bf16
        att = torch.empty(T, D, dtype=W.half, device=dev)
        g = torch.empty(T, F, dtype=W.half, device=dev)
        ss = torch.empty(T, ops.PRENORM_SLOTS, dtype=torch.float32, device=dev)
        q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
        qk_pair = qkv[:, :2 * D]
        # every pre-norm deferred (rf.h rf_gemm_add_prenorm / rf_gemm_rownorm), as rf_encoder_forward issues them:
        # h holds x * g, ss the row sums of squares, and the projection after the norm applies 1 / rms
        ops.prenorm(x, W.enc[0].query_norm, h, ss)
        qkn = cfg.view_indep_qk_norm
        qkss = torch.empty(T, 2, ops.PRENORM_SLOTS, dtype=torch.float32, device=dev) if W.qk_fused and qkn else None
        for li, L in enumerate(W.enc):
            if W.qk_fused:  # rf_encoder_forward's qk_fused sequence (stage.cpp), launch for launch
                ops.gemm_qk_rope(h, L.w_in, qkv, ss, EPS, D, 2, L.qk_norm if qkn else None, qkss, pos1, W.enc_freqs,
                                 q_scale=1.0 if qkn else ops.Q_LOG2_SCALE)
                if qkn:
                    ops.row_rms_scale(k, qkss[:, 1], EPS)
                    ops.attention(q, k, v, att, plan.prob1, plan.max_s, H, tag="attn_stage1", max_k_len=plan.max_s,
                                  schedule=plan.sched1, q_ss=qkss[:, 0], q_eps=EPS)
                else:
                    ops.attention(q, k, v, att, plan.prob1, plan.max_s, H, tag="attn_stage1", max_k_len=plan.max_s,
                                  q_prescaled=True, schedule=plan.sched1)
            else:
                ops.gemm_rownorm(h, L.w_in, qkv, ss, EPS)
                ops.qk_norm_rope(qk_pair, qk_pair, H, L.qk_norm if qkn else None, EPS, pos1, W.enc_freqs, n_seg=2,
                                 q_scale=ops.Q_LOG2_SCALE)
                ops.attention(q, k, v, att, plan.prob1, plan.max_s, H, tag="attn_stage1", max_k_len=plan.max_s,
                              q_prescaled=True, schedule=plan.sched1)
            ops.gemm_add_prenorm(att, L.w_out, x, L.ffn_norm, h, ss)
            ops.gemm_rownorm(h, L.w13, g, ss, EPS, ops.EPI_SWIGLU, tag="gemm_w13_stage1")
            if li + 1 < len(W.enc):
                ops.gemm_add_prenorm(g, L.w2, x, W.enc[li + 1].query_norm, h, ss)
            else:
                ops.gemm(g, L.w2, x, None, ops.EPI_ADD_F32)
        self._capture_stage1(plan, x)
        return x

    def _native_ok(self) -> bool:
        """Stages run as one library call each (rf_encoder_forward / rf_decoder_forward) unless RF_NATIVE_STAGES=0
        or the legacy split-KV attention is selected (RF_ATTN_SPLIT, a per-op diagnostic mode)."""
        return self.native_stages and int(os.environ.get("RF_ATTN_SPLIT", "0") or 0) == 0

    def _capture_stage1(self, plan: _Plan, x: torch.Tensor):
        cap = self._capture
        if cap is not None:  # (test capture, capture_taps): scene 0's rows of the stage-1 output
            s0 = self.config.num_register_tokens + plan.counts[0]
            cap["out"]["enc_rownorm"] = x[:s0].norm(dim=-1)
            if cap["enc"] is not None:
                cap["out"]["enc_rows"] = x.index_select(0, cap["enc"]).clone()

    def _kv_batch(self, T1: int) -> bool:
        """All decoder layers' K/V in one GEMM (see _DeviceWeights.wkv_all) unless RF_KV_BATCH=0 or it would exceed
        4 GiB."""
        cfg = self.config
        return (os.environ.get("RF_KV_BATCH", "1") != "0"
                and T1 * cfg.view_transformer_n_layers * 2 * cfg.view_transformer_latent_dim * 2 <= (4 << 30))

    def _stage2(self, plan: _Plan, x: torch.Tensor, ctx: torch.Tensor, pos2: torch.Tensor, ray_pos: torch.Tensor,
                kv_all: Optional[torch.Tensor] = None):
        """TransformerDecoder (attention.py:673-688): cross-attn rays->triangles, Swin/full self-attn, SwiGLU.
        ``kv_all``: every layer's K/V computed earlier (ops.scene_kv, an EncodedScene's), used in place of the
        context norm + K/V GEMM of the batched form; the fp8 and RF_KV_BATCH=0 paths project from ``ctx`` as ever."""
        cfg, W, dev = self.config, self._w, self._device
        D, H, F = cfg.view_transformer_latent_dim, cfg.view_transformer_n_heads, cfg.view_transformer_ffn_hidden_dim
        T2, R, P = x.shape[0], plan.R, plan.B * plan.V
        qk = cfg.qk_norm
        n_dec = len(W.dec)
        kv_batch = self._kv_batch(plan.T1)
        if not kv_batch or self.fp8:
            kv_all = None
        # (the rotated keys of all layers are kept when they fit in 4 GiB: T_kv grows with the view count)
        k_batch = kv_batch and os.environ.get("RF_K_BATCH", "1") != "0" and plan.T_kv * n_dec * D * 2 <= (4 << 30)
        swin = cfg.view_transformer_use_swin_attn
        cap = self._capture
        if self._native_ok() and not self.fp8 and not (cap is not None and cap["dec"] is not None):
            # the whole stack as ONE library call (rf_decoder_forward): the same launches in the same order
            if getattr(W, "dec_desc", None) is None:
                W.dec_desc = ops.decoder_layers(W.dec, qk)
            out_idx = sorted(i for i in set(cfg.out_layers) if 0 <= i < n_dec)
            planes = [W.dpt.empty_tap_planes(j, P, plan.hp, plan.wp, D, dev) for j in range(len(out_idx))]
            proj_kv = kv_batch and kv_all is None  # (a given kv_all: the descriptor carries it, no K/V weights)
            kv = dict(ctx_norm=W.ctx_unit if proj_kv else None, w_kv_all=W.wkv_all if proj_kv else None,
                      kv_all=kv_all, k_batch=k_batch, k_norm_all=W.k_norm_all if qk else None,
                      kv_src_rows=plan.kv_src_rows, kv_pos=pos2, freqs=W.dec_freqs)
            cross = dict(ray_pos=ray_pos, ray_pos_div=R, problems=plan.prob2, schedule=plan.sched2, qk_fused=W.qk_fused)
            sa = dict(swin=swin, n_images=P, grid_h=plan.hp, grid_w=plan.wp, window=SWIN_WINDOW, shift=SWIN_SHIFT,
                      problems=None if swin else plan.prob_self)
            ops.decoder_forward(x, W.dec_desc, n_dec, H, F, W.half, EPS, ctx, kv, cross, sa,
                                [(i, pl.hi, pl.lo, pl.hi.shape[-1]) for i, pl in zip(out_idx, planes)], tag="attn_cross")
            self._capture = None  # (one-shot; a decoder-row capture takes the per-op path below)
            return planes
        h = torch.empty(T2, D, dtype=W.half, device=dev)
        q2 = torch.empty(T2, D, dtype=torch.bfloat16, device=dev)
        att = torch.empty(T2, D, dtype=W.half, device=dev)
        g = torch.empty(T2, F, dtype=W.half, device=dev)
        hc = torch.empty(plan.T1, ctx.shape[1], dtype=W.half, device=dev) if kv_all is None else None
        if kv_batch:
            if kv_all is None:
                ops.rmsnorm(ctx, W.ctx_unit, EPS, hc)
                kv_all = torch.empty(plan.T1, n_dec * 2 * D, dtype=torch.bfloat16, device=dev)
                ops.gemm(hc, W.wkv_all, kv_all)
        else:
            kv = torch.empty(plan.T1, 2 * D, dtype=torch.bfloat16, device=dev)
        if k_batch:
            # keys of all layers normed + rotated in one launch: layer i's K is the D columns at 2*D*i of kv_all,
            # its rotated copy the D columns at D*i of kview_all
            kview_all = torch.empty(plan.T_kv, n_dec * D, dtype=torch.bfloat16, device=dev)
            ops.qk_norm_rope_groups(kv_all, 2 * D, kview_all, D, n_dec, H, W.k_norm_all if qk else None, EPS, pos2,
                                    W.dec_freqs, src_rows=plan.kv_src_rows, ilv=W.qk_fused)
        else:
            kview = torch.empty(plan.T_kv, D, dtype=torch.bfloat16, device=dev)
        qkv = torch.empty(T2, 3 * D, dtype=torch.bfloat16, device=dev) if cfg.view_transformer_include_self_attn else None
        fp8 = self.fp8
        if fp8:
            W.make_fp8()
            xq = ops.MX8.empty(T2, D, dev)
            gq = ops.MX8.empty(T2, F, dev)

        fp8_set = self.fp8_projections

        def proj(inp, w_bf16, w_fp8, out, epi=ops.EPI_BF16, tag=None, name=""):
            if fp8 and name in fp8_set:
                ops.gemm_mx8(ops.quant_mx8(inp, gq if inp.shape[1] == F and F != D else xq), w_fp8, out, None, epi,
                             tag=tag)
            else:
                ops.gemm(inp, w_bf16, out, None, epi, tag=tag)
        taps = []
        outl = set(cfg.out_layers)
        # pre-norms deferred into the GEMMs around them as rf_decoder_forward issues them (the fp8 mode keeps the
        # row kernel: its projections quantise the normalised operand)
        defer = not fp8
        ss = torch.empty(T2, ops.PRENORM_SLOTS, dtype=torch.float32, device=dev) if defer else None
        qkss = torch.empty(T2, 2, ops.PRENORM_SLOTS, dtype=torch.float32, device=dev) if defer and swin and qk else None
        # the cross-attention query's rotation in its projection's epilogue (rf_decoder_forward's qk_fused sequence)
        qfuse = W.qk_fused and defer
        q2ss = torch.empty(T2, 1, ops.PRENORM_SLOTS, dtype=torch.float32, device=dev) if qfuse and qk else None

        def norm_proj(norm_w, w_half, w_fp8, out, epi=ops.EPI_BF16, tag=None, name=""):
            """out (epi)= rmsnorm(x) @ w.T: from the deferred operands, or row kernel + proj in the fp8 mode"""
            if defer:
                ops.gemm_rownorm(h, w_half, out, ss, EPS, epi, tag=tag)
            else:
                ops.rmsnorm(x, norm_w, EPS, h)
                proj(h, w_half, w_fp8, out, epi, tag=tag, name=name)

        def add_proj(inp, w_half, w_fp8, next_norm, tag=None, name=""):
            """x += inp @ w.T, and the next pre-norm's deferred operands when there is one"""
            if defer and next_norm is not None:
                ops.gemm_add_prenorm(inp, w_half, x, next_norm, h, ss, tag=tag)
            else:
                proj(inp, w_half, w_fp8, x, ops.EPI_ADD_F32, tag=tag, name=name)

        if defer:
            ops.prenorm(x, W.dec[0].query_norm, h, ss)
        for i, L in enumerate(W.dec):
            # (i) cross-attention: K/V projections once per scene, K rotated per view
            if qfuse:
                ops.gemm_qk_rope(h, L.wq, q2, ss, EPS, D, 1, L.q_norm if qk else None, q2ss, ray_pos, W.dec_freqs,
                                 q_scale=1.0 if qk else ops.Q_LOG2_SCALE, pos_div=R)
            else:
                norm_proj(L.query_norm, L.wq, getattr(L, "wq8", None), q2, name="q")
            if kv_batch:
                kv = kv_all[:, 2 * D * i:2 * D * (i + 1)]
            else:
                ops.rmsnorm(ctx, L.kv_norm, EPS, hc)
                ops.gemm(hc, L.wkv, kv)
            if k_batch:
                kview = kview_all[:, D * i:D * (i + 1)]
            if not qfuse:
                ops.qk_norm_rope(q2, q2, H, L.q_norm if qk else None, EPS, ray_pos, W.dec_freqs, pos_div=R,
                                 q_scale=ops.Q_LOG2_SCALE, ilv=W.qk_fused)
            if not k_batch:
                ops.qk_norm_rope_groups(kv[:, :D], 0, kview, 0, 1, H, L.k_norm if qk else None, EPS, pos2, W.dec_freqs,
                                        src_rows=plan.kv_src_rows, ilv=W.qk_fused)
            if q2ss is not None:
                ops.attention(q2, kview, kv[:, D:], att, plan.prob2, R, H, tag="attn_cross", max_k_len=plan.max_s,
                              schedule=plan.sched2, q_ss=q2ss[:, 0], q_eps=EPS)
            else:
                ops.attention(q2, kview, kv[:, D:], att, plan.prob2, R, H, tag="attn_cross", max_k_len=plan.max_s,
                              q_prescaled=True, schedule=plan.sched2)
            add_proj(att, L.wo, getattr(L, "wo8", None), L.self_norm if qkv is not None else L.ffn_norm, name="out")
            # (ii) self-attention between ray tokens
            if qkv is not None:
                qs, ks, vs = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
                qks = qkv[:, :2 * D]
                # Swin: q/k norm folded into the attention's loads from the projection's row sums, as
                # rf_decoder_forward issues it (rf_swin_attn_fwd_qkn)
                qkn = swin and defer and qk and D % 256 == 0 and D <= ops.PRENORM_SLOTS * 128
                if qkn:
                    ops.gemm_rownorm(h, L.ws_in, qkv, ss, EPS, seg_ss=qkss, seg_w=D)
                else:
                    norm_proj(L.self_norm, L.ws_in, getattr(L, "ws_in8", None), qkv, name="self_in")
                if qkn:
                    ops.swin_attention(qs, ks, vs, att, P, plan.hp, plan.wp, 0 if i % 2 == 0 else SWIN_SHIFT, H,
                                       SWIN_WINDOW, qk_norm=(qkss, L.sqk_norm, EPS))
                elif swin:
                    ops.qk_norm_rope(qks, qks, H, L.sqk_norm if qk else None, EPS, n_seg=2, q_scale=ops.Q_LOG2_SCALE)
                    ops.swin_attention(qs, ks, vs, att, P, plan.hp, plan.wp, 0 if i % 2 == 0 else SWIN_SHIFT, H,
                                       SWIN_WINDOW, q_prescaled=True)
                else:
                    ops.qk_norm_rope(qks, qks, H, L.sqk_norm if qk else None, EPS, ray_pos, W.dec_freqs, pos_div=R,
                                     n_seg=2, q_scale=ops.Q_LOG2_SCALE)
                    ops.attention(qs, ks, vs, att, plan.prob_self, R, H, max_k_len=R, q_prescaled=True)
                add_proj(att, L.ws_out, getattr(L, "ws_out8", None), L.ffn_norm, name="self_out")
            # (iii) FFN
            norm_proj(L.ffn_norm, L.w13, getattr(L, "w13_8", None), g, ops.EPI_SWIGLU, tag="gemm_w13_stage2", name="w13")
            add_proj(g, L.w2, getattr(L, "w2_8", None), W.dec[i + 1].query_norm if i + 1 < n_dec else None,
                     tag="gemm_w2_stage2", name="w2")
            if i in outl:  # straight into the DPT projection's operand planes (no fp32 copy of x)
                taps.append(W.dpt.tap_planes(len(taps), x, P, plan.hp, plan.wp))
            cap = self._capture
            if cap is not None and cap["dec"] is not None:  # (test capture, capture_taps)
                rows = torch.cat([v * R + cap["dec"] for v in cap["views"]])
                cap["out"].setdefault("dec_rows", []).append(
                    x.index_select(0, rows).view(len(cap["views"]), -1, D).clone())
        if self._capture is not None:
            if "dec_rows" in self._capture["out"]:
                self._capture["out"]["dec_rows"] = torch.stack(self._capture["out"]["dec_rows"])
            self._capture = None  # one-shot
        return taps

    def _ray_embed(self, plan: _Plan, ray_in: torch.Tensor):
        cfg, W, dev = self.config, self._w, self._device
        D = cfg.view_transformer_latent_dim
        T2 = ray_in.shape[0]
        ray_lin = torch.empty(T2, D, dtype=torch.float32, device=dev)
        ops.gemm(ray_in, W.ray_w, ray_lin, W.ray_b, ops.EPI_F32)
        x2 = torch.empty(T2, D, dtype=torch.float32, device=dev)
        ops.embed(x2, None, T2, W.patch_token, 1, ray_lin, W.ray_norm, ops.FLT_EPS)
        return x2

    def _decode(self, plan: _Plan, taps, log_decode: bool, channels_last: bool, *, window=None):
        """DPT head + ELU(1e-3) (+ 10^x - 1) — the last two fused into the final conv.  ``window`` = (y0, x0, H, W):
        only that window of the plan's (padded) frame is returned (an overscanned frame; channels-last), as one more
        small launch behind the final conv, whose epilogue has already decoded the pixels."""
        out = self._w.dpt(taps, plan.B * plan.V, plan.hp, plan.wp, self.config.patch_size, 1e-3, log_decode,
                          channels_last)
        if window is None:
            return out
        if not channels_last:
            raise ValueError("a frame window is cut from channels-last frames")
        return ops.frame_window(out, window)

    # ------------------------------------------------------------------ entry points
    @torch.no_grad()
    def render_views(self, triangles, texture, mask, vn, c2w, fov, resolution, log_encode: bool = True,
                     timings: Optional[dict] = None, *, intrinsics=None, overscan: bool = False) -> torch.Tensor:
        """Pipeline fast path: rays, camera transform and positions are generated on the device.  ``resolution`` is
        an int (a square frame) or (height, width); ``fov`` is the vertical field of view of the frame height.
        Returns [B, V, H, W, C] linear HDR (log-decoded unless use_ldr).

        ``intrinsics`` (instead of ``fov``, which is then None): float32 [B, V, 4] = (fx, fy, cx, cy) in pixels of
        the requested H x W frame, origin at its top-left corner, pixel (x, y) centred at (x + 0.5, y + 0.5);
        camera-space direction ((x + 0.5 - cx) / fx, -(y + 0.5 - cy) / fy, -1), rotated by c2w and L2-normalised.
        The fov convention is fx = fy = H / 2 / tan(fov / 2), cx = W / 2, cy = H / 2.  Values are not read back:
        non-positive focal lengths are the caller's error.

        ``overscan=True`` takes any positive H x W (``frame_layout``): the model renders the frame padded to
        multiples of the frame unit with the same focal lengths, the requested frame centred in it (the border
        pixels are real rays of a slightly wider view), and only the requested window is returned.  Without it a
        side that is no multiple of the unit raises; with it on a frame that needs no padding the call issues the
        same launches and returns the same bits as without.

        Every launch goes to the current stream of the MODEL's device, whatever device is current in the
        caller (the reference's own infer.py places the model on cuda:1, infer.py:43)."""
        layout = frame_layout(self.config, resolution, overscan)
        _check_camera(c2w, fov, intrinsics)
        self._require()
        cam = dict(intrinsics=intrinsics, overscan=overscan)
        with torch.cuda.device(self._device):
            # the replay (an fp16 overflow's re-render) must not log-encode the texture a second time
            return self._guard.run(
                lambda: self._render_views(triangles, texture, mask, vn, c2w, fov, layout[:2], log_encode, **cam),
                lambda: self._render_views(triangles, texture, mask, vn, c2w, fov, layout[:2], False, **cam),
                (triangles, texture, mask, vn, c2w, fov if intrinsics is None else intrinsics))

    # ------------------------------------------------------------------ encode once, render many cameras
    @torch.no_grad()
    def encode_scene(self, triangles, texture, mask, vn, log_encode: bool = True) -> EncodedScene:
        """Everything of a render that does not depend on the camera, once: the triangle embedding, stage 1 and
        (in the batched K/V form) every decoder layer's K/V, exactly as ``render_views`` computes them.  The handle
        renders any number of cameras (``render_encoded``), each frame launching what a full render launches after
        its K/V GEMM, so on the same bits.  ``texture`` is log-encoded in place (once) like ``render_views``'.

        fp16 range check: the encode runs under a range word of its own and, unless ``range_check`` is "off", waits
        for its end event before returning (once per scene).  An overflow raises DeviceError in the "deferred" mode;
        "sync" / "lazy" move the model to bf16 operands (PrecisionWarning) and encode again."""
        self._require()
        with torch.cuda.device(self._device):
            self._on_device([(triangles, "triangles"), (texture, "texture"), (mask, "mask"), (vn, "vn")])
            sc = EncodedScene(self, self._generation, self._device, self._mask_host(mask),
                              (triangles, texture, mask, vn))
            with sc.lock:
                self._encode_checked(sc, log_encode)
            return sc

    def _encode(self, sc: EncodedScene, log_encode: bool):
        """Fill the handle from its inputs with the model's present weights, on the current stream."""
        cfg = self.config
        triangles, texture, _, vn = sc.inputs
        # (stage 1's tables do not depend on the view count or the resolution: the smallest valid plan)
        res0 = cfg.patch_size * (SWIN_WINDOW if cfg.view_transformer_use_swin_attn else 1)
        plan = self._plan_host(sc.mask_host, 1, res0)
        W = self._w
        tris, x1 = self._scene_front(plan, triangles, texture, vn, log_encode)
        kv_all = None
        if self._kv_batch(plan.T1) and not self.fp8 and plan.T1 > 0:
            kv_all = ops.scene_kv(x1, W.ctx_unit, W.wkv_all, EPS)
        stream = torch.cuda.current_stream()
        ev = torch.cuda.Event()
        ev.record(stream)
        sc.x1, sc.kv_all, sc.tris = x1, kv_all, tris
        sc.weights, sc.precision = W, (self.operands, self.dpt_precision)
        sc.stream, sc.event = stream, ev

    def _encode_checked(self, sc: EncodedScene, log_encode: bool):
        """_encode under a range word of its own, resolved before returning (the caller holds sc.lock)."""
        if not (self.operands == "f16" and self.range_check != "off"):  # (stage 1 has no other fp16 writer)
            return self._encode(sc, log_encode)
        with self._guard.bound() as word:
            self._encode(sc, log_encode)
        sc.event.synchronize()
        code, what = self._guard.take(word)
        if not code:
            return
        if self.range_check == "deferred":
            raise deferred_error(code, what, "encode with operands='bf16' (RF_OPERANDS=bf16), or range_check='sync' "
                                 "/ 'lazy' (encodes such a scene again)", where=" while encoding a scene")
        self._fall_back(code, what, "scene is encoded again", stacklevel=5)
        self._guard.replay(lambda: self._encode(sc, False))  # (the texture is log-encoded already)

    def _check_handle(self, sc: EncodedScene):
        if not isinstance(sc, EncodedScene):
            raise ValueError(f"render_encoded needs an EncodedScene (encode_scene / pipeline.encode), got {type(sc)}")
        if sc.model is not self:
            raise ValueError("this EncodedScene was encoded by another RenderFormer: a handle renders only with the "
                             "model that made it")
        if sc.device != self._device:
            raise ValueError(f"this EncodedScene lives on {sc.device}, the model on {self._device}")
        if sc.generation != self._generation:
            raise ValueError("this EncodedScene was made before the model's to() / load_state_dict: its stage-1 "
                             "output belongs to other weights; encode the scene again")

    def _refresh(self, sc: EncodedScene):
        """Staleness: a handle computed with other operands than the model has now (an fp16 fallback happened since)
        is encoded again in place from its retained inputs, on the current stream, before stage 2 reads it."""
        from ._lib import DeviceError
        with sc.lock:
            if sc.weights is self._w and sc.precision == (self.operands, self.dpt_precision):
                return
            if any(t._version != v for t, v in zip(sc.inputs, sc.versions)):
                raise DeviceError("this EncodedScene must be encoded again (the model fell back to "
                                  f"{self.operands} operands after an fp16 overflow), but its input tensors were "
                                  "modified in place since encode: keep them unchanged while the handle is in use, or "
                                  "encode the scene again")
            sc.event.synchronize()  # the old state may still be read on the encode's stream; then it is replaced
            self._encode(sc, False)

    @torch.no_grad()
    def render_encoded(self, scene: EncodedScene, c2w, fov, resolution, *, intrinsics=None,
                       overscan: bool = False) -> torch.Tensor:
        """Render the cameras ``c2w`` [B, V, 4, 4] / ``fov`` [B, V, ...] of an encoded batch of scenes: stage 2 +
        DPT only, per chunk of ``view_chunk`` views like ``render_views``.  ``resolution`` is an int or (height,
        width), ``intrinsics`` [B, V, 4] (with ``fov=None``) and ``overscan`` as in ``render_views``.  Returns
        [B, V, H, W, C] linear HDR,
        bit-identical to ``render_views`` of the same inputs.  Same range-check modes as ``render_views`` (``resolve
        (out)`` works); after an fp16 overflow, here or in any other render of the model, the handle is encoded
        again with the model's new operands before the frame is (re-)rendered."""
        layout = frame_layout(self.config, resolution, overscan)
        _check_camera(c2w, fov, intrinsics)
        self._require()
        self._check_handle(scene)
        with torch.cuda.device(self._device):
            run = lambda: self._render_encoded(scene, c2w, fov, layout[:2], intrinsics=intrinsics,  # noqa: E731
                                               overscan=overscan)
            return self._guard.run(run, run, (c2w, fov if intrinsics is None else intrinsics))

    def _render_encoded(self, sc: EncodedScene, c2w, fov, resolution, *, intrinsics=None, overscan=False):
        self._check_handle(sc)
        self._on_device([(c2w, "c2w"), (fov, "fov") if intrinsics is None else (intrinsics, "intrinsics")])
        if c2w.shape[0] != sc.batch_size:
            raise ValueError(f"c2w has batch size {c2w.shape[0]}, the encoded scene {sc.batch_size}")
        _, _, Hp, Wp, _, _ = frame_layout(self.config, resolution, overscan)  # (the entry point checked it)
        self._refresh(sc)
        with sc.lock:
            x1, kv_all, tris, ev, st = sc.x1, sc.kv_all, sc.tris, sc.event, sc.stream
        cur = torch.cuda.current_stream()
        if cur != st:  # another stream than the encode's: order after it, and keep the tensors alive for this one
            cur.wait_event(ev)
            for t in (x1, kv_all, tris):
                if t is not None:
                    t.record_stream(cur)
        return self._view_chunks(lambda n: self._plan_host(sc.mask_host, n, (Hp, Wp)), x1, tris, c2w, fov, resolution,
                                 kv_all, intrinsics=intrinsics, overscan=overscan)

    # ------------------------------------------------------------------ fp16 range check
    def _fall_back(self, code: int, what, redo: str, stacklevel: int):
        """Move the model to the operands an fp16 overflow (range code ``code``) asks for, and warn."""
        import warnings
        with self._guard.lock:
            # projections and attention (codes 1/2/4) -> bf16 operands; the DPT planes (code 8) -> bf16x3, and a
            # stage-1 or stage-2 overflow reaches the DPT as inf too, so it sets 8 as well
            operands = "bf16" if code & 7 else self.operands
            dpt = "bf16x3" if code & 8 and self.dpt_precision == "f16" else self.dpt_precision
            if (operands, dpt) != (self.operands, self.dpt_precision):  # (a frame that ran before an earlier
                # fallback only needs its re-render) ADVICE r5 (medium): the weights are rebuilt below, which frees
                # the old tensors into the caching allocator of the stream they were made on; frames still in flight
                # on other streams read them, so wait for every pending frame first (an overflow is rare: this wait
                # is the fallback path's only cost)
                for p in self._guard.pending:
                    p.event.synchronize()
                self.operands, self.dpt_precision = operands, dpt
                self._w = _DeviceWeights(self.config, self._sd, self._device, self.dpt_precision, self.operands)
            self.range_fallbacks += 1
        warnings.warn(f"fp16 operand overflow (range code {code}: {'/'.join(what)}): this checkpoint's activations "
                      f"exceed fp16's range; the {redo} and the model keeps "
                      f"{self.operands} projection operands and {self.dpt_precision} DPT planes from now on",
                      PrecisionWarning, stacklevel=stacklevel)

    def resolve(self, out: Optional[torch.Tensor] = None) -> bool:
        """Finish the range check of the frame whose output is ``out`` (every pending frame if None), waiting for
        it: afterwards ``out`` holds the final frame (rendered again if it overflowed fp16).  Returns True if a
        frame was rendered again.  batch_infer.py calls it where it already waits for the frame's copy; in the
        default "sync" mode render has already done it and this only reports."""
        return self._guard.resolve(out)

    def check_range(self):
        """Resolve every pending frame (waiting for each): deferred mode raises DeviceError for an overflowed frame,
        lazy mode re-renders it in place.  Call before reading frames whose range check is pending."""
        self._guard.check_range()

    def close(self):
        """Release the model's host-mapped range words: pending frames are waited for first.  Called
        by ``__del__``; the model stays usable (new words are allocated on the next render)."""
        self._guard.close()

    def __del__(self):
        try:
            if getattr(self, "_guard", None) is not None:
                self.close()
        except Exception:  # interpreter shutdown: the library or torch may already be gone
            pass

    @property
    def precision(self) -> str:
        """What the projections and attention compute with (the pipeline's last_precision["computed"])."""
        proj = {"f16": "fp16", "bf16": "bf16"}[self.operands]
        fp8 = f"; stage-2 {', '.join(sorted(self.fp8_projections))} as MX fp8" if self.fp8 else ""
        return (f"{proj} projection operands{fp8}, bf16 attention q/k/v, fp32 accumulate/softmax/residual; DPT "
                f"{'fp16' if self.dpt_precision == 'f16' else 'bf16x3'} operands, fp32 accumulate")

    def _render_views(self, triangles, texture, mask, vn, c2w, fov, resolution, log_encode, *, intrinsics=None,
                      overscan=False):
        self._on_device([(triangles, "triangles"), (texture, "texture"), (mask, "mask"), (vn, "vn"), (c2w, "c2w"),
                         (fov, "fov") if intrinsics is None else (intrinsics, "intrinsics")])
        _, _, Hp, Wp, _, _ = frame_layout(self.config, resolution, overscan)  # (the entry point checked it)
        # (plans are built for, and cached by, the padded frame; a mask tensor seen before is not read back)
        plan_of = lambda n: self._plan(mask, n, (Hp, Wp))  # noqa: E731
        tris, x1 = self._scene_front(plan_of(self._chunk(c2w.shape[1])), triangles, texture, vn, log_encode)
        return self._view_chunks(plan_of, x1, tris, c2w, fov, resolution, intrinsics=intrinsics, overscan=overscan)

    def _chunk(self, V: int) -> int:
        return V if not self.view_chunk else min(V, int(self.view_chunk))

    def _on_device(self, tensors):
        """Every tensor of the ``(tensor, name)`` pairs is on the model's device."""
        for t, n in tensors:
            if t.device != self._device:
                raise ValueError(f"{n} must be on {self._device} (got {t.device})")

    def _scene_front(self, plan: _Plan, triangles, texture, vn, log_encode: bool):
        """The camera-independent front of a render: packed triangles, their embedding and positions, stage 1.
        Returns (tris [B, N, 9] f32, x1 [T1, D] f32)."""
        B = plan.B
        tris = triangles.reshape(B, -1, 9).float().contiguous()
        x1 = self._embed_triangles(plan, texture, vn.reshape(B, -1, 9).float().contiguous(), log_encode)
        pos1 = torch.empty(plan.T1, 9, dtype=torch.float32, device=self._device)
        ops.scene_pos(tris, plan.valid_flat, plan.scene_off, None, B, 1, self.config.num_register_tokens, pos1,
                      plan.cu1, max(plan.counts))
        return tris, self._stage1(plan, x1, pos1)

    def _view_chunks(self, plan_of, x1, tris, c2w, fov, resolution, kv_all=None, *, intrinsics=None, overscan=False):
        """Stage 2 + DPT (``_views``) over the views in chunks of at most view_chunk, as [B, V, H, W, C];
        ``plan_of(n)`` is the plan of a chunk of n views.  Every chunk runs the same launch sequence on the same
        problem tables whatever the other views are, so a view's image does not depend on how the views of a scene
        are batched or split over ranks (bench.py c5)."""
        B, V = c2w.shape[:2]
        H, W = frame_layout(self.config, resolution, overscan)[:2]
        cut = lambda t, a, b: None if t is None else t[:, a:b]  # noqa: E731
        chunk = self._chunk(V)
        out = None
        for v0 in range(0, V, chunk):
            v1 = min(V, v0 + chunk)
            o = self._views(plan_of(v1 - v0), x1, tris, c2w[:, v0:v1], cut(fov, v0, v1), resolution, kv_all,
                            intrinsics=cut(intrinsics, v0, v1), overscan=overscan)
            o = o.view(B, v1 - v0, H, W, -1)
            if v1 - v0 == V:
                return o
            if out is None:
                out = torch.empty(B, V, *o.shape[2:], dtype=o.dtype, device=self._device)
            out[:, v0:v1] = o
        return out

    def _views(self, plan: _Plan, x1, tris, c2w, fov, resolution, kv_all=None, *, intrinsics=None, overscan=False):
        """Stage 2 + DPT + decode for the plan's views of every scene (c2w [B, Vc, 4, 4], fov [B, Vc, ...] or
        intrinsics [B, Vc, 4]); ``kv_all``: the scene's K/V of every decoder layer when it is already known (an
        EncodedScene's).  ``resolution`` is the requested (H, W); the plan is the padded frame's (frame_layout).
        Returns [P, H, W, C]."""
        cfg, dev = self.config, self._device
        B, V = plan.B, plan.V
        P = B * V
        H, W, Hp, Wp, y0, x0 = frame_layout(cfg, resolution, overscan)
        padded = (Hp, Wp) != (H, W)
        c2w_v = c2w.reshape(P, 4, 4).float().contiguous()
        eye = self._w.eyes.get(P)
        if eye is None:
            eye = self._w.eyes[P] = torch.eye(4, dtype=torch.float32).expand(P, 4, 4).contiguous().to(dev)
        rays_c2w, pos_c2w = (eye, c2w_v) if cfg.turn_to_cam_coord else (c2w_v, eye)
        ray_in = torch.empty(P * plan.R, 3 * cfg.patch_size ** 2, dtype=self._w.half, device=dev)
        ray_pos = torch.empty(P, 9, dtype=torch.float32, device=dev)
        if intrinsics is None and not padded:  # the plain frame keeps rf_ray_tokens_hw (the bench's launch sequence)
            ops.ray_tokens(rays_c2w, fov.reshape(P).float().contiguous(), resolution, cfg.patch_size, ray_in, ray_pos)
        else:
            ops.ray_tokens_cam(rays_c2w, None if fov is None else fov.reshape(P).float().contiguous(),
                               None if intrinsics is None else intrinsics.reshape(P, 4).contiguous(), (H, W),
                               (Hp, Wp), (y0, x0), cfg.patch_size, ray_in, ray_pos)
        x2 = self._ray_embed(plan, ray_in)
        pos2 = torch.empty(plan.T_kv, 9, dtype=torch.float32, device=dev)
        ops.scene_pos(tris, plan.valid_flat, plan.scene_off, pos_c2w, B, V, cfg.num_register_tokens, pos2,
                      plan.kv_off, max(plan.counts))
        taps = self._stage2(plan, x2, x1, pos2, ray_pos, kv_all)
        return self._decode(plan, taps, log_decode=not cfg.use_ldr, channels_last=True,
                            window=(y0, x0, H, W) if padded else None)

    @torch.no_grad()
    def forward(self, tri_vpos_list, texture_patch_list, valid_mask, vns, rays_o, rays_d, tri_vpos_view_tf,
                tf32_view_tf=False):
        """Reference signature (renderformer.py:171-206).  ``rays_d`` is [B, V, H, W, 3] for any valid H x W
        (frame_size), as the reference's ViewTransformer takes it.  Returns ELU'd log-space images [B, V, C, H, W]."""
        self._require()
        with torch.cuda.device(self._device):
            args = (tri_vpos_list, texture_patch_list, valid_mask, vns, rays_o, rays_d, tri_vpos_view_tf)
            return self._guard.run(lambda: self._forward(*args), lambda: self._forward(*args), args)

    def _forward(self, tri_vpos_list, texture_patch_list, valid_mask, vns, rays_o, rays_d, tri_vpos_view_tf):
        cfg, dev = self.config, self._device
        B, V = rays_o.shape[:2]
        H, W = frame_size(cfg, tuple(rays_d.shape[2:4]))
        plan = self._plan(valid_mask, V, (H, W))
        _, x1 = self._scene_front(plan, tri_vpos_list, texture_patch_list.float().contiguous(), vns, log_encode=False)
        P = B * V
        ray_in = torch.empty(P * plan.R, 3 * cfg.patch_size ** 2, dtype=self._w.half, device=dev)
        ops.patchify_rays(rays_d.reshape(P, H, W, 3).float().contiguous(), cfg.patch_size, ray_in)
        ray_pos = rays_o.reshape(P, 1, 3).float().expand(P, 3, 3).reshape(P, 9).contiguous()
        x2 = self._ray_embed(plan, ray_in)
        # per-view positions: every (b, v) is its own set over the [P*N, 9] camera-frame triangles
        N = valid_mask.shape[1]
        vmask = valid_mask.repeat_interleave(V, dim=0)
        view_valid = torch.nonzero(vmask.reshape(-1)).squeeze(1).to(torch.int32)
        view_off = torch.tensor([0] + [c for c in plan.counts for _ in range(V)], device=dev).cumsum(0).to(torch.int32)
        pos2 = torch.empty(plan.T_kv, 9, dtype=torch.float32, device=dev)
        ops.scene_pos(tri_vpos_view_tf.reshape(P * N, 9).float().contiguous(), view_valid, view_off, None, P, 1,
                      cfg.num_register_tokens, pos2, plan.kv_off, max(plan.counts))
        taps = self._stage2(plan, x2, x1, pos2, ray_pos)
        out = self._decode(plan, taps, log_decode=False, channels_last=False)
        return out.view(B, V, *out.shape[1:])

    __call__ = forward
