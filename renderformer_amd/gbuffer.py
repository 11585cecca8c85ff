"""Geometry buffers from primary rays: alpha, depth, triangle id, shading normal and diffuse albedo per pixel.

The frame the model renders is RGB radiance only.  Everything here is a function of the input triangles and the
primary rays the package already defines (``ops.ray_tokens_cam``: pixel centres at +0.5, the fov and intrinsics
conventions of ``RenderFormerRenderingPipeline.render``), found by one brute-force visibility pass on the device
(``ops.primary_hits``) and one elementwise shading pass (``ops.gbuffer_shade``).  No model weights are involved:
``trace`` takes the scene tensors, the tables of ``scene_tables`` and cameras.

Conventions (rf.h rf_primary_hits / rf_gbuffer_shade):
  alpha    uint8    255 where the pixel's ray hits a valid triangle, 0 elsewhere
  depth    float32  distance t along the NORMALISED ray (+inf on a miss); the z-depth of a rasteriser is
                    ``t / |d_cam|`` with ``d_cam = ((x + 0.5 - cx) / fx, -(y + 0.5 - cy) / fy, -1)``
  tri_id   int32    index on the N axis of ``triangles[b]`` (so ``texture[b, id]`` and ``vn[b, id]`` are the hit
                    triangle's), -1 on a miss
  normal   float32  world-space shading normal interpolated from ``vn``, not flipped toward the camera; 0 on a miss
  albedo   float32  the diffuse channels (0..2) of the hit triangle's texture at texel (0, 0), which is the whole
                    patch for the constant-per-triangle textures the scene converter writes; a lookup into patches
                    that vary over the triangle is not done.  0 on a miss
Triangles are double-sided, the nearest hit wins and among equal distances the lowest index; shared edges and
vertices are watertight.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch

from . import ops

OUTPUTS = ("alpha", "depth", "tri_id", "normal", "albedo")


class GBuffer(NamedTuple):
    """[B, V, H, W] (normal and albedo [B, V, H, W, 3]) device tensors; a buffer that was not asked for is None."""
    alpha: Optional[torch.Tensor] = None
    depth: Optional[torch.Tensor] = None
    tri_id: Optional[torch.Tensor] = None
    normal: Optional[torch.Tensor] = None
    albedo: Optional[torch.Tensor] = None


def check_outputs(outputs) -> Tuple[str, ...]:
    """``outputs`` (None = all) as a tuple of known names in OUTPUTS order; ValueError for an unknown name."""
    if outputs is None:
        return OUTPUTS
    if isinstance(outputs, str):
        outputs = (outputs,)
    names = tuple(outputs)
    bad = [n for n in names if n not in OUTPUTS]
    if bad or not names:
        raise ValueError(f"gbuffer: unknown outputs {bad}: choose from {OUTPUTS}" if bad else
                         f"gbuffer: outputs is empty: choose from {OUTPUTS}")
    return tuple(n for n in OUTPUTS if n in names)


def scene_tables(mask_host, device):
    """(valid_idx int32 [n_valid], scene_off int32 [B + 1], n_valid) of a HOST mask (bool [B, N]): the rows of the
    [B N, 9] triangle array that are valid, grouped by scene -- the tables a render's plan holds as ``valid_flat`` /
    ``scene_off``.  One pinned, non-blocking copy; nothing is read back."""
    import numpy as np
    m = np.asarray(mask_host, dtype=bool)
    valid = np.flatnonzero(m.reshape(-1)).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(m.sum(axis=1))]).astype(np.int32)
    buf = torch.from_numpy(np.concatenate([valid, off]))
    if torch.device(device).type == "cuda":
        buf = buf.pin_memory().to(device, non_blocking=True)
    return buf[:valid.size], buf[valid.size:], int(valid.size)


def trace(triangles: torch.Tensor, texture: Optional[torch.Tensor], vn: Optional[torch.Tensor], tables, c2w, fov,
          intrinsics, frame, outputs=None) -> GBuffer:
    """The G-buffer of an H x W ``frame`` for cameras ``c2w`` [B, V, 4, 4] with ``fov`` [B, V(, 1)] or ``intrinsics``
    [B, V, 4].  ``tables`` = (valid_idx, scene_off, n_valid) as from ``scene_tables``.  Only the buffers named in
    ``outputs`` are computed: without 'normal' no barycentrics are written, without 'normal' and 'albedo' the shading
    kernel is not launched.  Every input is only read."""
    names = check_outputs(outputs)
    valid_idx, scene_off, n_valid = tables
    B = c2w.shape[0]
    tris = triangles.reshape(B, -1, 9).float().contiguous()
    cam = c2w.float().contiguous()
    fov_c = None if fov is None else fov.float().contiguous()
    intr_c = None if intrinsics is None else intrinsics.contiguous()
    shade = [n for n in ("normal", "albedo") if n in names]
    hits = ops.primary_hits(tris, valid_idx, scene_off, n_valid, cam, fov_c, intr_c, frame,
                            bary="normal" in names, alpha="alpha" in names)
    res = dict(hits)
    if shade:
        res.update(ops.gbuffer_shade(hits["tri_id"], hits.get("bary"),
                                     vn.reshape(B, -1, 9).float().contiguous() if "normal" in names else None,
                                     texture if "albedo" in names else None, normal="normal" in names,
                                     albedo="albedo" in names))
    return GBuffer(**{n: res[n] for n in names})
