#!/usr/bin/env python
"""What a moving object and a changing material cost per frame, three ways: pipe.pose against the host and against torch.

The bench's default workload (bench.py's own argument defaults and scene helpers: large-proxy, the 5,633-triangle
synthetic scene) as a rig of two objects (the triangles alternate between them; every triangle has a material row of
its own).  Every frame turns object 1 a little further about z and sweeps the roughness of its material rows, then
runs the same pipe.encode + pipe.render_encoded (512 x 512, one camera) and ends with a wait for the stream; blocks
are timed with the host clock.  The arms differ in how the frame's scene tensors are made:

  host    rig.pose_numpy on the host, scenes.expand_texture of its rows to [1, N, 13, 32, 32], three uploads
  torch   on the device with torch ops: gathered matrix products on the triangles and normals (cofactor rows by
          torch.cross), the expanded texture rebuilt by broadcasting the rows against the patch mask
  pose    pipe.pose (one HIP launch) with material rows [1, N, 13]: nothing expanded

All arms run in one process in interleaved blocks (host torch pose host torch pose ...) after a warm-up of each.
Also reported: the pose launch alone (device events round REPS back-to-back calls, outside the timed blocks), the
device bytes each arm holds for the scene's texture, and the worst difference of the arms' frames from the pose arm's
(the three make the same scene up to fp32 rounding).  Prints ONE JSON line.

  python tools/posed_frames.py [--frames 4] [--blocks 5] [--out profiles/posed_frames.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  (the workload's defaults; bench.py itself is not run)
from camera_sweep import orbit  # noqa: E402

ARMS = ("host", "torch", "pose")
RES = 512
REPS = 20


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=4, help="frames per block")
    ap.add_argument("--blocks", type=int, default=5, help="interleaved blocks per arm")
    ap.add_argument("--warmup", type=int, default=2, help="untimed frames per arm before the first block")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("posed_frames.py: no HIP device (a timing needs the GPU)", file=sys.stderr)
        return 2
    w = bench.parse([])  # the bench's default workload
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    from renderformer_amd.config import named_config
    from renderformer_amd.rig import SceneRig, pose_numpy, trs
    from renderformer_amd.scenes import expand_texture, synthetic_scene, texture_mask
    from renderformer_amd.weights import synthetic_state_dict

    cfg = named_config(w.config)
    pipe = RenderFormerRenderingPipeline(RenderFormer(cfg, synthetic_state_dict(cfg, seed=0),
                                                      range_check="deferred")).to(dev)
    s = synthetic_scene(w.tris, 1, seed=1)
    N = s.triangles.shape[0]
    oid = (np.arange(N) % 2).astype(np.int32)[None]
    rig = SceneRig(s.triangles[None], s.vn[None], oid, np.arange(N, dtype=np.int32)[None], ["still", "turning"],
                   np.tile(trs().numpy(), (1, 2, 1, 1)), s.tex_channels[None])
    drig = rig.to(dev)
    moving = torch.from_numpy(oid[0] == 1)
    mask = drig.mask
    pipe.model.plan_hint(mask, rig.mask.numpy())
    c2w = orbit(1).to(dev)[None][:, :1].contiguous()
    fov = torch.from_numpy(s.fov[:1]).to(dev).reshape(1, 1, 1)
    stream = torch.cuda.current_stream(dev)
    maskf = torch.from_numpy(texture_mask(32)).to(dev).float()
    oid_l = drig.object_id[0].long()

    def frame_inputs(k, n):
        """(transforms [1, 2, 3, 4], materials [1, N, 13]) of frame k of n, on the host"""
        xf = rig.transforms0.clone()
        xf[0, 1] = trs((0.0, 0.0, 0.0), (0.0, 0.0, 3.0 * (k + 1)), 1.0)
        mat = rig.materials0.clone()
        mat[0, moving, 6] = float(np.float16((k + 1) / (n + 1)))
        return xf, mat

    def scene_host(xf, mat):
        t, n, rows = pose_numpy(rig, xf, mat)
        tex = expand_texture(rows.astype(np.float32))
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)  # noqa: E731
        return up(t), up(tex), mask, up(n)

    def scene_torch(xf, mat):
        xf, mat = xf.to(dev), mat.to(dev)
        A = xf[0, :, :, :3]
        cof = torch.stack([torch.cross(A[:, 1], A[:, 2], dim=-1), torch.cross(A[:, 2], A[:, 0], dim=-1),
                           torch.cross(A[:, 0], A[:, 1], dim=-1)], dim=1)
        det = (A[:, 0] * cof[:, 0]).sum(-1)
        cof = torch.where(det[:, None, None] < 0, -cof, cof)
        t = torch.einsum("nij,nvj->nvi", A[oid_l], drig.triangles[0]) + xf[0, oid_l, None, :, 3]
        g = torch.einsum("nij,nvj->nvi", cof[oid_l], drig.vn[0])
        ln = g.norm(dim=-1, keepdim=True)
        n = torch.where(ln > 0, g / ln.clamp_min(1e-30), torch.zeros_like(g))
        tex = (mat[0, drig.material_id[0].long()][:, :, None, None] * maskf).contiguous()
        return t[None].contiguous(), tex[None], mask, n[None].contiguous()

    def scene_pose(xf, mat):
        return pipe.pose(drig, xf.to(dev), mat.to(dev))

    make = {"host": scene_host, "torch": scene_torch, "pose": scene_pose}
    tex_bytes = {}

    def frames(arm, n):
        out = None
        for k in range(n):
            sc_in = make[arm](*frame_inputs(k, n))
            tex_bytes[arm] = sc_in[1].numel() * sc_in[1].element_size()
            scene = pipe.encode(*sc_in)
            out = pipe.render_encoded(scene, c2w, fov, RES, torch_dtype=torch.bfloat16)
            stream.synchronize()
        return out

    last = {}
    for arm in ARMS:
        frames(arm, min(a.warmup, a.frames))
    torch.cuda.synchronize()
    ms = {arm: [] for arm in ARMS}
    for _ in range(a.blocks):
        for arm in ARMS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[arm] = frames(arm, a.frames)
            ms[arm].append(1e3 * (time.perf_counter() - t0) / a.frames)
            if not torch.isfinite(last[arm]).all():
                raise RuntimeError(f"non-finite output of arm {arm}")
    pipe.check_range()
    # the pose launch alone
    xf, mat = (t.to(dev) for t in frame_inputs(0, a.frames))
    posed = pipe.pose(drig, xf, mat)
    pose_us = []
    for _ in range(a.blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(REPS):
            pipe.pose(drig, xf, mat, out=posed)
        e1.record(stream)
        e1.synchronize()
        pose_us.append(1e3 * e0.elapsed_time(e1) / REPS)
    rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm())  # noqa: E731
    med = {arm: statistics.median(v) for arm, v in ms.items()}
    rec = {
        "metric": "ms per frame: make the frame's scene tensors (one object turned, one roughness swept), pipe.encode, "
                  "pipe.render_encoded of one 512 x 512 camera, stream wait; host clock round blocks; median over "
                  "interleaved blocks",
        "arms": {"host": "pose_numpy + expand_texture on the host, uploads",
                 "torch": "torch ops on the device, expanded texture rebuilt by broadcasting",
                 "pose": "pipe.pose (one HIP launch), material rows [1, N, 13]"},
        "config": w.config, "tris": N, "resolution": RES, "device": torch.cuda.get_device_name(dev),
        "frames_per_block": a.frames, "blocks": a.blocks,
        "ms_per_frame": {arm: round(med[arm], 4) for arm in ARMS},
        "ms_blocks": {arm: [round(v, 4) for v in ms[arm]] for arm in ARMS},
        "block_spread": {arm: [round(min(ms[arm]) / med[arm], 4), round(max(ms[arm]) / med[arm], 4)] for arm in ARMS},
        "pose_minus_torch_ms": round(med["pose"] - med["torch"], 4),
        "pose_minus_host_ms": round(med["pose"] - med["host"], 4),
        "pose_launch_us": round(statistics.median(pose_us), 2),
        "pose_launch_us_blocks": [round(v, 2) for v in pose_us],
        "texture_device_bytes": tex_bytes,
        "frame_rel_l2_vs_pose": {arm: rel(last[arm], last["pose"]) for arm in ("host", "torch")},
    }
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
