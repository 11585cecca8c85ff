#!/usr/bin/env python
"""What a 16:9 frame costs: 1024 x 576 against the square frames around it, one encoded scene, one camera per call.

The bench's default workload (bench.py's own argument defaults and scene helpers: large-proxy, the 5,633-triangle
synthetic scene), encoded once (pipe.encode); every frame is a pipe.render_encoded(scene, c2w_k, fov_k, (H, W)) of
the next camera on the orbit tools/camera_sweep.py uses.  Shapes:

  1024 x 576   (H, W) = (576, 1024): 9,216 ray tokens, 589,824 pixels
  768 x 768    the same token and pixel counts, square
  1024 x 1024  what a caller without rectangular frames renders and crops: 16,384 tokens

All shapes run in the same process in interleaved blocks (A B C A B C ...) after a warm-up of every shape, each block
timed with a device event pair around its frames and no host wait inside (the fp16 range check is deferred, as in
bench.py, and read after the last block).  Prints ONE JSON line: per shape the median over blocks of the ms per
frame, and the ratios.

The two 9,216-token shapes launch the same kernels on the same amount of work; only the DPT levels' aspect differs
(512 x 288 / 256 x 144 / ... against 384^2 / 192^2 / ...).  Should 1024 x 576 ever come out more than 10 % behind
768 x 768, trace one frame of each with rocprofv3 --kernel-trace and compare the conv / halo kernels per level
(tools/prof_summary.py splits a kernel's launches by grid).

  python tools/rect_frames.py [--frames 8] [--blocks 5] [--out profiles/rect_frames.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tools")]

import torch  # noqa: E402

import bench  # noqa: E402  (the workload's defaults; bench.py itself is not run)
from camera_sweep import orbit  # noqa: E402

SHAPES = [(576, 1024), (768, 768), (1024, 1024)]  # (H, W)


def _name(hw) -> str:
    return f"{hw[1]}x{hw[0]}"  # width x height, as frame sizes are usually written


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=8, help="cameras per block")
    ap.add_argument("--blocks", type=int, default=5, help="interleaved blocks per shape")
    ap.add_argument("--warmup", type=int, default=2, help="untimed frames per shape before the first block")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("rect_frames.py: no HIP device (a timing needs the GPU)", file=sys.stderr)
        return 2
    w = bench.parse([])  # the bench's default workload
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    from renderformer_amd.config import named_config
    from renderformer_amd.scenes import batch_scenes, synthetic_scene
    from renderformer_amd.weights import synthetic_state_dict

    cfg = named_config(w.config)
    pipe = RenderFormerRenderingPipeline(RenderFormer(cfg, synthetic_state_dict(cfg, seed=0),
                                                      range_check="deferred")).to(dev)
    host = batch_scenes([synthetic_scene(w.tris, 1, seed=1)])
    b = {k: v.to(dev) for k, v in host.items() if k != "tex_channels"}
    pipe.model.plan_hint(b["mask"], host["mask"].numpy())
    cams = orbit(a.frames).to(dev)[None]                      # [1, frames, 4, 4]
    fov = b["fov"][:, :1].expand(1, a.frames, 1).contiguous()  # the scene's fov: vertical, of the frame height
    cam_list = [(cams[:, k:k + 1].contiguous(), fov[:, k:k + 1].contiguous()) for k in range(a.frames)]
    scene = pipe.encode(b["triangles"], b["texture"], b["mask"], b["vn"])

    def frames(hw, n):
        out = None
        for k in range(n):
            c, f = cam_list[k]
            out = pipe.render_encoded(scene, c, f, hw, torch_dtype=torch.bfloat16)
        return out

    for hw in SHAPES:  # warm-up: every shape
        out = frames(hw, min(a.warmup, a.frames))
        assert tuple(out.shape[2:4]) == hw
    torch.cuda.synchronize()
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    ms = {hw: [] for hw in SHAPES}
    for _ in range(a.blocks):
        for hw in SHAPES:
            e0, e1 = ev(), ev()
            e0.record()
            out = frames(hw, a.frames)
            e1.record()
            torch.cuda.synchronize()
            ms[hw].append(e0.elapsed_time(e1) / a.frames)
            if not torch.isfinite(out).all():
                raise RuntimeError(f"non-finite output at {_name(hw)}")
    pipe.check_range()
    med = {hw: statistics.median(v) for hw, v in ms.items()}
    wide, sq, big = SHAPES
    rec = {
        "metric": "ms per frame, render_encoded of one camera per call on an orbit, one encoded scene; median over "
                  "interleaved blocks",
        "config": w.config, "tris": w.tris, "device": torch.cuda.get_device_name(dev),
        "frames_per_block": a.frames, "blocks": a.blocks,
        "ms_per_frame": {_name(hw): round(med[hw], 4) for hw in SHAPES},
        "ray_tokens": {_name(hw): (hw[0] // cfg.patch_size) * (hw[1] // cfg.patch_size) for hw in SHAPES},
        "ratio_1024x576_over_768x768": round(med[wide] / med[sq], 4),
        "ratio_1024x576_over_1024x1024": round(med[wide] / med[big], 4),
        "ms_blocks": {_name(hw): [round(v, 4) for v in ms[hw]] for hw in SHAPES},
    }
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
