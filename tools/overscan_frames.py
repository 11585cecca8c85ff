#!/usr/bin/env python
"""What overscan costs: a standard frame size rendered with overscan=True against the native padded frame it runs as.

The bench's default workload (bench.py's own argument defaults and scene helpers: large-proxy, the 5,633-triangle
synthetic scene), encoded once (pipe.encode); every frame is a pipe.render_encoded(scene, c2w_k, fov_k, (H, W)) of the
next camera on the orbit tools/camera_sweep.py uses.  Pairs (requested with overscan, native):

  1280 x 720   overscan -> 768 x 1280 tokens' worth of work   against   1280 x 768   native
  1920 x 1080  overscan -> 1088 x 1920                        against   1920 x 1088  native

The two frames of a pair launch the same transformer and DPT kernels on the same shapes; the overscanned one runs
rf_ray_tokens_cam in place of rf_ray_tokens_hw and one more small launch, rf_frame_window, that copies the requested
window out of the padded frame.  So the expectation is a ratio of 1 within the spread of the native frame's own blocks,
which the record carries (min / max over the native blocks, relative to their median) as the yardstick.

All shapes run in the same process in interleaved blocks (A B C D A B C D ...) after a warm-up of every shape, each
block timed with a device event pair around its frames and no host wait inside (the fp16 range check is deferred, as
in bench.py, and read after the last block).  Prints ONE JSON line.

  python tools/overscan_frames.py [--frames 4] [--blocks 5] [--out profiles/overscan_frames.json]
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

PAIRS = [((720, 1280), (768, 1280)), ((1080, 1920), (1088, 1920))]  # ((H, W) with overscan, native (H', W'))


def _name(hw) -> str:
    return f"{hw[1]}x{hw[0]}"  # width x height, as frame sizes are usually written


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=4, help="cameras per block")
    ap.add_argument("--blocks", type=int, default=5, help="interleaved blocks per shape")
    ap.add_argument("--warmup", type=int, default=2, help="untimed frames per shape before the first block")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("overscan_frames.py: no HIP device (a timing needs the GPU)", file=sys.stderr)
        return 2
    w = bench.parse([])  # the bench's default workload
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    from renderformer_amd.config import named_config
    from renderformer_amd.model import frame_layout
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
    for over, native in PAIRS:  # a pair is a pair only if the overscanned frame runs as the native one
        assert frame_layout(cfg, over, True)[2:4] == native == frame_layout(cfg, native)[:2]
    shapes = [(hw, flag) for over, native in PAIRS for hw, flag in ((over, True), (native, False))]

    def frames(hw, overscan, n):
        out = None
        for k in range(n):
            c, f = cam_list[k]
            out = pipe.render_encoded(scene, c, f, hw, torch_dtype=torch.bfloat16, overscan=overscan)
        return out

    for hw, flag in shapes:  # warm-up: every shape
        out = frames(hw, flag, min(a.warmup, a.frames))
        assert tuple(out.shape[2:4]) == hw
    torch.cuda.synchronize()
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    ms = {s: [] for s in shapes}
    for _ in range(a.blocks):
        for s in shapes:
            e0, e1 = ev(), ev()
            e0.record()
            out = frames(*s, a.frames)
            e1.record()
            torch.cuda.synchronize()
            ms[s].append(e0.elapsed_time(e1) / a.frames)
            if not torch.isfinite(out).all():
                raise RuntimeError(f"non-finite output at {_name(s[0])}")
    pipe.check_range()
    med = {s: statistics.median(v) for s, v in ms.items()}
    key = lambda s: _name(s[0]) + ("_overscan" if s[1] else "")  # noqa: E731
    rec = {
        "metric": "ms per frame, render_encoded of one camera per call on an orbit, one encoded scene; median over "
                  "interleaved blocks",
        "config": w.config, "tris": w.tris, "device": torch.cuda.get_device_name(dev),
        "frames_per_block": a.frames, "blocks": a.blocks,
        "ms_per_frame": {key(s): round(med[s], 4) for s in shapes},
        "ms_blocks": {key(s): [round(v, 4) for v in ms[s]] for s in shapes},
    }
    for over, native in PAIRS:
        so, sn = (over, True), (native, False)
        rec[f"ratio_{_name(over)}_overscan_over_{_name(native)}"] = round(med[so] / med[sn], 4)
        rec[f"native_block_spread_{_name(native)}"] = [round(min(ms[sn]) / med[sn], 4), round(max(ms[sn]) / med[sn], 4)]
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
