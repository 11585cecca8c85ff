#!/usr/bin/env python
"""What a displayed frame costs: the 8-bit display frame made on the device (pipe.to_ldr) against the HDR frame
copied to the host and tone-mapped there with numpy (images.hdr_to_ldr).

The bench's default workload (bench.py's own argument defaults and scene helpers: large-proxy, the 5,633-triangle
synthetic scene), encoded once (pipe.encode); every frame is a pipe.render_encoded(scene, c2w_k, fov_k, (H, W),
overscan=True) of the next camera on the orbit tools/camera_sweep.py uses, at 512 x 512 and 1920 x 1080.  A displayed
frame is one whose uint8 pixels are in host memory, so every route ends each frame with a copy into a pinned host
buffer and a wait for it, and is timed with the host clock around the block (the route (a) has host work in it):

  render  the frame alone and a wait for it (what the routes add to)
  a       the current route: the HDR frame (12 B / pixel) copied to the host, images.hdr_to_ldr of it there
  b       pipe.to_ldr(frame, "none") and the 3 B / pixel copy
  c       pipe.to_ldr(frame, "pbr_neutral") and the same copy

All routes of both sizes run in the same process in interleaved blocks (render a b c render a b c ...) after a
warm-up of every route.  The kernel's own time comes from the library's kernel timer (the dispatch packet's
timestamps, as a kernel trace reports it), once per timed block, on the frame that block rendered; its traffic is 15 B
per pixel (12 in, 3 out), reported as a share of the 8.0 TB/s HBM peak -- the frame was just written by the render
and is small enough to sit in the Infinity Cache, so the share is of the yardstick, not a claim of where the bytes
came from.  Prints ONE JSON line.

  python tools/ldr_frames.py [--frames 4] [--blocks 5] [--out profiles/ldr_frames.json]
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

import torch  # noqa: E402

import bench  # noqa: E402  (the workload's defaults; bench.py itself is not run)
from camera_sweep import orbit  # noqa: E402

SIZES = [(512, 512), (1080, 1920)]  # (H, W)
ROUTES = ("render", "a", "b", "c")
HBM_PEAK = 8.0e12  # B/s


def _name(hw) -> str:
    return f"{hw[1]}x{hw[0]}"  # width x height, as frame sizes are usually written


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=4, help="cameras per block")
    ap.add_argument("--blocks", type=int, default=5, help="interleaved blocks per route and size")
    ap.add_argument("--warmup", type=int, default=2, help="untimed frames per route and size before the first block")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("ldr_frames.py: no HIP device (a timing needs the GPU)", file=sys.stderr)
        return 2
    w = bench.parse([])  # the bench's default workload
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline, ops
    from renderformer_amd.config import named_config
    from renderformer_amd.images import hdr_to_ldr
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
    pin_hdr = {hw: torch.empty(1, 1, *hw, 3, dtype=torch.float32, pin_memory=True) for hw in SIZES}
    pin_ldr = {hw: torch.empty(1, 1, *hw, 3, dtype=torch.uint8, pin_memory=True) for hw in SIZES}
    dev_ldr = {hw: torch.empty(1, 1, *hw, 3, dtype=torch.uint8, device=dev) for hw in SIZES}
    stream = torch.cuda.current_stream(dev)

    def frames(hw, route, n):
        """n displayed frames of one route; returns the last HDR frame on the device"""
        out = None
        for k in range(n):
            c, f = cam_list[k]
            out = pipe.render_encoded(scene, c, f, hw, torch_dtype=torch.bfloat16, overscan=True)
            if route == "a":
                pin_hdr[hw].copy_(out, non_blocking=True)
                stream.synchronize()
                hdr_to_ldr(pin_hdr[hw].numpy())
            elif route in ("b", "c"):
                pipe.to_ldr(out, "none" if route == "b" else "pbr_neutral", out=dev_ldr[hw])
                pin_ldr[hw].copy_(dev_ldr[hw], non_blocking=True)
                stream.synchronize()
            else:
                stream.synchronize()
        return out

    def kernel_us(frame, mapper):
        t = ops.KernelTimer("ldr")
        t.start("ldr")
        ops.tonemap_ldr8(frame, mapper, out=dev_ldr[tuple(frame.shape[2:4])])
        torch.cuda.synchronize()
        return 1e3 * t.durations_ms()[0]

    cases = [(hw, r) for hw in SIZES for r in ROUTES]
    for hw, r in cases:  # warm-up: every route at every size
        out = frames(hw, r, min(a.warmup, a.frames))
        assert tuple(out.shape[2:4]) == hw
    for hw in SIZES:
        kernel_us(out.new_zeros(1, 1, *hw, 3), "none"), kernel_us(out.new_zeros(1, 1, *hw, 3), "pbr_neutral")
    torch.cuda.synchronize()
    ms = {c: [] for c in cases}
    kus = {(hw, m): [] for hw in SIZES for m in ("none", "pbr_neutral")}
    for _ in range(a.blocks):
        for hw, r in cases:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = frames(hw, r, a.frames)
            ms[(hw, r)].append(1e3 * (time.perf_counter() - t0) / a.frames)
            if r == "render":  # outside the timed window: the kernel alone, on the frame just rendered
                if not torch.isfinite(out).all():
                    raise RuntimeError(f"non-finite output at {_name(hw)}")
                for m in ("none", "pbr_neutral"):
                    kus[(hw, m)].append(kernel_us(out, m))
    pipe.check_range()
    med = {c: statistics.median(v) for c, v in ms.items()}
    kmed = {c: statistics.median(v) for c, v in kus.items()}
    rec = {
        "metric": "ms per displayed frame (uint8 pixels in pinned host memory), render_encoded of one camera per call "
                  "with overscan=True on an orbit, one encoded scene, host clock; median over interleaved blocks",
        "routes": {"render": "the frame and a wait for it", "a": "HDR copy to the host + images.hdr_to_ldr",
                   "b": "to_ldr none + uint8 copy", "c": "to_ldr pbr_neutral + uint8 copy"},
        "config": w.config, "tris": w.tris, "device": torch.cuda.get_device_name(dev),
        "frames_per_block": a.frames, "blocks": a.blocks,
        "ms_per_frame": {_name(hw): {r: round(med[(hw, r)], 4) for r in ROUTES} for hw in SIZES},
        "ms_blocks": {_name(hw): {r: [round(v, 4) for v in ms[(hw, r)]] for r in ROUTES} for hw in SIZES},
        "kernel_us": {_name(hw): {m: round(kmed[(hw, m)], 2) for m in ("none", "pbr_neutral")} for hw in SIZES},
        "kernel_us_blocks": {_name(hw): {m: [round(v, 2) for v in kus[(hw, m)]] for m in ("none", "pbr_neutral")}
                             for hw in SIZES},
        "kernel_share_of_hbm_peak_at_15_B_per_pixel": {
            _name(hw): {m: round(15.0 * hw[0] * hw[1] / (kmed[(hw, m)] * 1e-6) / HBM_PEAK, 4)
                        for m in ("none", "pbr_neutral")} for hw in SIZES},
    }
    for hw in SIZES:
        base = ms[(hw, "render")]
        rec[f"render_block_spread_{_name(hw)}"] = [round(min(base) / med[(hw, "render")], 4),
                                                   round(max(base) / med[(hw, "render")], 4)]
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
