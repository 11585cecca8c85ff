#!/usr/bin/env python
"""Cameras that arrive one at a time: a full render per camera against encode once + render_encoded per camera.

The bench's default workload (bench.py's own argument defaults and scene helpers: large-proxy, the 5,633-triangle
synthetic scene, 512^2, one view per call), with the camera moving along the orbit synthetic_scene places its views
on, one camera per call:

  A  pipe(triangles, texture, mask, vn, c2w_k, fov_k)        every call pays stage 1 and the K/V GEMM
  B  scene = pipe.encode(triangles, texture, mask, vn)        once per block
     pipe.render_encoded(scene, c2w_k, fov_k)                 per camera

Both modes run in the same process in interleaved blocks (A B A B ...) after a warm-up of every shape, each block
timed with a device event pair around its frames (the encode with a pair of its own) and no host wait inside (the
fp16 range check is deferred, as in bench.py, and read after the last block).  Prints ONE JSON line: the median over
blocks of the ms per frame of A and B, of the encode's ms, their ratio and the handle's bytes.

  python tools/camera_sweep.py [--frames 12] [--blocks 5] [--out profiles/encoded_scene_sweep.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import bench  # noqa: E402  (the workload's defaults; bench.py itself is not run)


def orbit(n: int):
    """n cameras on synthetic_scene's orbit (scenes.py), starting at the bench's own camera."""
    import numpy as np
    from renderformer_amd.scenes import look_at_to_c2w
    c2w = []
    for k in range(n):
        ang = 2 * math.pi * k / n
        c2w.append(look_at_to_c2w((2.0 * math.sin(ang), -2.0 * math.cos(ang), 0.3 * math.sin(3 * ang))))
    return torch.from_numpy(np.stack(c2w).astype(np.float32))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=12, help="cameras per block")
    ap.add_argument("--blocks", type=int, default=5, help="interleaved blocks per mode")
    ap.add_argument("--warmup", type=int, default=3, help="untimed frames per mode before the first block")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("camera_sweep.py: no HIP device (a timing needs the GPU)", file=sys.stderr)
        return 2
    w = bench.parse([])  # the bench's default workload
    res, views = w.res or 512, w.views or 1
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    from renderformer_amd.config import named_config
    from renderformer_amd.scenes import batch_scenes, synthetic_scene
    from renderformer_amd.weights import synthetic_state_dict

    cfg = named_config(w.config)
    pipe = RenderFormerRenderingPipeline(RenderFormer(cfg, synthetic_state_dict(cfg, seed=0),
                                                      range_check="deferred")).to(dev)
    host = batch_scenes([synthetic_scene(w.tris, views, seed=1)])
    b = {k: v.to(dev) for k, v in host.items() if k != "tex_channels"}
    pipe.model.plan_hint(b["mask"], host["mask"].numpy())
    cams = orbit(a.frames).to(dev)[None]                      # [1, frames, 4, 4]
    fov = b["fov"][:, :1].expand(1, a.frames, 1).contiguous()
    cam = lambda k: (cams[:, k:k + 1].contiguous(), fov[:, k:k + 1].contiguous())  # noqa: E731
    cam_list = [cam(k) for k in range(a.frames)]
    # the pipeline log-encodes the texture in place: every full render and every encode gets a fresh copy, staged
    # (and restored between blocks) outside the timed windows
    tex0 = b["texture"].clone()
    staged = [tex0.clone() for _ in range(a.frames + 1)]

    def restore():
        for t in staged:
            t.copy_(tex0)

    def mode_a(n):
        out = None
        for k in range(n):
            c, f = cam_list[k]
            out = pipe(b["triangles"], staged[k], b["mask"], b["vn"], c, f, resolution=res, torch_dtype=torch.bfloat16)
        return out

    def mode_b(scene, n):
        out = None
        for k in range(n):
            c, f = cam_list[k]
            out = pipe.render_encoded(scene, c, f, res, torch_dtype=torch.bfloat16)
        return out

    # warm-up: every shape of both modes, and the two modes' frames of one camera compared bit for bit
    n_w = min(a.warmup, a.frames)
    fa = mode_a(n_w)
    scene = pipe.encode(b["triangles"], staged[a.frames], b["mask"], b["vn"])
    fb = mode_b(scene, n_w)
    torch.cuda.synchronize()
    equal = bool(torch.equal(fa, fb))
    handle_bytes = int(scene.nbytes)
    del scene

    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    a_ms, b_ms, enc_ms = [], [], []
    for _ in range(a.blocks):
        restore()
        torch.cuda.synchronize()
        e0, e1 = ev(), ev()
        e0.record()
        mode_a(a.frames)
        e1.record()
        torch.cuda.synchronize()
        a_ms.append(e0.elapsed_time(e1) / a.frames)
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        scene = pipe.encode(b["triangles"], staged[a.frames], b["mask"], b["vn"])
        e1.record()
        out = mode_b(scene, a.frames)
        e2.record()
        torch.cuda.synchronize()
        enc_ms.append(e0.elapsed_time(e1))
        b_ms.append(e1.elapsed_time(e2) / a.frames)
        del scene
    pipe.check_range()
    if not torch.isfinite(out).all():
        raise RuntimeError("non-finite output")
    med = statistics.median
    rec = {
        "metric": "ms per frame, one camera per call on an orbit: full render (A) vs encode once + render_encoded (B)",
        "config": w.config, "tris": w.tris, "res": res, "device": torch.cuda.get_device_name(dev),
        "frames_per_block": a.frames, "blocks": a.blocks,
        "a_ms_per_frame": round(med(a_ms), 4), "b_ms_per_frame": round(med(b_ms), 4),
        "encode_ms": round(med(enc_ms), 4), "ratio_a_over_b": round(med(a_ms) / med(b_ms), 4),
        "handle_bytes": handle_bytes, "frames_bit_identical": equal,
        "a_ms_blocks": [round(v, 4) for v in a_ms], "b_ms_blocks": [round(v, 4) for v in b_ms],
        "encode_ms_blocks": [round(v, 4) for v in enc_ms],
    }
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
