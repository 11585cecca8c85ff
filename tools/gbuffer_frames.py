#!/usr/bin/env python
"""What the geometry buffers cost beside a frame: pipe.gbuffer_encoded after pipe.render_encoded.

The bench's default workload (bench.py's own argument defaults and scene helpers: large-proxy, the 5,633-triangle
synthetic scene), encoded once (pipe.encode); every frame is a pipe.render_encoded(scene, c2w_k, fov_k, (H, W),
overscan=True) of the next camera on the orbit tools/camera_sweep.py uses, at 512 x 512 and 1920 x 1080, ended by a
wait for the stream and timed with the host clock around the block:

  render  the frame alone
  all     the frame, then gbuffer_encoded of the same camera, every buffer
  adi     the frame, then gbuffer_encoded(outputs=("alpha", "depth", "tri_id")): no barycentrics, no shading launch

All routes of both sizes run in one process in interleaved blocks (render all adi render all adi ...) after a warm-up
of every route.  The two ops' own times (ops.primary_hits: the setup and the trace launch; ops.gbuffer_shade) are
taken with device events round REPS back-to-back calls, outside the timed blocks, for both ways the trace kernel can
read its records (RF_VIS_STAGE=1: staged in LDS, 0: scalar loads; the library reads the knob per call).  The pair rate
is H W n_triangles / the primary_hits time; against it stands the derived per-pair work of the trace loop, 9 FMAs
(three edge functions), a 3-operand min, a 3-operand max, one min and one compare: 13 VALU instructions, and the
part's issue peak for unpacked fp32 instructions, 256 CUs x 64 lanes x 2.4 GHz = 39.3 T lane-instructions / s (half
the 157 TF vector peak, which counts packed FMAs).  The kernels' own durations come from a
`rocprofv3 --kernel-trace --stats` run of `--profile` (a short run of the `all` route).  Prints ONE JSON line.

  python tools/gbuffer_frames.py [--frames 4] [--blocks 5] [--out profiles/gbuffer_frames.json]
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
ROUTES = ("render", "all", "adi")
ADI = ("alpha", "depth", "tri_id")
VALU_PER_PAIR = 13
VALU_ISSUE_PEAK = 256 * 64 * 2.4e9  # lane-instructions / s, unpacked fp32
REPS = 10


def _name(hw) -> str:
    return f"{hw[1]}x{hw[0]}"  # width x height, as frame sizes are usually written


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=4, help="cameras per block")
    ap.add_argument("--blocks", type=int, default=5, help="interleaved blocks per route and size")
    ap.add_argument("--warmup", type=int, default=2, help="untimed frames per route and size before the first block")
    ap.add_argument("--profile", action="store_true", help="a short run of the `all` route only, for a kernel trace")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("gbuffer_frames.py: no HIP device (a timing needs the GPU)", file=sys.stderr)
        return 2
    w = bench.parse([])  # the bench's default workload
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline, ops
    from renderformer_amd.config import named_config
    from renderformer_amd.gbuffer import scene_tables
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
    stream = torch.cuda.current_stream(dev)

    def frames(hw, route, n):
        """n frames of one route; returns the last HDR frame and G-buffer"""
        out = gb = None
        for k in range(n):
            c, f = cam_list[k]
            out = pipe.render_encoded(scene, c, f, hw, torch_dtype=torch.bfloat16, overscan=True)
            if route != "render":
                gb = pipe.gbuffer_encoded(scene, c, f, hw, overscan=True, outputs=None if route == "all" else ADI)
            stream.synchronize()
        return out, gb

    if a.profile:
        for hw in SIZES:
            frames(hw, "all", a.frames)
        torch.cuda.synchronize()
        pipe.check_range()
        print(json.dumps({"profile": "all", "frames": a.frames, "sizes": [_name(hw) for hw in SIZES]}))
        return 0

    tris = b["triangles"].reshape(1, -1, 9).float().contiguous()
    vn = b["vn"].reshape(1, -1, 9).float().contiguous()
    tables = scene_tables(host["mask"].numpy(), dev)
    n_tris = tables[2]

    def op_us(hw, stage):
        """(primary_hits with bary, without, gbuffer_shade) microseconds per call: REPS calls between two events"""
        os.environ["RF_VIS_STAGE"] = str(stage)
        c, f = cam_list[0]
        res = []
        hits = None
        for kind in ("hits", "hits_adi", "shade"):
            for timed in (False, True):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(REPS if timed else 2):
                    if kind == "shade":
                        ops.gbuffer_shade(hits["tri_id"], hits["bary"], vn, b["texture"], normal=True, albedo=True)
                    else:
                        r = ops.primary_hits(tris, *tables, c.float().contiguous(), f.float().contiguous(), None, hw,
                                             bary=kind == "hits", alpha=True)
                        hits = r if kind == "hits" else hits
                e1.record(stream)
                e1.synchronize()
            res.append(1e3 * e0.elapsed_time(e1) / REPS)
        del os.environ["RF_VIS_STAGE"]
        return res

    cases = [(hw, r) for hw in SIZES for r in ROUTES]
    covered = {}
    for hw, r in cases:  # warm-up: every route at every size
        out, gb = frames(hw, r, min(a.warmup, a.frames))
        assert tuple(out.shape[2:4]) == hw
        if r == "all":
            assert tuple(gb.normal.shape[2:]) == hw + (3,)
            covered[_name(hw)] = round(float((gb.alpha == 255).float().mean()), 4)
    torch.cuda.synchronize()
    ms = {c: [] for c in cases}
    ops_us = {(hw, s): [] for hw in SIZES for s in (1, 0)}
    for _ in range(a.blocks):
        for hw, r in cases:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, _gb = frames(hw, r, a.frames)
            ms[(hw, r)].append(1e3 * (time.perf_counter() - t0) / a.frames)
            if r == "render":  # outside the timed window: the ops alone, both ways of reading the records
                if not torch.isfinite(out).all():
                    raise RuntimeError(f"non-finite output at {_name(hw)}")
                for s in (1, 0):
                    ops_us[(hw, s)].append(op_us(hw, s))
    pipe.check_range()
    med = {c: statistics.median(v) for c, v in ms.items()}
    omed = {c: [statistics.median(x[i] for x in v) for i in range(3)] for c, v in ops_us.items()}
    stage_name = {1: "lds", 0: "scalar"}
    rec = {
        "metric": "ms per frame, render_encoded of one camera per call with overscan=True on an orbit, one encoded "
                  "scene, alone and followed by gbuffer_encoded of the same camera; host clock round blocks that end "
                  "each frame with a stream wait; median over interleaved blocks",
        "routes": {"render": "the frame alone", "all": "the frame + every buffer",
                   "adi": "the frame + alpha, depth, tri_id"},
        "config": w.config, "tris": n_tris, "device": torch.cuda.get_device_name(dev),
        "frames_per_block": a.frames, "blocks": a.blocks, "covered_pixels": covered,
        "ms_per_frame": {_name(hw): {r: round(med[(hw, r)], 4) for r in ROUTES} for hw in SIZES},
        "ms_blocks": {_name(hw): {r: [round(v, 4) for v in ms[(hw, r)]] for r in ROUTES} for hw in SIZES},
        "added_ms": {_name(hw): {r: round(med[(hw, r)] - med[(hw, "render")], 4) for r in ("all", "adi")}
                     for hw in SIZES},
        "op_us": {_name(hw): {stage_name[s]: dict(zip(("primary_hits", "primary_hits_no_bary", "gbuffer_shade"),
                                                      (round(v, 2) for v in omed[(hw, s)]))) for s in (1, 0)}
                  for hw in SIZES},
        "op_us_blocks": {_name(hw): {stage_name[s]: [[round(v, 2) for v in x] for x in ops_us[(hw, s)]]
                                     for s in (1, 0)} for hw in SIZES},
        "valu_instructions_per_pair_derived": VALU_PER_PAIR,
        "valu_issue_peak_lane_instructions_per_s": VALU_ISSUE_PEAK,
    }
    rec["pairs_per_s"] = {}
    rec["share_of_valu_issue_peak"] = {}
    for hw in SIZES:
        pairs = hw[0] * hw[1] * n_tris
        rec["pairs_per_s"][_name(hw)] = {stage_name[s]: round(pairs / (omed[(hw, s)][0] * 1e-6), 0) for s in (1, 0)}
        rec["share_of_valu_issue_peak"][_name(hw)] = {
            stage_name[s]: round(VALU_PER_PAIR * pairs / (omed[(hw, s)][0] * 1e-6) / VALU_ISSUE_PEAK, 4)
            for s in (1, 0)}
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
