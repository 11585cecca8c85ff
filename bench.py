"""Headline benchmark: rendered frames/s at 512x512, RenderFormer-V1.1-swin-large (proxy shape), cbox.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload cbox|c4|c5] [--dump-outputs DIR] [--full] ...

Workloads (all synthetic, seeded, inputs resident in HBM before the timed region):

* ``cbox`` (default, BASELINE config 2; weak scaling): one step = every rank renders ``--scenes`` cbox-sized
  scenes (N = 5,633 triangles) x ``--views`` views at 512x512 through the drop-in pipeline (texture/vn
  encoders, stage 1 (14 layers), ray tokens, stage 2 (10 layers, Swin), DPT, HDR decode); with N > 1 ranks
  the finished HDR frames are all-gathered to every rank over RCCL (xGMI) inside the timed region.
* ``c4`` (BASELINE config 4; strong scaling): one step = 64 scenes cycling through the reference's 16 example
  scenes (examples/*.json converted to HDF5 by renderformer_amd.examples before the timed region, read back
  with the HDF5 reader), assigned to ranks by longest-processing-time on the FLOP model (parallel.assign_units),
  frames all-gathered.
* ``c5`` (BASELINE config 5's shape; strong scaling): one step = ONE scene with ``--views`` views (default 24)
  at ``--res`` (default 1024), the views split across ranks (parallel.shard_views; stage 1 recomputed on each
  rank), frames all-gathered.

Multi-GPU: one process per GPU.  Under ``torch.distributed.run`` the env (RANK/WORLD_SIZE/...) is read and
``--gpus`` must equal WORLD_SIZE; run directly with ``--gpus N > 1`` this script starts
``torch.distributed.run --nproc-per-node N`` itself (before any GPU call) and exits with its status.

A plain run sets up, warms up, times the ``--steps`` steps, writes the last step's frames when ``--dump-outputs
DIR`` is given (``DIR/frames.npy``, float32; inputs and weights are seeded, so two builds can be compared frame
for frame) and prints one JSON line.  The line carries ``ms_per_step`` and a roofline object for the dominant
kernel (stage-1 attention), each of its launches in the last timed step timed by HIP events that its own
dispatch packet timestamps (hipExtLaunchKernel; no run of its own).

``--full`` adds what takes work of its own after the timed region: the parity of the last GPU frame against the
reference (the committed reference-generated fixture when the workload is that fixture's, and the oracle frame
of the CPU baseline), and the CPU baseline itself: the oracle restatement of the reference (oracle/rf_ref.py,
PyTorch CPU fp32) on a bounded sample of the same workload, rank 0 at N = 1 only.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

import torch  # noqa: E402  (importing torch does not initialise the GPU)
import torch.distributed as dist  # noqa: E402

METRIC = "rendered frames/sec at 512×512, renderformer-v1.1-swin-large, 1/2/4/8 MI355X"
PEAK_BF16_TFLOPS = 2500.0  # MI355X dense bf16 MFMA (MI355X_MICROARCH.md, chip-level parameters)
PEAK_FP8_TFLOPS = 5000.0   # MI355X dense fp8 MFMA (same table)
DOMINANT = "attn_stage1"   # largest single kernel family by time in the rocprof summary (profiles/)
FIXTURE = ("large", 5633, 512, 1, 1, 1)  # tests/golden/large_cbox_r512.npz: config, N, res, views, scenes, seed


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", choices=["cbox", "c4", "c5"], default="cbox")
    ap.add_argument("--config", default="large")
    ap.add_argument("--tris", type=int, default=5633)
    ap.add_argument("--res", type=int, default=None, help="default 512 (1024 for c5)")
    ap.add_argument("--views", type=int, default=None, help="default 1 (24 for c5)")
    ap.add_argument("--scenes", type=int, default=1, help="cbox: scenes per rank per step; c4: scenes per step")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region also run what the headline figure does not need: the parity of the "
                         "last frame against the reference fixture, the CPU baseline and the parity against its frame")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="rank 0 writes the frames of the last timed step to DIR/frames.npy (float32; a fixed seeded "
                         "sample of the values, DIR/frames_sample.npy, when they exceed 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--cpu-frames", type=int, default=3)
    ap.add_argument("--profile", action="store_true", help="short run for rocprofv3 (no cpu baseline)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (gloo: CPU-side tests)")
    ap.add_argument("--same-device", action="store_true", help="every rank on cuda:0 (1-GPU rehearsal)")
    ap.add_argument("--dump", default=None, help="rank 0 saves the gathered frames of the last step (.npy)")
    ap.add_argument("--view-chunk", type=int, default=None,
                    help="stage 2 + DPT over at most this many views per pass (c5 default: 3 when views % 24 == 0, "
                         "else 1, so a view's image does not depend on the rank split; all views otherwise)")
    ap.add_argument("--fp8", action="store_true", help="opt-in fp8 mode: the stage-2 cross-attention Q and FFN W2 as "
                                                        "MX fp8 GEMMs (the subset inside the 1e-3 bar); roofline then "
                                                        "reports the stage-2 W2 fp8 GEMM")
    a = ap.parse_args(argv)
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if a.res is None:
        a.res = 1024 if a.workload == "c5" else 512
    if a.views is None:
        a.views = 24 if a.workload == "c5" else 1
    if a.workload == "c4" and a.scenes == 1:
        a.scenes = 64
    if a.view_chunk is None and a.workload == "c5":
        # fixed chunks make a view's image independent of the rank split; 3 views per pass (1024^2: 49k ray
        # tokens per GEMM) when every rank of a 1/2/4/8-GPU run holds whole chunks of the 24 views
        a.view_chunk = 3 if a.views % 24 == 0 else 1
    return a


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(args) -> int:
    """--gpus N > 1 without a torch.distributed.run environment: start one process per GPU as a child
    (this process has not touched the GPU) and return its exit status."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd)


def cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(cfg, sd, batch, res, frames):
    """Reference CPU path (oracle restatement, fp32) on this host's cores: median of `frames` after 1 warm-up,
    with the per-stage split of the same frames.  Returns (record, last oracle frame)."""
    from oracle import rf_ref
    threads = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    try:  # honour a cgroup CPU quota (the GPU box exposes 256 CPUs but grants 16)
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            threads = min(threads, max(1, int(int(q) / int(p))))
    except Exception:
        pass
    torch.set_num_threads(threads)
    times, splits, out = [], [], None
    for i in range(frames + 1):
        tex = batch["texture"].clone()
        rf_ref.STAMPS = st = {}
        t0 = time.perf_counter()
        out = rf_ref.render(sd, cfg, batch["triangles"], tex, batch["mask"], batch["vn"], batch["c2w"], batch["fov"],
                            res)
        t1 = time.perf_counter()
        rf_ref.STAMPS = None
        if i > 0:
            times.append(t1 - t0)
            splits.append({"prologue+stage1": st["stage1_end"] - t0, "stage2": st["stage2_end"] - st["stage1_end"],
                           "dpt+decode": t1 - st["stage2_end"]})
    t = statistics.median(times)
    split = {k: round(statistics.median(s[k] for s in splits), 3) for k in splits[0]}
    n_frames = int(batch["c2w"].shape[0] * batch["c2w"].shape[1])
    rec = {"value": round(n_frames / t, 5), "unit": "frames/s", "cores": threads, "kind": "port",
           "sample": f"{frames} render(s) of the same workload ({n_frames} frame(s) each; median after 1 warm-up), "
                     f"oracle/rf_ref.py fp32, torch {torch.__version__}, {threads} threads",
           "cpu_model": cpu_model(), "s_per_frame": round(t / n_frames, 3), "s_per_stage": split}
    return rec, out


def fixture_parity(args, frame):
    """rel L2 of the GPU frame against the reference-generated fixture when the workload is the fixture's."""
    if (args.config, args.tris, args.res, args.views, args.scenes, 1) != FIXTURE or args.workload != "cbox":
        return None
    path = os.path.join(REPO, "tests", "golden", "large_cbox_r512.npz")
    if not os.path.exists(path):
        return None
    import numpy as np
    ref = torch.from_numpy(np.load(path)["hdr"]).double()
    got = frame.detach().double().cpu().reshape(ref.shape)
    return float((got - ref).norm() / ref.norm())


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(directory, frames):
    """--dump-outputs: what a caller of the timed path receives from its last step, the gathered HDR frames
    [frames, res, res, channels], as float32 in DIR/frames.npy; past 64 MB a fixed seeded sample of the
    flattened values (the same positions on every run of the same arguments) in DIR/frames_sample.npy."""
    import numpy as np
    os.makedirs(directory, exist_ok=True)
    arr = frames.detach().to(torch.float32).cpu().contiguous().numpy()
    if arr.nbytes <= DUMP_LIMIT_BYTES:
        np.save(os.path.join(directory, "frames.npy"), arr)
        return
    flat = arr.reshape(-1)
    pos = np.sort(np.random.default_rng(0).choice(flat.size, DUMP_LIMIT_BYTES // 8, replace=False))
    np.save(os.path.join(directory, "frames_sample.npy"), flat[pos])


def main():
    args = parse()
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        return launch_ranks(args)
    world = int(env_world or "1")
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        return 2
    dev_index = 0 if args.same_device else local
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.backend)

    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline, ops
    from renderformer_amd.config import named_config
    from renderformer_amd.flops import frame_flops
    from renderformer_amd.parallel import FrameGather, PendingFrames, assign_units, max_over_ranks, scene_cost, shard_views
    from renderformer_amd.scenes import batch_scenes, synthetic_scene
    from renderformer_amd.weights import synthetic_state_dict

    cfg = named_config(args.config)
    sd = synthetic_state_dict(cfg, seed=0)
    # fp16 range check deferred: no per-frame host wait in the timed loop; checked once after it (check_range)
    pipe = RenderFormerRenderingPipeline(RenderFormer(cfg, sd, fp8=args.fp8, view_chunk=args.view_chunk,
                                                      range_check="deferred")).to(dev)

    # ---- the units of one step: (batch tensors on the device, global frame ids)
    if args.workload == "cbox":
        scenes = [synthetic_scene(args.tris, args.views, seed=1 + rank * args.scenes + i) for i in range(args.scenes)]
        hosts = [batch_scenes(scenes)]
        n_per_rank = args.scenes * args.views
        rank_ids = [list(range(r * n_per_rank, (r + 1) * n_per_rank)) for r in range(world)]
        n_frames_step = n_per_rank * world
        scaling = "weak"
    elif args.workload == "c4":
        # the reference's 16 example scenes (examples/*.json), converted to HDF5 by the package's converter
        # (cached; before the timed region) and read back with the HDF5 reader, cycled to --scenes
        from renderformer_amd.examples import convert_all, example_names
        from renderformer_amd.h5io import load_single_h5_data
        names = example_names()
        if world > 1:  # rank 0 converts (8 processes), the others wait and then only find the cached files
            if rank == 0:
                convert_all(names, workers=8)
            dist.barrier()
        files = convert_all(names, workers=8 if world == 1 else 1)
        step_names = [names[i % len(names)] for i in range(args.scenes)]
        scene_data = {n: load_single_h5_data(files[n]) for n in set(step_names)}
        counts = [int(scene_data[n]["triangles"].shape[0]) for n in step_names]
        costs = [scene_cost(cfg, n, args.views, args.res) for n in counts]
        plan = assign_units(costs, world)
        mine = plan[rank]
        hosts = []
        for i in mine:
            d = scene_data[step_names[i]]
            nv = int(d["c2w"].shape[0])
            vsel = [v % nv for v in range(args.views)]  # --views views of the scene's cameras (cycled)
            hosts.append({"triangles": d["triangles"][None], "texture": d["texture"][None], "mask": d["mask"][None],
                          "vn": d["vn"][None], "c2w": d["c2w"][vsel][None], "fov": d["fov"][vsel].reshape(1, -1, 1)})
        rank_ids = [[i * args.views + v for i in plan[r] for v in range(args.views)] for r in range(world)]
        n_frames_step = args.scenes * args.views
        scaling = "strong"
    else:  # c5
        sc = synthetic_scene(args.tris, args.views, seed=1)
        shards = shard_views(args.views, world)
        vr = shards[rank]
        sc.c2w, sc.fov = sc.c2w[vr.start:vr.stop], sc.fov[vr.start:vr.stop]
        hosts = [batch_scenes([sc])] if len(vr) else []
        rank_ids = [list(r) for r in shards]
        n_frames_step = args.views
        scaling = "strong"
    batches = [{k: v.to(dev) for k, v in h.items() if k != "tex_channels"} for h in hosts]
    for b, h in zip(batches, hosts):  # plans from the host masks: a new scene never reads its mask back
        pipe.model.plan_hint(b["mask"], h["mask"].numpy() if torch.is_tensor(h["mask"]) else h["mask"])
    tex0 = [b["texture"][:, :, -3:].clone() for b in batches]
    # the pipeline log-encodes the 3 emission channels in place (reference semantics): every step gets a
    # fresh input texture staged in HBM before the timed region (or, past 32 GiB of copies, the emission
    # channels are restored inside the step, which is then timed with that copy)
    n_in = args.warmup + args.steps
    tex_bytes = sum(b["texture"].numel() * 4 for b in batches)
    staged = ([[b["texture"].clone() for b in batches] for _ in range(n_in)] if n_in * tex_bytes <= (32 << 30)
              else None)
    calls = [0]
    chans = 4 if cfg.include_alpha else 3
    frame_shape = (args.res, args.res, chans)
    # finished frames to every rank: ONE RCCL all_gather per step with the static per-rank counts / ids above (no
    # host sync), issued asynchronously so it overlaps the next step's launches (parallel.FrameGather)
    gather = FrameGather(rank_ids, frame_shape, dev) if world > 1 else None

    def step():
        frames = []
        for j, b in enumerate(batches):
            if staged is not None:
                tex = staged[calls[0] % n_in][j]
            else:
                tex = b["texture"]
                tex[:, :, -3:].copy_(tex0[j])
            out = pipe(b["triangles"], tex, b["mask"], b["vn"], b["c2w"], b["fov"], resolution=args.res,
                       torch_dtype=torch.bfloat16)
            frames.append(out.reshape(-1, *frame_shape))
        calls[0] += 1
        if len(frames) == 1:
            local = frames[0]
        else:
            local = torch.cat(frames) if frames else torch.empty((0,) + frame_shape, device=dev)
        if world > 1:  # finished frames to every rank (RCCL all_gather over xGMI), completed by .result()
            return gather.start(local)
        return PendingFrames(out=local)

    for _ in range(args.warmup):
        step().result()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    # the dominant kernel's launches in the LAST timed step are dispatched with a start/stop HIP event pair
    # that the dispatch packet itself timestamps (librfhip's kernel timer, hipExtLaunchKernel): the kernel's
    # own duration, as rocprofv3 reports it (round 1 bracketed the launch with two marker events instead,
    # which added ~11-20 us of queue time per launch to the measured duration)
    timer = ops.KernelTimer("gemm_w2_stage2" if args.fp8 else DOMINANT)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    pend = None
    for i in range(args.steps):
        if i == args.steps - 1:
            ops.TIMER = timer
        nxt = step()
        if pend is not None:  # the previous step's gather ran beside this step's launches; the stream waits for it
            pend.result()
        pend = nxt
    out = pend.result()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    ops.TIMER = None
    pipe.check_range()  # every timed frame has completed: raise if one overflowed fp16 (DeviceError)
    elapsed = max_over_ranks(elapsed, device=dev if args.backend == "nccl" else None)
    if not torch.isfinite(out).all():
        raise RuntimeError("non-finite output")

    total_frames = n_frames_step * args.steps
    fps = total_frames / elapsed
    if args.workload == "cbox":
        fl_frame = frame_flops(cfg, args.tris, args.res, args.views)["total"] / args.views
        fl_step = fl_frame * n_frames_step
    elif args.workload == "c4":
        fl_step = sum(frame_flops(cfg, n, args.res, args.views)["total"] for n in counts)
    else:
        fl_step = frame_flops(cfg, args.tris, args.res, args.views)["total"] * world  # stage 1 on every rank
    durs = timer.durations_ms()
    per_step_launches = len(durs)  # one timed step
    kern_ms = statistics.mean(durs) if durs else float("nan")
    s_len = (args.tris if args.workload != "c4" else max(counts)) + cfg.num_register_tokens
    scenes_per_launch = args.scenes if args.workload == "cbox" else 1
    kern_flops = 4 * s_len * s_len * cfg.latent_dim * scenes_per_launch  # QK^T + PV per launch
    if args.workload == "c4":  # launches differ in S: use the mean algorithmic FLOP of this rank's scenes
        ss = [int(b["mask"].sum()) + cfg.num_register_tokens for b in batches]
        kern_flops = 4 * cfg.latent_dim * statistics.mean(s * s for s in ss) if ss else 0
    if args.fp8:  # the fp8 roofline object: stage-2 FFN W2 GEMM, 2 M N K per launch, vs the fp8 peak
        rows = sum(int(b["c2w"].shape[0] * b["c2w"].shape[1]) for b in batches) * (args.res // cfg.patch_size) ** 2
        if args.view_chunk:  # one launch per chunk of views
            rows = rows * args.view_chunk // max(1, sum(int(b["c2w"].shape[0] * b["c2w"].shape[1]) for b in batches))
        kern_flops = 2 * rows * cfg.view_transformer_ffn_hidden_dim * cfg.view_transformer_latent_dim
    achieved = kern_flops / (kern_ms * 1e-3) / 1e12 if durs else float("nan")
    # roofline.traffic: the stage-1 attention's HBM bytes per launch from the rocprofv3 FETCH_SIZE / WRITE_SIZE
    # passes (tools/gpu.sh round -> tools/pmc_traffic.py), reported only when that record was taken on the
    # attention sources of this tree (digest match); otherwise null with the reason
    traffic, traffic_src = None, None
    tpath = os.path.join(REPO, "profiles", "attn_stage1_traffic.json")
    if os.path.exists(tpath) and args.workload == "cbox" and args.scenes == 1:
        from renderformer_amd._lib import ATTN_SOURCES, source_digest
        try:
            trec = json.load(open(tpath))
            if trec.get("source_digest") == source_digest(*ATTN_SOURCES):
                traffic = int(trec["hbm_bytes_per_launch"])
                traffic_src = (f"profiles/attn_stage1_traffic.json (rocprofv3 FETCH_SIZE x2 + WRITE_SIZE passes on "
                               f"attention sources {trec['source_digest']}, this tree's)")
            else:
                traffic_src = "stale: profiles/attn_stage1_traffic.json was measured on other attention sources"
        except Exception as e:
            traffic_src = f"unreadable: {e}"

    if args.dump and rank == 0:
        import numpy as np
        np.save(args.dump, out.cpu().numpy())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, out)
    if rank == 0:
        if args.workload == "cbox":
            wl = (f"cbox-sized scene N={args.tris}, {args.res}x{args.res}, {args.views} view(s) x {args.scenes} "
                  f"scene(s) per rank per step")
        elif args.workload == "c4":
            wl = (f"{args.scenes} scenes per step cycling through the reference's 16 example scenes "
                  f"(examples/*.json -> HDF5, N {min(counts)}..{max(counts)}), {args.res}x{args.res}, "
                  f"{args.views} view(s) each, LPT-sharded over ranks")
        else:
            wl = (f"one scene N={args.tris}, {args.views} views at {args.res}x{args.res} per step, views split over "
                  f"ranks (stage 1 on every rank; stage 2 + DPT {args.view_chunk} view(s) per pass)")
        rec = {
            "metric": METRIC, "value": round(fps, 4), "unit": "frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True,
            "scaling": scaling, "vs_baseline": None, "dtype": "fp16+bf16+fp8" if args.fp8 else "fp16+bf16",
            "data": ("the reference's example scenes (examples/*.json -> HDF5), synthetic weights" if args.workload == "c4"
                     else "synthetic"),
            "config": {
                "workload": f"{'large-proxy' if args.config == 'large' else args.config} {wl}",
                "model": "renderformer-v1.1-swin-large" if args.config == "large" else args.config,
                "model_shape": f"D={cfg.latent_dim} H={cfg.num_heads} L1={cfg.num_layers} "
                               f"L2={cfg.view_transformer_n_layers} F={cfg.dim_feedforward} swin="
                               f"{cfg.view_transformer_use_swin_attn} dpt={cfg.dpt_features}/{cfg.dpt_out_channels}",
                "global_batch": n_frames_step, "seq_len": s_len, "res": args.res,
                "parallelism": f"dp{world}" + ("" if args.workload != "c5" else " (views)"),
                "gather": "one async RCCL all_gather of the HDR frames per step (static counts, overlaps the next step)"
                          if world > 1 and args.backend == "nccl" else
                          (f"{args.backend} all_gather" if world > 1 else "none (1 rank)"),
                "weights": "synthetic seed 0 (no checkpoint offline)",
                "precision": ("stage-2 cross-attention Q and FFN W2 MX fp8 (e4m3, E8M0 per 32) on bf16 operands, "
                              if args.fp8 else "fp16 projection operands, ") +
                             "bf16 attention q/k/v, fp32 accumulate/softmax/residual; DPT fp16 operands, fp32 accumulate",
            },
            "frame": {
                "gflop_per_step": round(fl_step / 1e9, 1),
                "tflops_effective": round(fl_step * args.steps / elapsed / world / 1e12, 1),
                "mfma_frac_bf16_peak": round(fl_step * args.steps / elapsed / world / 1e12 / PEAK_BF16_TFLOPS, 4),
            },
            "roofline": {
                "kernel": ("rf_gemm_mx8 — stage-2 FFN W2 projection, MX fp8 (e4m3 + E8M0 per 32)" if args.fp8 else
                           "rf_attn_fwd — stage-1 triangle self-attention (attn_sk_kernel: stream-K, in-kernel merge)"),
                "bound": "mfma", "achieved": round(achieved, 1),
                "peak": PEAK_FP8_TFLOPS if args.fp8 else PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                "frac": round(achieved / (PEAK_FP8_TFLOPS if args.fp8 else PEAK_BF16_TFLOPS), 4),
                "traffic": None if args.fp8 else traffic,
                "traffic_source": None if args.fp8 else traffic_src,
                "avg_launch_ms": round(kern_ms, 4), "launches_per_step": per_step_launches,
                "timing": "hipExtLaunchKernel start/stop events on the launch stream (dispatch-packet timestamps)",
                "algorithmic_flop_per_launch": kern_flops,
                # Q, K, V read once + O written once (bf16); traffic above this = K/V re-reads + split partials
                "algorithmic_bytes_per_launch": 4 * s_len * cfg.latent_dim * 2 * scenes_per_launch,
            },
            "parity": {"vs_reference_fixture_rel_l2": None, "vs_oracle_rel_l2": None},
            "cpu_baseline": None,
        }
        if args.full and args.workload == "cbox":
            fp = fixture_parity(args, out[:n_per_rank])
            rec["parity"]["vs_reference_fixture_rel_l2"] = None if fp is None else float(f"{fp:.3e}")
        if (args.full and world == 1 and args.workload == "cbox" and not args.no_cpu_baseline
                and not args.profile):
            cpu_batch = {k: v for k, v in hosts[0].items() if k != "tex_channels"}
            rec["cpu_baseline"], ref = cpu_baseline(cfg, sd, cpu_batch, args.res, args.cpu_frames)
            got = out.detach().double().cpu().reshape(ref.shape)
            rec["parity"]["vs_oracle_rel_l2"] = float(f"{float((got - ref.double()).norm() / ref.double().norm()):.3e}")
        print(json.dumps(rec), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
