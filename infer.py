"""Single-scene CLI, flag-compatible with the reference `infer.py:34-41`.

    python infer.py --h5_file scene.h5 [--model_id DIR|NAME] [--precision bf16|fp16|fp32]
                    [--resolution 512] [--height H] [--width W] [--output_dir DIR]
                    [--overscan] [--tone_mapper none|pbr_neutral] [--exposure STOPS] [--synthetic_seed S]

Reads the HDF5 scene with renderformer_amd.h5io (no h5py), renders every view on the HIP
device and writes `{base}_view_{i}.exr` (linear HDR) and `{base}_view_{i}.png` (clip to
[0, 1] x 255) like `infer.py:89-103`.  Offline additions: `--model_id` must be a local
snapshot directory (config.json + model.safetensors) unless `--synthetic_seed` is given, in
which case it names an architecture (e.g. renderformer-v1.1-swin-large) with deterministic
random weights.  `--height` / `--width` (each defaults to `--resolution`) render a
rectangular frame, e.g. `--height 576 --width 1024`; the scene's fov is the vertical field
of view of the frame height.  Each side must be a multiple of the model's frame unit (64 for the
released Swin models) unless `--overscan` is given, e.g. `--height 1080 --width 1920 --overscan`:
the padded frame (1088 rows) is rendered as a slightly wider view and the requested window
written.  `--tone_mapper pbr_neutral` (Khronos PBR Neutral + sRGB encode) and `--exposure`
(stops) make the PNG's 8-bit frame on the device (`pipeline.to_ldr`); 'agx' and 'filmic' need
the OCIO configs of `simple_ocio`, which are not available here, and are rejected.
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

from renderformer_amd import RenderFormerRenderingPipeline
from renderformer_amd.h5io import load_single_h5_data
from renderformer_amd.images import check_tone_mapper, hdr_to_ldr, write_exr, write_png

PRECISION = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}


def add_common_args(parser: argparse.ArgumentParser) -> None:
    parser.add_argument("--model_id", type=str, default="microsoft/renderformer-v1.1-swin-large",
                        help="Local snapshot directory, or an architecture name with --synthetic_seed")
    parser.add_argument("--precision", type=str, choices=["bf16", "fp16", "fp32"], default="fp16")
    parser.add_argument("--resolution", type=int, default=512)
    parser.add_argument("--height", type=int, default=None, help="Frame height in pixels (default: --resolution)")
    parser.add_argument("--width", type=int, default=None, help="Frame width in pixels (default: --resolution)")
    parser.add_argument("--overscan", action="store_true",
                        help="Render any frame size (e.g. --height 1080 --width 1920): the frame padded to multiples "
                             "of the model's frame unit is rendered and the requested window returned")
    parser.add_argument("--tone_mapper", type=str, choices=["none", "agx", "filmic", "pbr_neutral"], default="none")
    parser.add_argument("--exposure", type=float, default=0.0,
                        help="Exposure of the PNG frames in stops (the frame is scaled by 2^exposure; default 0)")
    parser.add_argument("--save_gbuffer", action="store_true",
                        help="Also write each view's geometry buffers (pipeline.gbuffer): <name>_alpha.png, "
                             "<name>_depth.exr (one channel, +inf where nothing is hit), <name>_normal.exr, "
                             "<name>_albedo.exr")
    parser.add_argument("--synthetic_seed", type=int, default=None,
                        help="(offline) random-init weights of the named architecture")


def frame_resolution(args):
    """The pipeline's ``resolution`` for the parsed flags: --height / --width, each defaulting to --resolution; a
    square frame stays the reference's int."""
    h = args.resolution if args.height is None else args.height
    w = args.resolution if args.width is None else args.width
    return h if h == w else (h, w)


def load_pipeline(args) -> RenderFormerRenderingPipeline:
    try:
        check_tone_mapper(args.tone_mapper)
    except ValueError as e:  # agx / filmic: LUT transforms of simple_ocio's OCIO configuration
        raise SystemExit(str(e))
    model_id = args.model_id
    if args.synthetic_seed is not None and model_id.startswith("microsoft/"):
        model_id = model_id.split("/", 1)[1]
    # "lazy" fp16 range check: the CLIs resolve each frame where they wait for its copy anyway (infer.py: before
    # reading it; batch_infer.py: before the D2H of the next batch), so render never blocks their pipelining
    pipe = RenderFormerRenderingPipeline.from_pretrained(model_id, synthetic_seed=args.synthetic_seed,
                                                         range_check="lazy")
    return pipe.to("cuda")


def device_ldr(args) -> bool:
    """Do the parsed flags ask for display frames made on the device (pipeline.to_ldr)?  Not with the defaults
    (--tone_mapper none --exposure 0): then the PNG is hdr_to_ldr of the host frame, as the reference writes it."""
    return args.tone_mapper != "none" or getattr(args, "exposure", 0.0) != 0.0


def save_views(hdr: torch.Tensor, output_dir: str, base_name: str, stages=None, ldr=None) -> list:
    """hdr [nv, H, W, 3] -> {base}_view_{i}.exr / .png (infer.py:89-103).  `stages`: batch_infer.StageTimes.
    `ldr` uint8 [nv, H, W, 3] (tensor or array): the PNG frames, written in place of hdr_to_ldr(hdr[i])."""
    paths = []
    for i in range(hdr.shape[0]):
        img = hdr[i].cpu().numpy().astype("float32")
        hdr_path = os.path.join(output_dir, f"{base_name}_view_{i}.exr")
        ldr_path = os.path.join(output_dir, f"{base_name}_view_{i}.png")

        def to_ldr():
            if ldr is None:
                return hdr_to_ldr(img)
            return ldr[i].cpu().numpy() if isinstance(ldr, torch.Tensor) else ldr[i]

        if stages is None:
            write_exr(hdr_path, img)
            write_png(ldr_path, to_ldr())
        else:
            stages.timed("write: EXR", write_exr, hdr_path, img)
            stages.timed("write: PNG", lambda: write_png(ldr_path, to_ldr()))
        paths += [hdr_path, ldr_path]
    return paths


def save_gbuffer(gb, output_dir: str, base_name: str) -> list:
    """One scene's GBuffer fields ([nv, H, W(, 3)], tensors or arrays) -> {base}_view_{i}_alpha.png, _depth.exr (one
    channel, misses +inf), _normal.exr, _albedo.exr, beside save_views' files."""
    host = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else t  # noqa: E731
    alpha, depth, normal, albedo = host(gb.alpha), host(gb.depth), host(gb.normal), host(gb.albedo)
    paths = []
    for i in range(depth.shape[0]):
        stem = os.path.join(output_dir, f"{base_name}_view_{i}")
        write_png(stem + "_alpha.png", alpha[i])
        write_exr(stem + "_depth.exr", depth[i])
        write_exr(stem + "_normal.exr", normal[i])
        write_exr(stem + "_albedo.exr", albedo[i])
        paths += [stem + "_alpha.png", stem + "_depth.exr", stem + "_normal.exr", stem + "_albedo.exr"]
    return paths


GBUFFER_FILES = ("alpha", "depth", "normal", "albedo")  # (the triangle id has no image file)


def main(argv=None):
    parser = argparse.ArgumentParser(description="Infer using triangle radiosity transformer model (MI355X)")
    parser.add_argument("--h5_file", type=str, required=True, help="Path to the input H5 file")
    parser.add_argument("--output_dir", type=str, required=False, help="Output directory (default: next to the H5)")
    add_common_args(parser)
    args = parser.parse_args(argv)

    pipeline = load_pipeline(args)
    data = load_single_h5_data(args.h5_file)
    dev = pipeline.device
    triangles = data["triangles"].unsqueeze(0).to(dev)
    texture = data["texture"].unsqueeze(0).to(dev)
    mask = data["mask"].unsqueeze(0).to(dev)
    vn = data["vn"].unsqueeze(0).to(dev)
    c2w = data["c2w"].unsqueeze(0).to(dev)
    fov = data["fov"].unsqueeze(0).unsqueeze(-1).to(dev)
    imgs = pipeline(triangles=triangles, texture=texture, mask=mask, vn=vn, c2w=c2w, fov=fov,
                    resolution=frame_resolution(args), torch_dtype=PRECISION[args.precision], overscan=args.overscan)
    pipeline.resolve(imgs)  # the frame's fp16 range check (re-rendered in place if it overflowed) before reading it
    # the display frames of a tone mapper / exposure are made on the device, after the frame's resolve
    ldr = pipeline.to_ldr(imgs, args.tone_mapper, args.exposure).cpu() if device_ldr(args) else None
    print("Inference completed. Rendered images shape:", imgs.shape)
    output_dir = args.output_dir if args.output_dir else os.path.dirname(os.path.abspath(args.h5_file))
    os.makedirs(output_dir, exist_ok=True)
    base = os.path.splitext(os.path.basename(args.h5_file))[0]
    for p in save_views(imgs[0], output_dir, base, ldr=None if ldr is None else ldr[0]):
        print(f"Saved {p}")
    if args.save_gbuffer:
        gb = pipeline.gbuffer(triangles, texture, mask, vn, c2w, fov, frame_resolution(args), overscan=args.overscan,
                              outputs=GBUFFER_FILES)
        for p in save_gbuffer(type(gb)(*(None if t is None else t[0] for t in gb)), output_dir, base):
            print(f"Saved {p}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
