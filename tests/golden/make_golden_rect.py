"""Generate the rectangular-frame fixtures (``rect_*.npz``) by running the *reference* RenderFormer on CPU fp32.

Run in the build container only (the reference checkout does not exist on the GPU box):
``python tests/golden/make_golden_rect.py [case ...]``.  Like ``make_golden.py`` it imports the reference package
read-only (``RF_REFERENCE``) with the ``roma`` stand-in in ``tests/golden/shim`` and
``ATTN_IMPL=sdpa``, loads the build-defined synthetic weights with ``load_state_dict(strict=True)`` and writes data
only.

The reference's ``RenderFormer.forward`` takes ray maps ``[B, V, H, W, 3]`` of any H x W; only its ``RayGenerator``
and ``pipeline.render(resolution: int)`` are square.  So each case builds the inputs the way ``make_golden.run_case``
does for ``tiny_swin`` (scenes of [61, 45] triangles, padding 64, 2 views), does what the reference pipeline does in
front of the model (log-encodes the emission channels, moves the triangles to camera space with the reference's
``trans_to_cam_coord``), generates the rays with ``rect_rays`` below and calls the reference model in fp32.

Camera convention (``rect_rays``): ``fov`` is the vertical field of view of the full frame height;
f = H / 2 / tan(fov / 2) pixels, cx = W / 2, cy = H / 2, pixel centres at +0.5, directions
((x - cx) / f, -(y - cy) / f, -1) rotated by R and L2-normalised.  With H == W this is the reference's formula.

Each fixture records cfg, weight seed and checksums, the inputs (HDF5 tensor format, as ``golden_util.load_case``
reads them), ``frame_hw`` = (H, W), the model inputs ``rays_o`` / ``rays_d`` / ``tris_cam``, the intermediate taps
``tap_enc_out``, ``tap_dec{i}``, ``tap_dpt``, the HDR frame (10^x - 1 of the output, channels last) and
``view01_rel_l2_ac``.  To keep every file below the repository's 1 MiB limit the decoder taps are a second file
(``<name>_taps.npz``, the images ``DEC_IMAGES``) and ``tap_dpt`` / the HDR frame keep every ``PIX_SUB``-th pixel row
and column of every image.
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
# make_golden sets the stage on import: ATTN_IMPL=sdpa, the roma shim, the reference checkout (RF_REFERENCE) and the
# repository on sys.path
from make_golden import HERE, TINY, weight_checksums  # noqa: E402

import torch  # noqa: E402

from renderformer_amd.config import RenderFormerConfig  # noqa: E402
from renderformer_amd.scenes import batch_scenes, synthetic_scene  # noqa: E402

SWIN = dict(TINY, view_transformer_use_swin_attn=True)
FULL = dict(TINY, view_transformer_use_swin_attn=False)
NTRIS, PAD, NVIEWS = [61, 45], 64, 2

CASES = {
    # name: (config overrides, (H, W), weight seed, scene seed)
    "rect_swin_64x128": (SWIN, (64, 128), 5, 21),
    "rect_swin_128x64": (SWIN, (128, 64), 6, 22),
    "rect_swin_64x192": (SWIN, (64, 192), 7, 23),   # three windows, 24 patches wide: not a power of two
    "rect_full_64x128": (FULL, (64, 128), 8, 24),
}
# The decoder-layer taps [B*V, R, D] are the bulk of a case (3 MiB at 64 x 192): they go to a file of their own,
# <name>_taps.npz, for the images (b * V + v) listed here: the second view of scene 1, whose rows sit behind every
# other image's (the decoder and the DPT head treat every image alike).
DEC_IMAGES = [3]
# tap_dpt and the HDR frame are recorded every PIX_SUB-th pixel row and column, offset PIX_OFF (as
# make_golden.HDR_SUB does for the big cases), together with the whole HDR frame's sum and sum of squares
PIX_SUB, PIX_OFF = 2, 1


def rect_rays(c2w, fov_rad, h, w):
    """(rays_o [..., 3], rays_d [..., h, w, 3]) for c2w [..., 4, 4] and the vertical fov [..., 1] in radians."""
    ys, xs = torch.meshgrid(torch.arange(h, dtype=c2w.dtype) + 0.5, torch.arange(w, dtype=c2w.dtype) + 0.5,
                            indexing="ij")
    f = h / 2 / torch.tan(0.5 * fov_rad[..., 0, None, None])
    lead = (1,) * (c2w.dim() - 2)
    xs, ys = xs.reshape(*lead, h, w), ys.reshape(*lead, h, w)
    dx = (xs - w / 2) / f
    dy = -(ys - h / 2) / f
    dirs = torch.stack([dx, dy, -torch.ones_like(dx)], dim=-1)
    rot = c2w[..., :3, :3]
    rays_d = torch.sum(dirs[..., None, :] * rot[..., None, None, :, :], dim=-1)
    return c2w[..., :3, 3], torch.nn.functional.normalize(rays_d, dim=-1, p=2)


def run_case(name, over, hw, wseed, sseed):
    from renderformer.models.config import RenderFormerConfig as RefConfig
    from renderformer.models.renderformer import RenderFormer as RefModel
    from renderformer.utils.transform import trans_to_cam_coord

    h, w = hw
    cfg = RenderFormerConfig(**over)
    from renderformer_amd.weights import synthetic_state_dict
    sd = synthetic_state_dict(cfg, seed=wseed)
    model = RefModel(RefConfig(**over))
    model.load_state_dict(sd, strict=True)
    model.eval()

    scenes = [synthetic_scene(n, NVIEWS, seed=sseed + i) for i, n in enumerate(NTRIS)]
    batch = batch_scenes(scenes, padding_length=PAD)
    t0 = time.time()
    tex = batch["texture"].clone()
    tex[:, :, -3:] = torch.log10(tex[:, :, -3:] + 1.0)
    c2w, tris = batch["c2w"], batch["triangles"]
    bs, nv = c2w.shape[:2]
    assert cfg.turn_to_cam_coord and not cfg.use_ldr
    tris_cam, c2w_cam, _ = trans_to_cam_coord(c2w.reshape(-1, 4, 4), torch.repeat_interleave(tris, nv, dim=0))
    tris_cam = tris_cam.reshape(bs, nv, -1, 9)
    rays_o, rays_d = rect_rays(c2w_cam.reshape(bs, nv, 4, 4), batch["fov"] / 180.0 * torch.pi, h, w)

    got = {}
    hooks = [model.transformer.register_forward_hook(lambda m, a, o: got.__setitem__("enc_out", o.clone()))]
    for i, layer in enumerate(model.view_transformer.transformer.layers):
        hooks.append(layer.register_forward_hook(lambda m, a, o, i=i: got.__setitem__(f"dec{i}", o.clone())))
    hooks.append(model.view_transformer.out_dpt.register_forward_hook(
        lambda m, a, o: got.__setitem__("dpt", o.clone())))
    with torch.no_grad():
        out = model(tris.reshape(bs, -1, 9), tex, batch["mask"], batch["vn"].reshape(bs, -1, 9), rays_o=rays_o,
                    rays_d=rays_d, tri_vpos_view_tf=tris_cam, tf32_view_tf=False)
    for hk in hooks:
        hk.remove()
    assert tuple(out.shape) == (bs, nv, 3, h, w) and torch.isfinite(out).all()
    hdr = torch.pow(10.0, out.permute(0, 1, 3, 4, 2)) - 1.0

    names, sums = weight_checksums(sd)
    sl = slice(PIX_OFF, None, PIX_SUB)
    h64 = hdr.double()
    a, b = h64[0, 1], h64[0, 0]
    rec = dict(
        cfg=json.dumps(cfg.to_dict()), weight_seed=np.int64(wseed), weight_names=np.array(names), weight_sums=sums,
        res=np.int64(max(h, w)), frame_hw=np.array([h, w], dtype=np.int64),
        triangles=tris.numpy(), vn=batch["vn"].numpy(), tex_channels=batch["tex_channels"].numpy(),
        mask=batch["mask"].numpy(), c2w=c2w.numpy(), fov=batch["fov"].numpy(),
        rays_o=rays_o.numpy().astype(np.float32), rays_d=rays_d.numpy().astype(np.float32),
        tris_cam=tris_cam.numpy().astype(np.float32),
        tap_enc_out=got["enc_out"].numpy().astype(np.float32),
        dec_images=np.array(DEC_IMAGES, dtype=np.int64),
        pix_sub=np.array([PIX_SUB, PIX_OFF], dtype=np.int64),
        tap_dpt=got["dpt"][:, :, sl, sl].numpy().astype(np.float32),
        hdr=hdr[:, :, sl, sl].numpy().astype(np.float32),
        hdr_sum=np.float64(h64.sum()), hdr_sumsq=np.float64((h64 ** 2).sum()),
        view01_rel_l2_ac=np.float64((a - b).norm() / (b - b.mean()).norm()),
    )
    taps = {f"tap_dec{i}": got[f"dec{i}"][DEC_IMAGES].numpy().astype(np.float32)
            for i in range(cfg.view_transformer_n_layers)}
    path, tpath = os.path.join(HERE, f"{name}.npz"), os.path.join(HERE, f"{name}_taps.npz")
    np.savez_compressed(path, **rec)
    np.savez_compressed(tpath, dec_images=rec["dec_images"], **taps)
    print(f"{name}: {time.time() - t0:.1f} s, out {tuple(out.shape)} hdr range [{hdr.min():.3g}, {hdr.max():.3g}], "
          f"view01_rel_l2_ac {float(rec['view01_rel_l2_ac']):.3g} -> {os.path.getsize(path) / 2**20:.3f} + "
          f"{os.path.getsize(tpath) / 2**20:.3f} MiB")


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    only = sys.argv[1:]
    for name, args in CASES.items():
        if not only or name in only:
            run_case(name, *args)
