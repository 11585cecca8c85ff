"""Pinhole intrinsics and overscan on the device: rf_ray_tokens_cam, the windowed output kernels and the pipeline.

The fixtures (tests/golden/cam_*.npz, make_golden_cam.py) are the reference model's own fp32 CPU output on a ray map
of the PADDED frame, cropped to the requested window.  The bars are the project's, taken from
test_rect_frames_gpu.py: HDR relative L2 < 1e-3, and per view the deviation from the mean within a quarter of what
separates two views of the fixture's scene.  Everything that is defined as "the same computation" (the fov mode
against rf_ray_tokens_hw, a window against a shifted principal point, an overscanned frame against the padded render
cropped, an encoded scene or one view at a time against the plain render) is compared bit for bit.
"""
import functools
import json

import numpy as np
import pytest
import torch

from golden_util import load_case, rel_l2, rel_l2_ac

pytestmark = pytest.mark.gpu
dev = "cuda"
HDR_TOL = 1e-3  # the project's bar (test_rect_frames_gpu.HDR_TOL)
PATCH = 8
CAM_CASES = ["cam_swin_45x99", "cam_swin_fov_44x100", "cam_full_20x44"]
K_CASES = ["cam_swin_45x99", "cam_full_20x44"]  # the fixtures rendered from off-axis intrinsics


@functools.lru_cache(maxsize=None)
def _case(name):
    cfg, sd, inp, _, z = load_case(name)
    return cfg, sd, inp, z


def _layout(z):
    """(H, W, Hp, Wp, y0, x0) as the fixture records them"""
    return tuple(int(v) for v in (*z["frame_hw"], *z["padded_hw"], *z["origin"]))


def _pipeline(cfg, sd, **kw):
    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    return RenderFormerRenderingPipeline(RenderFormer(cfg, sd, **kw)).to(dev)


def _inputs(inp):
    """fresh device copies (render log-encodes the texture in place)"""
    return {k: v.clone().to(dev) for k, v in inp.items()}


def _K(z, shift=(0, 0)):
    """the fixture's intrinsics [B, V, 4] on the device, the principal point moved by shift = (y, x) pixels"""
    return (torch.from_numpy(z["intrinsics"]) + torch.tensor([0.0, 0.0, shift[1], shift[0]])).contiguous().to(dev)


def _render(pipe, d, resolution, **kw):
    fov = None if "intrinsics" in kw else d["fov"]
    return pipe(d["triangles"], d["texture"], d["mask"], d["vn"], d["c2w"], fov, resolution=resolution,
                torch_dtype=torch.bfloat16, **kw)


def _camera_kw(z):
    """how the fixture's camera is passed: its intrinsics, or (the fov case) nothing besides the scenes' fov"""
    return {} if bool(z["uses_fov"]) else {"intrinsics": _K(z)}


def _host_tokens(rays, patch=PATCH):
    """'b (h1 p1) (w1 p2) c -> (b h1 w1) (c p1 p2)' of rays [P, H, W, 3]"""
    P, H, W, _ = rays.shape
    return rays.reshape(P, H // patch, patch, W // patch, patch, 3).permute(0, 1, 3, 5, 2, 4).reshape(
        P * (H // patch) * (W // patch), 3 * patch * patch)


def _tokens_cam(c2w, fov, K, frame, res, origin, dtype):
    from renderformer_amd import ops
    P = c2w.shape[0]
    tok = torch.zeros(P * (res[0] // PATCH) * (res[1] // PATCH), 3 * PATCH * PATCH, dtype=dtype, device=dev)
    rpos = torch.full((P, 9), 7.0, device=dev)
    ops.ray_tokens_cam(c2w, fov, K, frame, res, origin, PATCH, tok, rpos)
    return tok, rpos


def _world_cameras(name):
    """the fixture's world-frame cameras (real rotations) [P, 4, 4] and fov [P]"""
    inp = _case(name)[2]
    return (inp["c2w"].reshape(-1, 4, 4).float().contiguous().to(dev),
            inp["fov"].reshape(-1).float().contiguous().to(dev))


def _check_hdr(name, got, z):
    """the two bounds of a rendered frame [B, V, H, W, 3] against the fixture's (full) cropped HDR frame"""
    H, W = _layout(z)[:2]
    assert tuple(got.shape) == (2, 2, H, W, 3) and got.dtype == torch.float32 and got.is_contiguous()
    g = got.cpu()
    ref = torch.from_numpy(z["hdr"])
    err = rel_l2(g, ref)
    acs = [rel_l2_ac(g[:, v], ref[:, v]) for v in range(ref.shape[1])]
    sep = float(z["view01_rel_l2_ac"])
    print(f"{name}: HDR rel L2 {err:.3e} (bar {HDR_TOL}); per view deviation from the mean "
          f"{', '.join(f'{a:.3e}' for a in acs)} (bar 0.25 x {sep:.3e} = {0.25 * sep:.3e})")
    assert torch.isfinite(got).all()
    assert err < HDR_TOL
    for v, a in enumerate(acs):
        assert a <= 0.25 * sep, v


# ------------------------------------------------------------------------------------------------ 1-3. ray tokens
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_ray_tokens_cam_in_fov_mode_are_ray_tokens_hw_bits(dtype):
    from renderformer_amd import ops
    c2w, fov = _world_cameras("cam_swin_fov_44x100")
    P = c2w.shape[0]
    tok, rpos = _tokens_cam(c2w, fov, None, (64, 128), (64, 128), (0, 0), dtype)
    ref = torch.zeros_like(tok)
    ref_pos = torch.zeros_like(rpos)
    ops.ray_tokens(c2w, fov, (64, 128), PATCH, ref, ref_pos)
    assert ref.float().abs().sum() > 0
    assert torch.equal(tok, ref) and torch.equal(rpos, ref_pos)
    assert torch.equal(rpos.view(P, 3, 3)[:, 0], c2w[:, :3, 3])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("name", CAM_CASES)
def test_ray_tokens_cam_match_the_fixture_rays(name, dtype):
    """rf_ray_tokens_cam of the padded frame (window origin and camera as the fixture's: intrinsics, or fov for the fov
    case) against the fixture's rays_d (camera frame: c2w = identity) patchified on the host and rounded to the
    operand type.  The bar and its reasoning are test_ray_tokens_hw_match_the_fixture_rays': the device and the host
    round the fp32 direction differently by a few fp32 ulps, so a value may land on the other side of a rounding
    boundary of the 16-bit type: at most ONE 16-bit ulp below 1.0, for far fewer than 1 % of the values."""
    cfg, sd, inp, z = _case(name)
    H, W, Hp, Wp, y0, x0 = _layout(z)
    img = int(z["rays_image"])
    ref = _host_tokens(torch.from_numpy(z["rays_d"]).reshape(1, Hp, Wp, 3)).to(dtype)
    eye = torch.eye(4).reshape(1, 4, 4).contiguous().to(dev)
    if bool(z["uses_fov"]):
        fov, K = inp["fov"].reshape(-1)[img:img + 1].float().contiguous().to(dev), None
    else:
        fov, K = None, _K(z).reshape(-1, 4)[img:img + 1].contiguous()
    tok, rpos = _tokens_cam(eye, fov, K, (H, W), (Hp, Wp), (y0, x0), dtype)
    diff = (tok.float().cpu() - ref.float()).abs()
    ulp = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
    print(f"{name} {dtype}: max |diff| {diff.max():.3e} (one ulp {ulp:.3e}), differing "
          f"{float((diff > 0).float().mean()):.2e}")
    assert diff.max() <= ulp
    assert (diff > 0).float().mean() < 1e-2
    assert torch.equal(rpos.cpu(), torch.zeros(1, 9))  # the camera origin, three times


@pytest.mark.parametrize("name", K_CASES)
def test_a_window_is_a_shifted_principal_point(name):
    """cx, cy are multiples of 0.25, so (x - x0) + 0.5 - cx and x + 0.5 - (cx + x0) are both exact in fp32: the
    tokens of (K, y0, x0) are the tokens of the padded frame's own camera K + (0, 0, x0, y0), bit for bit."""
    z = _case(name)[3]
    H, W, Hp, Wp, y0, x0 = _layout(z)
    c2w, _ = _world_cameras(name)
    win, _ = _tokens_cam(c2w, None, _K(z).reshape(-1, 4), (H, W), (Hp, Wp), (y0, x0), torch.float16)
    own, _ = _tokens_cam(c2w, None, _K(z, (y0, x0)).reshape(-1, 4), (Hp, Wp), (Hp, Wp), (0, 0), torch.float16)
    assert win.float().abs().sum() > 0 and torch.equal(win, own)
    off, _ = _tokens_cam(c2w, None, _K(z).reshape(-1, 4), (H, W), (Hp, Wp), (y0, x0 - 1), torch.float16)
    assert not torch.equal(off, own)  # and the origin matters


# ------------------------------------------------------------------------------------------------ 4. output windows
@functools.lru_cache(maxsize=None)
def _logits():
    g = torch.Generator(device="cpu").manual_seed(7)
    return (torch.randn(2, 3, 24, 40, generator=g) * 1.5).to(dev)  # both ELU branches


@pytest.mark.parametrize("log_decode", [True, False])
@pytest.mark.parametrize("channels_last", [True, False])
def test_hdr_output_window_is_the_slice_of_hdr_output(channels_last, log_decode):
    from renderformer_amd import ops
    x = _logits()
    n, c, h, w = x.shape
    full = torch.zeros((n, h, w, c) if channels_last else (n, c, h, w), device=dev)
    ops.hdr_output(x, full, 1e-3, log_decode, channels_last)

    def window(y0, x0, oh, ow):
        out = torch.full((n, oh, ow, c) if channels_last else (n, c, oh, ow), -7.0, device=dev)
        ops.hdr_output_window(x, out, (y0, x0, oh, ow), 1e-3, log_decode, channels_last)
        ref = full[:, y0:y0 + oh, x0:x0 + ow] if channels_last else full[:, :, y0:y0 + oh, x0:x0 + ow]
        return out, ref
    out, ref = window(0, 0, h, w)
    assert torch.equal(out, full) and ref.shape == full.shape
    out, ref = window(5, 3, 13, 31)
    assert torch.equal(out, ref)
    out, ref = window(h - 1, w - 1, 1, 1)  # the last pixel
    assert torch.equal(out, ref)
    with pytest.raises(ValueError, match="must lie inside"):
        ops.hdr_output_window(x, out, (h - 1, w - 1, 1, 2), 1e-3, log_decode, channels_last)


def test_frame_window_is_the_slice_of_the_frames():
    from renderformer_amd import ops
    frames = _logits().permute(0, 2, 3, 1).contiguous()  # [2, 24, 40, 3]
    for y0, x0, oh, ow in ((0, 0, 24, 40), (5, 3, 13, 31), (23, 39, 1, 1), (2, 0, 20, 40)):
        out = ops.frame_window(frames, (y0, x0, oh, ow))
        assert out.is_contiguous() and torch.equal(out, frames[:, y0:y0 + oh, x0:x0 + ow])
    with pytest.raises(ValueError, match="must lie inside"):
        ops.frame_window(frames, (5, 3, 20, 31))


# ------------------------------------------------------------------------------------------------ 5-8. pipeline
@pytest.mark.parametrize("name", CAM_CASES)
def test_pipeline_renders_the_camera_fixture(name):
    cfg, sd, inp, z = _case(name)
    pipe = _pipeline(cfg, sd)
    out = _render(pipe, _inputs(inp), _layout(z)[:2], overscan=True, **_camera_kw(z))
    _check_hdr(name, out, z)


def test_fov_equivalent_intrinsics_render_the_fov_fixture():
    name = "cam_swin_fov_44x100"
    cfg, sd, inp, z = _case(name)
    out = _render(_pipeline(cfg, sd), _inputs(inp), _layout(z)[:2], overscan=True, intrinsics=_K(z))
    _check_hdr(name + " (intrinsics)", out, z)


def test_overscan_is_the_padded_render_cropped():
    cfg, sd, inp, z = _case("cam_swin_45x99")
    H, W, Hp, Wp, y0, x0 = _layout(z)
    pipe = _pipeline(cfg, sd)
    over = _render(pipe, _inputs(inp), (H, W), overscan=True, intrinsics=_K(z))
    padded = _render(pipe, _inputs(inp), (Hp, Wp), intrinsics=_K(z, (y0, x0)))
    assert tuple(padded.shape) == (2, 2, Hp, Wp, 3)
    assert torch.equal(over, padded[:, :, y0:y0 + H, x0:x0 + W])


def test_overscan_of_a_frame_of_whole_units_changes_nothing():
    cfg, sd, inp, z = _case("cam_swin_fov_44x100")
    pipe = _pipeline(cfg, sd)
    plain = _render(pipe, _inputs(inp), (64, 128))
    assert torch.equal(_render(pipe, _inputs(inp), (64, 128), overscan=True), plain)
    assert torch.isfinite(plain).all() and tuple(plain.shape) == (2, 2, 64, 128, 3)


@pytest.mark.parametrize("name", K_CASES)
def test_render_encoded_and_view_chunks_give_the_same_bits(name):
    cfg, sd, inp, z = _case(name)
    hw = _layout(z)[:2]
    pipe = _pipeline(cfg, sd)
    full = _render(pipe, _inputs(inp), hw, overscan=True, intrinsics=_K(z))
    d = _inputs(inp)
    scene = pipe.encode(d["triangles"], d["texture"], d["mask"], d["vn"])
    enc = pipe.render_encoded(scene, d["c2w"], None, hw, intrinsics=_K(z), overscan=True)
    assert enc.shape == full.shape and torch.equal(enc, full)
    chunked = _pipeline(cfg, sd, view_chunk=1)
    assert torch.equal(_render(chunked, _inputs(inp), hw, overscan=True, intrinsics=_K(z)), full)
    d = _inputs(inp)
    scene = chunked.encode(d["triangles"], d["texture"], d["mask"], d["vn"])
    assert torch.equal(chunked.render_encoded(scene, d["c2w"], None, hw, intrinsics=_K(z), overscan=True), full)


# ------------------------------------------------------------------------------------------------ 9. range guard
def test_range_guard_rerenders_an_overscanned_frame():
    """The overflowing checkpoint of test_range_guard_rerenders_a_rectangular_frame at 44 x 100 with overscan: the
    "sync" render notices, renders the frame again with bf16 operands and returns the WINDOW of that frame, the bits
    of a model built with those operands; a "lazy" model re-renders in place into the windowed tensor."""
    from renderformer_amd.model import PrecisionWarning
    cfg, sd, inp, z = _case("cam_swin_fov_44x100")
    big = dict(sd)
    for k in ("transformer.layers.0.ffn.w1.weight", "transformer.layers.0.ffn.w3.weight"):
        big[k] = big[k] * 2000.0
    pipe = _pipeline(cfg, big)
    with pytest.warns(PrecisionWarning, match="fp16 operand overflow"):
        out = _render(pipe, _inputs(inp), (44, 100), overscan=True)
    assert tuple(out.shape) == (2, 2, 44, 100, 3) and torch.isfinite(out).all()
    m = pipe.model
    assert m.range_fallbacks == 1 and m.operands == "bf16"
    ref = _render(_pipeline(cfg, big, operands="bf16", dpt_precision=m.dpt_precision), _inputs(inp), (44, 100),
                  overscan=True)
    assert torch.equal(ref, out)
    lazy = _pipeline(cfg, big, range_check="lazy")
    d = _inputs(inp)  # (kept unmodified until the frame is resolved)
    out2 = _render(lazy, d, (44, 100), overscan=True)
    with pytest.warns(PrecisionWarning, match="fp16 operand overflow"):
        assert lazy.resolve(out2) is True
    assert tuple(out2.shape) == (2, 2, 44, 100, 3) and torch.equal(out2, ref)


# ------------------------------------------------------------------------------------------------ 10. CLI
def test_infer_cli_writes_an_overscanned_frame(tmp_path):
    import infer
    from safetensors.torch import save_file

    from renderformer_amd import h5io
    from renderformer_amd.images import hdr_to_ldr, read_exr, read_png
    cfg, sd, inp, z = _case("cam_swin_fov_44x100")
    snap = tmp_path / "snap"
    snap.mkdir()
    (snap / "config.json").write_text(json.dumps(cfg.to_dict()))
    save_file({k: v.contiguous() for k, v in sd.items()}, str(snap / "model.safetensors"))
    m = inp["mask"][0].numpy().astype(bool)
    h5 = tmp_path / "cam.h5"
    h5io.write_scene(str(h5), inp["triangles"][0].numpy()[m], inp["vn"][0].numpy()[m],
                     inp["texture"][0].numpy()[m].astype(np.float32), inp["c2w"][0].numpy(),
                     inp["fov"][0].numpy().reshape(-1), texture_dtype=np.float32)
    out = tmp_path / "out"
    args = ["--h5_file", str(h5), "--model_id", str(snap), "--height", "44", "--width", "100", "--output_dir", str(out)]
    with pytest.raises(ValueError, match="height 44"):  # without the flag: the present error
        infer.main(args)
    assert infer.main(args + ["--overscan"]) == 0
    for i in range(2):
        hdr = read_exr(str(out / f"cam_view_{i}.exr"))
        assert hdr.shape == (44, 100, 3)
        assert rel_l2(hdr, z["hdr"][0, i]) < HDR_TOL
        png = read_png(str(out / f"cam_view_{i}.png"))
        assert png.shape[:2] == (44, 100)
        np.testing.assert_array_equal(png, hdr_to_ldr(hdr))
