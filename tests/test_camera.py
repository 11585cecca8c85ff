"""Pinhole intrinsics and overscan, host side (no GPU): the frame layout, the argument checks of the render entry
points, the CLI flag and the fixture generator's ray arithmetic."""
import argparse
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from renderformer_amd.config import RenderFormerConfig  # noqa: E402

TINY = dict(latent_dim=256, num_layers=2, num_heads=2, dim_feedforward=512, view_transformer_latent_dim=256,
            view_transformer_ffn_hidden_dim=512, view_transformer_n_heads=2, view_transformer_n_layers=4,
            dpt_features=32, dpt_out_channels=[16, 32, 64, 128])
SWIN = RenderFormerConfig(**dict(TINY, view_transformer_use_swin_attn=True))
FULL = RenderFormerConfig(**dict(TINY, view_transformer_use_swin_attn=False))


def test_frame_layout_pads_to_the_frame_unit_and_centres_the_frame():
    from renderformer_amd.model import frame_layout
    assert frame_layout(SWIN, (1080, 1920), True) == (1080, 1920, 1088, 1920, 4, 0)
    assert frame_layout(SWIN, (720, 1280), True) == (720, 1280, 768, 1280, 24, 0)
    assert frame_layout(SWIN, (45, 99), True) == (45, 99, 64, 128, 9, 14)
    assert frame_layout(SWIN, (44, 100), True) == (44, 100, 64, 128, 10, 14)
    assert frame_layout(FULL, (20, 44), True) == (20, 44, 24, 48, 2, 2)
    # a frame of whole units: its own size and zeros, with and without overscan, int or tuple
    for over in (False, True):
        assert frame_layout(SWIN, (64, 192), over) == (64, 192, 64, 192, 0, 0)
        assert frame_layout(SWIN, 128, over) == (128, 128, 128, 128, 0, 0)
        assert frame_layout(FULL, (8, 24), over) == (8, 24, 8, 24, 0, 0)


def test_frame_layout_without_overscan_is_frame_size():
    from renderformer_amd.model import frame_layout, frame_size
    assert frame_layout(SWIN, (576, 1024)) == frame_size(SWIN, (576, 1024)) + (576, 1024, 0, 0)
    with pytest.raises(ValueError, match="width 100 incompatible with patch/window size"):
        frame_layout(SWIN, (64, 100))
    with pytest.raises(ValueError, match="height 1080"):
        frame_layout(SWIN, (1080, 1920), False)
    for bad in ((0, 64), (64, -8)):
        for over in (False, True):
            with pytest.raises(ValueError):
                frame_layout(FULL, bad, over)


def _cams(b=1, v=2):
    return torch.eye(4).expand(b, v, 4, 4).contiguous(), torch.full((b, v, 1), 40.0), torch.tensor(
        [[[60.0, 55.0, 50.25, 20.5]] * v] * b)


def test_render_entry_points_check_the_camera_arguments():
    """Exactly one of fov / intrinsics, intrinsics float32 [B, V, 4]: refused before anything touches a device, by the
    model's two entry points and by the pipeline's in front of them."""
    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    m = RenderFormer(SWIN)
    pipe = RenderFormerRenderingPipeline(m)
    tex = torch.zeros(1, 4, 13, 32, 32)
    c2w, fov, K = _cams()
    res = (45, 99)

    def entry_points(fov_, **kw):
        yield lambda: m.render_views(None, None, None, None, c2w, fov_, res, overscan=True, **kw)
        yield lambda: m.render_encoded(None, c2w, fov_, res, overscan=True, **kw)
        yield lambda: pipe.render(None, tex, None, None, c2w, fov_, resolution=res, overscan=True, **kw)
        yield lambda: pipe.render_encoded(None, c2w, fov_, resolution=res, overscan=True, **kw)

    for call in entry_points(fov, intrinsics=K):
        with pytest.raises(ValueError, match="exactly one of fov and intrinsics"):
            call()
    for call in entry_points(None):
        with pytest.raises(ValueError, match="exactly one of fov and intrinsics"):
            call()
    for bad in (K[:, :, :3], K[0], K[:, :1], K.reshape(1, 2, 2, 2)):
        for call in entry_points(None, intrinsics=bad):
            with pytest.raises(ValueError, match=r"intrinsics must be \[B, V, 4\]"):
                call()
    for bad in (K.double(), K.half(), K.tolist()):
        for call in entry_points(None, intrinsics=bad):
            with pytest.raises(ValueError, match="intrinsics must be a float32 tensor"):
                call()
    # well-formed arguments pass the checks: what stops the call is the model not being on a device
    for call in list(entry_points(None, intrinsics=K))[:1] + list(entry_points(fov))[:1]:
        with pytest.raises(RuntimeError, match="call .to"):
            call()


def test_a_non_multiple_size_without_overscan_raises_as_before():
    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    m = RenderFormer(SWIN)
    pipe = RenderFormerRenderingPipeline(m)
    c2w, fov, K = _cams()
    msg = "height 45 incompatible with patch/window size"
    with pytest.raises(ValueError, match=msg):
        m.render_views(None, None, None, None, c2w, None, (45, 99), intrinsics=K)
    with pytest.raises(ValueError, match=msg):
        m.render_encoded(None, c2w, fov, (45, 99), overscan=False)
    with pytest.raises(ValueError, match=msg):
        pipe.render(None, torch.zeros(1, 4, 13, 32, 32), None, None, c2w, fov, resolution=(45, 99))
    with pytest.raises(ValueError, match="width 0"):  # overscan pads a frame; it does not invent one
        m.render_views(None, None, None, None, c2w, fov, (64, 0), overscan=True)


def test_pipeline_keywords_are_keyword_only_after_torch_dtype():
    import inspect

    from renderformer_amd import RenderFormerRenderingPipeline
    for fn in (RenderFormerRenderingPipeline.render, RenderFormerRenderingPipeline.render_encoded):
        p = inspect.signature(fn).parameters
        names = list(p)
        assert names[-3:] == ["torch_dtype", "intrinsics", "overscan"]
        assert p["intrinsics"].kind is p["overscan"].kind is inspect.Parameter.KEYWORD_ONLY
        assert p["intrinsics"].default is None and p["overscan"].default is False
        assert p["torch_dtype"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD


def test_ray_and_window_entry_points_check_their_arguments():
    """rf_ray_tokens_cam / rf_hdr_output_win / rf_frame_window validate before any launch (no device needed)."""
    import ctypes

    from renderformer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librfhip.so not built")
    lib = _lib.load(require_device=False)
    p = ctypes.c_void_p(16)
    cam = lambda fov, intr, fh, fw, h, w, y0, x0: lib.rf_ray_tokens_cam(  # noqa: E731
        p, fov, intr, 1, fh, fw, h, w, y0, x0, 8, p, None, 1, None)
    for fov, intr in ((p, p), (None, None)):
        assert cam(fov, intr, 45, 99, 64, 128, 9, 14) == 1 and b"exactly one" in lib.rf_last_error()
    assert cam(None, p, 45, 99, 64, 100, 9, 0) == 1 and b"width 100" in lib.rf_last_error()  # the token frame's checks
    for y0, x0 in ((-1, 14), (20, 14), (9, 30), (9, -1)):
        assert cam(None, p, 45, 99, 64, 128, y0, x0) == 1 and b"does not lie inside" in lib.rf_last_error()
    assert cam(p, None, 0, 99, 64, 128, 0, 0) == 1 and b"positive frame" in lib.rf_last_error()
    assert lib.rf_ray_tokens_cam(p, None, p, 0, 45, 99, 64, 128, 9, 14, 8, p, None, 1, None) == 0  # no views
    win = lambda y0, x0, oh, ow: lib.rf_hdr_output_win(p, p, 2, 3, 24, 40, y0, x0, oh, ow, 1e-3, 1, 1, None)  # noqa: E731
    crop = lambda y0, x0, oh, ow: lib.rf_frame_window(p, p, 2, 24, 40, 3, y0, x0, oh, ow, None)  # noqa: E731
    for fn in (win, crop):
        for y0, x0, oh, ow in ((5, 3, 20, 31), (5, 3, 13, 38), (-1, 0, 4, 4), (0, 0, 0, 4)):
            assert fn(y0, x0, oh, ow) == 1 and b"does not lie inside" in lib.rf_last_error()
    assert lib.rf_hdr_output_win(p, p, 0, 3, 24, 40, 5, 3, 13, 31, 1e-3, 1, 1, None) == 0  # no images: nothing to do
    assert lib.rf_frame_window(None, p, 2, 24, 40, 3, 5, 3, 13, 31, None) == 1 and b"null" in lib.rf_last_error()


def test_cli_parsers_accept_overscan():
    import batch_infer
    import infer
    p = argparse.ArgumentParser()
    infer.add_common_args(p)
    assert p.parse_args([]).overscan is False
    a = p.parse_args(["--height", "1080", "--width", "1920", "--overscan"])
    assert a.overscan is True and infer.frame_resolution(a) == (1080, 1920)
    assert batch_infer.add_common_args is infer.add_common_args  # the folder CLI shares the flags


def test_sharded_renderer_sizes_its_slots_by_the_requested_frame():
    from renderformer_amd.parallel import ShardedRenderer

    class _P:
        config = SWIN
    assert ShardedRenderer(_P())._frame_shape(4, (1080, 1920)) == (4, 1080, 1920, 3)


def _generators():
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import make_golden_cam
    import make_golden_rect
    return make_golden_cam, make_golden_rect


def test_generator_rays_reduce_to_the_rectangular_generators():
    """make_golden_cam.cam_rays with the fov-equivalent intrinsics and no window is make_golden_rect.rect_rays, up to
    fp32 rounding (the two divide by f in a different order of operations)."""
    cam, rect = _generators()
    g = torch.Generator().manual_seed(3)
    rot = torch.linalg.qr(torch.randn(2, 2, 3, 3, generator=g))[0]
    c2w = torch.eye(4).repeat(2, 2, 1, 1)
    c2w[..., :3, :3] = rot
    c2w[..., :3, 3] = torch.randn(2, 2, 3, generator=g)
    fov = torch.tensor([[[35.0], [50.0]], [[42.5], [61.0]]]) / 180.0 * torch.pi
    for h, w in ((64, 128), (44, 100)):
        K = cam.fov_intrinsics(fov, h, w)
        assert tuple(K.shape) == (2, 2, 4) and torch.equal(K[..., 0], K[..., 1])
        assert torch.equal(K[..., 2], torch.full((2, 2), w / 2)) and torch.equal(K[..., 3], torch.full((2, 2), h / 2))
        o, d = cam.cam_rays(c2w, K, h, w)
        o_ref, d_ref = rect.rect_rays(c2w, fov, h, w)
        assert torch.equal(o, o_ref) and tuple(d.shape) == (2, 2, h, w, 3)
        assert torch.allclose(d, d_ref, rtol=0, atol=4 * torch.finfo(torch.float32).eps)


def test_generator_window_is_a_shifted_principal_point():
    """The padded frame's rays are those of the camera whose principal point moved by the window origin, and its
    requested window holds the unpadded frame's rays (cx, cy multiples of 0.25: the pixel offsets are exact)."""
    cam, _ = _generators()
    c2w = torch.eye(4).repeat(1, 1, 1, 1)
    K = torch.tensor([[[60.0, 55.0, 60.75, 16.25]]])
    hp, wp, y0, x0 = cam.layout((45, 99), 64)
    assert (hp, wp, y0, x0) == (64, 128, 9, 14) and cam.layout((20, 44), 8) == (24, 48, 2, 2)
    _, pad = cam.cam_rays(c2w, K, hp, wp, y0, x0)
    _, shifted = cam.cam_rays(c2w, K + torch.tensor([0.0, 0.0, x0, y0]), hp, wp)
    _, plain = cam.cam_rays(c2w, K, 45, 99)
    assert torch.equal(pad, shifted)
    assert torch.equal(pad[:, :, y0:y0 + 45, x0:x0 + 99], plain)
