"""Rectangular frames, host side (no GPU): resolution = int | (height, width) in the plan, the validity checks, the
CLI flags and the FLOP model.  An int r must give, field by field, what (r, r) gives."""
import argparse
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from renderformer_amd.config import LARGE_PROXY, RenderFormerConfig  # noqa: E402
from renderformer_amd.flops import dpt_flops, frame_flops, frame_hw  # noqa: E402
from renderformer_amd.model import _build_plan, frame_size  # noqa: E402

TINY = dict(latent_dim=256, num_layers=2, num_heads=2, dim_feedforward=512, view_transformer_latent_dim=256,
            view_transformer_ffn_hidden_dim=512, view_transformer_n_heads=2, view_transformer_n_layers=4,
            dpt_features=32, dpt_out_channels=[16, 32, 64, 128])
N_REG, PATCH = 16, 8


def _mask():
    m = np.zeros((2, 64), dtype=bool)
    m[0, :61] = True
    m[1, 3:48] = True
    return m


def _plan(res, views=2):
    return _build_plan(_mask(), views, res, PATCH, N_REG, torch.device("cpu"))


@pytest.mark.parametrize("hw", [(64, 128), (128, 64)])
def test_plan_of_a_rectangular_frame(hw):
    h, w = hw
    p = _plan(hw)
    assert (p.H, p.W, p.hp, p.wp, p.R) == (h, w, h // 8, w // 8, 128)
    S, R, V = [N_REG + 61, N_REG + 45], 128, 2
    cu1 = [0, S[0], S[0] + S[1]]
    kv = 0
    for i in range(4):  # image i = scene b, view v: R ray-token rows each, keys = the scene's stage-1 rows
        b = i // V
        assert p.prob2[i].tolist() == [i * R, R, kv, S[b], cu1[b]]
        assert p.prob_self[i].tolist() == [i * R, R, i * R, R, i * R]
        kv += S[b]
    assert p.T_kv == kv and p.kv_off.tolist() == [0, S[0], 2 * S[0], 2 * S[0] + S[1], kv]
    # stage 1 does not know the frame
    q = _plan((64, 64))
    assert p.prob1.tolist() == q.prob1.tolist() and p.T1 == q.T1 == cu1[-1]


def test_plan_of_an_int_is_the_plan_of_the_square():
    a, b = _plan(128), _plan((128, 128))
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if isinstance(x, torch.Tensor):
            assert x.dtype == y.dtype and torch.equal(x, y), f.name
        else:
            assert x == y, f.name
    assert (a.H, a.W, a.hp, a.wp, a.R) == (128, 128, 16, 16, 256)
    assert frame_hw(128) == frame_hw((128, 128)) == frame_hw([128, 128]) == (128, 128)
    with pytest.raises(ValueError):
        frame_hw((1, 2, 3))


def test_plan_cache_does_not_tell_an_int_from_its_square(monkeypatch):
    from renderformer_amd import RenderFormer, ops
    m = RenderFormer(RenderFormerConfig(**dict(TINY, view_transformer_use_swin_attn=True)))
    m._device = torch.device("cpu")  # (host tables only: no stream-K range tables, which ask the device its size)
    monkeypatch.setattr(ops, "attn_schedule_enabled", lambda: False)
    assert m._plan_host(_mask(), 2, 64) is m._plan_host(_mask(), 2, (64, 64))
    assert m._plan_host(_mask(), 2, (64, 128)) is not m._plan_host(_mask(), 2, (128, 64))
    assert m._plan_host(_mask(), 2, (64, 128)).wp == 16 and m._plan_host(_mask(), 2, (128, 64)).wp == 8


def test_frame_size_checks_each_side():
    swin = RenderFormerConfig(**dict(TINY, view_transformer_use_swin_attn=True))
    full = RenderFormerConfig(**dict(TINY, view_transformer_use_swin_attn=False))
    assert frame_size(swin, 64) == (64, 64) and frame_size(swin, (64, 192)) == (64, 192)
    assert frame_size(swin, (576, 1024)) == (576, 1024)  # 16:9, both sides multiples of 64
    assert frame_size(full, (8, 24)) == (8, 24)
    with pytest.raises(ValueError, match="width 100"):
        frame_size(swin, (64, 100))
    with pytest.raises(ValueError, match="height 60"):
        frame_size(full, (60, 64))
    with pytest.raises(ValueError, match="height 72"):  # a multiple of the patch but not of patch x window
        frame_size(swin, (72, 64))
    with pytest.raises(ValueError, match="height 0"):
        frame_size(full, (0, 64))


def test_render_entry_points_name_the_offending_side():
    """render_views / render_encoded (and the pipeline's render / render_encoded in front of them) check the frame
    first: 64 x 100 under Swin names the width, 60 x 64 under full attention the height."""
    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    for swin, res, side in ((True, (64, 100), "width 100"), (False, (60, 64), "height 60")):
        m = RenderFormer(RenderFormerConfig(**dict(TINY, view_transformer_use_swin_attn=swin)))
        pipe = RenderFormerRenderingPipeline(m)
        tex = torch.zeros(1, 4, 13, 32, 32)
        with pytest.raises(ValueError, match=side):
            m.render_views(None, None, None, None, None, None, res)
        with pytest.raises(ValueError, match=side):
            m.render_encoded(None, None, None, res)
        with pytest.raises(ValueError, match=side):
            pipe.render(None, tex, None, None, None, None, resolution=res)
        with pytest.raises(ValueError, match=side):
            pipe.render_encoded(None, None, None, resolution=res)


def test_ray_entry_points_check_the_frame():
    """rf_ray_tokens_hw / rf_patchify_rays_hw refuse a side that is not whole patches, and a frame whose pixel index
    does not fit an int, before any launch (no device needed); the message names the side."""
    import ctypes

    from renderformer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librfhip.so not built")
    lib = _lib.load(require_device=False)
    p = ctypes.c_void_p(16)
    for h, w, msg in ((64, 100, b"width 100"), (60, 64, b"height 60"), (65536, 32768, b"32-bit"), (0, 64, b"positive")):
        assert lib.rf_ray_tokens_hw(p, p, 1, h, w, 8, p, None, 1, None) == 1
        assert msg in lib.rf_last_error(), lib.rf_last_error()
        assert lib.rf_patchify_rays_hw(p, 1, h, w, 8, p, 1, None) == 1
        assert msg in lib.rf_last_error(), lib.rf_last_error()
    assert lib.rf_ray_tokens_hw(p, p, 1, 64, 128, 8, p, None, 7, None) == 1 and b"out_dtype" in lib.rf_last_error()
    assert lib.rf_ray_tokens_hw(p, p, 0, 64, 128, 8, p, None, 1, None) == 0  # no views: nothing to do
    assert lib.rf_ray_tokens_dt(p, p, 1, 60, 8, p, None, 1, None) == 1  # the square symbol: the same checks


def _parser():
    import infer
    p = argparse.ArgumentParser()
    infer.add_common_args(p)
    return infer, p


def test_cli_height_and_width_default_to_resolution():
    infer, p = _parser()
    a = p.parse_args([])
    assert (a.resolution, a.height, a.width) == (512, None, None) and infer.frame_resolution(a) == 512
    a = p.parse_args(["--resolution", "256"])
    assert infer.frame_resolution(a) == 256
    a = p.parse_args(["--height", "576", "--width", "1024"])
    assert infer.frame_resolution(a) == (576, 1024)
    a = p.parse_args(["--resolution", "1024", "--height", "576"])
    assert infer.frame_resolution(a) == (576, 1024)
    a = p.parse_args(["--resolution", "256", "--width", "512"])
    assert infer.frame_resolution(a) == (256, 512)
    a = p.parse_args(["--resolution", "256", "--width", "256", "--height", "256"])
    assert infer.frame_resolution(a) == 256  # a square stays the reference's int
    # every reference flag is still there
    a = p.parse_args(["--model_id", "x", "--precision", "bf16", "--resolution", "64", "--tone_mapper", "none"])
    assert (a.model_id, a.precision, a.resolution, a.tone_mapper) == ("x", "bf16", 64, "none")


def test_batch_cli_shares_the_flags():
    import batch_infer
    assert batch_infer.frame_resolution is _parser()[0].frame_resolution


@pytest.mark.parametrize("cfg", [RenderFormerConfig(**dict(TINY, view_transformer_use_swin_attn=True)),
                                 RenderFormerConfig(**dict(TINY, view_transformer_use_swin_attn=False)), LARGE_PROXY])
def test_flops_of_a_square_tuple_equal_the_int(cfg):
    for r in (64, 512, 1024):
        assert frame_flops(cfg, 5633, (r, r), 3) == frame_flops(cfg, 5633, r, 3)
        assert dpt_flops(cfg, (r, r)) == dpt_flops(cfg, r)


def test_flops_count_tokens_and_pixels_of_both_sides():
    cfg = LARGE_PROXY
    a, b, sq = frame_flops(cfg, 5633, (576, 1024)), frame_flops(cfg, 5633, (1024, 576)), frame_flops(cfg, 5633, 768)
    assert a == b  # the model is symmetric in the two sides
    # 1024 x 576 and 768 x 768 have the same pixel and ray-token counts
    assert a == sq
    big = frame_flops(cfg, 5633, 1024)
    assert a["stage1"] == big["stage1"] and a["dpt"] * 16 == big["dpt"] * 9
    from renderformer_amd.parallel import ShardedRenderer, scene_cost

    class _P:
        config = cfg
    assert ShardedRenderer(_P())._frame_shape(4, (576, 1024)) == (4, 576, 1024, 3)
    assert ShardedRenderer(_P())._frame_shape(4, 512) == (4, 512, 512, 3)
    assert scene_cost(cfg, 100, 2, (64, 64)) == scene_cost(cfg, 100, 2, 64)
