"""Rectangular frames on the device: resolution = (height, width) from the ray kernels to pipeline.render.

The fixtures (tests/golden/rect_*.npz, make_golden_rect.py) are the reference model's own fp32 CPU output for
H x W ray maps: its RenderFormer.forward takes any H x W, only its RayGenerator and pipeline are square.  The bars
are the project's: 1e-3 relative L2 per tap and on the HDR pixels, and per view the deviation from the mean within a
quarter of what separates two views of the scene (test_parity_gpu.py: these renders sit on a large constant offset
that plain relative L2 would hide a scrambled patch order behind).  tap_dpt and the HDR frame are recorded every
pix_sub-th pixel row and column; the decoder taps (<name>_taps.npz) for the images `dec_images`.
"""
import functools
import math
import os

import numpy as np
import pytest
import torch

from golden_util import GOLDEN, load_case, rel_l2, rel_l2_ac

pytestmark = pytest.mark.gpu
dev = "cuda"
HDR_TOL = 1e-3   # the project's bar (test_parity_gpu.HDR_TOL)
TAP_TOL = 1e-3   # per-tap relative L2 (test_parity_gpu.TAP_TOL, test_oracle_golden)
SWIN_TOL = 6e-3  # test_kernels_gpu.test_swin_attention_matches_oracle_layout
RECT_CASES = ["rect_swin_64x128", "rect_swin_128x64", "rect_swin_64x192", "rect_full_64x128"]
PATCH = 8


@functools.lru_cache(maxsize=None)
def _case(name):
    cfg, sd, inp, _, z = load_case(name)
    taps = np.load(os.path.join(GOLDEN, name + "_taps.npz"), allow_pickle=False) if "frame_hw" in z.files else None
    return cfg, sd, inp, z, taps


def _hw(z):
    return int(z["frame_hw"][0]), int(z["frame_hw"][1])


def _sub(z):
    sub, off = (int(v) for v in z["pix_sub"])
    return slice(off, None, sub)


def _pipeline(cfg, sd, **kw):
    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    return RenderFormerRenderingPipeline(RenderFormer(cfg, sd, **kw)).to(dev)


def _inputs(inp):
    """fresh device copies (render log-encodes the texture in place)"""
    return {k: v.clone().to(dev) for k, v in inp.items()}


def _render(pipe, d, resolution):
    return pipe(d["triangles"], d["texture"], d["mask"], d["vn"], d["c2w"], d["fov"], resolution=resolution,
                torch_dtype=torch.bfloat16)


def _elu(x):
    x = torch.as_tensor(x, dtype=torch.float64)
    return torch.where(x > 0, x, 1e-3 * torch.expm1(x))  # ELU(alpha=1e-3), view_transformer.py:86


def _host_tokens(rays, patch=PATCH):
    """'b (h1 p1) (w1 p2) c -> (b h1 w1) (c p1 p2)' of rays [P, H, W, 3]"""
    P, H, W, _ = rays.shape
    return rays.reshape(P, H // patch, patch, W // patch, patch, 3).permute(0, 1, 3, 5, 2, 4).reshape(
        P * (H // patch) * (W // patch), 3 * patch * patch)


def _check_hdr(name, got, z):
    """the two bounds of a rendered frame [B, V, H, W, 3] against the fixture's (sub-sampled) HDR"""
    sl = _sub(z)
    assert tuple(got.shape) == (2, 2) + _hw(z) + (3,) and got.dtype == torch.float32
    g = got[:, :, sl, sl].cpu()
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


# ------------------------------------------------------------------------------------------------ 1. ray tokens
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("name", RECT_CASES[:3])
def test_ray_tokens_hw_match_the_fixture_rays(name, dtype):
    """rf_ray_tokens_hw against the fixture's rays_d (the reference's ray arithmetic with H != W, camera frame:
    c2w = identity) patchified on the host and rounded to the operand type.  The device and the host compute the
    fp32 direction with different tan / divide / sqrt roundings (a few fp32 ulps, ~1e-7 relative), so a value may
    land on the other side of a rounding boundary of the 16-bit type: at most ONE 16-bit ulp below 1.0 (2^-11 for
    fp16, 2^-8 for bf16), and for a fraction of the values of the order of 1e-7 / ulp, far below the 1 % allowed."""
    from renderformer_amd import ops
    cfg, sd, inp, z, _ = _case(name)
    H, W = _hw(z)
    P = 4
    ref = _host_tokens(torch.from_numpy(z["rays_d"]).reshape(P, H, W, 3)).to(dtype)
    eye = torch.eye(4).expand(P, 4, 4).contiguous().to(dev)
    fov = inp["fov"].reshape(P).float().contiguous().to(dev)
    tok = torch.zeros(P * (H // PATCH) * (W // PATCH), 3 * PATCH * PATCH, dtype=dtype, device=dev)
    rpos = torch.full((P, 9), 7.0, device=dev)
    ops.ray_tokens(eye, fov, (H, W), PATCH, tok, rpos)
    diff = (tok.float().cpu() - ref.float()).abs()
    ulp = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
    print(f"{name} {dtype}: max |diff| {diff.max():.3e} (one ulp {ulp:.3e}), differing {float((diff > 0).float().mean()):.2e}")
    assert diff.max() <= ulp
    assert (diff > 0).float().mean() < 1e-2
    assert torch.equal(rpos.cpu(), torch.zeros(P, 9))  # the camera origin, three times


def _cameras(name="rect_swin_64x128"):
    """the fixture's world-frame cameras: real rotations"""
    inp = _case(name)[2]
    c2w = inp["c2w"].reshape(-1, 4, 4).float().contiguous().to(dev)
    return c2w, inp["fov"].reshape(-1).float().contiguous().to(dev)


def _tokens(c2w, fov, hw, dtype):
    from renderformer_amd import ops
    h, w = hw
    P = c2w.shape[0]
    tok = torch.zeros(P * (h // PATCH) * (w // PATCH), 3 * PATCH * PATCH, dtype=dtype, device=dev)
    rpos = torch.zeros(P, 9, device=dev)
    ops.ray_tokens(c2w, fov, hw, PATCH, tok, rpos)
    return tok, rpos


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_ray_tokens_hw_of_a_square_are_the_square_entry_points_bits(dtype):
    from renderformer_amd import _lib, ops
    c2w, fov = _cameras()
    P = c2w.shape[0]
    tok, rpos = _tokens(c2w, fov, (64, 64), dtype)
    sq = torch.zeros_like(tok)
    sq_pos = torch.zeros_like(rpos)
    _lib.call("rf_ray_tokens_dt", _lib.ptr(c2w), _lib.ptr(fov), P, 64, PATCH, _lib.ptr(sq), _lib.ptr(sq_pos),
              ops.DT_F16 if dtype == torch.float16 else ops.DT_BF16, _lib.stream())
    assert torch.equal(tok, sq) and torch.equal(rpos, sq_pos)
    assert tok.float().abs().sum() > 0
    if dtype == torch.bfloat16:  # and the bf16-only symbol
        sq2 = torch.zeros_like(tok)
        _lib.call("rf_ray_tokens", _lib.ptr(c2w), _lib.ptr(fov), P, 64, PATCH, _lib.ptr(sq2), _lib.ptr(sq_pos),
                  _lib.stream())
        assert torch.equal(tok, sq2)


def test_ray_tokens_of_a_narrow_frame_are_the_centre_columns_of_the_square():
    """fov is the vertical field of view, so a 64 x 32 frame sees the centre columns of the 64 x 64 frame's rays:
    x + 0.5 - W/2 is exact in fp32 for both, f is the same: patch columns 2..5 of 8, bit for bit."""
    c2w, fov = _cameras()
    P = c2w.shape[0]
    sq, _ = _tokens(c2w, fov, (64, 64), torch.float16)
    nar, _ = _tokens(c2w, fov, (64, 32), torch.float16)
    assert torch.equal(nar.view(P, 8, 4, 192), sq.view(P, 8, 8, 192)[:, :, 2:6])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("name", RECT_CASES[:3])
def test_patchify_rays_hw_is_the_host_rearrange(name, dtype):
    from renderformer_amd import ops
    z = _case(name)[3]
    H, W = _hw(z)
    rays = torch.from_numpy(z["rays_d"]).reshape(4, H, W, 3).contiguous()
    tok = torch.zeros(4 * (H // PATCH) * (W // PATCH), 192, dtype=dtype, device=dev)
    ops.patchify_rays(rays.to(dev), PATCH, tok)
    assert torch.equal(tok.cpu(), _host_tokens(rays).to(dtype))


# ------------------------------------------------------------------------------------------------ 2. Swin
def _swin_reference(q, k, v, n_img, gh, gw, shift, H, ws=8):
    """fp64 SwinSelfAttention core (attention.py:316-370 with identity projections): roll by -shift, partition into
    ws x ws windows, attention inside a window between tokens of the same region of the ROLLED image (per axis the
    three slices [0, g - ws), [g - ws, g - shift), [g - shift, g)), reverse, roll back."""
    D = q.shape[1]
    hd = D // H

    def part(x):
        x = x.double().view(n_img, gh, gw, -1)
        if shift:
            x = torch.roll(x, (-shift, -shift), (1, 2))
        c = x.shape[-1]
        return x.view(n_img, gh // ws, ws, gw // ws, ws, c).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, c)

    def region(n):
        c = torch.arange(n)
        return (c >= n - ws).long() + (c >= n - shift).long()
    qw, kw, vw = (part(t).view(-1, ws * ws, H, hd).transpose(1, 2) for t in (q, k, v))
    s = qw @ kw.transpose(-1, -2) / math.sqrt(hd)
    if shift:
        lab = region(gh)[:, None] * 3 + region(gw)[None, :]  # [gh, gw], in the rolled image's coordinates
        lw = lab.view(gh // ws, ws, gw // ws, ws).permute(0, 2, 1, 3).reshape(-1, ws * ws)
        same = (lw[:, :, None] == lw[:, None, :]).repeat(n_img, 1, 1)  # [windows of every image, 64, 64]
        s = s.masked_fill(~same[:, None], float("-inf"))
    o = torch.softmax(s, -1) @ vw
    o = o.transpose(1, 2).reshape(n_img, gh // ws, gw // ws, ws, ws, D).permute(0, 1, 3, 2, 4, 5).reshape(n_img, gh, gw, D)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    return o.reshape(-1, D)


@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("gh,gw", [(8, 16), (16, 8), (8, 24)])
def test_swin_attention_on_rectangular_grids(gh, gw, shift):
    """One window along one axis (the -4 roll wraps inside it) while the other axis has real neighbours."""
    from renderformer_amd import ops
    H, D, n_img = 2, 256, 2
    T = n_img * gh * gw
    g = torch.Generator(device="cpu").manual_seed(100 * gh + gw + shift)
    q, k, v = [torch.randn(T, D, generator=g).bfloat16() for _ in range(3)]
    out = torch.zeros(T, D, device=dev, dtype=torch.bfloat16)
    ops.swin_attention(q.to(dev), k.to(dev), v.to(dev), out, n_img, gh, gw, shift, H)
    ref = _swin_reference(q.float(), k.float(), v.float(), n_img, gh, gw, shift, H)
    err = rel_l2(out.float().cpu(), ref)
    print(f"swin {gh}x{gw} shift {shift}: rel L2 {err:.3e} (bar {SWIN_TOL})")
    assert err < SWIN_TOL
    # the reference tells the axes apart: the transposed grid's answer is far away
    wrong = _swin_reference(q.float(), k.float(), v.float(), n_img, gw, gh, shift, H)
    assert rel_l2(wrong, ref) > 0.1


# ------------------------------------------------------------------------------------------------ 3. DPT alone
@pytest.mark.parametrize("name", RECT_CASES)
def test_dpt_head_on_the_fixture_taps(name):
    cfg, sd, inp, z, taps = _case(name)
    H, W = _hw(z)
    hp, wp = H // PATCH, W // PATCH
    m = _pipeline(cfg, sd).model
    imgs = [int(i) for i in taps["dec_images"]]
    rows = [torch.from_numpy(taps[f"tap_dec{i}"]).reshape(len(imgs) * hp * wp, -1).to(dev) for i in cfg.out_layers]
    out = m._w.dpt(rows, len(imgs), hp, wp, PATCH, 1e-3, False, False)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (len(imgs), 3, H, W)
    sl = _sub(z)
    err = rel_l2(out[:, :, sl, sl].cpu(), _elu(z["tap_dpt"][imgs]))
    print(f"{name}: DPT on the reference taps, rel L2 {err:.3e} (bar {TAP_TOL})")
    assert err < TAP_TOL


# ------------------------------------------------------------------------------------------------ 4. forward()
def _forward_args(inp, z):
    tex = inp["texture"].clone()
    tex[:, :, -3:] = torch.log10(tex[:, :, -3:] + 1.0)  # what the pipeline does in front of the model
    B = tex.shape[0]
    t = lambda a: torch.as_tensor(a).to(dev)  # noqa: E731
    return (t(inp["triangles"].reshape(B, -1, 9)), t(tex), t(inp["mask"]), t(inp["vn"].reshape(B, -1, 9)),
            t(z["rays_o"]), t(z["rays_d"]), t(z["tris_cam"]))


@pytest.mark.parametrize("name", RECT_CASES)
def test_forward_takes_rectangular_ray_maps(name):
    cfg, sd, inp, z, taps = _case(name)
    H, W = _hw(z)
    R = (H // PATCH) * (W // PATCH)
    m = _pipeline(cfg, sd).model
    args = _forward_args(inp, z)
    out = m.forward(*args)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (2, 2, 3, H, W)
    sl = _sub(z)
    o = out.cpu()
    e_dpt = rel_l2(o[:, :, :, sl, sl].reshape(4, 3, H // 2, W // 2), _elu(z["tap_dpt"]))
    print(f"{name}: forward() logits rel L2 {e_dpt:.3e} (bar {TAP_TOL})")
    _check_hdr(name, torch.pow(10.0, out.permute(0, 1, 3, 4, 2)) - 1.0, z)
    assert e_dpt < TAP_TOL
    # every decoder layer's output of the recorded images (the capture takes the per-op path of stage 2)
    imgs = [int(i) for i in taps["dec_images"]]
    cap = m.capture_taps(dec_rows=np.arange(R), dec_views=imgs)
    out2 = m.forward(*args)
    torch.cuda.synchronize()
    dec = cap["dec_rows"].cpu()
    assert tuple(dec.shape) == (cfg.view_transformer_n_layers, len(imgs), R, cfg.view_transformer_latent_dim)
    errs = [rel_l2(dec[i], taps[f"tap_dec{i}"]) for i in range(dec.shape[0])]
    print(f"{name}: decoder taps rel L2 {', '.join(f'{e:.3e}' for e in errs)} (bar {TAP_TOL})")
    assert all(e < TAP_TOL for e in errs)
    assert rel_l2(out2.cpu(), o) < TAP_TOL


# ------------------------------------------------------------------------------------------------ 5. pipeline
@pytest.mark.parametrize("name", RECT_CASES)
def test_pipeline_renders_the_rectangular_fixture(name):
    cfg, sd, inp, z, _ = _case(name)
    pipe = _pipeline(cfg, sd)
    out = _render(pipe, _inputs(inp), _hw(z))
    _check_hdr(name, out, z)


def test_square_tuple_renders_the_ints_bits():
    cfg, sd, inp, z, _ = _case("tiny_swin")
    pipe = _pipeline(cfg, sd)
    a = _render(pipe, _inputs(inp), 64)
    b = _render(pipe, _inputs(inp), (64, 64))
    assert a.shape == b.shape == (2, 2, 64, 64, 3) and torch.equal(a, b)
    assert rel_l2(a.cpu(), z["hdr"]) < HDR_TOL


@pytest.mark.parametrize("name", ["rect_swin_64x128", "rect_full_64x128"])
def test_render_encoded_and_view_chunks_give_the_same_bits(name):
    cfg, sd, inp, z, _ = _case(name)
    hw = _hw(z)
    pipe = _pipeline(cfg, sd)
    full = _render(pipe, _inputs(inp), hw)
    d = _inputs(inp)
    scene = pipe.encode(d["triangles"], d["texture"], d["mask"], d["vn"])
    enc = pipe.render_encoded(scene, d["c2w"], d["fov"], hw)
    assert enc.shape == full.shape and torch.equal(enc, full)
    sq = pipe.render_encoded(scene, d["c2w"], d["fov"], 64)  # the same handle, another frame size
    assert tuple(sq.shape) == (2, 2, 64, 64, 3) and torch.isfinite(sq).all()
    chunked = _pipeline(cfg, sd, view_chunk=1)
    one = _render(chunked, _inputs(inp), hw)
    assert torch.equal(one, full)
    d = _inputs(inp)
    scene = chunked.encode(d["triangles"], d["texture"], d["mask"], d["vn"])
    assert torch.equal(chunked.render_encoded(scene, d["c2w"], d["fov"], hw), full)


def test_range_guard_rerenders_a_rectangular_frame():
    """A checkpoint whose activations exceed fp16 (test_parity_gpu._overflow_sd's stand-in: stage-1 layer 0's SwiGLU
    weights scaled): the default "sync" render of a 64 x 128 frame notices, renders the frame again with bf16
    operands and returns THAT frame: the bits of a model built with those operands from the start."""
    from renderformer_amd.model import PrecisionWarning
    cfg, sd, inp, z, _ = _case("rect_swin_64x128")
    big = dict(sd)
    for k in ("transformer.layers.0.ffn.w1.weight", "transformer.layers.0.ffn.w3.weight"):
        big[k] = big[k] * 2000.0
    pipe = _pipeline(cfg, big)
    with pytest.warns(PrecisionWarning, match="fp16 operand overflow"):
        out = _render(pipe, _inputs(inp), (64, 128))
    assert tuple(out.shape) == (2, 2, 64, 128, 3) and torch.isfinite(out).all()
    m = pipe.model
    assert m.range_fallbacks == 1 and m.operands == "bf16"
    again = _render(pipe, _inputs(inp), (64, 128))  # the model keeps the operands: no second fallback
    assert m.range_fallbacks == 1 and torch.equal(again, out)
    ref = _render(_pipeline(cfg, big, operands="bf16", dpt_precision=m.dpt_precision), _inputs(inp), (64, 128))
    assert torch.equal(ref, out)
