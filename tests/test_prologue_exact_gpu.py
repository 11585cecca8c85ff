"""Per-element, guard-band and edge tests of the prologue and output kernels (prologue.hip) and of the fp32 resize.

Every output sits in a kernel_checks.Guarded buffer (guard rows everywhere; ld above the width wherever the C signature
takes a leading dimension, ld == width where the op writes the full stride or needs a dense buffer), strided inputs are
surrounded by NaN, and every output element is compared with an fp64 reference computed from the fp32 inputs the
kernel reads, within a bound built from the number formats (kernel_checks: one F32_ULP per fp32 operation, LIBM_ULPS
ulps per device math library call, the output rounding).  The shapes are the smallest that reach each path: rows that
are no multiple of a block, the second 64-block round of the centre reduction, the second 1024-column trip of the
texture Linear, empty sets, single pixels.  tests/test_kernel_checks.py proves on the CPU that these checks fail on
the defects they are there for.  Each test prints its worst |err| / bound.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import kernel_checks as kc
from kernel_checks import Guarded

pytestmark = pytest.mark.gpu
dev = "cuda"
BF16, F16, F32, I32 = torch.bfloat16, torch.float16, torch.float32, torch.int32
HALF = pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
ALPHA = 1e-3


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from renderformer_amd import _lib
    _lib.load()


def _ops():
    from renderformer_amd import ops
    return ops


def _report(what: str, ratio: float) -> float:
    print(f"{what}: worst |err| / bound {ratio:.3f}")
    return ratio


def _bits(g: Guarded) -> torch.Tensor:
    torch.cuda.synchronize()
    return g.ibuf.cpu().clone()


# ------------------------------------------------------------------------------------------------ vertex normals
@HALF
@pytest.mark.parametrize("n_freqs,ld", kc.VN_SHAPES)
@pytest.mark.parametrize("n_rows", kc.VN_ROWS)
def test_vn_encode_per_element(n_rows, n_freqs, ld, dtype):
    """rf_vn_encode_dt through a shuffled dst_row with holes, then without a dst_row: every element of every written
    row against fp64 (the padding exactly 0), the rows no input maps to and the guard rows untouched."""
    vn, dst, written = kc.vn_case(n_rows)
    ref, bound = kc.vn_encode_ref(vn, n_freqs, ld), kc.vn_encode_bound(vn, n_freqs, ld, dtype)
    out = Guarded(n_rows, ld, dtype, dev, g=3, ld=ld)  # the kernel writes 0:ldo of a row: guard rows only
    _ops().vn_encode(vn.to(dev), dst.to(dev), n_freqs, out.view)
    torch.cuda.synchronize()
    got = out.view.cpu()
    r1 = kc.assert_elementwise(got[written], kc.vn_scatter(ref, dst)[written], kc.vn_scatter(bound, dst)[written],
                               "scattered")
    assert not bool(got[written][:, 9 * (2 * n_freqs + 1):].float().any()), "padding not zero"
    out.assert_untouched(written_rows=written, what="vn_encode scattered")
    out.reset()
    _ops().vn_encode(vn.to(dev), None, n_freqs, out.view)
    torch.cuda.synchronize()
    r2 = kc.assert_elementwise(out.view.cpu(), ref, bound, "in order")
    out.assert_untouched(what="vn_encode in order")
    _report(f"vn_encode {n_rows} rows L {n_freqs} ld {ld} {dtype}", max(r1, r2))


# ------------------------------------------------------------------------------------------------ RoPE positions
@functools.lru_cache(maxsize=None)
def _scene_expected(counts, n_views):
    tris, valid, off, c2w = kc.scene_case(counts, n_views)
    rows, centres = kc.scene_pos_ref(tris, valid, off, c2w, n_views, 0)
    e_rows, e_centres = kc.scene_pos_bound(tris, valid, off, c2w, n_views, 0)
    return tris, valid, off, c2w, rows, centres, e_rows, e_centres


@pytest.mark.parametrize("n_reg", [0, 16])
@pytest.mark.parametrize("counts,n_views", [(kc.SCENE_COUNTS, 0), (kc.SCENE_COUNTS_VIEWS, 3)], ids=["scenes", "views"])
def test_scene_pos_per_element(counts, n_views, n_reg):
    """rf_scene_pos: 66 blocks (the centre kernel's second round), an empty set, 256 and 257 triangles; with c2w three
    views of 300, 0 and 513.  Rows against the rotate-translate bound (a copy without c2w: exact), centres against the
    reduction bound, two runs bit for bit, nothing outside pos_out written."""
    tris, valid, off, c2w, rows, centres, e_rows, e_centres = _scene_expected(counts, n_views)
    ref, set_off, is_centre = kc.scene_pos_pack(rows, centres, n_reg)
    bound = kc.scene_pos_pack(e_rows, e_centres, n_reg)[0]
    pos = Guarded(ref.shape[0], 9, F32, dev, g=8, ld=9)
    args = (tris.to(dev), valid.to(dev), off.to(dev), None if c2w is None else c2w.contiguous().to(dev), len(counts),
            max(n_views, 1), n_reg, pos.view, set_off.to(dev), max(counts))
    _ops().scene_pos(*args)
    first = _bits(pos)
    pos.assert_untouched(what="scene_pos")
    got = pos.view.cpu()
    pos.reset()
    _ops().scene_pos(*args)
    assert torch.equal(_bits(pos), first), "two runs differ"
    if c2w is None:
        assert torch.equal(got[~is_centre].double(), ref[~is_centre])
    r_rows = kc.assert_elementwise(got[~is_centre], ref[~is_centre], bound[~is_centre], "rows")
    r_c = kc.assert_elementwise(got[is_centre], ref[is_centre], bound[is_centre], "centres") if n_reg else 0.0
    _report(f"scene_pos {counts} views {n_views} n_reg {n_reg}: rows {r_rows:.3f}, centres", r_c)


# ------------------------------------------------------------------------------------------------ HDR output
LAYOUTS = [(cl, ld) for cl in (True, False) for ld in (True, False)]  # (channels_last, log_decode)


def _hdr_out(n, c, h, w, channels_last):
    g = Guarded(n * h * w, c, F32, dev, g=3, ld=c) if channels_last else Guarded(n * c, h * w, F32, dev, g=3, ld=h * w)
    return g, g.view.view((n, h, w, c) if channels_last else (n, c, h, w))


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("n,h,w", kc.HDR_SHAPES)
def test_hdr_output_per_element(n, h, w, c):
    x = kc.hdr_logits(n, c, h, w)
    worst = 0.0
    for channels_last, log_decode in LAYOUTS:
        g, out = _hdr_out(n, c, h, w, channels_last)
        _ops().hdr_output(x.to(dev), out, ALPHA, log_decode, channels_last)
        torch.cuda.synchronize()
        what = f"hdr_output channels_last {channels_last} log_decode {log_decode}"
        worst = max(worst, kc.assert_elementwise(out.cpu(), kc.hdr_ref(x, ALPHA, log_decode, channels_last),
                                                 kc.hdr_bound(x, ALPHA, log_decode, channels_last), what))
        g.assert_untouched(what=what)
    _report(f"hdr_output {n} x {c} x {h} x {w}", worst)


def _windows(h, w):
    oh, ow = min(h, 2), min(w, 5)
    return {"full": (0, 0, h, w), "pixel": (h // 2, w // 3, 1, 1), "corner": (h - oh, w - ow, oh, ow)}


WIN_CASES = [(s, "full") for s in kc.HDR_SHAPES] + [(s, k) for s in ((1, 15, 17), (2, 3, 7)) for k in ("pixel", "corner")]


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("shape,window", WIN_CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{k}" for s, k in WIN_CASES])
def test_hdr_output_window_per_element(shape, window, c):
    """rf_hdr_output_win against hdr_ref of the same window of the logits: the full image, one pixel, and a window that
    ends in the bottom-right corner."""
    n, h, w = shape
    y0, x0, oh, ow = _windows(h, w)[window]
    assert y0 + oh <= h and x0 + ow <= w and (window != "corner" or (y0 + oh == h and x0 + ow == w))
    x = kc.hdr_logits(n, c, h, w)
    xw = x[:, :, y0:y0 + oh, x0:x0 + ow]
    worst = 0.0
    for channels_last, log_decode in LAYOUTS:
        g, out = _hdr_out(n, c, oh, ow, channels_last)
        _ops().hdr_output_window(x.to(dev), out, (y0, x0, oh, ow), ALPHA, log_decode, channels_last)
        torch.cuda.synchronize()
        what = f"hdr_output_window channels_last {channels_last} log_decode {log_decode}"
        worst = max(worst, kc.assert_elementwise(out.cpu(), kc.hdr_ref(xw, ALPHA, log_decode, channels_last),
                                                 kc.hdr_bound(xw, ALPHA, log_decode, channels_last), what))
        g.assert_untouched(what=what)
    _report(f"hdr_output_window {shape} {window} c {c}", worst)


@pytest.mark.parametrize("window", ["full", "pixel", "corner"])
def test_frame_window_guarded(window):
    """rf_frame_window through the C entry point into a guarded buffer: the slice, bit for bit."""
    from renderformer_amd._lib import call, stream
    n, h, w, c = 2, 15, 17, 3
    y0, x0, oh, ow = _windows(h, w)[window]
    frames = torch.randn(n, h, w, c, generator=torch.Generator().manual_seed(5))
    out = Guarded(n * oh * ow, c, F32, dev, g=3, ld=c)
    fd = frames.to(dev)
    call("rf_frame_window", fd.data_ptr(), out.view.data_ptr(), n, h, w, c, y0, x0, oh, ow, stream())
    torch.cuda.synchronize()
    assert torch.equal(out.view.cpu().view(n, oh, ow, c), frames[:, y0:y0 + oh, x0:x0 + ow])
    out.assert_untouched(what="frame_window")


# ------------------------------------------------------------------------------------------------ texture Linear
@pytest.mark.parametrize("ldc", [16, 24])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("rows,channels,n", kc.TEXTURE_LINEAR_SHAPES)
def test_texture_linear_per_element(rows, channels, n, with_bias, ldc):
    """rf_texture_linear: one row, a partial last block of 16, idle threads (n < 1024), the second 1024-column trip
    (n > 1024), 1 and 16 channels; coef's padding columns and surrounding rows are NaN; out has ld = n + 8.  With the
    flag raised nothing is written."""
    coef, wsum, bias = kc.texture_linear_case(rows, channels, n)
    bias = bias if with_bias else None
    gc = Guarded(rows, channels, F32, dev, g=2, ld=ldc).fill(coef)
    out = Guarded(rows, n, F32, dev, g=2, ld=n + 8)
    flag = torch.ones(1, dtype=I32, device=dev)
    wd, bd = wsum.to(dev), None if bias is None else bias.to(dev)
    _ops().texture_linear(gc.view, wd, bd, out.view, flag)
    torch.cuda.synchronize()
    out.assert_untouched(written_rows=torch.zeros(rows, dtype=torch.bool), what="texture_linear with the flag raised")
    flag.zero_()
    _ops().texture_linear(gc.view, wd, bd, out.view, flag)
    torch.cuda.synchronize()
    got = out.view.cpu()
    kc.assert_finite(got, "texture_linear")
    ratio = kc.assert_elementwise(got, kc.texture_linear_ref(coef, wsum, bias), kc.texture_linear_bound(coef, wsum, bias),
                                  "texture_linear")
    out.assert_untouched(what="texture_linear")
    _report(f"texture_linear {rows} x {channels} -> {n} bias {with_bias} ldc {ldc}", ratio)


# ------------------------------------------------------------------------------------------------ texture scan / pack
TEX_ROWS = 5
TEX_DST = (3, 0, -1, 4, 1)  # input row -> coef / out row: shuffled, input row 2 is padding, output row 2 gets nothing
TEX_CASES = [(c, lc) for c in (1, 13, 32) for lc in sorted({0, min(3, c), c})]


def _texture(channels, seed=0):
    """[1, 5, C, 32, 32] of the to_h5 form: a constant in [0, 4) per row and channel inside the patch mask, 0 outside."""
    from renderformer_amd.scenes import texture_mask
    g = torch.Generator(device="cpu").manual_seed(6000 + seed)
    const = torch.rand(1, TEX_ROWS, channels, generator=g) * 4
    return (const[..., None, None] * torch.from_numpy(texture_mask(32)).float()).contiguous()


def _tex_written():
    w = torch.zeros(TEX_ROWS, dtype=torch.bool)
    w[[d for d in TEX_DST if d >= 0]] = True
    return w


def _scan(tex, channels, log_ch, flag_init=5, flag_clear_init=None):
    """One rf_texture_scan (or, with flag_clear_init, rf_texture_scan2 from flag 0) -> (texture after, coef Guarded,
    flags after as a list)."""
    t = tex.clone().to(dev)
    dst = torch.tensor(TEX_DST, dtype=I32, device=dev)
    coef = Guarded(TEX_ROWS, channels, F32, dev, g=2, ld=40)
    two = flag_clear_init is not None
    flags = Guarded(1, 2 if two else 1, I32, dev)
    flags.view[0, 0] = 0 if two else flag_init
    if two:
        flags.view[0, 1] = flag_clear_init
    _ops().texture_scan(t, log_ch, dst, coef.view, flags.view[0, 0:1], flags.view[0, 1:2] if two else None)
    torch.cuda.synchronize()
    flags.assert_untouched(what="scan flags")
    return t.cpu(), coef, flags.view[0].tolist()


def _check_encode(tex, enc, channels, log_ch, what):
    lo = channels - log_ch
    assert torch.equal(enc[:, :, :lo], tex[:, :, :lo]), f"{what}: a channel below log_from changed"
    if not log_ch:
        return 0.0
    ref, bound = kc.log_encode_ref(tex[:, :, lo:])
    return kc.assert_elementwise(enc[:, :, lo:], ref, bound, what)


@pytest.mark.parametrize("channels,log_ch", TEX_CASES)
def test_texture_scan_per_element(channels, log_ch):
    """rf_texture_scan and rf_texture_scan2: the in-place encode of all five rows (the padded one too) against fp64
    log10(fl32(x + 1)), coef rows at dst_row equal to texel (0, 0) of the encoded row bit for bit, the coef row nothing
    maps to and coef's padding untouched, the flag raised by a valid row that leaves the form (inside or outside the
    mask, or NaN) and not by the padded row, and scan2's two flags as rf.h states from both values of the second."""
    tex = _texture(channels)
    enc, coef, flags = _scan(tex, channels, log_ch)
    assert flags == [0]
    ratio = _check_encode(tex, enc, channels, log_ch, "scan encode")
    written = _tex_written()
    coef.assert_untouched(written_rows=written, what="scan coef")
    cv = coef.view.cpu()
    for r, d in enumerate(TEX_DST):
        if d >= 0:
            assert torch.equal(cv[d], enc[0, r, :, 0, 0]), (r, d)
    ch = channels - 1  # the last channel: log-encoded whenever any is
    bad_out, bad_in, bad_pad, bad_nan = tex.clone(), tex.clone(), tex.clone(), tex.clone()
    bad_out[0, 3, ch, 31, 2] = 0.5   # outside the mask (31 + 2 > 32), valid row
    bad_in[0, 0, ch, 31, 1] += 0.5   # inside the mask (31 + 1 <= 32), valid row
    bad_pad[0, 2, ch, 3, 3] += 1.0   # the padded row: only encoded
    bad_nan[0, 4, 0, 0, 0] = float("nan")
    assert [_scan(t, channels, log_ch)[2] for t in (bad_out, bad_in, bad_pad, bad_nan)] == [[1], [1], [0], [1]]
    for t, raised in ((tex, 0), (bad_in, 1)):
        for clear_init in (0, 1):
            enc2, coef2, flags2 = _scan(t, channels, log_ch, flag_clear_init=clear_init)
            assert flags2 == [raised, 0], (raised, clear_init, flags2)
            coef2.assert_untouched(written_rows=written, what="scan2 coef")
            if not raised:
                assert torch.equal(enc2, enc) and torch.equal(coef2.view.cpu()[written], cv[written])
    _report(f"texture_scan C {channels} log {log_ch}", ratio)


@pytest.mark.parametrize("channels,log_ch", TEX_CASES)
def test_texture_pack_per_element(channels, log_ch):
    """rf_texture_pack / rf_texture_pack_if: the encode against fp64 (and equal to the scan's bits), out = RNE bf16 of
    the encoded rows at dst_row with ld = C 1024 + 8, the hole row and the padding untouched; pack_if with the flag at
    0 changes neither the texture nor out."""
    ops = _ops()
    tex = _texture(channels)
    dst = torch.tensor(TEX_DST, dtype=I32, device=dev)
    written = _tex_written()
    n = channels * 1024

    def expect(t, out, what):
        torch.cuda.synchronize()
        enc = t.cpu()
        ratio = _check_encode(tex, enc, channels, log_ch, what)
        out.assert_untouched(written_rows=written, what=what)
        ov = out.view.cpu()
        for r, d in enumerate(TEX_DST):
            if d >= 0:
                assert torch.equal(ov[d], enc[0, r].reshape(-1).bfloat16()), (what, r, d)
        return enc, ratio

    t, out = tex.clone().to(dev), Guarded(TEX_ROWS, n, BF16, dev, g=2, ld=n + 8)
    ops.texture_pack(t, log_ch, dst, out.view)
    enc, ratio = expect(t, out, "pack")
    assert torch.equal(enc, _scan(tex, channels, log_ch)[0]), "pack and scan encode differently"
    t, out = tex.clone().to(dev), Guarded(TEX_ROWS, n, BF16, dev, g=2, ld=n + 8)
    flag = torch.zeros(1, dtype=I32, device=dev)
    ops.texture_pack_if(flag, t, log_ch, dst, out.view)
    torch.cuda.synchronize()
    assert torch.equal(t.cpu(), tex)
    out.assert_untouched(written_rows=torch.zeros(TEX_ROWS, dtype=torch.bool), what="pack_if with the flag at 0")
    flag.fill_(1)
    ops.texture_pack_if(flag, t, log_ch, dst, out.view)
    assert torch.equal(expect(t, out, "pack_if")[0], enc)
    _report(f"texture_pack C {channels} log {log_ch}", ratio)


# ------------------------------------------------------------------------------------------------ rays
RAY_VIEWS, RAY_FRAME, RAY_PATCH = 3, (24, 40), 8  # 960 pixels: 3 full blocks and one of 192
# (mode, requested frame, origin): the plain entry point; intrinsics on the whole frame; an 8 x 24 frame at (8, 8)
RAY_CASES = [("hw", RAY_FRAME, (0, 0)), ("intr", RAY_FRAME, (0, 0)), ("intr", (8, 24), (8, 8)), ("fov", (8, 24), (8, 8))]


@HALF
@pytest.mark.parametrize("with_pos", [True, False], ids=["pos", "nopos"])
@pytest.mark.parametrize("mode,frame,origin", RAY_CASES, ids=["hw", "cam-intr", "cam-intr-overscan", "cam-fov-overscan"])
def test_ray_tokens_per_element(mode, frame, origin, with_pos, dtype):
    ops = _ops()
    c2w, fov, intr = kc.camera_case(RAY_VIEWS)
    h, w = RAY_FRAME
    p = RAY_PATCH
    use_intr = mode == "intr"
    ref, ref_pos, bound = kc.ray_tokens_ref(c2w, None if use_intr else fov, intr if use_intr else None, frame, RAY_FRAME,
                                            origin, p, dtype)
    tok = Guarded(RAY_VIEWS * (h // p) * (w // p), 3 * p * p, dtype, dev, g=4, ld=3 * p * p)
    pos = Guarded(RAY_VIEWS, 9, F32, dev, g=2, ld=9) if with_pos else None
    pv = pos.view if with_pos else None
    if mode == "hw":
        ops.ray_tokens(c2w.to(dev), fov.to(dev), RAY_FRAME, p, tok.view, pv)
    else:
        ops.ray_tokens_cam(c2w.to(dev), None if use_intr else fov.to(dev), intr.to(dev) if use_intr else None, frame,
                           RAY_FRAME, origin, p, tok.view, pv)
    torch.cuda.synchronize()
    ratio = kc.assert_elementwise(tok.view.cpu(), ref, bound, f"ray tokens {mode}")
    tok.assert_untouched(what="ray tokens")
    if with_pos:
        assert torch.equal(pos.view.cpu().double(), ref_pos)
        pos.assert_untouched(what="ray_pos")
    _report(f"ray_tokens {mode} frame {frame} at {origin} {dtype}", ratio)


@HALF
def test_patchify_rays_guarded(dtype):
    h, w = RAY_FRAME
    p = RAY_PATCH
    rays = torch.randn(RAY_VIEWS, h, w, 3, generator=torch.Generator().manual_seed(8))
    tok = Guarded(RAY_VIEWS * (h // p) * (w // p), 3 * p * p, dtype, dev, g=4, ld=3 * p * p)
    _ops().patchify_rays(rays.to(dev), p, tok.view)
    torch.cuda.synchronize()
    assert torch.equal(tok.view.cpu(), kc.patchify_ref(rays, p).to(dtype))  # one RNE rounding of a copy
    tok.assert_untouched(what="patchify_rays")


# ------------------------------------------------------------------------------------------------ fp32 resize
@pytest.mark.parametrize("f16", [False, True], ids=["bf16x3", "f16"])
@pytest.mark.parametrize("hi,ho,c,p_ld", [(4, 9, 12, 20), (5, 7, 16, 24)])  # the 4- and the 8-channel-per-thread kernel
def test_upsample_bilinear_guarded(hi, ho, c, p_ld, f16):
    """rf_upsample_bilinear through the C entry point: the input inside NaN rows, `out` and the planes (p_ld > c) in
    guarded buffers; test_upsample_bilinear_align_corners' value check per element against F.interpolate in fp64; the
    plane-only launch writes the same planes."""
    from renderformer_amd._lib import call, stream
    n = 2
    x = torch.randn(n, c, hi, hi, generator=torch.Generator().manual_seed(hi + c))
    ref = F.interpolate(x.double(), size=(ho, ho), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).reshape(-1, c)
    bound = 1e-5 + 1e-5 * ref.abs()
    gin = Guarded(n * hi * hi, c, F32, dev, g=2 * (hi + 2), ld=c).fill(x.permute(0, 2, 3, 1).reshape(-1, c))
    pix = n * ho * ho
    pdt = F16 if f16 else BF16

    def launch(want_out):
        out = Guarded(pix, c, F32, dev, g=4, ld=c) if want_out else None
        p_hi = Guarded(pix, c, pdt, dev, g=4, ld=p_ld)
        p_lo = None if f16 else Guarded(pix, c, pdt, dev, g=4, ld=p_ld)
        call("rf_upsample_bilinear", gin.view.data_ptr(), n, hi, hi, c, out.view.data_ptr() if out else 0, ho, ho,
             p_hi.view.data_ptr(), p_lo.view.data_ptr() if p_lo else 0, p_ld, stream())
        torch.cuda.synchronize()
        for name, g in (("out", out), ("plane hi", p_hi), ("plane lo", p_lo)):
            if g is not None:
                g.assert_untouched(what=f"upsample {name}")
        return out, p_hi, p_lo

    out, p_hi, p_lo = launch(True)
    got = out.view.cpu()
    kc.assert_finite(got, "upsample")
    ratio = kc.assert_elementwise(got, ref, bound, "upsample out")
    if f16:
        assert torch.equal(p_hi.view.cpu(), got.half())  # RNE fp16 of the fp32 value
    else:
        ratio = max(ratio, kc.assert_elementwise(p_hi.view.cpu().float() + p_lo.view.cpu().float(), ref, bound, "planes"))
    _, q_hi, q_lo = launch(False)
    assert torch.equal(q_hi.view.cpu(), p_hi.view.cpu()) and (f16 or torch.equal(q_lo.view.cpu(), p_lo.view.cpu()))
    _report(f"upsample {hi} -> {ho}, c {c}, {'f16' if f16 else 'bf16x3'}", ratio)
