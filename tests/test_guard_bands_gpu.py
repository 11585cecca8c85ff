"""Guard bands around the row kernels' outputs and inputs, and rf_embed against fp64.

Every entry point whose C signature takes a leading dimension for what it writes gets a kernel_checks.Guarded output
(guard rows, ld above the width, a sentinel everywhere outside the view) and NaN-surrounded strided inputs, one small
shape per vector-width path with a row count that is no multiple of the 4 rows of a block; the value check is the one
the op's older test makes, applied to every element.  rf_embed, reached until now only through whole-frame parity, is
compared with fp64 per element on both of its paths, which must agree bit for bit.  The last section guards every
buffer of the DPT convolution entry points.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc
import kernel_checks as kc
from kernel_checks import Guarded
from oracle import rf_ref

pytestmark = pytest.mark.gpu
dev = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
EPS = 1e-6
U = kc.U_OUT


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from renderformer_amd import _lib
    _lib.load()


def _ops():
    from renderformer_amd import ops
    return ops


def _gin(t, **kw):
    """A NaN-surrounded strided input holding t."""
    return Guarded(t.shape[0], t.shape[1], t.dtype, dev, **kw).fill(t)


def _vec(x):
    return Guarded(1, x.numel(), x.dtype, dev).fill(x[None])


def _round_bound(ref, dtype, slack):
    """One RNE rounding of a value computed in fp32 within `slack` (absolute, per element) of ref; fp16 below its
    normal range rounds to a spacing of 2^-24 (half of it: 2^-25)."""
    b = U[dtype] * (ref.abs() + slack) + slack
    return b + 2.0 ** -25 if dtype == F16 else b


# ------------------------------------------------------------------------------------------------ RMSNorm, pre-norm
# dim / 256 in {2, 3, 4, 6, 8}: the whole-row vector kernels; 320 and 1280: the generic loop
@pytest.mark.parametrize("odt", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("dim", [512, 768, 1024, 1536, 2048, 320, 1280])
def test_rmsnorm_guarded(dim, odt):
    """test_rmsnorm's check per element: out = RNE(x w / rms(x)), the fp32 value within 8 ulps (the row sum, the
    divide, eps, sqrt, the reciprocal and two multiplies) of fp64."""
    ops = _ops()
    rows = 7
    g = torch.Generator(device="cpu").manual_seed(dim)
    x = torch.randn(rows, dim, generator=g) * 3
    w = torch.rand(dim, generator=g) + 0.5
    gx, gw = _gin(x), _vec(w)
    gout = Guarded(rows, dim, odt, dev, col_off=4)  # an origin that is 8-byte but not 16-byte aligned
    assert gout.view.data_ptr() % 16 == 8
    ops.rmsnorm(gx.view, gw.view[0], EPS, gout.view)
    ref = F.rms_norm(x.double(), (dim,), w.double(), EPS)
    kc.assert_elementwise(gout.view, ref, _round_bound(ref, odt, 8 * kc.F32_ULP * ref.abs()), f"rmsnorm {dim}")
    gout.assert_untouched(what=f"rmsnorm {dim}")


@pytest.mark.parametrize("odt", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("dim", [768, 320])
def test_prenorm_guarded(dim, odt):
    """test_prenorm_row_form's checks: xg = RNE(x w) bit for bit, slot 0 = sum x^2, the other slots 0; xg, ss guarded.
    The sum per element: a lane squares and adds its dim / 64 columns, then 6 butterfly adds across the wave, each
    operation within half an fp32 ulp of a partial sum: (dim / 64 + 8) 2^-24 of the sum."""
    ops = _ops()
    rows = 7
    g = torch.Generator(device="cpu").manual_seed(dim + 1)
    x = torch.randn(rows, dim, generator=g) * 3
    w = torch.rand(dim, generator=g) + 0.5
    gx, gw = _gin(x), _vec(w)
    gxg, gss = Guarded(rows, dim, odt, dev, col_off=4), Guarded(rows, 8, F32, dev, ld=8)
    ops.prenorm(gx.view, gw.view[0], gxg.view, gss.view)
    assert torch.equal(gxg.view.cpu(), (x * w).to(odt))
    ss = (x.double() ** 2).sum(1)
    kc.assert_elementwise(gss.view[:, 0], ss, (dim / 64 + 8) * 2.0 ** -24 * ss, "ss slot 0")
    assert torch.equal(gss.view[:, 1:], torch.zeros_like(gss.view[:, 1:]))
    gxg.assert_untouched(what="xg")
    gss.assert_untouched(what="ss")


# ------------------------------------------------------------------------------------------------ q/k norm + RoPE
def _rope_ref(z, pos, freqs, H):
    """The oracle's rotation in fp64 on the standard (half-split) layout; z [T, H * 128]."""
    cos, sin = rf_ref.rope_cos_sin(pos.double()[None], freqs.double(), 128)
    return rf_ref.rope_apply(z.view(1, -1, H, 128).transpose(1, 2), cos, sin).transpose(1, 2).reshape(z.shape)


def _rope_bound(z, ref, H):
    """out = RNE_bf16(z_a cos - z_b sin) computed in fp32: the normalised, weighted pair (z_a, z_b) = (z[m], z[m +- 64])
    is within 8 ulps of fp64 (as in test_rmsnorm_guarded), sin / cos of an angle |pos| freq <= 5 within 4 ulps of 1,
    the two products and the add 3 more: 2^-20 (16 ulps) of |z_a| + |z_b|, then one bf16 rounding."""
    T = z.shape[0]
    pair = z.abs().view(T, H, 2, 64)
    pair = (pair + pair.flip(2)).reshape(T, H * 128)
    return _round_bound(ref, BF16, 2.0 ** -20 * pair)


def _qk_case(T, H, n_seg, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    D = H * 128
    src = torch.randn(T, n_seg * D + 128, generator=g).to(BF16)  # (one more head to the right: a neighbour's data)
    w = torch.rand(n_seg * D, generator=g) + 0.5
    pos = torch.rand(T, 9, generator=g) * 2 - 1
    freqs = 2 ** torch.linspace(0, math.log2(5), 6)
    return src, w, pos, freqs


# units = n_seg * heads * 8 work units a row: <= 64 one a lane, <= 128 two, else four
@pytest.mark.parametrize("H,n_seg,split", [(2, 1, "1"), (8, 2, "1"), (16, 1, "1"), (8, 2, "0"), (16, 2, "0")])
def test_qk_norm_rope_guarded(monkeypatch, H, n_seg, split):
    """rf_qk_norm_rope (test_qk_norm_rope_matches_oracle's reference, per element) into a guarded dst from a
    NaN-surrounded src, gathered rows and a shared position per two rows included; the same bits as on dense buffers."""
    ops = _ops()
    monkeypatch.setenv("RF_QKN_SPLIT", split)
    T, D = 7, H * 128
    src, w, pos, freqs = _qk_case(T, H, n_seg, H + n_seg)
    rows = torch.tensor([5, 0, 6, 5, 2], dtype=torch.int32)
    q_scale = 0.37
    gsrc, gw, gpos = _gin(src), _vec(w), _gin(pos, ld=12)
    fd, rd = freqs.to(dev), rows.to(dev)
    for gather in (False, True):
        n, div = (rows.numel(), 2) if gather else (T, 1)
        gdst = Guarded(n, n_seg * D, BF16, dev)
        ops.qk_norm_rope(gsrc.view[:, :n_seg * D], gdst.view, H, gw.view[0], EPS, gpos.view, fd, pos_div=div,
                         src_rows=rd if gather else None, n_seg=n_seg, q_scale=q_scale)
        dense = torch.empty(n, n_seg * D, dtype=BF16, device=dev)
        ops.qk_norm_rope(src[:, :n_seg * D].contiguous().to(dev), dense, H, w.to(dev), EPS, pos.to(dev), fd,
                         pos_div=div, src_rows=rd if gather else None, n_seg=n_seg, q_scale=q_scale)
        assert torch.equal(gdst.view, dense)
        x = src[rows.long()] if gather else src
        p = pos[torch.arange(n) // div]
        for s in range(n_seg):
            z = F.rms_norm(x[:, s * D:(s + 1) * D].double(), (D,), w[s * D:(s + 1) * D].double(), EPS)
            z = z * (q_scale if s == 0 else 1.0)
            ref = _rope_ref(z, p, freqs, H)
            kc.assert_elementwise(gdst.view[:, s * D:(s + 1) * D], ref, _rope_bound(z, ref, H),
                                  f"seg {s} gather {gather}")
        gdst.assert_untouched(what=f"gather {gather}")


@pytest.mark.parametrize("ilv", [False, True], ids=["std", "ilv"])
@pytest.mark.parametrize("H", [2, 16])
def test_qk_norm_rope_groups_guarded(H, ilv):
    """rf_qk_norm_rope_groups and its pair-interleaved form: 3 groups at a column stride of 2 D in src, D in dst; the
    V columns between the groups of src hold NaN, dst is guarded, per element against the oracle (in the interleaved
    order: of the permuted row)."""
    ops = _ops()
    T, G, D = 7, 3, H * 128
    g = torch.Generator(device="cpu").manual_seed(H)
    kv = torch.randn(T, G * 2 * D, generator=g).to(BF16)
    w = torch.rand(G * D, generator=g) + 0.5
    pos = torch.rand(T, 9, generator=g) * 2 - 1
    freqs = 2 ** torch.linspace(0, math.log2(5), 6)
    perm = ops.rope_pair_perm(D) if ilv else torch.arange(D)
    src = torch.full((T, G * 2 * D), float("nan")).to(BF16)
    wp = torch.empty_like(w)
    for i in range(G):
        src[:, 2 * D * i:2 * D * i + D] = kv[:, 2 * D * i:2 * D * i + D][:, perm]
        wp[D * i:D * (i + 1)] = w[D * i:D * (i + 1)][perm]
    gsrc, gw, gpos = _gin(src), _vec(wp), _gin(pos, ld=12)
    gdst = Guarded(T, G * D, BF16, dev)
    ops.qk_norm_rope_groups(gsrc.view, 2 * D, gdst.view, D, G, H, gw.view[0], EPS, gpos.view, freqs.to(dev),
                            seg0_scale=2.5, ilv=ilv)
    kc.assert_finite(gdst.view)
    for i in range(G):
        z = F.rms_norm(kv[:, 2 * D * i:2 * D * i + D].double(), (D,), w[D * i:D * (i + 1)].double(), EPS) * 2.5
        ref = _rope_ref(z, pos, freqs, H)
        kc.assert_elementwise(gdst.view[:, D * i:D * (i + 1)], ref[:, perm], _rope_bound(z, ref, H)[:, perm],
                              f"group {i}")
    gdst.assert_untouched()


# dims: <= 512 one 16-byte chunk a lane, <= 1024 two, else four; 264 / 776 / 1544 leave lanes of the last chunk idle
@pytest.mark.parametrize("dim", [256, 264, 776, 1024, 1544, 2048])
def test_row_rms_scale_guarded(dim):
    """rf_row_rms_scale in place on a guarded x with the 8 partial sums read from a strided, NaN-surrounded ss:
    x' = RNE(x scale / rms), the factor in fp32 within 12 ulps (7 adds, divide, eps, sqrt, divide, multiply)."""
    ops = _ops()
    rows = 7
    g = torch.Generator(device="cpu").manual_seed(dim)
    x = torch.randn(rows, dim, generator=g).to(BF16)
    ss = torch.rand(rows, 8, generator=g) * dim / 4 + 1.0
    ss[:, 5:] = 0
    gx = _gin(x)
    gss = Guarded(rows, 8, F32, dev, ld=16, col_off=8).fill(ss)  # (seg_ss[:, 1] of a [rows, 2, 8] buffer)
    ops.row_rms_scale(gx.view, gss.view, EPS, scale=0.37)
    ref = x.double() * 0.37 / torch.sqrt(ss.double().sum(1, keepdim=True) / dim + EPS)
    kc.assert_elementwise(gx.view, ref, _round_bound(ref, BF16, 12 * kc.F32_ULP * ref.abs()), f"dim {dim}")
    gx.assert_untouched(what=f"dim {dim}")


# ------------------------------------------------------------------------------------------------ MX fp8 quantiser
@pytest.mark.parametrize("rows,cols", [(5, 96), (7, 1024)])
def test_quant_mx8_guarded(rows, cols):
    """test_quant_mx8_matches_reference's check (every scale and e4m3 byte equals the torch reference) on guarded q and
    scales, from a NaN-surrounded x."""
    ops = _ops()
    g = torch.Generator(device="cpu").manual_seed(rows + cols)
    x = (torch.randn(rows, cols, generator=g) * torch.logspace(-3, 3, cols)[None]).to(BF16)
    x[0, :32] = 0
    gx = _gin(x)
    gq = Guarded(rows, cols, torch.uint8, dev, ld=cols + 16)
    gs = Guarded(rows, cols // 32, torch.uint8, dev, ld=cols // 32 + 5)
    ops.quant_mx8(gx.view, ops.MX8(gq.view, gs.view))
    q_ref, s_ref = ops.mx8_quant_ref(x)
    assert torch.equal(gs.view.cpu(), s_ref) and torch.equal(gq.view.cpu(), q_ref)
    gq.assert_untouched(what="q")
    gs.assert_untouched(what="scales")


# ------------------------------------------------------------------------------------------------ DPT planes
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("f16", [False, True], ids=["bf16x3", "f16"])
def test_split_planes_guarded(f16, silu):
    """rf_split_planes (dpt.split_planes allocates its own planes, so through the C entry point): p_ld above c, guarded
    planes, x with ldx above c and NaN around.  fp16: the plane is RNE(x) bit for bit (test_split_planes_f16_rounding);
    bf16 hi / lo: hi = RNE(x), lo = RNE(x - hi), rf.h's definition; silu: that test's tolerance per element."""
    from renderformer_amd import _lib
    rows, c = 37, 20  # 185 threads: no multiple of the block
    g = torch.Generator(device="cpu").manual_seed(c)
    x = torch.randn(rows, c, generator=g) * 100
    x[0, :4] = torch.tensor([6e4, -6e4, 1e-8, 65504.0])
    gx = _gin(x, ld=24)
    dt = F16 if f16 else BF16
    ghi, glo = Guarded(rows, c, dt, dev, ld=28), (None if f16 else Guarded(rows, c, dt, dev, ld=28))
    _lib.call("rf_split_planes", gx.view.data_ptr(), rows, c, gx.ld, ghi.view.data_ptr(),
              glo.view.data_ptr() if glo else None, 28, int(silu), _lib.stream())
    v = F.silu(x) if silu else x
    hi = ghi.view.cpu()
    if silu:
        got = hi.float() if f16 else hi.float() + glo.view.cpu().float()
        kc.assert_elementwise(got, v, 1e-3 * v.abs() + 1e-6, "silu planes")
    elif f16:
        assert torch.equal(hi, x.half())
    else:
        assert torch.equal(hi, x.to(BF16)) and torch.equal(glo.view.cpu(), (x - x.to(BF16).float()).to(BF16))
    ghi.assert_untouched(what="hi")
    if glo:
        glo.assert_untouched(what="lo")


@pytest.mark.parametrize("hi,ho,c,ld_in,ld_out", [(4, 9, 16, 24, 40), (5, 7, 40, 48, 48)])
def test_upsample_planes_guarded(hi, ho, c, ld_in, ld_out):
    """rf_upsample_bilinear_h (dpt.upsample_planes allocates its own plane, so through the C entry point): in_ld and
    p_ld above c, the padded channels of the input hold NaN and those of the output keep the sentinel;
    test_upsample_planes_f16_in's per-element check against F.interpolate."""
    from renderformer_amd import _lib
    n = 2
    g = torch.Generator(device="cpu").manual_seed(hi + c)
    x = torch.randn(n, hi, hi, c, generator=g).half()
    gin = _gin(x.view(-1, c), ld=ld_in)
    gout = Guarded(n * ho * ho, c, F16, dev, ld=ld_out)
    _lib.call("rf_upsample_bilinear_h", gin.view.data_ptr(), ld_in, n, hi, hi, c, ho, ho, gout.view.data_ptr(), ld_out,
              _lib.stream())
    ref = F.interpolate(x.float().permute(0, 3, 1, 2), size=(ho, ho), mode="bilinear", align_corners=True)
    ref = ref.permute(0, 2, 3, 1).reshape(-1, c)
    kc.assert_elementwise(gout.view, ref, float(ref.abs().max()) * 2.0 ** -10, "one fp16 rounding")
    gout.assert_untouched()


# ------------------------------------------------------------------------------------------------ rf_embed
def _embed_ref(base, base_rows, in0, w0, in1, w1, rows, eps):
    """fp64 of (base + in0 s0 w0) + in1 s1 w1 and the per-element bound 4 x 2^-24 sum |terms| (the two adds, each
    within half an ulp of a partial sum, and the rounding of each product) + 2^-22 |term| for each normalised term
    (its 1 / rms: the row sum, divide, eps, sqrt, reciprocal: 4 ulps)."""
    b = base.double()[torch.arange(rows) % base_rows]
    ref, mag, rms = b.clone(), b.abs(), torch.zeros_like(b)
    for x, w in ((in0, w0), (in1, w1)):
        if x is None:
            continue
        t = x.double() / torch.sqrt((x.double() ** 2).mean(1, keepdim=True) + eps) * w.double()
        ref, mag, rms = ref + t, mag + t.abs(), rms + t.abs()
    return ref, 4 * 2.0 ** -24 * mag + 2.0 ** -22 * rms


EMBED_CASES = {
    # name: (dim, out ld - dim, in0 column offset); a vector launch needs dim % 256 == 0, ld % 4 == 0, 16-byte pointers
    "vec768": (768, 8, 0), "vec1024": (1024, 8, 0), "vec1536": (1536, 8, 0), "vec2048": (2048, 8, 0),
    "scalar320": (320, 8, 0),
    "scalar1024_ldo": (1024, 6, 0),   # ldo % 4 != 0
    "scalar1024_in0": (1024, 8, 1),   # in0 4-byte but not 16-byte aligned
}


@pytest.mark.parametrize("case", list(EMBED_CASES))
def test_embed_matches_fp64(case):
    """rf_embed on the vector kernels (dim / 256 in {3, 4, 6, 8}) and the scalar fallback (another dim, a row stride
    that is no multiple of 4, a misaligned input): rows 1 / 5 / 77, base_rows 1 / rows, in0 and in1 each present and
    absent, the rows scattered by a permutation with holes (the holes keep the sentinel), guarded out, NaN-surrounded
    inputs; per element against fp64.  Where dim allows both paths they agree bit for bit on the same inputs."""
    ops = _ops()
    dim, pad, off0 = EMBED_CASES[case]
    eps = ops.FLT_EPS
    for rows in (1, 5, 77):
        g = torch.Generator(device="cpu").manual_seed(dim + rows)
        in0, in1 = torch.randn(rows, dim, generator=g) * 2, torch.randn(rows, dim, generator=g) * 0.5
        w0, w1 = torch.rand(dim, generator=g) + 0.5, torch.rand(dim, generator=g) + 0.5
        g0, g1 = _gin(in0, col_off=off0, ld=dim + 8), _gin(in1)
        gw0, gw1 = _vec(w0), _vec(w1)
        out_rows = torch.randperm(2 * rows + 3, generator=g)[:rows].int()
        written = torch.zeros(2 * rows + 3, dtype=torch.bool)
        written[out_rows.long()] = True
        for base_rows in sorted({1, rows}):
            base = torch.randn(base_rows, dim, generator=g)
            gbase = Guarded(base_rows, dim, F32, dev, ld=dim).fill(base)  # (base rows are dense: stride dim)
            for use0 in (True, False):
                for use1 in (True, False):
                    a0, a1 = (in0 if use0 else None), (in1 if use1 else None)
                    ref, bound = _embed_ref(base, base_rows, a0, w0, a1, w1, rows, eps)
                    outs = []
                    for ld_pad in ([pad, 6] if dim % 256 == 0 and pad != 6 and off0 == 0 else [pad]):
                        gout = Guarded(2 * rows + 3, dim, F32, dev, ld=dim + ld_pad)
                        ops.embed(gout.view, out_rows.to(dev), rows, gbase.view, base_rows,
                                  g0.view if use0 else None, gw0.view[0] if use0 else None, eps,
                                  g1.view if use1 else None, gw1.view[0] if use1 else None, eps)
                        tag = f"{case} rows {rows} base_rows {base_rows} in0 {use0} in1 {use1} ld +{ld_pad}"
                        got = gout.view[out_rows.long().to(dev)]
                        kc.assert_elementwise(got, ref, bound, tag)
                        gout.assert_untouched(written_rows=written, what=tag)
                        outs.append(got)
                    if len(outs) == 2:
                        assert torch.equal(outs[0], outs[1]), f"{tag}: vector and scalar kernels differ"
                    elif case == "scalar1024_in0":  # against the vector kernel on an aligned copy of in0
                        gout = Guarded(2 * rows + 3, dim, F32, dev, ld=dim + 8)
                        ops.embed(gout.view, out_rows.to(dev), rows, gbase.view, base_rows,
                                  _gin(in0).view if use0 else None, gw0.view[0] if use0 else None, eps,
                                  g1.view if use1 else None, gw1.view[0] if use1 else None, eps)
                        assert torch.equal(gout.view[out_rows.long().to(dev)], outs[0]), f"{tag}: vector vs scalar"


# ------------------------------------------------------------------------------------------------ DPT convolutions
# The M-tail, padded-bank, deconvolution, NCHW-head, multi-image and grouped cases of conv_cases.py with every device
# buffer but the weights guarded (kernel_checks.ConvLaunch): 256 sentinel rows around `out` and the planes, sentinel
# padding columns in the planes (rf.h: the caller zeroes them, a kernel never writes them), NaN around the operand
# planes (the rows before image 0 and after the last image), the residuals and the bias rows.  Integer operands: the
# outputs must be finite and bit-equal to fp64 all the same.  Each case launches twice, the allocation reset in
# between and the planes at another column offset, so no value of the first launch can pass for the second.
CONV_GUARDED = ["ring64-mtail", "ring64-padded-bank", "ring64-stride2", "ring25664-bank32", "tile2561-gather",
                "tile256-gather", "sk64", "sk128", "sk1288-1x1", "hs-3img-3chunk", "hs-163264", "halo2-4128",
                "halo2-4064", "halo3", "halo3-16chunk", "tile128-halo", "tile25664-halo", "deconv2", "deconv4",
                "deconv2-tile256", "phased-dense", "phased-gather", "bf-sk128", "bf-ring2561", "bf-deconv4"]


@pytest.mark.parametrize("cid", CONV_GUARDED)
def test_conv_guarded(cid, monkeypatch):
    case = cc.BY_ID[cid]
    cc.set_env(case, monkeypatch)
    L, ref = cc.exact_case(case, dev, seed=7 + len(cid))
    cc.assert_plan(case, L)
    for ld, col_off in ((case.cout + 8, 4), (case.cout + 40, 24)):
        out, hi, lo = L(want_out=True, plane_ld=ld, col_off=col_off)
        what = f"{cid} col_off {col_off}"
        kc.assert_finite(out, what)
        assert torch.equal(L.shaped(out).double(), ref), what
        ehi, elo = kc.exact_planes(ref, L.conv.f16)
        assert torch.equal(L.shaped(hi), ehi) and (elo is None or torch.equal(L.shaped(lo), elo)), what
        L.assert_untouched(what)  # guard rows and padding columns still hold the sentinel
        for g_ in (L.out, L.p_hi, L.p_lo):
            if g_ is not None:
                g_.reset()
    out, hi, lo = L(want_out=False, plane_ld=case.cout + 8, col_off=0)  # plane-only: the fp16 frame's form
    assert torch.equal(L.shaped(hi), kc.exact_planes(ref, L.conv.f16)[0]), cid
    L.assert_untouched(cid + " plane-only")


@pytest.mark.parametrize("nchw", [True, False], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("cid", ["head-c32", "head-halo2", "head-ring"])
def test_conv_head_guarded(cid, nchw, monkeypatch):
    """The fused head's only output, [n n_fin, h w] (NCHW) or [pixels, n_fin], inside 256 guard rows; w_fin and b_fin
    NaN-surrounded too.  Two launches must agree bit for bit and stay finite (the values: test_conv_exact_gpu.py)."""
    case = cc.BY_ID[cid]
    cc.set_env(case, monkeypatch)
    x, w, b, _, _ = kc.int_conv_operands(case.n, case.cin, case.cout, 3, 3, case.h, case.w, seed=3, amax=1, pad=1)
    g = torch.Generator(device="cpu").manual_seed(6)
    fin = (torch.randn(3, case.cout, generator=g) / 64, torch.randn(3, generator=g) * 0.1, 1e-3)
    L = cc.launcher(case, x, w, b, device=dev)
    flags = 8 | (16 if nchw else 0)
    cc.assert_plan(case, L, 4 | flags, 3)
    outs = []
    for _ in range(2):
        out, _, _ = L(flags=flags, final=fin)
        kc.assert_finite(out, cid)
        L.assert_untouched(cid)
        outs.append(out.clone())
    assert torch.equal(outs[0], outs[1])


def test_conv_group_guarded():
    """rf_conv2d_f16_group and rf_conv1x1_f16_group: every member's buffers guarded, launched twice with the planes at
    another column offset."""
    for col_off in (4, 16):
        members = []
        for q, (kind, cin, cout, k, stride, pad, h, w, bias, out_f32) in enumerate(cc.GROUP):
            case = cc.Case(f"group{q}", "f16", kind, cin, cout, k, stride, pad, h, w, 2, {}, None, None, False, "")
            dk = k if kind == "deconv" else 0
            x, wt, b, _, _ = kc.int_conv_operands(2, cin, cout, k, k, h, w, seed=20 + q, stride=stride or 1, pad=pad,
                                                  deconv=dk)
            b = b if bias else None
            L = cc.launcher(case, x, wt, b, device=dev)
            L.alloc(want_out=out_f32, plane_ld=cout + 32, col_off=col_off)
            members.append((L, kc.conv_ref(x, wt, b, None, None, stride or 1, pad, dk)))
        kc.conv_group_launch([m for m, _ in members], [0] * len(members))
        for q, (L, ref) in enumerate(members):
            out, hi, _ = L.views()
            what = f"group member {q} col_off {col_off}"
            assert out is None or torch.equal(L.shaped(out).double(), ref), what
            assert torch.equal(L.shaped(hi), ref.half()), what
            L.assert_untouched(what)
        h, w, n = cc.GROUP_1X1_HW
        for which, spec in cc.GROUP_1X1.items():
            members = []
            for q, (cin, cout, bias) in enumerate(spec):
                case = cc.Case(f"g1x1-{q}", "f16", "conv", cin, cout, 1, 1, 0, h, w, n, {}, None, None, False, "")
                x, wt, b, _, _ = kc.int_conv_operands(n, cin, cout, 1, 1, h, w, seed=30 + q)
                b = b if bias else None
                L = cc.launcher(case, x, wt, b, device=dev)
                L.alloc(want_out=False, plane_ld=cout + 32, col_off=col_off)
                members.append((L, kc.conv_ref(x, wt, b)))
            kc.conv1x1_group_launch([m for m, _ in members])
            for q, (L, ref) in enumerate(members):
                assert torch.equal(L.shaped(L.views()[1]), ref.half()), (which, q, col_off)
                L.assert_untouched(f"1x1 group {which} member {q} col_off {col_off}")
